"""CPU: the big-integer model of tests/h2c_cases.py reproduces every recorded value of the four fixture files under tests/golden/h2c
(RFC 9380's vectors as the arkworks tests read them): msg_prime is implied by uniform_bytes, then u, Q0, Q1 and P of both groups."""
import pytest

import h2c_cases as hc


@pytest.mark.parametrize("name", ["expand_message_xmd_SHA256_38.json", "expand_message_xmd_SHA256_256.json"])
def test_expand_message_xmd(name):
    d = hc.fixture(name)
    dst = d["DST"].encode()
    assert len(d["tests"]) >= 5
    for t in d["tests"]:
        assert hc.dst_prime(dst).hex() == t["DST_prime"]
        n = int(t["len_in_bytes"], 16)
        assert hc.expand_message_xmd(t["msg"].encode(), dst, n).hex() == t["uniform_bytes"]


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_suite_vectors(group):
    d = hc.fixture("BLS12381%s_XMD-SHA-256_SSWU_RO_.json" % group.upper())
    dst = d["dst"].encode()
    assert [len(v["msg"]) for v in d["vectors"]] == [0, 3, 16, 133, 517]
    for v in d["vectors"]:
        msg = v["msg"].encode()
        u = hc.hash_to_field(group, msg, dst, 2)
        assert u == [hc.parse_el(group, t) for t in v["u"]]
        q0, q1 = hc.map_to_curve(group, u[0]), hc.map_to_curve(group, u[1])
        assert q0 == hc.parse_point(group, v["Q0"]) and q1 == hc.parse_point(group, v["Q1"])
        assert hc.on_curve(group, q0) and hc.on_curve(group, q1)
        assert hc.hash_to_curve(group, msg, dst) == hc.parse_point(group, v["P"])


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_h_eff_of_the_older_golden_file_agrees(group):
    for v in hc.KAT[group]["vectors"][:2]:
        q0, q1 = (tuple(hc.parse_el(group, v[k][c] if isinstance(v[k][c], str) else ",".join(v[k][c])) for c in "xy") for k in ("Q0", "Q1"))
        p = tuple(hc.parse_el(group, v["P"][c] if isinstance(v["P"][c], str) else ",".join(v["P"][c])) for c in "xy")
        assert hc.clear_cofactor(group, hc.add(group, q0, q1)) == p
