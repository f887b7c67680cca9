"""GPU: ea.HashToCurve (mi355_msm_h2c_*) on BLS12-381 G1 and G2.  RFC 9380's five vectors of each suite as ONE batch (a wave mixes 0- and
517-byte messages, hence different block counts): hash_to_field gives the recorded u, map_to_curve Q0 and Q1, hash P, byte-equal.
Random batches of n = 1, 63, 64, 65 and 257 messages of 0 .. 200 bytes with the padding-boundary lengths, against the host build of
the same code on all of them and against the big-integer model on 12; DSTs of 1, 255 and 256 bytes; encode; pairs (u, u) and (u, -u)
among ordinary ones; an empty batch; every output of a 257-message batch in the subgroup by ctx.check_bases; GPU tensors in and out,
out=, and a late producer on a side stream (flag bit 1); and a BLS signature in both arrangements, accepted by Pairing.check and
rejected when one message byte is flipped."""
import random
from contextlib import closing

import numpy as np
import pytest

import h2c_cases as hc
import stream_cases as st

pytestmark = pytest.mark.gpu

GROUPS = ("g1", "g2")
DST = b"QUUX-V01-CS02-with-BLS12381-test-suite-of-this-library"


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def engines(ea):
    made = {g: ea.HashToCurve(hc.CURVES[g], dst=DST) for g in GROUPS}
    yield made
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def reference(built):
    """per group: 257 random messages (the first ones at the padding-boundary lengths of this DST) and, from the HOST build of
    h2c.hpp with the checker armed, their field images (count 2), hash and encode images -- computed once"""
    ht = hc.hosttest()
    ht.ht_reset_checks()
    out = {}
    for g in GROUPS:
        msgs = hc.random_messages(257, "gpu h2c " + g, hc.boundary_lengths(len(DST)) + [0, 200, 1])
        out[g] = (msgs, hc.host_field(g, msgs, DST, 2), hc.host_hash(g, msgs, DST), hc.host_hash(g, msgs[:65], DST, encode=True))
    assert ht.ht_check_failures() == 0
    return out


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "is_cuda") else np.asarray(t).tobytes()


@pytest.mark.parametrize("group", GROUPS)
def test_rfc_vectors_as_one_batch(ea, group):
    d = hc.fixture("BLS12381%s_XMD-SHA-256_SSWU_RO_.json" % group.upper())
    msgs = [v["msg"].encode() for v in d["vectors"]]
    assert sorted(len(m) for m in msgs) == [0, 3, 16, 133, 517]
    s = hc.STRIDE[group]
    with ea.HashToCurve(hc.CURVES[group], dst=d["dst"]) as h:
        u = h.hash_to_field(msgs)
        assert raw_of(u) == hc.u_images([hc.parse_el(group, t) for v in d["vectors"] for t in v["u"]])
        q = h.map_to_curve(u)
        assert raw_of(q) == hc.images(group, [hc.parse_point(group, v[k]) for v in d["vectors"] for k in ("Q0", "Q1")])
        want = hc.images(group, [hc.parse_point(group, v["P"]) for v in d["vectors"]])
        assert raw_of(h.hash(msgs)) == want
        assert raw_of(h.map_to_curve(u, pairs=True)) == want
        assert h.query("last_launches") == 3 and h.query("lanes_in_flight") == 10
        assert u.shape == (10, s // 2 - 4) and q.shape == (10, s)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("group", GROUPS)
def test_random_batches_against_the_host_build(engines, reference, group, n):
    msgs, field, hashed, _ = reference[group]
    h, s, m = engines[group], hc.STRIDE[group], 1 if group == "g1" else 2
    assert raw_of(h.hash_to_field(msgs[:n])) == field[:n * 2 * 48 * m]
    assert raw_of(h.hash(msgs[:n])) == hashed[:n * s]


@pytest.mark.parametrize("group", GROUPS)
def test_twelve_messages_against_the_model(engines, reference, group):
    msgs, _, hashed, _ = reference[group]
    s = hc.STRIDE[group]
    for i in range(12):
        assert hashed[i * s:(i + 1) * s] == hc.affine_image(group, hc.hash_to_curve(group, msgs[i], DST), s), i
    assert raw_of(engines[group].hash(msgs[:12])) == hashed[:12 * s]


@pytest.mark.parametrize("group", GROUPS)
def test_encode_and_projective_images(engines, reference, group):
    msgs, _, hashed, encoded = reference[group]
    h, s = engines[group], hc.STRIDE[group]
    assert raw_of(h.encode(msgs[:65])) == encoded
    assert encoded[:s] == hc.affine_image(group, hc.encode_to_curve(group, msgs[0], DST), s)
    proj = raw_of(h.hash(msgs[:3], projective=True))
    w = (s - 8) // 2
    one = (hc.R384 % hc.P).to_bytes(48, "little") + bytes(w - 48)
    assert proj == b"".join(hashed[i * s:i * s + 2 * w] + one for i in range(3))


@pytest.mark.parametrize("dst_len", [1, 255, 256])
@pytest.mark.parametrize("group", GROUPS)
def test_dst_lengths(ea, group, dst_len):
    dst = bytes((7 * i + dst_len) & 0xff for i in range(dst_len))
    msgs = hc.random_messages(9, "dst %d" % dst_len, hc.boundary_lengths(dst_len))
    with ea.HashToCurve(hc.CURVES[group], dst=dst) as h:
        assert h.query("dst_oversize") == int(dst_len > 255) and h.query("dst_bytes") == min(dst_len, 32 if dst_len > 255 else 255)
        u = raw_of(h.hash_to_field(msgs, count=1))
    assert u == hc.u_images([hc.hash_to_field(group, x, dst, 1)[0] for x in msgs])
    assert u == hc.host_field(group, msgs, dst, 1)


@pytest.mark.parametrize("group", GROUPS)
def test_doubling_and_cancelling_pairs_and_an_empty_batch(engines, group):
    F = hc.suite(group)[0].F
    rng = random.Random("pairs " + group)
    us = [tuple(rng.randrange(hc.P) for _ in range(F.m)) for _ in range(4)]
    seq = [us[0], us[1], us[2], us[2], us[3], F.neg(us[3]), F.zero, us[0]]
    h = engines[group]
    got = hc.points(group, raw_of(h.map_to_curve(hc.u_images(seq), pairs=True)))
    assert got == [hc.map_pair(group, seq[2 * j], seq[2 * j + 1]) for j in range(4)]
    assert got[2] is None and got[1] is not None
    assert raw_of(h.map_to_curve(hc.u_images(seq), pairs=True)) == hc.host_map(group, hc.u_images(seq), 4)
    assert h.hash([]).shape == (0, hc.STRIDE[group]) and h.hash_to_field([]).shape[0] == 0 and h.map_to_curve(b"").shape[0] == 0
    assert h.query("last_launches") == 0


@pytest.mark.parametrize("group", GROUPS)
def test_every_output_is_in_the_subgroup(ea, engines, reference, group):
    msgs = reference[group][0]
    out = engines[group].hash(msgs)
    with closing(ea.MultiScalarMultContext(hc.CURVES[group])) as ctx:
        res = ctx.check_bases(out, exact=True)
        assert res.ok and not np.asarray(res.status).any()
        # the map alone leaves the subgroup: the judgement above is not vacuous
        raw = engines[group].map_to_curve(engines[group].hash_to_field(msgs[:8], count=1))
        assert (np.asarray(ctx.check_bases(raw).status) == 3).all()


@pytest.mark.parametrize("group", GROUPS)
def test_gpu_tensors_in_and_out(engines, reference, torch_, group):
    msgs, field, hashed, _ = reference[group]
    h, s = engines[group], hc.STRIDE[group]
    n = 65
    data, off = hc.pack(msgs[:n])
    td = torch_.frombuffer(bytearray(data), dtype=torch_.uint8).cuda()
    to = torch_.from_numpy(np.frombuffer(off, dtype=np.int64).copy()).cuda()
    got = h.hash((td, to))
    assert got.is_cuda and raw_of(got) == hashed[:n * s]
    out = torch_.zeros((n, s), dtype=torch_.uint8, device="cuda")
    assert h.hash((td, to), out=out) is out and raw_of(out) == hashed[:n * s]
    u = h.hash_to_field((td, to))
    assert u.is_cuda and raw_of(u) == field[:n * 2 * (s // 2 - 4)]
    assert raw_of(h.map_to_curve(u, pairs=True)) == hashed[:n * s]
    # an (n, len) tensor of equal-length messages, and offsets that point outside the buffer: clamped, never read
    same = [bytes([i]) * 32 for i in range(5)]
    t2 = torch_.frombuffer(bytearray(b"".join(same)), dtype=torch_.uint8).cuda().reshape(5, 32)
    assert raw_of(h.hash(t2)) == hc.host_hash(group, same, DST)
    bad = torch_.tensor([0, 64, 1 << 40, 32, 160], dtype=torch_.int64, device="cuda")
    clamped = [b"".join(same)[:64], b"".join(same)[64:160], b"", b"".join(same)[32:160]]
    assert raw_of(h.hash((t2.reshape(-1), bad))) == hc.host_hash(group, clamped, DST)


@pytest.fixture(scope="module")
def side(torch_):
    """(stream, calibrated delay) for the late producer of this module; the stream comes from torch's high-priority pool, for the
    reason tests/test_gpu_poseidon.py gives"""
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


@pytest.mark.parametrize("group", GROUPS)
def test_hash_after_a_late_producer_on_a_side_stream(engines, reference, torch_, side, group):
    """offsets, messages and the out= tensor behind ONE late producer on a side stream, which fills the output with OUT_POISON before it
    hands over the inputs: a result written on any other stream is overwritten afterwards"""
    msgs, _, hashed, _ = reference[group]
    h, s = engines[group], hc.STRIDE[group]
    stream, delay = side
    n = 70
    data, off = hc.pack(msgs[:n])
    out = st.poisoned(torch_, (n, s))
    to, td = st.late_many(torch_, [off, data], stream, delay, fill=[out])
    with torch_.cuda.stream(stream):
        assert st.window_open(to.produced) and st.window_open(out.produced), "invalid: the producer had finished before the call was made"
        got = h.hash((td, to.view(torch_.int64)), out=out)
    stream.synchronize()
    assert st.closed(to, out), "invalid: the producer took %s ms" % st.delay_ms(to)
    assert got is out and raw_of(out) == hashed[:n * s]


def test_a_bls_signature_in_both_arrangements(ea, torch_):
    """e(pk, H(m)) = e(g, sigma) with sigma = sk H(m) from ctx.mul_points, as a product of two pairings per message that Pairing.check
    finds to be one; with one message byte flipped it is not"""
    rng = random.Random("bls")
    msgs = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(8)]
    flipped = list(msgs)
    flipped[5] = bytes([msgs[5][0] ^ 1]) + msgs[5][1:]
    sks = np.frombuffer(b"".join(rng.randrange(1 << 250).to_bytes(32, "little") for _ in range(8)), dtype=np.uint8).reshape(8, 32)
    with ea.Pairing("bls12_381_g1") as pairing:
        for hash_group, key_group in (("g2", "g1"), ("g1", "g2")):
            hcurve, kcurve = hc.CURVES[hash_group], hc.CURVES[key_group]
            gen = ea.generate_points(1, distinct=1, seed=0x424c53, curve=kcurve)
            neg_gen = np.frombuffer(hc.images(key_group, [hc.neg(key_group, hc.points(key_group, gen.tobytes())[0])]), dtype=np.uint8)
            with ea.HashToCurve(hcurve, dst=b"BLS_SIG_TEST_XMD:SHA-256_SSWU_RO_NUL_") as h, closing(ea.MultiScalarMultContext(hcurve)) as hctx, \
                    closing(ea.MultiScalarMultContext(kcurve)) as kctx:
                pk = np.asarray(kctx.mul_points(np.tile(gen, (8, 1)), sks))
                hm = h.hash(msgs)
                sig = np.asarray(hctx.mul_points(hm, sks))
                assert hctx.check_bases(sig).ok
                for hashed, want in ((hm, [True] * 8), (h.hash(flipped), [True] * 5 + [False] + [True] * 2)):
                    # per message the pairs (pk, H(m)) and (-g, sigma), each in (G1, G2) order
                    key_side = np.stack([pk, np.tile(neg_gen, (8, 1))], axis=1).reshape(16, -1)
                    hash_side = np.stack([np.asarray(hashed), sig], axis=1).reshape(16, -1)
                    p, q = (key_side, hash_side) if key_group == "g1" else (hash_side, key_side)
                    assert pairing.check(p, q, group=2).tolist() == want
