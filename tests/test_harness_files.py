"""CPU: the committed TEST_LOAD_DATA_FROM data sets (tests/golden/harness/, written by tools/gen_golden.py) restate the ZPrize
FPGA harness's semantics (P1B hardcaml/zprize/msm_pippenger/test_fpga_harness/src/util.rs:72-140, tests/msm.rs:17-40):
scalars.bin holds normal-form integers a_i, and arkworks_results.bin[b] = sum_i (a_i * 2^256 mod r) P_i over batch b.
Also: the loader's checks, and the R2 constants behind the device conversion (csrc/field_consts.inc)."""
import os
import re
import struct

import pytest

import pymodel as m
from conftest import ROOT, oracle_msm

HDIR = os.path.join(ROOT, "tests", "golden", "harness")
SETS = {"377_g1_random": m.BLS12_377_G1, "377_g1_trivial": m.BLS12_377_G1, "381_g1_random": m.BLS12_381_G1}


def load(ea, name):
    return ea.formats.load_harness_dir(os.path.join(HDIR, name), SETS[name].name)


def decode_record(curve, rec):
    """One uncompressed G1 CanonicalSerialize record -> affine point (None for the infinity flag)."""
    cb = curve.coord_bytes
    if rec[-1] & 0x40:
        return None
    return int.from_bytes(rec[:cb], "little"), int.from_bytes(rec[cb:2 * cb - 1] + bytes([rec[-1] & 0x3F]), "little")


def oracle_results(oracle, curve, data, images):
    """Serialized oracle MSM per batch of data's bases, with the scalars mapped through `images`."""
    rb = 2 * curve.coord_bytes
    pts = [decode_record(curve, data.records[i * rb:(i + 1) * rb]) for i in range(data.n)]
    bases = curve.encode_affine_array(pts)
    sc = m.decode_scalars(data.scalars)
    out = []
    for b in range(data.batches):
        img = [images(a) for a in sc[b * data.n:(b + 1) * data.n]]
        got = oracle_msm(oracle, curve.curve_id, bases, m.encode_scalars(img), data.n)
        out.append(curve.encode_serialized(curve.decode_projective(got)))
    return out


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_layout(ea, name):
    curve = SETS[name]
    d = os.path.join(HDIR, name)
    data = load(ea, name)
    assert data.batches == 4 and data.n in (1 << 8, 1 << 10)
    for fn, count, size in (("points.bin", data.n, 2 * curve.coord_bytes), ("scalars.bin", 4 * data.n, 32),
                            ("arkworks_results.bin", 4, 2 * curve.coord_bytes)):
        raw = open(os.path.join(d, fn), "rb").read()
        assert struct.unpack("<Q", raw[:8])[0] == count and len(raw) == 8 + count * size, fn
        assert len(raw) < 256 * 1024


@pytest.mark.parametrize("name", sorted(SETS))
def test_results_are_the_msm_of_the_montgomery_images(ea, oracle, name):
    curve = SETS[name]
    data = load(ea, name)
    R = (1 << 256) % curve.r
    assert oracle_results(oracle, curve, data, lambda a: a * R % curve.r) == data.expected


def test_trivial_set_gives_the_generator(ea):
    c = m.BLS12_377_G1
    data = load(ea, "377_g1_trivial")
    g = c.encode_serialized(c.generator())
    assert data.records == g * data.n and data.expected == [g] * 4
    rinv = pow((1 << 256) % c.r, -1, c.r)        # Fp256::new(BigInteger256::from(1)): limbs 1, value R^-1
    sc = m.decode_scalars(data.scalars)
    assert sc == [rinv if i % data.n == 0 else 0 for i in range(4 * data.n)]


@pytest.mark.parametrize("name", ["377_g1_random", "381_g1_random"])
def test_plain_integers_give_other_results(ea, oracle, name):
    """Negative control: the file's integers taken as they are (what formats.py claimed before) miss every batch."""
    curve = SETS[name]
    data = load(ea, name)
    plain = oracle_results(oracle, curve, data, lambda a: a)
    assert all(p != e for p, e in zip(plain, data.expected))


@pytest.mark.parametrize("name", ["377_g1_random", "381_g1_random"])
def test_random_sets_hold_the_planted_edges(ea, name):
    curve = SETS[name]
    r = curve.r
    R = (1 << 256) % r
    data = load(ea, name)
    images = [a * R % r for a in m.decode_scalars(data.scalars)]
    for b in (0, 3):
        img = set(images[b * data.n:(b + 1) * data.n])
        assert {0, 1, r - 1, (r + 1) // 2, 1 << 252, R, (r - 1) * R % r} <= img, b
    rb = 2 * curve.coord_bytes
    assert data.records[3 * rb:4 * rb] == curve.encode_serialized(None)


def _write(path, count, payload):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", count) + payload)


def test_loader_rejects_short_files_and_scalars_not_below_r(ea, tmp_path):
    f = ea.formats
    r = m.BLS12_377_G1.r
    _write(tmp_path / "s.bin", 3, m.encode_scalars([1, 2, r - 1]))
    assert f.read_scalars_bin(str(tmp_path / "s.bin"), "bls12_377_g1") == (m.encode_scalars([1, 2, r - 1]), 3)
    for bad in (r, r + 1, (1 << 256) - 1, m.BLS12_381_G1.r):
        _write(tmp_path / "s.bin", 3, m.encode_scalars([1, bad, 2]))
        with pytest.raises(ValueError, match="scalar 1"):
            f.read_scalars_bin(str(tmp_path / "s.bin"), "bls12_377_g1")
    # no curve: the file could hold either field, so only what is >= r of both (BLS12-381's r is the larger) is rejected
    r381 = m.BLS12_381_G1.r
    _write(tmp_path / "s.bin", 3, m.encode_scalars([r, r381 - 1, 0]))
    assert f.read_scalars_bin(str(tmp_path / "s.bin")) == (m.encode_scalars([r, r381 - 1, 0]), 3)
    for bad in (r381, r381 + 1, (1 << 256) - 1):
        _write(tmp_path / "s.bin", 3, m.encode_scalars([1, bad, 2]))
        with pytest.raises(ValueError, match="scalar 1"):
            f.read_scalars_bin(str(tmp_path / "s.bin"))
    _write(tmp_path / "s.bin", 3, m.encode_scalars([m.BLS12_377_G1.r]))   # below r of BLS12-381: legal there, short here
    with pytest.raises(ValueError, match="short"):
        f.read_scalars_bin(str(tmp_path / "s.bin"), "bls12_381_g1")
    _write(tmp_path / "s.bin", 1, m.encode_scalars([m.BLS12_377_G1.r]))
    assert f.read_scalars_bin(str(tmp_path / "s.bin"), "bls12_381_g1")[1] == 1
    _write(tmp_path / "p.bin", 2, b"\0" * 150)
    with pytest.raises(ValueError, match="short"):
        f.read_points_bin(str(tmp_path / "p.bin"))
    open(tmp_path / "e.bin", "wb").write(b"\1\0\0")
    for reader in (f.read_points_bin, f.read_scalars_bin):
        with pytest.raises(ValueError):
            reader(str(tmp_path / "e.bin"))
    # a directory whose files do not make whole batches
    d = tmp_path / "set"
    d.mkdir()
    c = m.BLS12_377_G1
    g = c.encode_serialized(c.generator())
    _write(d / "points.bin", 2, g * 2)
    _write(d / "scalars.bin", 5, m.encode_scalars([1] * 5))
    _write(d / "arkworks_results.bin", 2, g * 2)
    with pytest.raises(ValueError, match="whole batches"):
        f.load_harness_dir(str(d))
    _write(d / "scalars.bin", 4, m.encode_scalars([1] * 4))
    _write(d / "arkworks_results.bin", 3, g * 3)
    with pytest.raises(ValueError, match="whole batches"):
        f.load_harness_dir(str(d))


def test_r2_constants():
    """csrc/field_consts.inc: R2 = 2^512 mod r of both scalar fields (the multiplier of fr_to_montgomery)."""
    inc = open(os.path.join(ROOT, "2022-entries_amd", "csrc", "field_consts.inc")).read()
    for name, r in (("Bls12_377_Fr", m.BLS12_377_G1.r), ("Bls12_381_Fr", m.BLS12_381_G1.r)):
        body = re.search(r"struct %s \{\n(.*?)\n\};" % name, inc, re.S).group(1)
        words = re.search(r"R2\[8\] = \{([^}]*)\}", body).group(1)
        limbs = [int(w.strip().rstrip("u"), 16) for w in words.split(",")]
        assert sum(x << (32 * i) for i, x in enumerate(limbs)) == pow(2, 512, r), name
