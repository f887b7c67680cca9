"""formats.py with compressed=True: the sizes and the argument errors without a GPU, the round trip through the GPU codec with one."""
import os
import struct

import pytest

import codec_cases as kc
import pymodel as pm
from conftest import ROOT


def test_record_bytes(ea):
    f = ea.formats
    for name in kc.CURVE_NAMES:
        cb = pm.CURVES[name].coord_bytes
        assert f.record_bytes(name) == 2 * cb and f.record_bytes(name, compressed=False) == 2 * cb
        assert f.record_bytes(name, compressed=True) == cb
    assert f.record_bytes("bls12_377_g1", compressed=True) == 48 and f.record_bytes("bls12_381_g2", compressed=True) == 96


def test_size_and_argument_errors(ea, tmp_path):
    f = ea.formats
    p = str(tmp_path / "points.bin")
    open(p, "wb").write(b"\x01\x02")
    with pytest.raises(ValueError, match="no element count"):
        f.read_points_bin(p, "bls12_377_g1", compressed=True)
    open(p, "wb").write(struct.pack("<Q", 3) + bytes(2 * 48))
    with pytest.raises(ValueError, match="expected 3 compressed records of 48 bytes"):
        f.read_points_bin(p, "bls12_377_g1", compressed=True)
    open(p, "wb").write(struct.pack("<Q", 1) + bytes(48))
    with pytest.raises(ValueError, match="expected 1 compressed records of 96 bytes"):
        f.read_points_bin(p, "bls12_377_g2", compressed=True)
    with pytest.raises(ValueError, match="not a multiple"):
        f.write_points_bin(p, bytes(95), "bls12_377_g1", compressed=True)
    with pytest.raises(ValueError, match="wrong projective image size"):
        f.point_to_serialized(bytes(143), "bls12_377_g1", compressed=True)
    with pytest.raises(ValueError):
        f.record_bytes("no_such_curve", compressed=True)
    # the defaults keep every existing call's bytes
    unc = bytes(range(96))
    f.write_points_bin(p, unc, "bls12_377_g1")
    assert open(p, "rb").read() == struct.pack("<Q", 1) + unc and f.read_points_bin(p, "bls12_377_g1") == (unc, 1)


def test_python_mirror_argument_checks(ea):
    """Raised before the library touches a device."""
    assert {"decompress_points", "compress_points", "set_bases_compressed"} <= set(dir(ea.MultiScalarMultContext))
    assert callable(ea.decompress_points) and callable(ea.compress_points) and ea.CodecResult
    lib = ea.load_library()
    for sym in ("mi355_msm_decompress_points", "mi355_msm_decompress_points_device", "mi355_msm_compress_points",
                "mi355_msm_compress_points_device", "mi355_msm_set_bases_compressed", "mi355_msm_point_to_compressed"):
        assert hasattr(lib, sym)


def test_point_to_compressed_is_host_arithmetic(ea):
    """mi355_msm_point_to_compressed needs no GPU: generator, its negative, a non-normalised Z, infinity -- against the model."""
    f = ea.formats
    for name in kc.CURVE_NAMES:
        curve = pm.CURVES[name]
        G = curve.generator()
        for P in (G, curve.neg(G), curve.mul(5, G)):
            want = kc.compress(curve, (kc.comps(curve, P[0]), kc.comps(curve, P[1])))
            assert f.point_to_serialized(curve.encode_projective_normalized(P), name, compressed=True) == want
            assert f.point_to_serialized(curve.encode_projective_normalized(P), name) == kc.uncompressed(curve, 0, (kc.comps(curve, P[0]), kc.comps(curve, P[1])))
        inf = f.point_to_serialized(curve.encode_projective_normalized(None), name, compressed=True)
        assert inf == kc.compress(curve, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_round_trip_through_the_gpu(ea, tmp_path, name):
    f = ea.formats
    curve = pm.CURVES[name]
    recs, statuses, labels, sub = kc.corpus(name)
    good = [r for r, s, g in zip(recs, statuses, sub) if s == 0 and g]
    unc = kc.expected(curve, b"".join(good), True)[1]
    p = str(tmp_path / "points.bin")
    f.write_points_bin(p, unc, name, compressed=True)
    raw = open(p, "rb").read()
    assert raw[:8] == struct.pack("<Q", len(good)) and len(raw) == 8 + len(good) * curve.coord_bytes
    # (infinity over garbage compresses to the clean infinity record)
    assert raw[8:] == b"".join(r if not (r[-1] & 0x40) else kc.compress(curve, None) for r in good)
    assert f.read_points_bin(p, name, compressed=True) == (unc, len(good))
    assert f.read_points_bin(p, name, compressed=True, validate=True) == (unc, len(good))
    # an off-subgroup record passes the unchecked reader and fails the checked one; a record that does not decode fails both
    off = next(r for r, s, g in zip(recs, statuses, sub) if s == 0 and not g)
    open(p, "wb").write(struct.pack("<Q", 3) + good[0] + off + good[1])
    assert f.read_points_bin(p, name, compressed=True)[1] == 3
    with pytest.raises(ValueError, match="record 1 .*status 3"):
        f.read_points_bin(p, name, compressed=True, validate=True)
    bad = recs[list(statuses).index(2)]
    open(p, "wb").write(struct.pack("<Q", 3) + good[0] + good[1] + bad)
    with pytest.raises(ValueError, match="record 2 .*status 2"):
        f.read_points_bin(p, name, compressed=True)
    with pytest.raises(ValueError, match="record 0 "):
        f.write_points_bin(p, (curve.p).to_bytes(48, "little") * (2 * curve.ext), name, compressed=True)
