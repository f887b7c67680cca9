"""GPU: mi355_msm_check_bases / _device (k_check_points) against the Python model on the corpus of tests/check_cases.py, against the
host build of the same templates, at scale, and behind the option "validate_bases"."""
import ctypes
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import check_cases as cc
import pymodel as pm
from conftest import ROOT, oracle_msm

pytestmark = pytest.mark.gpu

FORMS = [(False, False), (False, True), (True, False), (True, True)]   # (serialized, exact)


def _torch():
    import torch

    return torch


def _records(curve, cases, serialized):
    return cc.encode_all(curve, cases, serialized)


def _flags(cases):
    return [c[0] for c in cases]


def _expect(res, statuses, flags):
    n = len(statuses)
    s = cc.summary(statuses, flags)
    assert list(res.status) == list(statuses)
    assert [res.counts[k] for k in ("valid", "flagged_infinity", "not_canonical", "off_curve", "off_subgroup")] == s[:5]
    assert res.first_invalid == (None if s[5] == n else s[5])
    assert res.ok == (s[5] == n)
    assert sum(s[i] for i in (0, 2, 3, 4)) == n


@pytest.mark.parametrize("serialized,exact", FORMS, ids=["mem-endo", "mem-exact", "ser-endo", "ser-exact"])
@pytest.mark.parametrize("name", cc.CURVE_NAMES)
def test_corpus_through_the_abi(ea, name, serialized, exact):
    torch = _torch()
    curve = pm.CURVES[name]
    cases, statuses, _ = cc.corpus(name)
    rec = _records(curve, cases, serialized)
    ctx = ea.MultiScalarMultContext(name)
    try:
        host = ctx.check_bases(rec, serialized=serialized, exact=exact)
        _expect(host, statuses, _flags(cases))
        assert host.method == ("exact" if exact else "endomorphism")
        dev = ctx.check_bases(torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda(), serialized=serialized, exact=exact)
        _expect(dev, statuses, _flags(cases))
        # status = NULL, and n = 0
        out = (ctypes.c_uint64 * 8)()
        stride = len(rec) // len(cases)
        e = ctx._lib.mi355_msm_check_bases(ctx.context, rec, len(cases), stride, (1 if serialized else 0) | (2 if exact else 0), None, out)
        assert e.code == 0 and list(out)[:6] == cc.summary(statuses, _flags(cases))
        empty = ctx.check_bases(b"", serialized=serialized, exact=exact)
        assert empty.ok and empty.first_invalid is None and not any(empty.counts.values()) and len(empty.status) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("name", cc.CURVE_NAMES)
def test_placement_and_device_equals_host_build(ea, name, n):
    """Bad points at index 0, 63, 64, 255, 256 and n - 1; the engine's bytes equal those of libmsm_hosttest.so on the same records."""
    curve = pm.CURVES[name]
    cases, statuses = cc.placed(name, n, seed=3)
    ht = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    ht.ht_check_points.argtypes = [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p]
    ctx = ea.MultiScalarMultContext(name)
    try:
        for serialized, exact in FORMS:
            rec = _records(curve, cases, serialized)
            res = ctx.check_bases(rec, serialized=serialized, exact=exact)
            _expect(res, statuses, _flags(cases))
            out = ctypes.create_string_buffer(n)
            assert ht.ht_check_points(curve.curve_id, int(serialized), int(not exact), rec, len(rec) // n, n, out) == 0
            assert bytes(res.status) == out.raw[:n]
    finally:
        ctx.close()


@pytest.mark.parametrize("name,logn", [("bls12_377_g1", 22), ("bls12_381_g1", 22), ("bls12_377_g2", 20), ("bls12_381_g2", 20)])
def test_scale_with_planted_points(ea, name, logn):
    torch = _torch()
    curve = pm.CURVES[name]
    n = 1 << logn
    stride = curve.affine_stride
    bases = np.array(ea.generate_points(n, distinct=1 << 12, seed=77, curve=name), copy=True).reshape(n, stride)
    bs = cc.by_status(name)
    rng = random.Random(logn * 7 + curve.curve_id)
    pos = [0, n - 1] + rng.sample(range(1, n - 1), 62)
    exp = np.zeros(n, dtype=np.uint8)
    for k, at in enumerate(pos):
        s = 1 + k % 3
        bases[at] = np.frombuffer(cc.encode(curve, bs[s][(k // 3) % len(bs[s])], False), dtype=np.uint8)
        exp[at] = s
    d = torch.from_numpy(bases.reshape(-1)).cuda()
    ctx = ea.MultiScalarMultContext(name)
    try:
        endo = ctx.check_bases(d)
        exact = ctx.check_bases(d, exact=True)
        host = ctx.check_bases(bases.reshape(-1))          # staged from host memory in pieces
    finally:
        ctx.close()
    print(f"{name} n=2^{logn}: endomorphism {endo.device_us} us, exact {exact.device_us} us")
    assert np.array_equal(endo.status, exp) and np.array_equal(exact.status, exp) and np.array_equal(host.status, exp)
    for r in (endo, exact, host):
        c = r.counts
        assert c["valid"] + c["not_canonical"] + c["off_curve"] + c["off_subgroup"] == n and c["valid"] == n - 64
        assert r.first_invalid == 0


def test_clean_2_26_g1(ea):
    torch = _torch()
    name, n = "bls12_377_g1", 1 << 26
    d = torch.from_numpy(np.asarray(ea.generate_points(n, distinct=1 << 12, seed=5, curve=name)).reshape(-1)).cuda()
    ctx = ea.MultiScalarMultContext(name)
    try:
        res = ctx.check_bases(d)
    finally:
        ctx.close()
    print(f"2^26 clean: {res.device_us} us ({res.method})")
    assert res.ok and res.counts["valid"] == n and res.first_invalid is None and not res.status.any()


@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g2"])
def test_validate_bases_option(ea, oracle, name):
    curve = pm.CURVES[name]
    rng = random.Random(11)
    n = 300
    good = pm.random_points(curve, n, rng, distinct=40)
    ks = pm.random_scalars(curve, n, rng)
    bases, scalars = curve.encode_affine_array(good), pm.encode_scalars(ks)
    exp = ctypes.create_string_buffer(curve.projective_bytes)
    assert oracle.oracle_msm(curve.curve_id, bases, curve.affine_stride, scalars, n, exp, 0) == 0
    bad_at = 123
    bad = bytearray(bases)
    st = curve.affine_stride
    bad[bad_at * st:(bad_at + 1) * st] = cc.encode(curve, cc.by_status(name)[3][0], False)
    ctx = ea.MultiScalarMultContext(name)
    try:
        assert ctx.query("bases_validated") == 0
        ctx.set_option("validate_bases", 1)
        ctx.set_bases(bases)
        assert ctx.query("bases_validated") == 1 and ctx.query("validate_bases") == 1
        first = ctx.run(scalars)[0]
        assert first == exp.raw
        for form in ("host", "device"):
            arg = bytes(bad) if form == "host" else _torch().frombuffer(bytearray(bad), dtype=_torch().uint8).cuda()
            with pytest.raises(ea.MsmError) as ei:
                ctx.set_bases(arg)
            assert ei.value.code == -1 and "point 123 " in ei.value.message and "status 3" in ei.value.message
            assert ctx.query("bases_validated") == 1
            assert ctx.run(scalars)[0] == first          # the previous bases, byte for byte
        ctx.set_option("validate_bases", 0)
        ctx.set_bases(bytes(bad))                         # uploads as it always did
        assert ctx.query("bases_validated") == 0
        ctx.run(scalars)
    finally:
        ctx.close()


def test_validate_bases_serialized(ea):
    name = "bls12_377_g1"
    curve = pm.CURVES[name]
    cases, statuses = cc.placed(name, 100, seed=1)
    good = [c for c, s in zip(cases, statuses) if s == 0]
    ctx = ea.MultiScalarMultContext(name)
    try:
        ctx.set_option("validate_bases", 1)
        ea.formats.set_bases_serialized(ctx, cc.encode_all(curve, good, True))
        assert ctx.query("bases_validated") == 1
        with pytest.raises(ea.MsmError) as ei:
            ea.formats.set_bases_serialized(ctx, cc.encode_all(curve, cases, True))
        assert "point 0 " in ei.value.message and ctx.query("bases_validated") == 1
    finally:
        ctx.close()


def test_assume_subgroup_tie_in(ea):
    """The seven order-2r points of tests/test_gpu_fold.py::test_default_stays_exact_outside_the_subgroup: status 3, and refused."""
    curve = pm.BLS12_377_G1
    T = (curve.p - 1, 0)
    G = curve.generator()
    bases = curve.encode_affine_array([curve.add(curve.mul(3 + i, G), T) for i in range(7)])
    ctx = ea.MultiScalarMultContext(curve.name)
    try:
        for exact in (False, True):
            res = ctx.check_bases(bases, exact=exact)
            assert list(res.status) == [3] * 7 and res.first_invalid == 0
        ctx.set_option("assume_subgroup", 1)
        ctx.set_option("validate_bases", 1)
        with pytest.raises(ea.MsmError):
            ctx.set_bases(bases)
    finally:
        ctx.close()


@pytest.mark.parametrize("d", sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "harness", "*"))), ids=os.path.basename)
def test_checked_reader_on_the_harness_files(ea, d, tmp_path):
    name = "bls12_377_g1" if os.path.basename(d).startswith("377") else "bls12_381_g1"
    curve = pm.CURVES[name]
    path = os.path.join(d, "points.bin")
    records, n = ea.formats.read_points_bin(path, name)
    rb = len(records) // n
    model = []
    for i in range(n):
        r = records[i * rb:(i + 1) * rb]
        flag = (r[-1] >> 6) & 1
        x = int.from_bytes(r[:48], "little")
        y = int.from_bytes(r[48:], "little") & ((1 << 382) - 1)
        lift = (int(x >= curve.p),), (int(y >= curve.p),)
        model.append(cc.model_status(curve, (flag, (x % curve.p,), (y % curve.p,), lift[0], lift[1])))
    first = next((i for i, s in enumerate(model) if s), None)
    if first is None:
        assert ea.formats.read_points_bin(path, name, validate=True) == (records, n)
        assert ea.formats.load_harness_dir(d, name, validate=True).n == n
    else:
        with pytest.raises(ValueError, match=f"record {first} "):
            ea.formats.read_points_bin(path, name, validate=True)
    # one record's y incremented: off the curve
    at = next(i for i, s in enumerate(model) if s == 0 and not ((records[(i + 1) * rb - 1] >> 6) & 1))
    if first is not None and first < at:
        return
    bad = bytearray(records)
    y = int.from_bytes(bad[at * rb + 48:(at + 1) * rb], "little") + 1
    bad[at * rb + 48:(at + 1) * rb] = y.to_bytes(48, "little")
    p2 = str(tmp_path / "points.bin")
    ea.formats.write_points_bin(p2, bytes(bad), name)
    with pytest.raises(ValueError, match=f"record {at} "):
        ea.formats.read_points_bin(p2, name, validate=True)
    assert ea.formats.read_points_bin(p2, name) == (bytes(bad), n)     # the unchecked reader is as it was


def test_errors(ea):
    name = "bls12_377_g1"
    curve = pm.CURVES[name]
    rec = curve.encode_affine_array([curve.generator()] * 4)
    ctx = ea.MultiScalarMultContext(name)
    out = (ctypes.c_uint64 * 8)()
    try:
        for stride in (96, 98, 102):
            e = ctx._lib.mi355_msm_check_bases(ctx.context, rec, 1, stride, 0, None, out)
            assert e.code == -1 and b"stride" in ctypes.string_at(e.message)
        e = ctx._lib.mi355_msm_check_bases(ctx.context, rec, 4, 104, 8, None, out)
        assert e.code == -1
    finally:
        ctx.close()
    sh = ea.MultiScalarMultContext(name, devices=[0, 0])
    try:
        with pytest.raises(ea.MsmError) as ei:
            sh.check_bases(rec)
        assert ei.value.code == -1 and "sharded" in ei.value.message
        # the option is refused where it is set, with a message that names it; turning it off is accepted, and bases upload as before
        with pytest.raises(ea.MsmError) as ei:
            sh.set_option("validate_bases", 1)
        assert ei.value.code == -1 and "validate_bases" in ei.value.message and "sharded" in ei.value.message
        sh.set_option("validate_bases", 0)
        sh.set_bases(rec)
        assert sh.query("bases_validated") == 0
    finally:
        sh.close()


def test_environment_switch_is_refused_for_a_sharded_context(ea, monkeypatch):
    monkeypatch.setenv("MI355_MSM_DEVICES", "0,0")
    monkeypatch.setenv("MI355_MSM_VALIDATE_BASES", "1")
    with pytest.raises(ea.MsmError) as ei:
        ea.MultiScalarMultContext.from_env("bls12_377_g1")
    assert ei.value.code == -1 and "validate_bases" in ei.value.message and "MI355_MSM_VALIDATE_BASES" in ei.value.message
    monkeypatch.setenv("MI355_MSM_VALIDATE_BASES", "0")
    ctx = ea.MultiScalarMultContext.from_env("bls12_377_g1")
    assert ctx.query("shards") == 2
    ctx.close()


def test_serialized_record_with_both_flag_bits_counts_as_infinity(ea):
    """Documented difference from arkworks' reader (csrc/check_points.hpp): only bit 6 is read."""
    curve = pm.BLS12_377_G1
    rec = bytearray(cc.encode(curve, (1, (5,), (7,), (0,), (0,)), True))
    rec[-1] |= 0x80
    res = ea.check_points(bytes(rec), curve=curve.name, serialized=True)
    assert res.ok and res.counts["flagged_infinity"] == 1


@pytest.mark.skipif("__import__('torch').cuda.device_count() < 2", reason="needs two GPUs")
def test_wrong_device_is_refused(ea):
    torch = _torch()
    curve = pm.BLS12_377_G1
    rec = curve.encode_affine_array([curve.generator()] * 4)
    ctx = ea.MultiScalarMultContext(curve.name, device=0)
    try:
        with pytest.raises(ea.MsmError, match="cuda:1"):
            ctx.check_bases(torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda:1"))
    finally:
        ctx.close()


def test_environment_switch_in_a_fresh_process(ea):
    code = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import entries_amd as ea, pymodel as pm, check_cases as cc
curve = pm.BLS12_377_G1
ctx = ea.MultiScalarMultContext.from_env(curve.name)
assert ctx.query("validate_bases") == 1
good = curve.encode_affine_array([curve.mul(k, curve.generator()) for k in (1, 2, 3)])
ctx.set_bases(good)
assert ctx.query("bases_validated") == 1
bad = good + cc.encode(curve, (0, (curve.p - 1,), (0,), (0,), (0,)), False)
try:
    ctx.set_bases(bad)
except ea.MsmError as e:
    assert "point 3 " in e.message, e.message
    print("REFUSED")
ctx.close()
""" % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    env = dict(os.environ, MI355_MSM_VALIDATE_BASES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED" in r.stdout, r.stdout + r.stderr
