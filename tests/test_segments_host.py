"""CPU: the segmented MSM of csrc/seg_msm.hpp compiled for the host with the limb-bound checker armed (libmsm_hosttest.so, ht_sm_*):
the signed digits for every window size, a whole call walked serially through the kernels' per-element steps against
pymodel.Curve.msm_naive, the launch plan, and the same host code under AddressSanitizer as a stand-alone program."""
import ctypes
import functools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import pymodel as pm
import segments_cases as sc
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
LENGTHS = (0, 1, 2, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(PKG, "libmsm_hosttest.so"))
    cp, sz, ci, u64 = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64
    p32, p64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
    lib.ht_sm_digits.argtypes = [cp, ci, p32, p32]
    lib.ht_sm_segments.argtypes = [ci, cp, sz, cp, p64, sz, u64, ci, ci, ctypes.c_uint, cp, sz]
    lib.ht_sm_plan.argtypes = [p64, sz, u64, ci, ci, sz, sz, sz, sz, p64, sz, ctypes.POINTER(ctypes.c_uint32), sz, p64, sz, p64]
    lib.ht_sm_plan.restype = ctypes.c_long
    lib.ht_sm_geometry.argtypes = [ci, ci, u64, ci, ctypes.POINTER(ctypes.c_uint32)]
    lib.ht_sm_window_for.argtypes = [u64]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def test_signed_digits_for_every_window_size(ht):
    """sum d_j 2^(c j) == s, |d_j| <= 2^(c-1), ceil(257 / c) digits suffice, for c = 1..9 -- the register form and the memory form of
    the digit alike, and both equal to Booth's rule written out; the alternating scalars reach both extremes"""
    rng = random.Random(0x5E6D)
    scalars = sc.edge_scalars(pm.BLS12_377_G1) + sc.edge_scalars(pm.BLS12_381_G1) + [rng.getrandbits(256) for _ in range(2000)]
    scalars += [(1 << b) - 1 for b in range(1, 257)] + [1 << b for b in range(256)]
    out, mem = (ctypes.c_int32 * 257)(), (ctypes.c_int32 * 257)()
    for c in range(1, 10):
        nd = (257 + c - 1) // c
        for s in scalars:
            assert ht.ht_sm_digits(s.to_bytes(32, "little"), c, out, mem) == nd
            d = list(out[:nd])
            assert d == list(mem[:nd]) == sc.booth_digits(s, c), (c, hex(s))
            assert all(abs(x) <= 1 << (c - 1) for x in d), (c, hex(s))
            assert sum(x << (c * j) for j, x in enumerate(d)) == s, (c, hex(s))
        if c >= 2:
            for s in sc.alternating_extremes(c):
                d = sc.booth_digits(s, c)
                assert (1 << (c - 1)) in d and -(1 << (c - 1)) in d, (c, hex(s))
    assert ht.ht_sm_digits(bytes(32), 0, out, mem) == -1 and ht.ht_sm_digits(bytes(32), 10, out, mem) == -1


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """segments of LENGTHS over one base kind: (images, scalars, offsets, expected Affine images by msm_naive)"""
    curve = pm.CURVES[name]
    lengths = LENGTHS if kind == "planted" else (2, 65, 0, 3)
    offsets = sc.offsets_of(lengths)
    n = offsets[-1]
    _, pts, imgs = sc.base_set(name, kind, n)
    edges = sc.edge_scalars(curve)
    scalars = (edges + sc.random_scalars(n, 0x40 + curve.curve_id))[:n]
    want = sc.images(curve, sc.expected_naive(curve, pts, scalars, offsets))
    return imgs, scalars, offsets, want


def _run(ht, curve, imgs, scalars, offsets, c, tile, flags=0, shared_len=0):
    nseg = len(offsets) - 1 if offsets is not None else len(scalars) // shared_len
    size = curve.projective_bytes if flags & 8 else curve.affine_stride
    out = ctypes.create_string_buffer(b"\xa5" * (size * nseg), size * nseg)
    offs = None if offsets is None else (ctypes.c_uint64 * len(offsets))(*offsets)
    assert ht.ht_sm_segments(curve.curve_id, imgs, curve.affine_stride, sc.scalar_bytes(scalars), offs, nseg, shared_len, c, tile, flags, out, size) == 0
    return out.raw


@pytest.mark.parametrize("name", sc.CURVE_NAMES)
@pytest.mark.parametrize("kind", ("planted", "same", "pairs"))
def test_serial_walk_against_msm_naive(ht, name, kind):
    """every window size, both tiles (129 > 2 * 64: three tiles, the last of one point), byte for byte"""
    curve = pm.CURVES[name]
    imgs, scalars, offsets, want = _case(name, kind)
    before = ht.ht_check_failures()
    for c in range(1, 10):
        for tile in (64, 128):
            assert _run(ht, curve, imgs, scalars, offsets, c, tile) == want, (name, kind, c, tile)
    assert _run(ht, curve, imgs, scalars, offsets, 0, 1024) == want
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


def test_serial_walk_projective_montgomery_and_shared(ht):
    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    imgs, scalars, offsets, _ = _case(name, "planted")
    _, pts, _ = sc.base_set(name, "planted", offsets[-1])
    want = sc.expected_naive(curve, pts, scalars, offsets)
    assert _run(ht, curve, imgs, scalars, offsets, 5, 64, flags=8) == sc.images(curve, want, projective=True)
    mont = [(s << 256) % curve.r for s in scalars]   # the Fr image of s mod r; the engine converts any 256-bit image
    small = [s % curve.r for s in scalars]
    assert _run(ht, curve, imgs, mont, offsets, 4, 64, flags=1) == _run(ht, curve, imgs, small, offsets, 4, 64)
    # shared: 3 segments over the first 65 bases
    L, S = 65, 3
    sh = sc.random_scalars(S * L, 0x5A)
    # (the buffer handed over holds more than L bases, so an index that runs on behind the first L reads a wrong base, not wild memory)
    got = _run(ht, curve, imgs, sh, None, 6, 64, flags=4, shared_len=L)
    tiled = imgs[:L * curve.affine_stride] * S
    assert got == _run(ht, curve, tiled, sh, sc.offsets_of([L] * S), 4, 128)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def _plan(ht, lengths, force_c=0, tile=0, max_segs=0, limit=2 << 30, xyzz=224, el=56, shared=None):
    nseg = len(lengths) if shared is None else shared[0]
    offs = None
    if shared is None:
        o = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)
        offs = o.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    classes = (ctypes.c_uint64 * (11 * 9 * (nseg + 1)))()
    ids = (ctypes.c_uint32 * (nseg + 1))()
    bounds = (ctypes.c_uint64 * (3 * (nseg + 1)))()
    summary = (ctypes.c_uint64 * 3)()
    nc = ht.ht_sm_plan(offs, nseg, 0 if shared is None else shared[1], force_c, tile, max_segs, limit, xyzz, el, classes, 9 * (nseg + 1), ids, nseg + 1,
                       bounds, nseg + 1, summary)
    if nc < 0:
        return nc, None, None, None, None
    rows = np.frombuffer(classes, dtype=np.uint64)[:11 * nc].reshape(nc, 11).astype(np.int64)
    return nc, rows, np.frombuffer(ids, dtype=np.uint32), np.frombuffer(bounds, dtype=np.uint64)[:3 * summary[0]].reshape(-1, 3).astype(np.int64), list(summary)


def _check_plan(ht, lengths, xyzz=224, el=56, **kw):
    lengths = np.asarray(lengths, dtype=np.int64)
    limit = kw.get("limit", 2 << 30)
    nc, rows, ids, bounds, summary = _plan(ht, lengths, xyzz=xyzz, el=el, **kw)
    assert nc >= 0
    nseg = len(lengths)
    # the chunks tile [0, nseg) in order, each within the limit and the segment cap it was given
    if nseg:
        assert bounds[0, 0] == 0 and bounds[-1, 1] == nseg and (bounds[1:, 0] == bounds[:-1, 1]).all() and (bounds[:, 1] > bounds[:, 0]).all()
    assert (bounds[:, 2] <= limit).all()
    if kw.get("max_segs"):
        assert (bounds[:, 1] - bounds[:, 0] <= kw["max_segs"]).all()
    seen = np.zeros(nseg, dtype=np.int64)
    geo = (ctypes.c_uint32 * 4)()
    for chunk, s0, s1, c, nwin, tile, n, ids_at, wsum_at, work, wsum_records in rows:
        assert 1 <= c <= 9 and nwin == (257 + c - 1) // c and n >= 1
        mine = ids[ids_at:ids_at + n].astype(np.int64)
        assert len(mine) == n and (mine >= 0).all() and (mine < s1 - s0).all() and len(set(mine.tolist())) == n
        seg = mine + s0
        seen[seg] += 1
        assert (lengths[seg] > 0).all()
        if not kw.get("force_c"):
            assert all(ht.ht_sm_window_for(int(x)) == c for x in lengths[seg][:64])
        else:
            assert c == kw["force_c"]
        # every (segment, window) of the class has a record of its own inside the chunk's buffer
        assert wsum_at + nwin * n <= wsum_records
        assert work >= wsum_records * xyzz + (s1 - s0) * (xyzz + el + 4)
        assert tile >= 64 and tile & (tile - 1) == 0 and tile <= max(kw.get("tile") or 1024, 64)
        assert ht.ht_sm_geometry(int(c), int(kw.get("tile") or 0), int(lengths[seg].max()), xyzz // 4, geo) == 0
        slices, threads, lds_words, t2 = list(geo)
        assert t2 == tile and threads == max(64, 1 << (c - 1)) and slices * (1 << (c - 1)) <= threads
        assert 4 + slices * (tile + tile // 2 + 2 * (1 << (c - 1))) <= lds_words and 4 + threads * (xyzz // 4) <= lds_words and 4 * lds_words <= 152 << 10
    # the record ranges of a chunk's classes do not overlap
    for k in set(rows[:, 0].tolist()) if len(rows) else ():
        spans = sorted((r[8], r[8] + r[4] * r[6]) for r in rows if r[0] == k)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert (seen == (lengths > 0)).all()
    return rows, bounds, summary


def test_launch_plan(ht):
    rng = np.random.default_rng(0x91A)
    _check_plan(ht, [])
    _check_plan(ht, [0] * 37)
    _check_plan(ht, [5])
    for trial in range(12):
        n = int(rng.integers(1, 400))
        lengths = rng.integers(0, [3, 70, 300, 5000][trial % 4], size=n)
        _check_plan(ht, lengths)
        _check_plan(ht, lengths, xyzz=448, el=112, max_segs=int(rng.integers(1, 50)))
        _check_plan(ht, lengths, force_c=int(rng.integers(1, 10)), tile=int(1 << rng.integers(6, 13)))
        # a limit that forces several chunks: room for about five segments at the widest record count
        _check_plan(ht, lengths, limit=5 * (65 * 224 + 224 + 56 + 4))
    huge = [3] * 40 + [(1 << 31) + 7] + [1] * 40
    rows, bounds, _ = _check_plan(ht, huge)
    assert 9 in rows[:, 3]
    rows, bounds, summary = _check_plan(ht, [64] * (1 << 16))
    assert len(rows) == 1 and rows[0][3] == 4 and summary[0] == 1
    rows, bounds, summary = _check_plan(ht, [64] * (1 << 16), limit=64 << 20)
    assert summary[0] > 1
    # a limit no single segment fits
    assert _plan(ht, [100], limit=1000)[0] == -2
    # the shared form: one class, every segment in order
    nc, rows, ids, bounds, summary = _plan(ht, None, shared=(33, 100))
    assert nc == 1 and rows[0][6] == 33 and list(ids[:33]) == list(range(33))


def test_window_table_follows_the_count(ht):
    """the crossings of cost(c) = ceil(257 / c) (len + 2^c (c - 1)), and sm_window_for at and just past each of its thresholds: every
    threshold is its crossing rounded to a multiple of 256, within 10 % of it"""
    cost = lambda c, n: ((257 + c - 1) // c) * (n + (1 << c) * (c - 1))
    cross = []
    for c in range(4, 9):
        n = 1
        while cost(c, n) <= cost(c + 1, n):
            n += 1
        cross.append(n - 1)
    assert cross == [272, 789, 2442, 7680, 14912]
    table = [256, 768, 2560, 8192, 16384]
    for c, (edge, x) in enumerate(zip(table, cross), start=4):
        assert ht.ht_sm_window_for(edge) == c and ht.ht_sm_window_for(edge + 1) == c + 1, (c, edge)
        assert edge % 256 == 0 and abs(edge - x) <= 0.1 * x, (edge, x)
    assert ht.ht_sm_window_for(1) == 4 and ht.ht_sm_window_for(1 << 40) == 9
    assert [ht.ht_sm_window_for(n) for n in (16, 64, 1024, 4096)] == [4, 4, 6, 7]


def test_host_code_under_address_sanitizer(tmp_path):
    """tests/asan_segments.cpp: the plan and the serial walk on adversarial offsets, as a stand-alone program built with
    -fsanitize=address,undefined and run as a child process"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_segments")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "asan_segments.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
