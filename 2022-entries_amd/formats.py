"""On-disk input formats of the reference harnesses.

* arkworks ``CanonicalSerialize`` files written by the FPGA harness with ``serialize_unchecked``
  (P1B hardcaml/zprize/msm_pippenger/test_fpga_harness/src/util.rs:126-140): ``points.bin`` (``Vec<G1Affine>``),
  ``scalars.bin`` (``Vec<Fr>``), ``arkworks_results.bin`` (``Vec<G1Affine>``).  A ``Vec`` is a little-endian u64 element
  count followed by the elements; an affine point is ``x | y`` as little-endian NORMAL-form integers with ``SWFlags`` in the
  top two bits of the last byte (bit 6 = infinity; P1B nickray driver/algebra/serialize/src/flags.rs:107-134); an ``Fr`` is
  its 32-byte little-endian NORMAL-form integer ``a`` (``into_repr``; P1B nickray driver/algebra/ff/src/fields/models/fp/mod.rs:583-608).
  That is NOT the integer the harness's MSM runs on: it deserializes the file into ``Fr`` (whose limbs hold the Montgomery
  image ``a * 2^256 mod r``) and hands those limbs over through ``transmute::<&[Fr], &[BigInteger256]>`` (util.rs:72-140,
  tests/msm.rs:17-40), so ``arkworks_results.bin[b] = sum_i (a_i * 2^256 mod r) P_i``.  Run the file's integers with the
  context option ``scalars_to_montgomery`` = 1 (``run_harness_dir``) to get those results.
* whitespace-separated hex text (one big-endian hex number per token; points as x then y) as read by
  ``MSMReadHexPoints`` / ``MSMReadHexScalars`` (CMB MSM.cu:77-128) and ``parseHex`` (prize4 yrrid C/Reader.c:10-54).

Point records are handed to the device as they are (``MultiScalarMultContext.set_bases_serialized``); nothing here does
field arithmetic on the host.
"""
from __future__ import annotations

import ctypes
import struct
from typing import List, NamedTuple, Tuple

import numpy as np

from .msm import MultiScalarMultContext, _check, _curve_id, _COORD_BYTES, load_library, projective_bytes


def record_bytes(curve, compressed: bool = False) -> int:
    """Bytes of one serialized affine point: uncompressed 96 for G1, 192 for G2; ``compressed`` (x and two flag bits) 48 / 96."""
    return (1 if compressed else 2) * _COORD_BYTES[_curve_id(curve)]


def _read_compressed_points_bin(path: str, curve, validate: bool) -> Tuple[bytes, int]:
    rb = record_bytes(curve, compressed=True)
    with open(path, "rb") as f:
        head = f.read(8)
        if len(head) != 8:
            raise ValueError(f"{path}: no element count")
        (n,) = struct.unpack("<Q", head)
        data = f.read(n * rb)
    if len(data) != n * rb:
        raise ValueError(f"{path}: expected {n} compressed records of {rb} bytes, file is short")
    from .msm import CODEC_STATUS_TEXT, decompress_points

    res = decompress_points(data, curve=curve, uncompressed=True, validate=validate)
    if not res.ok:
        i = res.first_invalid
        raise ValueError(f"{path}: record {i} is not a valid point (status {int(res.status[i])}: {CODEC_STATUS_TEXT[int(res.status[i])]}); "
                         f"{n - res.counts['valid']} of {n} records are invalid")
    return res.points, n


def read_points_bin(path: str, curve="bls12_377_g1", validate: bool = False, compressed: bool = False) -> Tuple[bytes, int]:
    """``points.bin`` -> (uncompressed records without the length prefix, count).  ``validate=True`` is arkworks' ``deserialize_uncompressed``
    beside the default ``deserialize_unchecked``: the records go through the GPU check (msm.check_points) and a ValueError names the
    first record that has a non-canonical coordinate, is off the curve or lies outside the order-r subgroup.
    ``compressed=True``: the file holds COMPRESSED records (arkworks' plain ``serialize``); they are decoded on the GPU
    (msm.decompress_points) into the same uncompressed records, a record that does not decode raises ValueError, and with
    ``validate=True`` the subgroup check runs after decoding (``deserialize`` beside ``deserialize_compressed_unchecked``)."""
    if compressed:
        return _read_compressed_points_bin(path, curve, validate)
    rb = record_bytes(curve)
    with open(path, "rb") as f:
        head = f.read(8)
        if len(head) != 8:
            raise ValueError(f"{path}: no element count")
        (n,) = struct.unpack("<Q", head)
        data = f.read(n * rb)
    if len(data) != n * rb:
        raise ValueError(f"{path}: expected {n} records of {rb} bytes, file is short")
    if validate:
        from .msm import CHECK_STATUS_TEXT, check_points

        res = check_points(data, curve=curve, serialized=True)
        if not res.ok:
            i = res.first_invalid
            raise ValueError(f"{path}: record {i} is not a valid point (status {int(res.status[i])}: {CHECK_STATUS_TEXT[int(res.status[i])]}); "
                             f"{n - res.counts['valid']} of {n} records are invalid")
    return data, n


def write_points_bin(path: str, records: bytes, curve="bls12_377_g1", compressed: bool = False) -> None:
    """Uncompressed records -> ``Vec<Affine>`` file.  ``compressed=True`` writes the COMPRESSED form of the same points (encoded on
    the GPU, msm.compress_points); a record with a non-canonical coordinate raises ValueError."""
    rb = record_bytes(curve)
    if len(records) % rb:
        raise ValueError("records length is not a multiple of the record size")
    n = len(records) // rb
    if compressed:
        from .msm import compress_points

        res = compress_points(records, curve=curve, serialized=True)
        if not res.ok:
            raise ValueError(f"record {res.first_invalid} has a coordinate that is not below p")
        records = res.points
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", n))
        f.write(records)


# the scalar field order r of each curve id (BLS12-377 Fr: ARKC bls12_377/src/fields/fr.rs:24; BLS12-381 Fr: bls12_381/src/fields/fr.rs:4)
_FR_377 = 8444461749428370424248824938781546531375899335154063827935233455917409239041
_FR_381 = 52435875175126190479447740508185965837690552500527637822603658699938581184513
SCALAR_FIELD_ORDER = {0: _FR_377, 1: _FR_381, 2: _FR_377, 3: _FR_381}


def _first_not_below(data: bytes, r: int) -> int:
    """Index of the first 32-byte little-endian integer >= r, or -1."""
    a = np.frombuffer(data, dtype="<u8").reshape(-1, 4)
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for i in (3, 2, 1, 0):
        ri = np.uint64((r >> (64 * i)) & ((1 << 64) - 1))
        lt |= eq & (a[:, i] < ri)
        eq &= a[:, i] == ri
    bad = np.flatnonzero(~lt)
    return int(bad[0]) if bad.size else -1


def read_scalars_bin(path: str, curve=None) -> Tuple[bytes, int]:
    """``scalars.bin`` (``Vec<Fr>``) -> (the file's 32-byte little-endian normal-form integers, count).  A value >= r is rejected
    with ValueError, as arkworks' ``from_repr`` rejects it: r of ``curve``'s scalar field, or -- no curve given, the file does not
    say which field it holds -- the larger r of the two (BLS12-381's), which no scalar of either field reaches.  The harness runs
    these integers as their Montgomery images (module docstring)."""
    with open(path, "rb") as f:
        head = f.read(8)
        if len(head) != 8:
            raise ValueError(f"{path}: no element count")
        (n,) = struct.unpack("<Q", head)
        data = f.read(n * 32)
    if len(data) != n * 32:
        raise ValueError(f"{path}: expected {n} scalars, file is short")
    r = max(SCALAR_FIELD_ORDER.values()) if curve is None else SCALAR_FIELD_ORDER[_curve_id(curve)]
    bad = _first_not_below(data, r)
    if bad >= 0:
        raise ValueError(f"{path}: scalar {bad} is not below the scalar field order")
    return data, n


def write_scalars_bin(path: str, scalars: bytes) -> None:
    if len(scalars) % 32:
        raise ValueError("scalars must be 32-byte integers")
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(scalars) // 32))
        f.write(scalars)


def _hex_tokens(path: str) -> List[str]:
    with open(path) as f:
        return f.read().split()


def read_hex_scalars(path: str, count: int = -1) -> bytes:
    toks = _hex_tokens(path)
    toks = toks if count < 0 else toks[:count]
    return b"".join(int(t, 16).to_bytes(32, "little") for t in toks)


def read_hex_points(path: str, count: int = -1, curve="bls12_377_g1") -> bytes:
    """x y pairs in hex (normal form) -> uncompressed serialized records (G1 only: one token per coordinate)."""
    if _COORD_BYTES[_curve_id(curve)] != 48:
        raise ValueError("hex point files hold G1 points")
    toks = _hex_tokens(path)
    if len(toks) % 2:
        raise ValueError(f"{path}: odd number of coordinates")
    pairs = len(toks) // 2 if count < 0 else count
    out = bytearray()
    for i in range(pairs):
        out += int(toks[2 * i], 16).to_bytes(48, "little") + int(toks[2 * i + 1], 16).to_bytes(48, "little")
    return bytes(out)


def set_bases_serialized(ctx: MultiScalarMultContext, records: bytes) -> None:
    """Upload uncompressed serialized points (see module docstring); conversion to Montgomery form runs on the GPU."""
    rb = record_bytes(ctx.curve)
    if len(records) % rb:
        raise ValueError(f"records must be {rb}-byte uncompressed points")
    n = len(records) // rb
    buf = ctypes.create_string_buffer(records, len(records) or 1)
    lib = load_library()
    _check(lib.mi355_msm_set_bases_serialized(ctx.context, buf, n))
    ctx.npoints = n


def point_to_serialized(projective: bytes, curve="bls12_377_g1", compressed: bool = False) -> bytes:
    """A result (Projective image) as one uncompressed serialized affine record, comparable with arkworks_results.bin;
    ``compressed``: as one compressed record (x and the two flag bits)."""
    lib = load_library()
    if len(projective) != projective_bytes(curve):
        raise ValueError("wrong projective image size")
    out = ctypes.create_string_buffer(record_bytes(curve, compressed))
    buf = ctypes.create_string_buffer(projective, len(projective))
    fn = lib.mi355_msm_point_to_compressed if compressed else lib.mi355_msm_point_to_serialized
    _check(fn(_curve_id(curve), buf, out))
    return out.raw


def write_results_bin(path: str, results: List[bytes], curve="bls12_377_g1") -> None:
    """``arkworks_results.bin``: the per-batch results as ``Vec<Affine>``."""
    write_points_bin(path, b"".join(point_to_serialized(r, curve) for r in results), curve)


class HarnessData(NamedTuple):
    """A ``TEST_LOAD_DATA_FROM`` directory: ``records`` (serialized points), ``scalars`` (the file's normal-form integers, batch after
    batch), ``n`` points, ``batches``, ``expected`` (one serialized record per batch, from ``arkworks_results.bin``)."""
    records: bytes
    scalars: bytes
    n: int
    batches: int
    expected: List[bytes]


def load_harness_dir(path: str, curve="bls12_377_g1", validate: bool = False) -> HarnessData:
    """Read ``points.bin``, ``scalars.bin`` and ``arkworks_results.bin`` of a harness data directory (P1B test_fpga_harness
    src/util.rs:72-140: ``batches`` scalar vectors of ``n`` each, one result per batch)."""
    import os

    records, n = read_points_bin(os.path.join(path, "points.bin"), curve, validate=validate)   # (validate: the bases, not the results)
    scalars, ns = read_scalars_bin(os.path.join(path, "scalars.bin"), curve)
    res, nr = read_points_bin(os.path.join(path, "arkworks_results.bin"), curve)
    if n == 0 or ns % n or ns // n != nr:
        raise ValueError(f"{path}: {ns} scalars and {nr} results do not make whole batches of {n} points")
    rb = record_bytes(curve)
    return HarnessData(records, scalars, n, nr, [res[i * rb:(i + 1) * rb] for i in range(nr)])


def run_harness_dir(ctx: MultiScalarMultContext, data: HarnessData, scalars=None, to_montgomery: bool = True) -> List[bool]:
    """What the harness computes for a loaded data set: the file's integers run as their Montgomery images (context option
    ``scalars_to_montgomery``, left set on ``ctx``), one MSM per batch.  ``scalars``: the same bytes elsewhere (e.g. a device
    tensor) instead of ``data.scalars``.  Returns, per batch, whether the serialized result equals ``arkworks_results.bin``."""
    ctx.set_option("scalars_to_montgomery", 1 if to_montgomery else 0)
    set_bases_serialized(ctx, data.records)
    got = ctx.run(data.scalars if scalars is None else scalars, data.n)
    return [point_to_serialized(g, ctx.curve) == e for g, e in zip(got, data.expected)]
