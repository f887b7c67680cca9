"""ctypes binding of libmi355msm.so plus the host-side mirror of the reference operator API.

Mirrors (names, argument meaning, error behaviour) the Rust layer every prize1a entry exposes:

  * ``multi_scalar_mult_init(points) -> MultiScalarMultContext`` and
    ``multi_scalar_mult(ctx, points, scalars) -> Vec<G::Projective>`` with
    ``batch_size = scalars.len() / points.len()``
    (P1A 6block/src/lib.rs:54-109, yrrid/src/lib.rs:38-90; the Rust side panics on a non-zero
    error code -- here that is ``MsmError``);
  * ``VariableBaseMSM::msm(bases, scalars)`` truncating to the shorter slice and ``msm_checked``
    (ARK ec/src/msm/variable_base/mod.rs:44-65).

Inputs are the byte images the reference passes across its FFI: arkworks
``G1Affine`` arrays (104-B stride), ``BigInteger256`` arrays (32 B), results are 144-B normalised
``G1Projective`` images.  They may be ``bytes``/``bytearray``/NumPy uint8 arrays (host) or torch uint8
tensors (host or device; device tensors are used in place through their ``data_ptr``).

There is no CPU fallback here: if the HIP library is missing or no GPU is visible, calls raise.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import List, Optional, Sequence

CURVE_IDS = {"bls12_377_g1": 0, "bls12_381_g1": 1, "bls12_377_g2": 2, "bls12_381_g2": 3}
AFFINE_STRIDE = 104          # size_of::<G1Affine>()
SCALAR_BYTES = 32
PROJECTIVE_BYTES = 144       # size_of::<G1Projective>()
_COORD_BYTES = {0: 48, 1: 48, 2: 96, 3: 96}   # G2 coordinates live in Fq2 (c0 | c1)


def affine_stride(curve) -> int:
    """size_of::<Affine>() for the curve: two coordinates + the infinity flag, padded to 8 (104 for G1, 200 for G2)."""
    return 2 * _COORD_BYTES[_curve_id(curve)] + 8


def projective_bytes(curve) -> int:
    """size_of::<Projective>(): three coordinates (144 for G1, 288 for G2)."""
    return 3 * _COORD_BYTES[_curve_id(curve)]
T_NAMES = ("digits", "sort", "accumulate", "segreduce", "bucket_reduce", "host_fold", "total")

_LIB = None


class MsmError(RuntimeError):
    """Non-zero RustError from the C ABI (the Rust harness panics here)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"mi355_msm error {code}: {message}")
        self.code = code
        self.message = message


class _RustError(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int), ("message", ctypes.c_void_p)]


def library_path() -> str:
    """The product library; MI355_MSM_LIBRARY names another build of it (tests: libmi355msm_debug.so, the -DMSM_DEBUG build)."""
    override = os.environ.get("MI355_MSM_LIBRARY")
    if override:
        return override if os.path.isabs(override) else os.path.join(os.path.dirname(os.path.abspath(__file__)), override)
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmi355msm.so")


def load_library() -> ctypes.CDLL:
    """Load the HIP shared library built by ``__graft_entry__.build()``; fail loudly when absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build the gfx950 extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the MSM path.")
    # torch bundles its own libamdhip64.so.7; whichever HIP runtime is mapped first serves the whole process.
    # Import torch first so that tensors handed to this library and the library itself share ONE runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    sigs = {
        "mi355_msm_create": [ctypes.POINTER(vp), ci, ci],
        "mi355_msm_create_sharded": [ctypes.POINTER(vp), ci, ctypes.POINTER(ci), ci],
        "mi355_msm_create_env": [ctypes.POINTER(vp), ci],
        "mi355_msm_shard_bounds": [sz, ci, ci, ctypes.POINTER(sz), ctypes.POINTER(sz)],
        "mi355_msm_destroy": [vp],
        "mi355_msm_set_bases": [vp, vp, sz, sz],
        "mi355_msm_set_bases_device": [vp, vp, sz, sz],
        "mi355_msm_check_bases": [vp, vp, sz, sz, ctypes.c_uint, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_check_bases_device": [vp, vp, sz, sz, ctypes.c_uint, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_run": [vp, vp, vp, sz, sz],
        "mi355_msm_run_device": [vp, vp, vp, sz, sz, vp],
        "mi355_msm_run_async": [vp, vp, vp, sz, sz, vp, vp, vp, ctypes.POINTER(vp)],
        "mi355_msm_job_wait": [vp],
        "mi355_msm_set_option": [vp, ctypes.c_char_p, ctypes.c_long],
        "mi355_msm_last_timings": [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_shard_timings": [vp, ci, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm": [ci, vp, vp, sz, vp, sz],
        "mi355_msm_fold": [ci, vp, vp, sz],
        "mi355_msm_generate_points": [ci, ctypes.c_uint64, sz, sz, vp, sz],
        "mi355_msm_plan": [ci, sz, ci, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_set_bases_serialized": [vp, vp, sz],
        "mi355_msm_point_to_serialized": [ci, vp, vp],
        "mi355_msm_decompress_points": [vp, vp, sz, vp, sz, ctypes.c_uint, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_decompress_points_device": [vp, vp, sz, vp, sz, ctypes.c_uint, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_compress_points": [vp, vp, sz, sz, ctypes.c_uint, vp, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_compress_points_device": [vp, vp, sz, sz, ctypes.c_uint, vp, vp, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_set_bases_compressed": [vp, vp, sz],
        "mi355_msm_point_to_compressed": [ci, vp, vp],
        "mi355_msm_mul_points": [vp, vp, sz, sz, vp, sz, ctypes.c_uint, vp, sz],
        "mi355_msm_mul_points_device": [vp, vp, sz, sz, vp, sz, ctypes.c_uint, vp, sz, vp],
        "mi355_msm_segments": [vp, vp, sz, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_uint, vp, sz, vp],
        "mi355_msm_fft_points": [vp, vp, vp, sz, vp, sz, sz, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_fft_points_device": [vp, vp, vp, sz, vp, sz, sz, ctypes.c_uint, ctypes.c_uint, vp, vp],
        "mi355_msm_last_stateless": [ctypes.POINTER(ctypes.c_double), sz],
        "mi355_msm_stream_create": [ctypes.POINTER(vp), ci, ci, sz, ci],
        "mi355_msm_stream_set_option": [vp, ctypes.c_char_p, ctypes.c_long],
        "mi355_msm_stream_add": [vp, vp, sz, vp, sz],
        "mi355_msm_stream_finalize": [vp, vp],
        "mi355_msm_stream_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_stream_destroy": [vp],
        "mi355_msm_fixed_create": [ctypes.POINTER(vp), ci, ci, vp, ci, sz],
        "mi355_msm_fixed_mul": [vp, vp, sz, vp, sz, ctypes.c_uint],
        "mi355_msm_fixed_mul_device": [vp, vp, sz, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_fixed_set_option": [vp, ctypes.c_char_p, ctypes.c_long],
        "mi355_msm_fixed_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_fixed_destroy": [vp],
        "mi355_msm_domain_create": [ctypes.POINTER(vp), ci, ci, sz],
        "mi355_msm_domain_transform": [vp, vp, vp, sz, sz, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_domain_transform_device": [vp, vp, vp, sz, sz, ctypes.c_uint, ctypes.c_uint, vp, vp],
        "mi355_msm_domain_mul": [vp, vp, vp, vp, sz, ctypes.c_uint],
        "mi355_msm_domain_mul_device": [vp, vp, vp, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_domain_set_option": [vp, ctypes.c_char_p, ctypes.c_long],
        "mi355_msm_domain_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_domain_element": [vp, ctypes.c_uint64, vp],
        "mi355_msm_domain_destroy": [vp],
        "mi355_msm_domain_batch_inverse": [vp, vp, vp, sz, vp, ctypes.c_uint],
        "mi355_msm_domain_batch_inverse_device": [vp, vp, vp, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_vec_op": [vp, vp, vp, vp, vp, sz, ctypes.c_uint, ctypes.c_uint],
        "mi355_msm_domain_vec_op_device": [vp, vp, vp, vp, vp, sz, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_domain_evaluate": [vp, vp, vp, sz, vp, ctypes.c_uint],
        "mi355_msm_domain_evaluate_device": [vp, vp, vp, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_divide_by_linear": [vp, vp, vp, vp, sz, vp, ctypes.c_uint],
        "mi355_msm_domain_divide_by_linear_device": [vp, vp, vp, vp, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_lagrange": [vp, vp, vp, ctypes.c_uint],
        "mi355_msm_domain_lagrange_device": [vp, vp, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_vanishing": [vp, vp, vp, ctypes.c_uint],
        "mi355_msm_domain_divide_by_vanishing_on_coset": [vp, vp, vp, sz, vp, ctypes.c_uint],
        "mi355_msm_domain_divide_by_vanishing_on_coset_device": [vp, vp, vp, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_scan": [vp, vp, vp, vp, sz, ctypes.c_uint, ctypes.c_uint],
        "mi355_msm_domain_scan_device": [vp, vp, vp, vp, sz, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_domain_permutation_product": [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, ctypes.c_uint],
        "mi355_msm_domain_permutation_product_device": [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_plonk_quotient": [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, ctypes.c_uint],
        "mi355_msm_domain_plonk_quotient_device": [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp, ctypes.c_uint, vp],
        "mi355_msm_domain_linear_combination": [vp, vp, vp, vp, vp, sz, ctypes.c_uint],
        "mi355_msm_domain_linear_combination_device": [vp, vp, vp, vp, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_sparse_create": [ctypes.POINTER(vp), vp, sz, sz, vp, vp, vp, ctypes.c_uint],
        "mi355_msm_sparse_apply": [vp, vp, vp, ctypes.c_uint, vp],
        "mi355_msm_sparse_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_sparse_destroy": [vp],
        "mi355_msm_lookup_create": [ctypes.POINTER(vp), vp, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_lookup_count": [vp, vp, vp, vp, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_lookup_sorted": [vp, vp, vp, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_lookup_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_lookup_destroy": [vp],
        "mi355_msm_domain_logup_sum": [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_expr_create": [ctypes.POINTER(vp), vp, vp, sz, vp, sz, sz, sz, ctypes.c_uint],
        "mi355_msm_expr_run": [vp, vp, vp, vp, sz, sz, sz, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_expr_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_expr_destroy": [vp],
        "mi355_msm_poseidon_create": [ctypes.POINTER(vp), vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, vp, vp, ctypes.c_uint],
        "mi355_msm_poseidon_hash": [vp, vp, vp, sz, sz, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_poseidon_merkle": [vp, vp, vp, sz, sz, vp, ctypes.c_uint, vp],
        "mi355_msm_poseidon_set_option": [vp, ctypes.c_char_p, ctypes.c_long],
        "mi355_msm_poseidon_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_poseidon_destroy": [vp],
        "mi355_msm_pairing_create": [ctypes.POINTER(vp), ci, ci],
        "mi355_msm_pairing_run": [vp, vp, vp, sz, vp, sz, sz, sz, ctypes.c_uint, vp],
        "mi355_msm_pairing_check": [vp, vp, vp, sz, vp, sz, sz, sz, ctypes.c_uint, vp],
        "mi355_msm_pairing_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_pairing_destroy": [vp],
        "mi355_msm_h2c_create": [ctypes.POINTER(vp), ci, vp, sz, ci],
        "mi355_msm_h2c_field": [vp, vp, vp, sz, vp, sz, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_h2c_map": [vp, vp, sz, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_h2c_hash": [vp, vp, sz, vp, sz, vp, sz, ctypes.c_uint, vp],
        "mi355_msm_h2c_query": [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)],
        "mi355_msm_h2c_destroy": [vp],
        "mi355_msm_domain_mle_fix": [vp, vp, vp, ctypes.c_uint, vp, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_domain_mle_eq": [vp, vp, vp, ctypes.c_uint, ctypes.c_uint, vp],
        "mi355_msm_domain_sumcheck_round": [vp, vp, vp, sz, ctypes.c_uint, vp, sz, vp, vp, ctypes.c_uint, vp],
        "mi355_msm_trim": [],
        "mi355_msm_pool_stats": [ctypes.POINTER(ctypes.c_uint64), sz],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = _RustError
    lib.mi355_msm_version.restype = ctypes.c_char_p
    lib.mi355_msm_fixed_window_size.argtypes = [sz]
    lib.mi355_msm_fixed_window_size.restype = sz
    lib.mi355_msm_job_done.argtypes = [vp]
    lib.mi355_msm_job_done.restype = ci
    _LIB = lib
    return lib


_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]


def _check(err: _RustError) -> None:
    if err.code != 0:
        msg = ctypes.string_at(err.message).decode("utf-8", "replace") if err.message else "(no message)"
        if err.message:
            _libc.free(err.message)
        raise MsmError(err.code, msg)


def _curve_id(curve) -> int:
    if isinstance(curve, int):
        return curve
    try:
        return CURVE_IDS[curve]
    except KeyError:
        raise ValueError(f"unknown curve {curve!r}; known: {sorted(CURVE_IDS)}") from None


class _Buf:
    """Uniform view of bytes / numpy / torch inputs: pointer, byte length, device flag, keep-alive."""

    def __init__(self, obj):
        self.keep = obj
        self.is_device = False
        self.stream = None
        if hasattr(obj, "data_ptr") and hasattr(obj, "is_cuda"):  # torch tensor
            import torch

            t = obj
            if t.dtype != torch.uint8:
                raise TypeError("tensor inputs must be torch.uint8 byte images")
            if not t.is_contiguous():
                t = t.contiguous()
            self.keep = t
            self.ptr = t.data_ptr()
            self.nbytes = t.numel()
            self.is_device = bool(t.is_cuda)
            if self.is_device:
                self.device_index = t.device.index if t.device.index is not None else torch.cuda.current_device()
                self.stream = torch.cuda.current_stream(t.device).cuda_stream
        elif hasattr(obj, "__array_interface__"):  # numpy
            import numpy as np

            a = np.ascontiguousarray(obj)
            if a.dtype != np.uint8:
                a = a.view(np.uint8)
            self.keep = a
            self.ptr = a.ctypes.data
            self.nbytes = a.nbytes
        else:
            b = obj if isinstance(obj, (bytes, bytearray)) else bytes(obj)
            self.keep = (ctypes.c_char * len(b)).from_buffer_copy(b) if len(b) else ctypes.create_string_buffer(1)
            self.ptr = ctypes.addressof(self.keep)
            self.nbytes = len(b)


def _flat_bytes(obj):
    """1-D byte view of a bytes / numpy / torch input, sliceable by byte offset."""
    if hasattr(obj, "data_ptr") and hasattr(obj, "is_cuda"):
        return obj.contiguous().reshape(-1)
    if hasattr(obj, "__array_interface__"):
        import numpy as np

        return np.ascontiguousarray(obj).view(np.uint8).reshape(-1)
    return memoryview(obj if isinstance(obj, (bytes, bytearray)) else bytes(obj))


CHECK_STATUS_TEXT = ("valid", "a coordinate is not below p", "not on the curve", "outside the order-r subgroup")


class CheckResult:
    """What MultiScalarMultContext.check_bases found: `status` holds one byte per point (0 valid, 1 not canonical, 2 off the curve,
    3 outside the order-r subgroup)."""

    def __init__(self, ok, counts, first_invalid, status, method, device_us):
        self.ok, self.counts, self.first_invalid, self.status, self.method, self.device_us = ok, counts, first_invalid, status, method, device_us

    def __repr__(self):
        return f"CheckResult(ok={self.ok}, counts={self.counts}, first_invalid={self.first_invalid}, method={self.method!r}, device_us={self.device_us})"


CODEC_STATUS_TEXT = ("decoded", "malformed: x is not below p or both flag bits are set", "no point has this x",
                     "outside the order-r subgroup")


class CodecResult:
    """What decompress_points / compress_points produced: `points` (decompress: Affine images or uncompressed records; compress: the
    compressed records) in the kind of container the input came in, `status` one byte per record (decompress: 0 decoded or flagged
    infinity, 1 malformed, 2 no point has this x, 3 outside the order-r subgroup when validation was asked for; compress: 1 = a
    coordinate is not canonical), `counts`, `first_invalid` (None when every status is 0)."""

    def __init__(self, points, ok, counts, first_invalid, status, method, device_us):
        self.points, self.ok, self.counts, self.first_invalid, self.status = points, ok, counts, first_invalid, status
        self.method, self.device_us = method, device_us

    @property
    def records(self):
        return self.points

    def __repr__(self):
        return f"CodecResult(ok={self.ok}, counts={self.counts}, first_invalid={self.first_invalid}, device_us={self.device_us})"


def _like_input(src, out_np, shape):
    """A NumPy result in the container kind of `src`: torch CPU tensor, NumPy array or bytes."""
    if hasattr(src, "data_ptr") and hasattr(src, "is_cuda"):
        import torch

        return torch.from_numpy(out_np.reshape(shape))
    if hasattr(src, "__array_interface__"):
        return out_np.reshape(shape)
    return out_np.tobytes()


class MultiScalarMultContext:
    """``#[repr(C)] struct MultiScalarMultContext { context: *mut c_void }`` (P1A 6block/src/lib.rs:18-21)."""

    def __init__(self, curve="bls12_377_g1", device: Optional[int] = None, devices: Optional[Sequence[int]] = None):
        """``device``: one GPU (None = the current HIP device).  ``devices``: a SHARDED context over those GPUs, one slice of the
        bases and of every scalar batch per entry (an id may repeat: logical shards on one GPU); same methods, same results."""
        self.curve = _curve_id(curve)
        self._lib = load_library()
        self.context = ctypes.c_void_p()
        self.devices = None if devices is None else [int(d) for d in devices]
        if self.devices is not None:
            arr = (ctypes.c_int * len(self.devices))(*self.devices)
            _check(self._lib.mi355_msm_create_sharded(ctypes.byref(self.context), self.curve, arr, len(self.devices)))
            self.device = None
        else:
            _check(self._lib.mi355_msm_create(ctypes.byref(self.context), self.curve, -1 if device is None else device))
            self.device = self.query("device")
        self.npoints = 0

    def _check_device(self, b: "_Buf", what: str) -> None:
        # a pointer from another GPU would be dereferenced after hipSetDevice(ctx.device): fail with a clear message instead
        if b.is_device and self.device is not None and b.device_index != self.device:
            raise MsmError(-1, f"{what} live on cuda:{b.device_index} but this context is bound to device {self.device}")

    @classmethod
    def from_env(cls, curve="bls12_377_g1") -> "MultiScalarMultContext":
        """What the harness shims do: honour MI355_MSM_DEVICES ("0,1,2,3", "0-7", "all"; unset = the current device),
        MI355_MSM_ASSUME_SUBGROUP (0 | 1: the context option of that name) and MI355_MSM_PRECOMPUTE (auto | 1 | 0) /
        MI355_MSM_TABLE_LEVELS (options "precompute" / "table_levels")."""
        self = cls.__new__(cls)
        self.curve = _curve_id(curve)
        self._lib = load_library()
        self.context = ctypes.c_void_p()
        _check(self._lib.mi355_msm_create_env(ctypes.byref(self.context), self.curve))
        self.npoints = 0
        self.devices = None
        self.device = None if self.query("shards") else self.query("device")
        return self

    def set_bases(self, points, stride: Optional[int] = None) -> None:
        stride = affine_stride(self.curve) if stride is None else stride
        b = _Buf(points)
        if b.nbytes % stride:
            raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {stride}-byte affine stride")
        n = b.nbytes // stride
        self._check_device(b, "bases")
        fn = self._lib.mi355_msm_set_bases_device if b.is_device else self._lib.mi355_msm_set_bases
        _check(fn(self.context, b.ptr, n, stride))
        self.npoints = n

    def check_bases(self, points, stride: Optional[int] = None, serialized: bool = False, exact: bool = False) -> "CheckResult":
        """On-curve and subgroup check of `points` on the context's device (mi355_msm_check_bases): bytes, numpy or torch CPU / GPU
        tensors like set_bases.  `serialized`: uncompressed CanonicalSerialize records instead of in-memory Affine images.  `exact`:
        decide the subgroup by [r]P == O instead of the endomorphism test (same verdicts).  The context's bases are not touched."""
        import numpy as np

        rec = 2 * (projective_bytes(self.curve) // 3) if serialized else (affine_stride(self.curve) if stride is None else stride)
        b = _Buf(points)
        if b.nbytes % rec:
            raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {rec}-byte record")
        n = b.nbytes // rec
        self._check_device(b, "points")
        status = np.zeros(n, dtype=np.uint8)
        out = (ctypes.c_uint64 * 8)()
        fn = self._lib.mi355_msm_check_bases_device if b.is_device else self._lib.mi355_msm_check_bases
        flags = (1 if serialized else 0) | (2 if exact else 0)
        _check(fn(self.context, b.ptr, n, rec, flags, status.ctypes.data_as(ctypes.c_void_p) if n else None, out))
        counts = {"valid": int(out[0]), "flagged_infinity": int(out[1]), "not_canonical": int(out[2]), "off_curve": int(out[3]),
                  "off_subgroup": int(out[4])}
        first = int(out[5])
        return CheckResult(ok=first == n, counts=counts, first_invalid=None if first == n else first, status=status,
                           method="endomorphism" if out[6] else "exact", device_us=int(out[7]))

    def _codec_result(self, points, out, n, kind) -> "CodecResult":
        counts = {"valid": int(out[0]), "flagged_infinity": int(out[1]), "malformed" if kind == "decode" else "not_canonical": int(out[2])}
        if kind == "decode":
            counts.update(no_point=int(out[3]), off_subgroup=int(out[4]))
        first = int(out[5])
        return CodecResult(points, first == n, counts, None if first == n else first, None,
                           "endomorphism" if out[6] else "exact", int(out[7]))

    def decompress_points(self, records, uncompressed: bool = False, validate: bool = False, exact: bool = False,
                          stride: Optional[int] = None) -> "CodecResult":
        """arkworks COMPRESSED records (x + two flag bits: 48 bytes per G1 point, 96 per G2 point) -> in-memory Affine images `stride`
        bytes apart (default: the image size), or with `uncompressed` uncompressed CanonicalSerialize records, decoded on the
        context's device (mi355_msm_decompress_points).  `validate`: also run the subgroup check of check_bases over the decoded
        points (status 3; `exact`: by [r]P == O).  bytes, NumPy and torch CPU inputs give the same kind back; a torch GPU tensor is
        read in place and gives a GPU tensor.  A record that fails decodes to zeros (see CodecResult.status)."""
        import numpy as np

        cid = self.curve
        cb = projective_bytes(cid) // 3
        rec = 2 * cb if uncompressed else (affine_stride(cid) if stride is None else int(stride))
        if not uncompressed and (rec % 4 or rec < 2 * cb + 1):
            raise ValueError(f"stride {rec} must be a multiple of 4 and at least {2 * cb + 1}")
        b = _Buf(records)
        if b.nbytes % cb:
            raise ValueError(f"records of {b.nbytes} bytes are not a multiple of the {cb}-byte compressed record")
        n = b.nbytes // cb
        self._check_device(b, "records")
        status = np.zeros(n, dtype=np.uint8)
        out8 = (ctypes.c_uint64 * 8)()
        flags = (1 if uncompressed else 0) | (2 if validate else 0) | (4 if exact else 0)
        sp = status.ctypes.data_as(ctypes.c_void_p) if n else None
        if b.is_device:
            import torch

            pts = torch.zeros((n, rec), dtype=torch.uint8, device=b.keep.device)
            _check(self._lib.mi355_msm_decompress_points_device(self.context, b.ptr, n, pts.data_ptr() if n else None, rec, flags, sp, out8))
        else:
            o = np.zeros(n * rec, dtype=np.uint8)
            _check(self._lib.mi355_msm_decompress_points(self.context, b.ptr, n, o.ctypes.data if n else None, rec, flags, sp, out8))
            pts = _like_input(records, o, (n, rec))
        res = self._codec_result(pts, out8, n, "decode")
        res.status = status
        return res

    def compress_points(self, points, serialized: bool = False, stride: Optional[int] = None) -> "CodecResult":
        """In-memory Affine images (`stride` bytes apart) or, with `serialized`, uncompressed records -> compressed records
        (mi355_msm_compress_points): what arkworks' plain `serialize` writes.  Containers as in decompress_points.  Status 1: a
        coordinate is not canonical (the record is then all zeros); there is no curve test, as in arkworks."""
        import numpy as np

        cid = self.curve
        cb = projective_bytes(cid) // 3
        rec = 2 * cb if serialized else (affine_stride(cid) if stride is None else int(stride))
        b = _Buf(points)
        if b.nbytes % rec:
            raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {rec}-byte record")
        n = b.nbytes // rec
        self._check_device(b, "points")
        status = np.zeros(n, dtype=np.uint8)
        out8 = (ctypes.c_uint64 * 8)()
        sp = status.ctypes.data_as(ctypes.c_void_p) if n else None
        if b.is_device:
            import torch

            recs = torch.zeros((n, cb), dtype=torch.uint8, device=b.keep.device)
            _check(self._lib.mi355_msm_compress_points_device(self.context, b.ptr, n, rec, 1 if serialized else 0, recs.data_ptr() if n else None, sp, out8))
        else:
            o = np.zeros(n * cb, dtype=np.uint8)
            _check(self._lib.mi355_msm_compress_points(self.context, b.ptr, n, rec, 1 if serialized else 0, o.ctypes.data if n else None, sp, out8))
            recs = _like_input(points, o, (n, cb))
        res = self._codec_result(recs, out8, n, "encode")
        res.status = status
        return res

    def set_bases_compressed(self, records) -> None:
        """Upload bases as compressed records in host memory (mi355_msm_set_bases_compressed): the square roots run on the GPU.  A
        record that does not decode raises MsmError naming its index and status, and the previous bases stay in force."""
        cb = projective_bytes(self.curve) // 3
        b = _Buf(records)
        if b.is_device:
            raise TypeError("set_bases_compressed takes host records; decode a device tensor with decompress_points and pass the images to set_bases")
        if b.nbytes % cb:
            raise ValueError(f"records must be {cb}-byte compressed points")
        n = b.nbytes // cb
        _check(self._lib.mi355_msm_set_bases_compressed(self.context, b.ptr, n))
        self.npoints = n

    def _mul_points(self, points, scalars, scalar_bytes, flags, stride, out_stride):
        """mi355_msm_mul_points[_device]: `scalars` is a _Buf of pairwise scalars, or the bytes of one scalar (flag bit 2), or None."""
        import numpy as np

        cid = self.curve
        size = projective_bytes(cid) if flags & 2 else affine_stride(cid)
        stride = affine_stride(cid) if stride is None else int(stride)
        out_stride = size if out_stride is None else int(out_stride)
        if stride % 4 or stride < 2 * (projective_bytes(cid) // 3) + 1:
            raise ValueError(f"stride {stride} must be a multiple of 4 and hold two coordinates and the flag byte")
        if out_stride % 4 or out_stride < size:
            raise ValueError(f"out_stride {out_stride} must be a multiple of 4 and at least the {size}-byte image")
        b = _Buf(points)
        if b.nbytes % stride:
            raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {stride}-byte stride")
        n = b.nbytes // stride
        self._check_device(b, "points")
        pairwise = isinstance(scalars, _Buf)
        if pairwise:
            if scalars.nbytes != n * SCALAR_BYTES:
                raise ValueError(f"{n} points need {n * SCALAR_BYTES} bytes of scalars, not {scalars.nbytes}")
            if scalars.is_device != b.is_device:
                raise TypeError("points and scalars must both be host data or both be GPU tensors")
            self._check_device(scalars, "scalars")
            sptr = scalars.ptr
        elif scalars is None:
            sptr = None
        else:
            keep = (ctypes.c_char * len(scalars)).from_buffer_copy(scalars)
            sptr = ctypes.addressof(keep)
        if b.is_device:
            import torch

            out = torch.zeros((n, out_stride), dtype=torch.uint8, device=b.keep.device)
            if n:
                _check(self._lib.mi355_msm_mul_points_device(self.context, b.ptr, n, stride, sptr, scalar_bytes, flags, out.data_ptr(), out_stride, b.stream))
            return out
        o = np.zeros(n * out_stride, dtype=np.uint8)
        if n:
            _check(self._lib.mi355_msm_mul_points(self.context, b.ptr, n, stride, sptr, scalar_bytes, flags, o.ctypes.data, out_stride))
        return _like_input(points, o, (n, out_stride))

    def mul_points(self, points, scalars, montgomery: bool = False, projective: bool = False, stride: Optional[int] = None,
                   out_stride: Optional[int] = None):
        """``out[i] = scalars[i] * points[i]`` on the context's device (mi355_msm_mul_points): arkworks' ``mul_bigint`` over a vector,
        then ``batch_normalization_into_affine``.  ``points``: Affine images ``stride`` bytes apart, ANY curve points (no curve or
        subgroup test; the flag byte is authoritative).  ``scalars``: 32-byte little-endian integers, all 256 bits significant (the
        integer multiple, never reduced mod r); ``montgomery``: arkworks ``Fr`` images.  Affine images out (``projective``: normalised
        Projective images), ``out_stride`` bytes apart.  bytes / NumPy / torch CPU in give the same kind out; GPU tensors (points and
        scalars) are read in place on the current torch stream and give a GPU tensor, ready for ``set_bases``."""
        return self._mul_points(points, _Buf(scalars), SCALAR_BYTES, (1 if montgomery else 0) | (2 if projective else 0), stride, out_stride)

    def msm_segments(self, points, scalars, offsets=None, shared: bool = False, montgomery: bool = False, projective: bool = False,
                     stride: Optional[int] = None, out_stride: Optional[int] = None, out=None, lengths=None):
        """Many small MSMs in one call (mi355_msm_segments): ``out[s] = sum of scalars[i] * points[i]`` over
        ``offsets[s] <= i < offsets[s + 1]``; an empty segment gives the point at infinity.  ``offsets``: any integer sequence or array
        of S + 1 values, 0 first, non-decreasing, the number of points last (``lengths``: the S segment lengths instead); always taken
        to the host.  ``shared=True``: ``scalars`` is ``(S, L, 32)`` and every segment runs over all L ``points``.  ``points``: Affine
        images ``stride`` bytes apart, read as ``mul_points`` reads them (the flag byte is authoritative, no curve or subgroup test).
        ``scalars``: 32-byte little-endian integers, all 256 bits significant; ``montgomery``: arkworks ``Fr`` images.  Affine images out
        (``projective``: normalised Projective images), ``out_stride`` bytes apart.  bytes / NumPy / torch CPU in give the same kind
        out; GPU tensors (points and scalars) are read in place on the current torch stream and give a GPU tensor (``out``: a GPU
        uint8 tensor of S * out_stride bytes to write into), ready for ``set_bases``, ``fft_points`` and ``compress_points``."""
        import numpy as np

        a = _segments_args(self.curve, points, scalars, offsets, lengths, shared, projective, stride, out_stride, out)
        b, sc, offs, nseg, npoints, nscalars, stride, out_stride = a
        self._check_device(b, "points")
        self._check_device(sc, "scalars")
        flags = (1 if montgomery else 0) | (2 if b.is_device else 0) | (4 if shared else 0) | (8 if projective else 0)
        optr = None if offs is None else offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        if b.is_device:
            import torch

            if out is None:
                out = torch.zeros((nseg, out_stride), dtype=torch.uint8, device=b.keep.device)
            else:
                ob = _Buf(out)
                self._check_device(ob, "out")
            if nseg:
                _check(self._lib.mi355_msm_segments(self.context, b.ptr if npoints else None, npoints, stride, sc.ptr if nscalars else None, nscalars, optr, nseg,
                                                    flags, out.data_ptr(), out_stride, b.stream))
            return out
        o = np.zeros(nseg * out_stride, dtype=np.uint8)
        if nseg:
            _check(self._lib.mi355_msm_segments(self.context, b.ptr if npoints else None, npoints, stride, sc.ptr if nscalars else None, nscalars, optr, nseg,
                                                flags, o.ctypes.data, out_stride, None))
        return _like_input(points, o, (nseg, out_stride))

    def mul_points_by(self, points, k, projective: bool = False, stride: Optional[int] = None, out_stride: Optional[int] = None):
        """``out[i] = k * points[i]`` for ONE integer k of up to 512 bits (an int, or little-endian bytes whose length is a multiple of 4
        from 4 to 64): no table, one doubling per bit and one addition per non-zero digit of k's non-adjacent form."""
        if isinstance(k, int):
            if k < 0 or k >> 512:
                raise ValueError("k must be an integer in [0, 2^512)")
            k = k.to_bytes(max(4, (k.bit_length() + 31) // 32 * 4), "little")
        k = bytes(k)
        if len(k) % 4 or not 4 <= len(k) <= 64:
            raise ValueError("k as bytes is a multiple of 4 from 4 to 64 bytes long")
        return self._mul_points(points, k, len(k), 4 | (2 if projective else 0), stride, out_stride)

    def mul_by_cofactor(self, points, projective: bool = False, stride: Optional[int] = None, out_stride: Optional[int] = None):
        """``out[i] = COFACTOR * points[i]``: arkworks' ``mul_by_cofactor`` (NOT ``clear_cofactor``, which for BLS12-381 is another map)."""
        return self._mul_points(points, None, 0, 8 | (2 if projective else 0), stride, out_stride)

    def fft_points(self, dom, points, kind: Optional[int] = None, inverse: bool = False, coset: bool = False, offset=None,
                   in_len: Optional[int] = None, projective: bool = False, stride: Optional[int] = None, out_stride: Optional[int] = None,
                   out=None):
        """``dom.fft`` / ``ifft`` / ``coset_fft`` / ``coset_ifft`` of a vector of GROUP elements (mi355_msm_fft_points): ``out[i] = sum_j
        omega^(i j) points[j]`` and its three relatives, the multipliers the canonical integers of the field elements -- what turns a
        monomial SRS ``[tau^j] G`` into the Lagrange SRS ``[L_i(tau)] G`` (``inverse=True``).  ``dom``: a ``Radix2EvaluationDomain`` of
        this curve's family on this context's device.  ``points``: Affine images ``stride`` bytes apart (flag byte authoritative,
        infinities anywhere; subgroup points, nothing is tested); the first ``in_len`` (default: all) are read and the vector is
        extended to ``dom.size`` with the point at infinity.  ``kind`` 0..3 or ``inverse`` / ``coset``; ``offset``: the coset offset as
        an integer (default: GENERATOR).  ``dom.size`` Affine images out (``projective``: normalised Projective images),
        ``out_stride`` bytes apart, in the kind of container that came in; GPU tensors are read in place on the current torch stream
        and give a GPU tensor, ready for ``set_bases``.  ``out``: a GPU tensor to write into; it may be the input when the strides are
        equal."""
        import numpy as np

        if not getattr(dom, "handle", None):
            raise MsmError(-1, "the domain is closed")
        if kind is None:
            kind = (1 if inverse else 0) | (2 if coset else 0)
        elif inverse or coset:
            raise ValueError("give kind= or inverse= / coset=, not both")
        kind = int(kind)
        if not 0 <= kind <= 3:
            raise ValueError(f"kind {kind}: 0 forward, 1 inverse, 2 coset forward, 3 coset inverse")
        if offset is not None and not kind & 2:
            raise ValueError("an offset goes with the coset kinds")
        cid = self.curve
        flags = 2 if projective else 0
        size = projective_bytes(cid) if projective else affine_stride(cid)
        stride = affine_stride(cid) if stride is None else int(stride)
        out_stride = size if out_stride is None else int(out_stride)
        if stride % 4 or stride < 2 * (projective_bytes(cid) // 3) + 1:
            raise ValueError(f"stride {stride} must be a multiple of 4 and hold two coordinates and the flag byte")
        if out_stride % 4 or out_stride < size:
            raise ValueError(f"out_stride {out_stride} must be a multiple of 4 and at least the {size}-byte image")
        b = _Buf(points)
        if b.nbytes % stride:
            raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {stride}-byte stride")
        have = b.nbytes // stride
        in_len = have if in_len is None else int(in_len)
        if in_len < 0 or in_len > have:
            raise ValueError(f"in_len {in_len} with {have} points given")
        n = int(dom.size)
        if in_len > n:
            raise ValueError(f"{in_len} points exceed the domain size {n}")
        off = None
        if offset is not None:
            off = ((int(offset) % dom.modulus) << 256) % dom.modulus
            off = off.to_bytes(32, "little")
        self._check_device(b, "points")
        if b.is_device:
            import torch

            if out is None:
                out = torch.zeros((n, out_stride), dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != n * out_stride or ob.keep is not out:
                raise ValueError(f"out must be a contiguous uint8 GPU tensor of {n * out_stride} bytes")
            self._check_device(ob, "out")
            _check(self._lib.mi355_msm_fft_points_device(self.context, dom.handle, ob.ptr, out_stride, b.ptr if in_len else None, in_len, stride, kind,
                                                         flags, off, b.stream))
            return out
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        o = np.zeros(n * out_stride, dtype=np.uint8)
        _check(self._lib.mi355_msm_fft_points(self.context, dom.handle, o.ctypes.data, out_stride, b.ptr if in_len else None, in_len, stride, kind, flags, off))
        return _like_input(points, o, (n, out_stride))

    def ifft_points(self, dom, points, **kw):
        return self.fft_points(dom, points, inverse=True, **kw)

    def run(self, scalars, npoints: Optional[int] = None) -> List[bytes]:
        b = _Buf(scalars)
        self._check_device(b, "scalars")
        n = self.npoints if npoints is None else npoints
        if b.nbytes % SCALAR_BYTES:
            raise ValueError("scalars image is not a multiple of 32 bytes")
        count = b.nbytes // SCALAR_BYTES
        if n == 0:
            batches = 1 if count == 0 else None
        else:
            batches = count // n if count % n == 0 else None
        if batches is None:
            raise ValueError(f"{count} scalars is not a whole number of batches of {n} points")
        pb = projective_bytes(self.curve)
        out = ctypes.create_string_buffer(pb * max(batches, 1))
        if b.is_device:
            _check(self._lib.mi355_msm_run_device(self.context, out, b.ptr, n, batches, b.stream))
        else:
            _check(self._lib.mi355_msm_run(self.context, out, b.ptr, n, batches))
        raw = out.raw
        return [raw[i * pb:(i + 1) * pb] for i in range(batches)]

    def run_async(self, scalars, npoints: Optional[int] = None, stream=None) -> "MsmJob":
        """Stream-ordered run (mi355_msm_run_async; the role of ML bellman-cuda.h:48-75 msm_execute_async): returns at once with a job
        handle.  ``scalars`` must be a device tensor; the MSM is ordered after the work already enqueued in ``stream`` (default: the
        tensor's current torch stream) and runs on the context's own stream, so whatever the caller launches next overlaps it.
        ``job.wait()`` returns the projective images; jobs of one context run in submission order."""
        b = _Buf(scalars)
        if not b.is_device:
            raise TypeError("run_async takes scalars that are resident on the device (use run() for host scalars)")
        self._check_device(b, "scalars")
        n = self.npoints if npoints is None else npoints
        count = b.nbytes // SCALAR_BYTES
        if b.nbytes % SCALAR_BYTES or n == 0 or count % n:
            raise ValueError(f"{count} scalars is not a whole number of batches of {n} points")
        batches = count // n
        pb = projective_bytes(self.curve)
        out = ctypes.create_string_buffer(pb * batches)
        job = ctypes.c_void_p()
        st = b.stream if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)
        _check(self._lib.mi355_msm_run_async(self.context, out, b.ptr, n, batches, st, None, None, ctypes.byref(job)))
        return MsmJob(self._lib, job, out, pb, batches, b)

    def set_option(self, key: str, value: int) -> None:
        _check(self._lib.mi355_msm_set_option(self.context, key.encode(), int(value)))

    def query(self, key: str) -> int:
        """Context state: "twisted_edwards", "twisted_edwards_fallbacks", "twisted_edwards_demotions", "oom_backoffs", "chunk_cap",
        "device", "shards", "rccl_exchanges", "peer_stagings", "bases", "table_levels", "table_window_bits", "base_bytes", "assume_subgroup",
        "carry", "precompute", "g2_paired", "anchor", "anchored_window", "anchor_sums", "anchor_sum_us", "anchor_wide", "anchor_wide_active", "anchor_wide_fallbacks",
        "anchor_wide_demotions", "entries32", "entries32_active" (the most recent chunk's sorted entries were 32-bit words with run steps),
        and the geometry of the most recent chunk: "bucket_windows", "l1_bits", "l1_bins", "group_passes",
        and how its buckets were reduced: "reduce_path" (0 recursive chunked levels only, 1 direct scan on the buckets, 2 one chunked level
        then a scan on full rows, 3 the same on rows padded to a power of two), "reduce_chunks" (chunks per bucket set on the first
        level, T0) and "reduce_row" (elements of a scan row).  A sharded context reports the largest over its shards."""
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_query(self.context, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def last_timings(self) -> dict:
        ms = (ctypes.c_float * 8)()
        info = (ctypes.c_uint64 * 8)()
        _check(self._lib.mi355_msm_last_timings(self.context, ms, info))
        d = {name: float(ms[i]) for i, name in enumerate(T_NAMES)}
        d.update(window_bits=int(info[0]), windows=int(info[1]), entries=int(info[2]), lane_entries=int(info[3]),
                 launches=int(info[4]), lanes=int(info[5]), tables=bool(info[6]), twisted_edwards=bool(info[7]))
        return d

    def shard_timings(self) -> list:
        """Per-shard stage times of the most recent run (one entry for an unsharded context)."""
        out = []
        for g in range(max(1, self.query("shards"))):
            ms = (ctypes.c_float * 8)()
            info = (ctypes.c_uint64 * 8)()
            _check(self._lib.mi355_msm_shard_timings(self.context, g, ms, info))
            d = {name: float(ms[i]) for i, name in enumerate(T_NAMES)}
            d.update(shard=g, window_bits=int(info[0]), entries=int(info[2]), launches=int(info[4]))
            out.append(d)
        return out

    def close(self) -> None:
        if self.context:
            _check(self._lib.mi355_msm_destroy(self.context))
            self.context = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_scalar_mult_init(points, curve="bls12_377_g1", device: Optional[int] = None,
                           devices: Optional[Sequence[int]] = None) -> MultiScalarMultContext:
    """Upload (and convert) the fixed base vector once; untimed in the reference bench (benches/msm.rs:21).
    ``devices`` shards the vector over several GPUs behind the same context (see MultiScalarMultContext)."""
    if devices is None and device is None and os.environ.get("MI355_MSM_DEVICES"):
        ctx = MultiScalarMultContext.from_env(curve)
        ctx.set_bases(points)
        return ctx
    ctx = MultiScalarMultContext(curve, device, devices)
    ctx.set_bases(points)
    return ctx


def check_points(points, curve="bls12_377_g1", stride: Optional[int] = None, serialized: bool = False, exact: bool = False,
                 device: Optional[int] = None) -> CheckResult:
    """MultiScalarMultContext.check_bases on a throwaway context."""
    ctx = MultiScalarMultContext(curve, device)
    try:
        return ctx.check_bases(points, stride=stride, serialized=serialized, exact=exact)
    finally:
        ctx.close()


def decompress_points(records, curve="bls12_377_g1", uncompressed: bool = False, validate: bool = False, exact: bool = False,
                      stride: Optional[int] = None, device: Optional[int] = None) -> CodecResult:
    """MultiScalarMultContext.decompress_points on a throwaway context (on the tensor's device for a GPU tensor)."""
    if device is None and getattr(records, "is_cuda", False):
        device = records.device.index
    ctx = MultiScalarMultContext(curve, device)
    try:
        return ctx.decompress_points(records, uncompressed=uncompressed, validate=validate, exact=exact, stride=stride)
    finally:
        ctx.close()


def compress_points(points, curve="bls12_377_g1", serialized: bool = False, stride: Optional[int] = None,
                    device: Optional[int] = None) -> CodecResult:
    """MultiScalarMultContext.compress_points on a throwaway context (on the tensor's device for a GPU tensor)."""
    if device is None and getattr(points, "is_cuda", False):
        device = points.device.index
    ctx = MultiScalarMultContext(curve, device)
    try:
        return ctx.compress_points(points, serialized=serialized, stride=stride)
    finally:
        ctx.close()


def _throwaway(points, curve, device, call):
    if device is None and getattr(points, "is_cuda", False):
        device = points.device.index
    ctx = MultiScalarMultContext(curve, device)
    try:
        return call(ctx)
    finally:
        ctx.close()


def mul_points(points, scalars, curve="bls12_377_g1", montgomery: bool = False, projective: bool = False, stride: Optional[int] = None,
               out_stride: Optional[int] = None, device: Optional[int] = None):
    """MultiScalarMultContext.mul_points on a throwaway context (on the tensor's device for a GPU tensor)."""
    return _throwaway(points, curve, device, lambda c: c.mul_points(points, scalars, montgomery=montgomery, projective=projective, stride=stride,
                                                                   out_stride=out_stride))


def _segments_args(cid, points, scalars, offsets, lengths, shared, projective, stride, out_stride, out):
    """The argument checks of msm_segments, all on the host and before any GPU work: (points _Buf, scalars _Buf, offsets as a uint64
    array or None, segments, points, scalars, stride, out_stride)."""
    import numpy as np

    size = projective_bytes(cid) if projective else affine_stride(cid)
    stride = affine_stride(cid) if stride is None else int(stride)
    out_stride = size if out_stride is None else int(out_stride)
    if stride % 4 or stride < 2 * (projective_bytes(cid) // 3) + 1:
        raise ValueError(f"stride {stride} must be a multiple of 4 and hold two coordinates and the flag byte")
    if out_stride % 4 or out_stride < size:
        raise ValueError(f"out_stride {out_stride} must be a multiple of 4 and at least the {size}-byte image")
    b, sc = _Buf(points), _Buf(scalars)
    if b.nbytes % stride:
        raise ValueError(f"points image of {b.nbytes} bytes is not a multiple of the {stride}-byte stride")
    if sc.nbytes % SCALAR_BYTES:
        raise ValueError(f"scalars of {sc.nbytes} bytes are not a multiple of {SCALAR_BYTES}")
    if sc.is_device != b.is_device:
        raise TypeError("points and scalars must both be host data or both be GPU tensors")
    npoints, nscalars = b.nbytes // stride, sc.nbytes // SCALAR_BYTES
    if npoints >= 1 << 32:
        raise ValueError(f"{npoints} points exceed 2^32-1")
    if shared:
        if offsets is not None or lengths is not None:
            raise ValueError("shared=True takes neither offsets nor lengths: every segment runs over all points")
        shape = tuple(getattr(scalars, "shape", ()))
        if len(shape) == 3 and shape[1] != npoints:
            raise ValueError(f"shared=True takes scalars of shape (S, {npoints}, 32), not {shape}")
        if npoints == 0:
            if len(shape) != 3:
                raise ValueError("shared=True with no points takes scalars of shape (S, 0, 32): the number of segments is its first dimension")
            nseg = int(shape[0])
        else:
            if nscalars % npoints:
                raise ValueError(f"shared=True: {nscalars} scalars are not a multiple of the {npoints} points")
            nseg = nscalars // npoints
        offs = None
    else:
        if (offsets is None) == (lengths is None):
            raise ValueError("pass offsets (S + 1 values) or lengths (S values), one of them")
        src = offsets if offsets is not None else lengths
        if hasattr(src, "detach"):
            src = src.detach().cpu().numpy()
        arr = np.asarray(src)
        if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
            raise ValueError("offsets / lengths must be a one-dimensional integer sequence")
        if arr.size and int(arr.min()) < 0:
            raise ValueError("offsets / lengths must not be negative")
        arr = arr.astype(np.uint64)
        if offsets is None:
            arr = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(arr, dtype=np.uint64)])
        if arr.size == 0:
            raise ValueError("offsets hold S + 1 values: at least the leading 0")
        if int(arr[0]) != 0:
            raise ValueError(f"offsets[0] = {int(arr[0])}: the first offset must be 0")
        down = np.nonzero(arr[1:] < arr[:-1])[0]
        if down.size:
            i = int(down[0]) + 1
            raise ValueError(f"offsets[{i}] = {int(arr[i])} is smaller than offsets[{i - 1}] = {int(arr[i - 1])}: offsets must not decrease")
        if int(arr[-1]) != npoints:
            raise ValueError(f"offsets[{arr.size - 1}] = {int(arr[-1])}: the last offset must equal the {npoints} points")
        if nscalars != npoints:
            raise ValueError(f"{npoints} points need {npoints} scalars, not {nscalars}")
        offs = np.ascontiguousarray(arr)
        nseg = arr.size - 1
    if out is not None:
        if not b.is_device:
            raise TypeError("out= goes with GPU tensors; host inputs return a new container")
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.is_contiguous() and out.numel() == nseg * out_stride):
            raise ValueError(f"out must be a contiguous GPU uint8 tensor of {nseg} * {out_stride} bytes")
    return b, sc, offs, nseg, npoints, nscalars, stride, out_stride


def msm_segments(points, scalars, offsets=None, curve="bls12_377_g1", shared: bool = False, montgomery: bool = False, projective: bool = False,
                 stride: Optional[int] = None, out_stride: Optional[int] = None, out=None, lengths=None, device: Optional[int] = None):
    """MultiScalarMultContext.msm_segments on a throwaway context (on the tensor's device for a GPU tensor); the arguments are judged
    before the context is made."""
    _segments_args(_curve_id(curve), points, scalars, offsets, lengths, shared, projective, stride, out_stride, out)
    return _throwaway(points, curve, device, lambda c: c.msm_segments(points, scalars, offsets, shared=shared, montgomery=montgomery, projective=projective,
                                                                     stride=stride, out_stride=out_stride, out=out, lengths=lengths))


def mul_points_by(points, k, curve="bls12_377_g1", projective: bool = False, stride: Optional[int] = None, out_stride: Optional[int] = None,
                  device: Optional[int] = None):
    """MultiScalarMultContext.mul_points_by on a throwaway context."""
    return _throwaway(points, curve, device, lambda c: c.mul_points_by(points, k, projective=projective, stride=stride, out_stride=out_stride))


def mul_by_cofactor(points, curve="bls12_377_g1", projective: bool = False, stride: Optional[int] = None, out_stride: Optional[int] = None,
                    device: Optional[int] = None):
    """MultiScalarMultContext.mul_by_cofactor on a throwaway context."""
    return _throwaway(points, curve, device, lambda c: c.mul_by_cofactor(points, projective=projective, stride=stride, out_stride=out_stride))


def multi_scalar_mult(ctx: MultiScalarMultContext, points, scalars) -> List[bytes]:
    """One 144-byte projective image per batch; ``points`` is only used for its length, as in the reference
    (``npoints = points.len()``, P1A 6block/src/lib.rs:92-101)."""
    npoints = ctx.npoints if points is None else _Buf(points).nbytes // affine_stride(ctx.curve)
    if npoints != ctx.npoints:
        raise MsmError(-1, f"context was initialised with {ctx.npoints} points, called with {npoints}")
    return ctx.run(scalars, npoints)


def msm(bases, scalars, curve="bls12_377_g1") -> bytes:
    """Stateless ``msm(bases, scalars, n)``; chops to the shorter input like VariableBaseMSM::msm."""
    stride = affine_stride(curve)
    nb = _Buf(bases).nbytes // stride
    ns = _Buf(scalars).nbytes // SCALAR_BYTES
    n = min(nb, ns)
    pb, sb = _Buf(bases), _Buf(scalars)
    if not (pb.is_device or sb.is_device):
        # both operands in host memory: the stateless C entry (a pipeline: slices cross PCIe while earlier ones compute)
        out = ctypes.create_string_buffer(projective_bytes(curve))
        _check(load_library().mi355_msm(_curve_id(curve), out, pb.ptr, n, sb.ptr, stride))
        return out.raw
    ctx = MultiScalarMultContext(curve)
    try:
        # chop BYTES, not rows: the inputs are usually 2-D (N, 104) / (N, 32) tensors
        ctx.set_bases(_flat_bytes(bases)[: n * stride])
        return ctx.run(_flat_bytes(scalars)[: n * SCALAR_BYTES], n)[0]
    finally:
        ctx.close()


def last_stateless() -> dict:
    """What this thread's most recent stateless ``msm`` call did (mi355_msm_last_stateless)."""
    v = (ctypes.c_double * 10)()
    _check(load_library().mi355_msm_last_stateless(v, 10))
    names = ("total_ms", "setup_ms", "wait_upload_ms", "compute_ms", "tail_ms", "slices", "threads", "bytes", "dma_done_ms", "first_dma_ms")
    return {k: float(v[i]) for i, k in enumerate(names)}


def trim() -> None:
    """Give back what the stateless entry points keep between calls (pinned rings, idle contexts): mi355_msm_trim."""
    _check(load_library().mi355_msm_trim())


def pool_stats() -> dict:
    """mi355_msm_pool_stats: idle contexts of the stateless path and the memory they hold."""
    v = (ctypes.c_uint64 * 4)()
    _check(load_library().mi355_msm_pool_stats(v, 4))
    return {"idle_contexts": int(v[0]), "idle_device_bytes": int(v[1]), "idle_rings": int(v[2]), "idle_pinned_bytes": int(v[3])}


class VariableBaseMSM:
    """Shape of the arkworks trait (ARK ec/src/msm/variable_base/mod.rs:15-65) for one curve."""

    def __init__(self, curve="bls12_377_g1"):
        self.curve = curve

    def msm(self, bases, scalars) -> bytes:
        return msm(bases, scalars, self.curve)

    def msm_checked(self, bases, scalars):
        """``Ok(point)`` as bytes, or ``Err(min_len)`` as an int when lengths differ."""
        nb = _Buf(bases).nbytes // affine_stride(self.curve)
        ns = _Buf(scalars).nbytes // SCALAR_BYTES
        if nb != ns:
            return min(nb, ns)
        return self.msm(bases, scalars)

    msm_bigint = msm

    def msm_chunks(self, bases_stream, scalars_stream, step: int = 1 << 20) -> bytes:
        """Streaming form (ARK ec/src/msm/variable_base/mod.rs:165-199): ``scalars_stream`` holds ``Fr`` values (Montgomery
        form, converted on the device like ``into_bigint``) and must not be longer than ``bases_stream``; the LAST
        ``len(scalars)`` bases are used ("align the streams"), ``step`` pairs at a time, and the partial sums are added.
        The reference hard-codes step = 2^20; any step gives the same point."""
        stride = affine_stride(self.curve)
        bases_stream, scalars_stream = _flat_bytes(bases_stream), _flat_bytes(scalars_stream)
        nb, ns = len(bases_stream) // stride, len(scalars_stream) // SCALAR_BYTES
        if ns > nb:
            raise MsmError(-1, f"msm_chunks: {ns} scalars for {nb} bases (scalars_stream.len() <= bases_stream.len())")
        if step <= 0:
            raise MsmError(-1, "msm_chunks: step must be positive")
        skip = nb - ns
        ctx = MultiScalarMultContext(self.curve)
        try:
            ctx.set_option("scalars_montgomery", 1)
            partials = []
            for lo in range(0, ns, step):
                hi = min(ns, lo + step)
                ctx.set_bases(bases_stream[(skip + lo) * stride:(skip + hi) * stride])
                partials.append(ctx.run(scalars_stream[lo * SCALAR_BYTES:hi * SCALAR_BYTES], hi - lo)[0])
            return fold_partials(partials, self.curve)
        finally:
            ctx.close()


class ChunkedPippenger:
    """``ChunkedPippenger::{new, with_size, add, finalize}`` (ARK ec/src/msm/variable_base/stream_pippenger.rs:11-75): buffer
    (base, BigInt scalar) pairs; every ``buf_size`` pairs ``result += msm_bigint(buffer)``; ``finalize`` flushes the rest.
    ``add`` takes one pair or arrays of pairs (byte images as everywhere in this module)."""

    _HASHMAP = 0

    def __init__(self, max_msm_buffer: int, curve="bls12_377_g1", device: Optional[int] = None):
        self.curve = _curve_id(curve)
        self._lib = load_library()
        self.stream = ctypes.c_void_p()
        _check(self._lib.mi355_msm_stream_create(ctypes.byref(self.stream), self.curve, -1 if device is None else device,
                                                 max_msm_buffer, self._HASHMAP))

    new = classmethod(lambda cls, max_msm_buffer, curve="bls12_377_g1": cls(max_msm_buffer, curve))
    with_size = new

    def set_option(self, key: str, value: int) -> None:
        _check(self._lib.mi355_msm_stream_set_option(self.stream, key.encode(), int(value)))

    def add(self, bases, scalars, stride: Optional[int] = None) -> None:
        stride = affine_stride(self.curve) if stride is None else stride
        b, s = _Buf(bases), _Buf(scalars)
        if b.is_device or s.is_device:
            raise TypeError("the streaming accumulators buffer pairs on the host: pass host arrays")
        if b.nbytes % stride or s.nbytes % SCALAR_BYTES or b.nbytes // stride != s.nbytes // SCALAR_BYTES:
            raise ValueError("bases and scalars must hold the same number of pairs")
        _check(self._lib.mi355_msm_stream_add(self.stream, b.ptr, stride, s.ptr, s.nbytes // SCALAR_BYTES))

    def finalize(self) -> bytes:
        out = ctypes.create_string_buffer(projective_bytes(self.curve))
        _check(self._lib.mi355_msm_stream_finalize(self.stream, out))
        return out.raw

    def query(self, key: str) -> int:
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_stream_query(self.stream, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.stream:
            _check(self._lib.mi355_msm_stream_destroy(self.stream))
            self.stream = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HashMapPippenger(ChunkedPippenger):
    """``HashMapPippenger::{new, add, finalize}`` (stream_pippenger.rs:78-140): a pair whose base is already buffered adds its
    scalar (an ``Fr`` value) to that entry modulo r; the MSM runs when ``max_msm_buffer`` DISTINCT bases are buffered."""

    _HASHMAP = 1


class WindowTable:
    """The window table of ONE base, resident on one GPU (mi355_msm_fixed_*): what ``FixedBase::get_window_table`` returns in arkworks
    (ARK ec/src/msm/fixed_base.rs:19-58), built on the device.  ``msm`` multiplies the base by every scalar of a batch."""

    def __init__(self, g, curve="bls12_377_g1", window: int = 0, device: Optional[int] = None, expected_scalars: int = 0):
        self.curve = _curve_id(curve)
        self.handle = ctypes.c_void_p()
        b = _Buf(g)
        if b.is_device:
            raise TypeError("the base is one Affine image in host memory")
        if b.nbytes != affine_stride(self.curve):
            raise ValueError(f"base image of {b.nbytes} bytes: one {affine_stride(self.curve)}-byte Affine image expected")
        self._lib = load_library()
        _check(self._lib.mi355_msm_fixed_create(ctypes.byref(self.handle), self.curve, -1 if device is None else device, b.ptr, int(window),
                                                int(expected_scalars)))
        self.device = self.query("device")

    def msm(self, scalars, montgomery: bool = False, projective: bool = False, stride: Optional[int] = None):
        """``out[i] = scalars[i] * g`` as arkworks Affine images (``projective``: normalised Projective images), ``stride`` bytes apart
        (default: the image size).  ``scalars``: 32-byte little-endian integers, all 256 bits significant; ``montgomery``: arkworks ``Fr``
        images, which is what ``FixedBase::msm`` takes.  bytes in, bytes out; a NumPy array or a torch CPU tensor gives an array /
        tensor of shape (n, stride); a torch GPU tensor is read in place and gives a GPU tensor, ready for ``set_bases``."""
        size = projective_bytes(self.curve) if projective else affine_stride(self.curve)
        stride = size if stride is None else int(stride)
        b = _Buf(scalars)
        if b.nbytes % SCALAR_BYTES:
            raise ValueError("scalars image is not a multiple of 32 bytes")
        if stride % 4 or stride < size:
            raise ValueError(f"stride {stride} must be a multiple of 4 and at least the {size}-byte image")
        if not self.handle:
            raise MsmError(-1, "the window table is closed")
        if b.is_device and b.device_index != self.device:
            raise MsmError(-1, f"scalars live on cuda:{b.device_index} but this table is bound to device {self.device}")
        n = b.nbytes // SCALAR_BYTES
        flags = (1 if montgomery else 0) | (2 if projective else 0)
        if b.is_device:
            import torch

            out = torch.zeros((n, stride), dtype=torch.uint8, device=b.keep.device)
            if n:
                _check(self._lib.mi355_msm_fixed_mul_device(self.handle, out.data_ptr(), stride, b.ptr, n, flags, b.stream))
            return out
        import numpy as np

        out = np.zeros((n, stride), dtype=np.uint8)
        if n:
            _check(self._lib.mi355_msm_fixed_mul(self.handle, out.ctypes.data, stride, b.ptr, n, flags))
        if hasattr(scalars, "data_ptr") and hasattr(scalars, "is_cuda"):
            import torch

            return torch.from_numpy(out)
        if hasattr(scalars, "__array_interface__"):
            return out
        return out.tobytes()

    def set_option(self, key: str, value: int) -> None:
        _check(self._lib.mi355_msm_fixed_set_option(self.handle, key.encode(), int(value)))

    def query(self, key: str) -> int:
        """ "window_bits", "levels", "table_bytes", "signed_digits", "build_us", "device", "last_mul_us", "last_device_us", "max_chunk", "work_bytes" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_fixed_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_fixed_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FR_MODULUS = {
    0: 8444461749428370424248824938781546531375899335154063827935233455917409239041,   # BLS12-377 Fr
    1: 52435875175126190479447740508185965837690552500527637822603658699938581184513,  # BLS12-381 Fr
}


class Radix2EvaluationDomain:
    """``Radix2EvaluationDomain::<Fr>::new(num_coeffs)`` (ARK poly/src/domain/radix2/mod.rs) on one GPU (mi355_msm_domain_*): the
    domain of the smallest power of two >= ``num_coeffs`` over the scalar field of ``curve``'s family.

    ``fft``, ``ifft``, ``coset_fft``, ``coset_ifft`` take vectors of 32-byte elements -- bytes, a NumPy array or a torch tensor of shape
    ``(n, 32)`` or ``(batch, n, 32)``; fewer than ``size`` elements per vector are zero-extended (single vectors only) -- and return
    the same kind of container; a torch GPU tensor is read in place on its current stream and gives a GPU tensor, which
    ``MultiScalarMultContext.run`` takes as it is under the option ``scalars_montgomery``.  ``montgomery=True`` (default): arkworks
    ``Fr`` images; ``False``: plain little-endian integers.  ``order``: "NN" (default), "NR" (forward: bit-reversed output) or "RN"
    (inverse: bit-reversed input).  ``offset``: the coset offset as an integer (default: the field's GENERATOR).  ``out``: a GPU
    tensor to write into (may be the input)."""

    FORWARD, INVERSE, COSET_FORWARD, COSET_INVERSE = 0, 1, 2, 3

    def __init__(self, num_coeffs: int, curve="bls12_377_g1", device: Optional[int] = None):
        self.curve = _curve_id(curve)
        self.modulus = FR_MODULUS[self.curve & 1]
        self.handle = ctypes.c_void_p()
        self._lib = load_library()
        if num_coeffs < 0 or num_coeffs >= 1 << 63:
            raise ValueError("num_coeffs out of range")
        _check(self._lib.mi355_msm_domain_create(ctypes.byref(self.handle), self.curve, -1 if device is None else device, int(num_coeffs)))
        self.size = self.query("size")
        self.log_size_of_group = self.query("log_size")
        self.device = self.query("device")

    def element(self, i: int) -> int:
        """omega^i as an integer"""
        out = ctypes.create_string_buffer(32)
        _check(self._lib.mi355_msm_domain_element(self.handle, int(i) % self.size, out))
        return int.from_bytes(out.raw, "little") * pow(1 << 256, -1, self.modulus) % self.modulus

    @property
    def group_gen(self) -> int:
        return self.element(1)

    @property
    def size_inv(self) -> int:
        return pow(self.size, -1, self.modulus)

    def _flags(self, kind, montgomery, order):
        flags = 0 if montgomery else 1
        if order == "NR":
            flags |= 2
        elif order == "RN":
            flags |= 4
        elif order != "NN":
            raise ValueError(f"order {order!r}: one of 'NN', 'NR', 'RN'")
        return flags

    def _offset(self, offset, montgomery):
        if offset is None:
            return None
        v = int(offset) % self.modulus
        return ((v << 256) % self.modulus if montgomery else v).to_bytes(32, "little")

    def _shape(self, src, nbytes):
        """(batch, in_len, result shape or None for bytes) of an input"""
        shape = getattr(src, "shape", None)
        if shape is not None and len(shape) == 3:
            if shape[2] != 32 or shape[1] != self.size:
                raise ValueError(f"a batch has shape (batch, {self.size}, 32), not {tuple(shape)}")
            return int(shape[0]), self.size, (int(shape[0]), self.size, 32)
        if nbytes % 32:
            raise ValueError("the input is not a multiple of 32 bytes")
        return 1, nbytes // 32, (self.size, 32)

    def _transform(self, kind, values, montgomery=True, order="NN", offset=None, out=None):
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        flags = self._flags(kind, montgomery, order)
        off = self._offset(offset, montgomery)
        b = _Buf(values)
        batch, in_len, shape = self._shape(values, b.nbytes)
        if b.is_device:
            import torch

            if b.device_index != self.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.device}")
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != batch * self.size * 32 or ob.keep is not out:
                raise ValueError(f"out must be a contiguous uint8 GPU tensor of {batch * self.size * 32} bytes")
            _check(self._lib.mi355_msm_domain_transform_device(self.handle, ob.ptr, b.ptr, in_len, batch, kind, flags, off, b.stream))
            return out
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros(batch * self.size * 32, dtype=np.uint8)
        _check(self._lib.mi355_msm_domain_transform(self.handle, res.ctypes.data, b.ptr, in_len, batch, kind, flags, off))
        return _like_input(values, res, shape)

    def fft(self, coeffs, **kw):
        return self._transform(self.FORWARD, coeffs, **kw)

    def ifft(self, evals, **kw):
        return self._transform(self.INVERSE, evals, **kw)

    def coset_fft(self, coeffs, **kw):
        return self._transform(self.COSET_FORWARD, coeffs, **kw)

    def coset_ifft(self, evals, **kw):
        return self._transform(self.COSET_INVERSE, evals, **kw)

    def mul(self, a, b, montgomery: bool = True, out=None):
        """``out[i] = a[i] * b[i]`` (mul_polynomials_in_evaluation_domain); any number of elements"""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        ba, bb = _Buf(a), _Buf(b)
        if ba.nbytes != bb.nbytes or ba.nbytes % 32 or ba.is_device != bb.is_device:
            raise ValueError("a and b must hold the same number of 32-byte elements, in the same kind of memory")
        n = ba.nbytes // 32
        flags = 0 if montgomery else 1
        if ba.is_device:
            import torch

            if out is None:
                out = torch.empty(tuple(a.shape), dtype=torch.uint8, device=ba.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != ba.nbytes or ob.keep is not out:
                raise ValueError("out must be a contiguous uint8 GPU tensor of the inputs' size")
            _check(self._lib.mi355_msm_domain_mul_device(self.handle, ob.ptr, ba.ptr, bb.ptr, n, flags, ba.stream))
            return out
        import numpy as np

        res = np.zeros(ba.nbytes, dtype=np.uint8)
        _check(self._lib.mi355_msm_domain_mul(self.handle, res.ctypes.data, ba.ptr, bb.ptr, n, flags))
        return _like_input(a, res, getattr(a, "shape", None) or (n, 32))

    # ---- between a transform and an MSM (mi355_msm_domain_batch_inverse .. _divide_by_vanishing_on_coset) -------------------------
    # Vectors are bytes, NumPy arrays or torch tensors of n 32-byte elements (any n; the Lagrange call alone is tied to ``size``); a
    # torch GPU tensor is read in place on its current stream and gives a GPU tensor (``out=`` as in ``mul``).  Scalars (``z``,
    # ``tau``, ``coeff``, ``s``, ``offset``) are Python integers and so are scalar results.

    def _scalar(self, v, montgomery):
        v = int(v) % self.modulus
        return ((v << 256) % self.modulus if montgomery else v).to_bytes(32, "little")

    def _scalar_out(self, raw, montgomery):
        v = int.from_bytes(raw, "little")
        return v * pow(1 << 256, -1, self.modulus) % self.modulus if montgomery else v

    def _vectors(self, *vs):
        """the buffers of same-sized inputs in one kind of memory, and their element count"""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        bufs = [_Buf(v) for v in vs]
        b0 = bufs[0]
        for b in bufs:
            if b.nbytes != b0.nbytes or b.nbytes % 32 or b.is_device != b0.is_device:
                raise ValueError("the vectors must hold the same number of 32-byte elements, in the same kind of memory")
            if b.is_device and b.device_index != self.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.device}")
        return bufs, b0.nbytes // 32

    def _out(self, src, b, out, n):
        """(result container, its _Buf) for n elements: a GPU tensor for GPU inputs, else a NumPy array"""
        if b.is_device:
            import torch

            if out is None:
                out = torch.empty((n, 32), dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != n * 32 or ob.keep is not out:
                raise ValueError(f"out must be a contiguous uint8 GPU tensor of {n * 32} bytes")
            return out, ob
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros(max(n, 1) * 32, dtype=np.uint8)[:n * 32]
        return res, _Buf(res)

    def _map(self, name, src, b, n, out, tail, shape=None):
        """one vector in, one vector out: name(handle, out, in, n, *tail[, stream])"""
        res, ob = self._out(src, b, out, n)
        if b.is_device:
            _check(getattr(self._lib, name + "_device")(self.handle, ob.ptr, b.ptr, n, *tail, b.stream))
            return res
        _check(getattr(self._lib, name)(self.handle, ob.ptr, b.ptr, n, *tail))
        return _like_input(src, res, shape or (n, 32))

    def batch_inversion_and_mul(self, v, coeff=None, montgomery: bool = True, out=None):
        """``out[i] = coeff / v[i]`` (``coeff`` None: 1); elements that are zero stay zero, as arkworks skips them.  ``out`` may be ``v``."""
        (b,), n = self._vectors(v)
        c = None if coeff is None else self._scalar(coeff, montgomery)
        return self._map("mi355_msm_domain_batch_inverse", v, b, n, out, (c, 0 if montgomery else 1))

    def batch_inversion(self, v, montgomery: bool = True, out=None):
        return self.batch_inversion_and_mul(v, None, montgomery=montgomery, out=out)

    ADD, SUB, MUL_SUB, SCALE = 0, 1, 2, 3

    def _vec_op(self, op, a, b, c, montgomery, out):
        flags = 0 if montgomery else 1
        if op == self.SCALE:
            (ba,), n = self._vectors(a)
            ptrs = (self._scalar(b, montgomery), None)
        elif op == self.MUL_SUB:
            (ba, bb, bc), n = self._vectors(a, b, c)
            ptrs = (bb.ptr, bc.ptr)
        else:
            (ba, bb), n = self._vectors(a, b)
            ptrs = (bb.ptr, None)
        res, ob = self._out(a, ba, out, n)
        if ba.is_device:
            _check(self._lib.mi355_msm_domain_vec_op_device(self.handle, ob.ptr, ba.ptr, ptrs[0], ptrs[1], n, op, flags, ba.stream))
            return res
        _check(self._lib.mi355_msm_domain_vec_op(self.handle, ob.ptr, ba.ptr, ptrs[0], ptrs[1], n, op, flags))
        return _like_input(a, res, (n, 32))

    def add(self, a, b, montgomery: bool = True, out=None):
        """``a[i] + b[i]``; ``out`` may be any input"""
        return self._vec_op(self.ADD, a, b, None, montgomery, out)

    def sub(self, a, b, montgomery: bool = True, out=None):
        """``a[i] - b[i]``"""
        return self._vec_op(self.SUB, a, b, None, montgomery, out)

    def mul_sub(self, a, b, c, montgomery: bool = True, out=None):
        """``a[i] * b[i] - c[i]``: the numerator of the quotient polynomial"""
        return self._vec_op(self.MUL_SUB, a, b, c, montgomery, out)

    def scale(self, a, s: int, montgomery: bool = True, out=None):
        """``s * a[i]`` for one integer ``s``"""
        return self._vec_op(self.SCALE, a, s, None, montgomery, out)

    def evaluate(self, coeffs, z: int, montgomery: bool = True) -> int:
        """``DensePolynomial::evaluate``: ``sum coeffs[i] z^i`` as an integer"""
        (b,), n = self._vectors(coeffs)
        res = ctypes.create_string_buffer(32)
        zz, flags = self._scalar(z, montgomery), 0 if montgomery else 1
        if b.is_device:
            _check(self._lib.mi355_msm_domain_evaluate_device(self.handle, res, b.ptr, n, zz, flags, b.stream))
        else:
            _check(self._lib.mi355_msm_domain_evaluate(self.handle, res, b.ptr, n, zz, flags))
        return self._scalar_out(res.raw, montgomery)

    def divide_by_linear(self, coeffs, z: int, montgomery: bool = True, out=None):
        """``(p - p(z)) / (X - z)`` and ``p(z)``: (the n - 1 quotient coefficients, the remainder as an integer).  ``out`` must not
        overlap ``coeffs``."""
        (b,), n = self._vectors(coeffs)
        qn = max(n - 1, 0)
        q, qb = self._out(coeffs, b, out, qn)
        rem = ctypes.create_string_buffer(32)
        zz, flags = self._scalar(z, montgomery), 0 if montgomery else 1
        if b.is_device:
            _check(self._lib.mi355_msm_domain_divide_by_linear_device(self.handle, qb.ptr if qn else None, rem, b.ptr, n, zz, flags, b.stream))
        else:
            _check(self._lib.mi355_msm_domain_divide_by_linear(self.handle, qb.ptr if qn else None, rem, b.ptr, n, zz, flags))
            q = _like_input(coeffs, q, (qn, 32))
        return q, self._scalar_out(rem.raw, montgomery)

    def evaluate_all_lagrange_coefficients(self, tau: int, montgomery: bool = True, out=None, device: bool = False):
        """the ``size`` values ``L_i(tau)``; ``tau`` in the domain gives the unit vector.  A NumPy array, or with ``out=`` / ``device=True``
        a GPU tensor written on the current stream."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        t, flags = self._scalar(tau, montgomery), 0 if montgomery else 1
        if out is not None or device:
            import torch

            if out is None:
                out = torch.empty((self.size, 32), dtype=torch.uint8, device=torch.device("cuda", self.device))
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != self.size * 32 or ob.keep is not out or ob.device_index != self.device:
                raise ValueError(f"out must be a contiguous uint8 tensor of {self.size * 32} bytes on cuda:{self.device}")
            _check(self._lib.mi355_msm_domain_lagrange_device(self.handle, ob.ptr, t, flags, ob.stream))
            return out
        import numpy as np

        res = np.zeros((self.size, 32), dtype=np.uint8)
        _check(self._lib.mi355_msm_domain_lagrange(self.handle, res.ctypes.data, t, flags))
        return res

    def evaluate_vanishing_polynomial(self, tau: int) -> int:
        """``tau^size - 1`` (host arithmetic)"""
        res = ctypes.create_string_buffer(32)
        _check(self._lib.mi355_msm_domain_vanishing(self.handle, res, self._scalar(tau, False), 1))
        return int.from_bytes(res.raw, "little")

    def divide_by_vanishing_poly_on_coset(self, evals, offset=None, montgomery: bool = True, out=None):
        """``evals[i] / (g^size - 1)`` for the coset offset ``g`` (default: GENERATOR); ``out`` may be ``evals``"""
        (b,), n = self._vectors(evals)
        off = None if offset is None else self._scalar(offset, montgomery)
        return self._map("mi355_msm_domain_divide_by_vanishing_on_coset", evals, b, n, out, (off, 0 if montgomery else 1))

    # ---- prefix scans and the permutation product (mi355_msm_domain_scan, _permutation_product) -------------------------------------

    PRODUCT, SUM = 0, 1

    def _scan(self, op, v, inclusive, montgomery, out):
        (b,), n = self._vectors(v)
        res, ob = self._out(v, b, out, n)
        tot = ctypes.create_string_buffer(32)
        flags = (0 if montgomery else 1) | (2 if inclusive else 0)
        if b.is_device:
            _check(self._lib.mi355_msm_domain_scan_device(self.handle, ob.ptr, tot, b.ptr, n, op, flags, b.stream))
        else:
            _check(self._lib.mi355_msm_domain_scan(self.handle, ob.ptr, tot, b.ptr, n, op, flags))
            res = _like_input(v, res, (n, 32))
        return res, self._scalar_out(tot.raw, montgomery)

    def prefix_product(self, v, inclusive: bool = False, montgomery: bool = True, out=None):
        """(the running product, the product of all of ``v`` as an integer).  Exclusive by default -- ``out[0] = 1``,
        ``out[i] = v[0] * .. * v[i-1]``, what a grand product wants; ``inclusive=True``: ``out[i] = v[0] * .. * v[i]``.  Zeros are NOT
        skipped (unlike ``batch_inversion``): after a zero every later product is zero.  ``out`` may be ``v``."""
        return self._scan(self.PRODUCT, v, inclusive, montgomery, out)

    def prefix_sum(self, v, inclusive: bool = False, montgomery: bool = True, out=None):
        """(the running sum, the sum of all of ``v`` as an integer): ``out[0] = 0``, ``out[i] = v[0] + .. + v[i-1]``, or with
        ``inclusive=True`` up to ``v[i]``.  ``out`` may be ``v``."""
        return self._scan(self.SUM, v, inclusive, montgomery, out)

    def _columns(self, cols, what, most: int = 8, strided: bool = False):
        """(buffer, m, stride in elements) of the m columns of ``size`` elements: a (m, size, 32) array or tensor, or a list of m
        vectors; ``strided``: an array or tensor may hold its columns further apart, (m, stride, 32) with ``stride >= size``"""
        if isinstance(cols, (list, tuple)):
            first = cols[0] if len(cols) else None
            if hasattr(first, "is_cuda") and hasattr(first, "data_ptr"):
                import torch

                cols = torch.stack([c.reshape(-1, 32) for c in cols])
            else:
                import numpy as np

                cols = np.stack([np.frombuffer(_flat_bytes(c), dtype=np.uint8).reshape(-1, 32) for c in cols]) if len(cols) else np.zeros((0, self.size, 32), np.uint8)
        shape = tuple(getattr(cols, "shape", ()))
        if len(shape) != 3 or shape[2] != 32 or not 1 <= shape[0] <= most or (shape[1] < self.size if strided else shape[1] != self.size):
            raise ValueError(f"{what}: m columns (1 <= m <= {most}) of {self.size} 32-byte elements, shape (m, {self.size}, 32), not {shape}")
        return _Buf(cols), int(shape[0]), int(shape[1])

    def permutation_product(self, wires, sigmas, beta: int, gamma: int, ks, montgomery: bool = True, out=None):
        """The Plonk permutation grand product over the ``size`` rows of the domain: ``z[0] = 1``,
        ``z[j+1] = z[j] * prod_i (w_i[j] + beta ks[i] omega^j + gamma) / prod_i (w_i[j] + beta sigma_i[j] + gamma)``.  Returns
        ``(z, total)``: the ``size`` values of ``z`` (ready for ``ifft``) and ``total = z[size-1] * f[size-1]`` as an integer, which is 1
        exactly when the copy constraints hold.  ``wires`` and ``sigmas``: a ``(m, size, 32)`` array or tensor, or a list of ``m``
        vectors; ``ks``: the ``m`` coset representatives as integers.  A zero denominator does not raise: that row's factor is 0 and
        so are all later values of ``z`` and ``total``.  ``out`` must not overlap the inputs."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        bw, m, stride = self._columns(wires, "wires")
        bs, ms, _ = self._columns(sigmas, "sigmas")
        ks = [int(k) for k in ks]
        if ms != m or len(ks) != m or bw.is_device != bs.is_device:
            raise ValueError("wires, sigmas and ks must agree in the number of columns, and wires and sigmas in the kind of memory")
        for b in (bw, bs):
            if b.is_device and b.device_index != self.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.device}")
        res, ob = self._out(wires, bw, out, self.size)
        tot = ctypes.create_string_buffer(32)
        kb = b"".join(self._scalar(k, montgomery) for k in ks)
        bb, gb, flags = self._scalar(beta, montgomery), self._scalar(gamma, montgomery), 0 if montgomery else 1
        if bw.is_device:
            _check(self._lib.mi355_msm_domain_permutation_product_device(self.handle, ob.ptr, tot, bw.ptr, bs.ptr, m, stride, kb, bb, gb, flags, bw.stream))
        else:
            _check(self._lib.mi355_msm_domain_permutation_product(self.handle, ob.ptr, tot, bw.ptr, bs.ptr, m, stride, kb, bb, gb, flags))
            res = res.reshape(self.size, 32) if isinstance(wires, (list, tuple)) else _like_input(wires, res, (self.size, 32))
        return res, self._scalar_out(tot.raw, montgomery)

    # ---- the rows of the Plonk quotient and linear combinations (mi355_msm_domain_plonk_quotient, _linear_combination) -------------

    def plonk_quotient(self, wires, sigmas, z, alpha: int, beta: int, gamma: int, ks, n: int, selectors=None, pi=None, offset=None,
                       montgomery: bool = True, out=None):
        """The row loop of a TurboPlonk prover's third round on THIS domain as the quotient domain (``size = M``): all vectors hold the
        ``M`` evaluations on ``offset * H_M`` that ``coset_fft`` writes, ``n`` is the size of the constraint domain (``M / n`` in 2, 4,
        8, 16).  With ``x = offset * omega^i``::

            gate    = q_c + pi + sum_j q_lc[j] w_j + q_mul[0] w0 w1 + q_mul[1] w2 w3 + q_ecc w0 w1 w2 w3 w4 + sum_j q_hash[j] w_j^5 - q_o w4
            out[i]  = (gate + alpha (z[i] prod_j (w_j + beta ks[j] x + gamma) - z[i + M/n] prod_j (w_j + beta sigma_j + gamma))) / (x^n - 1)
                      + alpha^2 (z[i] - 1) / (n (x - 1))

        ``wires`` and ``sigmas``: ``(m, stride, 32)`` arrays or tensors with ``stride >= M``, or lists of ``m`` vectors; ``selectors``:
        the same with the 13 columns ``q_lc[0..3], q_mul[0..1], q_hash[0..3], q_o, q_c, q_ecc`` (then ``m == 5``), or None: the gate
        is ``pi`` alone (``1 <= m <= 8``), for a prover that brings its own gate evaluations.  ``pi`` None: 0.  ``offset`` None: the
        field's GENERATOR; one whose ``n``-th power is a ``M/n``-th root of unity is refused.  ``out`` must not overlap any input.
        Returns the ``M`` values, ready for ``coset_ifft``."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        bw, m, stride = self._columns(wires, "wires", strided=True)
        bs, ms, sstride = self._columns(sigmas, "sigmas", strided=True)
        ks = [int(k) for k in ks]
        if ms != m or len(ks) != m or sstride != stride:
            raise ValueError("wires, sigmas and ks must agree in the number of columns, and wires and sigmas in the stride")
        bufs = [bw, bs]
        bq = None
        if selectors is not None:
            bq, mq, qstride = self._columns(selectors, "selectors", most=13, strided=True)
            if mq != 13 or m != 5 or qstride != stride:
                raise ValueError("selectors: 13 columns with the stride of the wires, beside 5 columns of wires")
            bufs.append(bq)
        (bz,), nz = self._vectors(z)
        bp = None
        if pi is not None:
            (bp,), npi = self._vectors(pi)
            if npi != nz:
                raise ValueError("z and pi must hold the same number of 32-byte elements")
            bufs.append(bp)
        if nz != self.size:
            raise ValueError(f"z: {self.size} 32-byte elements, not {nz}")
        for b in bufs:
            if b.is_device != bz.is_device:
                raise ValueError("all vectors must live in the same kind of memory")
            if b.is_device and b.device_index != self.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.device}")
        res, ob = self._out(z, bz, out, self.size)
        kb = b"".join(self._scalar(k, montgomery) for k in ks)
        ab, bb, gb = (self._scalar(v, montgomery) for v in (alpha, beta, gamma))
        off, flags = self._offset(offset, montgomery), 0 if montgomery else 1
        ptrs = (ob.ptr, bw.ptr, bs.ptr, bq.ptr if bq else None, bz.ptr, bp.ptr if bp else None)
        if bz.is_device:
            _check(self._lib.mi355_msm_domain_plonk_quotient_device(self.handle, *ptrs, m, stride, int(n), kb, ab, bb, gb, off, flags, bz.stream))
            return res
        _check(self._lib.mi355_msm_domain_plonk_quotient(self.handle, *ptrs, m, stride, int(n), kb, ab, bb, gb, off, flags))
        return _like_input(z, res, (self.size, 32))

    def linear_combination(self, cols, coeffs, montgomery: bool = True, out=None):
        """``out[i] = sum_j coeffs[j] * cols[j][i]`` for ``i < max(len(cols[j]))``: a list of 1 .. 32 vectors of any lengths (a vector
        contributes 0 past its end) and as many integers -- a linearisation or a batched opening polynomial in one pass.  ``out`` may
        be one of the vectors (the longest).  The length has nothing to do with the domain's size."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        cols, coeffs = list(cols), [int(c) for c in coeffs]
        if not 1 <= len(cols) <= 32 or len(coeffs) != len(cols):
            raise ValueError("cols: 1 .. 32 columns, and as many coefficients")
        bufs = [_Buf(c) for c in cols]
        for b in bufs:
            if b.nbytes % 32 or b.is_device != bufs[0].is_device:
                raise ValueError("the vectors must hold 32-byte elements, in the same kind of memory")
            if b.is_device and b.device_index != self.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.device}")
        m = len(bufs)
        lens = [b.nbytes // 32 for b in bufs]
        n = max(lens)
        first = bufs[lens.index(n)]
        res, ob = self._out(cols[lens.index(n)], first, out, n)
        ptrs = (ctypes.c_void_p * m)(*[b.ptr if ln else None for b, ln in zip(bufs, lens)])
        lv = (ctypes.c_size_t * m)(*lens)
        cb = b"".join(self._scalar(c, montgomery) for c in coeffs)
        flags = 0 if montgomery else 1
        if first.is_device:
            _check(self._lib.mi355_msm_domain_linear_combination_device(self.handle, ob.ptr if n else None, ptrs, lv, cb, m, flags, first.stream))
            return res
        _check(self._lib.mi355_msm_domain_linear_combination(self.handle, ob.ptr if n else None, ptrs, lv, cb, m, flags))
        return _like_input(cols[lens.index(n)], res, (n, 32))

    def compile_expression(self, expr, ncols: int):
        """An ``Expr`` over ``ncols`` columns, compiled once for this domain's field and device into a ``GateProgram``: one launch of
        ``prog.run(cols, ...)`` then evaluates it for every row, reading each column where it lies.  Raises ``MsmError`` when the
        expression needs more slots than the kernel has (the message names ``S`` and the limit): split the sum over an output column."""
        return GateProgram(self, expr, ncols)

    # ---- dense multilinear extensions and sumcheck prover rounds (mi355_msm_domain_mle_*, _sumcheck_round) --------------------------

    def _point(self, point, montgomery):
        pts = [int(x) for x in point]
        return pts, b"".join(self._scalar(x, montgomery) for x in pts)

    def _table(self, evals, what="evals"):
        """(the buffer of a table of 2^nv 32-byte elements, nv)"""
        (b,), n = self._vectors(evals)
        if n < 1 or n & (n - 1):
            raise ValueError(f"{what}: a table holds 2^num_vars 32-byte elements, not {n}")
        return b, n.bit_length() - 1

    def _mle_fix(self, evals, point, montgomery, out):
        b, nv = self._table(evals)
        pts, raw = self._point(point, montgomery)
        if len(pts) > nv:
            raise ValueError(f"point: {len(pts)} values for a table of {nv} variables")
        n_out = 1 << (nv - len(pts))
        res, ob = self._out(evals, b, out, n_out)
        flags = (0 if montgomery else 1) | (2 if b.is_device else 0)
        _check(self._lib.mi355_msm_domain_mle_fix(self.handle, ob.ptr, b.ptr, nv, raw if pts else None, len(pts), flags, b.stream if b.is_device else None))
        return res, b.is_device, n_out

    def mle_fix_variables(self, evals, point, montgomery: bool = True, out=None):
        """``DenseMultilinearExtension::fix_variables``: ``evals`` is a table of ``2^nv`` elements, index ``b`` standing for the point
        ``(b_0, .., b_{nv-1})`` with ``b_0`` the lowest bit; ``point`` (integers) fixes ``x_1 .. x_k`` from the lowest bit upward and the
        result holds ``2^(nv - k)`` canonical elements.  ``out`` must not overlap ``evals``.  GPU tensors are read in place on their
        current stream and give a GPU tensor."""
        res, dev, n_out = self._mle_fix(evals, point, montgomery, out)
        return res if dev else _like_input(evals, res, (n_out, 32))

    def mle_evaluate(self, evals, point, montgomery: bool = True) -> int:
        """``DenseMultilinearExtension::evaluate``: the value at ``point`` (``nv`` integers) as an integer"""
        res, dev, n_out = self._mle_fix(evals, point, montgomery, None)
        if n_out != 1:
            raise ValueError(f"point: {len(point)} values do not fix every variable of the table")
        return self._scalar_out(res.cpu().numpy().tobytes() if dev else res.tobytes(), montgomery)

    def eq_table(self, point, montgomery: bool = True, out=None, device: bool = False):
        """the ``2^k`` values ``eq(b, point) = prod_i (b_i ? point[i] : 1 - point[i])``.  A NumPy array ``(2^k, 32)``, or with ``out=`` /
        ``device=True`` a GPU tensor written on the current stream."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        pts, raw = self._point(point, montgomery)
        n, flags = 1 << len(pts), 0 if montgomery else 1
        if out is not None or device:
            import torch

            if out is None:
                out = torch.empty((n, 32), dtype=torch.uint8, device=torch.device("cuda", self.device))
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != n * 32 or ob.keep is not out or ob.device_index != self.device:
                raise ValueError(f"out must be a contiguous uint8 tensor of {n * 32} bytes on cuda:{self.device}")
            _check(self._lib.mi355_msm_domain_mle_eq(self.handle, ob.ptr, raw if pts else None, len(pts), flags | 2, ob.stream))
            return out
        import numpy as np

        res = np.zeros((n, 32), dtype=np.uint8)
        _check(self._lib.mi355_msm_domain_mle_eq(self.handle, res.ctypes.data, raw if pts else None, len(pts), flags, None))
        return res

    def _terms(self, terms, montgomery):
        recs, d = [], 0
        for coeff, factors in terms:
            fs = [int(f) for f in factors]
            if len(fs) > 5 or any(f < 0 or f >= 1 << 32 for f in fs):
                raise ValueError("a term takes at most 5 factor indices, each a table index")
            recs.append(self._scalar(coeff, montgomery) + len(fs).to_bytes(4, "little") + b"".join(f.to_bytes(4, "little") for f in fs + [0] * (5 - len(fs))))
            d = max(d, len(fs))
        return b"".join(recs), len(recs), d

    def sumcheck_round(self, tables, terms, r_prev=None, montgomery: bool = True, out=None):
        """One prover round of the sumcheck protocol for ``g = sum_j c_j prod_{k in S_j} f_k``: ``tables`` is a list of ``m <= 12``
        tables of ``2^nv`` elements, ``terms`` a list of ``(c_j, [table indices])`` with at most 8 terms of at most 5 factors (a repeated
        index is a power).  Returns the ``d + 1`` integers ``P(t) = sum_b sum_j c_j prod_k (f_k[2b] + t (f_k[2b+1] - f_k[2b]))``,
        ``t = 0 .. d``.  With ``r_prev`` the call first fixes ``x_1 = r_prev`` in every table, in the same pass, and returns
        ``(evals, folded)``: the evaluations of the folded tables and the list of the ``m`` folded tables (``out=``: a list of ``m``
        GPU tensors of ``2^(nv - 1)`` elements to write them into; none may overlap a table)."""
        tables = list(tables)
        bufs, n = self._vectors(*tables)
        if n < 2 or n & (n - 1):
            raise ValueError(f"tables: each holds 2^num_vars >= 2 32-byte elements, not {n}")
        nv, m, dev = n.bit_length() - 1, len(bufs), bufs[0].is_device
        recs, n_terms, d = self._terms(terms, montgomery)
        flags = (0 if montgomery else 1) | (2 if dev else 0)
        ptrs = (ctypes.c_void_p * m)(*[b.ptr for b in bufs])
        evals = ctypes.create_string_buffer(32 * 6)
        stream = bufs[0].stream if dev else None
        if r_prev is None:
            if out is not None:
                raise ValueError("out= goes with r_prev")
            _check(self._lib.mi355_msm_domain_sumcheck_round(self.handle, evals, ptrs, m, nv, recs, n_terms, None, None, flags, stream))
            return [self._scalar_out(evals.raw[32 * t:32 * t + 32], montgomery) for t in range(d + 1)]
        outs = list(out) if out is not None else [None] * m
        if len(outs) != m:
            raise ValueError(f"out: one tensor per table, {m}")
        made = [self._out(tables[i], bufs[i], outs[i], n // 2) for i in range(m)]
        fptrs = (ctypes.c_void_p * m)(*[ob.ptr for _, ob in made])
        _check(self._lib.mi355_msm_domain_sumcheck_round(self.handle, evals, ptrs, m, nv, recs, n_terms, self._scalar(r_prev, montgomery), fptrs, flags, stream))
        folded = [res if dev else _like_input(tables[i], res, (n // 2, 32)) for i, (res, _) in enumerate(made)]
        return [self._scalar_out(evals.raw[32 * t:32 * t + 32], montgomery) for t in range(d + 1)], folded

    def sumcheck_prove(self, tables, terms, challenge, montgomery: bool = True):
        """The prover of the sumcheck protocol over ``nv`` rounds; Fiat-Shamir is the caller's: ``challenge(i, evals) -> int`` gets the
        round index and the round's ``d + 1`` evaluations and returns ``r_i``.  The first round is plain, every later one fused with the
        fold by the previous challenge, ping-ponging between two sets of buffers whose sizes halve; the caller's tables are not modified.
        Returns ``(rounds, point, finals)``: the evaluations of every round, the point ``(r_0, .., r_{nv-1})`` and the ``m`` values
        ``f_k(point)``."""
        tables = list(tables)
        bufs, n = self._vectors(*tables)
        if n < 2 or n & (n - 1):
            raise ValueError(f"tables: each holds 2^num_vars >= 2 32-byte elements, not {n}")
        nv, m, dev = n.bit_length() - 1, len(bufs), bufs[0].is_device
        sets = [None, None]
        if dev and nv >= 2:
            import torch

            sets = [[torch.empty((n >> (1 + j), 32), dtype=torch.uint8, device=bufs[0].keep.device) for _ in range(m)] for j in range(2 if nv >= 3 else 1)] + [None]
        ev = self.sumcheck_round(tables, terms, montgomery=montgomery)
        rounds, point, cur = [ev], [int(challenge(0, ev))], tables
        for i in range(1, nv):
            outs = [t[:n >> i] for t in sets[(i - 1) & 1]] if dev else None
            ev, cur = self.sumcheck_round(cur, terms, r_prev=point[-1], montgomery=montgomery, out=outs)
            rounds.append(ev)
            point.append(int(challenge(i, ev)))
        finals = [self.mle_evaluate(t, [point[-1]], montgomery=montgomery) for t in cur]
        return rounds, point, finals

    # ---- resident sparse matrices and Groth16's witness map (mi355_msm_sparse_*) -----------------------------------------------------

    def sparse_matrix(self, rows, cols, row_ptr, col_idx, values, montgomery: bool = True) -> "SparseMatrix":
        """A CSR matrix over this domain's field, uploaded once and kept on this domain's device: ``row_ptr`` (``rows + 1`` offsets) and
        ``col_idx`` (``nnz`` indices) as integer arrays (NumPy, torch CPU, or bytes of little-endian uint64 / uint32), ``values`` as
        ``nnz`` 32-byte elements (bytes, NumPy or torch CPU).  Duplicate columns in a row are summed.  The domain must outlive the
        matrix; the matrix keeps a reference to it."""
        return SparseMatrix(self, rows, cols, row_ptr, col_idx, values, montgomery=montgomery)

    def groth16_witness_map(self, A, B, z, num_inputs, montgomery: bool = True):
        """ark-groth16's ``LibsnarkReduction::witness_map`` from the full assignment ``z`` to the ``size`` coefficients of ``h``, with the
        R1CS matrices ``A`` and ``B`` as ``SparseMatrix`` on this domain: ``a = A z`` with ``z[0 .. num_inputs)`` appended at rows
        ``n .. n + num_inputs`` (``n = A.rows`` constraints), ``b = B z``, ``c = a * b`` element by element, all zero-padded to ``size``;
        ``h = coset_ifft((coset_fft(ifft(a)) * coset_fft(ifft(b)) - coset_fft(ifft(c))) / Z(g))``.  With a GPU tensor in, every step
        runs on the tensor's current stream and the result is a GPU tensor; nothing but ``z`` comes from the host and nothing goes back.
        ``h[:size - 1]`` (the last coefficient is 0) is what ``MultiScalarMultContext.run`` takes as it is over ``h_query`` when the
        context reads the form this call wrote: arkworks images (``montgomery=True``, the default here) need the context's option
        ``scalars_montgomery`` set to 1 -- a new context has it at 0 and would read the images as plain integers, a wrong point and no
        error --, plain integers (``montgomery=False``) need it at 0.  tests/test_gpu_groth16.py proves whole proofs in both forms."""
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        n, ni = int(A.rows), int(num_inputs)
        if B.rows != n or A.cols != B.cols:
            raise ValueError(f"A is {A.rows} x {A.cols} and B is {B.rows} x {B.cols}: the two matrices must agree in shape")
        if ni < 0 or ni > A.cols or n + ni > self.size:
            raise ValueError(f"{n} constraints and {ni} inputs do not fit a domain of {self.size} points (or exceed the {A.cols} variables)")
        if not (hasattr(z, "data_ptr") and hasattr(z, "is_cuda") and z.is_cuda):
            import numpy as np

            z = np.frombuffer(_flat_bytes(z), dtype=np.uint8)
            if z.size != A.cols * 32:
                raise ValueError(f"z: {A.cols} 32-byte elements, shape ({A.cols}, 32)")
            z = z.reshape(A.cols, 32)
            a = np.zeros((self.size, 32), dtype=np.uint8)
            b = np.zeros((self.size, 32), dtype=np.uint8)
            a[:n] = A.apply(z, montgomery=montgomery)
            b[:n] = B.apply(z, montgomery=montgomery)
        else:
            import torch

            if tuple(z.shape) != (A.cols, 32):
                raise ValueError(f"z: {A.cols} 32-byte elements, shape ({A.cols}, 32), not {tuple(z.shape)}")
            z = z.contiguous()
            a = torch.zeros((self.size, 32), dtype=torch.uint8, device=z.device)
            b = torch.zeros((self.size, 32), dtype=torch.uint8, device=z.device)
            A.apply(z, montgomery=montgomery, out=a[:n])
            B.apply(z, montgomery=montgomery, out=b[:n])
        a[n:n + ni] = z[:ni]
        kw = dict(montgomery=montgomery)
        c = self.mul(a, b, **kw)
        ea, eb, ec = (self.coset_fft(self.ifft(v, **kw), **kw) for v in (a, b, c))
        h = self.mul_sub(ea, eb, ec, **kw)
        h = self.divide_by_vanishing_poly_on_coset(h, **kw)
        return self.coset_ifft(h, **kw)

    # ---- lookup arguments: resident tables and the logUp running sum (mi355_msm_lookup_*, mi355_msm_domain_logup_sum) ----------------

    def logup_sum(self, table, mult, values, beta: int, helpers: bool = False, montgomery: bool = True, out=None):
        """The logUp running sum over ``n`` rows (any ``n``, not the domain's size): with
        ``term[j] = sum_c 1 / (beta + values_c[j]) - mult[j] / (beta + table[j])``, ``phi[0] = 0`` and ``phi[j+1] = phi[j] + term[j]``.
        Returns ``(phi, total)``, or ``(phi, total, helper_columns)`` with ``helpers=True``: ``total = phi[n-1] + term[n-1]`` as an
        integer, 0 exactly when the multiset relation holds; the helper columns are the ``m`` columns ``1 / (beta + values_c[j])``
        and then ``mult[j] / (beta + table[j])``, shape ``(m + 1, n, 32)`` -- what sumcheck-based logUp commits to instead of ``phi``.
        ``table`` and ``mult`` hold ``n`` elements (``mult`` as ``LookupTable.multiplicities`` returns it); ``values`` is one vector
        of ``n``, a list of ``m <= 8`` vectors or a ``(m, n, 32)`` array or tensor.  A zero denominator does not raise: that term is 0.
        GPU tensors in give GPU tensors out on the current stream.

        Tuple lookups compress their columns on both sides first, with one random ``zeta``::

            f = dom.linear_combination([a, b, c], [1, zeta, zeta * zeta % r])
            t = dom.linear_combination([ta, tb, tc], [1, zeta, zeta * zeta % r])
            lt = ea.LookupTable(dom, t)
            mult, missing, first_missing = lt.multiplicities(f)
            phi, total = dom.logup_sum(t, mult, f, beta)      # total == 0
        """
        if not self.handle:
            raise MsmError(-1, "the domain is closed")
        (bt, bm), n = self._vectors(table, mult)
        if isinstance(values, (list, tuple)) or len(getattr(values, "shape", ())) == 3:
            if isinstance(values, (list, tuple)):
                first = values[0] if len(values) else None
                if hasattr(first, "is_cuda") and hasattr(first, "data_ptr"):
                    import torch

                    values = torch.stack([c.reshape(-1, 32) for c in values])
                else:
                    import numpy as np

                    values = np.stack([np.frombuffer(_flat_bytes(c), dtype=np.uint8).reshape(-1, 32) for c in values]) if len(values) else np.zeros((0, n, 32), np.uint8)
            shape = tuple(values.shape)
            if len(shape) != 3 or shape[2] != 32 or not 1 <= shape[0] <= 8 or shape[1] < n:
                raise ValueError(f"values: m columns (1 <= m <= 8) of {n} 32-byte elements, shape (m, {n}, 32), not {shape}")
            bv, m, stride = _Buf(values), int(shape[0]), int(shape[1])
        else:
            bv, m, stride = _Buf(values), 1, n
            if bv.nbytes != n * 32:
                raise ValueError(f"values: {n} 32-byte elements beside a table of {n}, not {bv.nbytes} bytes")
        if bv.is_device != bt.is_device:
            raise ValueError("table, mult and values must live in the same kind of memory")
        if bv.is_device and bv.device_index != self.device:
            raise MsmError(-1, f"the input lives on cuda:{bv.device_index} but this domain is bound to device {self.device}")
        res, ob = self._out(table, bt, out, n)
        tot = ctypes.create_string_buffer(32)
        flags = 0 if montgomery else 1
        hres = hb = None
        if helpers:
            if bt.is_device:
                import torch

                hres = torch.empty((m + 1, n, 32), dtype=torch.uint8, device=bt.keep.device)
            else:
                import numpy as np

                hres = np.zeros((m + 1, n, 32), dtype=np.uint8)
            hb = _Buf(hres)
        _check(self._lib.mi355_msm_domain_logup_sum(self.handle, ob.ptr if n else None, tot, hb.ptr if helpers and n else None, bt.ptr if n else None,
                                                    bm.ptr if n else None, bv.ptr if n else None, m, stride, n, self._scalar(beta, montgomery),
                                                    flags | (2 if bt.is_device else 0), bt.stream if bt.is_device else None))
        if not bt.is_device:
            res = _like_input(table, res, (n, 32))
        total = self._scalar_out(tot.raw, montgomery)
        return (res, total, hres) if helpers else (res, total)

    def set_option(self, key: str, value: int) -> None:
        _check(self._lib.mi355_msm_domain_set_option(self.handle, key.encode(), int(value)))

    def query(self, key: str) -> int:
        """ "size", "log_size", "passes", "pass_log", "table_bytes", "work_bytes", "poly_work_bytes", "scan_work_bytes", "quotient_work_bytes",
        "mle_work_bytes", "logup_work_bytes", "sumcheck_levels", "sumcheck_max_tables", "sumcheck_max_terms", "sumcheck_max_factors", "poly_tile_log",
        "device", "last_us", "last_device_us" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_domain_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_domain_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _index_array(obj, dtype, what):
    """a contiguous NumPy array of `dtype` from an integer array (NumPy, torch CPU, a list) or little-endian bytes of that type"""
    import numpy as np

    if hasattr(obj, "data_ptr") and hasattr(obj, "is_cuda"):
        if obj.is_cuda:
            raise ValueError(f"{what}: the structure of a matrix is read from host memory")
        obj = obj.numpy()
    if isinstance(obj, (bytes, bytearray, memoryview)):
        if len(obj) % np.dtype(dtype).itemsize:
            raise ValueError(f"{what}: not a whole number of {np.dtype(dtype).itemsize}-byte integers")
        return np.frombuffer(bytes(obj), dtype=dtype)
    return np.ascontiguousarray(np.asarray(obj).reshape(-1), dtype=dtype)


class SparseMatrix:
    """A sparse matrix over ``Fr`` resident on one GPU (mi355_msm_sparse_*): the R1CS matrices of a proving key, uploaded once like the
    bases of an MSM.  ``apply(z)`` is ``y = M z``.  Made by ``Radix2EvaluationDomain.sparse_matrix`` or ``SparseMatrix.from_rows``."""

    def __init__(self, dom, rows, cols, row_ptr, col_idx, values, montgomery: bool = True):
        import numpy as np

        self.handle = ctypes.c_void_p()
        self.dom = dom
        if not dom.handle:
            raise MsmError(-1, "the domain is closed")
        self._lib = dom._lib
        rows, cols = int(rows), int(cols)
        if rows < 0 or cols < 0:
            raise ValueError("rows and cols must not be negative")
        rp = _index_array(row_ptr, np.uint64, "row_ptr")
        ci = _index_array(col_idx, np.uint32, "col_idx")
        if rp.size != rows + 1:
            raise ValueError(f"row_ptr: {rows + 1} offsets for {rows} rows, not {rp.size}")
        vb = _Buf(values)
        if vb.is_device:
            raise ValueError("values: the coefficients of a matrix are read from host memory")
        if vb.nbytes != ci.size * 32:
            raise ValueError(f"values: {ci.size} 32-byte elements beside {ci.size} column indices, not {vb.nbytes} bytes")
        _check(self._lib.mi355_msm_sparse_create(ctypes.byref(self.handle), dom.handle, rows, cols, rp.ctypes.data, ci.ctypes.data if ci.size else None,
                                                 vb.ptr if ci.size else None, 0 if montgomery else 1))
        self.rows, self.cols, self.nnz = self.query("rows"), self.query("cols"), self.query("nnz")

    @classmethod
    def from_rows(cls, dom, rows_list, cols) -> "SparseMatrix":
        """arkworks' ``Matrix<F> = Vec<Vec<(F, usize)>>``: a list of rows, each a list of ``(coefficient as an integer, column)``"""
        import numpy as np

        row_ptr, col_idx, vals = [0], [], []
        for row in rows_list:
            for coeff, col in row:
                col_idx.append(int(col))
                vals.append((int(coeff) % dom.modulus).to_bytes(32, "little"))
            row_ptr.append(len(col_idx))
        if any(c < 0 or c >= 1 << 32 for c in col_idx):
            raise ValueError("a column index is out of range")
        return cls(dom, len(row_ptr) - 1, cols, np.array(row_ptr, dtype=np.uint64), np.array(col_idx, dtype=np.uint32), b"".join(vals), montgomery=False)

    def apply(self, z, montgomery: bool = True, out=None):
        """``y = M z``: ``z`` holds ``cols`` 32-byte elements.  Bytes or NumPy in gives a NumPy array ``(rows, 32)``; a torch GPU tensor of
        shape ``(cols, 32)`` is read in place on its current stream and gives a GPU tensor (``out=``: one of shape ``(rows, 32)`` to write
        into, which must not overlap ``z``).  ``montgomery`` is the form of ``z`` and of the result, whatever the form given at creation."""
        if not self.handle:
            raise MsmError(-1, "the matrix is closed")
        shape = getattr(z, "shape", None)
        b = _Buf(z)
        if b.nbytes != self.cols * 32 or (shape is not None and tuple(shape) != (self.cols, 32)):
            raise ValueError(f"z: {self.cols} 32-byte elements, shape ({self.cols}, 32), not {tuple(shape) if shape is not None else b.nbytes}")
        flags = 0 if montgomery else 1
        if b.is_device:
            import torch

            if b.device_index != self.dom.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this matrix is bound to device {self.dom.device}")
            if out is None:
                out = torch.empty((self.rows, 32), dtype=torch.uint8, device=b.keep.device)
            if tuple(getattr(out, "shape", ())) != (self.rows, 32):
                raise ValueError(f"out: a contiguous uint8 GPU tensor of shape ({self.rows}, 32)")
            ob = _Buf(out)
            if not ob.is_device or ob.keep is not out:
                raise ValueError(f"out: a contiguous uint8 GPU tensor of shape ({self.rows}, 32)")
            _check(self._lib.mi355_msm_sparse_apply(self.handle, ob.ptr if self.rows else None, b.ptr if self.cols else None, flags | 2, b.stream))
            return out
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros((self.rows, 32), dtype=np.uint8)
        _check(self._lib.mi355_msm_sparse_apply(self.handle, res.ctypes.data if self.rows else None, b.ptr if self.cols else None, flags, None))
        return res

    def query(self, key: str) -> int:
        """ "rows", "cols", "nnz", "entries_per_lane", "block_lanes", "work_bytes" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_sparse_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_sparse_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LookupTable:
    """A lookup table over ``Fr`` resident on one GPU (mi355_msm_lookup_*): ``table`` holds ``1 <= n_t <= 2^28`` 32-byte elements (bytes,
    NumPy or torch; a GPU tensor is read on its current stream).  Equality is equality modulo r in the form given here, and every
    later call must bring values in the same form.  Duplicates are allowed; every match is credited to the first occurrence.
    ``multiplicities(values)`` are logUp's ``m``; ``sorted(values)`` is plookup's ``s = (f, t)`` sorted by ``t``."""

    def __init__(self, dom, table, montgomery: bool = True):
        self.handle = ctypes.c_void_p()
        self.dom = dom
        if not dom.handle:
            raise MsmError(-1, "the domain is closed")
        self._lib = dom._lib
        self.montgomery = bool(montgomery)
        b = _Buf(table)
        if b.nbytes == 0 or b.nbytes % 32:
            raise ValueError(f"table: a whole number (at least one) of 32-byte elements, not {b.nbytes} bytes")
        if b.is_device and b.device_index != dom.device:
            raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {dom.device}")
        self._flags = 0 if montgomery else 1
        _check(self._lib.mi355_msm_lookup_create(ctypes.byref(self.handle), dom.handle, b.ptr, b.nbytes // 32, self._flags | (2 if b.is_device else 0),
                                                 b.stream if b.is_device else None))
        self.n = b.nbytes // 32

    def _values(self, values):
        if not self.handle:
            raise MsmError(-1, "the lookup table is closed")
        b = _Buf(values)
        if b.nbytes % 32:
            raise ValueError(f"values: a whole number of 32-byte elements, not {b.nbytes} bytes")
        if b.is_device and b.device_index != self.dom.device:
            raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this table is bound to device {self.dom.device}")
        return b, b.nbytes // 32

    def multiplicities(self, values, index: bool = False):
        """``(mult, missing, first_missing)``, with ``index=True`` ``(mult, missing, first_missing, index)``: ``mult`` holds ``n`` elements
        in the form of the table, ``mult[i]`` = how many values equal ``table[i]`` (0 at later duplicates); ``index[j]`` (uint32) is the
        first table index of ``values[j]`` or 0xFFFFFFFF; ``missing`` values have no match, the first at ``first_missing``
        (``len(values)`` when none).  A missing value does not raise."""
        b, n_f = self._values(values)
        stats = (ctypes.c_uint64 * 2)()
        if b.is_device:
            import torch

            mult = torch.empty((self.n, 32), dtype=torch.uint8, device=b.keep.device)
            idx = torch.empty((n_f,), dtype=torch.int32, device=b.keep.device) if index else None
            _check(self._lib.mi355_msm_lookup_count(self.handle, mult.data_ptr(), idx.data_ptr() if index and n_f else None, stats, b.ptr if n_f else None,
                                                    n_f, self._flags | 2, b.stream))
            if index:
                idx = idx.view(torch.uint32) if hasattr(torch, "uint32") else idx
        else:
            import numpy as np

            mult = np.zeros((self.n, 32), dtype=np.uint8)
            idx = np.zeros(n_f, dtype=np.uint32) if index else None
            _check(self._lib.mi355_msm_lookup_count(self.handle, mult.ctypes.data, idx.ctypes.data if index and n_f else None, stats, b.ptr if n_f else None,
                                                    n_f, self._flags, None))
            mult = _like_input(values, mult.reshape(-1), (self.n, 32))
        return (mult, int(stats[0]), int(stats[1]), idx) if index else (mult, int(stats[0]), int(stats[1]))

    def sorted(self, values, out=None):
        """plookup's sorted vector: the ``n + len(values)`` canonical elements ``table[i]`` followed by ``mult[i]`` further copies, for
        ``i`` in order.  Jellyfish's ``h1 = s[:n]``, ``h2 = s[n-1:]`` and Plonkup's alternating halves are slices of it.  Raises
        ``MsmError`` naming ``first_missing`` when a value is absent from the table (``out`` is then untouched)."""
        b, n_f = self._values(values)
        total = self.n + n_f
        stats = (ctypes.c_uint64 * 2)()
        if b.is_device:
            import torch

            if out is None:
                out = torch.empty((total, 32), dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.nbytes != total * 32 or ob.keep is not out:
                raise ValueError(f"out must be a contiguous uint8 GPU tensor of {total * 32} bytes")
            _check(self._lib.mi355_msm_lookup_sorted(self.handle, ob.ptr, stats, b.ptr if n_f else None, n_f, self._flags | 2, b.stream))
            res = out
        else:
            if out is not None:
                raise ValueError("out= goes with GPU tensors")
            import numpy as np

            res = np.zeros((total, 32), dtype=np.uint8)
            _check(self._lib.mi355_msm_lookup_sorted(self.handle, res.ctypes.data, stats, b.ptr if n_f else None, n_f, self._flags, None))
            res = _like_input(values, res.reshape(-1), (total, 32))
        if stats[0]:
            raise MsmError(-1, f"{int(stats[0])} values are not in the table; first_missing = {int(stats[1])}")
        return res

    def query(self, key: str) -> int:
        """ "n", "slots", "distinct", "max_probe", "table_bytes", "lookup_work_bytes" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_lookup_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_lookup_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- custom-gate expressions over Fr columns with rotations (mi355_msm_expr_*) ------------------------------------------------------------

class Expr:
    """A polynomial expression over columns of ``Fr``, built with ``+ - * **`` (a small non-negative integer exponent) and unary minus
    from the leaves ``Expr.col(j, rot=0)`` (column ``j`` at row ``i + rot * rot_step``), ``Expr.const(v)`` (an integer, fixed when the
    expression is compiled) and ``Expr.challenge(k)`` (given at every run).  Integers mix in as constants.  Equal sub-expressions are
    ONE object (hash-consing; ``a + b`` and ``b + a`` alike), so a shared term is evaluated once per row.  ``nodes()`` is the flat
    DAG ``mi355_msm_expr_create`` takes."""

    COL, CONST, CHAL, ADD, SUB, MUL, NEG, SQR = range(8)
    __slots__ = ("op", "a", "b", "serial", "__weakref__")
    _interned = weakref.WeakValueDictionary()
    _count = 0

    def __init__(self, op, a, b):
        raise TypeError("build expressions from Expr.col, Expr.const and Expr.challenge")

    @classmethod
    def _make(cls, op, a, b=None):
        leaf = op <= cls.CHAL
        if op in (cls.ADD, cls.MUL) and b.serial < a.serial:
            a, b = b, a
        key = (op, a, b) if leaf else (op, a.serial, b.serial if b is not None else -1)
        e = cls._interned.get(key)
        if e is None:
            e = object.__new__(cls)
            e.op, e.a, e.b = op, a, b
            Expr._count += 1
            e.serial = Expr._count
            cls._interned[key] = e
        return e

    @classmethod
    def col(cls, j: int, rot: int = 0):
        j, rot = int(j), int(rot)
        if j < 0:
            raise ValueError("a column index is not negative")
        return cls._make(cls.COL, j, rot)

    @classmethod
    def const(cls, v: int):
        return cls._make(cls.CONST, int(v), None)

    @classmethod
    def challenge(cls, k: int):
        k = int(k)
        if k < 0:
            raise ValueError("a challenge index is not negative")
        return cls._make(cls.CHAL, k, None)

    @classmethod
    def _of(cls, x):
        if isinstance(x, Expr):
            return x
        if isinstance(x, int) and not isinstance(x, bool):
            return cls.const(x)
        return None

    def __add__(self, o):
        o = Expr._of(o)
        return NotImplemented if o is None else Expr._make(Expr.ADD, self, o)

    __radd__ = __add__

    def __sub__(self, o):
        o = Expr._of(o)
        return NotImplemented if o is None else Expr._make(Expr.SUB, self, o)

    def __rsub__(self, o):
        o = Expr._of(o)
        return NotImplemented if o is None else Expr._make(Expr.SUB, o, self)

    def __mul__(self, o):
        o = Expr._of(o)
        if o is None:
            return NotImplemented
        return Expr._make(Expr.SQR, self) if o is self else Expr._make(Expr.MUL, self, o)

    __rmul__ = __mul__

    def __neg__(self):
        return Expr._make(Expr.NEG, self)

    def __pow__(self, e):
        if not isinstance(e, int) or isinstance(e, bool) or not 0 <= e <= 1 << 16:
            raise ValueError("the exponent is an integer 0 .. 65536")
        if e == 0:
            return Expr.const(1)
        acc = self
        for bit in bin(e)[3:]:            # square and multiply from the top bit
            acc = acc * acc
            if bit == "1":
                acc = acc * self
        return acc

    def nodes(self, modulus: Optional[int] = None):
        """``(nodes, consts, n_chal, n_cols_used)``: the sub-expressions this one depends on as ``(op, a, b)`` triples in topological
        order, this one last; ``consts`` the distinct constants (reduced modulo ``modulus`` when given) that ``CONST`` nodes index."""
        index, out, consts, const_at = {}, [], [], {}
        n_chal = n_cols = 0
        stack = [(self, False)]
        while stack:
            e, seen = stack.pop()
            if e.serial in index:
                continue
            if e.op <= Expr.CHAL:
                if e.op == Expr.COL:
                    n_cols = max(n_cols, e.a + 1)
                    node = (Expr.COL, e.a, e.b & 0xFFFFFFFF)
                elif e.op == Expr.CONST:
                    v = e.a % modulus if modulus else e.a
                    if v in const_at:                 # constants that are equal modulo the field are one node
                        index[e.serial] = const_at[v]
                        continue
                    const_at[v] = len(out)
                    consts.append(v)
                    node = (Expr.CONST, len(consts) - 1, 0)
                else:
                    n_chal = max(n_chal, e.a + 1)
                    node = (Expr.CHAL, e.a, 0)
            elif not seen:
                stack.append((e, True))
                for c in (e.b, e.a):
                    if c is not None and c.serial not in index:
                        stack.append((c, False))
                continue
            else:
                node = (e.op, index[e.a.serial], index[e.b.serial] if e.b is not None else 0)
            index[e.serial] = len(out)
            out.append(node)
        return out, consts, n_chal, n_cols

    def __repr__(self):
        if self.op == Expr.COL:
            return f"col({self.a}, {self.b})"
        if self.op == Expr.CONST:
            return f"const({self.a})"
        if self.op == Expr.CHAL:
            return f"challenge({self.a})"
        return f"<Expr {('add', 'sub', 'mul', 'neg', 'sqr')[self.op - 3]} #{self.serial}>"


class GateProgram:
    """An ``Expr`` compiled for one domain's field and device (mi355_msm_expr_*; ``dom.compile_expression(expr, ncols)``): a straight-line
    program whose one launch evaluates the expression for every row.  ``query``: "nodes", "instructions", "slots", "products" (field
    products per row, conversions included), "reduces", "columns", "lds_bytes", "last_us", "last_device_us"."""

    def __init__(self, dom, expr, ncols: int):
        self.handle = ctypes.c_void_p()
        self.dom = dom
        if not dom.handle:
            raise MsmError(-1, "the domain is closed")
        if not isinstance(expr, Expr):
            raise TypeError("expr: an Expr")
        self._lib = dom._lib
        nodes, consts, self.n_chal, used = expr.nodes(dom.modulus)
        self.ncols = int(ncols)
        if used > self.ncols:
            raise ValueError(f"the expression reads column {used - 1}, ncols is {self.ncols}")
        flat = (ctypes.c_uint32 * (3 * len(nodes)))(*[w for node in nodes for w in node])
        cb = b"".join(v.to_bytes(32, "little") for v in consts)
        _check(self._lib.mi355_msm_expr_create(ctypes.byref(self.handle), dom.handle, flat, len(nodes), cb if consts else None, len(consts), self.n_chal,
                                               self.ncols, 1))

    def run(self, cols, challenges=(), rot_step: int = 1, montgomery: bool = True, out=None):
        """``out[i]`` = the expression at row ``i`` for ``i < len = max(len(cols[j]))``: ``cols`` is a list of ``ncols`` vectors of 32-byte
        elements (bytes, NumPy or torch, all in one kind of memory) whose lengths divide ``len``; column ``j`` at rotation ``rot`` is read
        at row ``((i + rot * rot_step) mod len) mod len(cols[j])``, so a periodic column costs its period and a column of one element is a
        scalar.  ``challenges``: ``n_chal`` integers.  ``rot_step`` is ``M / n`` on a quotient domain, 1 on the constraint domain.  GPU
        tensors in give a GPU tensor out, on the current stream; ``out`` may be one of the full-length columns if the expression reads
        that column at rotation 0 only."""
        if not self.handle:
            raise MsmError(-1, "the program is closed")
        cols = list(cols)
        challenges = [int(c) for c in challenges]
        if len(cols) != self.ncols or len(challenges) != self.n_chal:
            raise ValueError(f"the program takes {self.ncols} columns and {self.n_chal} challenges")
        bufs = [_Buf(c) for c in cols]
        for b in bufs:
            if b.nbytes % 32 or b.is_device != bufs[0].is_device:
                raise ValueError("the columns must hold 32-byte elements, in the same kind of memory")
            if b.is_device and b.device_index != self.dom.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this domain is bound to device {self.dom.device}")
        lens = [b.nbytes // 32 for b in bufs]
        if not bufs:
            raise ValueError("a program without columns has no rows")
        n = max(lens)
        first = bufs[lens.index(n)]
        res, ob = self.dom._out(cols[lens.index(n)], first, out, n)
        m = self.ncols
        ptrs = (ctypes.c_void_p * m)(*[b.ptr for b in bufs])
        lv = (ctypes.c_size_t * m)(*lens)
        cb = b"".join(self.dom._scalar(c, montgomery) for c in challenges)
        flags = (0 if montgomery else 1) | (2 if first.is_device else 0)
        _check(self._lib.mi355_msm_expr_run(self.handle, ob.ptr if n else None, ptrs, lv, m, n, int(rot_step), cb if challenges else None, len(challenges),
                                            flags, first.stream if first.is_device else None))
        if first.is_device:
            return res
        return _like_input(cols[lens.index(n)], res, (n, 32))

    def query(self, key: str) -> int:
        """ "nodes", "instructions", "slots", "products", "reduces", "columns", "lds_bytes", "last_us", "last_device_us" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_expr_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_expr_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Poseidon sponges and Merkle trees over Fr (mi355_msm_poseidon_*) ------------------------------------------------------------------

SNARKVM_POSEIDON = {"alpha": 17, "full_rounds": 8, "partial_rounds": 31, "skip_matrices": 0}   # BLS12-377, every rate 2 .. 8


class _Grain:
    """The 80-bit Grain LFSR of the Poseidon paper in self-shrinking mode, as a shift register in one integer (bit 79 is b0)."""

    TAPS = (0, 13, 23, 38, 51, 62)

    def __init__(self, field_bits, t, full_rounds, partial_rounds):
        state = 0
        # b0 b1 = 01: a prime field; b2 .. b5 = 0000: x^alpha; then n in 12 bits, t in 12, R_F in 10, R_P in 10, and thirty ones
        for value, width in ((1, 2), (0, 4), (field_bits, 12), (t, 12), (full_rounds, 10), (partial_rounds, 10), ((1 << 30) - 1, 30)):
            if value >> width:
                raise ValueError("a parameter does not fit the generator's seed")
            state = (state << width) | value
        self.state, self.bits = state, field_bits
        for _ in range(160):
            self._next()

    def _next(self):
        b = 0
        for k in self.TAPS:
            b ^= (self.state >> (79 - k)) & 1
        self.state = ((self.state << 1) & ((1 << 80) - 1)) | b
        return b

    def integer(self):
        """field_bits bits, the first the most significant: pairs of bits, the second of which counts when the first is 1"""
        v = 0
        for _ in range(self.bits):
            while True:
                first, second = self._next(), self._next()
                if first:
                    break
            v = (v << 1) | second
        return v


def poseidon_parameters(curve, rate: int, alpha: int, full_rounds: int, partial_rounds: int, skip_matrices: int = 0):
    """Round constants and MDS matrix of a Poseidon instance over the scalar field of ``curve``, by the rule of snarkVM's
    ``find_poseidon_ark_and_mds``: ``(full_rounds + partial_rounds)`` rows of ``rate + 1`` constants by rejection sampling from the
    Grain LFSR, ``skip_matrices`` discarded matrices, then ``xs`` and ``ys`` reduced mod p and ``mds[i][j] = 1 / (xs[i] + ys[j])``.
    Returns ``(ark, mds)`` as lists of rows of integers.  ``alpha`` does not enter the generator (only its sign does)."""
    p = FR_MODULUS[_curve_id(curve) & 1]
    t = int(rate) + 1
    if not 1 <= rate <= 8:
        raise ValueError("rate: 1 .. 8")
    if alpha < 3 or not alpha & 1:
        raise ValueError("alpha: odd, at least 3")
    g = _Grain(p.bit_length(), t, int(full_rounds), int(partial_rounds))
    ark = []
    for _ in range(full_rounds + partial_rounds):
        row = []
        while len(row) < t:
            v = g.integer()
            if v < p:
                row.append(v)
        ark.append(row)
    for _ in range(2 * t * skip_matrices):
        g.integer()
    xs = [g.integer() % p for _ in range(t)]
    ys = [g.integer() % p for _ in range(t)]
    if any((x + y) % p == 0 for x in xs for y in ys):
        raise ValueError("this matrix does not exist (x + y = 0): skip it")
    return ark, [[pow(x + y, -1, p) for y in ys] for x in xs]


def _rows_of(inputs, in_len, what):
    """(buffer, n, in_len) of a batch of rows: shape (n, in_len, 32), (in_len, 32) for one row, or flat bytes with in_len given"""
    shape = getattr(inputs, "shape", None)
    b = _Buf(inputs)
    if b.nbytes % 32:
        raise ValueError(f"{what}: 32-byte elements")
    if shape is not None and len(shape) == 3 and shape[2] == 32:
        n, ln = int(shape[0]), int(shape[1])
    elif shape is not None and len(shape) == 2 and shape[1] == 32 and in_len is None:
        n, ln = 1, int(shape[0])
    else:
        total = b.nbytes // 32
        ln = total if in_len is None else int(in_len)
        if ln < 0 or (ln == 0 and total) or (ln and total % ln):
            raise ValueError(f"{what}: {total} elements are no whole number of rows of {ln}")
        n = total // ln if ln else 1
    if in_len is not None and ln != int(in_len):
        raise ValueError(f"{what}: rows of {ln} elements, not in_len = {in_len}")
    return b, n, ln


class Poseidon:
    """Poseidon over ``Fr`` on one GPU (mi355_msm_poseidon_*): snarkVM's ``PoseidonSponge``, ``Poseidon::hash_many`` / ``hash`` and its
    Poseidon Merkle tree, for batches.  ``parameters``: ``None`` for snarkVM's instance on BLS12-377 (alpha 17, 8 full and 31 partial
    rounds), or a dict with ``alpha``, ``full_rounds``, ``partial_rounds`` and either ``ark`` and ``mds`` (rows of integers) or
    ``skip_matrices`` for ``poseidon_parameters``.  ``domain``: the domain separator of ``hash_many``, ``hash`` and ``merkle_tree``, a
    string read as snarkVM's ``from_bytes_le_mod_order`` or an integer.  Inputs are batches of rows of 32-byte elements -- a NumPy
    array or torch tensor of shape ``(n, in_len, 32)``, or bytes with ``in_len=`` -- ``montgomery`` selects arkworks images (default) or
    plain integers; a torch GPU tensor is read in place on its current stream and gives a GPU tensor (``out=``: one to write into)."""

    def __init__(self, dom, rate: int, parameters=None, domain=None):
        self.handle = ctypes.c_void_p()
        self.dom = dom
        if not dom.handle:
            raise MsmError(-1, "the domain is closed")
        self._lib = dom._lib
        if parameters is None:
            if dom.curve & 1:
                raise ValueError("parameters=None is snarkVM's instance over BLS12-377; the reference fixes none for BLS12-381: pass parameters")
            parameters = dict(SNARKVM_POSEIDON)
        par = dict(parameters)
        alpha, rf, rp = int(par["alpha"]), int(par["full_rounds"]), int(par["partial_rounds"])
        if "ark" in par or "mds" in par:
            ark, mds = par["ark"], par["mds"]
        else:
            ark, mds = poseidon_parameters(dom.curve, rate, alpha, rf, rp, int(par.get("skip_matrices", 0)))
        t = int(rate) + 1
        if len(ark) != rf + rp or any(len(r) != t for r in ark) or len(mds) != t or any(len(r) != t for r in mds):
            raise ValueError(f"ark: {rf + rp} rows of {t} integers, mds: {t} rows of {t}")
        p = dom.modulus
        ab = b"".join((int(v) % p).to_bytes(32, "little") for r in ark for v in r)
        mb = b"".join((int(v) % p).to_bytes(32, "little") for r in mds for v in r)
        _check(self._lib.mi355_msm_poseidon_create(ctypes.byref(self.handle), dom.handle, int(rate), alpha, rf, rp, ab, mb, 1))
        self.rate, self.alpha, self.full_rounds, self.partial_rounds = int(rate), alpha, rf, rp
        if isinstance(domain, str):
            domain = int.from_bytes(domain.encode(), "little")
        self.domain = None if domain is None else int(domain) % p

    def _element(self, value, montgomery):
        p = self.dom.modulus
        return ((value << 256) % p if montgomery else value % p).to_bytes(32, "little")

    def _header(self, length, montgomery):
        if self.domain is None:
            raise ValueError("hash_many, hash and merkle_tree need the domain separator: Poseidon(.., domain=...)")
        if self.rate < 2:
            raise ValueError("the header [domain, length, 0 ..] needs a rate of at least 2")
        return b"".join(self._element(v, montgomery) for v in [self.domain, length] + [0] * (self.rate - 2))

    def _run(self, inputs, n_out, in_len, montgomery, out, header):
        if not self.handle:
            raise MsmError(-1, "the Poseidon handle is closed")
        b, n, ln = _rows_of(inputs, in_len, "inputs")
        n_out = int(n_out)
        if n_out < 0:
            raise ValueError("n_out must not be negative")
        hdr = header(ln) if header else None
        flags = 0 if montgomery else 1
        if b.is_device:
            import torch

            if b.device_index != self.dom.device:
                raise MsmError(-1, f"the input lives on cuda:{b.device_index} but this handle is bound to device {self.dom.device}")
            if out is None:
                out = torch.empty((n, n_out, 32), dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.keep is not out or ob.nbytes != n * n_out * 32:
                raise ValueError(f"out: a contiguous uint8 GPU tensor of {n} x {n_out} 32-byte elements")
            _check(self._lib.mi355_msm_poseidon_hash(self.handle, ob.ptr if ob.nbytes else None, b.ptr if b.nbytes else None, n, ln, n_out, hdr,
                                                     flags | 2, b.stream))
            return out
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros((n, n_out, 32), dtype=np.uint8)
        _check(self._lib.mi355_msm_poseidon_hash(self.handle, res.ctypes.data if res.size else None, b.ptr if b.nbytes else None, n, ln, n_out, hdr,
                                                 flags, None))
        return res

    def sponge(self, inputs, n_out: int, in_len=None, montgomery: bool = True, out=None):
        """The raw ``PoseidonSponge``: absorb each row, squeeze ``n_out`` elements; the result has shape ``(n, n_out, 32)``."""
        return self._run(inputs, n_out, in_len, montgomery, out, None)

    def hash_many(self, inputs, n_out: int, in_len=None, montgomery: bool = True, out=None):
        """``Poseidon::hash_many`` of each row: the preimage is ``[domain, in_len, 0 ..] || row``; shape ``(n, n_out, 32)``."""
        return self._run(inputs, n_out, in_len, montgomery, out, lambda ln: self._header(ln, montgomery))

    def hash(self, inputs, in_len=None, montgomery: bool = True, out=None):
        """``Poseidon::hash`` of each row: ``hash_many(row, 1)[0]``; shape ``(n, 32)``"""
        res = self.hash_many(inputs, 1, in_len=in_len, montgomery=montgomery, out=out)
        return res.reshape(res.shape[0], 32)

    def merkle_tree(self, leaves, leaf_len=None, montgomery: bool = True, out=None) -> "PoseidonMerkleTree":
        """snarkVM's Poseidon Merkle tree over ``leaves`` -- shape ``(n_leaves, leaf_len, 32)`` -- as a ``PoseidonMerkleTree``: ``nodes`` are
        the ``2P - 1`` nodes in the reference's order (root of the built part first, leaf hashes from ``P - 1``)."""
        if not self.handle:
            raise MsmError(-1, "the Poseidon handle is closed")
        b, n, ln = _rows_of(leaves, leaf_len, "leaves")
        if n < 1:
            raise ValueError("a tree has at least one leaf")
        self._header(3, montgomery)
        P = 1 << (n - 1).bit_length()
        sep = self._element(self.domain, montgomery)
        flags = 0 if montgomery else 1
        if b.is_device:
            import torch

            if b.device_index != self.dom.device:
                raise MsmError(-1, f"the leaves live on cuda:{b.device_index} but this handle is bound to device {self.dom.device}")
            if out is None:
                out = torch.empty((2 * P - 1, 32), dtype=torch.uint8, device=b.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.keep is not out or ob.nbytes != (2 * P - 1) * 32:
                raise ValueError(f"out: a contiguous uint8 GPU tensor of shape ({2 * P - 1}, 32)")
            _check(self._lib.mi355_msm_poseidon_merkle(self.handle, ob.ptr, b.ptr if b.nbytes else None, n, ln, sep, flags | 2, b.stream))
            return PoseidonMerkleTree(self, out, n, montgomery)
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros((2 * P - 1, 32), dtype=np.uint8)
        _check(self._lib.mi355_msm_poseidon_merkle(self.handle, res.ctypes.data, b.ptr if b.nbytes else None, n, ln, sep, flags, None))
        return PoseidonMerkleTree(self, res, n, montgomery)

    def set_option(self, key: str, value: int) -> None:
        """ "sparse": 1 (default) or 0, the partial rounds run densely from ark and mds (a test hook; the results are identical)"""
        _check(self._lib.mi355_msm_poseidon_set_option(self.handle, key.encode(), int(value)))

    def query(self, key: str) -> int:
        """ "rate", "state", "rounds", "sparse", "products_per_permutation", "lds_bytes", "work_bytes", "block_lanes" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_poseidon_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_poseidon_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseidonMerkleTree:
    """The result of ``Poseidon.merkle_tree``: ``nodes`` (NumPy or GPU tensor, shape ``(2P - 1, 32)``), ``number_of_leaves``,
    ``root(depth)`` and ``path(i)`` as snarkVM's ``MerkleTree::root`` and ``prove`` give them."""

    def __init__(self, hasher, nodes, number_of_leaves, montgomery):
        self.hasher, self.nodes, self.number_of_leaves, self.montgomery = hasher, nodes, int(number_of_leaves), montgomery
        self.leaf_count = (int(nodes.shape[0]) + 1) // 2
        self.levels = self.leaf_count.bit_length() - 1

    def _node(self, i) -> bytes:
        row = self.nodes[i]
        return bytes(row.cpu().numpy().tobytes() if hasattr(row, "cpu") else row.tobytes())

    def empty_hash(self) -> bytes:
        """``hash_children(0, 0)``: a padding leaf of this tree when it has one, else one hash"""
        if self.number_of_leaves < self.leaf_count:
            return self._node(self.leaf_count - 1 + self.number_of_leaves)
        one = self.hasher._element(1, self.montgomery)
        return self.hasher.hash(one + bytes(64), in_len=3, montgomery=self.montgomery).tobytes()

    def root(self, depth=None) -> bytes:
        """The root of a tree of ``depth`` levels: the root of the built part hashed ``depth - levels`` times with the empty hash on its
        right (a handful of single hashes); ``depth=None`` is the built part's own root."""
        root = self._node(0)
        if depth is None or depth == self.levels:
            return root
        if depth < self.levels:
            raise ValueError(f"{self.number_of_leaves} leaves need a depth of at least {self.levels}")
        one, empty = self.hasher._element(1, self.montgomery), self.empty_hash()
        for _ in range(depth - self.levels):
            root = self.hasher.hash(one + root + empty, in_len=3, montgomery=self.montgomery).tobytes()
        return root

    def path(self, i: int):
        """The sibling hashes from leaf ``i`` up to below the root of the built part, as a list of 32-byte elements"""
        if not 0 <= i < self.number_of_leaves:
            raise ValueError("the leaf index is out of bounds")
        idx, out = self.leaf_count - 1 + int(i), []
        while idx:
            out.append(self._node(idx + 1 if idx & 1 else idx - 1))
            idx = (idx - 1) // 2
        return out


class Pairing:
    """Batch pairings and pairing products on one GPU (mi355_msm_pairing_*): arkworks' / snarkVM's ``Bls12::pairing`` and
    ``product_of_pairings`` for the family of ``curve`` (any of the four names selects it).  ``p`` holds n arkworks ``Affine<G1>`` images
    (104 bytes each, or ``p_stride``), ``q`` n ``Affine<G2>`` images (200 bytes, or ``q_stride``) -- bytes, a NumPy array or a torch
    tensor; the points must be of order r or flagged infinity, nothing is tested.  A Gt value is 576 bytes: arkworks' in-memory ``Fq12``
    (Montgomery), or with ``canonical=True`` its ``CanonicalSerialize``.  Torch GPU tensors are read in place on the current stream and
    give GPU tensors (``out=``: one to write into)."""

    GT_BYTES = 576

    def __init__(self, curve="bls12_377_g1", device: Optional[int] = None):
        self.curve = _curve_id(curve)
        self.handle = ctypes.c_void_p()
        self._lib = load_library()
        _check(self._lib.mi355_msm_pairing_create(ctypes.byref(self.handle), self.curve, -1 if device is None else device))
        self.device = self.query("device")

    def _inputs(self, p, q, p_stride, q_stride):
        if not self.handle:
            raise MsmError(-1, "the pairing handle is closed")
        a, b = _Buf(p), _Buf(q)
        s1, s2 = int(p_stride or 104), int(q_stride or 200)
        if s1 <= 0 or s2 <= 0 or a.nbytes % s1 or b.nbytes % s2 or a.nbytes // s1 != b.nbytes // s2:
            raise ValueError(f"p: n images of {s1} bytes, q: n images of {s2} bytes ({a.nbytes} and {b.nbytes} bytes given)")
        if a.is_device != b.is_device:
            raise ValueError("p and q must both be GPU tensors or both live on the host")
        if a.is_device:
            for t in (a, b):
                if t.device_index != self.device:
                    raise MsmError(-1, f"an input lives on cuda:{t.device_index} but this handle is bound to device {self.device}")
        return a, b, s1, s2, a.nbytes // s1

    def _call(self, name, p, q, group, unit, flags, out, p_stride, q_stride):
        a, b, s1, s2, n = self._inputs(p, q, p_stride, q_stride)
        fn = getattr(self._lib, name)
        group = int(group)
        if group < 1 or n % group:
            raise ValueError(f"{n} pairs are not whole groups of {group}")
        m = n // group
        shape = (m, unit) if unit > 1 else (m,)
        if a.is_device:
            import torch

            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=a.keep.device)
            ob = _Buf(out)
            if not ob.is_device or ob.keep is not out or ob.nbytes != m * unit:
                raise ValueError(f"out: a contiguous uint8 GPU tensor of {m} x {unit} bytes")
            _check(fn(self.handle, ob.ptr if n else None, a.ptr if n else None, s1, b.ptr if n else None, s2, n, group, flags | 2, a.stream))
            return out
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros(shape, dtype=np.uint8)
        _check(fn(self.handle, res.ctypes.data if n else None, a.ptr if n else None, s1, b.ptr if n else None, s2, n, group, flags, None))
        return res

    def pairing(self, p, q, group: int = 1, canonical: bool = False, out=None, p_stride=None, q_stride=None):
        """``out[j] = prod_{i < group} e(p[j group + i], q[j group + i])``: shape ``(n / group, 576)`` uint8"""
        return self._call("mi355_msm_pairing_run", p, q, group, self.GT_BYTES, 1 if canonical else 0, out, p_stride, q_stride)

    def product_of_pairings(self, p, q, canonical: bool = False, p_stride=None, q_stride=None):
        """``product_of_pairings``: the 576 bytes of ``prod_i e(p[i], q[i])`` (the empty product is one)"""
        n = self._inputs(p, q, p_stride, q_stride)[4]
        if n == 0:
            raise ValueError("product_of_pairings needs at least one pair")
        res = self.pairing(p, q, group=n, canonical=canonical, p_stride=p_stride, q_stride=q_stride)
        return res.reshape(-1) if hasattr(res, "is_cuda") else res.tobytes()

    def check(self, p, q, group=None, out=None, p_stride=None, q_stride=None):
        """Whether the product over each group of ``group`` pairs is one: a bool array of n / group entries, or -- ``group=None``, the
        whole input -- one bool.  No Gt image leaves the device."""
        n = self._inputs(p, q, p_stride, q_stride)[4]
        whole = group is None
        if whole and n == 0:
            return True
        res = self._call("mi355_msm_pairing_check", p, q, n if whole else group, 1, 0, out, p_stride, q_stride)
        if hasattr(res, "is_cuda"):
            res = res != 0
            return bool(res[0].item()) if whole else res
        res = res.astype(bool)
        return bool(res[0]) if whole else res

    def query(self, key: str) -> int:
        """ "workspace_bytes", "work_bytes", "last_launches", "products_miller", "products_product_step", "products_final_exponentiation",
        "program_ops", "device", "curve", "block_lanes", "lane_bytes", "max_lanes", "serial_group" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_pairing_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_pairing_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HashToCurve:
    """Batch hash-to-curve on one GPU (mi355_msm_h2c_*): RFC 9380 for ``bls12_381_g1`` or ``bls12_381_g2`` with one domain separation
    tag -- arkworks' ``MapToCurveBasedHasher<_, DefaultFieldHasher<Sha256, 128>, WBMap<_>>``.  ``msgs`` is a list of ``bytes``, an
    ``(n, len)`` uint8 array or torch tensor (CPU or GPU), or a ``(data, offsets)`` pair (bytes and n + 1 offsets; on the GPU a uint8
    tensor and an int64 tensor).  GPU tensors in give a GPU tensor out on the current stream (``out=``: one to write into).  The points
    are arkworks ``Affine`` images (104 / 200 bytes a row; ``projective=True``: 144 / 288), ready for ``mul_points``, ``compress_points``
    and ``Pairing.check``.  Meant for short messages; both BLS12-377 curves are refused (no standard suite exists)."""

    def __init__(self, curve="bls12_381_g2", dst=b"", device: Optional[int] = None):
        self.curve = _curve_id(curve)
        self.handle = ctypes.c_void_p()
        self._lib = load_library()
        tag = dst.encode() if isinstance(dst, str) else bytes(dst)
        keep = ctypes.create_string_buffer(tag, len(tag)) if tag else None
        _check(self._lib.mi355_msm_h2c_create(ctypes.byref(self.handle), self.curve, ctypes.addressof(keep) if tag else None, len(tag),
                                              -1 if device is None else device))
        self.device = self.query("device")
        self.m = 2 if self.curve >= 2 else 1

    def _messages(self, msgs):
        """-> (data _Buf or None, offsets pointer, keep-alive, n, data bytes, on the GPU?, stream, torch device)"""
        if not self.handle:
            raise MsmError(-1, "the hash-to-curve handle is closed")
        import numpy as np

        if isinstance(msgs, tuple) and len(msgs) == 2:
            data, off = msgs
            if hasattr(off, "is_cuda") and off.is_cuda:
                import torch

                if off.dtype != torch.int64 or off.dim() != 1 or off.numel() < 1 or not off.is_contiguous():
                    raise ValueError("offsets on the GPU: a contiguous 1-D int64 tensor of n + 1 entries")
                d = _Buf(data)
                if not d.is_device or d.device_index != self.device or off.device.index != self.device:
                    raise MsmError(-1, f"data and offsets must both live on device {self.device}")
                return d, off.data_ptr(), off, off.numel() - 1, d.nbytes, True, d.stream, d.keep.device
            off = np.ascontiguousarray(np.asarray(off.cpu() if hasattr(off, "cpu") else off), dtype=np.uint64)
            if off.ndim != 1 or off.size < 1:
                raise ValueError("offsets: n + 1 entries")
            d = _Buf(data.cpu() if hasattr(data, "cpu") else data)
            return d, off.ctypes.data, off, off.size - 1, d.nbytes, False, None, None
        if hasattr(msgs, "is_cuda") or hasattr(msgs, "__array_interface__"):
            if len(msgs.shape) != 2:
                raise ValueError("an array of messages has the shape (n, len)")
            n, ln = int(msgs.shape[0]), int(msgs.shape[1])
            d = _Buf(msgs)
            if d.is_device:
                import torch

                if d.device_index != self.device:
                    raise MsmError(-1, f"an input lives on cuda:{d.device_index} but this handle is bound to device {self.device}")
                off = torch.arange(n + 1, dtype=torch.int64, device=d.keep.device) * ln
                return d, off.data_ptr(), off, n, d.nbytes, True, d.stream, d.keep.device
            off = np.arange(n + 1, dtype=np.uint64) * np.uint64(ln)
            return d, off.ctypes.data, off, n, d.nbytes, False, None, None
        msgs = [bytes(x) for x in msgs]
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        d = _Buf(b"".join(msgs))
        return d, off.ctypes.data, off, len(msgs), d.nbytes, False, None, None

    def _output(self, rows, width, on_gpu, out, tdev):
        if on_gpu:
            import torch

            if out is None:
                out = torch.empty((rows, width), dtype=torch.uint8, device=tdev)
            ob = _Buf(out)
            if not ob.is_device or ob.keep is not out or ob.nbytes != rows * width:
                raise ValueError(f"out: a contiguous uint8 GPU tensor of {rows} x {width} bytes")
            return out, ob.ptr
        if out is not None:
            raise ValueError("out= goes with GPU tensors")
        import numpy as np

        res = np.zeros((rows, width), dtype=np.uint8)
        return res, res.ctypes.data

    def _image(self, projective):
        return 144 * self.m if projective else 96 * self.m + 8

    def _hash(self, msgs, flags, projective, out):
        d, off, keep, n, nbytes, gpu, stream, tdev = self._messages(msgs)
        width = self._image(projective)
        res, ptr = self._output(n, width, gpu, out, tdev)
        _check(self._lib.mi355_msm_h2c_hash(self.handle, ptr if n else None, width, d.ptr if nbytes else None, nbytes, off, n,
                                            flags | (8 if projective else 0) | (2 if gpu else 0), stream))
        del keep
        return res

    def hash(self, msgs, projective: bool = False, out=None):
        """``hash_to_curve``: one point of the order-r subgroup per message, shape ``(n, image bytes)`` uint8"""
        return self._hash(msgs, 0, projective, out)

    def encode(self, msgs, projective: bool = False, out=None):
        """``encode_to_curve`` (the non-uniform ``_NU_`` suite): one u per message"""
        return self._hash(msgs, 1, projective, out)

    def hash_to_field(self, msgs, count: int = 2, out=None):
        """``count`` (1 or 2) elements of the base field per message: shape ``(n * count, 48 m)`` uint8, Montgomery images"""
        if count not in (1, 2):
            raise ValueError("count is 1 or 2")
        d, off, keep, n, nbytes, gpu, stream, tdev = self._messages(msgs)
        res, ptr = self._output(n * count, 48 * self.m, gpu, out, tdev)
        _check(self._lib.mi355_msm_h2c_field(self.handle, ptr if n else None, d.ptr if nbytes else None, nbytes, off, n, count, 2 if gpu else 0, stream))
        del keep
        return res

    def map_to_curve(self, u, pairs: bool = False, projective: bool = False, out=None):
        """``WBMap::map_to_curve`` of n field images (no cofactor clearing); ``pairs=True``: n / 2 points
        ``clear_cofactor(map(u[2j]) + map(u[2j + 1]))``"""
        if not self.handle:
            raise MsmError(-1, "the hash-to-curve handle is closed")
        b = _Buf(u)
        unit = 48 * self.m
        if b.nbytes % unit:
            raise ValueError(f"u: n images of {unit} bytes ({b.nbytes} bytes given)")
        n = b.nbytes // unit
        if pairs and n % 2:
            raise ValueError(f"{n} field images are not whole pairs")
        if b.is_device and b.device_index != self.device:
            raise MsmError(-1, f"an input lives on cuda:{b.device_index} but this handle is bound to device {self.device}")
        width = self._image(projective)
        res, ptr = self._output(n // 2 if pairs else n, width, b.is_device, out, b.keep.device if b.is_device else None)
        _check(self._lib.mi355_msm_h2c_map(self.handle, ptr if n else None, width, b.ptr if n else None, n,
                                           (4 if pairs else 0) | (8 if projective else 0) | (2 if b.is_device else 0), b.stream))
        return res

    def query(self, key: str) -> int:
        """ "work_bytes", "lanes_in_flight", "last_launches", "device", "curve", "dst_bytes", "dst_oversize", "block_lanes", "max_lanes" """
        v = ctypes.c_uint64(0)
        _check(self._lib.mi355_msm_h2c_query(self.handle, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def close(self) -> None:
        if self.handle:
            _check(self._lib.mi355_msm_h2c_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FixedBase:
    """Shape of arkworks' ``FixedBase`` (ARK ec/src/msm/fixed_base.rs:8-97)."""

    @staticmethod
    def get_mul_window_size(num_scalars: int) -> int:
        """arkworks' rule (3 below 32 scalars, else ``ln_without_floats``), for API parity: a CPU cache heuristic that no table here
        uses -- ``WindowTable.query("window_bits")`` says what one does."""
        return int(load_library().mi355_msm_fixed_window_size(int(num_scalars)))

    @staticmethod
    def get_window_table(g, curve="bls12_377_g1", window: int = 0, device: Optional[int] = None, expected_scalars: int = 0) -> WindowTable:
        return WindowTable(g, curve=curve, window=window, device=device, expected_scalars=expected_scalars)

    @staticmethod
    def msm(table: WindowTable, scalars, montgomery: bool = True, projective: bool = True):
        """``FixedBase::msm(.., table, v: &[ScalarField]) -> Vec<Projective>``: Fr images in, Projective images out by default."""
        return table.msm(scalars, montgomery=montgomery, projective=projective)


def fixed_base_msm(g, scalars, curve="bls12_377_g1", montgomery: bool = False, projective: bool = False):
    """One call: build the table of ``g`` for this many scalars, multiply, free the table.  Affine images of ``scalars[i] * g``."""
    nbytes = _Buf(scalars).nbytes
    if nbytes % SCALAR_BYTES:
        raise ValueError("scalars image is not a multiple of 32 bytes")
    with WindowTable(g, curve=curve, expected_scalars=max(nbytes // SCALAR_BYTES, 1)) as table:
        return table.msm(scalars, montgomery=montgomery, projective=projective)


def fold_partials(partials: Sequence[bytes], curve="bls12_377_g1") -> bytes:
    """Sum per-GPU partial results (projective images: 144 B for G1, 288 B for G2) into one normalised image."""
    lib = load_library()
    pb = projective_bytes(curve)
    blob = b"".join(bytes(p) for p in partials)
    if len(blob) % pb:
        raise ValueError(f"partials must be {pb}-byte projective images")
    out = ctypes.create_string_buffer(pb)
    buf = ctypes.create_string_buffer(blob, len(blob) if blob else 1)
    _check(lib.mi355_msm_fold(_curve_id(curve), out, buf, len(blob) // pb))
    return out.raw


def generate_points(npoints: int, distinct: int = 1 << 15, seed: int = 0x5A5052495A45, curve="bls12_377_g1"):
    """Synthetic bases in the reference generator's shape (P1A yrrid/src/util.rs:15-28): ``distinct`` subgroup points
    replicated by doubling up to ``npoints``; returns a NumPy uint8 array of shape (npoints, stride) (stride 104, G2: 200)."""
    import numpy as np

    lib = load_library()
    stride = affine_stride(curve)
    out = np.zeros((npoints, stride), dtype=np.uint8)
    _check(lib.mi355_msm_generate_points(_curve_id(curve), seed, distinct, npoints, out.ctypes.data, stride))
    return out


class MsmJob:
    """A run in flight (MultiScalarMultContext.run_async).  Keeps the scalars and the output buffer alive until it is waited for."""

    def __init__(self, lib, handle, out, pb, batches, keep):
        self._lib, self._handle, self._out, self._pb, self._batches, self._keep = lib, handle, out, pb, batches, keep
        self._result = None

    def done(self) -> bool:
        return self._handle is None or bool(self._lib.mi355_msm_job_done(self._handle))

    def wait(self) -> List[bytes]:
        if self._handle is not None:
            h, self._handle = self._handle, None
            _check(self._lib.mi355_msm_job_wait(h))      # (releases the handle, whatever the status)
            raw = self._out.raw
            self._result = [raw[i * self._pb:(i + 1) * self._pb] for i in range(self._batches)]
            self._keep = None
        if self._result is None:
            raise MsmError(-1, "this job failed (its error was raised by the first wait())")
        return self._result

    def __del__(self):
        try:
            if self._handle is not None:
                self.wait()
        except Exception:
            pass


def plan(npoints: int, curve="bls12_377_g1", precompute: bool = False, window_bits: int = 0, lane_entries: int = 0,
         seg_entries: int = 0, table_levels: int = 0) -> dict:
    """The engine's execution plan for an MSM of ``npoints`` pairs (host arithmetic only; works without a GPU).
    ``precompute`` with ``table_levels`` = k > 1 plans what a context with those two options runs (k levels, ceil(windows / k)
    bucket sets); ``table_levels`` = 0 is a level per window."""
    lib = load_library()
    opts = (ctypes.c_long * 3)(window_bits, lane_entries, seg_entries)
    out = (ctypes.c_uint64 * 10)()
    if table_levels == 1:
        raise ValueError("table_levels = 1 is no table at all: pass precompute=False")
    _check(lib.mi355_msm_plan(_curve_id(curve), npoints, (table_levels if table_levels > 1 else 1) if precompute else 0, opts, out))
    names = ("window_bits", "windows", "bucket_windows", "entries", "lane_entries", "lanes", "merge_launches", "reduce_launches",
             "key_bits", "work_bytes")
    return {k: int(out[i]) for i, k in enumerate(names)}
