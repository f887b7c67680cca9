"""Helpers shared by the tests of the transforms over curve points (csrc/group_fft.hpp, mi355_msm_fft_points).

Discrete-log oracle, as in distinct_cases.py.  When in[j] = h_j * G for known h_j (G the generator of the order-r subgroup), a
transform of the points is the image of the transform of the logs over Fr,

    out[i] = sum_j c_ij * (h_j * G) = ((sum_j c_ij h_j) mod r) * G,

so the expected output is (ntt_cases.transform of h) * G for k <= 12 and (the CPU oracle's oracle_ntt of h) * G above: exact, byte
for byte, on every output.  The multiples of G come from the Python model (host tests) or from the fixed-base entry on the GPU
(GPU tests; FixedBase shares no code with the transform but the field arithmetic and is pinned by test_gpu_fixed_base.py).
Nothing here needs a GPU to import."""
import functools

import numpy as np

import distinct_cases as dc
import fixed_base_cases as fc
import ntt_cases as nc
import pymodel as pm

CURVE_NAMES = fc.CURVE_NAMES
KINDS = (nc.FORWARD, nc.INVERSE, nc.COSET_FORWARD, nc.COSET_INVERSE)
PY_MAX_LOG = 12          # ntt_cases.transform (Python integers) up to here, oracle_ntt above
OTHER_OFFSET = 0x5EED0FF5E7   # a coset offset that is not the GENERATOR


def field(name):
    return nc.FIELD_OF_CURVE[name]


def random_logs(name, n, seed):
    return nc.random_values(field(name), n, seed)


def log2(n):
    k = n.bit_length() - 1
    assert 1 << k == n
    return k


def transform_logs(name, n, kind, logs, offset=None, oracle=None):
    """the transform of the logs (zero-extended to n) as integers below r"""
    k = log2(n)
    if k <= PY_MAX_LOG:
        return nc.transform(field(name), k, kind, logs, offset)
    assert oracle is not None
    raw = words(logs).view(np.uint8).reshape(-1)
    off = None if offset is None else (offset % nc.modulus(field(name))).to_bytes(32, "little")
    out = nc.oracle_ntt(oracle, field(name), k, kind, nc.FLAG_NORMAL, raw, in_len=len(logs), offset=off)
    return out


def words(ints):
    """integers below 2^256 -> (n, 4) uint64, the scalar image the fixed-base entry reads"""
    if isinstance(ints, np.ndarray):
        return np.ascontiguousarray(ints).view(np.uint64).reshape(-1, 4)
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


@functools.lru_cache(maxsize=None)
def generator_expect(name):
    """k * G through the Python model, memoised"""
    curve = pm.CURVES[name]
    return fc.Expect(curve, curve.generator())


def model_images(name, logs, projective=False):
    """(h * G for h in logs) as Affine (Projective) images by the Python model"""
    exp = generator_expect(name)
    r = pm.CURVES[name].r
    ks = [h % r for h in logs]
    return exp.projective(ks) if projective else exp.affine(ks)


def device_images(ea, name, logs, projective=False):
    """(h * G for h in logs) as a GPU tensor of images, by the fixed-base entry"""
    import torch

    curve = pm.CURVES[name]
    w = words(logs)
    if len(w) == 0:
        return torch.zeros((0, curve.projective_bytes if projective else curve.affine_stride), dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(dc.as_bytes(w).reshape(-1).copy()).cuda()
    with ea.FixedBase.get_window_table(dc.generator_image(curve), curve=name, expected_scalars=len(w)) as table:
        return table.msm(d, projective=projective)


def infinity_image(curve, projective=False):
    return curve.encode_projective_normalized(None) if projective else curve.encode_affine(None)
