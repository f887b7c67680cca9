"""Big-integer model of the radix-2 domains (arkworks' Radix2EvaluationDomain over BLS12-377 Fr and BLS12-381 Fr) for the tests of
csrc/fr.hpp and csrc/ntt.hpp: an iterative NTT, the direct O(n^2) evaluation that pins it, and the 32-byte element forms.

Elements cross the ABI as 32 little-endian bytes: an arkworks image (a * 2^256 mod r) by default, the plain integer with the
normal-form flag.  Any 256-bit input stands for its residue; every output is canonical."""
import random

FIELDS = {
    # name: (r, multiplicative generator, 2-adicity)
    "bls12_377": (8444461749428370424248824938781546531375899335154063827935233455917409239041, 22, 47),
    "bls12_381": (52435875175126190479447740508185965837690552500527637822603658699938581184513, 7, 32),
}
FIELD_IDS = {"bls12_377": 0, "bls12_381": 1}
FIELD_OF_CURVE = {"bls12_377_g1": "bls12_377", "bls12_381_g1": "bls12_381", "bls12_377_g2": "bls12_377", "bls12_381_g2": "bls12_381"}
FORWARD, INVERSE, COSET_FORWARD, COSET_INVERSE = 0, 1, 2, 3
FLAG_NORMAL, FLAG_NR, FLAG_RN = 1, 2, 4
MONT = 1 << 256


def modulus(field):
    return FIELDS[field][0]


def generator(field):
    return FIELDS[field][1]


def two_adic_root(field):
    r, g, s = FIELDS[field]
    return pow(g, (r - 1) >> s, r)


def root_of_unity(field, k):
    """get_root_of_unity(2^k): the two-adic root squared s - k times"""
    r, _, s = FIELDS[field]
    assert k <= s
    return pow(two_adic_root(field), 1 << (s - k), r)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def ntt(values, omega, r):
    """sum_j values[j] * omega^(i j) for every i: iterative decimation in time, natural order in and out"""
    n = len(values)
    k = n.bit_length() - 1
    assert 1 << k == n
    a = [values[bitrev(i, k)] for i in range(n)]
    size = 2
    while size <= n:
        w_step = pow(omega, n // size, r)
        half = size // 2
        tw = [1] * half
        for i in range(1, half):
            tw[i] = tw[i - 1] * w_step % r
        for start in range(0, n, size):
            for i in range(half):
                u, v = a[start + i], a[start + i + half] * tw[i] % r
                a[start + i], a[start + i + half] = (u + v) % r, (u - v) % r
        size *= 2
    return a


def dft_direct(values, omega, r):
    n = len(values)
    return [sum(v * pow(omega, i * j, r) for j, v in enumerate(values)) % r for i in range(n)]


def transform(field, k, kind, values, offset=None, order_flags=0):
    """The four calls on integers (normal form), `values` shorter than 2^k is zero-extended.  FLAG_NR: the forward result in
    bit-reversed order; FLAG_RN: the inverse input in bit-reversed order."""
    r = modulus(field)
    n = 1 << k
    g = generator(field) if offset is None else offset % r
    x = [v % r for v in values] + [0] * (n - len(values))
    assert len(x) == n
    omega = root_of_unity(field, k)
    if order_flags & FLAG_RN:
        x = [x[bitrev(i, k)] for i in range(n)]
    if kind == COSET_FORWARD:
        x = [v * pow(g, j, r) % r for j, v in enumerate(x)]
    if kind in (FORWARD, COSET_FORWARD):
        y = ntt(x, omega, r)
    else:
        ninv = pow(n, -1, r)
        y = [v * ninv % r for v in ntt(x, pow(omega, -1, r), r)]
        if kind == COSET_INVERSE:
            ginv = pow(g, -1, r)
            y = [v * pow(ginv, j, r) % r for j, v in enumerate(y)]
    if order_flags & FLAG_NR:
        y = [y[bitrev(i, k)] for i in range(n)]
    return y


def encode(field, values, normal):
    """integers -> canonical 32-byte elements"""
    r = modulus(field)
    f = 1 if normal else MONT
    return b"".join((v * f % r).to_bytes(32, "little") for v in values)


def decode(field, raw, normal):
    """32-byte elements (any 256-bit value) -> the integers they stand for"""
    r = modulus(field)
    f = 1 if normal else pow(MONT, -1, r)
    return [int.from_bytes(raw[i:i + 32], "little") * f % r for i in range(0, len(raw), 32)]


def oracle_ntt(lib, field, k, kind, flags, raw, in_len=None, offset=None, threads=0):
    """One vector through the CPU oracle's NTT (oracle/ntt_oracle.c; `lib` is the `oracle` fixture): `raw` is bytes or a NumPy uint8
    array of in_len (default: all of it) elements, `offset` 32 bytes in the form of the call or None for the generator.  Returns a
    NumPy uint8 array of shape (2^k, 32).  threads 0: as many as there are CPUs (the oracle stops at 16)."""
    import ctypes
    import os

    import numpy as np

    lib.oracle_ntt.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_void_p, ctypes.c_int]
    lib.oracle_ntt.restype = ctypes.c_int
    if isinstance(raw, (bytes, bytearray)):
        raw = np.frombuffer(raw, dtype=np.uint8)
    raw = np.ascontiguousarray(raw).reshape(-1)
    assert raw.dtype == np.uint8 and raw.size % 32 == 0
    in_len = raw.size // 32 if in_len is None else in_len
    assert in_len * 32 <= raw.size
    out = np.empty((1 << k, 32), dtype=np.uint8)
    rc = lib.oracle_ntt(FIELD_IDS[field], k, kind, flags, offset, raw.ctypes.data if in_len else None, in_len, out.ctypes.data,
                        threads or min(16, os.cpu_count() or 1))
    assert rc == 0, (field, k, kind, flags, in_len)
    return out


def edge_values(field):
    r = modulus(field)
    return [0, 1, r - 1, r, r + 1, (1 << 256) - 1]


def random_values(field, n, seed):
    rng = random.Random(seed)
    r = modulus(field)
    return [rng.randrange(r) for _ in range(n)]
