"""A big-integer model of RFC 9380 hash-to-curve for BLS12-381 G1 and G2, written from the RFC's definitions: hashlib SHA-256 for
expand_message_xmd (section 5.3.1, with the oversize-DST rule of 5.3.3), hash_to_field (5.2), the non-optimised simplified SWU of
section 6.6.2, Velu's isogeny as its sums, and cofactor clearing as the plain multiple by h_eff.  It shares nothing with csrc/h2c.hpp.
It is NOT independent of tools/gen_h2c_consts.py, the program that writes the kernels' constants: the field, the curve arithmetic, the
SWU map, the kernel of the isogeny and Velu's sums are that module's.  What ties both to the outside are the RFC's vectors
(tests/test_h2c_model.py: every u, Q0, Q1 and P) and, for the polynomials the kernels evaluate, their comparison with the sums in
tests/test_h2c_consts.py.  Field elements are tuples of m integers, points are (x, y) or None."""
import hashlib
import json
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_h2c_consts as gen  # noqa: E402

P = gen.P
GOLDEN = os.path.join(ROOT, "tests", "golden", "h2c")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "h2c_kat_bls12_381.json")))
H_EFF = {g: int(KAT[g]["h_eff"], 16) for g in ("g1", "g2")}
CURVES = {"g1": "bls12_381_g1", "g2": "bls12_381_g2"}
L = 64

_suites = {}


def suite(group):
    """(Suite, derived isogeny), computed once."""
    if group not in _suites:
        S = gen.Suite(group)
        _suites[group] = (S, gen.derive(S))
    return _suites[group]


def fixture(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def dst_prime(dst: bytes) -> bytes:
    if len(dst) > 255:
        dst = hashlib.sha256(b"H2C-OVERSIZE-DST-" + dst).digest()
    return dst + bytes([len(dst)])


def expand_message_xmd(msg: bytes, dst: bytes, n: int) -> bytes:
    ell = (n + 31) // 32
    assert ell <= 255 and n <= 65535
    dp = dst_prime(dst)
    b0 = hashlib.sha256(bytes(64) + msg + n.to_bytes(2, "big") + b"\0" + dp).digest()
    b = [hashlib.sha256(b0 + b"\1" + dp).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dp).digest())
    return b"".join(b)[:n]


def hash_to_field(group, msg: bytes, dst: bytes, count: int = 2):
    m = suite(group)[0].F.m
    ub = expand_message_xmd(msg, dst, count * m * L)
    return [tuple(int.from_bytes(ub[L * (j + i * m):L * (j + i * m + 1)], "big") % P for j in range(m)) for i in range(count)]


def map_to_curve(group, u):
    S, iso = suite(group)
    return gen.isogeny(S, iso, gen.sswu(S, u))


def add(group, a, b):
    F = suite(group)[0].F
    return gen.ec_add(F, F.zero, a, b)


def mul(group, k, a):
    F = suite(group)[0].F
    return gen.ec_mul(F, F.zero, k, a)


def neg(group, a):
    return gen.ec_neg(suite(group)[0].F, a)


def clear_cofactor(group, a):
    return mul(group, H_EFF[group], a)


def map_pair(group, u0, u1):
    return clear_cofactor(group, add(group, map_to_curve(group, u0), map_to_curve(group, u1)))


def hash_to_curve(group, msg: bytes, dst: bytes):
    u = hash_to_field(group, msg, dst, 2)
    return map_pair(group, u[0], u[1])


def encode_to_curve(group, msg: bytes, dst: bytes):
    return clear_cofactor(group, map_to_curve(group, hash_to_field(group, msg, dst, 1)[0]))


def on_curve(group, a):
    S, _ = suite(group)
    F = S.F
    return a is None or F.sqr(a[1]) == F.add(F.mul(F.sqr(a[0]), a[0]), S.B_E)


def parse_el(group, text):
    F = suite(group)[0].F
    return F.el(*[int(c, 16) for c in text.split(",")])


def parse_point(group, d):
    return (parse_el(group, d["x"]), parse_el(group, d["y"]))


# ---- the library's images: twelve 32-bit words of x 2^384 mod p per Fp component, c0 first ------------------------------------------
R384 = 1 << 384


def el_image(a) -> bytes:
    return b"".join((c * R384 % P).to_bytes(48, "little") for c in a)


def el_from_image(b: bytes):
    inv = pow(R384, -1, P)
    return tuple(int.from_bytes(b[i:i + 48], "little") * inv % P for i in range(0, len(b), 48))


def affine_image(group, a, stride) -> bytes:
    """x, y, then the infinity flag byte, padded to the stride (the Affine record of the library)."""
    m = suite(group)[0].F.m
    if a is None:
        body = bytes(96 * m) + b"\1"
    else:
        body = el_image(a[0]) + el_image(a[1]) + b"\0"
    return body + bytes(stride - len(body))


def point_from_image(group, b: bytes):
    m = suite(group)[0].F.m
    if b[96 * m]:
        return None
    return (el_from_image(b[:48 * m]), el_from_image(b[48 * m:96 * m]))


def random_messages(n, seed, lengths=None):
    """n messages of lengths 0 .. 200; the first ones have the lengths that put the SHA-256 padding of b_0 on each side of a
    block boundary for a 43-byte DST (the caller may pass others)."""
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = lengths[i] if lengths and i < len(lengths) else rng.randrange(201)
        out.append(bytes(rng.randrange(256) for _ in range(ln)))
    return out


def boundary_lengths(dst_len):
    """Message lengths at which 64 + len + 3 + dst_len + 1 is 55, 56, 63, 0 (mod 64): the padding of b_0 fits, spills, ..."""
    tail = 64 + 3 + min(dst_len, 255 if dst_len <= 255 else 32) + 1
    if dst_len > 255:
        tail = 64 + 3 + 32 + 1
    return [(r - tail) % 64 for r in (55, 56, 63, 0)] + [(r - tail) % 64 + 64 for r in (55, 56, 63, 0)]


# ---- the host build of csrc/h2c.hpp (libmsm_hosttest.so, ht_h2c_*) ----------------------------------------------------------------------
import ctypes  # noqa: E402

PKG = os.path.join(ROOT, "2022-entries_amd")
GROUP_ID = {"g1": 0, "g2": 1}
STRIDE = {"g1": 104, "g2": 200}
_HT = None


def hosttest():
    global _HT
    if _HT is None:
        _HT = ctypes.CDLL(os.path.join(PKG, "libmsm_hosttest.so"))
        _HT.ht_check_failures.restype = ctypes.c_long
        cp, sz, ci, cu = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
        _HT.ht_h2c_sha256.argtypes = [cp, sz, cp]
        _HT.ht_h2c_dst.argtypes = [cp, sz, cp, cp]
        _HT.ht_h2c_reduce.argtypes = [cp, sz, cp]
        _HT.ht_h2c_check_offsets.argtypes = [cp, sz, sz, cp, sz]
        _HT.ht_h2c_field.argtypes = [ci, cp, sz, cp, sz, cp, sz, cu, cp]
        _HT.ht_h2c_map.argtypes = [ci, cp, sz, cu, cp, sz]
        _HT.ht_h2c_clear.argtypes = [ci, ci, cp, sz, sz, cp, sz, cp, sz]
        _HT.ht_h2c_sqrt_ratio.argtypes = [ci, cp, cp, cp]
        _HT.ht_h2c_iso.argtypes = [ci, cp, cp, cp, cp, sz]
    return _HT


def pack(msgs):
    """(data, offsets as n + 1 little-endian 64-bit integers)"""
    off, at = [0], 0
    for m in msgs:
        at += len(m)
        off.append(at)
    return b"".join(msgs), b"".join(o.to_bytes(8, "little") for o in off)


def host_sha256(data: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    assert hosttest().ht_h2c_sha256(data, len(data), out) == 0
    return out.raw


def host_dst(dst: bytes):
    prime, z = ctypes.create_string_buffer(256), ctypes.create_string_buffer(32)
    n = hosttest().ht_h2c_dst(dst, len(dst), prime, z)
    assert n > 0
    return prime.raw[:n], z.raw


def host_reduce(strings) -> bytes:
    """the reduction of hash_to_field on raw 64-byte big-endian strings: one 48-byte image each"""
    assert all(len(x) == 64 for x in strings)
    out = ctypes.create_string_buffer(48 * len(strings))
    assert hosttest().ht_h2c_reduce(b"".join(strings), len(strings), out) == 0
    return out.raw


def host_check_offsets(offsets, data_bytes):
    msg = ctypes.create_string_buffer(128)
    raw = b"".join(o.to_bytes(8, "little") for o in offsets)
    rc = hosttest().ht_h2c_check_offsets(raw, len(offsets) - 1, data_bytes, msg, 128)
    return rc, msg.value.decode()


def host_field(group, msgs, dst, count=2) -> bytes:
    data, off = pack(msgs)
    m = suite(group)[0].F.m
    out = ctypes.create_string_buffer(max(1, len(msgs) * count * m * 48))
    assert hosttest().ht_h2c_field(GROUP_ID[group], dst, len(dst), data, len(data), off, len(msgs), count, out) == 0
    return out.raw[:len(msgs) * count * m * 48]


def host_map(group, u_images: bytes, flags=0, stride=None) -> bytes:
    m = suite(group)[0].F.m
    n = len(u_images) // (48 * m)
    proj = bool(flags & 8)
    stride = stride or (144 * m if proj else STRIDE[group])
    outs = n // 2 if flags & 4 else n
    out = ctypes.create_string_buffer(max(1, outs * stride))
    assert hosttest().ht_h2c_map(GROUP_ID[group], u_images, n, flags, out, stride) == 0
    return out.raw[:outs * stride]


def host_hash(group, msgs, dst, encode=False, flags=0) -> bytes:
    u = host_field(group, msgs, dst, 1 if encode else 2)
    return host_map(group, u, (1 if encode else 4) | flags)


def host_clear(group, images: bytes, k: int = None) -> bytes:
    s = STRIDE[group]
    n = len(images) // s
    out = ctypes.create_string_buffer(max(1, n * s))
    kb = k.to_bytes((k.bit_length() + 7) // 8, "little") if k is not None else None
    assert hosttest().ht_h2c_clear(GROUP_ID[group], 0 if k is None else 1, images, s, n, kb, len(kb) if kb else 0, out, s) == 0
    return out.raw[:n * s]


def host_sqrt_ratio(group, u, v):
    m = suite(group)[0].F.m
    y = ctypes.create_string_buffer(48 * m)
    sq = hosttest().ht_h2c_sqrt_ratio(GROUP_ID[group], el_image(u), el_image(v), y)
    return bool(sq), el_from_image(y.raw)


def host_iso(group, xn, xd, y):
    out = ctypes.create_string_buffer(STRIDE[group])
    assert hosttest().ht_h2c_iso(GROUP_ID[group], el_image(xn), el_image(xd), el_image(y), out, STRIDE[group]) == 0
    return point_from_image(group, out.raw)


def images(group, pts) -> bytes:
    return b"".join(affine_image(group, p, STRIDE[group]) for p in pts)


def points(group, raw: bytes):
    s = STRIDE[group]
    return [point_from_image(group, raw[i:i + s]) for i in range(0, len(raw), s)]


def u_images(us) -> bytes:
    return b"".join(el_image(u) for u in us)
