"""Big-integer model of Poseidon over BLS12-377 Fr and BLS12-381 Fr for the tests of csrc/poseidon.hpp: the Grain LFSR and the rule by
which snarkVM derives round constants and the MDS matrix, the duplex sponge of console/algorithms/src/poseidon/helpers/sponge.rs,
hash_many, and the Poseidon Merkle tree of console/collections/src/merkle_tree.  tests/golden/poseidon holds, in one archive, snarkVM's recorded results
for BLS12-377 (14 parameter files, 100 sponge transcripts at rate 2, two samples of the generator); the model reproduces all of them
(tests/test_poseidon_golden.py), which is what makes it an oracle for the other rates, the other field and other parameters."""
import functools
import os
import random
import re
import tarfile

import ntt_cases as nc

# snarkVM's resources/ directory (test_parameters, test_sponge, test_grain_lfsr: 116 .snap files), every file unchanged, in one archive
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon", "snarkvm_poseidon_resources.tar.gz")
SNARKVM = dict(alpha=17, full_rounds=8, partial_rounds=31)     # every rate of BLS12-377
SPONGE_INPUT = 1237812                                         # the element the recorded transcripts absorb, `absorb` times
ALT_381 = dict(alpha=5, full_rounds=6, partial_rounds=11)      # a second parameter set, on BLS12-381


@functools.lru_cache(maxsize=None)
def _resources():
    with tarfile.open(GOLDEN) as tf:
        return {m.name: tf.extractfile(m).read().decode() for m in tf.getmembers()}


def snapshot(*path):
    """the integers of a snapshot file, nested as recorded"""
    text = _resources()["/".join(path)].strip().replace("field", "")
    assert re.fullmatch(r"[\[\]0-9, ]*", text), path
    return eval(text, {"__builtins__": {}})       # brackets, digits and commas only


class GrainLFSR:
    def __init__(self, bits, t, full_rounds, partial_rounds):
        self.bits = bits
        s = [0, 1] + [0] * 4
        for value, width in ((bits, 12), (t, 12), (full_rounds, 10), (partial_rounds, 10)):
            s += [(value >> (width - 1 - i)) & 1 for i in range(width)]
        s += [1] * 30
        assert len(s) == 80
        self.s = s
        for _ in range(160):
            self.step()

    def step(self):
        s = self.s
        b = s[62] ^ s[51] ^ s[38] ^ s[23] ^ s[13] ^ s[0]
        self.s = s[1:] + [b]
        return b

    def word(self):
        """`bits` bits, most significant first: of every pair, the second is kept when the first is 1"""
        v = 0
        for _ in range(self.bits):
            while not self.step():
                self.step()
            v = (v << 1) | self.step()
        return v

    def sample(self, p):
        while True:
            v = self.word()
            if v < p:
                return v


@functools.lru_cache(maxsize=None)
def parameters(field, rate, alpha=17, full_rounds=8, partial_rounds=31, skip_matrices=0):
    """(ark, mds) as lists of rows of integers"""
    p = nc.modulus(field)
    t = rate + 1
    g = GrainLFSR(p.bit_length(), t, full_rounds, partial_rounds)
    ark = [[g.sample(p) for _ in range(t)] for _ in range(full_rounds + partial_rounds)]
    for _ in range(skip_matrices * 2 * t):
        g.word()
    xs = [g.word() % p for _ in range(t)]
    ys = [g.word() % p for _ in range(t)]
    mds = [[pow(x + y, p - 2, p) for y in ys] for x in xs]
    return ark, mds


def permute(p, state, ark, mds, alpha, full_rounds, partial_rounds):
    t = len(state)
    h = full_rounds // 2
    for r in range(full_rounds + partial_rounds):
        state = [(s + c) % p for s, c in zip(state, ark[r])]
        if h <= r < h + partial_rounds:
            state[0] = pow(state[0], alpha, p)
        else:
            state = [pow(s, alpha, p) for s in state]
        state = [sum(m * s for m, s in zip(mds[i], state)) % p for i in range(t)]
    return state


class Model:
    """one parameter set over one field"""

    def __init__(self, field, rate, ark, mds, alpha=17, full_rounds=8, partial_rounds=31):
        self.field, self.p, self.rate = field, nc.modulus(field), rate
        self.ark, self.mds, self.alpha, self.full_rounds, self.partial_rounds = ark, mds, alpha, full_rounds, partial_rounds

    @classmethod
    def generated(cls, field, rate, **kw):
        ark, mds = parameters(field, rate, **kw)
        kw.pop("skip_matrices", None)
        return cls(field, rate, ark, mds, **kw)

    def permute(self, state):
        return permute(self.p, state, self.ark, self.mds, self.alpha, self.full_rounds, self.partial_rounds)

    def sponge(self, inputs, n_out):
        """absorb(inputs) then squeeze(n_out), with the duplex rules of the reference"""
        rate, p = self.rate, self.p
        state = [0] * (rate + 1)
        idx = 0
        for x in inputs:
            if idx == rate:
                state = self.permute(state)
                idx = 0
            state[1 + idx] = (state[1 + idx] + x) % p
            idx += 1
        out = []
        idx = rate
        for _ in range(n_out):
            if idx == rate:
                state = self.permute(state)
                idx = 0
            out.append(state[1 + idx])
            idx += 1
        return out

    def header(self, domain, length):
        return [domain % self.p, length] + [0] * (self.rate - 2)

    def hash_many(self, domain, inputs, n_out):
        return self.sponge(self.header(domain, len(inputs)) + list(inputs), n_out)

    def hash(self, domain, inputs):
        return self.hash_many(domain, inputs, 1)[0]

    def merkle(self, domain, leaves):
        """the 2P - 1 nodes in the reference's order and the empty hash"""
        n = len(leaves)
        P = 1
        while P < n:
            P *= 2
        empty = self.hash(domain, [1, 0, 0])
        tree = [empty] * (2 * P - 1)
        for i, leaf in enumerate(leaves):
            tree[P - 1 + i] = self.hash(domain, [0] + list(leaf))
        for i in range(P - 2, -1, -1):
            tree[i] = self.hash(domain, [1, tree[2 * i + 1], tree[2 * i + 2]])
        return tree, empty

    def merkle_root(self, domain, tree, empty, depth):
        levels = (len(tree) + 1).bit_length() - 2          # the depth of the built part
        root = tree[0]
        for _ in range(depth - levels):
            root = self.hash(domain, [1, root, empty])
        return root

    @staticmethod
    def merkle_path(tree, i):
        P = (len(tree) + 1) // 2
        idx = P - 1 + i
        path = []
        while idx:
            path.append(tree[idx + 1 if idx & 1 else idx - 1])
            idx = (idx - 1) // 2
        return path


def domain_element(text, p):
    """snarkVM's Field::new_domain_separator: the bytes of the string, little-endian, mod p"""
    return int.from_bytes(text.encode(), "little") % p


def encode(field, values, montgomery):
    """integers -> canonical 32-byte elements in the form of a call"""
    return nc.encode(field, values, not montgomery)


def decode(field, raw, montgomery):
    """32-byte elements (any 256-bit value) -> the integers they stand for"""
    return nc.decode(field, bytes(raw), not montgomery)


def raw_words(values):
    """256-bit values as they are, not reduced: what decode() reads as their residue"""
    return b"".join(v.to_bytes(32, "little") for v in values)


def edge_words(field):
    p = nc.modulus(field)
    return [0, p - 1, p, (1 << 256) - 1]


def flat(rows):
    return [v for row in rows for v in row]


# the shapes at which the sponge takes another path: nothing, one element, one below, at and one above a rate block, two blocks and one
def in_lens(rate):
    return sorted({0, 1, rate - 1, rate, rate + 1, 2 * rate + 1})


def out_lens(rate):
    return sorted({1, rate, rate + 1, 2 * rate + 1})


def host_lib(root):
    """libmsm_hosttest.so with the ht_poseidon_* entry points declared"""
    import ctypes

    lib = ctypes.CDLL(os.path.join(root, "2022-entries_amd", "libmsm_hosttest.so"))
    ci, cu, cp, u64 = ctypes.c_int, ctypes.c_uint, ctypes.c_char_p, ctypes.c_uint64
    lib.ht_poseidon_hash.argtypes = [ci, cu, cu, cu, cu, cu, cu, cp, cp, ci, u64, cu, cu, cp, cp, cp]
    lib.ht_poseidon_merkle.argtypes = [ci, cu, cu, cu, cu, cu, cu, cp, cp, ci, u64, cu, cp, cp, cp]
    lib.ht_poseidon_permute.argtypes = [ci, cu, cu, cu, cu, cu, cp, cp, ci, cp, cp, ctypes.POINTER(u64)]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def host_hash(lib, m, rows, n_out, montgomery=True, sparse=1, header=None, raw=None):
    """rows of integers (or `raw`, the bytes as they are) through the host build: a list of rows of residues"""
    import ctypes

    n, in_len = len(rows), len(rows[0]) if rows else 0
    out = ctypes.create_string_buffer(max(n * n_out * 32, 1))
    rc = lib.ht_poseidon_hash(nc.FIELD_IDS[m.field], 1, 0 if montgomery else 1, m.rate, m.alpha, m.full_rounds, m.partial_rounds,
                              encode(m.field, flat(m.ark), False), encode(m.field, flat(m.mds), False), sparse, n, in_len, n_out,
                              encode(m.field, header, montgomery) if header else None,
                              raw if raw is not None else encode(m.field, flat(rows), montgomery), out)
    assert rc == 0, rc
    got = decode(m.field, out.raw[:n * n_out * 32], montgomery)
    return [got[i * n_out:(i + 1) * n_out] for i in range(n)], out.raw[:n * n_out * 32]
