"""Whole Groth16 proofs as Python integers: the reference of tests/test_gpu_groth16.py, judged on its own by
tests/test_groth16_reference.py.  Nothing here comes from the code under test and nothing needs a GPU to import.

A discrete-log oracle for a whole proof.  The test chooses the toxic waste tau, alpha, beta, gamma, delta itself, so every element of
the CRS is a known multiple of a generator, and so is every element of a proof: with L_j = L_j(tau) the Lagrange basis of the domain
(sparse_cases.lagrange_at), n constraints, size = 2^k and

    u_i = sum_j L_j A[j][i]  (+ L_{n+i} for i < num_inputs),    v_i = sum_j L_j B[j][i],    w_i = sum_j L_j C[j][i],
    t = tau^size - 1,    lq_i = beta u_i + alpha v_i + w_i,

the CRS holds, as logs (scalars of the generators of G1 and G2),

    a_query[i] = u_i     b_g1_query[i] = b_g2_query[i] = v_i     l_query[i] = lq_i / delta (i >= num_inputs)
    gamma_abc[i] = lq_i / gamma (i < num_inputs)                  h_query[j] = tau^j t / delta (j < size - 1)

and the proof of an assignment z with randomizers r_, s_ is

    a = alpha + sum z_i u_i + r_ delta        b = beta + sum z_i v_i + s_ delta
    c = (sum_{i >= num_inputs} z_i lq_i + h(tau) t) / delta + s_ a + r_ b - r_ s_ delta

with h(tau) = ((sum L_j a_j)(sum L_j b_j) - sum L_j a_j b_j) / t from the padded vectors of R1cs.padded -- the quotient at ONE point,
which no transform computes.  A, B and C are then a G1, b G2 and c G1: Python integers give the log and one one-pair multiplication
by the CPU oracle gives the bytes (distinct_cases.oracle_mul).  The verifier in the exponent, with x = sum_{i < num_inputs} z_i lq_i /
gamma, is a b == alpha beta + x gamma + c delta (mod r).

The instances are circuits, not only assignments: every row's C is ONE entry on a private variable of its own (the row's output), which
occurs in no row of B and in A only in later rows, so a second assignment of the same A, B and C follows from fresh values of the other
variables, row by row (Instance.second_witness) -- the same CRS proves both."""
import bisect
import random

import ntt_cases as nc
import sparse_cases as sp

FAMILIES = ("bls12_377", "bls12_381")


class Instance(sp.R1cs):
    """n constraints over nvars variables, z[0] = 1, in the shape of sparse_cases.R1cs (field, n, nvars, num_inputs, z, A, B, C, a, b,
    padded), with the edges a prover's input has:

      * variables 0 .. num_inputs - 1 are public; the last of them has z = 0 (where there is one besides z[0] = 1);
      * then `free` private variables, then the n outputs, variable out(i) = num_inputs + free + i for row i;
      * the private values: 0, 1 and r - 1 are the first three free ones; of the others every second one lies in {0, 1} (an output: 1,
        since C divides by it), the rest are uniform and not 0;
      * self.no_a: two free variables and the last output occur in no row of A (those a_query points are infinity);
      * self.in_b: the only variables a row of B may use, fewer than a third of all (most of b_g1_query and b_g2_query is infinity);
      * self.dead: one free variable in no row of A, B or C (that l_query point is infinity).

    C[i] = [(a_i b_i / z[out(i)], out(i))], and a_i b_i != 0 in every row, so the coefficient is not 0 and the output of any other
    assignment follows from it.  satisfied=False misses row n // 2 of C by one, as R1cs does."""

    def __init__(self, field, n, nvars, num_inputs, rng, satisfied=True):
        r = nc.modulus(field)
        self.field, self.n, self.nvars, self.num_inputs, self.satisfied = field, n, nvars, num_inputs, satisfied
        self.free = nvars - num_inputs - n
        assert n >= 2 and num_inputs >= 1 and self.free >= 8, (n, nvars, num_inputs)
        self.first_out = num_inputs + self.free
        frees = list(range(num_inputs, self.first_out))
        self.dead = frees[3]
        self.no_a = [frees[3], frees[4], self.first_out + n - 1]
        others = [i for i in range(1, nvars) if i != self.dead and i < self.first_out + n - 1]
        self.in_b = sorted([0] + rng.sample(others, min(len(others), max(2, nvars // 3 - 1))))
        self.z = self._values(rng, r)
        self.A, self.B, self.a, self.b = [], [], [], []
        in_a = [c for c in range(nvars) if c not in self.no_a]
        for i in range(n):
            # row i may use the variables below its own output: the public and free ones and the outputs of earlier rows
            for rows, vals, cols in ((self.A, self.a, in_a), (self.B, self.b, self.in_b)):
                count = bisect.bisect_left(cols, self.first_out + i)
                while True:
                    rw = [(rng.randrange(r), cols[rng.randrange(count)]) for _ in range(rng.choice((1, 1, 2, 3, 3, 7)))]
                    v = sum(c * self.z[j] for c, j in rw) % r
                    if v:
                        break
                rows.append(rw)
                vals.append(v)
        self.C = [[(self.a[i] * self.b[i] * pow(self.z[self.out(i)], -1, r) % r, self.out(i))] for i in range(n)]
        if not satisfied:
            c, j = self.C[n // 2][0]
            self.C[n // 2] = [((c + 1) % r, j)]

    def out(self, i):
        return self.first_out + i

    def _values(self, rng, r, outputs=True):
        z = [1] + [rng.randrange(1, r) for _ in range(self.num_inputs - 1)]
        if self.num_inputs > 1:
            z[-1] = 0
        z += [0, 1, r - 1] + [rng.randrange(1, r) if i % 2 else rng.randrange(2) for i in range(self.free - 3)]
        if outputs:
            z += [rng.randrange(1, r) if i % 2 else 1 for i in range(self.n)]
        return z

    def is_satisfied(self, z=None):
        r = nc.modulus(self.field)
        z = self.z if z is None else z
        dot = lambda rw: sum(c * z[j] for c, j in rw) % r
        return all(dot(ra) * dot(rb) % r == dot(rc) for ra, rb, rc in zip(self.A, self.B, self.C))

    def second_witness(self, rng):
        """another assignment of the SAME A, B and C (the lists themselves): fresh public and free values, every output from its row"""
        r = nc.modulus(self.field)
        other = Instance.__new__(Instance)
        other.__dict__.update(self.__dict__)
        z = self._values(rng, r, outputs=False) + [0] * self.n
        other.a, other.b = [], []
        for i in range(self.n):
            other.a.append(sum(c * z[j] for c, j in self.A[i]) % r)
            other.b.append(sum(c * z[j] for c, j in self.B[i]) % r)
            z[self.out(i)] = other.a[i] * other.b[i] * pow(self.C[i][0][0], -1, r) % r
        other.z = z
        return other


class Setup:
    """the toxic waste, seeded from the case's name, and the CRS of one instance as logs"""

    QUERIES = ("a_query", "b_query", "l_query", "gamma_abc", "h_query")

    def __init__(self, inst, k, name):
        field = inst.field
        r = self.r = nc.modulus(field)
        self.inst, self.k, self.size = inst, k, 1 << k
        n, ni = inst.n, inst.num_inputs
        assert n + ni <= self.size
        rng = random.Random("groth16 setup " + name)
        while True:
            self.tau = rng.randrange(2, r)
            if pow(self.tau, self.size, r) != 1:
                break
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(2, r) for _ in range(4))
        self.lag = sp.lagrange_at(field, k, self.tau)
        self.t = (pow(self.tau, self.size, r) - 1) % r
        self.u, self.v, self.w = ([0] * inst.nvars for _ in range(3))
        for acc, rows in ((self.u, inst.A), (self.v, inst.B), (self.w, inst.C)):
            for j, rw in enumerate(rows):
                for c, i in rw:
                    acc[i] = (acc[i] + self.lag[j] * c) % r
        for i in range(ni):
            self.u[i] = (self.u[i] + self.lag[n + i]) % r
        self.lq = [(self.beta * x + self.alpha * y + z) % r for x, y, z in zip(self.u, self.v, self.w)]
        di, gi = pow(self.delta, -1, r), pow(self.gamma, -1, r)
        self.a_query = list(self.u)
        self.b_query = list(self.v)
        self.l_query = [x * di % r for x in self.lq[ni:]]
        self.gamma_abc = [x * gi % r for x in self.lq[:ni]]
        self.h_query = [pow(self.tau, j, r) * self.t % r * di % r for j in range(self.size - 1)]

    def h_at_tau(self, inst):
        """h(tau) of an assignment, from its padded a and b at the one point tau"""
        r = self.r
        a, b = inst.padded(self.size)
        at = sum(l * x for l, x in zip(self.lag, a)) % r
        bt = sum(l * x for l, x in zip(self.lag, b)) % r
        ct = sum(l * x * y for l, x, y in zip(self.lag, a, b)) % r
        return (at * bt - ct) * pow(self.t, -1, r) % r

    def public_log(self, z_pub):
        """x: the log of vk_x = sum_{i < num_inputs} z_i gamma_abc[i]"""
        assert len(z_pub) == self.inst.num_inputs
        return sum(z * g for z, g in zip(z_pub, self.gamma_abc)) % self.r

    def prove(self, inst, r_, s_, h_shift=0):
        """{"a", "b", "c", "x", "h_tau"}: the logs of A (G1), B (G2 and, as B1, G1) and C (G1), of vk_x, and h(tau) + h_shift as used"""
        r, ni = self.r, inst.num_inputs
        z = inst.z
        assert inst.A is self.inst.A and inst.B is self.inst.B and inst.C is self.inst.C, "another circuit's CRS"
        a = (self.alpha + sum(x * y for x, y in zip(z, self.u)) + r_ * self.delta) % r
        b = (self.beta + sum(x * y for x, y in zip(z, self.v)) + s_ * self.delta) % r
        h_tau = (self.h_at_tau(inst) + h_shift) % r
        priv = sum(x * y for x, y in zip(z[ni:], self.lq[ni:])) % r
        c = ((priv + h_tau * self.t) * pow(self.delta, -1, r) + s_ * a + r_ * b - r_ * s_ * self.delta) % r
        return {"a": a, "b": b, "c": c, "x": self.public_log(z[:ni]), "h_tau": h_tau}

    def verifies(self, proof, z_pub=None):
        """the verifier in the exponent: a b == alpha beta + x gamma + c delta; z_pub: other public inputs than the proof's own"""
        x = proof["x"] if z_pub is None else self.public_log(z_pub)
        return proof["a"] * proof["b"] % self.r == (self.alpha * self.beta + x * self.gamma + proof["c"] * self.delta) % self.r


class Case:
    """one circuit in a family: the satisfied instance and its CRS, the unsatisfied twin (the same A, B and z, one row of C missed, a
    CRS of its own under the same toxic waste), a second assignment of the satisfied circuit, and the randomizers.  Everything is made
    on first use and kept."""

    def __init__(self, family, k, slack, num_inputs):
        self.family, self.k, self.slack, self.num_inputs = family, k, slack, num_inputs
        self.size = 1 << k
        self.n = self.size - num_inputs - slack
        self.nvars = num_inputs + max(8, self.n // 4) + self.n
        self.name = "%s k=%d slack=%d inputs=%d" % (family, k, slack, num_inputs)
        self._made = {}

    def __repr__(self):
        return self.name

    def _get(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def instance(self, satisfied=True):
        return self._get(("inst", satisfied), lambda: Instance(self.family, self.n, self.nvars, self.num_inputs,
                                                               random.Random("groth16 instance " + self.name), satisfied=satisfied))

    def setup(self, satisfied=True):
        return self._get(("setup", satisfied), lambda: Setup(self.instance(satisfied), self.k, self.name))

    def second(self):
        return self._get("second", lambda: self.instance().second_witness(random.Random("groth16 second " + self.name)))

    def randomizers(self, which=0):
        """(r_, s_) in [1, r): `which` 0 for the first proof, 1 for the second assignment's"""
        rng = random.Random("groth16 randomizers %d %s" % (which, self.name))
        r = nc.modulus(self.family)
        return rng.randrange(1, r), rng.randrange(1, r)


SHAPES = ((4, 0, 3), (6, 9, 3), (10, 0, 3), (4, 0, 1))        # (k, slack, num_inputs); the last: a one-point public MSM
_CASES = {}


def cases(family=None):
    out = []
    for fam in FAMILIES if family is None else (family,):
        for shape in SHAPES:
            if (fam, shape) not in _CASES:
                _CASES[(fam, shape)] = Case(fam, *shape)
            out.append(_CASES[(fam, shape)])
    return out


def zero_logs(logs):
    return sum(1 for x in logs if x == 0)
