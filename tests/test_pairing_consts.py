"""CPU: csrc/pairing_consts.inc is what tools/gen_pairing_consts.py writes, and its Frobenius coefficients are the ones recomputed here
from p and xi alone: gamma[j][k] = xi^(k (p^j - 1) / 6), checked against the big-integer model's Frobenius map (a plain power by p^j)."""
import os
import re
import subprocess
import sys

import pytest

import pairing_cases as pc
from conftest import ROOT

INC = os.path.join(ROOT, "2022-entries_amd", "csrc", "pairing_consts.inc")


def test_the_committed_file_is_the_generated_one():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pairing_consts.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(INC).read()


@pytest.mark.parametrize("fam", sorted(pc.FAMILIES))
def test_frobenius_coefficients_recomputed(fam):
    F = pc.FAMILIES[fam]
    text = open(INC).read()
    body = text[text.index("struct %s_Pairing" % fam.replace("bls", "Bls")):]
    body = body[:body.index("};\n};") if "};\n};" in body else len(body)]
    rows = re.findall(r"\{((?:0x[0-9a-f]{8}u(?:, )?){24})\}", body)
    assert len(rows) >= 15
    w = [0] * 12
    w[1] = 1
    for j in (1, 2, 3):
        g = pc.f2_pow(F, F.xi, (F.p ** j - 1) // 6)
        # w^(p^j) = gamma[j][1] w in the model's Fp12
        assert pc.f12_frobenius(F, w, j) == pc.f12_from_f2(F, g, 1)
        for k in range(1, 6):
            words = [int(v[:-1], 16) for v in rows[5 * (j - 1) + (k - 1)].split(", ")]
            c0 = sum(v << (32 * i) for i, v in enumerate(words[:12]))
            c1 = sum(v << (32 * i) for i, v in enumerate(words[12:]))
            assert (c0, c1) == pc.f2_pow(F, g, k), (j, k)
