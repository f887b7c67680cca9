"""CPU: the cross-compiled gfx950 code of the kernel of csrc/expr.hpp, judged by the compiler's resource remarks and the count of 64-bit
multiply-adds alone (the method of tests/test_isa_lookup.py): no scratch and no dynamic stack, the code holds the three products
DESIGN.md section 4p states -- the conversion of a column operand, the product of MUL / SQR / MUL1, the conversion of the result --
measured against the yardstick kernel (one Fr product), which shows that the instruction loop and the operand loop are rolled, and the
VGPRs and the static LDS are as stated there (the slots are dynamic LDS)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PRODUCTS = 3
VGPRS = 96           # the largest VGPR count DESIGN.md 4p states (both fields alike): 5 waves per SIMD as far as registers go,
WAVES = 5            # which is also what the LDS leaves at S = 4; above that the slots decide


def _kernels(FR):
    decls = "template __global__ void k_fr_yardstick<%s>(const Fr*, const Fr*, Fr*, uint32_t);\n" % FR
    decls += "template __global__ void k_expr_rows<%s>(ExprRun);\n" % FR
    src = '#include "%s/2022-entries_amd/csrc/ntt.hpp"\n#include "%s/2022-entries_amd/csrc/expr.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, ROOT, decls)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "expr.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "expr.hip", "-o", "expr.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "expr-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_expr_rows)INS_\d+\w+?Fr29EEEv\w+):", asm, flags=re.M):
        name, key = m.group(1), m.group(2)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[key] = dict(mads=ops.count("v_mad_u64_u32"),
                        scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                        dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                        vgprs=int(re.search(r"VGPRs: (\d+)", blk).group(1)),
                        waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                        lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("FR", ["Bls12_377_Fr29", "Bls12_381_Fr29"])
def test_expr_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == ["k_expr_rows", "k_fr_yardstick"]
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4p
    v = ks["k_expr_rows"]
    assert v["scratch"] == 0 and v["dynamic_stack"] == "False", v
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    # every product the kernel's code holds, once: the loops over the instructions and over the two operands are rolled.  The m r of a
    # SUB and index arithmetic add a few multiply-adds, well below half a product
    assert v["mads"] <= (PRODUCTS + 0.5) * base, (v["mads"], base)
    assert v["mads"] >= (PRODUCTS - 0.5) * base, (v["mads"], base)
    assert v["lds"] == 0, v                      # static LDS: none
    assert v["vgprs"] <= VGPRS and v["waves"] >= WAVES, v
