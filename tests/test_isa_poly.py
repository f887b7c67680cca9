"""CPU: the cross-compiled gfx950 code of the kernels of csrc/poly.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone: no scratch and no dynamic stack in any new kernel, the Fermat loop of the tile inversion stays rolled,
and every kernel holds the products DESIGN.md section 4f counts for it -- measured against the yardstick kernel (one Fr product)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = """
template __global__ void k_fr_yardstick<%(FR)s>(const Fr*, const Fr*, Fr*, uint32_t);
template __global__ void k_poly_eval<%(FR)s>(PolyEval);
template __global__ void k_poly_div<%(FR)s>(PolyDiv);
template __global__ void k_poly_inv_prod<%(FR)s>(PolyInv);
template __global__ void k_poly_inv_tiles<%(FR)s>(Fr*, uint64_t, Fr);
template __global__ void k_poly_inv_apply<%(FR)s>(PolyInv);
template __global__ void k_poly_lagrange<%(FR)s>(PolyLagrange);
template __global__ void k_poly_vec_op<%(FR)s>(PolyVecOp);
"""
NAMES = ["k_fr_yardstick", "k_poly_div", "k_poly_eval", "k_poly_inv_apply", "k_poly_inv_prod", "k_poly_inv_tiles", "k_poly_lagrange", "k_poly_vec_op"]

# Fr products in the code of each kernel: conversions on the way in and out, the lane's run, one tree or scan step
# (the step loop is rolled), the lane's last step
PRODUCTS = {
    "k_poly_eval": 1 + 3 + 1 + 1,               # load, Horner, tree step, the partial back to class M
    "k_poly_div": 1 + 1 + 3 + 1 + 4 + 1 + 2,    # load, carry, suffix Horner, scan step, finish, store (ABI), store (class M: quotient level, remainder)
    "k_poly_inv_prod": 1 + 3 + 1,               # load, run, tree step
    "k_poly_inv_tiles": 2 + 1,                  # the square and the multiply of the rolled Fermat loop, coeff
    "k_poly_inv_apply": 1 + 5 + 2 + 2 + 6 + 1,  # load, run, the two scans' step, the lane's factor, the four outputs, store
    "k_poly_lagrange": 1 + 1 + 2 + 1,           # w^i, the constant, w^-i, store
    "k_poly_vec_op": 3 + 1 + 1 + 1,             # three loads, a*b, the scaling, store
}


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/poly.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "poly.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "poly.hip", "-o", "poly.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "poly-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(%s)\w+):" % "|".join(NAMES), asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[m.group(2)] = dict(mads=ops.count("v_mad_u64_u32"), valu=sum(1 for o in ops if o.startswith("v_")),
                               scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                               dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                               vgprs=int(re.search(r"VGPRs: (\d+)", blk).group(1)),
                               waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                               lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("FR", ["Bls12_377_Fr29", "Bls12_381_Fr29"])
def test_poly_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == NAMES
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4f
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once: nothing is unrolled into copies, and the index arithmetic adds a few
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
    # the exponentiation loop stays rolled: a small multiple of one product, not the 380 of an unrolled x^(r - 2)
    assert ks["k_poly_inv_tiles"]["mads"] <= 3.5 * base
    # the tile (36 bytes an element) plus the scan arrays fit the 64 KiB a block may have, and two blocks fit a CU's 160 KiB
    assert ks["k_poly_eval"]["lds"] == 36 * 1024 and ks["k_poly_inv_prod"]["lds"] == 36 * 1024
    assert ks["k_poly_div"]["lds"] == 36 * (1024 + 256) and ks["k_poly_inv_apply"]["lds"] == 36 * (1024 + 512)
    assert ks["k_poly_eval"]["waves"] >= 4 and ks["k_poly_div"]["waves"] >= 3 and ks["k_poly_inv_apply"]["waves"] >= 2
