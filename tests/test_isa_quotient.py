"""CPU: the cross-compiled gfx950 code of the kernels of csrc/quotient.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_scan.py): no scratch and no dynamic stack in any new kernel, the column
loops stay rolled, every kernel holds the products DESIGN.md section 4i counts for it -- measured against the yardstick kernel (one Fr
product) -- and has the VGPRs and waves per SIMD stated there."""
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
template __global__ void k_quot_xm1<%(FR)s>(QuotXm1);
template __global__ void k_quot_rows<%(FR)s>(QuotRows);
template __global__ void k_lincomb<%(FR)s>(LinComb);
"""
NAMES = ["k_fr_yardstick", "k_lincomb", "k_quot_rows", "k_quot_xm1"]

# Fr products in the code of each kernel, each once: the column loops are rolled
PRODUCTS = {
    "k_quot_xm1": 2 + 1,                             # omega^i and g; the store
    # x (2); z[i], z[i + ratio], 1 / (x - 1), pi and q_c on the way in (5); t_perm2 (1); per column two loads and the four products of
    # the two factors (6); a gate column below the fifth: q_lc and q_hash on the way in and times w and w^5, w^2, w^4, w^5, and at odd
    # columns w w', q_mul on the way in and times it (11); the running product of the wires (1); the fifth column: q_ecc and q_o on the
    # way in, times the running product and times w4 (4); alpha, 1 / Z_H, the store (3)
    "k_quot_rows": 2 + 5 + 1 + 6 + 11 + 1 + 4 + 3,
    "k_lincomb": 1 + 1 + 1,                          # per column the load and the coefficient; the store
}
# the largest VGPR count and the smallest occupancy DESIGN.md 4i states (both fields alike)
VGPRS = {"k_quot_xm1": 64, "k_quot_rows": 168, "k_lincomb": 64}
WAVES = {"k_quot_xm1": 8, "k_quot_rows": 3, "k_lincomb": 8}


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/quotient.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "quot.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "quot.hip", "-o", "quot.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "quot-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_quot_xm1|k_quot_rows|k_lincomb)INS_\d+\w+?Fr29EE\w+):", asm, flags=re.M):
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
def test_quotient_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == NAMES
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs and waves per SIMD: recorded in DESIGN.md 4i
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once: the column loops are not unrolled into copies (five columns would add some
        # seventy products to the rows, a second column two to the combination), and the index arithmetic adds a few multiply-adds
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["mads"] >= (products - 1.5) * base, (k, ks[k]["mads"], products, base)
    for k in PRODUCTS:
        assert ks[k]["lds"] == 0, k              # one lane per row or element: nothing is shared
        assert ks[k]["vgprs"] <= VGPRS[k] and ks[k]["waves"] >= WAVES[k], (k, ks[k])
