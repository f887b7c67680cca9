"""CPU: the cross-compiled gfx950 code of the kernels of csrc/sparse.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_quotient.py): no scratch and no dynamic stack in any new kernel, the entry
loops stay rolled, every kernel holds the products DESIGN.md section 4j counts for it -- measured against the yardstick kernel (one Fr
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
template __global__ void k_sparse_vals<%(FR)s>(SparseVals);
template __global__ void k_sparse_z<%(FR)s>(SparseZ);
template __global__ void k_sparse_totals<%(FR)s>(SparseRun);
template __global__ void k_sparse_rows<%(FR)s>(SparseRun);
template __global__ void k_sparse_cross<%(FR)s>(SparseRun);
"""
NAMES = ["k_fr_yardstick", "k_sparse_cross", "k_sparse_rows", "k_sparse_totals", "k_sparse_vals", "k_sparse_z"]

# Fr products in the code of each kernel, each once: the entry loops are rolled
PRODUCTS = {
    "k_sparse_vals": 1,                              # the coefficient on the way in (create)
    "k_sparse_z": 1,                                 # z on the way in
    "k_sparse_totals": 1 + 1,                        # the entry; the store of the total
    # the prefix on the way in; the entry; the store of a row that ends inside the lane; the products by 1 into bend and bstart
    "k_sparse_rows": 1 + 1 + 1 + 1 + 1,
    "k_sparse_cross": 1,                             # the store
}
# the largest VGPR count and the smallest occupancy DESIGN.md 4j states (both fields alike)
VGPRS = {"k_sparse_vals": 64, "k_sparse_z": 64, "k_sparse_totals": 64, "k_sparse_rows": 104, "k_sparse_cross": 64}
WAVES = {"k_sparse_vals": 8, "k_sparse_z": 8, "k_sparse_totals": 8, "k_sparse_rows": 4, "k_sparse_cross": 8}


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/sparse.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "sparse.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "sparse.hip", "-o", "sparse.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "sparse-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_sparse_vals|k_sparse_z|k_sparse_totals|k_sparse_rows|k_sparse_cross)INS_\d+\w+?Fr29EE\w+):", asm, flags=re.M):
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
def test_sparse_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == NAMES
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs and waves per SIMD: recorded in DESIGN.md 4j
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once: the entry loops are not unrolled into copies (a second entry would add a product
        # to the totals and two or more to the rows), and the index arithmetic adds a few multiply-adds
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["mads"] >= (products - 1.5) * base, (k, ks[k]["mads"], products, base)
    for k in PRODUCTS:
        assert ks[k]["lds"] == 0, k              # one lane per slot, column, run of entries or row: nothing is shared
        assert ks[k]["vgprs"] <= VGPRS[k] and ks[k]["waves"] >= WAVES[k], (k, ks[k])
