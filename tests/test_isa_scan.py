"""CPU: the cross-compiled gfx950 code of the kernels of csrc/scan.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_poly.py): no scratch and no dynamic stack in any new kernel, the step loops
and the column loop of the permutation product stay rolled, every kernel holds the products DESIGN.md section 4h counts for it --
measured against the yardstick kernel (one Fr product) -- and has the VGPRs, LDS and waves per SIMD stated there."""
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
template __global__ void k_scan_up<%(FR)s, kScanProduct>(ScanUp);
template __global__ void k_scan_up<%(FR)s, kScanSum>(ScanUp);
template __global__ void k_scan_down<%(FR)s, kScanProduct>(ScanDown);
template __global__ void k_scan_down<%(FR)s, kScanSum>(ScanDown);
template __global__ void k_scan_perm<%(FR)s>(ScanPerm);
"""
NAMES = ["k_fr_yardstick", "k_scan_down.product", "k_scan_down.sum", "k_scan_perm", "k_scan_up.product", "k_scan_up.sum"]

# Fr products in the code of each kernel: conversions on the way in and out, the lane's run, one tree or scan step (the
# step loop is rolled), the lane's last step.  The load holds three: the conversion, and for the permutation product's second vector
# one more conversion and the product of the two.  A sum holds products only where a value comes back to class M.
PRODUCTS = {
    "k_scan_up.product": 3 + 3 + 1,                  # load, run, tree step (the total is stored as it is)
    "k_scan_up.sum": 3 + 1 + 1,                      # load, the reduction of an odd tree step, the total to class M
    "k_scan_down.product": 3 + 3 + 1 + 1 + 4 + 1,    # load, prefixes of the run, scan step, offset, four outputs, store (ABI)
    "k_scan_down.sum": 3 + 1 + 1 + 1 + 1,            # load, the reduction of an odd scan step, the total, store (ABI), store (class M)
    "k_scan_perm": 2 + 6 + 2,                        # omega^j and beta; per column two loads, beta k id, beta sigma, two factors; two stores
}
# the largest VGPR count and the smallest occupancy DESIGN.md 4h states (both fields alike)
VGPRS = {"k_scan_up.product": 64, "k_scan_up.sum": 64, "k_scan_down.product": 128, "k_scan_down.sum": 96, "k_scan_perm": 144}
WAVES = {"k_scan_up.product": 4, "k_scan_up.sum": 4, "k_scan_down.product": 3, "k_scan_down.sum": 3, "k_scan_perm": 3}


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/scan.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "scan.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "scan.hip", "-o", "scan.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "scan-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_scan_up|k_scan_down|k_scan_perm)INS_\d+\w+?Fr29E(?:Lj([01]))?E\w+):", asm, flags=re.M):
        name = m.group(1)
        key = m.group(2) + ("" if m.group(3) is None else (".product", ".sum")[int(m.group(3))])
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
def test_scan_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == NAMES
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4h
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once: the step loops and the column loop are not unrolled into copies (eight scan
        # steps would add seven products, eight columns forty-two), and the index arithmetic adds a few multiply-adds
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["mads"] >= (products - 1.5) * base, (k, ks[k]["mads"], products, base)
    # the tile (36 bytes an element), and on the way down the lane totals beside it
    assert ks["k_scan_up.product"]["lds"] == 36 * 1024 and ks["k_scan_up.sum"]["lds"] == 36 * 1024
    assert ks["k_scan_down.product"]["lds"] == 36 * (1024 + 256) and ks["k_scan_down.sum"]["lds"] == 36 * (1024 + 256)
    assert ks["k_scan_perm"]["lds"] == 0
    for k in PRODUCTS:
        assert ks[k]["vgprs"] <= VGPRS[k] and ks[k]["waves"] >= WAVES[k], (k, ks[k])
