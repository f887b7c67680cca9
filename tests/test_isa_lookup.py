"""CPU: the cross-compiled gfx950 code of the kernels of csrc/lookup.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_scan.py): no scratch and no dynamic stack in any new kernel, the build and the
probe of the hash table hold no Fr product at all, the counter-to-element kernel at most one, the logUp rows the products DESIGN.md
section 4o counts -- measured against the yardstick kernel (one Fr product) -- and every kernel has the VGPRs, LDS and waves per SIMD
stated there."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

NEW = ["k_lookup_canon", "k_lookup_build", "k_lookup_probe", "k_lookup_mult", "k_lookup_scan_up", "k_lookup_scan_down", "k_lookup_expand",
       "k_logup_den", "k_logup_term"]
ARGS = {"k_lookup_canon": "LookupCanon", "k_lookup_build": "LookupBuild", "k_lookup_probe": "LookupProbe", "k_lookup_mult": "LookupMult",
        "k_lookup_scan_up": "LookupScan", "k_lookup_scan_down": "LookupScan", "k_lookup_expand": "LookupExpand", "k_logup_den": "LogupRows",
        "k_logup_term": "LogupRows"}

# Fr products in the code of each kernel.  The table side is integer work: reductions, a hash, compares, atomics.  A counter
# becomes an arkworks image by one product (none in the plain form: the same kernel).  The denominators: a conversion in and one out,
# inside the rolled column loop.  The terms: a conversion per helper column (rolled), the inverse and the multiplicity in, their product,
# the last helper column out, the term out.
PRODUCTS = {"k_lookup_canon": 0, "k_lookup_build": 0, "k_lookup_probe": 0, "k_lookup_scan_up": 0, "k_lookup_scan_down": 0, "k_lookup_expand": 0,
            "k_lookup_mult": 1, "k_logup_den": 2, "k_logup_term": 6}
# the largest VGPR count and the smallest occupancy DESIGN.md 4o states (both fields alike)
VGPRS = {"k_lookup_canon": 48, "k_lookup_build": 32, "k_lookup_probe": 64, "k_lookup_mult": 40, "k_lookup_scan_up": 16, "k_lookup_scan_down": 16,
         "k_lookup_expand": 16, "k_logup_den": 64, "k_logup_term": 64}
WAVES = {k: 8 for k in NEW}
LDS = {"k_lookup_scan_up": 4 * 256, "k_lookup_scan_down": 2 * 4 * 256, "k_lookup_probe": 4 * (4 + 4 + 8 + 8)}


def _kernels(FR):
    decls = "template __global__ void k_fr_yardstick<%s>(const Fr*, const Fr*, Fr*, uint32_t);\n" % FR
    decls += "".join("template __global__ void %s<%s>(%s);\n" % (k, FR, ARGS[k]) for k in NEW)
    src = '#include "%s/2022-entries_amd/csrc/lookup.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, decls)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "lookup.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "lookup.hip", "-o", "lookup.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "lookup-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|%s)INS_\d+\w+?Fr29EEEv\w+):" % "|".join(NEW), asm, flags=re.M):
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
def test_lookup_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == sorted(NEW + ["k_fr_yardstick"])
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4o
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once (the column loops are rolled); index arithmetic adds a few multiply-adds, well
        # below half a product
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["mads"] >= (products - 0.5) * base, (k, ks[k]["mads"], products, base)
    for k in NEW:
        assert ks[k]["lds"] == LDS.get(k, 0), (k, ks[k])
        assert ks[k]["vgprs"] <= VGPRS[k] and ks[k]["waves"] >= WAVES[k], (k, ks[k])
