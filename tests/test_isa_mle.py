"""CPU: the cross-compiled gfx950 code of the kernels of csrc/mle.hpp, judged by the compiler's resource remarks and the count of 64-bit
multiply-adds alone (the method of tests/test_isa_sparse.py): no scratch and no dynamic stack in any new kernel -- the accumulators and
running products of a round stay in registers for every degree --, the point, term and factor loops stay rolled, every kernel holds the
products DESIGN.md section 4k counts for it, measured against the yardstick kernel (one Fr product), a lane's pair is loaded as
dwordx4s, and every kernel has the VGPRs, the LDS and the waves per SIMD stated there."""
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
template __global__ void k_mle_fix<%(FR)s>(MleFix);
template __global__ void k_mle_eq<%(FR)s>(MleEq);
template __global__ void k_mle_round<%(FR)s, 1>(MleRound);
template __global__ void k_mle_round<%(FR)s, 2>(MleRound);
template __global__ void k_mle_round<%(FR)s, 3>(MleRound);
template __global__ void k_mle_round<%(FR)s, 4>(MleRound);
template __global__ void k_mle_round<%(FR)s, 5>(MleRound);
template __global__ void k_mle_sum<%(FR)s>(MleSum);
"""
ROUNDS = ["k_mle_round%d" % D for D in range(1, 6)]
NAMES = sorted(["k_fr_yardstick", "k_mle_fix", "k_mle_eq", "k_mle_sum"] + ROUNDS)

# Fr products on the vector unit in the code of each kernel, each once: the loops over points, terms, factors, tables
# and tree levels are rolled.  The product by 1 in front of a block's store is done by lane 0 alone on a uniform value, and the compiler
# runs it on the scalar unit: it is not among the v_mad_u64_u32.
PRODUCTS = {
    "k_mle_fix": 1 + 2 + 1,                          # the conversion of a copy (k == 0); a level; the store
    "k_mle_eq": 1,
    "k_mle_sum": 1 + 1,                              # the lane sum to class M; the tree's product by 1
}
for D in range(1, 6):
    # the fold (2) and its store; the pair of a factor to class M (2); per evaluation point: the running product, the lane sum to
    # class M, the tree's product by 1
    PRODUCTS["k_mle_round%d" % D] = 2 + 1 + 2 + 3 * (D + 1)
# the largest VGPR count, the LDS and the smallest occupancy DESIGN.md 4k states (both fields alike)
VGPRS = {"k_mle_fix": 104, "k_mle_eq": 56, "k_mle_sum": 48, "k_mle_round1": 120, "k_mle_round2": 136, "k_mle_round3": 152, "k_mle_round4": 160,
         "k_mle_round5": 184}
WAVES = {"k_mle_fix": 4, "k_mle_eq": 8, "k_mle_sum": 7, "k_mle_round1": 4, "k_mle_round2": 3, "k_mle_round3": 3, "k_mle_round4": 3, "k_mle_round5": 2}
LDS = {"k_mle_fix": 1024 * 36, "k_mle_eq": 0, "k_mle_sum": 256 * 36}
LDS.update({k: 256 * 36 for k in ROUNDS})


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/mle.hpp"\n#include "%s/2022-entries_amd/csrc/ntt.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "mle.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "mle.hip", "-o", "mle.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "mle-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_mle_fix|k_mle_eq|k_mle_round|k_mle_sum)INS_\d+\w+?Fr29E(?:Li(\d)E)?E\w+):", asm, flags=re.M):
        name, key = m.group(1), m.group(2) + (m.group(3) or "")
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[key] = dict(mads=ops.count("v_mad_u64_u32"), wide_loads=ops.count("global_load_dwordx4"), narrow_loads=ops.count("global_load_dword"),
                        scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                        dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                        vgprs=int(re.search(r" VGPRs: (\d+)", blk).group(1)),
                        waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                        lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("FR", ["Bls12_377_Fr29", "Bls12_381_Fr29"])
def test_mle_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == NAMES
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4k
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    for k, products in PRODUCTS.items():
        # every product the kernel's code holds, once: a loop unrolled into copies would add at least a product, and the index
        # arithmetic adds a few multiply-adds
        assert ks[k]["mads"] <= (products + 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["mads"] >= (products - 0.5) * base, (k, ks[k]["mads"], products, base)
        assert ks[k]["lds"] == LDS[k], (k, ks[k])
        assert ks[k]["vgprs"] <= VGPRS[k] and ks[k]["waves"] >= WAVES[k], (k, ks[k])
    for k in ROUNDS:
        # the 64 bytes of a pair and the 128 bytes a fold reads: four and eight loads of 16 bytes per lane, and no narrower vector load
        assert ks[k]["wide_loads"] == 8 and ks[k]["narrow_loads"] == 0, (k, ks[k])
