"""CPU: the cross-compiled gfx950 code of the transform kernels (csrc/ntt.hpp), judged by the compiler's resource remarks and the
count of 64-bit multiply-adds alone: no scratch and no dynamic stack in any new kernel, and a butterfly level costs what the
yardstick kernel (one Fr product, one add, one sub) costs -- the levels redo no conversion and no twiddle power."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = """
// the level loop of k_ntt_pass alone
template <class FR>
__global__ void __launch_bounds__(NTT_THREADS) k_levels(NttPass ps) {
  __shared__ Fr lds[NTT_TILE];
  const uint32_t elems = 1u << (ps.p + ps.log_c);
  for (uint32_t l = 0; l < ps.p; l++) {
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < elems / 2; u += NTT_THREADS) ntt_butterfly<FR>(lds, ps, l, u);
  }
}
template __global__ void k_levels<%(FR)s>(NttPass);
template __global__ void k_fr_yardstick<%(FR)s>(const Fr*, const Fr*, Fr*, uint32_t);
template __global__ void k_ntt_pass<%(FR)s>(NttPass);
template __global__ void k_fr_mul_vec<%(FR)s>(const uint32_t*, const uint32_t*, uint32_t*, size_t, uint32_t);
template __global__ void k_ntt_table<%(FR)s>(Fr, uint32_t, Fr*);
"""


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/ntt.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "ntt.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "ntt.hip", "-o", "ntt.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "ntt-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_levels|k_fr_yardstick|k_ntt_pass|k_fr_mul_vec|k_ntt_table)\w+):", asm, flags=re.M):
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
def test_ntt_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == ["k_fr_mul_vec", "k_fr_yardstick", "k_levels", "k_ntt_pass", "k_ntt_table"]
    for k, v in ks.items():
        print(FR, k, v)
    for k, v in ks.items():
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", k
    base = ks["k_fr_yardstick"]["mads"]
    # one 9 x 29 product: 81 a*b terms and 72 to 81 m*r terms (r_0 = 1: the compiler may turn those nine into plain adds)
    assert 100 <= base <= 162, base
    assert ks["k_levels"]["mads"] <= 1.25 * base, (ks["k_levels"]["mads"], base)
    # the whole pass: the conversion and the two offset products of the first load, one level, and at the store the two-level
    # twiddle, or the scale, the two offset products and the conversion
    assert ks["k_ntt_pass"]["mads"] <= 10.5 * base, (ks["k_ntt_pass"]["mads"], base)
    assert ks["k_fr_mul_vec"]["mads"] <= 2.1 * base
    assert ks["k_ntt_pass"]["lds"] == 36 * 1024 and ks["k_ntt_pass"]["waves"] >= 4
