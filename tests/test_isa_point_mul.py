"""CPU: the cross-compiled gfx950 code of k_pm_table, k_pm_mul and k_pm_mul_uniform (csrc/point_mul.hpp), judged by the compiler's
resource remarks and the count of 64-bit multiply-adds alone: no scratch, the digit loops ROLLED -- measured against the yardstick
kernel of tests/test_isa_check.py (one xyzz_dbl and one xyzz_madd) -- and, over Fp, registers for two waves per SIMD in k_pm_mul."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = """
template <class E>
__global__ void __launch_bounds__(256) k_yardstick(const XyzzT<typename E::T>* in, const AffineT<typename E::T>* base, XyzzT<typename E::T>* out) {
  typename E::Md md;
  XyzzT<typename E::T> acc = in[threadIdx.x];
  AffineT<typename E::T> p = base[threadIdx.x];
  xyzz_dbl<E>(acc, md);
  xyzz_madd<E>(acc, p, false, false, md);
  out[threadIdx.x] = acc;
}
template __global__ void k_yardstick<%(E)s>(const XyzzT<%(E)s::T>*, const AffineT<%(E)s::T>*, XyzzT<%(E)s::T>*);
template __global__ void k_pm_table<%(E)s>(const uint8_t*, size_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_pm_mul<%(E)s>(const AffineDevT<%(E)s::T>*, const uint32_t*, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_pm_mul_uniform<%(E)s>(const uint8_t*, size_t, uint32_t, const PmNaf, XyzzDevT<%(E)s::T>*);
"""


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/point_mul.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "pm.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "pm.hip", "-o", "pm.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "pm-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm(?:11k_yardstick|10k_pm_table|8k_pm_mul|16k_pm_mul_uniform)\w+):", asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        waves = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[name] = dict(mads=ops.count("v_mad_u64_u32"), scratch=scratch, vgprs=vgprs, waves=waves)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", ["FpEl<Bls12_377_Fq>", "Fp2El<Bls12_381_Fq, 1>"], ids=["fp", "fp2"])
def test_point_mul_kernel_isa(E):
    ks = _kernels(E)
    yard = [v for k, v in ks.items() if "k_yardstick" in k]
    table = [v for k, v in ks.items() if "k_pm_table" in k]
    mul = [v for k, v in ks.items() if "8k_pm_mul" in k]
    uni = [v for k, v in ks.items() if "k_pm_mul_uniform" in k]
    assert len(yard) == 1 and len(table) == 1 and len(mul) == 1 and len(uni) == 1
    base = yard[0]["mads"]
    assert base > 1000
    for k, v in ks.items():
        print(k[:40], v)
    for v in table + mul + uni:
        assert v["scratch"] == 0
    # rolled: one inlined doubling and one inlined addition (with its rare same-x half), whatever the number of digits
    assert mul[0]["mads"] < 2 * base, (mul[0]["mads"], base)
    assert uni[0]["mads"] < 2 * base, (uni[0]["mads"], base)
    # the table build has the doubling, the addition of its loop and the conversions of the input image
    assert table[0]["mads"] < 3 * base, (table[0]["mads"], base)
    if E.startswith("FpEl"):
        assert mul[0]["waves"] >= 2, mul[0]["vgprs"]
