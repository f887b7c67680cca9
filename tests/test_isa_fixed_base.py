"""CPU: the cross-compiled gfx950 code of k_fb_mul and k_fb_normalize (csrc/fixed_base.hpp): no scratch, no dynamic register
indexing, the loop over the table levels ROLLED -- measured against the yardstick kernel of tests/test_isa_check.py (one xyzz_dbl
and one xyzz_madd) -- and, over Fp, registers for two waves per SIMD."""
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
template __global__ void k_fb_mul<%(E)s>(const AffineDevT<%(E)s::T>*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_fb_normalize<%(E)s, false>(const XyzzDevT<%(E)s::T>*, uint32_t, %(E)s::T*, uint8_t*, size_t);
template __global__ void k_fb_normalize<%(E)s, true>(const XyzzDevT<%(E)s::T>*, uint32_t, %(E)s::T*, uint8_t*, size_t);
"""


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/fixed_base.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "fb.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "fb.hip", "-o", "fb.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "fb-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm(?:11k_yardstick|8k_fb_mul|14k_fb_normalize)\w+):", asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        waves = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[name] = dict(body=body, mads=ops.count("v_mad_u64_u32"), scratch=scratch, vgprs=vgprs, waves=waves)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", ["FpEl<Bls12_377_Fq>", "Fp2El<Bls12_381_Fq, 1>"], ids=["fp", "fp2"])
def test_fixed_base_kernel_isa(E):
    ks = _kernels(E)
    yard = [v for k, v in ks.items() if "k_yardstick" in k]
    mul = [v for k, v in ks.items() if "k_fb_mul" in k]
    norm = [v for k, v in ks.items() if "k_fb_normalize" in k]
    assert len(yard) == 1 and len(mul) == 1 and len(norm) == 2
    base = yard[0]["mads"]
    assert base > 1000
    for k, v in ks.items():
        print(k[:40], {x: v[x] for x in ("mads", "scratch", "vgprs", "waves")})
    for v in mul + norm:
        assert v["scratch"] == 0
        assert "s_set_gpr_idx_on" not in v["body"] and "scratch_" not in v["body"]
    # rolled: one inlined addition (with its rare same-x half) is below the yardstick's doubling + addition; 16 unrolled levels
    # would be about six times it
    assert mul[0]["mads"] < 2 * base, (mul[0]["mads"], base)
    if E.startswith("FpEl"):
        assert mul[0]["waves"] >= 2, mul[0]["vgprs"]
        assert all(v["waves"] >= 2 for v in norm)
