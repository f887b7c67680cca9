"""CPU: the cross-compiled gfx950 code of k_sm_accumulate and k_sm_tail (csrc/seg_msm.hpp), judged by the compiler's resource remarks
and the count of 64-bit multiply-adds alone: no scratch in either kernel over either field, the loops over windows, tiles, list
entries and reduction steps ROLLED -- measured against the yardstick kernel of tests/test_isa_point_mul.py (one xyzz_dbl and one
xyzz_madd) -- and the register counts DESIGN 4q quotes: two waves per SIMD over Fp, one over Fp2."""
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
template __global__ void k_sm_accumulate<%(E)s>(const SmLaunch, XyzzDevT<%(E)s::T>*);
template __global__ void k_sm_tail<%(E)s>(const XyzzDevT<%(E)s::T>*, const uint32_t*, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
"""


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/seg_msm.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "sm.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "sm.hip", "-o", "sm.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "sm-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm(?:11k_yardstick|15k_sm_accumulate|9k_sm_tail)\w+):", asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[name] = dict(mads=ops.count("v_mad_u64_u32"),
                         scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                         dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                         vgprs=int(re.search(r"VGPRs: (\d+)", blk).group(1)),
                         agprs=int(re.search(r"AGPRs: (\d+)", blk).group(1)),
                         waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", ["FpEl<Bls12_377_Fq>", "Fp2El<Bls12_381_Fq, 1>"], ids=["fp", "fp2"])
def test_segment_kernel_isa(E):
    ks = _kernels(E)
    yard = [v for k, v in ks.items() if "k_yardstick" in k]
    acc = [v for k, v in ks.items() if "k_sm_accumulate" in k]
    tail = [v for k, v in ks.items() if "k_sm_tail" in k]
    assert len(yard) == 1 and len(acc) == 1 and len(tail) == 1
    base = yard[0]["mads"]
    assert base > 1000
    for k, v in ks.items():
        print(k[:40], v)
    for v in acc + tail:
        assert v["scratch"] == 0 and v["dynamic_stack"] == "False", v
    # rolled.  The accumulate kernel holds ONE mixed addition (with its rare same-x half: a doubling) and the three additions of the
    # fold, scan and sum loops, each with its rare doubling: in products (10 + 8) + 3 (14 + 9) = 87 against the yardstick's
    # 9 + 10 + 8 = 27, so below 4 yardsticks; unrolled over the 2 (c - 1) steps of one window size alone it would be above 10.
    assert acc[0]["mads"] < 4 * base, (acc[0]["mads"], base)
    # the tail: one doubling, one addition with its rare doubling -- 9 + 14 + 9 = 32 products, below 2 yardsticks, whatever the windows
    assert tail[0]["mads"] < 2 * base, (tail[0]["mads"], base)
    if E.startswith("FpEl"):
        # 256 registers at most over Fp, so two waves per SIMD
        # (quoted there: 197 and 238 VGPRs, no AGPRs; pinned with the margin of one allocation step of 8)
        assert acc[0]["waves"] >= 2 and acc[0]["vgprs"] <= 208 and acc[0]["agprs"] == 0, acc[0]
        assert tail[0]["waves"] >= 2 and tail[0]["vgprs"] <= 248 and tail[0]["agprs"] == 0, tail[0]
    else:
        # over Fp2 one wave per SIMD: all 256 VGPRs and, quoted in DESIGN 4q, 179 and 183 AGPRs -- pinned at 192, a quarter of the
        # accumulator file to spare; a build that needs more is on its way to scratch
        assert acc[0]["waves"] == 1 and tail[0]["waves"] == 1
        assert acc[0]["vgprs"] <= 256 and acc[0]["agprs"] <= 192, acc[0]
        assert tail[0]["vgprs"] <= 256 and tail[0]["agprs"] <= 192, tail[0]
