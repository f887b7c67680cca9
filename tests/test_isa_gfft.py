"""CPU: the cross-compiled gfx950 code of k_gf_table, k_gf_stage and k_gf_scale (csrc/group_fft.hpp), judged by the compiler's resource
remarks and the count of 64-bit multiply-adds alone: no scratch and no dynamic stack, the walk ROLLED, and the stage kernel's
multiply-adds within what its parts cost -- the k_pm_mul walk, two mixed additions, the twiddle's two Fr products, and the conversions
of A's image and of T's y -- each measured by a yardstick kernel compiled next to it."""
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
__global__ void __launch_bounds__(256) k_y_dbl_madd(const XyzzT<typename E::T>* in, const AffineT<typename E::T>* base, XyzzT<typename E::T>* out) {
  typename E::Md md;
  XyzzT<typename E::T> acc = in[threadIdx.x];
  AffineT<typename E::T> p = base[threadIdx.x];
  xyzz_dbl<E>(acc, md);
  xyzz_madd<E>(acc, p, false, false, md);
  out[threadIdx.x] = acc;
}
template <class E>
__global__ void __launch_bounds__(256) k_y_madd(const XyzzT<typename E::T>* in, const AffineT<typename E::T>* base, XyzzT<typename E::T>* out) {
  typename E::Md md;
  XyzzT<typename E::T> acc = in[threadIdx.x];
  AffineT<typename E::T> p = base[threadIdx.x];
  xyzz_madd<E>(acc, p, false, false, md);
  out[threadIdx.x] = acc;
}
// the conversions a butterfly adds to the walk: A's image to limbs, T's y through a product by 1
template <class E>
__global__ void __launch_bounds__(256) k_y_load(GfVec v, typename E::T* out) {
  typename E::Md md;
  AffineT<typename E::T> p;
  gf_load<E>(p, v, threadIdx.x, md);
  typename E::T one, y;
  E::set_one(one);
  E::mul(y, p.y, one, md);
  out[2 * threadIdx.x] = p.x;
  out[2 * threadIdx.x + 1] = y;
}
template <class E>
__global__ void __launch_bounds__(256) k_y_frmul(const Fr* a, const Fr* b, Fr* out) {
  Fr x = a[threadIdx.x], y = b[threadIdx.x];
  fr_mul<GfFr<E>>(x, x, y);
  out[threadIdx.x] = x;
}
template __global__ void k_y_dbl_madd<%(E)s>(const XyzzT<%(E)s::T>*, const AffineT<%(E)s::T>*, XyzzT<%(E)s::T>*);
template __global__ void k_y_madd<%(E)s>(const XyzzT<%(E)s::T>*, const AffineT<%(E)s::T>*, XyzzT<%(E)s::T>*);
template __global__ void k_y_load<%(E)s>(GfVec, %(E)s::T*);
template __global__ void k_y_frmul<%(E)s>(const Fr*, const Fr*, Fr*);
template __global__ void k_pm_mul<%(E)s>(const AffineDevT<%(E)s::T>*, const uint32_t*, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_gf_table<%(E)s>(GfVec, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_gf_stage<%(E)s, true>(GfVec, const AffineDevT<%(E)s::T>*, NttTable, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_gf_stage<%(E)s, false>(GfVec, const AffineDevT<%(E)s::T>*, NttTable, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
template __global__ void k_gf_scale<%(E)s>(const AffineDevT<%(E)s::T>*, GfScale, uint32_t, uint32_t, uint32_t, uint32_t, XyzzDevT<%(E)s::T>*);
"""

# v_mad_u64_u32 in k_gf_stage<E, true>, as the compiler of this toolchain emits it (pinned: a change here is a change of the hot path)
PINNED_STAGE_MADS = {"fp": 23134, "fp2": 78833}


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/group_fft.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "gf.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "gf.hip", "-o", "gf.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "gf-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_y_dbl_madd|k_y_madd|k_y_load|k_y_frmul|k_pm_mul|k_gf_table|k_gf_stage|k_gf_scale)I\w+):", asm, flags=re.M):
        name, short = m.group(1), m.group(2)
        if short == "k_gf_stage":
            short += "_mul" if "ELb1E" in name else "_first"
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        blk = blk[:blk.index("LDS Size")]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        waves = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", blk).group(1)
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        assert short not in out, short
        out[short] = dict(mads=ops.count("v_mad_u64_u32"), scratch=scratch, vgprs=vgprs, waves=waves, dynamic_stack=dyn)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", ["FpEl<Bls12_377_Fq>", "Fp2El<Bls12_381_Fq, 1>"], ids=["fp", "fp2"])
def test_group_fft_kernel_isa(E):
    ks = _kernels(E)
    assert set(ks) == {"k_y_dbl_madd", "k_y_madd", "k_y_load", "k_y_frmul", "k_pm_mul", "k_gf_table", "k_gf_stage_mul", "k_gf_stage_first", "k_gf_scale"}
    for k, v in ks.items():
        print(k, v)
    base, madd, load, frmul, walk = (ks[k]["mads"] for k in ("k_y_dbl_madd", "k_y_madd", "k_y_load", "k_y_frmul", "k_pm_mul"))
    assert base > 1000 and madd > 500 and 150 <= frmul <= 160      # 81 + 72 multiply-adds per Fr product (fr.hpp) and the address arithmetic
    for k in ("k_gf_table", "k_gf_stage_mul", "k_gf_stage_first", "k_gf_scale"):
        assert ks[k]["scratch"] == 0, (k, ks[k])
        assert ks[k]["dynamic_stack"] == "False", (k, ks[k])
    # rolled: the walk is inlined once whatever the number of digits
    assert walk < 2 * base
    stage = ks["k_gf_stage_mul"]["mads"]
    # the walk, the two mixed additions of the butterfly, LO * HI and the product that takes the twiddle out of Montgomery form, A's image and T's y
    assert stage <= walk + 2 * madd + 2 * frmul + load, (stage, walk, madd, frmul, load)
    pinned = PINNED_STAGE_MADS["fp" if E.startswith("FpEl") else "fp2"]
    assert stage == pinned, (stage, pinned)
    # stage 0 multiplies nothing: two additions and two images
    assert ks["k_gf_stage_first"]["mads"] <= 2 * madd + 2 * load, (ks["k_gf_stage_first"]["mads"], madd, load)
    # the factor of a point outside the stages: the walk and at most three Fr products
    assert ks["k_gf_scale"]["mads"] <= walk + 3 * frmul, (ks["k_gf_scale"]["mads"], walk, frmul)
    # the table build has the doubling, the addition of its loop and the conversions of the input image
    assert ks["k_gf_table"]["mads"] < 3 * base, (ks["k_gf_table"]["mads"], base)
    if E.startswith("FpEl"):
        assert ks["k_gf_stage_mul"]["waves"] >= 2, ks["k_gf_stage_mul"]["vgprs"]
