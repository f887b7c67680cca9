"""CPU: the cross-compiled gfx950 code of k_check_points (csrc/check_points.hpp): no scratch, no dynamic register indexing, and the
double-and-add loop ROLLED -- measured against a yardstick kernel that does one xyzz_dbl and one xyzz_madd."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

YARDSTICK = """
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
template __global__ void k_check_points<%(E)s, false, CHECK_EXACT>(const uint8_t*, size_t, uint32_t, uint8_t*);
template __global__ void k_check_points<%(E)s, true, CHECK_ENDO>(const uint8_t*, size_t, uint32_t, uint8_t*);
"""


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/check_points.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, YARDSTICK % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "chk.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "chk.hip", "-o", "chk.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "chk-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm(?:11k_yardstick|14k_check_points)\w+):", asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[name] = (body, ops.count("v_mad_u64_u32"), scratch)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", ["FpEl<Bls12_377_Fq>", "Fp2El<Bls12_381_Fq, 1>"], ids=["fp", "fp2"])
def test_check_kernel_isa(E):
    ks = _kernels(E)
    yard = [v for k, v in ks.items() if "k_yardstick" in k]
    checks = {k: v for k, v in ks.items() if "k_check_points" in k}
    assert len(yard) == 1 and len(checks) == 2
    base = yard[0][1]
    assert base > 1000
    for name, (body, mads, scratch) in checks.items():
        assert scratch == 0, (name, scratch)
        assert "s_set_gpr_idx_on" not in body and "scratch_" not in body, name
        assert mads < 10 * base, (name, mads, base)       # rolled: an unrolled loop would be above 60 times
