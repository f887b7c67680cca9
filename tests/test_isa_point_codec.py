"""CPU: the cross-compiled gfx950 code of the point-codec kernels (csrc/point_codec.hpp): no scratch, no dynamic stack, no dynamic
register indexing, and the exponent and Tonelli-Shanks loops ROLLED -- the multiply count of each decompress kernel is pinned and
measured against a yardstick kernel that does one product and one squaring of the kernel's coordinate field."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SRC = """
template <class E>
__global__ void __launch_bounds__(256) k_yardstick(const typename E::T* in, typename E::T* out) {
  typename E::Md md;
  typename E::T a = in[threadIdx.x], b = in[threadIdx.x + 256], r, s;
  E::mul(r, a, b, md);
  E::sqr(s, r, md);
  out[threadIdx.x] = s;
}
template __global__ void k_yardstick<%(E)s>(const %(E)s::T*, %(E)s::T*);
template __global__ void k_decompress_points<%(E)s, false>(const uint8_t*, uint32_t, uint8_t*, size_t, uint8_t*);
template __global__ void k_decompress_points<%(E)s, true>(const uint8_t*, uint32_t, uint8_t*, size_t, uint8_t*);
template __global__ void k_compress_points<%(E)s, false>(const uint8_t*, size_t, uint32_t, uint8_t*, uint8_t*);
template __global__ void k_compress_points<%(E)s, true>(const uint8_t*, size_t, uint32_t, uint8_t*, uint8_t*);
"""

# v_mad_u64_u32 per decompress kernel (images, uncompressed records) as hipcc gives them, and the VGPRs DESIGN section 4c quotes
PINNED = {
    "FpEl<Bls12_377_Fq>": {"mads": (6548, 6169), "vgprs": (111, 108)},
    "FpEl<Bls12_381_Fq>": {"mads": (4644, 4251), "vgprs": (103, 100)},
    "Fp2El<Bls12_377_Fq, 5>": {"mads": (13616, 12859), "vgprs": (212, 206)},
    "Fp2El<Bls12_381_Fq, 1>": {"mads": (11910, 11125), "vgprs": (204, 199)},
}


def _kernels(E):
    src = '#include "%s/2022-entries_amd/csrc/point_codec.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, SRC % {"E": E})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "codec.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "codec.hip", "-o", "codec.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "codec-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm(?:11k_yardstick|19k_decompress_points|17k_compress_points)\w+):", asm, flags=re.M):
        name = m.group(1)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        blk = blk[:blk.index("LDS Size")]
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        dyn = re.search(r"Dynamic Stack: (\w+)", blk).group(1)
        vgprs = int(re.search(r" VGPRs: (\d+)", blk).group(1))
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[name] = dict(body=body, mads=ops.count("v_mad_u64_u32"), scratch=scratch, dynamic_stack=dyn, vgprs=vgprs)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("E", sorted(PINNED), ids=["fp2_377", "fp2_381", "fp_377", "fp_381"])
def test_codec_kernel_isa(E):
    ks = _kernels(E)
    yard = [v for k, v in ks.items() if "k_yardstick" in k]
    dec = {("Lb1E" in k): v for k, v in ks.items() if "k_decompress_points" in k}     # keyed by OUT_SERIALIZED
    enc = [v for k, v in ks.items() if "k_compress_points" in k]
    assert len(yard) == 1 and len(dec) == 2 and len(enc) == 2
    base = yard[0]["mads"]      # one product + one squaring of the coordinate field
    assert base > 500
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["dynamic_stack"] == "False", (name, k["scratch"], k["dynamic_stack"])
        assert "s_set_gpr_idx_on" not in k["body"] and "scratch_" not in k["body"], name
    got = (dec[False]["mads"], dec[True]["mads"])
    print(E, "yardstick", base, "decompress mads", got, "vgprs", (dec[False]["vgprs"], dec[True]["vgprs"]),
          "compress mads", [k["mads"] for k in enc], "vgprs", [k["vgprs"] for k in enc])
    for k in dec.values():
        # rolled: the (p + 1)/4 exponent alone is 379 squarings, a Tonelli-Shanks 990 more
        assert k["mads"] < 16 * base, (k["mads"], base)
    assert got == PINNED[E]["mads"]
    assert (dec[False]["vgprs"], dec[True]["vgprs"]) == PINNED[E]["vgprs"]
    for k in enc:
        assert k["mads"] < 6 * base
