"""CPU: the cross-compiled gfx950 code of the kernels of csrc/h2c.hpp, judged by the compiler's resource remarks and the count of 64-bit
multiply-adds alone (the method of tests/test_isa_pairing.py).  Pinned for every kernel: no scratch, no dynamic stack, no LDS, at least
two waves per SIMD.  The VGPRs and multiply-adds are printed; DESIGN.md section 4n records them.

What the compiler reports (hipcc -O3, gfx950):
  k_h2c_expand          100 VGPRs, 4 waves per SIMD
  k_h2c_map   over Fp   212 VGPRs, 2 waves
  k_h2c_clear over Fp   241 VGPRs, 2 waves
  k_h2c_map   over Fp2  229 VGPRs, 2 waves
  k_h2c_clear over Fp2  177 VGPRs, 2 waves
none with scratch.  Over Fp2 the values wait in the lane's work slots between products (csrc/h2c.hpp, "over Fp2"; DESIGN.md 4n says why)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SOURCE = """
#include "%(ROOT)s/2022-entries_amd/csrc/h2c.hpp"
namespace msm {
template <class F>
__global__ void k_fp_yardstick(const Fe* a, const Fe* b, Fe* r) {
  const Modulus<F> md;
  Fe x = a[threadIdx.x], y = b[threadIdx.x], z;
  fe_mul<F>(z, x, y, md);
  r[threadIdx.x] = z;
}
template __global__ void k_fp_yardstick<Bls12_381_Fq>(const Fe*, const Fe*, Fe*);
template __global__ void k_h2c_expand<Bls12_381_Fq>(const H2cRun, uint32_t, uint32_t, uint32_t*);
template __global__ void k_h2c_map<FpEl<Bls12_381_Fq>>(const uint32_t*, uint32_t, uint8_t*, XyzzDevT<Fe>*);
template __global__ void k_h2c_clear<FpEl<Bls12_381_Fq>>(const XyzzDevT<Fe>*, uint32_t, uint32_t, uint8_t*, XyzzDevT<Fe>*);
template __global__ void k_h2c_map<Fp2El<Bls12_381_Fq, 1>>(const uint32_t*, uint32_t, uint8_t*, XyzzDevT<Fe2>*);
template __global__ void k_h2c_clear<Fp2El<Bls12_381_Fq, 1>>(const XyzzDevT<Fe2>*, uint32_t, uint32_t, uint8_t*, XyzzDevT<Fe2>*);
}
"""
KERNELS = ["k_h2c_expand", "k_h2c_map/Fp", "k_h2c_clear/Fp", "k_h2c_map/Fp2", "k_h2c_clear/Fp2"]


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(HIPCC), "hipcc is what builds the package: it cannot be missing here"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "h2c.hip"), "w").write(SOURCE % {"ROOT": ROOT})
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "h2c.hip", "-o", "h2c.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "h2c-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fp_yardstick|k_h2c_expand|k_h2c_map|k_h2c_clear)I(\w+)):", asm, flags=re.M):
        name, key = m.group(1), m.group(2)
        if key in ("k_h2c_map", "k_h2c_clear"):
            key += "/Fp2" if "Fp2El" in m.group(3) else "/Fp"
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        out[key] = dict(mads=ops.count("v_mad_u64_u32"), insns=len(ops), scratch_ops=sum(o.startswith("scratch_") for o in ops),
                        scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                        dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                        vgprs=int(re.search(r" VGPRs: (\d+)", blk).group(1)), agprs=int(re.search(r" AGPRs: (\d+)", blk).group(1)),
                        waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                        lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


def test_every_kernel_was_found(kernels):
    assert sorted(kernels) == sorted(KERNELS + ["k_fp_yardstick"])
    assert 360 <= kernels["k_fp_yardstick"]["mads"] <= 400      # one 14 x 28 product: 196 + 182 multiply-adds


@pytest.mark.parametrize("name", KERNELS)
def test_h2c_kernel_isa(kernels, name):
    k = kernels[name]
    print(name, k, "products in the code: %.1f" % (k["mads"] / kernels["k_fp_yardstick"]["mads"]))   # recorded in DESIGN.md 4n
    assert k["dynamic_stack"] == "False" and k["lds"] == 0, (name, k)
    assert k["scratch"] == 0 and k["scratch_ops"] == 0, (name, k)
    assert k["waves"] >= 2, (name, k)
    assert k["mads"] > 0, (name, k)                              # (expand multiplies too: the reduction)
