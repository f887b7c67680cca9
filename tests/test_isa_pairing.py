"""CPU: the cross-compiled gfx950 code of the three kernels of csrc/pairing.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_poseidon.py): no scratch and no dynamic stack; each kernel holds exactly ONE
Fp2 product -- the tower, the bits of x and the steps of the chain are data, not code, so an unrolled loop would add at least a product
--, measured against the yardstick kernel (one Fp product); the text stays below 48 KB; the operations and constants are read on the
scalar unit; and the VGPRs and the waves per SIMD are those DESIGN.md section 4m records."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SOURCE = """
#include "%(ROOT)s/2022-entries_amd/csrc/pairing.hpp"
namespace msm {
template <class F>
__global__ void k_fp_yardstick(const Fe* a, const Fe* b, Fe* r) {
  const Modulus<F> md;
  Fe x = a[threadIdx.x], y = b[threadIdx.x], z;
  fe_mul<F>(z, x, y, md);
  r[threadIdx.x] = z;
}
template __global__ void k_fp_yardstick<%(F)s>(const Fe*, const Fe*, Fe*);
template __global__ void k_pairing_miller<Fp2El<%(F)s, %(NB)s>>(PrRun, uint64_t);
template __global__ void k_pairing_product<Fp2El<%(F)s, %(NB)s>>(PrRun, uint64_t);
template __global__ void k_pairing_final<Fp2El<%(F)s, %(NB)s>>(PrRun, uint64_t);
}
"""
# Fp products in the code of each kernel: the interpreter's one Fp2 product is two fused dual products, 2 * (2 * 196 + 182)
# multiply-adds against the 196 + 182 of the yardstick -- 3.04 of them -- and nothing else multiplies: the ABI boundary is crossed by
# products of the programs.
PRODUCTS = 3.04
TEXT_LIMIT = 48 << 10
VGPRS, WAVES, LDS = 211, 2, 0


def _kernels(F, NB):
    src = SOURCE % {"ROOT": ROOT, "F": F, "NB": NB}
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "pr.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "pr.hip", "-o", "pr.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "pr-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fp_yardstick|k_pairing_miller|k_pairing_product|k_pairing_final)I\w+):", asm, flags=re.M):
        name, key = m.group(1), m.group(2)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        # an upper bound of the text: no gfx950 instruction is longer than 12 bytes (a 64-bit encoding and a literal)
        out[key] = dict(mads=ops.count("v_mad_u64_u32"), insns=len(ops), scalar_loads=sum(o.startswith("s_load") for o in ops),
                        scratch_ops=sum(o.startswith("scratch_") for o in ops),
                        scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                        dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                        vgprs=int(re.search(r" VGPRs: (\d+)", blk).group(1)),
                        waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                        lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.parametrize("F,NB", [("Bls12_377_Fq", 5), ("Bls12_381_Fq", 1)])
def test_pairing_kernels_isa(F, NB):
    assert os.path.exists(HIPCC), "hipcc is what builds the package: it cannot be missing here"
    ks = _kernels(F, NB)
    assert sorted(ks) == ["k_fp_yardstick", "k_pairing_final", "k_pairing_miller", "k_pairing_product"]
    for k, v in ks.items():
        print(F, k, v)                           # VGPRs and waves per SIMD: recorded in DESIGN.md 4m
    base = ks["k_fp_yardstick"]["mads"]
    assert 360 <= base <= 400, base              # one 14 x 28 product: 196 + 182 multiply-adds (BLS12-377's p_0 = 1 saves the 14 of m p_0)
    for name in ("k_pairing_miller", "k_pairing_product", "k_pairing_final"):
        k = ks[name]
        assert k["scratch"] == 0 and k["scratch_ops"] == 0 and k["dynamic_stack"] == "False", (name, k)
        # every product the kernel's code holds, once: a tower, bit or chain loop unrolled into copies would add at least a product
        assert (PRODUCTS - 0.5) * base <= k["mads"] <= (PRODUCTS + 0.5) * base, (name, k["mads"], base)
        assert k["insns"] * 12 < TEXT_LIMIT, (name, k["insns"])
        assert k["lds"] == LDS, (name, k)
        assert k["scalar_loads"] >= 9, (name, k)                     # operations and constants come in through the scalar unit
        assert k["vgprs"] <= VGPRS and k["waves"] >= WAVES, (name, k)
