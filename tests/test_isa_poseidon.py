"""CPU: the cross-compiled gfx950 code of the kernel of csrc/poseidon.hpp, judged by the compiler's resource remarks and the count of
64-bit multiply-adds alone (the method of tests/test_isa_mle.py): no scratch and no dynamic stack, the loops over rounds, elements,
matrix rows and columns and the bits of alpha stay rolled -- the code holds the products DESIGN.md section 4l counts, measured against
the yardstick kernel (one Fr product) --, the text stays far below the instruction cache two CUs share, the round constants and
matrices are read on the scalar unit, and the VGPRs, the LDS and the waves per SIMD are those stated there."""
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
template __global__ void k_poseidon_hash<%(FR)s>(PosRun);
"""
# Fr products in the code of the kernel, each once: an absorbed element to class M and a squeezed one out (2); the two
# places that add a round constant and run the S-box (the dense layer's element loop, element 0 of a sparse partial round), each the
# reduction, the square and the multiply (6); the dense matrix (1); N00 s_0, the reduction of a lazy element, v^_j s_j and w_j s_0 (4).
# Thirteen sites; the two squares have one operand and the compiler takes their symmetric terms once, which saves a quarter of a
# product each: 12.5 yardsticks.
PRODUCTS = 12.5
TEXT_LIMIT = 48 << 10
VGPRS, WAVES, STATIC_LDS = 88, 5, 0           # the state's LDS is dynamic: 2 t * 36 bytes a lane, 64 lanes a block


def _kernels(FR):
    src = '#include "%s/2022-entries_amd/csrc/poseidon.hpp"\nnamespace msm {\n%s\n}\n' % (ROOT, KERNELS % {"FR": FR})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "pos.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "pos.hip", "-o", "pos.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "pos-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for m in re.finditer(r"^(_ZN3msm\d+(k_fr_yardstick|k_poseidon_hash)INS_\d+\w+?Fr29EE\w+):", asm, flags=re.M):
        name, key = m.group(1), m.group(2)
        body = asm[m.end():]
        body = body[:body.index("s_endpgm")]
        blk = remarks[remarks.index("Function Name: " + name):]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        # an upper bound of the text: no gfx950 instruction is longer than 12 bytes (a 64-bit encoding and a literal)
        out[key] = dict(mads=ops.count("v_mad_u64_u32"), insns=len(ops), scalar_loads=sum(o.startswith("s_load") for o in ops),
                        lds_ops=sum(o.startswith("ds_") for o in ops),
                        scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)),
                        dynamic_stack=re.search(r"Dynamic Stack: (\w+)", blk).group(1),
                        vgprs=int(re.search(r" VGPRs: (\d+)", blk).group(1)),
                        waves=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1)),
                        lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("FR", ["Bls12_377_Fr29", "Bls12_381_Fr29"])
def test_poseidon_kernel_isa(FR):
    ks = _kernels(FR)
    assert sorted(ks) == ["k_fr_yardstick", "k_poseidon_hash"]
    for k, v in ks.items():
        print(FR, k, v)                          # VGPRs, LDS and waves per SIMD: recorded in DESIGN.md 4l
    k = ks["k_poseidon_hash"]
    assert k["scratch"] == 0 and k["dynamic_stack"] == "False"
    base = ks["k_fr_yardstick"]["mads"]
    assert 100 <= base <= 162, base              # one 9 x 29 product (tests/test_isa_ntt.py)
    # every product the kernel's code holds, once: a round, element, row, column or exponent loop unrolled into copies would add at
    # least a product
    assert (PRODUCTS - 0.5) * base <= k["mads"] <= (PRODUCTS + 0.5) * base, (k["mads"], base)
    assert k["insns"] * 12 < TEXT_LIMIT, k["insns"]
    assert k["lds"] == STATIC_LDS and k["lds_ops"] > 0           # the state is read and written through LDS
    assert k["scalar_loads"] >= 9, k                                # constants and matrices come in through the scalar unit
    assert k["vgprs"] <= VGPRS and k["waves"] >= WAVES, k
