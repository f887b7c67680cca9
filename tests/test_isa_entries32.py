"""ISA-level regression tests (no GPU needed) for the 32-bit sorted entries (csrc/msm_types.hpp Entries32).

The twisted-Edwards accumulation sits at its register limit for three waves per SIMD, and its entry queue exists so that no entry
costs a memory request of its own: the Entries32 instantiation of k_accumulate_glds must keep both -- measured against the 64-bit
instantiation compiled in the same run -- and the last grouping pass, which now writes the format, must stay within the LDS and
register bounds of a 1024-thread block."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARGS = "const uint32_t*, uint32_t, const TeAffineDev*, SegOut, uint32_t, uint32_t*"
KERNEL = "_ZN3msm17k_accumulate_gldsINS_5TeLawINS_14Bls12_377_Fq29EEENS_9%sE"


def _compile_both():
    """-> {format: (body, ops, resources)} of k_accumulate_glds<TeLaw<Bls12_377_Fq29>> for Entries64 (the default) and Entries32"""
    src = ('#include "%s/2022-entries_amd/csrc/msm_kernels.hpp"\nnamespace msm {\n'
           "template __global__ void k_accumulate_glds<TeLaw<Bls12_377_Fq29>>(const uint2*, %s);\n"
           "template __global__ void k_accumulate_glds<TeLaw<Bls12_377_Fq29>, Entries32>(Entries32Ptr, %s);\n}\n" % (ROOT, ARGS, ARGS))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "acc.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "acc.hip", "-o", "acc.o", "-save-temps",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(d, "acc-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        remarks = r.stderr
    out = {}
    for fmt in ("Entries64", "Entries32"):
        name = KERNEL % fmt
        body = asm[asm.index(name):]          # (its .globl directive: behind every other kernel's code)
        body = body[:body.index("s_endpgm")]
        ops = re.findall(r"^\s+([a-z_0-9]+)", body, flags=re.M)
        blk = remarks[remarks.index("Function Name: " + name):]
        res = {k: int(re.search(pat, blk).group(1)) for k, pat in
               (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                ("vgprs", r"VGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))}
        out[fmt] = (body, ops, res)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_entries32_accumulate_kernel_isa():
    both = _compile_both()
    body64, ops64, res64 = both["Entries64"]
    body, ops, res = both["Entries32"]
    mads = ops.count("v_mad_u64_u32")
    assert 2359 <= mads <= 2410, mads                     # 7 multiplications of 337 multiply-adds: the addition is untouched
    assert mads == ops64.count("v_mad_u64_u32")
    assert res["scratch"] == 0 and "scratch_" not in body
    assert res["vgprs"] <= res64["vgprs"], (res["vgprs"], res64["vgprs"])
    assert res["occupancy"] == 3 and res64["occupancy"] == 3
    assert res["lds"] == res64["lds"]
    # the entries arrive through the same register queue: 16-byte loads only (16 entries per 64-byte refill).  The 4-byte loads the
    # kernel has are the cold ones the 64-bit form has too -- the words of a carried bucket's record that are no whole 16 bytes, and ONE
    # key: run_keys[e] at a lane start or an escape, where the 64-bit form reads the key of the entry before the lane
    assert ops.count("global_load_dwordx2") == 0 and ops64.count("global_load_dwordx2") == 0
    assert ops.count("global_load_dword") <= ops64.count("global_load_dword"), (ops.count("global_load_dword"), ops64.count("global_load_dword"))
    assert ops.count("global_load_dwordx4") == ops64.count("global_load_dwordx4") >= 2 * 4
    assert ops.count("global_load_dwordx3") == 0 and ops.count("global_load_ushort") == 0 and ops.count("global_load_ubyte") == 0
    # the gathers: 4 records x 3 sectors by LDS-DMA, at the prologue and in the loop
    assert ops.count("global_load_lds_dwordx4") == ops64.count("global_load_lds_dwordx4") == 2 * 4 * 3
    assert ops.count("ds_write_b128") == 0 and "s_set_gpr_idx_on" not in body and "v_accvgpr" not in body
    # the rest of the VALU stream: the queue moves by one word per entry (16 moves where the 64-bit form has 14), the run test is a
    # bit-field extract; nothing else may grow (static count of the whole kernel, the 64-bit form's bound is 1200)
    valu = [o for o in ops if o.startswith("v_")]
    valu64 = [o for o in ops64 if o.startswith("v_")]
    assert len(valu) - mads <= 1300 and len(valu) <= len(valu64) + 100, (len(valu), len(valu64))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_entries32_pass_scatter_isa():
    """Both forms of the last pass's scatter: no scratch, <= 128 VGPRs (1024 threads per block), and the LDS of the 64-bit form -- the
    steps travel in the high half of a word the block keeps anyway."""
    src = '#include "%s/2022-entries_amd/csrc/partition.hip"\n' % ROOT
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "part.hip"), "w").write(src)
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-c", "part.hip", "-o", "part.o",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        remarks = r.stderr
    seen = {}
    for blk in remarks.split("Function Name: ")[1:]:
        name = blk.split()[0]
        if "k_pass_scatter" not in name:
            continue
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
        assert scratch == 0 and vgprs <= 128 and 64 * 1024 <= lds <= 150 * 1024, (name, scratch, vgprs, lds)
        seen["Lb1" in name] = lds
    assert set(seen) == {False, True}, seen          # k_pass_scatter<false> and k_pass_scatter<true>
    assert seen[True] == seen[False]
