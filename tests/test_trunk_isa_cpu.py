"""Build-time guard for the persistent trunk's fp32 issue forms (the single-issue
col_comb / combine_kx of csrc/conv_wino4.hip): both fp16x2 instantiations of k_trunk_wino4 in the built library hold the
packed-fp32 count the shipped default claims -- the input transform single-issue (no packed
fp32 left in it), the fold, the epilogues and the heads packed as before -- use no scratch,
and keep two waves per SIMD (at most 256 vector registers of the SIMD's 512 per lane).  CPU
only: llvm-objdump / llvm-readelf on the .so, skipped without them."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "scripts"), os.path.join(ROOT, "alphazero-othello_amd")]
import ds_war_scan as scan  # noqa: E402

LIB = os.environ.get("AZ_ISA_LIB") or os.path.join(ROOT, "alphazero-othello_amd", "libaz_othello.so")
OBJDUMP = os.path.join(scan.LLVM, "llvm-objdump")
READELF = os.path.join(scan.LLVM, "llvm-readelf")
# k_trunk_wino4<W4<AZ_CONV_FP16X2 = 2, 1, 2, 8, 4>, heads = false / true>
FP16X2 = re.compile(r"k_trunk_wino4INS_2W4ILi2ELi1ELi2ELi8ELi4EEELb[01]E")
# v_pk_{add,mul,fma}_f32 per kernel (without / with the fused heads) with the single-issue
# input transform; the commit before it: 2,976 / 1,992, every part single-issue: 0 / 0
PACKED_F32_SHIPPED = {"Lb0E": 1514, "Lb1E": 1017}

needs_tools = pytest.mark.skipif(
    not (os.path.exists(LIB) and os.path.exists(OBJDUMP) and os.path.exists(READELF)),
    reason="needs the built library, llvm-objdump and llvm-readelf")


def kernel_notes(path):
    """{kernel symbol: {metadata key: int}} from the gfx950 code objects' notes."""
    out = {}
    with tempfile.TemporaryDirectory(prefix="trunkisa_") as tmp:
        lib = os.path.join(tmp, "lib.so")
        with open(path, "rb") as src, open(lib, "wb") as dst:
            dst.write(src.read())
        subprocess.run([OBJDUMP, "--offloading", lib], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" in f and "gfx950" in f:
                notes = subprocess.run([READELF, "--notes", os.path.join(tmp, f)], check=True,
                                       capture_output=True, text=True).stdout
                for block in notes.split("\n  - ")[1:]:
                    name = re.search(r"^\s*\.name:\s+(\S+)", block, re.M)
                    if name:
                        out[name.group(1)] = {k: int(v) for k, v in
                                              re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def packed_f32_counts(path, pattern):
    """{kernel symbol: number of v_pk_{add,mul,fma}_f32} for the kernels matching pattern."""
    counts = {}
    for _, text in scan.disassemble_so(path):
        cur = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
            if m:
                cur = m.group(1) if pattern.search(m.group(1)) else None
                if cur:
                    counts[cur] = 0
            elif cur and scan.PK_PRODUCER.match(line.strip().split(" ")[0].split("\t")[0]):
                counts[cur] += 1
    return counts


@needs_tools
def test_fp16x2_trunk_kernels_hold_the_shipped_packed_f32_count():
    counts = packed_f32_counts(LIB, FP16X2)
    assert len(counts) == 2, counts  # with and without the fused heads
    for k, c in counts.items():
        assert c == PACKED_F32_SHIPPED[FP16X2.search(k).group(0)[-4:]], counts


@needs_tools
def test_fp16x2_trunk_kernels_have_no_scratch_and_two_waves_per_simd():
    notes = {k: v for k, v in kernel_notes(LIB).items() if FP16X2.search(k) and not k.endswith(".kd")}
    assert len(notes) == 2, sorted(notes)
    for k, n in notes.items():
        assert n["private_segment_fixed_size"] == 0, (k, n)
        assert n.get("vgpr_spill_count", 0) == 0, (k, n)
        # gfx950: 512 unified vector registers per lane and SIMD; waves per SIMD = 512 // the
        # kernel's allocation (VGPRs + AGPRs, in blocks of 8)
        alloc = -(-(n["vgpr_count"] + n.get("agpr_count", 0)) // 8) * 8
        assert 512 // alloc >= 2, (k, n["vgpr_count"], n.get("agpr_count"))
        assert n["max_flat_workgroup_size"] == 256, (k, n)
