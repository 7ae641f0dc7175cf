"""What the compiler makes of the kernels the B/32 and L/14 forwards launch: registers, scratch, resident waves.

The designs of these kernels are stated in waves per SIMD: LDS blocks are sized for them, latency hiding is reasoned
from them.  Twice the shipped binary did not have the occupancy its header comment promised (the SAE select kernel six-deep
instead of eight; ``attn_wave_kernel<64, true>`` with its accumulators parked in 64 AGPRs on top of 105 VGPRs: two waves per
SIMD where its LDS was sized for four).  hipcc cross-compiles without a GPU, so this is checked here: attention.hip, rowops.hip,
gemm.hip, sae_enc_gemm.hip and sae_enc.hip are compiled with build.py's flags plus ``-Rpass-analysis=kernel-resource-usage`` and the report is held against
the table below.

Not ``gpu``-marked; skipped where no hipcc is found.  About a minute of compiling (the five sources in parallel).
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import re
import subprocess

import pytest

from vit_prisma_amd import build as pv_build

SOURCES = ("attention.hip", "rowops.hip", "gemm.hip", "sae_enc_gemm.hip", "sae_enc.hip")

# instance -> (source, its mangled name up to the argument list, least waves per SIMD the design states).  Scratch must be 0 for
# all.  The floor is the DESIGN's figure, not a snapshot: a kernel may do better.  (Mangled: t = unsigned short = bf16 storage,
# Li5E = the integer 5, Lb1E = true; the report names kernels that way and no demangler is needed.)
EXPECTED = {
    # B/32 attention: 9 KB of LDS per wave = 16 waves per CU = 4 per SIMD (<d_head, staged rows, V as whole rows>)
    "attn_wave_kernel<64, true, true>": ("attention.hip", "16attn_wave_kernelILi64ELb1ELb1EEEv", 4),
    "attn_wave_kernel<64, false, false>": ("attention.hip", "16attn_wave_kernelILi64ELb0ELb0EEEv", 4),
    "attn_wave_kernel<32, true, true>": ("attention.hip", "16attn_wave_kernelILi32ELb1ELb1EEEv", 4),
    "attn_wave_kernel<32, false, false>": ("attention.hip", "16attn_wave_kernelILi32ELb0ELb0EEEv", 4),
    # L/14 attention: three 4-wave workgroups per CU
    "attn_lean_kernel<64, true>": ("attention.hip", "16attn_lean_kernelILi64ELb1EEEv", 3),
    "attn_lean_kernel<64, false>": ("attention.hip", "16attn_lean_kernelILi64ELb0EEEv", 3),
    # LayerNorm: HBM-bound row kernel
    "ln_kernel<bf16, false>": ("rowops.hip", "9ln_kernelItLb0EEEv", 6),
    # the bf16 GEMM family: one 512-thread workgroup per CU = 2 waves per SIMD; v4: three 256-thread workgroups
    "gemm_kernel_v8<bf16, 5, 1, 0>": ("gemm.hip", "14gemm_kernel_v8ItLi5ELi1ELi0EEEv", 2),
    "gemm_kernel_v8<bf16, 5, 3, 0>": ("gemm.hip", "14gemm_kernel_v8ItLi5ELi3ELi0EEEv", 2),
    "gemm_kernel_v7<bf16, 5, 2, 0, 2>": ("gemm.hip", "14gemm_kernel_v7ItLi5ELi2ELi0ELi2EEEv", 2),
    "gemm_kernel_v7<bf16, 5, 0, 0, 0>": ("gemm.hip", "14gemm_kernel_v7ItLi5ELi0ELi0ELi0EEEv", 2),
    "gemm_kernel_v4<bf16>": ("gemm.hip", "14gemm_kernel_v4ItEEv", 3),
    # every user of the shared K loop (kloop.hpp): the pipelined 64-byte-slab form and the persistent kernel at MB = 4, and the SAE
    # filter GEMM <MODE, LP, ONE, MB> -- the bench shape's filter pass with and without the one-round epilogue, the 128-row sample
    # pass, the pipelined sample pass
    "gemm_kernel_v7<bf16, 4, 3, 1, 1>": ("gemm.hip", "14gemm_kernel_v7ItLi4ELi3ELi1ELi1EEEv", 2),
    "gemm_kernel_v8<bf16, 4, 2, 0>": ("gemm.hip", "14gemm_kernel_v8ItLi4ELi2ELi0EEEv", 2),
    "sae_enc_gemm_kernel<1, 2, false, 4>": ("sae_enc_gemm.hip", "19sae_enc_gemm_kernelILi1ELi2ELb0ELi4EEEv", 2),
    "sae_enc_gemm_kernel<1, 2, true, 4>": ("sae_enc_gemm.hip", "19sae_enc_gemm_kernelILi1ELi2ELb1ELi4EEEv", 2),
    "sae_enc_gemm_kernel<0, 2, false, 2>": ("sae_enc_gemm.hip", "19sae_enc_gemm_kernelILi0ELi2ELb0ELi2EEEv", 2),
    "sae_enc_gemm_kernel<0, 1, false, 4>": ("sae_enc_gemm.hip", "19sae_enc_gemm_kernelILi0ELi1ELb0ELi4EEEv", 2),
    # the top-k select kernel at the bench width (d_in 768), listed and inline fallback: its own PV_SEL_WAVES launch bound
    "sae_select_kernel<3, false>": ("sae_enc.hip", "17sae_select_kernelILi3ELb0EEEv", 8),
    "sae_select_kernel<3, true>": ("sae_enc.hip", "17sae_select_kernelILi3ELb1EEEv", 8),
}

_FIELDS = {
    "VGPRs": "vgprs",
    "AGPRs": "agprs",
    "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy",
    "LDS Size [bytes/block]": "lds",
}


def _find_hipcc():
    try:
        return pv_build._hipcc()
    except RuntimeError:
        return None


def parse_resource_report(text: str) -> dict:
    """{mangled kernel name: {vgprs, agprs, scratch, occupancy, lds}} from hipcc's kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in _FIELDS:
            cur[_FIELDS[m.group(1)]] = int(m.group(2))
    return out


def compile_report(hipcc: str, src: str, outdir: str) -> str:
    cmd = [hipcc, *pv_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(pv_build.CSRC, src),
           "-o", os.path.join(outdir, src.replace(".hip", ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"hipcc failed for {src}:\n{r.stderr[-4000:]}"
    return r.stderr


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    outdir = str(tmp_path_factory.mktemp("kernel_resources"))
    with cf.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        reports = list(ex.map(lambda s: compile_report(hipcc, s, outdir), SOURCES))
    table = {}
    for src, text in zip(SOURCES, reports):
        parsed = parse_resource_report(text)
        assert parsed, f"{src}: hipcc printed no kernel-resource-usage remarks"
        for mangled, res in parsed.items():
            table[(src, mangled)] = res
    return table


def test_report_parser_reads_the_compiler_format():
    text = (
        "a.hip:310:1: remark: Function Name: _ZN12_GLOBAL__N_116attn_wave_kernelILi64ELb1EEEv10AttnParams [-Rpass-analysis=kernel-resource-usage]\n"
        "  310 | __global__ void k() {\n"
        "a.hip:310:1: remark:     TotalSGPRs: 106 [-Rpass-analysis=kernel-resource-usage]\n"
        "a.hip:310:1: remark:     VGPRs: 105 [-Rpass-analysis=kernel-resource-usage]\n"
        "a.hip:310:1: remark:     AGPRs: 64 [-Rpass-analysis=kernel-resource-usage]\n"
        "a.hip:310:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
        "a.hip:310:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]\n"
        "a.hip:310:1: remark:     LDS Size [bytes/block]: 36864 [-Rpass-analysis=kernel-resource-usage]\n")
    got = parse_resource_report(text)
    assert got == {"_ZN12_GLOBAL__N_116attn_wave_kernelILi64ELb1EEEv10AttnParams":
                   {"vgprs": 105, "agprs": 64, "scratch": 0, "occupancy": 2, "lds": 36864}}


@pytest.mark.parametrize("kernel", sorted(EXPECTED))
def test_kernel_occupancy_and_scratch(resources, kernel):
    src, fragment, floor = EXPECTED[kernel]
    hits = [k for k in resources if k[0] == src and fragment in k[1]]
    assert len(hits) == 1, (f"{kernel} ({fragment}) is not among the kernels {src} compiles to: "
                            f"{sorted(m for s_, m in resources if s_ == src and fragment[2:fragment.index('I')] in m)}")
    got = resources[hits[0]]
    print(f"{kernel}: {got}")
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["occupancy"] >= floor, f"{kernel}: {got['occupancy']} waves per SIMD, the design states >= {floor}: {got}"


def test_wave_attention_lds_matches_its_occupancy(resources):
    """Four 4-wave blocks of attn_wave_kernel fit a CU's 160 KiB of LDS: the LDS must not be what caps it below 4 per SIMD."""
    got = next(v for k, v in resources.items() if EXPECTED["attn_wave_kernel<64, true, true>"][1] in k[1])
    assert got["lds"] * 4 <= 160 * 1024, got
    assert got["agprs"] == 0, f"the accumulators went to AGPRs on top of the VGPRs again: {got}"
