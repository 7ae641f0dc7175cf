"""What the compiler makes of the text tower's kernels: attn_causal_kernel (csrc/attention_causal.hip), token_embed_kernel and
eot_rows_kernel (csrc/rowops.hip).

Modelled on test_kernel_resources_cpu.py / test_attention_long_resources_cpu.py (whose parser and compile step it reuses): the sources
are compiled with build.py's flags plus ``-Rpass-analysis=kernel-resource-usage``.  attn_causal_kernel is held to no scratch and to at
least the waves per SIMD attn_stream_kernel states for the same instance (the same body, the same launch bounds: 3, 3, 3, and 2 for
<float, 64>, whose 66 KB of LDS admit two workgroups per CU); the two row kernels to no scratch.

Not ``gpu``-marked; skipped where no hipcc is found.
"""
from __future__ import annotations

import concurrent.futures as cf

import pytest

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

SOURCES = ("attention_causal.hip", "rowops.hip")
LDS_PER_CU = 160 * 1024

# instance -> (source, mangled-name fragment, least waves per SIMD).  t = unsigned short = bf16 storage, f = float.
CAUSAL = {
    "attn_causal_kernel<float, 32>": ("attention_causal.hip", "18attn_causal_kernelIfLi32EEEv", 3),
    "attn_causal_kernel<float, 64>": ("attention_causal.hip", "18attn_causal_kernelIfLi64EEEv", 2),
    "attn_causal_kernel<bf16, 32>": ("attention_causal.hip", "18attn_causal_kernelItLi32EEEv", 3),
    "attn_causal_kernel<bf16, 64>": ("attention_causal.hip", "18attn_causal_kernelItLi64EEEv", 3),
}
ROWS = {
    "token_embed_kernel<float>": ("rowops.hip", "18token_embed_kernelIfEEv"),
    "token_embed_kernel<bf16>": ("rowops.hip", "18token_embed_kernelItEEv"),
    "eot_rows_kernel<float>": ("rowops.hip", "15eot_rows_kernelIfEEv"),
    "eot_rows_kernel<bf16>": ("rowops.hip", "15eot_rows_kernelItEEv"),
}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    outdir = str(tmp_path_factory.mktemp("kernel_resources_text"))
    with cf.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        reports = list(ex.map(lambda s: compile_report(hipcc, s, outdir), SOURCES))
    table = {}
    for src, text in zip(SOURCES, reports):
        parsed = parse_resource_report(text)
        assert parsed, f"{src}: hipcc printed no kernel-resource-usage remarks"
        for mangled, res in parsed.items():
            table[(src, mangled)] = res
    return table


def _one(resources, kernel, src, fragment):
    hits = [k for k in resources if k[0] == src and fragment in k[1]]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels {src} compiles to: {sorted(m for s_, m in resources if s_ == src)}"
    got = resources[hits[0]]
    print(f"{kernel}: {got}")
    return got


@pytest.mark.parametrize("kernel", sorted(CAUSAL))
def test_causal_attention_scratch_lds_and_waves(resources, kernel):
    src, fragment, floor = CAUSAL[kernel]
    got = _one(resources, kernel, src, fragment)
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert 0 < got["lds"] <= LDS_PER_CU, f"{kernel}: {got['lds']} bytes of LDS per workgroup: {got}"
    waves = min(got["occupancy"], LDS_PER_CU // got["lds"])          # 256-thread workgroups: one wave per SIMD each
    assert waves >= floor, f"{kernel}: {waves} waves per SIMD (registers {got['occupancy']}, LDS {LDS_PER_CU // got['lds']}), stated >= {floor}: {got}"


@pytest.mark.parametrize("kernel", sorted(ROWS))
def test_text_row_kernels_have_no_scratch(resources, kernel):
    src, fragment = ROWS[kernel]
    got = _one(resources, kernel, src, fragment)
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"


def test_only_the_four_causal_instances_exist(resources):
    listed = {v[1] for v in CAUSAL.values()}
    causal = [m for s, m in resources if s == "attention_causal.hip"]
    assert len(causal) == 4 and all(any(f in m for f in listed) for m in causal), causal
