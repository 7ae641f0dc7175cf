"""What the compiler makes of the kernels behind 640 < T <= 2048 and the pooled final stages: scratch, LDS, resident waves.

Modelled on test_kernel_resources_cpu.py (whose parser and compile step it reuses): attention.hip and rowops.hip are compiled with
build.py's flags plus ``-Rpass-analysis=kernel-resource-usage``, and every instance of ``attn_stream_kernel``, ``attn_resume_kernel``
and ``token_mean_kernel`` is held to no scratch, at most 160 KiB of LDS and the waves per SIMD its header comment states -- where the
LDS block caps the resident workgroups below what the registers allow, the LDS figure is what counts (the compiler's occupancy
remark knows the registers and the static LDS of ONE workgroup).

Not ``gpu``-marked; skipped where no hipcc is found.
"""
from __future__ import annotations

import concurrent.futures as cf

import pytest

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

SOURCES = ("attention.hip", "rowops.hip")
LDS_PER_CU = 160 * 1024

# instance -> (source, mangled name up to the argument list, least waves per SIMD its header comment states).  t = unsigned short =
# bf16 storage, f = float.  attn_stream_kernel: attention.hip's comment (<float, 64>: 66 KB of LDS = two workgroups per CU); the
# resume kernel: 32 KiB of LDS per workgroup = five per CU, stated as 4; token_mean_kernel: ln_kernel's 6.
EXPECTED = {
    "attn_stream_kernel<float, 32>": ("attention.hip", "18attn_stream_kernelIfLi32EEEv", 3),
    "attn_stream_kernel<float, 64>": ("attention.hip", "18attn_stream_kernelIfLi64EEEv", 2),
    "attn_stream_kernel<bf16, 32>": ("attention.hip", "18attn_stream_kernelItLi32EEEv", 3),
    "attn_stream_kernel<bf16, 64>": ("attention.hip", "18attn_stream_kernelItLi64EEEv", 3),
    "attn_resume_kernel<float>": ("attention.hip", "18attn_resume_kernelIfEEv", 4),
    "attn_resume_kernel<bf16>": ("attention.hip", "18attn_resume_kernelItEEv", 4),
    "token_mean_kernel<float, false>": ("rowops.hip", "17token_mean_kernelIfLb0EEEv", 6),
    "token_mean_kernel<float, true>": ("rowops.hip", "17token_mean_kernelIfLb1EEEv", 6),
    "token_mean_kernel<bf16, false>": ("rowops.hip", "17token_mean_kernelItLb0EEEv", 6),
    "token_mean_kernel<bf16, true>": ("rowops.hip", "17token_mean_kernelItLb1EEEv", 6),
}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    outdir = str(tmp_path_factory.mktemp("kernel_resources_long"))
    with cf.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        reports = list(ex.map(lambda s: compile_report(hipcc, s, outdir), SOURCES))
    table = {}
    for src, text in zip(SOURCES, reports):
        parsed = parse_resource_report(text)
        assert parsed, f"{src}: hipcc printed no kernel-resource-usage remarks"
        for mangled, res in parsed.items():
            table[(src, mangled)] = res
    return table


@pytest.mark.parametrize("kernel", sorted(EXPECTED))
def test_long_attention_kernels_scratch_lds_and_waves(resources, kernel):
    src, fragment, floor = EXPECTED[kernel]
    hits = [k for k in resources if k[0] == src and fragment in k[1]]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels {src} compiles to: {sorted(m for s_, m in resources if s_ == src)}"
    got = resources[hits[0]]
    print(f"{kernel}: {got}")
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["lds"] <= LDS_PER_CU, f"{kernel}: {got['lds']} bytes of LDS per workgroup: {got}"
    # 256-thread workgroups: one wave per SIMD each; resident workgroups per CU = the lesser of what registers and LDS admit
    by_lds = LDS_PER_CU // got["lds"] if got["lds"] else 8
    waves = min(got["occupancy"], by_lds)
    assert waves >= floor, f"{kernel}: {waves} waves per SIMD (registers {got['occupancy']}, LDS {by_lds}), the design states >= {floor}: {got}"


def test_every_instance_of_the_new_kernels_is_listed(resources):
    """An instance added later (another d_head, another dtype) must be given its floor here."""
    listed = {v[1] for v in EXPECTED.values()}
    for src, mangled in resources:
        for name in ("attn_stream_kernel", "attn_resume_kernel", "token_mean_kernel"):
            if name in mangled:
                assert any(f in mangled for f in listed), f"{mangled} has no entry in EXPECTED"
