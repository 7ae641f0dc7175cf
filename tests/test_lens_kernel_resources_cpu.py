"""What the compiler makes of the logit-lens kernels (csrc/lens.hip): the eight instances of lens_gemm_kernel<MODE, MB, LP> and the
two row kernels.

Modelled on test_text_kernel_resources_cpu.py (whose parser and compile step it reuses): lens.hip is compiled with build.py's flags
plus ``-Rpass-analysis=kernel-resource-usage``.  lens_gemm_kernel is a one-workgroup-per-CU kernel like gemm_kernel_v7: 512 threads
= 2 waves per SIMD, no scratch, and its ring (four 64-byte-slab slots or two full-line slots) within the CU's 160 KiB of LDS.

Not ``gpu``-marked; skipped where no hipcc is found.
"""
from __future__ import annotations

import pytest

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

LDS_PER_CU = 160 * 1024
GEMM = {f"lens_gemm_kernel<{mode}, {mb}, {lp}>": f"16lens_gemm_kernelILi{mode}ELi{mb}ELi{lp}EEEv"
        for mode in (0, 1) for mb in (2, 4) for lp in (0, 2)}
ROWS = {"lens_rowstat_kernel": "19lens_rowstat_kernelE", "lens_top_finish_kernel": "22lens_top_finish_kernelE"}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    parsed = parse_resource_report(compile_report(hipcc, "lens.hip", str(tmp_path_factory.mktemp("kernel_resources_lens"))))
    assert parsed, "lens.hip: hipcc printed no kernel-resource-usage remarks"
    return parsed


def _one(resources, kernel, fragment):
    hits = [m for m in resources if fragment in m]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels lens.hip compiles to: {sorted(resources)}"
    print(f"{kernel}: {resources[hits[0]]}")
    return resources[hits[0]]


@pytest.mark.parametrize("kernel", sorted(GEMM))
def test_lens_gemm_scratch_lds_and_waves(resources, kernel):
    got = _one(resources, kernel, GEMM[kernel])
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["occupancy"] >= 2, f"{kernel}: a 512-thread workgroup needs 2 waves per SIMD: {got}"
    assert 0 < got["lds"] <= LDS_PER_CU, f"{kernel}: {got['lds']} bytes of LDS per workgroup: {got}"


@pytest.mark.parametrize("kernel", sorted(ROWS))
def test_lens_row_kernels_have_no_scratch(resources, kernel):
    assert _one(resources, kernel, ROWS[kernel])["scratch"] == 0


def test_only_the_listed_kernels_exist(resources):
    listed = list(GEMM.values()) + list(ROWS.values())
    assert len(resources) == len(listed) and all(any(f in m for f in listed) for m in resources), sorted(resources)
