"""What the compiler makes of the head-attribution kernels (csrc/attribution.hip): the fold kernel and the nine instances of
attr_head_kernel<LPH, OC> (lanes per head 4 / 8 / 16 x answers held in registers 1 / 4 / 16).

The pattern of test_lens_kernel_resources_cpu.py: attribution.hip is compiled with build.py's flags plus
``-Rpass-analysis=kernel-resource-usage``.  Neither kernel may spill: the head kernel's point is that a lane keeps its head's share
of up to 16 answers (128 floats) in registers while the tap streams past, and a spill would put that share in memory.

Not ``gpu``-marked; skipped where no hipcc is found.
"""
from __future__ import annotations

import pytest

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

HEAD = {f"attr_head_kernel<{lph}, {oc}>": f"16attr_head_kernelILi{lph}ELi{oc}EEEv" for lph in (4, 8, 16) for oc in (1, 4, 16)}
FOLD = {"attr_fold_kernel": "16attr_fold_kernelE"}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    parsed = parse_resource_report(compile_report(hipcc, "attribution.hip", str(tmp_path_factory.mktemp("kernel_resources_attr"))))
    assert parsed, "attribution.hip: hipcc printed no kernel-resource-usage remarks"
    return parsed


def _one(resources, kernel, fragment):
    hits = [m for m in resources if fragment in m]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels attribution.hip compiles to: {sorted(resources)}"
    print(f"{kernel}: {resources[hits[0]]}")
    return resources[hits[0]]


@pytest.mark.parametrize("kernel", sorted(HEAD))
def test_head_kernel_keeps_its_answers_in_registers(resources, kernel):
    got = _one(resources, kernel, HEAD[kernel])
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["lds"] == 0, f"{kernel} needs no LDS: {got}"
    assert got["occupancy"] >= 1, got


def test_fold_kernel_has_no_scratch(resources):
    got = _one(resources, "attr_fold_kernel", FOLD["attr_fold_kernel"])
    assert got["scratch"] == 0, got
    assert 0 < got["lds"] <= 64 * 1024, got


def test_only_the_listed_kernels_exist(resources):
    listed = list(HEAD.values()) + list(FOLD.values())
    assert len(resources) == len(listed) and all(any(f in m for f in listed) for m in resources), sorted(resources)
