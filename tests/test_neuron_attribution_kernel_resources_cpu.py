"""What the compiler makes of the neuron-attribution kernels (csrc/attribution_neuron.hip): the three instances of
nattr_dense_kernel<OC> (answers held in registers 1 / 4 / 16) and the top-k kernel.

The pattern of test_attribution_kernel_resources_cpu.py: the file is compiled with build.py's flags plus
``-Rpass-analysis=kernel-resource-usage``.  The dense kernel's point is that a lane keeps its 8 neurons' share of up to 16 answers
(128 floats) in registers while the tap streams past: no scratch, and no LDS at all.  The top-k kernel reads its L tap pointers by
a lane-dependent layer index; it keeps them in LDS so that the kernel arguments are not copied to scratch, beside the 256 maxima and
the candidate list: no scratch, LDS within 64 KiB.

Not ``gpu``-marked; skipped where no hipcc is found.
"""
from __future__ import annotations

import pytest

from test_kernel_resources_cpu import _find_hipcc, compile_report, parse_resource_report

DENSE = {f"nattr_dense_kernel<{oc}>": f"18nattr_dense_kernelILi{oc}EEEv" for oc in (1, 4, 16)}
TOPK = {"nattr_topk_kernel": "17nattr_topk_kernelE"}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    hipcc = _find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    parsed = parse_resource_report(compile_report(hipcc, "attribution_neuron.hip", str(tmp_path_factory.mktemp("kernel_resources_nattr"))))
    assert parsed, "attribution_neuron.hip: hipcc printed no kernel-resource-usage remarks"
    return parsed


def _one(resources, kernel, fragment):
    hits = [m for m in resources if fragment in m]
    assert len(hits) == 1, f"{kernel} ({fragment}) is not among the kernels attribution_neuron.hip compiles to: {sorted(resources)}"
    print(f"{kernel}: {resources[hits[0]]}")
    return resources[hits[0]]


@pytest.mark.parametrize("kernel", sorted(DENSE))
def test_dense_kernel_keeps_its_answers_in_registers(resources, kernel):
    got = _one(resources, kernel, DENSE[kernel])
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["lds"] == 0, f"{kernel} needs no LDS: {got}"
    assert got["occupancy"] >= 1, got


def test_topk_kernel_has_no_scratch(resources):
    got = _one(resources, "nattr_topk_kernel", TOPK["nattr_topk_kernel"])
    assert got["scratch"] == 0, got
    assert 0 < got["lds"] <= 64 * 1024, got


def test_only_the_listed_kernels_exist(resources):
    listed = list(DENSE.values()) + list(TOPK.values())
    assert len(resources) == len(listed) and all(any(f in m for f in listed) for m in resources), sorted(resources)
