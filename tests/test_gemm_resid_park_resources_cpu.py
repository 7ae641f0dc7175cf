"""What the compiler makes of the residual park (csrc/gemm_tiled.hpp, ResidParkSrc): the two instances that carry it,
gemm_kernel_v7<bf16, 5, RESID, 0, 2> and <bf16, 4, RESID, 0, 2>, held to the budget their design states.

The GEMM sources (gemm.hip, which includes gemm_v4.hpp and gemm_tiled.hpp, and gemm_generic.hip: all the kernels the one gemm.hip held) are compiled twice
with build.py's flags and ``-Rpass-analysis=kernel-resource-usage``, as tests/test_kernel_resources_cpu.py
does: as built, and with ``-DPV_GEMM_RESID_PARK=0``, which is the form before the park (tools/isa_vs_parent.py finds that build's
kernels instruction for instruction those of the commit before: profiles/r18_resid_park_isa_vs_parent.txt).  The second build is where
"the parent's figure" below is read from; at the time of writing it is 247 VGPRs (MB = 5) and 216 (MB = 4), the park's 240 and 205.

    no scratch                 the loop body runs at the register limit: a spill would sit among its MFMAs
    LDS <= 160 KB              two 72 KB ring slots + 2 KB of transposition per wave is exactly a CU's LDS at MB = 5
    2 waves per SIMD           one 512-thread workgroup per CU
    VGPRs <= the parent's      the park may cost no register (it frees the sixteen the rows of blocks 1 .. were loaded into)

and every OTHER kernel of the GEMM sources must report the same resources in both builds: the switch touches nothing else.

Not ``gpu``-marked; skipped where no hipcc is found.  Two compilations of each source, all in parallel, about a minute.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import re
import subprocess

import pytest

from vit_prisma_amd import build as pv_build

# mangled: t = unsigned short = bf16 storage, Li5E = 5, <T, MB, EPI = 2 (RESID), ACT = 0, LP = 2>
PARKED = {
    "gemm_kernel_v7<bf16, 5, RESID, 0, 2>": "14gemm_kernel_v7ItLi5ELi2ELi0ELi2EEEv",
    "gemm_kernel_v7<bf16, 4, RESID, 0, 2>": "14gemm_kernel_v7ItLi4ELi2ELi0ELi2EEEv",
}
_FIELDS = {
    "TotalSGPRs": "sgprs",
    "VGPRs": "vgprs",
    "AGPRs": "agprs",
    "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy",
    "LDS Size [bytes/block]": "lds",
}


# every GEMM source
SOURCES = tuple(s for s in pv_build.sources() if s.startswith("gemm"))


def _report(hipcc, outdir, tag, extra, src):
    cmd = [hipcc, *pv_build.FLAGS, *extra, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(pv_build.CSRC, src),
           "-o", os.path.join(outdir, f"{src[:-4]}_{tag}.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"hipcc failed ({src}, {tag}):\n{r.stderr[-4000:]}"
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in _FIELDS:
            cur[_FIELDS[m.group(1)]] = int(m.group(2))
    return out


def _reports(ex, hipcc, outdir, tag, extra):
    return [ex.submit(_report, hipcc, outdir, tag, extra, src) for src in SOURCES]


def _merged(futures, tag):
    out = {}
    for f in futures:
        part = f.result()
        assert not set(part) & set(out), f"a kernel in two sources ({tag}): {sorted(set(part) & set(out))}"
        out.update(part)
    assert out, f"hipcc printed no kernel-resource-usage remarks ({tag})"
    return out


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    try:
        hipcc = pv_build._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc: the resource report needs the ROCm compiler")
    outdir = str(tmp_path_factory.mktemp("resid_park_resources"))
    assert "gemm.hip" in SOURCES and "gemm_generic.hip" in SOURCES, SOURCES
    with cf.ThreadPoolExecutor(max_workers=2 * len(SOURCES)) as ex:
        park = _reports(ex, hipcc, outdir, "park", [])
        parent = _reports(ex, hipcc, outdir, "parent", ["-DPV_GEMM_RESID_PARK=0"])
        return _merged(park, "park"), _merged(parent, "parent")


def _one(table, fragment):
    hits = [k for k in table if fragment in k]
    assert len(hits) == 1, (fragment, hits)
    return table[hits[0]]


@pytest.mark.parametrize("kernel", sorted(PARKED))
def test_parked_instances_keep_their_budget(builds, kernel):
    park, parent = builds
    got, was = _one(park, PARKED[kernel]), _one(parent, PARKED[kernel])
    print(f"{kernel}: park {got}; parent's form {was}")
    assert got["scratch"] == 0, f"{kernel} spills to scratch: {got}"
    assert got["lds"] <= 160 * 1024, f"{kernel}: {got['lds']} bytes of LDS do not fit a CU: {got}"
    assert got["occupancy"] == 2, f"{kernel}: {got['occupancy']} waves per SIMD, the design states 2: {got}"
    assert got["vgprs"] <= was["vgprs"], f"{kernel}: {got['vgprs']} VGPRs, the form before the park has {was['vgprs']}"
    # the parked rows really are in LDS: the ring's two slots and the eight 2 KB transposition buffers
    mb = 5 if "5, RESID" in kernel else 4
    assert got["lds"] == 2 * (64 * mb + 256) * 128 + 8 * 2048, got
    assert was["lds"] == 2 * (64 * mb + 256) * 128, was


def test_the_switch_touches_no_other_kernel(builds):
    park, parent = builds
    assert sorted(park) == sorted(parent)
    others = [k for k in park if not any(f in k for f in PARKED.values())]
    assert len(others) == len(park) - 2 and len(others) == 59, len(others)      # (the kernels of all GEMM sources: 61)
    differ = {k: (parent[k], park[k]) for k in others if parent[k] != park[k]}
    assert not differ, differ
