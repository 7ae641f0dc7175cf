"""Seams of the tapped B/32 forward out of a rocprofv3 kernel trace: what the time between two dependent kernels is, by predecessor.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python bench.py --steps 15 --warmup 5
    python tools/seam_gaps.py [--skip 5] LABEL=DIR/..._kernel_trace.csv [LABEL2=...csv ...] [--json OUT.json]

(--skip N leaves the first N forwards of every trace out: the warm-up steps, whose first forward is several hundred us longer.)

A forward is the run of launches from the patch-embedding GEMM (the GEMM right in front of ``ln_kernel<.., true>``) to
``l2norm_kernel``.  Every launch in it is put in a group by what it is -- patch, embed-LN, LN, QKV, attention, O-proj, MLP-1, MLP-2,
head, l2norm, other (copies, transposes) -- the GEMMs by their neighbours (before attention: QKV; after it: O-proj; after a
LayerNorm and before a GEMM: MLP-1; after a GEMM: MLP-2), so the table does not depend on which GEMM kernel a shape selects.
Per group, over all forwards of the trace: the gap ``start[i+1] - end[i]`` behind the kernel, its duration, and duration + gap
(the quantity a store policy has to be judged by: writing through moves the write-back out of the gap into the body); per
forward: the sums, with their forward-to-forward spread.  With several traces, a comparison of every later one with the first.
"""
from __future__ import annotations

import csv
import json
import statistics as st
import sys

GEMM_GROUPS = ("patch", "QKV", "O-proj", "MLP-1", "MLP-2", "head")
ORDER = ("patch", "embed-LN", "LN", "QKV", "attention", "O-proj", "MLP-1", "MLP-2", "head", "l2norm", "other")


def kind(name: str) -> str:
    if "ln_kernel<" in name:
        return "embed-LN" if name.split("ln_kernel<")[1].split(">")[0].replace(" ", "").endswith(",true") else "LN"
    if "gemm_kernel" in name:
        return "gemm"
    if "attn_" in name:
        return "attention"
    if "l2norm_kernel" in name:
        return "l2norm"
    return "other"


def read_trace(path: str):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def forwards(rows):
    """[[(start, end, group)]]: one list per complete forward."""
    kinds = [kind(n) for _, _, n in rows]
    out, i, n = [], 0, len(rows)
    while i < n:
        if kinds[i] != "embed-LN":
            i += 1
            continue
        first = i
        j = i - 1
        while j >= 0 and kinds[j] == "other":
            j -= 1
        if j >= 0 and kinds[j] == "gemm":
            first = j
        last = i + 1
        while last < n and kinds[last] not in ("l2norm", "embed-LN"):
            last += 1
        if last >= n or kinds[last] != "l2norm":
            i += 1
            continue
        idx = list(range(first, last + 1))
        core = [k for k in idx if kinds[k] != "other"]
        group = {}
        for c, k in enumerate(core):
            g = kinds[k]
            if g == "gemm":
                prev = kinds[core[c - 1]] if c > 0 else None
                nxt = kinds[core[c + 1]] if c + 1 < len(core) else None
                if nxt == "embed-LN":
                    g = "patch"
                elif nxt == "attention":
                    g = "QKV"
                elif prev == "attention":
                    g = "O-proj"
                elif nxt in ("l2norm", None):
                    g = "head"
                elif prev == "gemm":
                    g = "MLP-2"
                else:
                    g = "MLP-1"
            group[k] = g
        out.append([(rows[k][0], rows[k][1], group.get(k, "other")) for k in idx])
        i = last + 1
    return out


def _stats(xs):
    xs = sorted(xs)
    return {"n": len(xs), "min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "mean": st.fmean(xs),
            "std": st.pstdev(xs) if len(xs) > 1 else 0.0}


def analyse(rows, skip=0):
    fw = forwards(rows)[skip:]
    if not fw:
        raise SystemExit("no complete forward (patch GEMM ... l2norm_kernel) in the trace")
    per_group = {}          # group -> {"gap": [...], "dur": [...], "both": [...]}   (us, every launch that has a successor)
    sums = []               # per forward: {group: sum of dur + gap, ...}
    for f in fw:
        s = {"_gaps": 0.0, "_kernels": 0.0, "_span": (f[-1][1] - f[0][0]) / 1e3, "_launches": len(f)}
        for i, (t0, t1, g) in enumerate(f):
            dur = (t1 - t0) / 1e3
            s["_kernels"] += dur
            if i + 1 == len(f):
                continue
            gap = (f[i + 1][0] - t1) / 1e3
            d = per_group.setdefault(g, {"gap": [], "dur": [], "both": []})
            d["gap"].append(gap)
            d["dur"].append(dur)
            d["both"].append(dur + gap)
            s[g] = s.get(g, 0.0) + dur + gap
            s["_gaps"] += gap
        s["_gemm"] = sum(s.get(g, 0.0) for g in GEMM_GROUPS)
        sums.append(s)
    res = {"forwards": len(fw), "launches_per_forward": _stats([s["_launches"] for s in sums]),
           "groups": {g: {"per_forward": len(d["gap"]) / len(fw), "gap_us": _stats(d["gap"]), "dur_us": _stats(d["dur"]),
                          "dur_plus_gap_us": _stats(d["both"])} for g, d in per_group.items()},
           "per_forward_us": {"gaps": _stats([s["_gaps"] for s in sums]), "kernels": _stats([s["_kernels"] for s in sums]),
                              "span": _stats([s["_span"] for s in sums]), "gemm_dur_plus_gap": _stats([s["_gemm"] for s in sums]),
                              **{g: _stats([s.get(g, 0.0) for s in sums]) for g in per_group}}}
    return res


def show(label, res):
    print(f"## {label}: {res['forwards']} forwards, {res['launches_per_forward']['median']} launches each")
    print(f"{'predecessor':<10} {'n/fwd':>5} | {'gap us: min':>11} {'median':>7} {'max':>7} | {'dur us: mean':>12} {'min':>7} | "
          f"{'dur+gap us: min':>15} {'median':>7} {'max':>7} {'mean':>7} {'std':>6}")
    for g in ORDER:
        if g not in res["groups"]:
            continue
        d = res["groups"][g]
        a, b, c = d["gap_us"], d["dur_us"], d["dur_plus_gap_us"]
        print(f"{g:<10} {d['per_forward']:>5.1f} | {a['min']:>11.2f} {a['median']:>7.2f} {a['max']:>7.2f} | {b['mean']:>12.2f} {b['min']:>7.2f} | "
              f"{c['min']:>15.2f} {c['median']:>7.2f} {c['max']:>7.2f} {c['mean']:>7.2f} {c['std']:>6.2f}")
    p = res["per_forward_us"]
    for key, title in (("gaps", "sum of gaps"), ("kernels", "sum of kernel durations"), ("span", "first start .. last end"),
                       ("gemm_dur_plus_gap", "GEMM launches, dur + gap")):
        x = p[key]
        print(f"per forward, {title:<26} mean {x['mean']:>8.1f}  min {x['min']:>8.1f}  max {x['max']:>8.1f}  std {x['std']:>6.1f} us")
    print()


def compare(base_label, base, label, res):
    print(f"## {label} against {base_label}: mean duration + following gap per launch (us); 'worse' = above the base by more than the base's own std")
    for g in ORDER:
        if g in base["groups"] and g in res["groups"]:
            a, b = base["groups"][g]["dur_plus_gap_us"], res["groups"][g]["dur_plus_gap_us"]
            flag = "worse" if b["mean"] - a["mean"] > a["std"] else ""
            print(f"{g:<10} {a['mean']:>8.2f} -> {b['mean']:>8.2f}  ({b['mean'] - a['mean']:>+7.2f}; base std {a['std']:.2f}) {flag}")
    a, b = base["per_forward_us"]["gemm_dur_plus_gap"], res["per_forward_us"]["gemm_dur_plus_gap"]
    spread = a["max"] - a["min"]
    print(f"GEMM launches of a forward, dur + gap: {a['mean']:.1f} -> {b['mean']:.1f} us ({b['mean'] - a['mean']:+.1f}); the base's forward-to-forward "
          f"spread (max - min) is {spread:.1f}: {'lower by more than it' if a['mean'] - b['mean'] > spread else 'NOT lower by more than it'}")
    a, b = base["per_forward_us"]["span"], res["per_forward_us"]["span"]
    print(f"forward span: {a['mean']:.1f} -> {b['mean']:.1f} us ({b['mean'] - a['mean']:+.1f})\n")


def main(argv):
    out_json, items, skip = None, [], 0
    it = iter(argv)
    for a in it:
        if a == "--json":
            out_json = next(it)
        elif a == "--skip":
            skip = int(next(it))
        else:
            label, _, path = a.partition("=")
            items.append((label, path) if path else (a, a))
    if not items:
        raise SystemExit(__doc__)
    results = [(label, analyse(read_trace(path), skip)) for label, path in items]
    for label, res in results:
        show(label, res)
    for label, res in results[1:]:
        compare(results[0][0], results[0][1], label, res)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({label: res for label, res in results}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
