"""Do two trees compile to the same kernels?  (build container, no GPU)

    python tools/isa_vs_parent.py PARENT_DIR NEW_DIR [--gone=SUBSTR,...] [--renamed=OLD:NEW ...] > report.txt

Each directory holds, per HIP source, NAME.s and NAME.remarks: hipcc with build.py's FLAGS plus
`-S --cuda-device-only -Rpass-analysis=kernel-resource-usage` (stdout -> NAME.s with -o, stderr -> NAME.remarks).  Kernels are matched by
mangled name across all files of a directory.  Compared: the instruction stream -- comments, directives and .loc lines dropped, the
function ordinal n of .LBB<n>_<m> labels dropped (it shifts when a kernel changes files) -- and the resource remarks (SGPRs, VGPRs,
AGPRs, scratch, occupancy, LDS).  --renamed=OLD:NEW pairs a parent kernel that is missing with the one whose mangled name has the
substring OLD replaced by NEW (a parameter struct that left a namespace) and compares the two like the rest.  Exit status 1 if a kernel
differs, is new, or is missing without being named in --gone."""
import glob, os, re, subprocess, sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def load(d):
    kernels = {}
    for rem in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        src = os.path.basename(rem)[:-len(".remarks")] + ".hip"
        cur = None
        for line in open(rem):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                assert cur not in kernels, f"{cur} twice in {d}"
                kernels[cur] = {"src": src, "res": {}}
                continue
            m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
            if m and cur and m.group(1) in FIELDS:
                kernels[cur]["res"][m.group(1)] = m.group(2)
        lines = open(rem[:-len(".remarks")] + ".s").read().split("\n")
        i = 0
        while i < len(lines):
            m = re.match(r"(\w+):", lines[i])            # "name: ; @name"
            name = m.group(1) if m else None
            if name in kernels and kernels[name]["src"] == src and "insns" not in kernels[name]:
                body = []
                i += 1
                while not lines[i].startswith(".Lfunc_end"):
                    t = lines[i].split(";")[0].strip()
                    if t and (not t.startswith(".") or t.startswith(".LBB")):
                        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
                    i += 1
                kernels[name]["insns"] = body
            i += 1
    return kernels


def demangle(names):
    try:
        out = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, (o.replace("(anonymous namespace)::", "") for o in out)))
    except Exception:
        return {n: n for n in names}


def main():
    gone = set()
    renames = []
    args = [a for a in sys.argv[1:] if not a.startswith(("--gone=", "--renamed="))]
    for a in sys.argv[1:]:
        if a.startswith("--gone="):
            gone |= set(a[len("--gone="):].split(","))
        if a.startswith("--renamed="):
            renames.append(tuple(a[len("--renamed="):].split(":", 1)))
    old, new = load(args[0]), load(args[1])
    pretty = demangle(sorted(set(old) | set(new)))
    bad = 0
    moved = 0
    renamed = {}                                   # new mangled name -> the parent's
    for name in sorted(old, key=lambda n: (old[n]["src"], pretty[n])):
        o = old[name]
        now = name
        if name not in new:
            # a parameter type that changed namespace changes the mangled name: pair the kernel through the substring given
            for a, b in renames:
                if a in name and name.replace(a, b) in new:
                    now = name.replace(a, b)
                    renamed[now] = name
        if now not in new:
            ok = any(g in name for g in gone)
            bad += not ok
            print(f"{'gone   ' if ok else 'MISSING'} {o['src']:14s} {pretty[name]}")
            continue
        n = new[now]
        same = o["insns"] == n["insns"] and o["res"] == n["res"]
        bad += not same
        moved += o["src"] != n["src"]
        r = n["res"]
        where = o["src"] if o["src"] == n["src"] else f"{o['src']} -> {n['src']}"
        tag = ("renamed" if now != name else "same   ") if same else "DIFFERS"
        print(f"{tag} {where:26s} {pretty[name]}  insns {len(o['insns'])} sgpr {r[FIELDS[0]]} vgpr {r[FIELDS[1]]} "
              f"agpr {r[FIELDS[2]]} scratch {r[FIELDS[3]]} occ {r[FIELDS[4]]} lds {r[FIELDS[5]]}")
        if now != name:
            print(f"        {name} -> {now}")
        if not same:
            for f in FIELDS:
                if o["res"].get(f) != r.get(f):
                    print(f"        {f}: {o['res'].get(f)} -> {r.get(f)}")
            if o["insns"] != n["insns"]:
                print(f"        instructions: {len(o['insns'])} -> {len(n['insns'])}")
    for name in sorted(set(new) - set(old) - set(renamed)):
        bad += 1
        print(f"NEW     {new[name]['src']:14s} {pretty[name]}")
    print(f"\n{len(old)} kernels in the parent, {len(new)} now; {moved} changed files; {len(renamed)} renamed; {bad} not as required")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
