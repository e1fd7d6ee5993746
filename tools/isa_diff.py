"""Compare two gfx950 assembly files of kernels.hip kernel by kernel: which kernels' instructions differ, and every kernel's
registers, scratch, spills, LDS and occupancy side by side.

The files come from the Makefile's compile line for kernels.hip with `--cuda-device-only -S` in place of `-c`:
    hipcc $(CXXFLAGS) $(HIPFLAGS) --cuda-device-only -S csrc/kernels.hip -o head.s
Usage: python tools/isa_diff.py parent.s head.s [--show NAME]     (--show: a unified diff of the kernels whose name contains NAME)
Exit status 1 when a kernel gained scratch or a spill, lost occupancy or changed its LDS size; else 0."""
import difflib, re, subprocess, sys

INFO = {"NumVgprs": "vgpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "LDSByteSize": "lds", "Occupancy": "occ"}
META = {".sgpr_spill_count": "sspill", ".vgpr_spill_count": "vspill"}
COLS = ("vgpr", "sgpr", "scratch", "sspill", "vspill", "lds", "occ")


def parse(path):
    """{mangled name: (instruction lines with the basic-block labels renumbered, {column: value})}"""
    kernels, name, body, res, in_info = {}, None, None, None, False
    spills, meta_name, meta = {}, None, {}
    for line in open(path, errors="replace"):
        line = line.rstrip("\n")
        m = re.match(r"\t\.type\t(\S+),@function", line)
        if m:
            name, body, res, in_info = m.group(1), [], {}, False
            continue
        if name is not None and body is not None and not in_info:
            if line.startswith(".Lfunc_end"):
                kernels[name] = [body, res]
                body = None
            elif re.match(r"\.LBB\d+_\d+:", line):
                body.append(line.split(":")[0] + ":")
            elif re.match(r"\t[a-z]", line):
                body.append(line.split(";")[0].strip())
            continue
        if line == "; Kernel info:":
            in_info = True
            continue
        if in_info:
            m = re.match(r"; (\w+)\s*: (\d+)", line)
            if m and m.group(1) in INFO:
                kernels[name][1][INFO[m.group(1)]] = int(m.group(2))
            if not line.startswith(";"):
                in_info, name = False, None
            continue
        m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)", line)   # the metadata note: one mapping per kernel
        if m:
            if line.lstrip().startswith("- ") and meta_name:
                spills[meta_name], meta_name, meta = meta, None, {}
            if m.group(1) == ".name" and m.group(2) in kernels:
                meta_name = m.group(2)
            elif m.group(1) in META:
                meta[META[m.group(1)]] = int(m.group(2))
    if meta_name:
        spills[meta_name] = meta
    out = {}
    for k, (body, res) in kernels.items():
        if "occ" not in res:
            continue   # a device function, not a kernel
        res.update(spills.get(k, {}))
        labels = {}
        for t in re.findall(r"\.LBB\d+_\d+", "\n".join(body)):
            labels.setdefault(t, "L%d" % len(labels))
        out[k] = ([re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], ln) for ln in body], res)
    return out


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (re.sub(r"\(.*", "", re.sub(r"^void ", "", o)) for o in out)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    args = sys.argv[1:]
    show = args[args.index("--show") + 1] if "--show" in args else None
    a, b = parse(args[0]), parse(args[1])
    short = demangle(sorted(set(a) | set(b)))
    only = sorted(set(a) ^ set(b))
    both = sorted(set(a) & set(b), key=lambda k: short[k])
    differ = [k for k in both if a[k][0] != b[k][0]]
    print("kernels: %d in %s, %d in %s, %d in both, %d instruction-identical, %d differ" % (len(a), args[0], len(b), args[1], len(both), len(both) - len(differ), len(differ)))
    for k in only:
        print("only in %s: %s" % (args[0] if k in a else args[1], short[k]))
    print("\nkernels whose instruction text differs (instructions parent -> head, lines changed):")
    for k in differ:
        sm = difflib.SequenceMatcher(None, a[k][0], b[k][0], autojunk=False)
        changed = sum(max(i2 - i1, j2 - j1) for op, i1, i2, j1, j2 in sm.get_opcodes() if op != "equal")
        print("  %-64s %5d -> %5d  %5d" % (short[k], len(a[k][0]), len(b[k][0]), changed))
    bad = []
    print("\n%-64s %s   (parent/head; * = differs)" % ("kernel", " ".join("%11s" % c for c in COLS)))
    for k in both:
        ra, rb = a[k][1], b[k][1]
        cells = ["%11s" % ("%s/%s%s" % (ra.get(c, "?"), rb.get(c, "?"), "*" if ra.get(c) != rb.get(c) else "")) for c in COLS]
        print("%-64s %s" % (short[k], " ".join(cells)))
        worse = [c for c in ("scratch", "sspill", "vspill") if rb.get(c, 0) > ra.get(c, 0)]
        if rb.get("occ", 0) < ra.get("occ", 0):
            worse.append("occ")
        if rb.get("lds") != ra.get("lds"):
            worse.append("lds")
        if worse:
            bad.append((short[k], worse))
    print()
    for k, worse in bad:
        print("WORSE: %s: %s" % (k, ", ".join(worse)))
    print("conditions (no scratch or spill gained, no occupancy lost, no LDS size changed): %s" % ("FAIL" if bad else "hold"))
    if show:
        for k in differ:
            if show in short[k]:
                print("\n".join(difflib.unified_diff(a[k][0], b[k][0], "parent " + short[k], "head " + short[k], lineterm="", n=2)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
