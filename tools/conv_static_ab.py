"""Static A/B of kernels: device assembly of two trees, per kernel instance.

  python tools/conv_static_ab.py <dir_a> <dir_b> [--md out.md] [--files a.hip,b.hip,...] [--rename 'regex=replacement' ...] [--unmatched N]

<dir_*> hold <file>.s / .log for each file (default: conv_wave{4,5,5h,5x,6h}.hip), compiled with its flags of
openpcseg_amd/build.py plus `--offload-device-only -S -Rpass-analysis=kernel-resource-usage` (stderr in the .log). For every
kernel symbol: LDS, VGPRs, spills, scratch, occupancy (waves per SIMD), MFMA and total instruction counts. Exit status 1 when B
has another symbol set or LDS size, more spills / scratch, another occupancy or another MFMA count than A.

With --rename the files are pooled and a kernel is known by its demangled name without the argument list, after the
substitutions (both sides): a kernel that moved to another file, or whose template arguments were renamed, meets its parent.
Kernels on one side only are then listed, counted in the verdict line, and fail the gate unless --unmatched N says how many
are expected (a refactor that merges kernels leaves some; a mistyped substitution must not shrink the compared set unseen).
"""
import os
import re
import shutil
import subprocess
import sys

FILES = ["conv_wave4.hip", "conv_wave5.hip", "conv_wave5h.hip", "conv_wave5x.hip", "conv_wave6h.hip"]
KEYS = ["group_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"]


def parse(d, f):
    text = open("%s/%s.s" % (d, f)).read()
    out = {}
    for rec in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:   # one metadata record per kernel
        name = re.search(r"\.symbol:\s+(\S+)\.kd", rec).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, rec).group(1)) for k in KEYS}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\.amdhsa_kernel \1$", text, re.S | re.M):
        body = [l.strip() for l in m.group(2).split("\n") if re.match(r"\t[a-z]\w+", l)]
        out[m.group(1)]["insts"] = len(body)
        out[m.group(1)]["mfma"] = sum(1 for l in body if l.startswith("v_mfma"))
    log = open("%s/%s.log" % (d, f)).read()
    for m in re.finditer(r"Function Name: (\S+).*?Occupancy \[waves/SIMD\]: (\d+)", log, re.S):
        if m.group(1) in out:
            out[m.group(1)]["occ"] = int(m.group(2))
    return out


def same_text(da, db, f):   # (__hip_cuid_*: a hash of the source path)
    strip = lambda p: [l for l in open(p) if not re.match(r'\s*\.(file|ident)\b', l) and "__hip_cuid_" not in l]
    return strip("%s/%s.s" % (da, f)) == strip("%s/%s.s" % (db, f))


def pooled(d, files, renames):
    """{readable kernel name: record} over all of `files` present in d"""
    out = {}
    for f in files:
        if os.path.exists("%s/%s.s" % (d, f)):
            out.update(parse(d, f))
    names = sorted(out)
    plain = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(names), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    res = {}
    for sym, name in zip(names, plain):
        name = re.sub(r"^void ", "", name.replace("(anonymous namespace)::", "")).split("(")[0]
        for r in renames:
            pat, rep = r.split("=", 1)
            name = re.sub(pat, rep, name)
        if name in res:   # two symbols under one name would drop an instance from the comparison unseen
            raise SystemExit("conv_static_ab: %s: two kernels are called `%s` after the --rename substitutions" % (d, name))
        res[name] = out[sym]
    return res


def main():
    da, db = sys.argv[1], sys.argv[2]
    md = open(sys.argv[sys.argv.index("--md") + 1], "w") if "--md" in sys.argv else None
    files = sys.argv[sys.argv.index("--files") + 1].split(",") if "--files" in sys.argv else FILES
    renames = [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == "--rename"]
    expected = int(sys.argv[sys.argv.index("--unmatched") + 1]) if "--unmatched" in sys.argv else 0
    bad = unmatched = 0
    cols = ["vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "occ",
            "mfma", "insts"]
    for f in ([", ".join(files)] if renames else files):
        if renames:
            a, b = pooled(da, files, renames), pooled(db, files, renames)
            head = "%s: %d kernels in A, %d in B, %d in both" % (f, len(a), len(b), len(set(a) & set(b)))
        elif not os.path.exists("%s/%s.s" % (db, f)):
            print("%s: not in %s, skipped" % (f, db))
            continue
        else:
            a, b = parse(da, f), parse(db, f)
            head = "%s: %d kernels%s" % (f, len(a), ", assembly identical" if same_text(da, db, f) else "")
        print(head)
        if md:
            md.write("\n### %s\n\n| kernel | VGPRs | VGPR spills | SGPR spills | scratch | LDS | waves/SIMD | MFMAs | instructions |\n"
                     "|---|---|---|---|---|---|---|---|---|\n" % head)
        if set(a) != set(b):
            print("  SYMBOL SET DIFFERS:" if not renames else "  on one side only:", sorted(set(a) ^ set(b)))
            unmatched += len(set(a) ^ set(b))
            bad += not renames
        for k in sorted(set(a) & set(b)):
            x, y = a[k], b[k]
            fail = (x["group_segment_fixed_size"] != y["group_segment_fixed_size"] or x["occ"] != y["occ"] or x["mfma"] != y["mfma"]
                    or any(y[c] > x[c] for c in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")))
            bad += fail
            if fail or any(x[c] != y[c] for c in cols if c != "insts"):
                print("  %s %s" % ("FAIL" if fail else "diff", k), " ".join("%s %d->%d" % (c, x[c], y[c]) for c in cols if x[c] != y[c]))
            if md:
                md.write("| `%s` | %s |\n" % (k, " | ".join(str(x[c]) if x[c] == y[c] else "%d -> %d" % (x[c], y[c]) for c in cols)))
    if renames and unmatched != expected:
        print("  %d kernels on one side only, %d expected (--unmatched)" % (unmatched, expected))
        bad += 1
    print("FAILED: %d" % bad if bad else "gate passed (%d kernels on one side only)" % unmatched)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
