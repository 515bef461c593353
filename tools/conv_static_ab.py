"""Static A/B of the wave conv kernels: device assembly of two trees, per kernel instance.

  python tools/conv_static_ab.py <dir_a> <dir_b> [--md out.md]

<dir_*> hold conv_wave{4,5,5h,5x,6h}.hip.s / .log: each file compiled with its flags of openpcseg_amd/build.py plus
`--offload-device-only -S -Rpass-analysis=kernel-resource-usage` (stderr in the .log). For every kernel symbol: LDS, VGPRs,
spills, scratch, occupancy (waves per SIMD), MFMA and total instruction counts. Exit status 1 when B has another symbol set or
LDS size, more spills / scratch, another occupancy or another MFMA count than A.
"""
import os
import re
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


def same_text(da, db, f):
    strip = lambda p: [l for l in open(p) if not re.match(r'\s*\.(file|ident)\b', l)]
    return strip("%s/%s.s" % (da, f)) == strip("%s/%s.s" % (db, f))


def main():
    da, db = sys.argv[1], sys.argv[2]
    md = open(sys.argv[sys.argv.index("--md") + 1], "w") if "--md" in sys.argv else None
    bad = 0
    cols = ["vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "occ",
            "mfma", "insts"]
    for f in FILES:
        if not os.path.exists("%s/%s.s" % (db, f)):
            print("%s: not in %s, skipped" % (f, db))
            continue
        a, b = parse(da, f), parse(db, f)
        ident = same_text(da, db, f)
        head = "%s: %d kernels%s" % (f, len(a), ", assembly identical" if ident else "")
        print(head)
        if md:
            md.write("\n### %s\n\n| kernel | VGPRs | VGPR spills | SGPR spills | scratch | LDS | waves/SIMD | MFMAs | instructions |\n"
                     "|---|---|---|---|---|---|---|---|---|\n" % head)
        if set(a) != set(b):
            print("  SYMBOL SET DIFFERS:", sorted(set(a) ^ set(b)))
            bad += 1
        for k in sorted(set(a) & set(b)):
            x, y = a[k], b[k]
            fail = (x["group_segment_fixed_size"] != y["group_segment_fixed_size"] or x["occ"] != y["occ"] or x["mfma"] != y["mfma"]
                    or any(y[c] > x[c] for c in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")))
            bad += fail
            if fail or any(x[c] != y[c] for c in cols if c != "insts"):
                print("  %s %s" % ("FAIL" if fail else "diff", k), " ".join("%s %d->%d" % (c, x[c], y[c]) for c in cols if x[c] != y[c]))
            if md:
                md.write("| `%s` | %s |\n" % (k, " | ".join(str(x[c]) if x[c] == y[c] else "%d -> %d" % (x[c], y[c]) for c in cols)))
    print("FAILED: %d" % bad if bad else "gate passed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
