#!/usr/bin/env python3
"""spvoxelize / spdevoxelize on the 12-scan bench batch at the shapes of SPVCNN's point <-> voxel hops: today's autocast path
(bf16 -> fp32 cast, the fp32 kernel, fp32 -> bf16 cast for the consumer) against the 16-bit instances of csrc/pointvoxel.hip,
the latter as shipped and, where the kernel has that choice (the lane-row segmented kernels), forced to 2 and to 4 row loads in
flight.

Device events around blocks of calls, the variants alternating block by block, the median block per variant. GB/s are on the
ALGORITHMIC bytes of the op with 16-bit features (every input and output row once, plus the index / weight arrays the kernel
reads), for both paths: the job is the same, bf16 in and bf16 out. Writes profiles/pointvoxel_half_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from openpcseg_amd import functional as F  # noqa: E402
from openpcseg_amd import native  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_batch  # noqa: E402

SHAPES = [(1, 32), (16, 256), (4, 128), (1, 96)]   # (stride, channels) of SPVCNN's hops


def block_us(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternate(variants, reps, rounds, warm):
    """{name: run} -> {name: median us per call}; one block of every variant per round, in turn."""
    for run in variants.values():
        for _ in range(warm):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, run in variants.items():
            times[k].append(block_us(run, reps))
    return {k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pointvoxel_half_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pointvoxel_bench: needs an MI355X (no CPU timing)")
    be = native.backend()
    inflight = be.lib.pcs_debug_pointvoxel_h_inflight
    dev, hd = "cuda", torch.bfloat16
    c1 = make_batch(list(range(args.scans)), n_points=args.points)["lidar"].C.to(dev)
    c1 = c1[torch.argsort(be.hash(c1))].contiguous()      # voxel order of initial_voxelize: ascending hash
    lv = {1: c1}
    for s in (1, 2, 4, 8):
        lv[2 * s] = be.downsample(lv[s], [2 * s] * 3)
    zc = c1.float()                                      # the points of the point branch are the input rows
    n = zc.shape[0]
    rec = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "scans": args.scans, "points": n, "reps": args.reps,
           "rounds": args.rounds, "bytes": "algorithmic, 16-bit feature rows once + index / weight arrays", "ops": []}
    slower = []
    for s, c in SHAPES:
        vox = lv[s]
        m = vox.shape[0]
        idx8, w8 = be.corner_map(zc, vox, s)
        cell = torch.cat([torch.floor(zc[:, :3] / s).int() * s, zc[:, -1].int().view(-1, 1)], 1)
        idx = (be.table_query(be.level_table(vox), F.sphash(cell)) - 1).int().contiguous()
        counts = F.spcount(idx, m)
        entries = int((idx8 >= 0).sum())
        pf, vf = torch.randn(n, c, device=dev).to(hd), torch.randn(m, c, device=dev).to(hd)
        rows = (n + m) * c * 2
        ops = {
            "voxelize_fwd": (lambda x: be.voxelize_fwd(x, idx, counts), pf, rows + n * 8 + (m + 1) * 8 + m * 4, True),
            "voxelize_bwd": (lambda x: be.voxelize_bwd(x, idx, counts, n), vf, rows + n * 4 + m * 4, False),
            "devoxelize_fwd": (lambda x: be.devoxelize_fwd(x, idx8, w8), vf, rows + n * 8 * 8, False),
            "devoxelize_bwd": (lambda x: be.devoxelize_bwd(x, idx8, w8, m), pf, rows + entries * 12 + (m + 1) * 8, True),
        }
        for name, (op, x, nbytes, has_inflight) in ops.items():
            variants = {"cast_fp32_cast": lambda op=op, x=x: op(x.float()).to(hd), "fp32_kernel_alone": lambda op=op, x=x.float(): op(x)}
            inflight(0)
            ref, got = variants["cast_fp32_cast"](), op(x)
            diff = float((ref.float() - got.float()).abs().max())
            if has_inflight:
                inflight(4)
                same = bool(torch.equal(got.view(torch.int16), op(x).view(torch.int16)))
                variants["half"] = lambda op=op, x=x: (inflight(0), op(x))[1]
                variants["half_2_loads"] = lambda op=op, x=x: (inflight(2), op(x))[1]
                variants["half_4_loads"] = lambda op=op, x=x: (inflight(4), op(x))[1]
            else:
                same = None
                variants["half"] = lambda op=op, x=x: op(x)
            med, spread = alternate(variants, args.reps, args.rounds, args.warmup)
            inflight(0)
            shipped = med["half"]
            row = {"op": name, "stride": s, "c": c, "points": n, "voxels": m, "algorithmic_bytes": nbytes,
                   "us": {k: round(v, 2) for k, v in med.items()}, "us_min_max": {k: [round(a, 2), round(b, 2)] for k, (a, b) in spread.items()},
                   "gbps": {k: round(nbytes / v / 1e3, 1) for k, v in med.items()},
                   "speedup_vs_cast_fp32_cast": round(med["cast_fp32_cast"] / shipped, 3),
                   "max_abs_diff_vs_fp32_path": diff, "inflight_4_bit_identical": same}
            if shipped > med["cast_fp32_cast"]:
                slower.append("%s stride %d c %d" % (name, s, c))
            rec["ops"].append(row)
            print(json.dumps(row), flush=True)
    rec["slower_than_cast_fp32_cast"] = slower
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s; slower than today's path: %s" % (args.out, slower or "none"))


if __name__ == "__main__":
    main()
