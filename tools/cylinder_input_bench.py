#!/usr/bin/env python3
"""The cylinder dataset's batch on the device (openpcseg_amd/cylinder.py device_batch, csrc/cylscan.hip) against the per-frame path
the package had before it.

On bench.py's raw batch (12 scans x 120 000 points, resident in HBM) at the cy480 grid:
  train_batch   cylinder.device_batch(raw)  vs  12 x cylinder.cylinder_sample + workloads.cylinder.cylinder_batch -- the same
                batch (checked: equal tensors);
On ONE scan under the ten votes of test-time augmentation:
  tta_batch     cylinder.device_batch(votes=10)  vs  ten (torch composition of the affine map + cylinder_sample) + cylinder_batch
                (checked: equal tensors);
The kernel alone (pcs_cylinder_scan_batch_f32 through its binding), 1 vote of the batch, 10 votes of one scan, 10 votes of the batch:
  kernel_*      the three store forms: staged (features and cells through LDS, contiguous 16-byte stores), direct (every lane
                stores its own row), staged_feat (features staged, cells direct), with GB/s on the ALGORITHMIC bytes: the scan read
                once (4 C B per row), per vote 4 (8 + C - 3) + 12 + 8 B written.

Device events around blocks of calls, the variants of a case alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. Writes profiles/cylinder_batch_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import cylinder, native  # noqa: E402
from openpcseg_amd import transform as T  # noqa: E402
from openpcseg_amd.workloads import synthetic  # noqa: E402
from openpcseg_amd.workloads.cylinder import cylinder_batch  # noqa: E402

LO, HI, GRID = [0, -180, -4], [50, 180, 2], [480, 360, 32]   # R:tools/cfgs/voxel/semantic_kitti/cylinder_cy480_cr10.yaml
CLASSES = 20
FORMS = {"staged": 0, "direct": 1, "staged_feat": 2}
TENSORS = ("point_feature", "point_coord", "point_label", "voxel_coord", "voxel_label", "inverse_map")


def block_ms(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, reps, rounds, warm):
    """{name: run} -> {name: median ms per call}, {name: (min, max)}; one block of every variant per round, in turn."""
    for run in variants.values():
        for _ in range(warm):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, run in variants.items():
            times[k].append(block_ms(run, reps))
    return {k: statistics.median(v) for k, v in times.items()}, {k: (min(v), max(v)) for k, v in times.items()}


def kernel_bytes(n, c, votes):
    return n * 4 * c + votes * n * (4 * (8 + c - 3) + 12 + 8)


def per_frame_batch(raw):
    """The per-frame path: one cylinder_sample per frame, then the concatenation."""
    off = raw["offsets"]
    return cylinder_batch([cylinder.cylinder_sample(raw["points"][off[f]:off[f + 1]], raw["labels"][off[f]:off[f + 1]], LO, HI, GRID, CLASSES)
                           for f in range(raw["num_frames"])])


def torch_vote(pts, row):
    """One vote of one scan in torch: the arithmetic of transform.transform_scan_host, one elementwise launch per operation."""
    c, s, scale, sx, sy, jx, jy, jz = (float(x) for x in row)
    x, y, z = pts[:, 0].double(), pts[:, 1].double(), pts[:, 2].double()
    X = (x * c + y * (-s)) * scale * sx + jx
    Y = (x * s + y * c) * scale * sy + jy
    Z = z * scale + jz
    return torch.cat([torch.stack([X, Y, Z], 1).float(), pts[:, 3:]], 1)


def ten_votes_per_frame(one, params, votes):
    return cylinder_batch([cylinder.cylinder_sample(torch_vote(one["points"], params[v]), one["labels"], LO, HI, GRID, CLASSES)
                           for v in range(votes)])


def same_batch(a, b):
    return bool(all(torch.equal(a[k], b[k]) for k in TENSORS) and torch.equal(a["offset"].cpu(), b["offset"].cpu()))


def record(name, med, spread, new, old, extra):
    row = {"case": name, "ms": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()}}
    if old is not None:
        row["speedup"] = round(med[old] / med[new], 3)
        row["difference_beyond_spread"] = bool(spread[new][1] < spread[old][0] or spread[new][0] > spread[old][1])
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan, 120 000)")
    ap.add_argument("--reps", type=int, default=10, help="calls per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cylinder_batch_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cylinder_input_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    be = native.backend()
    store = be.lib.pcs_debug_cylscan_store
    host = synthetic.make_raw_batch(list(range(args.scans)), n_points=args.points, num_classes=CLASSES)
    raw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in host.items()}
    n, c = raw["points"].shape
    rows = []

    same = same_batch(cylinder.device_batch(raw, LO, HI, GRID, CLASSES), per_frame_batch(raw))
    med, spread = alternate({"device_batch": lambda: cylinder.device_batch(raw, LO, HI, GRID, CLASSES),
                             "per_frame": lambda: per_frame_batch(raw)}, args.reps, args.rounds, args.warmup)
    rows.append(record("train_batch", med, spread, "device_batch", "per_frame", {"points": n, "frames": args.scans, "equal_tensors": same}))

    n1 = raw["offsets"][1]
    one = {"points": raw["points"][:n1].contiguous(), "labels": raw["labels"][:n1].contiguous(), "num_frames": 1, "offsets": [0, n1]}
    params = T.tta_params(1, 10, scale_range=(0.95, 1.05), rng=np.random.RandomState(0))
    same = same_batch(cylinder.device_batch(one, LO, HI, GRID, CLASSES, params, votes=10), ten_votes_per_frame(one, params, 10))
    med, spread = alternate({"device_batch": lambda: cylinder.device_batch(one, LO, HI, GRID, CLASSES, params, votes=10),
                             "per_frame": lambda: ten_votes_per_frame(one, params, 10)}, args.reps, args.rounds, args.warmup)
    rows.append(record("tta_batch", med, spread, "device_batch", "per_frame", {"points": n1, "votes": 10, "equal_tensors": same}))

    big = T.tta_params(args.scans, 10, scale_range=(0.95, 1.05), rng=np.random.RandomState(1))
    kernel_cases = {"kernel_batch_1_vote": (raw["points"], raw["offsets"], T.identity_params(args.scans), 1),
                    "kernel_scan_10_votes": (one["points"], one["offsets"], params, 10),
                    "kernel_batch_10_votes": (raw["points"], raw["offsets"], big, 10)}
    try:
        for name, (pts, off, par, votes) in kernel_cases.items():
            def run_form(form):
                def run():
                    store(form)
                    return be.cylinder_scan_batch(pts, off, par, votes, LO, HI, GRID)
                return run
            outs = {k: run_form(f)() for k, f in FORMS.items()}
            same = bool(all(torch.equal(a, b) for k in ("direct", "staged_feat") for a, b in zip(outs["staged"], outs[k])))
            del outs
            med, spread = alternate({k: run_form(f) for k, f in FORMS.items()}, args.reps * 2, args.rounds, args.warmup)
            nbytes = kernel_bytes(pts.shape[0], c, votes)
            extra = {"points": int(pts.shape[0]), "votes": votes, "algorithmic_bytes": nbytes, "equal_outputs": same,
                     "gbps": {k: round(nbytes / v / 1e6, 1) for k, v in med.items()}}
            rows.append(record(name, med, spread, "staged", "direct", extra))
    finally:
        store(-1)

    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points_per_scan": n // args.scans, "columns": c,
           "grid": GRID, "reps_per_block": args.reps, "rounds": args.rounds,
           "method": "device events, alternating blocks, median block per variant", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
