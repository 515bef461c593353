#!/usr/bin/env python3
"""The dataset transform on the device (openpcseg_amd/transform.py, csrc/scantransform.hip) against what the package had before it.

On bench.py's raw batch (12 scans x 120 000 points, resident in HBM):
  batch      transform.device_batch(raw) with identity parameters  vs  workloads.synthetic.device_collate(raw) -- the same batch
             (checked: equal tensors) --, both ending in the same sparse_quantize_frames;
  front      the part that differs: pcs_scan_transform + pcs_scan_shift  vs  the torch elementwise front of device_collate
             (/, round, int, amin, -).
On ONE scan under the ten votes of test-time augmentation:
  tta_front  one pcs_scan_transform + pcs_scan_shift call for all ten votes  vs  ten sequential torch compositions of the same
             arithmetic (float64 affine map, float32 store, /, round, int, amin, -; checked: equal coordinates and features);
  tta_batch  transform.device_batch(votes=10), alone (nothing in the package built that batch on the device before).

Device events around blocks of calls, the variants of a pair alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. The bytes are ALGORITHMIC, from shapes: the scan read once (4 C B per row), per
vote 4 C + 12 B written by the transform, 12 B read and 12 + 8 B written by the shift. Writes profiles/transform_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import native  # noqa: E402
from openpcseg_amd import transform as T  # noqa: E402
from openpcseg_amd.workloads import synthetic  # noqa: E402


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


def front_bytes(n, c, votes):
    return n * 4 * c + votes * n * (4 * c + 12) + votes * n * (12 + 12 + 8)


def torch_front(raw, voxel_size):
    """The elementwise front of synthetic.device_collate, as it stands there."""
    pts, nf, off = raw["points"], raw["num_frames"], raw["offsets"]
    v = torch.full((), voxel_size, dtype=torch.float32, device=pts.device)
    pc = torch.round(pts[:, :3] / v).int()
    sizes = {off[i + 1] - off[i] for i in range(nf)}
    if len(sizes) == 1:
        n = sizes.pop()
        return (pc.view(nf, n, 3) - pc.view(nf, n, 3).amin(1, keepdim=True)).view(-1, 3)
    return torch.cat([pc[off[i]:off[i + 1]] - pc[off[i]:off[i + 1]].amin(0, keepdim=True) for i in range(nf)])


def torch_vote(pts, row, voxel):
    """One vote of one scan in torch: the arithmetic of transform.transform_scan_host, one elementwise launch per operation."""
    c, s, scale, sx, sy, jx, jy, jz = (float(x) for x in row)
    x, y, z = pts[:, 0].double(), pts[:, 1].double(), pts[:, 2].double()
    X = (x * c + y * (-s)) * scale * sx + jx
    Y = (x * s + y * c) * scale * sy + jy
    Z = z * scale + jz
    feats = torch.cat([torch.stack([X, Y, Z], 1).float(), pts[:, 3:]], 1)
    # a TENSOR divisor, as in device_collate: `tensor / python_float` is a multiplication by the reciprocal on the device
    pc = torch.round(feats[:, :3] / torch.full((), voxel, dtype=torch.float32, device=pts.device)).int()
    return feats, pc - pc.amin(0, keepdim=True)


def kernel_front(be, pts, off, params, votes, voxel_size):
    feats, coords, mins, off_dev = be.scan_transform(pts, off, params, votes, voxel_size)
    scenes = be.scan_shift(coords, mins, off_dev, votes)
    return feats, coords, scenes


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
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=20, help="calls per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transform_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    be = native.backend()
    host = synthetic.make_raw_batch(list(range(args.scans)), n_points=args.points)
    raw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in host.items()}
    n, c = raw["points"].shape
    ident = T.identity_params(args.scans)
    rows = []

    a, b = T.device_batch(raw, args.voxel), synthetic.device_collate(raw, args.voxel)
    same = all(torch.equal(a[k].F, b[k].F) and torch.equal(a[k].C, b[k].C) for k in ("lidar", "targets"))
    med, spread = alternate({"device_batch": lambda: T.device_batch(raw, args.voxel),
                             "device_collate": lambda: synthetic.device_collate(raw, args.voxel)}, args.reps, args.rounds, args.warmup)
    rows.append(record("batch", med, spread, "device_batch", "device_collate",
                       {"points": n, "voxels": int(a["lidar"].C.shape[0]), "equal_tensors": same}))

    same = bool(torch.equal(kernel_front(be, raw["points"], raw["offsets"], ident, 1, args.voxel)[1], torch_front(raw, args.voxel)))
    med, spread = alternate({"kernels": lambda: kernel_front(be, raw["points"], raw["offsets"], ident, 1, args.voxel),
                             "torch": lambda: torch_front(raw, args.voxel)}, args.reps, args.rounds, args.warmup)
    nbytes = front_bytes(n, c, 1)
    rows.append(record("front", med, spread, "kernels", "torch",
                       {"points": n, "algorithmic_bytes": nbytes, "kernels_gbps": round(nbytes / med["kernels"] / 1e6, 1), "equal_coords": same}))

    one = {"points": raw["points"][:raw["offsets"][1]].contiguous(), "labels": raw["labels"][:raw["offsets"][1]].contiguous(),
           "num_frames": 1, "offsets": [0, raw["offsets"][1]]}
    n1 = one["offsets"][1]
    params = T.tta_params(1, 10, rng=np.random.RandomState(0))

    def ten_torch():
        return [torch_vote(one["points"], params[v], args.voxel) for v in range(10)]

    kf, kc, _ = kernel_front(be, one["points"], one["offsets"], params, 10, args.voxel)
    tt = ten_torch()
    same = bool(torch.equal(kf, torch.cat([f for f, _ in tt])) and torch.equal(kc, torch.cat([p for _, p in tt])))
    med, spread = alternate({"kernels": lambda: kernel_front(be, one["points"], one["offsets"], params, 10, args.voxel),
                             "ten_torch": ten_torch}, args.reps, args.rounds, args.warmup)
    nbytes = front_bytes(n1, c, 10)
    rows.append(record("tta_front", med, spread, "kernels", "ten_torch",
                       {"points": n1, "votes": 10, "algorithmic_bytes": nbytes, "kernels_gbps": round(nbytes / med["kernels"] / 1e6, 1),
                        "equal_feats_and_coords": same}))

    med, spread = alternate({"device_batch": lambda: T.device_batch(one, args.voxel, params, votes=10, eval_maps=True)},
                            args.reps, args.rounds, args.warmup)
    rows.append(record("tta_batch", med, spread, "device_batch", None, {"points": n1, "votes": 10}))

    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points_per_scan": n // args.scans, "columns": c,
           "voxel_size": args.voxel, "reps_per_block": args.reps, "rounds": args.rounds,
           "method": "device events, alternating blocks, median block per variant", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
