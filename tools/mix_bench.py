#!/usr/bin/env python3
"""PolarMix of raw batches on the device (openpcseg_amd/scanmix.py device_mix, csrc/scanmix.hip) against the same result composed
from torch operations in this process.

On the bench's twelve 120 000-point scans (workloads.synthetic.make_raw_batch) and their partners (make_partner_raw_batch), both
resident in HBM, PolarMix on every frame (alpha and the swap drawn per frame, the paste always on), with and without the ring column:
  mix, mix_ring    scanmix.device_mix  vs  torch_mix: per frame the float32 sector test on a double arctan2 rounded once, boolean
                   masks, the instance rows class by class, the two rotations in float64, `cat`, and the ring as a flag + `cumsum`.
                   The two must give EQUAL tensors (asserted before anything is timed).
The synthetic labels are uniform over 20 classes, so 40 % of a partner scan are instance rows and a mixed frame is about 2.2 times
its scan: far more pasted rows than a SemanticKITTI frame carries.

Device events around blocks of calls, the variants of a case alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. Writes profiles/mix_bench.json (--out)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import scanmix  # noqa: E402
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


def torch_mix(raw, partner, plan, omega, ring, classes=scanmix.INSTANCE_CLASSES):
    """scanmix.mix_scan_host(atan="double") + ring_ids_host(atan="double") per frame, as torch operations on the device. Divisors
    are TENSORS (torch turns `tensor / python_float` into a multiplication by the reciprocal); every float64 product and sum is a
    launch of its own, so nothing is fused."""
    dev = raw["points"].device
    f32 = lambda v: torch.full((), float(v), dtype=torch.float32, device=dev)
    pi = f32(math.pi)
    rot = scanmix.omega_params(omega)
    pts_out, lab_out, sizes = [], [], []
    for f in range(raw["num_frames"]):
        p1, l1 = raw["points"][raw["offsets"][f]:raw["offsets"][f + 1]], raw["labels"][raw["offsets"][f]:raw["offsets"][f + 1]]
        p2, l2 = partner["points"][partner["offsets"][f]:partner["offsets"][f + 1]], partner["labels"][partner["offsets"][f]:partner["offsets"][f + 1]]
        kind, alpha, swap, paste = plan[f]
        assert kind == scanmix.POLARMIX
        pts, labs = [p1], [l1]
        if swap:
            a, b = (f32(v) for v in scanmix.sector_edges(alpha))
            yaw1 = -torch.atan2(p1[:, 1].double(), p1[:, 0].double()).float()
            yaw2 = -torch.atan2(p2[:, 1].double(), p2[:, 0].double()).float()
            in1, in2 = (yaw1 > a) & (yaw1 < b), (yaw2 > a) & (yaw2 < b)
            pts, labs = [p1[~in1], p2[in2]], [l1[~in1], l2[in2]]
        if paste:
            idx = torch.cat([torch.nonzero(l2 == c).reshape(-1) for c in classes])
            inst, inst_l = p2[idx], l2[idx]
            pts.append(inst)
            labs.append(inst_l)
            x, y, z = (inst[:, k].double() for k in range(3))
            for j in range(2):
                c, s = float(rot[j, 0]), float(rot[j, 1])
                X, Y, Z = (x * c + y * (-s)) + 0.0, (x * s + y * c) + 0.0, z + 0.0   # the affine map's additions of a zero jitter
                pts.append(torch.stack([X.float(), Y.float(), Z.float(), inst[:, 3]], dim=1))
                labs.append(inst_l)
        mixed = torch.cat(pts)
        if ring:
            yaw = -torch.atan2(mixed[:, 1].double(), (-mixed[:, 0]).double()).float()
            proj = 0.5 * (yaw / pi + 1.0)
            flag = torch.zeros(mixed.shape[0], dtype=torch.int64, device=dev)
            flag[1:] = (proj[1:] < 0.2) & (proj[:-1] > 0.8)
            mixed = torch.cat([mixed, torch.cumsum(flag, 0).clamp(0, 63).float()[:, None]], dim=1)
        pts_out.append(mixed)
        lab_out.append(torch.cat(labs))
        sizes.append(mixed.shape[0])
    return {"points": torch.cat(pts_out), "labels": torch.cat(lab_out), "offsets": [0] + np.cumsum(sizes).tolist(), "num_frames": raw["num_frames"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan, 120 000)")
    ap.add_argument("--reps", type=int, default=10, help="calls per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    seeds = list(range(args.scans))
    cuda = lambda d: {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    raw, partner = cuda(synthetic.make_raw_batch(seeds, args.points)), cuda(synthetic.make_partner_raw_batch(seeds, args.points))
    rng = np.random.RandomState(0)
    omega = scanmix.draw_omega(rng)
    plan = np.array([[scanmix.POLARMIX, (rng.random() - 1) * np.pi, rng.random() < 0.5, rng.random() < 1.0] for _ in seeds], dtype=np.float64)
    rows = []
    for tag, ring in (("mix", False), ("mix_ring", True)):
        a, b = scanmix.device_mix(raw, partner, plan, omega, ring=ring), torch_mix(raw, partner, plan, omega, ring)
        same = bool(a["offsets"] == b["offsets"] and torch.equal(a["points"].view(torch.int32), b["points"].view(torch.int32))
                    and torch.equal(a["labels"], b["labels"]))
        assert same, "%s: device_mix and the torch composition differ" % tag
        mixed_rows = a["offsets"][-1]
        del a, b
        med, spread = alternate({"device_mix": lambda: scanmix.device_mix(raw, partner, plan, omega, ring=ring),
                                 "torch_composition": lambda: torch_mix(raw, partner, plan, omega, ring)}, args.reps, args.rounds, args.warmup)
        row = {"case": tag, "ms": {k: round(v, 4) for k, v in med.items()},
               "ms_min_max": {k: [round(lo, 4), round(hi, 4)] for k, (lo, hi) in spread.items()},
               "speedup": round(med["torch_composition"] / med["device_mix"], 3),
               "difference_beyond_spread": bool(spread["device_mix"][1] < spread["torch_composition"][0]
                                                or spread["device_mix"][0] > spread["torch_composition"][1]),
               "frames": args.scans, "points": int(raw["points"].shape[0]), "partner_points": int(partner["points"].shape[0]),
               "mixed_rows": int(mixed_rows), "swaps": int(plan[:, 2].sum()), "equal_tensors": same}
        print(json.dumps(row), flush=True)
        rows.append(row)
    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points_per_scan": int(raw["points"].shape[0]) // args.scans,
           "reps_per_block": args.reps, "rounds": args.rounds, "method": "device events, alternating blocks, median block per variant",
           "not_measured": ["lasermix='radians'", "the kernels alone through the C ABI", "device_mix inside a training step"], "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
