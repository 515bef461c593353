#!/usr/bin/env python3
"""The fusion (RPVNet) dataset's batch on the device (openpcseg_amd/rangeview.py device_batch, csrc/rangeproj.hip) against the
same arithmetic composed from torch operations in this process.

On twelve 120 000-point scans with their rings (workloads.synthetic.make_fusion_raw_batch, resident in HBM), one cut per scan, and
on ONE scan under the ten votes of test-time augmentation:
  *_batch    rangeview.device_batch  vs  transform.device_batch + torch_range_view: the projection as elementwise torch launches,
             the collision rule as scatter_reduce(amax) on the row index (index_put with duplicates is not deterministic), the
             image as a gather + where + permute. Whether the two give equal tensors is reported, not assumed.
  *_view     the range view alone on the batch's voxel rows: native range_project (the cuts' upload, the two clears and the two
             kernels) vs torch_range_view.
  *_kernels  pcs_range_project_f32 and pcs_range_image_fill_f32 alone through the C ABI, each with GB/s on its ALGORITHMIC bytes: the
             projection reads 4 c + 4 B and writes 12 B per row (its clear of `winner` is part of the entry and of the time); the
             fill reads the winners (4 B per pixel) and the winning rows (4 c B per hit pixel) and writes 20 B per pixel.

Device events around blocks of calls, the variants of a case alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. Writes profiles/rpvnet_batch_bench.json (--out)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import native, rangeview  # noqa: E402
from openpcseg_amd import transform as T  # noqa: E402
from openpcseg_amd.workloads import synthetic  # noqa: E402

HW = (64, 2048)
VOXEL = 0.05


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


def torch_range_view(feats, scenes, cuts, num_scenes, hw):
    """rangeview.range_view_host(atan="double") per scene + the collates' table, as torch operations on the device. Divisors are
    TENSORS: torch turns `tensor / python_float` into a multiplication by the reciprocal, which is not NumPy's float32 division."""
    h, w = hw
    dev = feats.device
    f32 = lambda v: torch.full((), v, dtype=torch.float32, device=dev)
    pi, two_pi = f32(math.pi), f32(2 * math.pi)
    x, y, z, refl, ring = (feats[:, k] for k in range(5))
    cut = native._h2d(rangeview.cut_value(cuts).reshape(-1).tolist(), torch.float32, dev)
    yaw = torch.atan2(y.double(), (-x).double()).float() + cut[scenes]
    yaw = torch.remainder(yaw, two_pi) - pi
    ix = torch.round(0.5 * (yaw / pi + 1.0) * float(w - 1)).long()
    iy = torch.round(ring).long()
    n = feats.shape[0]
    winner = torch.full((num_scenes * h * w,), -1, dtype=torch.int64, device=dev)
    winner.scatter_reduce_(0, (scenes * h + iy) * w + ix, torch.arange(n, device=dev), "amax")
    hit = winner >= 0
    rows = feats[winner.clamp(min=0)]
    depth = torch.sqrt((rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1]) + rows[:, 2] * rows[:, 2])
    ch0 = (25 * ((f32(1.0) / depth).double() - 0.4)).float()
    ch1 = (20 * (rows[:, 3].double() - 0.5)).float()
    px = torch.stack([ch0, ch1, rows[:, 0], rows[:, 1], rows[:, 2]], dim=1)
    empty = torch.tensor([-10.0, -10.0, 0.0, 0.0, 0.0], device=dev)
    image = torch.where(hit[:, None], px, empty).view(num_scenes, h, w, 5).permute(0, 3, 1, 2).contiguous()
    pxpy = torch.stack([scenes.float(), (2.0 * (ix.double() / (w - 1) - 0.5)).float(), (2.0 * (iy.double() / (h - 1) - 0.5)).float()], dim=1)
    return image, pxpy


def torch_batch(raw, params, cuts, votes):
    out = T.device_batch(raw, VOXEL, params, votes=votes)
    scenes = out["lidar"].C[:, 3].long()
    out["range_image"], out["range_pxpy"] = torch_range_view(out["lidar"].F, scenes, cuts, votes * raw["num_frames"], HW)
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpvnet_batch_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rpvnet_input_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    be = native.backend()
    host = synthetic.make_fusion_raw_batch(list(range(args.scans)), n_points=args.points)
    raw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in host.items()}
    n, c = raw["points"].shape
    n1 = raw["offsets"][1]
    one = {"points": raw["points"][:n1].contiguous(), "labels": raw["labels"][:n1].contiguous(), "num_frames": 1, "offsets": [0, n1]}
    rng = np.random.RandomState(0)
    train = (raw, T.draw_train_params(args.scans, rng=rng), rng.rand(args.scans), 1)
    tta = (one,) + rangeview.tta_params(1, 10, rng=rng) + (10,)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = []
    for tag, (batch_raw, params, cuts, votes) in (("train", train), ("tta", tta)):
        scenes_n = votes * batch_raw["num_frames"]
        a, b = rangeview.device_batch(batch_raw, VOXEL, params, cuts, votes=votes), torch_batch(batch_raw, params, cuts, votes)
        same = {k: bool(torch.equal(a[k], b[k])) for k in ("range_image", "range_pxpy")}
        feats, scenes = a["lidar"].F.contiguous(), a["lidar"].C[:, 3].contiguous()
        hits = int((a["range_image"][:, 0] != -10).sum())
        del a, b
        med, spread = alternate({"device_batch": lambda: rangeview.device_batch(batch_raw, VOXEL, params, cuts, votes=votes, check=False),
                                 "torch_composition": lambda: torch_batch(batch_raw, params, cuts, votes)}, args.reps, args.rounds, args.warmup)
        common = {"points": int(batch_raw["points"].shape[0]), "scenes": scenes_n, "voxel_rows": int(feats.shape[0]), "hit_pixels": hits}
        rows.append(record(tag + "_batch", med, spread, "device_batch", "torch_composition", dict(common, equal_tensors=same)))

        scenes64 = scenes.long()
        med, spread = alternate({"range_project": lambda: be.range_project(feats, scenes, cuts, scenes_n, HW),
                                 "torch_composition": lambda: torch_range_view(feats, scenes64, cuts, scenes_n, HW)},
                                args.reps, args.rounds, args.warmup)
        rows.append(record(tag + "_view", med, spread, "range_project", "torch_composition", common))

        m, pixels = feats.shape[0], scenes_n * HW[0] * HW[1]
        cut_dev = torch.from_numpy(rangeview.cut_value(cuts).reshape(-1)).cuda()
        winner = torch.empty(pixels, dtype=torch.int32, device="cuda")
        pxpy = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        bad = torch.empty(1, dtype=torch.int32, device="cuda")
        image = torch.empty((scenes_n, 5) + HW, dtype=torch.float32, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def project():
            native._check(be.lib.pcs_range_project_f32(ptr(feats), m, c, ptr(scenes), ptr(cut_dev), scenes_n, HW[0], HW[1], ptr(winner), ptr(pxpy),
                                                       ptr(bad), st), "pcs_range_project_f32")

        def fill():
            native._check(be.lib.pcs_range_image_fill_f32(ptr(winner), ptr(feats), m, c, scenes_n, HW[0], HW[1], ptr(image), st),
                          "pcs_range_image_fill_f32")

        project()
        med, spread = alternate({"project": project, "fill": fill}, args.reps * 2, args.rounds, args.warmup)
        nbytes = {"project": m * (4 * c + 4 + 12), "fill": pixels * (4 + 20) + hits * 4 * c}
        rows.append(record(tag + "_kernels", med, spread, None, None,
                           dict(common, algorithmic_bytes=nbytes, gbps={k: round(nbytes[k] / v / 1e6, 1) for k, v in med.items()})))

    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points_per_scan": n // args.scans, "columns": c, "hw": list(HW),
           "reps_per_block": args.reps, "rounds": args.rounds,
           "method": "device events, alternating blocks, median block per variant", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
