#!/usr/bin/env python3
"""The range-view scan and its KNN label vote on the device (openpcseg_amd/rangescan.py, csrc/rangescan.hip) against the same
results composed from torch operations in this process.

On twelve 120 000-point scans (workloads.synthetic.make_raw_batch, resident in HBM) and on ONE scan, at 64 x 2048:
  *_scan   rangescan.device_batch  vs  torch_scan: the projection as elementwise torch launches, the collision rule as ONE sort of
           (depth, index) keys in descending order followed by a "last write wins" put (scatter_reduce(amax) of the sorted position:
           index_put with duplicate indices is not deterministic on the device), the images as gathers + where. Equal tensors are
           ASSERTED before anything is timed.
  *_vote   rangescan.knn_vote  vs  torch_vote: the reference's own sequence per scan (two F.unfold, the gathers, topk, scatter_add_
           into a one-hot tensor, argmax). Equal outputs are ASSERTED; the proj_argmax is a seeded block-constant image, as in the
           fixture.
The kernels alone are measured in a run of their own: `rocprofv3 --kernel-trace --stats -- python tools/rangescan_bench.py --trace`
runs only the native calls (a few dozen of each), for the profiler's per-kernel table.

Device events around blocks of calls, the variants of a case alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. Writes profiles/rangescan_bench.json (--out)."""
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
import torch.nn.functional as F  # noqa: E402

from openpcseg_amd import rangescan  # noqa: E402
from openpcseg_amd.workloads import synthetic  # noqa: E402

HW = (64, 2048)
NUM_CLASS = 20
VOTE = dict(knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=NUM_CLASS)


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


def frame_ids(raw):
    """(frame of every row, its index within the frame) on the points' device. Built ONCE per batch, outside the timed calls, as a
    caller composing the scan from torch operations would: the uploads are pageable copies and repeat_interleave with device
    repeats waits for the host."""
    off, dev = raw["offsets"], raw["points"].device
    nf = raw["num_frames"]
    counts = torch.tensor([off[i + 1] - off[i] for i in range(nf)], device=dev)
    frame = torch.repeat_interleave(torch.arange(nf, device=dev), counts)
    local = torch.arange(raw["points"].shape[0], device=dev) - torch.tensor(off[:-1], device=dev)[frame]
    return frame, local


def torch_scan(raw, ids, hw=HW, fov=rangescan.FOV):
    """rangescan.device_batch (mask="reference", no table) as torch operations on the device; ids = frame_ids(raw). Divisors are
    TENSORS: torch turns `tensor / python_float` into a multiplication by the reciprocal, which is not NumPy's float32 division."""
    h, w = hw
    pts, labels = raw["points"], raw["labels"]
    dev, n, nf = pts.device, pts.shape[0], raw["num_frames"]
    frame, local = ids
    f32 = lambda v: torch.full((), float(v), dtype=torch.float32, device=dev)
    fov_down_abs, fov_total = (f32(v) for v in rangescan._fov_consts(fov))
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    # the square root in double, rounded once: that IS the correctly rounded float32 root (53 >= 2 * 24 + 2 bits), whatever the
    # float32 torch.sqrt of the build at hand does in its last bit
    depth = torch.sqrt(((x * x + y * y) + z * z).double()).float()
    yaw = -torch.atan2(y.double(), x.double()).float()
    pitch = torch.asin((z / depth).double()).float()
    fx = (0.5 * (yaw / f32(math.pi) + 1.0)) * float(w)
    fy = (1.0 - (pitch + fov_down_abs) / fov_total) * float(h)
    ix = torch.floor(fx).clamp(0, w - 1).int()
    iy = torch.floor(fy).clamp(0, h - 1).int()
    key = (depth.view(torch.int32).long() << 32) | local
    order = torch.argsort(key, descending=True)                 # far to near, among equal depths high index to low
    pixel = (frame * h + iy.long()) * w + ix.long()
    last = torch.full((nf * h * w,), -1, dtype=torch.int64, device=dev)
    last.scatter_reduce_(0, pixel[order], torch.arange(n, device=dev), "amax")    # the last write of every pixel, deterministically
    hit = last >= 0
    row = order[last.clamp(min=0)]
    minus = f32(-1.0)
    g = lambda v: torch.where(hit, v[row], minus)
    idx = torch.where(hit, local[row], torch.full((), -1, dtype=torch.int64, device=dev))
    mask = (idx > 0).float()
    scan = torch.stack([g(x) / f32(50.0), g(y) / f32(50.0), g(z) / f32(3.0), g(pts[:, 3]), g(depth) / f32(80.0), mask], dim=0)
    scan = scan.view(6, nf, h, w).permute(1, 0, 2, 3).contiguous()
    label = torch.where(hit, labels[row] & 0xFFFF, torch.zeros((), dtype=torch.int64, device=dev))
    return {"scan_rv": scan, "label_rv": label.view(nf, h, w), "mask_rv": mask.view(nf, h, w), "proj_idx": idx.int().view(nf, h, w),
            "proj_x": ix, "proj_y": iy, "unproj_range": depth}


def torch_vote(proj_range, proj_argmax, unproj_range, px, py, off, weights, knn, search, cutoff, num_class):
    """KNN.forward scan by scan, as the reference's validation loop calls it."""
    out = []
    pad = (search - 1) // 2
    w = proj_range.shape[2]
    for b in range(proj_range.shape[0]):
        u = unproj_range[off[b]:off[b + 1]]
        idx = py[off[b]:off[b + 1]].long() * w + px[off[b]:off[b + 1]].long()
        window = F.unfold(proj_range[b][None, None, ...], kernel_size=(search, search), padding=(pad, pad))[:, :, idx]
        window[window < 0] = float("inf")
        window[:, (search * search - 1) // 2, :] = u
        dist = torch.abs(window - u) * weights.view(1, -1, 1)
        _, knn_idx = dist.topk(knn, dim=1, largest=False, sorted=False)
        labels = F.unfold(proj_argmax[b][None, None, ...].float(), kernel_size=(search, search), padding=(pad, pad)).long()[:, :, idx]
        votes = torch.gather(labels, 1, knn_idx)
        if cutoff > 0:
            votes[torch.gather(dist, 1, knn_idx) > cutoff] = num_class
        onehot = torch.zeros((1, num_class + 1, u.shape[0]), device=u.device).scatter_add_(1, votes, torch.ones_like(votes).float())
        out.append((onehot[:, 1:-1].argmax(dim=1) + 1).view(-1))
    return torch.cat(out)


def block_argmax(nf, hw, seed=91, block=(4, 8)):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, NUM_CLASS, size=(nf, -(-hw[0] // block[0]), -(-hw[1] // block[1])))
    return torch.from_numpy(np.repeat(np.repeat(blocks, block[0], axis=1), block[1], axis=2)[:, :hw[0], :hw[1]].astype(np.int64)).cuda()


def record(name, med, spread, new, old, extra):
    row = {"case": name, "ms": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
           "speedup": round(med[old] / med[new], 3),
           "difference_beyond_spread": bool(spread[new][1] < spread[old][0] or spread[new][0] > spread[old][1])}
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
    ap.add_argument("--trace", action="store_true", help="only run the native calls, for a profiler's kernel table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rangescan_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rangescan_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    host = synthetic.make_raw_batch(list(range(args.scans)), n_points=args.points)
    raw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in host.items()}
    n1 = raw["offsets"][1]
    one = {"points": raw["points"][:n1].contiguous(), "labels": raw["labels"][:n1].contiguous(), "num_frames": 1, "offsets": [0, n1]}
    weights = torch.from_numpy(rangescan.inv_gauss_weights(VOTE["search"], VOTE["sigma"])).cuda()
    rows = []
    for tag, batch in (("batch", raw), ("one", one)):
        nf = batch["num_frames"]
        a = rangescan.device_batch(batch, HW)
        argmax = block_argmax(nf, HW)
        proj_range = a["scan_rv"][:, 4] * 80
        vote_args = (proj_range, argmax, a["unproj_range"], a["proj_x"], a["proj_y"], a["point_offset"])
        native_vote = lambda: rangescan.knn_vote(*vote_args, **VOTE)
        if args.trace:
            for _ in range(20):
                rangescan.device_batch(batch, HW, check=False)
                native_vote()
            torch.cuda.synchronize()
            continue
        ids = frame_ids(batch)
        b = torch_scan(batch, ids)
        differing = {k: int((a[k] != b[k]).sum()) for k in b}
        assert not any(differing.values()), ("device_batch and the torch composition differ", differing)
        hits = int((a["proj_idx"] >= 0).sum())
        common = {"points": int(batch["points"].shape[0]), "scans": nf, "hit_pixels": hits}
        del b
        med, spread = alternate({"device_batch": lambda: rangescan.device_batch(batch, HW, check=False), "torch_composition": lambda: torch_scan(batch, ids)},
                                args.reps, args.rounds, args.warmup)
        rows.append(record(tag + "_scan", med, spread, "device_batch", "torch_composition", dict(common, equal_tensors=True)))

        composed = lambda: torch_vote(*vote_args, weights, VOTE["knn"], VOTE["search"], VOTE["cutoff"], NUM_CLASS)
        mine, theirs = native_vote(), composed()
        assert torch.equal(mine, theirs), ("knn_vote and the torch composition differ", int((mine != theirs).sum()))
        pixel_label = torch.cat([argmax[s][a["proj_y"][lo:hi].long(), a["proj_x"][lo:hi].long()]
                                 for s, (lo, hi) in enumerate(zip(a["point_offset"][:-1], a["point_offset"][1:]))])
        changed = float((mine != pixel_label).float().mean())
        med, spread = alternate({"knn_vote": native_vote, "torch_composition": composed}, args.reps, args.rounds, args.warmup)
        rows.append(record(tag + "_vote", med, spread, "knn_vote", "torch_composition",
                           dict(common, equal_outputs=True, vote_changes_fraction=round(changed, 4))))
    if args.trace:
        return
    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points_per_scan": raw["points"].shape[0] // args.scans, "hw": list(HW),
           "vote": VOTE, "reps_per_block": args.reps, "rounds": args.rounds,
           "method": "device events, alternating blocks, median block per variant", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
