#!/usr/bin/env python3
"""The RPVNet-34 cr 1.75 workload (openpcseg_amd/workloads/rpvnet.py) on the 4-frame batch tools/modelbench.py uses for it (5-channel
points, one (5, 64, 2048) range image per frame): one training step (forward, loss, backward, SGD update) in fp32 and under bf16
autocast with the range-point-voxel merge kernel on and off (PCS_RANGE_MERGE; 0 = the kernel sequence of the commit before the
kernel); and each of the four merge hops alone, the kernel route of csrc/rangemerge.hip against the literal sequence (devoxelize,
range_sample, add, BatchNorm apply, add). At the widths that are no multiple of 32 (56 and 168) the kernel route is the BatchNorm
apply pass followed by the kernel in add mode.

Device events around blocks of steps / calls, the variants alternating block by block, the median of the blocks of a variant
(three rounds by default) and the block-to-block spread. The hop bytes are ALGORITHMIC: the Linear output read once, the merged rows
written once, the mask, the corner map, pxpy, and the voxel rows and the image once (bn mode); add mode adds the BatchNorm pass's
read and write. A hop whose kernel median is slower than the literal median beyond the spread is listed under "slower_hops": that
width belongs on the literal sequence. Writes profiles/rpvnet_workload_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

import fullsize as fs  # noqa: E402
from openpcseg_amd import native  # noqa: E402
from openpcseg_amd.sparse import SparseTensor  # noqa: E402
from openpcseg_amd.workloads.rpvnet import RPVNet  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_batch  # noqa: E402

HOPS = [(1, 56, 1), (16, 448, 16), (4, 224, 4), (1, 168, 1)]   # (stride of the voxel level, channels, reduction of the range image)


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


def make_inputs(scans, points):
    b = make_batch(list(range(scans)), n_points=points)
    feats, coords, labels = b["lidar"].F, b["lidar"].C, b["targets"].F
    feats = torch.cat([feats, torch.frac(feats[:, :1] * 0.37 + feats[:, 3:4] * 1.9).abs()], dim=1).contiguous()   # the fifth channel
    imgs, pxpy = [], []
    for i in range(scans):
        img, pp = fs.range_view(feats[coords[:, 3] == i])
        pp[:, 0] = i
        imgs.append(img)
        pxpy.append(pp)
    return feats.cuda(), coords.cuda().contiguous(), labels.cuda(), torch.cat(imgs, 0).cuda(), torch.cat(pxpy, 0).cuda()


def hop_bench(args, coords, pxpy, frames):
    be = native.backend()
    c1 = coords[torch.argsort(be.hash(coords))].contiguous()   # voxel order of initial_voxelize: ascending hash
    lv = {1: c1}
    for s in (1, 2, 4, 8):
        lv[2 * s] = be.downsample(lv[s], [2 * s] * 3)
    zc = coords.float()
    n = zc.shape[0]
    rows = []
    for s, c, red in HOPS:
        vox = lv[s]
        m = vox.shape[0]
        h, w = fs.RANGE_H // red, fs.RANGE_W // red
        idx8, w8 = be.corner_map(zc, vox, s)
        img = torch.randn(frames, c, h, w, device="cuda")
        stat = torch.cat([0.1 * torch.randn(c, dtype=torch.float64), 0.5 + torch.rand(c, dtype=torch.float64)]).cuda()
        gamma, beta = (0.75 + 0.5 * torch.rand(c)).cuda(), (0.2 * torch.rand(c) - 0.1).cuda()
        bn_mode = c % 32 == 0
        for dtype in (torch.float32, torch.bfloat16):
            e = 4 if dtype == torch.float32 else 2
            vf, lin = torch.randn(m, c, device="cuda").to(dtype), torch.randn(n, c, device="cuda").to(dtype)

            def literal(vf=vf, lin=lin):
                if bn_mode:
                    y, _ = be.bn_apply(lin, None, stat, gamma, beta, True, want_mask=True)
                else:
                    y = be.bn_apply(lin, None, stat, gamma, beta, True)
                return be.devoxelize_fwd(vf, idx8, w8) + be.range_sample_fwd(img, pxpy) + y

            def kernel(vf=vf, lin=lin):
                if bn_mode:
                    return be.range_point_merge(vf, idx8, w8, img, pxpy, lin, stat, gamma, beta)[0]
                y = be.bn_apply(lin, None, stat, gamma, beta, True)
                return be.range_point_merge(vf, idx8, w8, img, pxpy, y, None, None, None)[0]

            variants = {"kernel": kernel, "literal": literal}
            same = bool(torch.equal(kernel(), literal())) if dtype == torch.float32 else None
            med, spread = alternate(variants, args.reps, args.rounds, args.warmup)
            nbytes = (2 * n + m) * c * e + n * 64 + n * 12 + frames * c * h * w * 4 + (n * c // 8 if bn_mode else 2 * n * c * e)
            row = {"stride": s, "c": c, "mode": "bn" if bn_mode else "bn_apply + add", "image": [frames, c, h, w],
                   "dtype": str(dtype).split(".")[1], "points": n, "voxels": m, "algorithmic_bytes": nbytes,
                   "us": {k: round(v * 1e3, 1) for k, v in med.items()},
                   "us_min_max": {k: [round(a * 1e3, 1), round(b * 1e3, 1)] for k, (a, b) in spread.items()},
                   "kernel_gbps": round(nbytes / med["kernel"] / 1e6, 1), "speedup": round(med["literal"] / med["kernel"], 3),
                   "kernel_slower_beyond_spread": bool(spread["kernel"][0] > spread["literal"][1]), "fp32_bit_identical": same}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_bench(args, feats, coords, labels, image, pxpy):
    model = RPVNet(num_class=20).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)

    def step(amp, merge):
        def run():
            os.environ["PCS_RANGE_MERGE"] = merge
            cc = coords.view_as(coords)   # new tensor objects every step: the memos hung on caller tensors are rebuilt as in training
            batch = {"lidar": SparseTensor(feats.view_as(feats), cc), "targets": SparseTensor(labels.view_as(labels), cc),
                     "range_image": image.view_as(image), "range_pxpy": pxpy.view_as(pxpy)}
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                loss = model(batch)["loss"]
            loss.backward()
            opt.step()
        return run

    variants = {"fp32/merge": step(False, "1"), "fp32/literal": step(False, "0"),
                "bf16/merge": step(True, "1"), "bf16/literal": step(True, "0")}
    try:
        med, spread = alternate(variants, args.steps, args.rounds, args.step_warmup)
    finally:
        os.environ.pop("PCS_RANGE_MERGE", None)
    frames = image.shape[0]
    return {k: {"ms_per_step": round(v, 2), "ms_min_max": [round(spread[k][0], 2), round(spread[k][1], 2)],
                "frames_per_s": round(frames / v * 1e3, 2)} for k, v in med.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan)")
    ap.add_argument("--reps", type=int, default=20, help="calls per block of the hop measurement")
    ap.add_argument("--steps", type=int, default=3, help="training steps per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true", help="the hop measurement only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpvnet_workload_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rpvnet_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    feats, coords, labels, image, pxpy = make_inputs(args.scans, args.points)
    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points": int(coords.shape[0]), "rounds": args.rounds,
           "hop_reps": args.reps, "steps_per_block": args.steps, "method": "device events, alternating blocks, median block per variant"}
    rec["hops"] = hop_bench(args, coords, pxpy, args.scans)
    rec["slower_hops"] = [{"c": r["c"], "dtype": r["dtype"], "speedup": r["speedup"]} for r in rec["hops"] if r["kernel_slower_beyond_spread"]]
    if not args.no_steps:
        rec["training_step"] = step_bench(args, feats, coords, labels, image, pxpy)
        print(json.dumps(rec["training_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
