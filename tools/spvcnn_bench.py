#!/usr/bin/env python3
"""The SPVCNN-18 workload (openpcseg_amd/workloads/spvcnn.py) on the 12-scan bench batch: one training step (forward, loss,
backward, SGD update) in fp32 and under bf16 autocast, with the point-branch merge kernel on and off (PCS_POINT_MERGE) and, in
bf16, with the point <-> voxel policy "fp32" (cast around every hop: "cast") against "keep" (the 16-bit kernels); and each of the
three merge hops alone, the kernel of csrc/pointmerge.hip against the three operations it replaces (devoxelize, BatchNorm apply
with the gate mask, add).

Device events around blocks of steps / calls, the variants alternating block by block, the median of the blocks of a variant
(three rounds by default). The hop bytes are ALGORITHMIC: the Linear output read once, the merged rows written once, the mask,
the corner map, and the voxel rows once. Writes profiles/spvcnn_workload_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from openpcseg_amd import functional as F  # noqa: E402
from openpcseg_amd import native  # noqa: E402
from openpcseg_amd.sparse import SparseTensor  # noqa: E402
from openpcseg_amd.workloads.spvcnn import SPVCNN  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_batch  # noqa: E402

HOPS = [(16, 256), (4, 128), (1, 96)]   # (stride of the voxel level, channels) of the three merges


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


def hop_bench(args, coords):
    be = native.backend()
    c1 = coords[torch.argsort(be.hash(coords))].contiguous()   # voxel order of initial_voxelize: ascending hash
    lv = {1: c1}
    for s in (1, 2, 4, 8):
        lv[2 * s] = be.downsample(lv[s], [2 * s] * 3)
    zc = coords.float()
    n = zc.shape[0]
    rows = []
    for s, c in HOPS:
        vox = lv[s]
        m = vox.shape[0]
        idx8, w8 = be.corner_map(zc, vox, s)
        stat = torch.cat([0.1 * torch.randn(c, dtype=torch.float64), 0.5 + torch.rand(c, dtype=torch.float64)]).cuda()
        gamma, beta = (0.75 + 0.5 * torch.rand(c)).cuda(), (0.2 * torch.rand(c) - 0.1).cuda()
        for dtype in (torch.float32, torch.bfloat16):
            e = 4 if dtype == torch.float32 else 2
            vf, lin = torch.randn(m, c, device="cuda").to(dtype), torch.randn(n, c, device="cuda").to(dtype)

            def three(vf=vf, lin=lin):
                y, mask = be.bn_apply(lin, None, stat, gamma, beta, True, want_mask=True)
                return be.devoxelize_fwd(vf, idx8, w8) + y

            variants = {"merge": lambda vf=vf, lin=lin: be.point_merge(vf, idx8, w8, lin, stat, gamma, beta)[0], "three_ops": three}
            same = bool(torch.equal(variants["merge"](), three())) if dtype == torch.float32 else None
            med, spread = alternate(variants, args.reps, args.rounds, args.warmup)
            nbytes = (2 * n + m) * c * e + n * c // 8 + n * 64
            row = {"stride": s, "c": c, "dtype": str(dtype).split(".")[1], "points": n, "voxels": m, "algorithmic_bytes": nbytes,
                   "us": {k: round(v * 1e3, 1) for k, v in med.items()},
                   "us_min_max": {k: [round(a * 1e3, 1), round(b * 1e3, 1)] for k, (a, b) in spread.items()},
                   "merge_gbps": round(nbytes / med["merge"] / 1e6, 1), "speedup": round(med["three_ops"] / med["merge"], 3),
                   "fp32_bit_identical": same}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def step_bench(args, feats, coords, labels):
    model = SPVCNN(num_class=20, cr=1.0).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)

    def step(amp, policy, merge):
        def run():
            os.environ["PCS_POINT_MERGE"] = merge
            F.set_pointvoxel_policy(policy)
            batch = {"lidar": SparseTensor(feats, coords), "targets": SparseTensor(labels, coords)}
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                loss = model(batch)["loss"]
            loss.backward()
            opt.step()
        return run

    variants = {"fp32/merge": step(False, "fp32", "1"), "fp32/literal": step(False, "fp32", "0"),
                "bf16_cast/merge": step(True, "fp32", "1"), "bf16_cast/literal": step(True, "fp32", "0"),
                "bf16_keep/merge": step(True, "keep", "1"), "bf16_keep/literal": step(True, "keep", "0")}
    try:
        med, spread = alternate(variants, args.steps, args.rounds, args.step_warmup)
    finally:
        F.set_pointvoxel_policy("fp32")
        os.environ.pop("PCS_POINT_MERGE", None)
    frames = int(coords[:, 3].max()) + 1
    return {k: {"ms_per_step": round(v, 2), "ms_min_max": [round(spread[k][0], 2), round(spread[k][1], 2)],
                "frames_per_s": round(frames / v * 1e3, 2)} for k, v in med.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan)")
    ap.add_argument("--reps", type=int, default=20, help="calls per block of the hop measurement")
    ap.add_argument("--steps", type=int, default=4, help="training steps per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true", help="the hop measurement only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spvcnn_workload_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spvcnn_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    b = make_batch(list(range(args.scans)), n_points=args.points)
    feats, coords, labels = b["lidar"].F.cuda(), b["lidar"].C.cuda().contiguous(), b["targets"].F.cuda()
    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points": int(coords.shape[0]), "rounds": args.rounds,
           "hop_reps": args.reps, "steps_per_block": args.steps, "method": "device events, alternating blocks, median block per variant"}
    rec["hops"] = hop_bench(args, coords)
    if not args.no_steps:
        rec["training_step"] = step_bench(args, feats, coords, labels)
        print(json.dumps(rec["training_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
