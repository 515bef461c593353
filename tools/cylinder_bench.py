#!/usr/bin/env python3
"""The Cylinder3D workload (openpcseg_amd/workloads/cylinder.py) on a batch built by `cylinder.cylinder_sample` from the bench's
synthetic scans: the ReconBlock gate alone -- the kernels of csrc/recongate.hip against the literal sequence they replace
(three BatchNorm applies, three sigmoids, two adds, a multiply, and their autograd backward), forward and backward, fp32 and
bf16 -- and one training step (forward, loss, backward, SGD update) in fp32 and under bf16 autocast with the gate kernel on and
off (PCS_RECON_GATE). --eval: the evaluation forward (eval mode, no grad) of the same batch, unfrozen against
`openpcseg_amd.freeze` (every conv -> LeakyReLU -> BatchNorm triple one launch, PCS_EP_POST_AFFINE), in fp32 and under bf16
autocast; that section alone is measured and merged into the record --out already holds.

Device events around blocks of calls / steps, the variants alternating block by block, the median of the blocks of a variant
(three rounds by default), after a warm-up of every variant. The gate's bytes are ALGORITHMIC, counted from shapes: forward 4
reads + 1 write of an (N, C) tensor, backward 5 reads twice + 4 writes. Writes profiles/cylinder_workload_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import cylinder, fused  # noqa: E402
from openpcseg_amd.fused import FusedBatchNorm  # noqa: E402
from openpcseg_amd.workloads.cylinder import CylinderTS, cylinder_batch  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_scan  # noqa: E402

CYL_LO, CYL_HI, CYL_GRID = [0, -180, -4], [50, 180, 2], [480, 360, 32]   # R:tools/cfgs/voxel/semantic_kitti/cylinder_cy480_cr10.yaml:7-9


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


def gate_bench(args, n, c):
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        e = 4 if dtype == torch.float32 else 2
        bns = [FusedBatchNorm(c).cuda().train() for _ in range(3)]
        a3 = [(3.0 * k + torch.randn(n, c, device="cuda")).to(dtype).requires_grad_() for k in range(3)]
        x = torch.randn(n, c, device="cuda").to(dtype).requires_grad_()
        dy = torch.randn(n, c, device="cuda").to(dtype)

        def forward(switch):
            def run():
                os.environ["PCS_RECON_GATE"] = switch
                with torch.no_grad():
                    for bn in bns:
                        bn.eval()       # the apply pass alone: the statistics passes are the same on both sides
                    fused.recon_gate(bns, a3, x)
                    for bn in bns:
                        bn.train()
            return run

        def both(switch):
            def run():
                os.environ["PCS_RECON_GATE"] = switch
                for t in a3 + [x]:
                    t.grad = None
                fused.recon_gate(bns, a3, x).backward(dy)
            return run

        variants = {"forward/gate": forward("1"), "forward/literal": forward("0"), "train/gate": both("1"), "train/literal": both("0")}
        try:
            med, spread = alternate(variants, args.reps, args.rounds, args.warmup)
        finally:
            os.environ.pop("PCS_RECON_GATE", None)
        fwd_bytes, bwd_bytes = 5 * n * c * e, 14 * n * c * e
        row = {"n": n, "c": c, "dtype": str(dtype).split(".")[1], "forward_algorithmic_bytes": fwd_bytes, "backward_algorithmic_bytes": bwd_bytes,
               "us": {k: round(v * 1e3, 1) for k, v in med.items()},
               "us_min_max": {k: [round(a * 1e3, 1), round(b * 1e3, 1)] for k, (a, b) in spread.items()},
               "forward_gate_gbps": round(fwd_bytes / med["forward/gate"] / 1e6, 1),
               "forward_speedup": round(med["forward/literal"] / med["forward/gate"], 3),
               "train_speedup": round(med["train/literal"] / med["train/gate"], 3),
               "note": "train/* = training-mode forward (statistics included) + backward"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def step_bench(args, batch):
    model = CylinderTS(num_class=20, init_size=32).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4, momentum=0.9)

    def step(amp, switch):
        def run():
            os.environ["PCS_RECON_GATE"] = switch
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                loss = model(batch)["loss"]
            loss.backward()
            opt.step()
        return run

    variants = {"fp32/gate": step(False, "1"), "fp32/literal": step(False, "0"), "bf16/gate": step(True, "1"), "bf16/literal": step(True, "0")}
    try:
        med, spread = alternate(variants, args.steps, args.rounds, args.step_warmup)
    finally:
        os.environ.pop("PCS_RECON_GATE", None)
    frames = int(batch["point_coord"][:, -1].max()) + 1
    return {k: {"ms_per_step": round(v, 2), "ms_min_max": [round(spread[k][0], 2), round(spread[k][1], 2)],
                "frames_per_s": round(frames / v * 1e3, 2)} for k, v in med.items()}


def eval_bench(args, batch):
    """Eval-mode forward, two models with the same weights: one as it is, one frozen. The traffic the frozen forward no longer
    moves is counted from shapes: a triple's (N, C) output is neither read again nor written a second time, 2 N C e bytes."""
    import openpcseg_amd
    plain = CylinderTS(num_class=20, init_size=32).cuda().eval()
    frozen = CylinderTS(num_class=20, init_size=32).cuda().eval()
    frozen.load_state_dict(plain.state_dict())
    report = openpcseg_amd.freeze(frozen)

    def forward(model, amp):
        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                model(batch)
        return run

    variants = {"fp32/unfrozen": forward(plain, False), "fp32/frozen": forward(frozen, False),
                "bf16/unfrozen": forward(plain, True), "bf16/frozen": forward(frozen, True)}
    med, spread = alternate(variants, args.steps, args.rounds, args.step_warmup)
    frames = int(batch["point_coord"][:, -1].max()) + 1
    out = {k: {"ms_per_forward": round(v, 2), "ms_min_max": [round(spread[k][0], 2), round(spread[k][1], 2)],
               "frames_per_s": round(frames / v * 1e3, 2)} for k, v in med.items()}
    out["freeze_report"] = report
    out["frozen_speedup"] = {d: round(med[d + "/unfrozen"] / med[d + "/frozen"], 3) for d in ("fp32", "bf16")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=2)
    ap.add_argument("--points", type=int, default=None, help="rays per scan (default: the full scan)")
    ap.add_argument("--reps", type=int, default=20, help="calls per block of the gate measurement")
    ap.add_argument("--steps", type=int, default=4, help="training steps per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true", help="the gate measurement only")
    ap.add_argument("--eval", action="store_true", help="the eval forward, unfrozen against frozen, only; merged into --out")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cylinder_workload_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cylinder_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    samples = []
    for seed in range(args.scans):
        pts = torch.from_numpy(make_scan(seed, args.points).astype(np.float32)).cuda()
        labels = torch.from_numpy(np.random.default_rng(seed + 100).integers(0, 20, size=pts.shape[0]).astype(np.int64)).cuda()
        samples.append(cylinder.cylinder_sample(pts, labels, CYL_LO, CYL_HI, CYL_GRID, 20))
    batch = cylinder_batch(samples)
    n = int(batch["voxel_coord"].shape[0])
    rec = {"device": torch.cuda.get_device_name(0), "scans": args.scans, "points": int(batch["point_coord"].shape[0]), "voxels": n,
           "rounds": args.rounds, "gate_reps": args.reps, "steps_per_block": args.steps,
           "method": "device events, alternating blocks, median block per variant"}
    if args.eval:
        if os.path.exists(args.out):
            with open(args.out) as f:
                rec = json.load(f)
        rec["eval_forward"] = dict(eval_bench(args, batch), scans=args.scans, points=int(batch["point_coord"].shape[0]), voxels=n,
                                   forwards_per_block=args.steps, rounds=args.rounds, device=torch.cuda.get_device_name(0))
        print(json.dumps(rec["eval_forward"]), flush=True)
    else:
        rec["gate"] = gate_bench(args, n, 64)
    if not args.no_steps and not args.eval:
        rec["training_step"] = step_bench(args, batch)
        print(json.dumps(rec["training_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
