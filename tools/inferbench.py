"""Evaluation forward of the MinkUNet-34 cr 1.0 workload, unfrozen vs frozen (openpcseg_amd.freeze), and the prediction tail.

    python tools/inferbench.py [--out profiles/inference_bench.json] [--block-seconds 2] [--blocks 3] [--batches 1,12]

Same synthetic scans as bench.py (workloads/synthetic.py, seeds 0..11). For batch 1 and batch 12, fp32 and bf16 autocast, two
models with the same weights -- one frozen -- are timed IN THE SAME PROCESS IN ALTERNATING BLOCKS: every shape warmed up, each block
at least --block-seconds of back-to-back forwards between two device events and ended by a synchronise, --blocks blocks each.
Reported per mode: the per-block milliseconds per forward, their median and spread (max - min). The tail: the one-launch kernel
(inference.SegEvaluator.update) against a restatement of the reference's per-scene loop in torch on the device
(R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:436-455 + np.bincount scoring, R:infer.py:35-40). Profiler off; needs a GPU.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import openpcseg_amd  # noqa: E402
from openpcseg_amd import native  # noqa: E402
from openpcseg_amd.hostdata import sparse_collate_fn, sparse_quantize  # noqa: E402
from openpcseg_amd.inference import SegEvaluator  # noqa: E402
from openpcseg_amd.sparse import SparseTensor  # noqa: E402
from openpcseg_amd.workloads.minkunet import MK34_LAYERS, MinkUNet  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_scan  # noqa: E402


def eval_frames(seeds, n_points=None, num_classes=20):
    """Per-scan eval samples as the reference's dataset makes them: voxels + inverse_map + per-point labels."""
    frames = []
    for s in seeds:
        pts = make_scan(s, n_points)
        pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
        pc -= pc.min(0, keepdims=1)
        _, inds, inverse = sparse_quantize(pc, return_index=True, return_inverse=True)
        labels = np.random.default_rng(s + 12345).integers(0, num_classes, size=pts.shape[0]).astype(np.int64)
        frames.append({"lidar": SparseTensor(pts[inds].astype(np.float32), pc[inds]), "targets_mapped": SparseTensor(labels, pc),
                       "inverse_map": SparseTensor(np.asarray(inverse).astype(np.int64), pc), "num_points": np.array([pts.shape[0]])})
    return frames


def to_device(batch, dev):
    return {k: (SparseTensor(v.F.to(dev), v.C.int().to(dev)) if isinstance(v, SparseTensor) else v) for k, v in batch.items()}


def timed_blocks(fns, block_seconds, blocks):
    """fns: {name: callable}. Alternating blocks; -> {name: [ms per call of every block]}."""
    iters = {}
    for name, fn in fns.items():   # warm-up (every shape, code objects, prepared weights) and the per-call estimate
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(math.ceil(block_seconds / max((time.perf_counter() - t0) / 3, 1e-6))))
    out = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / iters[name])
    return out, iters


def summary(ms):
    return {"blocks_ms": [round(v, 4) for v in ms], "median_ms": round(float(np.median(ms)), 4), "spread_ms": round(max(ms) - min(ms), 4)}


def count_backend_calls(fn):
    be = native.backend()
    names = [n for n in dir(be) if not n.startswith("_") and callable(getattr(be, n)) and not isinstance(getattr(type(be), n, None), type)]
    counts, saved = {}, {}
    for n in names:
        saved[n] = getattr(be, n)

        def wrapped(*a, _o=saved[n], _n=n, **kw):
            counts[_n] = counts.get(_n, 0) + 1
            return _o(*a, **kw)
        setattr(be, n, wrapped)
    try:
        fn()
    finally:
        for n in names:
            delattr(be, n)
    return counts


def reference_tail_torch(logits, batch, hist_host, c):
    """The reference's loop with its host round trips, in torch on the device."""
    invs, labels, x = batch["inverse_map"], batch["targets_mapped"], batch["lidar"]
    for idx in range(int(invs.C[:, -1].max()) + 1):
        cur_scene = (x.C[:, -1] == idx).cpu().numpy()
        cur_inv = invs.F[invs.C[:, -1] == idx].cpu().numpy()
        cur_label = (labels.C[:, -1] == idx).cpu().numpy()
        n = int(batch["num_points"][idx])
        pred = logits[cur_scene][cur_inv].argmax(1)[:n].cpu().numpy()
        lab = labels.F[cur_label][:n].cpu().numpy()
        k = (lab >= 0) & (lab < c)
        hist_host += np.bincount(c * lab[k].astype(int) + pred[k], minlength=c * c)[:c * c].reshape(c, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "inference_bench.json"))
    ap.add_argument("--block-seconds", type=float, default=2.0)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--batches", default="1,12")
    ap.add_argument("--n-points", type=int, default=None, help="subsample every scan (rehearsals); default: full 120 000-point scans")
    ap.add_argument("--forward-only", choices=["frozen", "unfrozen"], default=None,
                    help="no timing: 3 warm-up + 5 forwards of the first --batches entry in this mode, for a run under "
                         "`rocprofv3 --kernel-trace --stats -- python tools/inferbench.py --forward-only frozen [--amp]`")
    ap.add_argument("--amp", action="store_true", help="with --forward-only: bf16 autocast")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inferbench needs an MI355X: a timing without the GPU says nothing")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    plain = MinkUNet(num_class=20, num_layer=MK34_LAYERS, cr=1.0).to(dev).eval()
    frozen = MinkUNet(num_class=20, num_layer=MK34_LAYERS, cr=1.0).to(dev).eval()
    frozen.load_state_dict(plain.state_dict())
    info = openpcseg_amd.freeze(frozen)
    if args.forward_only:
        nb = int(args.batches.split(",")[0])
        batch = to_device(sparse_collate_fn(eval_frames(list(range(nb)), args.n_points)), dev)
        model = frozen if args.forward_only == "frozen" else plain
        for _ in range(8):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.amp):
                model({"lidar": SparseTensor(batch["lidar"].F, batch["lidar"].C)})
        torch.cuda.synchronize()
        print(json.dumps({"forward_only": args.forward_only, "amp": args.amp, "batch": nb, "forwards": 8}))
        return
    result = {"device": torch.cuda.get_device_name(0), "model": "MinkUNet-34 cr1.0, eval forward", "freeze": info,
              "block_seconds": args.block_seconds, "blocks": args.blocks, "forward": {}, "tail": {}}

    for nb in [int(v) for v in args.batches.split(",")]:
        batch = to_device(sparse_collate_fn(eval_frames(list(range(nb)), args.n_points)), dev)
        feats, coords = batch["lidar"].F, batch["lidar"].C

        def forward(model, amp):
            def fn():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                    return model({"lidar": SparseTensor(feats, coords)})["logits"]
            return fn

        for amp in (False, True):
            key = "batch%d_%s" % (nb, "bf16" if amp else "fp32")
            fns = {"unfrozen": forward(plain, amp), "frozen": forward(frozen, amp)}
            ms, iters = timed_blocks(fns, args.block_seconds, args.blocks)
            rec = {name: summary(v) for name, v in ms.items()}
            rec["iterations_per_block"] = iters
            rec["voxels"] = int(coords.shape[0])
            rec["speedup_median"] = round(rec["unfrozen"]["median_ms"] / rec["frozen"]["median_ms"], 4)
            rec["difference_exceeds_spread"] = bool(rec["unfrozen"]["median_ms"] - rec["frozen"]["median_ms"] >
                                                    max(rec["unfrozen"]["spread_ms"], rec["frozen"]["spread_ms"]))
            calls = {name: count_backend_calls(fn) for name, fn in fns.items()}
            rec["backend_calls"] = {name: {"total": sum(c.values()), "bn_apply": c.get("bn_apply", 0),
                                           "conv": c.get("conv_gather_gemm", 0) + c.get("conv_gather_gemm_h", 0),
                                           "weight_preparation": c.get("prepare_weights_h", 0) + c.get("weights_multi", 0)}
                                    for name, c in calls.items()}
            a, b = fns["unfrozen"]().float(), fns["frozen"]().float()
            rec["max_abs_logit_difference"] = float((a - b).abs().max())
            rec["logit_rms"] = float(a.pow(2).mean().sqrt())
            result["forward"][key] = rec
            print(key, json.dumps(rec), flush=True)

        # the tail alone, on this batch's maps
        c = 20
        logits = torch.randn(coords.shape[0], c, device=dev) * 3
        ev = SegEvaluator(c)
        host_hist = np.zeros((c, c), dtype=np.int64)
        fns = {"kernel": lambda: ev.update(logits, batch), "reference_loop_torch": lambda: reference_tail_torch(logits, batch, host_hist, c)}
        ms, iters = timed_blocks(fns, min(args.block_seconds, 1.0), args.blocks)
        calls = {name: int(iters[name]) * args.blocks + 6 for name in fns}   # + warm-up calls: both histograms count every call
        hk = ev.hist.cpu().numpy()
        rec = {name: summary(v) for name, v in ms.items()}
        rec["points"] = int(batch["inverse_map"].F.shape[0])
        rec["histograms_agree"] = bool(np.array_equal(hk // calls["kernel"], host_hist // calls["reference_loop_torch"]) and
                                       (hk % calls["kernel"] == 0).all())
        result["tail"]["batch%d" % nb] = rec
        print("tail batch%d" % nb, json.dumps(rec), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
