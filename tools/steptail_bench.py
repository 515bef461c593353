"""The tail of a training step, torch's sequence against openpcseg_amd.optim.FusedSGD, on bench.py's MinkUNet-34.

(a) what bench.py runs: clip_grad_norm_(params, 10) + torch.optim.SGD(momentum 0.9, weight decay 1e-4, nesterov).step(); under fp16
    also scaler.unscale_ / scaler.step / scaler.update of torch.amp.GradScaler.
(b) FusedSGD.step(max_norm=10, scaler=LossScaler under fp16): csrc/steptail.hip, two launches.

Per precision regime (fp32, autocast bf16, autocast fp16):
  tail   the tail alone over the gradients of one real backward, kept resident: device events around a block of calls (so the gaps
         the host leaves between launches count, as they do in a training step) and the host's wall time inside the calls;
  step   the whole training step (zero_grad, forward, loss, backward, tail) with either tail.
The variants alternate block by block; a figure is the median block of a variant (three rounds by default) and comes with the
block-to-block spread. Both tails update the same parameters from the same gradients, so the model stays one model; torch's tail
rescales the resident gradients in place on every call, which changes values, not the work. Writes profiles/steptail_bench.json (--out).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from openpcseg_amd import optim  # noqa: E402
from openpcseg_amd.workloads.minkunet import MinkUNet  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_batch  # noqa: E402

import bench  # noqa: E402  (the flagship workload's layer counts and batch helpers)


def block(run, reps):
    """(device ms per call by events, host ms per call spent inside the calls) of one block."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host * 1e3 / reps


def alternate(variants, reps, rounds, warm):
    for run in variants.values():
        for _ in range(warm):
            run()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, run in variants.items():
            times[k].append(block(run, reps))

    def stats(vals):
        return {"median": round(statistics.median(vals), 4), "min": round(min(vals), 4), "max": round(max(vals), 4)}
    return {k: {"device_ms": stats([d for d, _ in v]), "host_ms": stats([h for _, h in v])} for k, v in times.items()}


def beyond_spread(res, key):
    a, b = res["torch"][key], res["fused"][key]
    return bool(b["max"] < a["min"] or b["min"] > a["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20, help="tail calls per block")
    ap.add_argument("--steps", type=int, default=5, help="training steps per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--amp", default="off,bf16,fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steptail_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batch = bench.to_device(make_batch(list(range(args.frames))), dev)
    out = {"workload": "MinkUNet-34 cr1.0, %d frames, %d voxels" % (args.frames, batch["lidar"].C.shape[0]),
           "device": torch.cuda.get_device_name(0), "method": "device events around blocks, variants alternating block by block, median "
           "block of %d rounds, min / max = block-to-block spread; tail: %d calls per block, step: %d steps per block"
           % (args.rounds, args.reps, args.steps), "regimes": {}}
    for amp in args.amp.split(","):
        torch.manual_seed(0)
        model = MinkUNet(num_class=20, num_layer=bench.MK34_LAYERS, cr=1.0).to(dev).train()
        params = [p for p in model.parameters() if p.requires_grad]
        kw = dict(lr=0.02 * args.frames / 8, momentum=0.9, weight_decay=1e-4, nesterov=True)
        topt, fopt = torch.optim.SGD(params, **kw), optim.FusedSGD(params, **kw)
        amp_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(amp)
        tscaler = torch.amp.GradScaler("cuda") if amp == "fp16" else None
        fscaler = optim.LossScaler() if amp == "fp16" else None

        def backward(scaler):
            if amp_dtype is None:
                loss = model(bench.fresh(batch))["loss"]
            else:
                with torch.autocast("cuda", dtype=amp_dtype):
                    loss = model(bench.fresh(batch))["loss"]
            (loss if scaler is None else scaler.scale(loss)).backward()

        def torch_tail():
            if tscaler is not None:
                tscaler.unscale_(topt)
            torch.nn.utils.clip_grad_norm_(params, 10.0)
            if tscaler is not None:
                tscaler.step(topt)
                tscaler.update()
            else:
                topt.step()

        def fused_tail():
            fopt.step(max_norm=10.0, scaler=fscaler)

        def torch_step():
            topt.zero_grad(set_to_none=True)
            backward(tscaler)
            torch_tail()

        def fused_step():
            fopt.zero_grad(set_to_none=True)
            backward(fscaler)
            fused_tail()

        rec = {"parameters": sum(p.numel() for p in params), "tensors": len(params)}
        rec["step"] = alternate({"torch": torch_step, "fused": fused_step}, args.steps, args.rounds, warm=3)
        topt.zero_grad(set_to_none=True)
        backward(tscaler)                    # the resident gradients of the tail-only blocks
        if fscaler is not None:              # both scalers at the scale these gradients carry
            fscaler.load_state_dict(tscaler.state_dict())
        rec["tail"] = alternate({"torch": torch_tail, "fused": fused_tail}, args.reps, args.rounds, warm=3)
        for part in ("tail", "step"):
            rec[part]["fused_differs_beyond_spread"] = {k: beyond_spread(rec[part], k) for k in ("device_ms", "host_ms")}
        out["regimes"][amp] = rec
        print(amp, json.dumps(rec))
        del model, params, topt, fopt
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
