#!/usr/bin/env python3
"""The range-view training criterion on the device (openpcseg_amd/rangeloss.py, csrc/rangeloss.hip) against the same criterion
composed from torch operations in this process.

Criterion forward + backward on (30, 20, 64, 512) and (12, 20, 64, 2048) logits -- BATCH_SIZE_PER_GPU of the reference's range
configs at the two image widths --, fp32 and bf16, seeded block-constant labels with class 0 present:
  range_criterion    rangeloss.RangeCriterion: statistics pass, one-sort Lovasz, fold, gradient pass;
  torch_composition  rangeloss.range_criterion_host in float32 on the same device tensors -- the reference's operations line by
                     line (three softmax calls, the one-hot builds, two max_pool2d, the reductions), with the Lovasz term in its
                     batched torch form (workloads/losses.py; the reference's own per-class loop is slower still) -- and autograd.
Before anything is timed the five values of both are ASSERTED against the float64 host form on the CPU within the bound of
tests/test_rangeloss.py: |x - host64| <= 4 max(|host32 - host64|, 2^-23 |host64|).

Device events around blocks of calls, the variants of a case alternating block by block, the median block of a variant (three
rounds by default) and the block-to-block spread. Writes profiles/rangeloss_bench.json (--out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from openpcseg_amd import rangeloss  # noqa: E402

SHAPES = ((30, 20, 64, 512), (12, 20, 64, 2048))
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
TERMS = ("total", "ce", "dice", "ls", "bd")


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


def make_input(shape, seed=5, block=(5, 23)):
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    logits = torch.from_numpy((rng.standard_normal(shape) * 3.0).astype(np.float32))
    blocks = rng.integers(0, c, size=(b, -(-h // block[0]), -(-w // block[1])))
    blocks[:, 0, 0] = 0
    labels = np.repeat(np.repeat(blocks, block[0], axis=1), block[1], axis=2)[:, :h, :w].astype(np.int64)
    return logits, torch.from_numpy(np.ascontiguousarray(labels))


def host_values(logits, labels, dtype):
    with torch.no_grad():
        total, terms = rangeloss.range_criterion_host(logits, labels, dtype=dtype)
    return [total.item()] + [t.item() for t in terms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="calls per block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rangeloss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rangeloss_bench: needs an MI355X (no CPU timing)")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        logits_host, labels_host = make_input(shape)
        for tag, dtype in DTYPES.items():
            stored = logits_host.to(dtype)
            h64, h32 = host_values(stored.float(), labels_host, torch.float64), host_values(stored.float(), labels_host, torch.float32)
            x = stored.to(dev).requires_grad_(True)
            labels = labels_host.to(dev)
            crit = rangeloss.RangeCriterion(shape[1]).to(dev)
            assert crit.uses_kernel(x)

            def native():
                x.grad = None
                crit(x, labels).backward()

            def composed():
                x.grad = None
                rangeloss.range_criterion_host(x, labels, dtype=torch.float32)[0].backward()

            loss = crit(x, labels)
            mine = [loss.item()] + crit.last_terms.tolist()
            total, terms = rangeloss.range_criterion_host(x, labels, dtype=torch.float32)
            theirs = [total.item()] + [t.item() for t in terms]
            ratios = {}
            for i, k in enumerate(TERMS):
                bound = 4.0 * max(abs(h32[i] - h64[i]), 2.0 ** -23 * abs(h64[i]))
                for who, v in (("range_criterion", mine[i]), ("torch_composition", theirs[i])):
                    assert abs(v - h64[i]) <= bound, (shape, tag, k, who, v, h64[i], h32[i])
                ratios[k] = round(abs(mine[i] - h64[i]) / bound, 4) if bound else 0.0
            del loss, total, terms
            med, spread = alternate({"range_criterion": native, "torch_composition": composed}, args.reps, args.rounds, args.warmup)
            row = {"case": "x".join(map(str, shape)) + "_" + tag, "ms": {k: round(v, 4) for k, v in med.items()},
                   "ms_min_max": {k: [round(a, 4), round(b, 4)] for k, (a, b) in spread.items()},
                   "speedup": round(med["torch_composition"] / med["range_criterion"], 3),
                   "difference_beyond_spread": bool(spread["range_criterion"][1] < spread["torch_composition"][0] or
                                                    spread["range_criterion"][0] > spread["torch_composition"][1]),
                   "values": dict(zip(TERMS, mine)), "value_error_over_bound": ratios, "equal_values_within_bound": True}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x, crit
            torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "reps_per_block": args.reps, "rounds": args.rounds,
           "method": "device events, alternating blocks, median block per variant; criterion forward + backward", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
