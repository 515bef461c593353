#!/usr/bin/env python3
"""Inference mode (`freeze`, the fold records, the prediction tail) on seeded small models: per model one line with the
SHA-256 of every record's folded tensors, of the frozen eval logits in fp32 and under bf16 autocast, and -- on a device -- of `predict`
with an evaluator and of `predict_tta` with 3 votes in chunks of 1 and 3. Two trees that compute the same bits print the same file.

  python tools/inference_sha.py > new.txt          # all lines, on the device
  python tools/inference_sha.py --cpu > new.txt    # the fold and fp32 frozen-forward fields on the pure-PyTorch backend

Uses public names only (freeze, `_pcs_folds`, predict, SegEvaluator, predict_tta), so it runs on any tree that has them."""
import argparse
import contextlib
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_POINTS = 2000


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = torch.as_tensor(t).detach().cpu().contiguous()
        h.update(str((tuple(t.shape), t.dtype)).encode())
        h.update(t.view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


def fold_sha(model):
    """Every record's folded tensors, modules in named_modules order, records in the order of their dict."""
    out = []
    for name, m in model.named_modules():
        rec = m.__dict__.get("_pcs_folds") or {}
        for key, v in rec.items():
            for f in (v if isinstance(v, list) else [v]):
                for attr in ("weight", "bias", "scale", "shift"):
                    t = getattr(f, attr, None)
                    if isinstance(t, torch.Tensor):
                        out.append(t)
    return "%d:%s" % (len(out), sha(*out))


def lidar_frames(seeds, in_dim):
    """Host batch of the reference's eval loader: lidar, targets_mapped, inverse_map, num_points (+ the range view for in_dim 4)."""
    from openpcseg_amd.hostdata import sparse_collate_fn, sparse_quantize
    from openpcseg_amd.sparse import SparseTensor
    from openpcseg_amd.workloads.synthetic import make_scan
    frames = []
    for s in seeds:
        pts = make_scan(s, N_POINTS - 87 * s)
        pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
        pc -= pc.min(0, keepdims=1)
        _, inds, inverse = sparse_quantize(pc, return_index=True, return_inverse=True)
        labels = np.random.default_rng(s).integers(0, 20, size=pts.shape[0]).astype(np.int64)
        frames.append({"lidar": SparseTensor(pts[inds], pc[inds]), "targets_mapped": SparseTensor(labels, pc),
                       "inverse_map": SparseTensor(np.asarray(inverse).astype(np.int64), pc), "num_points": np.array([pts.shape[0]])})
    return sparse_collate_fn(frames)


def with_range_view(batch):
    import fullsize as fs
    feats, frame = batch["lidar"].F, batch["lidar"].C[:, -1]
    imgs, pxpy = [], torch.zeros(feats.shape[0], 3)
    for i in range(int(frame.max()) + 1):
        img, pp = fs.range_view(feats[frame == i], h=64, w=512)
        pp[:, 0] = i
        imgs.append(img)
        pxpy[frame == i] = pp
    batch["range_image"], batch["range_pxpy"] = torch.cat(imgs, 0), pxpy
    return batch


def cylinder_frames():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "models_e2e_golden.npz"))
    keys = ["point_feature", "point_coord", "voxel_coord", "voxel_label", "point_label", "offset"]
    batch = {k: torch.from_numpy(np.ascontiguousarray(gold["cyl_" + k])) for k in keys}
    batch["num_points"] = np.array([batch["point_feature"].shape[0]])
    return batch


def to_device(batch, dev):
    from openpcseg_amd.sparse import SparseTensor
    out = {}
    for k, v in batch.items():
        if isinstance(v, SparseTensor):
            out[k] = SparseTensor(v.F.to(dev), v.C.int().to(dev).contiguous())
        else:
            out[k] = v.to(dev) if isinstance(v, torch.Tensor) and k != "num_points" else v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cpu", action="store_true", help="pure-PyTorch backend: the fold and frozen-forward lines only")
    args = ap.parse_args()
    import openpcseg_amd
    from openpcseg_amd import cpu_fallback
    from openpcseg_amd.inference import SegEvaluator, predict_tta
    from openpcseg_amd.workloads import minkunet as mk
    from openpcseg_amd.workloads.cylinder import CylinderTS
    from openpcseg_amd.workloads.rpvnet import RPVNet
    from openpcseg_amd.workloads.spvcnn import SPVCNN
    from openpcseg_amd.workloads.synthetic import make_raw_batch
    from seeded import seeded_state
    dev = torch.device("cpu" if args.cpu else "cuda:0")
    models = [
        ("MinkUNet mk18 cr0.5", lambda: mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5), lambda: lidar_frames([0, 1], 4)),
        ("SPVCNN mk18 cr0.5", lambda: SPVCNN(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5), lambda: lidar_frames([0, 1], 4)),
        ("RPVNet mk18 cr0.25", lambda: RPVNet(num_class=20, in_dim=4, num_layer=[2] * 8, cr=0.25), lambda: with_range_view(lidar_frames([0, 1], 4))),
        ("CylinderTS init 8", lambda: CylinderTS(num_class=20, in_dim=9, init_size=8), cylinder_frames),
    ]
    with (cpu_fallback.enabled() if args.cpu else contextlib.nullcontext()):
        for name, make, frames in models:
            model = make().eval()
            seeded_state(model)
            model.to(dev)
            host = frames()
            report = openpcseg_amd.freeze(model)
            fields = ["folded=%d skipped=%d" % (report["folded"], len(report["skipped"]))]
            for amp in ((False,) if args.cpu else (False, True)):   # the pure-PyTorch backend has no half path
                with torch.no_grad(), torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp):
                    out = model(to_device(host, dev))
                fields.append("%s=%s" % ("bf16" if amp else "fp32", sha(*[out[k].float() for k in ("logits", "point_logits") if k in out])))
                if not amp:
                    fields.insert(1, "folds=" + fold_sha(model))
            if not args.cpu:
                ev = SegEvaluator(20)
                out = model.predict(to_device(host, dev), evaluator=ev)
                fields.append("predict=%s" % sha(out["point_predict"], ev.hist, torch.tensor(out["point_offset"])))
                if callable(getattr(model, "point_logits", None)) and not isinstance(model.point_logits, torch.nn.Module) \
                        and "range_image" not in host:
                    raw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in make_raw_batch([1, 2], n_points=N_POINTS).items()}
                    for chunk in (1, 3):
                        ev = SegEvaluator(20)
                        out = predict_tta(model, raw, num_votes=3, evaluator=ev, vote_chunk=chunk, rng=np.random.RandomState(4))
                        fields.append("tta%d=%s" % (chunk, sha(out["pred"], out["votes"], ev.hist)))
            print("%-20s %s" % (name, " ".join(fields)))
    if not args.cpu:
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
