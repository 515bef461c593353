#!/usr/bin/env python3
"""The device input builders and the voted evaluations on two small unequal frames: per case one line with the
SHA-256 of every tensor or host array of the returned dict, in sorted key order (a SparseTensor as F then C, a list entry by entry).
Two trees that compute the same bits print the same file.

  python tools/input_sha.py > new.txt

The frames are make_scan(1, 200) and make_scan(2, 137); the cases are transform / cylinder / rangeview `device_batch`, `device_mix`,
the range-view scan (`rangescan.device_batch` with and without a label table, both masks), its `knn_vote` for every search window
and one `native.predict_points` with scenes, votes and a confusion matrix, and the three `predict_tta` on seeded small models with
3 votes in chunks of 1 and None. Uses public names only (`device_batch`, `device_mix`, `tta_params`, `knn_vote`, `predict_points`,
`predict_tta`, SegEvaluator), so it runs on any tree that has them."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((1, 200), (2, 137))   # (make_scan seed, rows)
C = 20
LO, HI, GRID = [0, -180, -4], [50, 180, 2], [120, 90, 16]
HW = (64, 512)
OMEGA = (0.7, 2.9)


def leaves(v):
    from openpcseg_amd.sparse import SparseTensor
    if isinstance(v, SparseTensor):
        return [v.F, v.C]
    if isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor):
        return list(v)
    return [v]


def sha(out):
    h = hashlib.sha256()
    for key in sorted(out):
        for t in leaves(out[key]):
            t = torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).detach().cpu().contiguous()
            h.update(str((key, tuple(t.shape), t.dtype)).encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return "%s keys=%s" % (h.hexdigest()[:16], ",".join(sorted(out)))


def make_raw(dev, shift=0, ring=False):
    from openpcseg_amd.workloads.synthetic import make_scan, scan_rings
    pts = [make_scan(s + shift, n) for s, n in SIZES]
    if ring:
        pts = [np.concatenate([p, scan_rings(p.shape[0])[:, None]], axis=1) for p in pts]
    labels = [np.random.default_rng(s + shift + 77).integers(0, C, size=p.shape[0]).astype(np.int64) for (s, _), p in zip(SIZES, pts)]
    return {"points": torch.from_numpy(np.ascontiguousarray(np.concatenate(pts), dtype=np.float32)).to(dev),
            "labels": torch.from_numpy(np.concatenate(labels)).to(dev), "num_frames": len(pts),
            "offsets": [0] + np.cumsum([p.shape[0] for p in pts]).tolist()}


def main():
    from openpcseg_amd import cylinder, native, rangescan, rangeview, scanmix, transform
    from openpcseg_amd.inference import SegEvaluator, predict_tta
    from openpcseg_amd.workloads import minkunet as mk
    from openpcseg_amd.workloads.cylinder import CylinderTS
    from openpcseg_amd.workloads.rpvnet import RPVNet
    from seeded import seeded_state
    dev = torch.device("cuda:0")
    raw, fusion = make_raw(dev), make_raw(dev, ring=True)
    nf = raw["num_frames"]

    def line(name, out):
        print("%-44s %s" % (name, sha(out)), flush=True)

    for v in (1, 3):
        params = transform.tta_params(nf, v, rng=np.random.RandomState(3))
        line("transform.device_batch votes=%d" % v, transform.device_batch(raw, 0.05, params, votes=v, eval_maps=True))
        for labels in (True, False):
            line("cylinder.device_batch votes=%d labels=%d" % (v, labels),
                 cylinder.device_batch(raw, LO, HI, GRID, C, params, votes=v, labels=labels))
    params, cuts = rangeview.tta_params(nf, 3, rng=np.random.RandomState(5))
    line("rangeview.device_batch votes=3", rangeview.device_batch(fusion, 0.05, params, cuts, votes=3, eval_maps=True, hw=HW))
    plan = np.array([[scanmix.POLARMIX, -1.0, 1, 1], [scanmix.LASERMIX, 1, 0, 0]], dtype=np.float64)
    for lasermix in ("reference", "radians"):
        line("scanmix.device_mix ring lasermix=%s" % lasermix,
             scanmix.device_mix(raw, make_raw(dev, shift=1000), plan, OMEGA, ring=True, lasermix=lasermix))
    # the range-view scan, its KNN vote and the prediction tail: seeded inputs, every confusion matrix counted in the launch
    lut = [(7 * i + 3) % C for i in range(C)]
    for table in (None, lut):
        for mask in ("reference", "hit"):
            view = rangescan.device_batch(raw, hw=HW, label_lut=table, mask=mask)
            line("rangescan.device_batch lut=%d mask=%s" % (table is not None, mask), view)
    gen = torch.Generator().manual_seed(11)
    argmax = torch.randint(0, C, tuple(view["scan_rv"][:, 4].shape), generator=gen).to(dev)
    for search in (3, 5, 7):
        hist = torch.zeros((C, C), dtype=torch.int64, device=dev)
        pred = rangescan.knn_vote(view["scan_rv"][:, 4] * 80, argmax, view["unproj_range"], view["proj_x"], view["proj_y"],
                                  view["point_offset"], knn=5, search=search, num_class=C, labels=raw["labels"], hist=hist)
        line("rangescan.knn_vote search=%d hist" % search, {"pred": pred, "hist": hist})
    rows = (50, 40)   # voxel rows of the two scenes
    logits = torch.randn((sum(rows), C), generator=gen).to(dev)
    inverse = torch.cat([torch.randint(0, r, (n,), generator=gen) for r, (_, n) in zip(rows, SIZES)]).to(dev)
    hist = torch.zeros((C, C), dtype=torch.int64, device=dev)
    votes = torch.zeros((inverse.numel(), C), dtype=torch.float32, device=dev)
    for _ in range(2):   # two passes summed into the votes
        pred, bad = native.predict_points(logits, inverse=inverse, point_offset=torch.tensor(raw["offsets"], device=dev),
                                          row_offset=torch.tensor([0, rows[0], sum(rows)], device=dev), labels=raw["labels"],
                                          votes=votes, hist=hist)
    line("native.predict_points scenes votes hist", {"pred": pred, "bad": bad, "votes": votes, "hist": hist})

    def seeded(model):
        model = model.eval()
        seeded_state(model)
        return model.to(dev)

    voted = [
        ("inference.predict_tta", seeded(mk.MinkUNet(num_class=C, num_layer=mk.MK18_LAYERS, cr=0.5)),
         lambda m, **kw: predict_tta(m, raw, voxel_size=0.05, **kw)),
        ("RPVNet.predict_tta", seeded(RPVNet(num_class=C, in_dim=5, num_layer=[2] * 8, cr=0.25)),
         lambda m, **kw: m.predict_tta(fusion, hw=HW, **kw)),
        ("CylinderTS.predict_tta", seeded(CylinderTS(num_class=C, init_size=8)),
         lambda m, **kw: m.predict_tta(raw, LO, HI, GRID, **kw)),
    ]
    for name, model, run in voted:
        for chunk in (1, None):
            for with_ev in (True, False):
                ev = SegEvaluator(C) if with_ev else None
                out = run(model, num_votes=3, evaluator=ev, vote_chunk=chunk, rng=np.random.RandomState(4), return_logits=True)
                if ev is not None:
                    out["evaluator_hist"], out["evaluator_bad"] = ev.hist, ev.bad
                line("%s chunk=%s evaluator=%d" % (name, chunk, with_ev), out)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
