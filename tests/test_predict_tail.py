"""Prediction tail of an evaluation pass: csrc/predict.hip (pcs_predict_points_f32), inference.SegEvaluator, MinkUNet.predict.

The yardstick is a NumPy restatement of the reference's per-scene loop
(R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:436-455) and of its scoring (R:infer.py:35-52 fast_hist, fast_hist_crop,
per_class_iu; R:train.py:459-465). Arg-max and the confusion matrix are integer results: compared exactly.
"""
import numpy as np
import pytest
import torch

from openpcseg_amd import native
from openpcseg_amd.inference import SegEvaluator, point_predict
from openpcseg_amd.sparse import SparseTensor


# ---- the reference, restated -------------------------------------------------------------------------------------------
def fast_hist(pred, label, n):
    k = (label >= 0) & (label < n)
    return np.bincount(n * label[k].astype(int) + pred[k], minlength=n ** 2)[:n ** 2].reshape(n, n)


def per_class_iu(hist):
    return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist) + 1e-9)


def fast_hist_crop(output, target, unique_label):
    hist = fast_hist(output.flatten(), target.flatten(), np.max(unique_label) + 2)
    hist = hist[unique_label + 1, :]
    return hist[:, unique_label + 1]


def reference_tail(scores, batch, softmax=False):
    """-> per-scene lists (point_predict or softmax rows, point_labels), as the reference's eval branch returns them."""
    lidar_b = batch["lidar"].C[:, -1].cpu().numpy()
    inv_b, inv = batch["inverse_map"].C[:, -1].cpu().numpy(), batch["inverse_map"].F.cpu().numpy()
    lab_b, lab = batch["targets_mapped"].C[:, -1].cpu().numpy(), batch["targets_mapped"].F.cpu().numpy()
    num_points = np.asarray(batch["num_points"]).reshape(-1)
    preds, labels = [], []
    for idx in range(int(inv_b.max()) + 1):
        rows = scores[lidar_b == idx][inv[inv_b == idx]]
        if softmax:
            e = np.exp(rows.astype(np.float64) - rows.astype(np.float64).max(1, keepdims=True))
            mapped = e / e.sum(1, keepdims=True)
        else:
            mapped = rows.argmax(1)
        preds.append(mapped[:num_points[idx]])
        labels.append(lab[lab_b == idx][:num_points[idx]])
    return preds, labels


def make_tail_batch(rng, c, voxels=(5000, 7000, 6000), points=(9000, 12000, 10000), cut=(0, 137, 0), device="cpu"):
    """Three scenes with their own inverse maps, labels that include -1, c and 255, one shortened num_points."""
    lidar_c, inv_f, inv_c, lab_f = [], [], [], []
    for b, (m, n) in enumerate(zip(voxels, points)):
        lidar_c.append(np.concatenate([rng.integers(0, 400, size=(m, 3)), np.full((m, 1), b)], 1))
        inv_f.append(rng.integers(0, m, size=n))
        inv_c.append(np.concatenate([rng.integers(0, 400, size=(n, 3)), np.full((n, 1), b)], 1))
        lab = rng.integers(0, c, size=n)
        lab[rng.random(n) < 0.05] = -1
        lab[rng.random(n) < 0.03] = c
        lab[rng.random(n) < 0.03] = 255
        lab_f.append(lab)
    ti = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int32)).to(device)
    tl = lambda a: torch.from_numpy(np.concatenate(a).astype(np.int64)).to(device)
    coords_p = ti(inv_c)
    return {"lidar": SparseTensor(torch.zeros(sum(voxels), 4, device=device), ti(lidar_c)),
            "inverse_map": SparseTensor(tl(inv_f), coords_p), "targets_mapped": SparseTensor(tl(lab_f), coords_p),
            "num_points": np.array([[n - k] for n, k in zip(points, cut)])}


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_evaluator_compute_arithmetic():
    """compute() from a hand-made full histogram = fast_hist_crop + per_class_iu + nanmean of the reference."""
    rng = np.random.default_rng(4)
    c = 20
    label = rng.integers(-1, c + 1, size=50000)
    label[:100] = 255
    pred = np.where(rng.random(50000) < 0.7, np.clip(label, 0, c - 1), rng.integers(0, c, size=50000))
    pred[label == 7] = 3     # a class that is never predicted where it occurs
    full = fast_hist(pred, label, c)
    for unique in (np.arange(c - 1), np.array([0, 2, 5, 18])):
        ev = SegEvaluator(c, unique_label=unique)
        ev.hist, ev.bad = torch.from_numpy(full.astype(np.int64)), torch.zeros(1, dtype=torch.int32)
        hist, iou, miou = ev.compute()
        want = fast_hist_crop(pred, label, unique)
        assert np.array_equal(hist, want)
        assert np.array_equal(iou, per_class_iu(want)) and miou == float(np.nanmean(per_class_iu(want)))
    assert iou.shape == (4,) and SegEvaluator(c).unique_label.tolist() == list(range(c - 1))
    other = SegEvaluator(c)
    other.hist, other.bad = torch.from_numpy(full.astype(np.int64)), torch.zeros(1, dtype=torch.int32)
    assert np.array_equal(ev.merge(other).hist.numpy(), 2 * full)
    with pytest.raises(ValueError):
        SegEvaluator(c, unique_label=np.arange(c))


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", [20, 19])
def test_tail_argmax_and_histogram_exact(hip, c):
    """No-vote mode on logits N(0, 3^2) quantised to 1/4 (ties occur): pred and hist EXACTLY the reference loop's; hist adds up
    over two updates; two runs are bit-identical."""
    rng = np.random.default_rng(c)
    batch = make_tail_batch(rng, c, device="cuda")
    m = batch["lidar"].C.shape[0]
    logits = np.round(rng.normal(0, 3, size=(m, c)) * 4) / 4
    assert (np.sort(logits, 1)[:, -1] == np.sort(logits, 1)[:, -2]).mean() > 0.01   # ties at the top do occur
    preds, labels = reference_tail(logits.astype(np.float32), batch)
    want_pred = np.concatenate(preds)
    want_hist = sum(fast_hist(p, l, c) for p, l in zip(preds, labels))
    dl = torch.from_numpy(logits.astype(np.float32)).cuda()
    ev = SegEvaluator(c)
    pred = ev.update(dl, batch)
    assert ev.last_offsets == [0] + np.cumsum([p.shape[0] for p in preds]).tolist()
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), want_pred)
    assert np.array_equal(ev.hist.cpu().numpy(), want_hist) and int(ev.bad) == 0
    ev.update(dl, batch)
    assert np.array_equal(ev.hist.cpu().numpy(), 2 * want_hist)
    ev2 = SegEvaluator(c)
    pred2 = ev2.update(dl, batch)
    ev2.update(dl, batch)
    assert torch.equal(pred2, pred) and torch.equal(ev2.hist, ev.hist)
    hist, iou, miou = ev.compute()
    unique = np.arange(c - 1)
    want = sum(fast_hist_crop(p, l, unique) for p, l in zip(preds, labels)) * 2
    assert np.array_equal(hist, want) and miou == float(np.nanmean(per_class_iu(want)))
    # without shortening (every scene keeps its points) and without labels: the prediction alone
    batch["num_points"] = np.array([[9000], [12000], [10000]])
    del batch["targets_mapped"]
    full, offsets, bad = point_predict(dl, batch)
    inv_b = batch["inverse_map"].C[:, -1].cpu().numpy()
    lidar_b = batch["lidar"].C[:, -1].cpu().numpy()
    want_full = np.concatenate([logits[lidar_b == b][batch["inverse_map"].F.cpu().numpy()[inv_b == b]].argmax(1) for b in range(3)])
    assert np.array_equal(full.cpu().numpy(), want_full) and offsets == [0, 9000, 21000, 31000] and int(bad) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [2, 4])
def test_tail_softmax_votes(hip, passes):
    """Vote mode on unquantised N(0, 3^2) logits, c = 20: votes within passes * 1e-6 of float64 (per pass: exp, sum, divide
    <= ~4 ulp of a value <= 1, plus half an ulp of a running sum <= 4: < 5e-7; twice that as the margin); pred equal wherever the
    float64 top-2 gap is >= 1e-5 (twice the 4-pass bound on each of the two competing sums); the left-out share <= 1e-3."""
    c = 20
    rng = np.random.default_rng(40 + passes)
    batch = make_tail_batch(rng, c, device="cuda")
    m = batch["lidar"].C.shape[0]
    n_kept = int(np.asarray(batch["num_points"]).sum())
    votes = torch.zeros(n_kept, c, device="cuda")
    ref = np.zeros((n_kept, c))
    ev = SegEvaluator(c)
    for _ in range(passes):
        logits = rng.normal(0, 3, size=(m, c)).astype(np.float32)
        pred = ev.update(torch.from_numpy(logits).cuda(), batch, votes=votes)
        ref += np.concatenate(reference_tail(logits, batch, softmax=True)[0])
    err = float(np.abs(votes.cpu().numpy().astype(np.float64) - ref).max())
    print("votes: max abs error %.3e over %d passes" % (err, passes))
    assert err <= passes * 1e-6, err
    top2 = np.sort(ref, 1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] >= 1e-5
    print("left-out share %.3e" % (1.0 - clear.mean()))
    assert 1.0 - clear.mean() <= 1e-3
    assert np.array_equal(pred.cpu().numpy()[clear], ref.argmax(1)[clear])
    assert int(ev.bad) == 0


@pytest.mark.gpu
def test_tail_refuses_rows_outside_their_scene(hip):
    """Input validation: an inverse index that is negative or >= its scene's row count sets bad_flag, gives pred = -1 and is not
    counted; every other point is unaffected. Also the single-scene forms (n_scenes = 0, with and without an inverse map)."""
    c = 20
    rng = np.random.default_rng(9)
    voxels, points = (3000, 2000, 4000), (5000, 5000, 5000)
    m, n = sum(voxels), sum(points)
    logits = torch.from_numpy((np.round(rng.normal(0, 3, size=(m, c)) * 4) / 4).astype(np.float32)).cuda()
    inv = np.concatenate([rng.integers(0, v, size=p) for v, p in zip(voxels, points)])
    labels = rng.integers(0, c, size=n)
    scene = np.repeat(np.arange(3), points)
    row0 = np.concatenate([[0], np.cumsum(voxels)])
    bad_at = np.array([3, 4999, 5000, 7777, 14999])
    inv[bad_at] = [-1, 3000, 2000, -(2 ** 40), 2 ** 40]   # scene 0 has 3000 rows, scene 1 2000 (row 2000 exists, in scene 2), scene 2 4000
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()
    hist = torch.zeros(c, c, dtype=torch.int64, device="cuda")
    pred, bad = hip.predict_points(logits, inverse=dev(inv), point_offset=dev(np.concatenate([[0], np.cumsum(points)])),
                                   row_offset=dev(row0), labels=dev(labels), hist=hist)
    ok = np.ones(n, dtype=bool)
    ok[bad_at] = False
    want = np.full(n, -1)
    want[ok] = logits.cpu().numpy()[row0[scene[ok]] + inv[ok]].argmax(1)
    assert int(bad) == 1 and np.array_equal(pred.cpu().numpy(), want)
    assert np.array_equal(hist.cpu().numpy(), fast_hist(want[ok], labels[ok], c)) and int(hist.sum()) == n - 5
    # one scene spanning everything
    flat = rng.integers(0, m, size=n)
    pred, bad = hip.predict_points(logits, inverse=dev(flat))
    assert int(bad) == 0 and np.array_equal(pred.cpu().numpy(), logits.cpu().numpy()[flat].argmax(1))
    assert torch.equal(pred, hip.rows_argmax_gather(logits, dev(flat)))
    pred, bad = hip.predict_points(logits)
    assert int(bad) == 0 and np.array_equal(pred.cpu().numpy(), logits.cpu().numpy().argmax(1))
    with pytest.raises(RuntimeError):
        hip.predict_points(torch.zeros(8, 65, device="cuda"))   # c <= 64
    assert native.predict_points(logits)[0].shape == (m,)


@pytest.mark.gpu
def test_minkunet_predict_three_scans(hip):
    """MinkUNet.predict on a three-scan batch: point_predict = the reference-style loop applied to the same logits; the
    evaluator's mIoU = the NumPy restatement. Frozen and unfrozen."""
    import openpcseg_amd
    from openpcseg_amd.hostdata import sparse_collate_fn, sparse_quantize
    from openpcseg_amd.workloads import minkunet as mk
    from openpcseg_amd.workloads.synthetic import make_scan
    from seeded import seeded_state
    frames = []
    for seed, n in ((1, 12000), (2, 20000), (3, 16000)):
        pts = make_scan(seed, n)
        pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
        pc -= pc.min(0, keepdims=1)
        _, inds, inverse = sparse_quantize(pc, return_index=True, return_inverse=True)
        labels = np.random.default_rng(seed).integers(0, 20, size=pts.shape[0]).astype(np.int64)
        frames.append({"lidar": SparseTensor(pts[inds], pc[inds]), "targets_mapped": SparseTensor(labels, pc),
                       "inverse_map": SparseTensor(np.asarray(inverse).astype(np.int64), pc), "num_points": np.array([pts.shape[0]])})
    host = sparse_collate_fn(frames)
    model = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5).cuda().eval()
    seeded_state(model)
    for frozen in (False, True):
        if frozen:
            openpcseg_amd.freeze(model)
        batch = {k: (SparseTensor(v.F.cuda(), v.C.int().cuda()) if isinstance(v, SparseTensor) else v) for k, v in host.items()}
        ev = SegEvaluator(20)
        out = model.predict(batch, evaluator=ev)
        logits = out["logits"].cpu().numpy()
        preds, labels = reference_tail(logits, batch)
        assert np.array_equal(out["point_predict"].cpu().numpy(), np.concatenate(preds))
        assert out["point_offset"] == [0, 12000, 32000, 48000]
        hist, iou, miou = ev.compute()
        want = sum(fast_hist_crop(p, l, np.arange(19)) for p, l in zip(preds, labels))
        assert np.array_equal(hist, want) and miou == float(np.nanmean(per_class_iu(want)))
        batch2 = {k: (SparseTensor(v.F.cuda(), v.C.int().cuda()) if isinstance(v, SparseTensor) else v) for k, v in host.items()}
        plain = model.predict(batch2)
        assert torch.equal(plain["point_predict"], out["point_predict"])
    model.train()
    with pytest.raises(RuntimeError):
        model.predict(batch)
