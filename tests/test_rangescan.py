"""The range-view scan and its KNN vote on the device: csrc/rangescan.hip through rangescan.device_batch,
rangescan.knn_vote and rangescan.predict.

The yardsticks are rangescan.range_scan_host(atan="double") + input_host and knn_vote_host -- the reference's code restated in
NumPy, held to the reference's own output by tests/test_rangescan_host.py -- and the fixture itself (whose seed guards make
"double" and the reference's float32 functions agree bit for bit on it). Every comparison is EQUALITY."""
import numpy as np
import pytest
import torch

import rangescan_cases as rc
from openpcseg_amd import rangescan
from openpcseg_amd.inference import SegEvaluator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return rc.load_gold()


@pytest.fixture(autouse=True)
def _device(hip):
    """Every test here runs on the device (the session's backend fixture skips where there is none)."""


def raw_batch(frames, labels=True):
    """[(points, labels)] -> the raw batch on the device (the layout hostdata.raw_frames reads)."""
    raw = {"points": torch.from_numpy(np.concatenate([p for p, _ in frames]).astype(np.float32)).cuda(),
           "offsets": [0] + np.cumsum([p.shape[0] for p, _ in frames]).tolist(), "num_frames": len(frames)}
    if labels:
        raw["labels"] = torch.from_numpy(np.concatenate([l.astype(np.int64) for _, l in frames])).cuda()
    return raw


def host_batch(frames, hw, lut=None, mask="reference", labels=True):
    views = [rangescan.range_scan_host(p, l if labels else None, hw, atan="double", mask=mask) for p, l in frames]
    inputs = [rangescan.input_host(v, lut) for v in views]
    out = {"scan_rv": np.stack([i[0] for i in inputs]), "label_rv": np.stack([i[1] for i in inputs]), "mask_rv": np.stack([i[2] for i in inputs]),
           "proj_idx": np.stack([v["proj_idx"] for v in views])}
    out.update({k: np.concatenate([v[k] for v in views]) for k in ("proj_x", "proj_y", "unproj_range")})
    return out


def assert_batch_equal(got, want):
    for key, w in want.items():
        g = got[key].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, g.shape, w.dtype, w.shape)
        same = np.array_equal(g.view(np.uint32), w.view(np.uint32)) if w.dtype == np.float32 else np.array_equal(g, w)
        assert same, "%s: %d values differ" % (key, int((g != w).sum()))


# ---- a. the scan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lut", [True, False])
@pytest.mark.parametrize("hw", [(16, 64), (64, 512)])
def test_device_batch_equals_the_fixture_and_the_host(gold, hw, with_lut):
    frames, lut = rc.frames(gold), rc.lut(gold)
    out = rangescan.device_batch(raw_batch(frames), hw, label_lut=lut if with_lut else None)
    assert out["point_offset"] == [0, 3000, 5117] and "bad" not in out
    assert_batch_equal(out, host_batch(frames, hw, lut if with_lut else None))
    off = out["point_offset"]
    for i in range(2):
        pre = rc.prefix(i, hw)
        assert rc.crc(out["scan_rv"][i].cpu().numpy()) == gold[pre + "crc_scan"]
        assert rc.crc(out["mask_rv"][i].cpu().numpy()) == gold[pre + "crc_proj_mask"]
        assert rc.crc(out["proj_idx"][i].cpu().numpy()) == gold[pre + "crc_proj_idx"]
        label = out["label_rv"][i].cpu().numpy()
        if with_lut:
            assert rc.crc(label) == gold[pre + "crc_label"]
        else:
            assert rc.crc(label.astype(np.int32)) == gold[pre + "crc_proj_sem_label"]
        for key in ("proj_x", "proj_y", "unproj_range"):
            assert np.array_equal(out[key][off[i]:off[i + 1]].cpu().numpy(), gold[pre + key]), (pre, key)


def test_batch_without_labels_and_extra_columns(gold):
    frames = [(np.concatenate([p, np.full((p.shape[0], 2), 9.0, dtype=np.float32)], axis=1), l) for p, l in rc.frames(gold)]
    out = rangescan.device_batch(raw_batch(frames, labels=False), (16, 64), mask="hit")
    assert_batch_equal(out, host_batch(frames, (16, 64), mask="hit", labels=False))
    assert int(out["label_rv"].abs().sum()) == 0


def collision_frames():
    """Frame 0: one ray five times (equal depths at rows 1, 2, 4; the far ones at 0, 3) + a fan of heavy collisions; frame 1: the
    same ray reversed, so that row 0 is a winner; frame 2: one point."""
    rng = np.random.default_rng(5)
    ray = np.array([[10.0, 1.0, -1.0, 0.1], [5.0, 0.5, -0.5, 0.2], [5.0, 0.5, -0.5, 0.3], [10.0, 1.0, -1.0, 0.4], [5.0, 0.5, -0.5, 0.5]], dtype=np.float32)
    az, el, r = np.deg2rad(rng.uniform(40, 44, 900)), np.deg2rad(rng.uniform(-6, -4, 900)), rng.uniform(4, 40, 900)
    fan = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(0, 1, 900)], axis=1).astype(np.float32)
    fan[450:] = fan[:450]                                  # every fan point twice: equal depths everywhere
    labels = lambda n: rng.integers(0, 20, n).astype(np.int64) | (rng.integers(0, 50, n).astype(np.int64) << 16)
    return [(np.concatenate([ray, fan]), labels(905)), (ray[::-1].copy(), labels(5)), (ray[:1].copy(), labels(1))]


@pytest.mark.parametrize("mask", ["reference", "hit"])
def test_constructed_collisions(mask):
    frames = collision_frames()
    out = rangescan.device_batch(raw_batch(frames), (16, 64), mask=mask)
    want = host_batch(frames, (16, 64), mask=mask)
    assert_batch_equal(out, want)
    idx, m = out["proj_idx"].cpu().numpy(), out["mask_rv"].cpu().numpy()
    y, x = int(want["proj_y"][0]), int(want["proj_x"][0])
    assert idx[0, y, x] == 1 and idx[1, y, x] == 0 and idx[2, y, x] == 0          # the lowest index among the equally near
    assert m[0, y, x] == 1 and m[1, y, x] == m[2, y, x] == (1 if mask == "hit" else 0)  # point 0 as a winner under both rules
    assert (idx[0] >= 0).sum() < 200 and (idx[0][idx[0] >= 5] < 455).all()        # of every doubled fan point the first copy


def test_bad_rows_touch_nothing(gold):
    frames = [(p.copy(), l) for p, l in rc.frames(gold)]
    clean = rangescan.device_batch(raw_batch(frames), (16, 64), check=False)
    assert int(clean["bad"].item()) == 0
    bad_rows = {0: (17, [np.nan] * 4), 1: (5, [0.0, 0.0, 0.0, 0.5])}
    for f, (row, value) in bad_rows.items():
        frames[f][0][row] = value
    raw = raw_batch(frames)
    with pytest.raises(ValueError, match="not finite or has zero depth"):
        rangescan.device_batch(raw, (16, 64))
    out = rangescan.device_batch(raw, (16, 64), check=False)
    assert int(out["bad"].item()) == 1
    rows = [17, 3000 + 5]
    px, py = out["proj_x"].cpu().numpy(), out["proj_y"].cpu().numpy()
    assert (px[rows] == -1).all() and (py[rows] == -1).all()
    keep = np.ones(5117, dtype=bool)
    keep[rows] = False
    for key in ("proj_x", "proj_y", "unproj_range"):
        assert np.array_equal(out[key].cpu().numpy()[keep], clean[key].cpu().numpy()[keep]), key
    # the images are those of the scans WITHOUT the two rows, under the rows' original numbering
    for f, (row, _) in bad_rows.items():
        p, l = frames[f]
        sel = np.flatnonzero(np.arange(p.shape[0]) != row)
        view = rangescan.range_scan_host(p[sel], l[sel], (16, 64), atan="double")
        idx = view["proj_idx"].copy()
        idx[idx >= 0] = sel[idx[idx >= 0]]
        got = out["proj_idx"][f].cpu().numpy()
        assert np.array_equal(got, idx) and not (got == row).any()
        view["proj_idx"] = idx
        view["proj_mask"] = (idx > 0).astype(np.float32)
        assert np.array_equal(out["scan_rv"][f].cpu().numpy().view(np.uint32), rangescan.input_host(view)[0].view(np.uint32))


def test_row_without_a_pitch_is_a_bad_row(gold):
    """x = y = 0 and z * z in the subnormals: float32 z / depth exceeds 1 (1.0000026 at z = 1e-20), arcsin has no value. The host
    raises; the device flags the row and touches no pixel with it."""
    pts, labels = rc.frames(gold)[1]
    pts = pts[:200].copy()
    pts[3] = [0.0, 0.0, 1e-20, 0.5]
    with pytest.raises(ValueError, match="no pitch"):
        rangescan.range_scan_host(pts, labels[:200], (16, 64))
    out = rangescan.device_batch(raw_batch([(pts, labels[:200])]), (16, 64), check=False)
    assert int(out["bad"].item()) == 1 and int(out["proj_x"][3]) == -1 and int(out["proj_y"][3]) == -1
    sel = np.flatnonzero(np.arange(200) != 3)
    view = rangescan.range_scan_host(pts[sel], labels[:200][sel], (16, 64), atan="double")
    idx = view["proj_idx"].copy()
    idx[idx >= 0] = sel[idx[idx >= 0]]
    assert np.array_equal(out["proj_idx"][0].cpu().numpy(), idx)
    assert np.array_equal(out["proj_x"].cpu().numpy()[sel], view["proj_x"]) and np.array_equal(out["proj_y"].cpu().numpy()[sel], view["proj_y"])


# ---- b. the vote ---------------------------------------------------------------------------------------------------------------------
def device_vote(cases, labels=None, hist=None, **kw):
    """knn_vote on a list of one-scan case dicts as ONE batch."""
    cat = lambda key, dtype: torch.from_numpy(np.concatenate([np.asarray(c[key]).reshape(-1) for c in cases]).astype(dtype)).cuda()
    img = torch.from_numpy(np.stack([c["proj_range"] for c in cases]).astype(np.float32)).cuda()
    arg = torch.from_numpy(np.stack([c["proj_argmax"] for c in cases]).astype(np.int64)).cuda()
    off = [0] + np.cumsum([np.asarray(c["px"]).shape[0] for c in cases]).tolist()
    return rangescan.knn_vote(img, arg, cat("unproj_range", np.float32), cat("px", np.int32), cat("py", np.int32), off, labels=labels,
                              hist=hist, **kw)


def host_vote(cases, **kw):
    return np.concatenate([rangescan.knn_vote_host(c["proj_range"], c["proj_argmax"], c["unproj_range"], c["px"], c["py"], **kw) for c in cases])


def fixture_cases(gold, hw):
    return [dict(zip(("proj_range", "proj_argmax", "unproj_range", "px", "py"), rc.vote_inputs(gold, i, hw))) for i in range(2)]


@pytest.mark.parametrize("hw", [(16, 64), (64, 512)])
def test_vote_equals_the_fixture(gold, hw):
    got = device_vote(fixture_cases(gold, hw), knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=20).cpu().numpy()
    assert got.dtype == np.int64
    assert np.array_equal(got, np.concatenate([gold[rc.prefix(i, hw) + "vote"] for i in range(2)]))


@pytest.mark.parametrize("num_class", [3, 20])
@pytest.mark.parametrize("cutoff", [0.0, 1.0])
@pytest.mark.parametrize("search", [3, 5, 7])
def test_vote_equals_the_host_on_constructed_sets(search, cutoff, num_class):
    """Border points, windows of empty pixels, points that lost their pixel and near zero padding: four scans in one batch.
    The grid search x knn x cutoff x num_class runs over these four constructed sets only: the fixture's proj_argmax holds 20
    classes, which num_class = 3 refuses, so the fixture has its own test above at its own parameters."""
    cases = [rc.vote_case(kind, num_class, seed=search) for kind in rc.VOTE_KINDS]
    for knn in (1, 5, search * search):
        kw = dict(knn=knn, search=search, sigma=1.0, cutoff=cutoff, num_class=num_class)
        got, want = device_vote(cases, **kw).cpu().numpy(), host_vote(cases, **kw)
        assert np.array_equal(got, want), (kw, int((got != want).sum()))
        assert got.min() >= 1 and got.max() <= num_class - 1


def test_labels_that_are_no_class_vote_for_nothing():
    """proj_argmax values outside [0, num_class) -- also ones whose low 32 bits look like a class -- take their place among the knn
    nearest and vote for nothing, exactly as class 0 does there."""
    case = rc.vote_case("border", 20, seed=9)
    rng = np.random.default_rng(9)
    junk = rng.uniform(size=case["proj_argmax"].shape) < 0.3
    values = rng.choice(np.array([2 ** 32 + 3, -5, 20, 64, 2 ** 40 + 7, -(2 ** 32) + 2], dtype=np.int64), size=case["proj_argmax"].shape)
    dirty, clean = dict(case), dict(case)
    dirty["proj_argmax"] = np.where(junk, values, case["proj_argmax"])
    clean["proj_argmax"] = np.where(junk, 0, case["proj_argmax"])
    for cutoff in (0.0, 1.0):
        kw = dict(knn=5, search=5, sigma=1.0, cutoff=cutoff, num_class=20)
        assert np.array_equal(device_vote([dirty], **kw).cpu().numpy(), host_vote([clean], **kw))


def test_fused_histogram_and_bad_points(gold):
    cases = fixture_cases(gold, (16, 64))
    n = 5117
    rng = np.random.default_rng(3)
    labels = rng.integers(-2, 23, size=n)                     # some outside [0, 20): skipped
    cases[0]["px"] = cases[0]["px"].copy()
    cases[0]["px"][[0, 99]] = -1                              # the scan's bad rows: prediction 0, not counted
    hist = torch.zeros((20, 20), dtype=torch.int64, device="cuda")
    kw = dict(knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=20)
    pred = device_vote(cases, labels=torch.from_numpy(labels).cuda(), hist=hist, **kw).cpu().numpy()
    good = np.ones(n, dtype=bool)
    good[[0, 99]] = False
    host_cases = [dict(c) for c in cases]
    host_cases[0] = {k: (v[good[:3000]] if k in ("px", "py", "unproj_range") else v) for k, v in cases[0].items()}
    assert (pred[~good] == 0).all() and np.array_equal(pred[good], host_vote(host_cases, **kw))
    count = good & (labels >= 0) & (labels < 20)
    want = np.bincount(labels[count] * 20 + pred[count], minlength=400).reshape(20, 20)
    assert np.array_equal(hist.cpu().numpy(), want) and want.sum() < n
    again = device_vote(cases, labels=torch.from_numpy(labels).cuda(), hist=hist, **kw).cpu().numpy()   # accumulates; same prediction
    assert np.array_equal(again, pred) and np.array_equal(hist.cpu().numpy(), 2 * want)


def test_two_calls_give_identical_tensors(gold):
    raw = raw_batch(rc.frames(gold))
    a, b = (rangescan.device_batch(raw, (64, 512), label_lut=rc.lut(gold)) for _ in range(2))
    for key in ("scan_rv", "label_rv", "mask_rv", "proj_idx", "proj_x", "proj_y", "unproj_range"):
        assert torch.equal(a[key], b[key]), key
    votes = [device_vote(fixture_cases(gold, (64, 512)), knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=20) for _ in range(2)]
    assert torch.equal(votes[0], votes[1])


# ---- c. the evaluation pass ----------------------------------------------------------------------------------------------------------
def test_predict_equals_the_host_composition(gold):
    frames, lut, hw = rc.frames(gold), rc.lut(gold), (16, 64)
    torch.manual_seed(11)
    model = torch.nn.Sequential(torch.nn.Conv2d(6, 8, 3, stride=2, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 20, 1)).cuda().eval()
    evaluator = SegEvaluator(20)
    seen = []                                                                    # the device's own logits, as the model returned them
    hook = model.register_forward_hook(lambda module, args, output: seen.append(output.detach()))
    out = rangescan.predict(model, raw_batch(frames), evaluator, hw=hw, label_lut=lut)
    hook.remove()
    assert sorted(out) == ["point_offset", "pred"] and len(seen) == 1 and seen[0].shape == (2, 20, 8, 32)      # half resolution
    logits = torch.nn.functional.interpolate(seen[0], size=hw, mode="bilinear", align_corners=True).cpu().numpy()
    assert out["point_offset"] == [0, 3000, 5117] and evaluator.last_offsets == out["point_offset"]
    host = host_batch(frames, hw, lut)
    off = out["point_offset"]
    want = np.concatenate([rangescan.knn_vote_host(host["scan_rv"][i, 4] * np.float32(80.0), logits[i].argmax(0), host["unproj_range"][off[i]:off[i + 1]],
                                                   host["proj_x"][off[i]:off[i + 1]], host["proj_y"][off[i]:off[i + 1]], num_class=20) for i in range(2)])
    pred = out["pred"].cpu().numpy()
    assert np.array_equal(pred, want)
    point_labels = lut[np.concatenate([l.astype(np.int64) & 0xFFFF for _, l in frames])]
    assert np.array_equal(rangescan.point_labels(raw_batch(frames)["labels"], lut).cpu().numpy(), point_labels)
    assert np.array_equal(evaluator.hist.cpu().numpy(), np.bincount(point_labels * 20 + pred, minlength=400).reshape(20, 20))
    assert evaluator.hist.sum().item() == 5117                                   # once per point
    with pytest.raises(RuntimeError, match="eval"):
        rangescan.predict(model.train(), raw_batch(frames), hw=hw)
