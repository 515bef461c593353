"""The cylinder dataset's batch on the device: csrc/cylscan.hip, cylinder.device_batch, CylinderTS.predict_tta.

  * device against device, exact: every tensor equals what the per-frame path (scan_transform's augmented rows -> cylinder_sample ->
    cylinder_batch) gives, for every vote-bound instance, row width, store form and a points base off 16 bytes;
  * nothing outside the votes * n output rows is written (guard rows around the raw C entry's buffers);
  * against the reference's own dataset (tests/golden/cylinder_batch_golden.npz): integers bit-exact, floats to 1e-6 max(1, max|ref|)
    -- the tolerance of tests/test_cylinder_frontend.py -- with that file's one allowance: NumPy takes arctan2 from the host libm
    and the kernel rounds a double atan2 once, so a point whose angle lies within one float32 ulp of a cell face may fall into the
    neighbouring cell; such rows must be face cases and at most max(1, 1e-4 rows) per scene;
  * the voted evaluation: votes within num_votes * 1e-6 of the float64 softmax sum of the logits the call itself used (the bound and
    derivation of tests/test_predict_tta.py), the decision, the evaluator's counts, the one-vote identity against predict."""
import ctypes
import os

import numpy as np
import pytest
import torch

from openpcseg_amd import transform
from openpcseg_amd.inference import SegEvaluator
from oracle import oracle as orc
from seeded import seeded_state
from transform_cases import raw_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LO, HI, GRID = [0, -180, -4], [50, 180, 2], [120, 90, 16]
C = 20
TENSORS = ("point_feature", "point_coord", "point_label", "voxel_feature", "voxel_coord", "voxel_label", "inverse_map")


def _cuda(raw):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}


def _frames(sizes, c, seed=0):
    """Frames of the given sizes with c columns: xyz (+ intensity) from make_scan, further columns random."""
    from openpcseg_amd.workloads.synthetic import make_scan
    out = []
    for k, n in enumerate(sizes):
        scan = make_scan(seed + k, max(n, 64))[:n].astype(np.float32)
        extra = np.random.default_rng(seed + 50 + k).random((n, max(c - 4, 0)), dtype=np.float32)
        out.append(np.ascontiguousarray(np.concatenate([scan, extra], axis=1)[:, :c]))
    return out


def _per_frame_batch(hip, raw, params, votes):
    """The parent's path: the augmented rows of scan_transform, cylinder_sample per (vote, frame), cylinder_batch."""
    from openpcseg_amd import cylinder
    from openpcseg_amd.workloads.cylinder import cylinder_batch
    off, n = raw["offsets"], raw["points"].shape[0]
    feats = hip.scan_transform(raw["points"], off, params, votes, 0.05)[0]
    samples = []
    for v in range(votes):
        for f in range(raw["num_frames"]):
            s = cylinder.cylinder_sample(feats[v * n + off[f]:v * n + off[f + 1]].contiguous(), raw["labels"][off[f]:off[f + 1]], LO, HI, GRID, C)
            samples.append(s)
    batch = cylinder_batch(samples)
    batch["voxel_feature"] = torch.cat([s["voxel_feature"] for s in samples])
    return batch


def _assert_same_batch(got, want, what):
    for k in TENSORS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (what, k)
    assert got["offset"].dtype == torch.int32 and torch.equal(got["offset"].cpu(), want["offset"]), what
    assert np.array_equal(got["num_points"], want["num_points"]), what


@pytest.fixture()
def store_form(hip):
    yield hip.lib.pcs_debug_cylscan_store
    hip.lib.pcs_debug_cylscan_store(-1)


@pytest.mark.parametrize("c", [3, 4, 5, 8])
@pytest.mark.parametrize("votes", [1, 3, 10, 16])
def test_device_batch_equals_the_per_frame_path(hip, store_form, votes, c):
    """(512, 301): n = 813 is odd, so the staged range starts on another 16-byte phase for every vote; (1, 257, 256): a one-row
    frame, one row past a workgroup, exactly one workgroup. 3 votes run the 4-bound instance with a partial loop."""
    from openpcseg_amd import cylinder
    for sizes in ((512, 301), (1, 257, 256)):
        raw = _cuda(raw_of(_frames(sizes, c, seed=votes), labels_seed=votes, num_classes=C))
        params = transform.draw_train_params(votes * len(sizes), rng=np.random.RandomState(10 * votes + c), scale_range=(0.95, 1.05))
        want = _per_frame_batch(hip, raw, params, votes)
        for form in (0, 1, 2):   # staged, row per lane, staged features with direct cells: equal bits
            store_form(form)
            got = cylinder.device_batch(raw, LO, HI, GRID, C, params, votes=votes)
            _assert_same_batch(got, want, (sizes, form))


def test_points_base_off_sixteen_bytes(hip, store_form):
    """c = 4 with the base 4 bytes past a 16-byte boundary: the scalar row loads."""
    from openpcseg_amd import cylinder
    host = raw_of(_frames((512, 301), 4, seed=5), labels_seed=5, num_classes=C)
    raw = _cuda(host)
    flat = torch.empty(raw["points"].numel() + 1, dtype=torch.float32, device="cuda")
    flat[1:] = raw["points"].reshape(-1)
    shifted = dict(raw, points=flat[1:].view(-1, 4))
    assert shifted["points"].data_ptr() % 16 == 4 and shifted["points"].is_contiguous()
    params = transform.tta_params(2, 10, scale_range=(0.95, 1.05), rng=np.random.RandomState(3))
    for form in (0, 1):
        store_form(form)
        a = cylinder.device_batch(raw, LO, HI, GRID, C, params, votes=10)
        b = cylinder.device_batch(shifted, LO, HI, GRID, C, params, votes=10)
        _assert_same_batch(b, {k: (v.cpu() if k == "offset" else v) for k, v in a.items()}, form)


@pytest.mark.parametrize("c,votes", [(4, 1), (4, 10), (5, 3), (3, 16)])
def test_nothing_outside_the_outputs_is_written(hip, store_form, c, votes):
    """The raw C entry into buffers with NaN / -1 guard rows before and after; frame boundaries outside [0, n] are clamped, an empty
    frame in the middle writes nothing and the rows of the other frames are those of the binding."""
    sizes = (300, 213)
    n, fdim, guard = sum(sizes), 8 + c - 3, 3   # 3 guard rows of 36 bytes: the output base is off 16 bytes at c = 4
    pts = torch.from_numpy(np.concatenate(_frames(sizes, c, seed=7))).cuda()
    params = transform.draw_train_params(votes * 3, rng=np.random.RandomState(votes), scale_range=(0.95, 1.05))
    # three frames: [clamped from -5, 300), an empty one, [300, clamped from n + 9)
    offsets = torch.tensor([-5, 300, 300, n + 9], dtype=torch.int64, device="cuda")
    par = torch.from_numpy(params).cuda()
    lo, hi, grid = (ctypes.c_double * 3)(*LO), (ctypes.c_double * 3)(*HI), (ctypes.c_int32 * 3)(*GRID)
    from openpcseg_amd.native import _stream
    results = []
    for form in (0, 1, 2):
        store_form(form)
        feat = torch.full((votes * n + 2 * guard, fdim), float("nan"), device="cuda")
        coord = torch.full((votes * n + 2 * guard, 3), -1, dtype=torch.int32, device="cuda")
        scenes = torch.full((votes * n + 2 * guard,), -1, dtype=torch.int64, device="cuda")
        rc = hip.lib.pcs_cylinder_scan_batch_f32(pts.data_ptr(), n, c, offsets.data_ptr(), 3, par.data_ptr(), votes, lo, hi, grid,
                                                 feat[guard:].data_ptr(), coord[guard:].data_ptr(), scenes[guard:].data_ptr(), _stream())
        assert rc == 0, hip.lib.pcs_last_error()
        torch.cuda.synchronize()
        for t, empty in ((feat, None), (coord, -1), (scenes, -1)):
            for g in (t[:guard], t[-guard:]):
                assert bool(torch.isnan(g).all()) if empty is None else bool((g == empty).all())
        inner = (feat[guard:-guard], coord[guard:-guard], scenes[guard:-guard])
        assert not bool(torch.isnan(inner[0]).any()) and bool((inner[1] >= 0).all())
        assert torch.equal(inner[2].view(votes, n), (torch.arange(votes, device="cuda") * 3)[:, None] + torch.tensor([0] * 300 + [2] * 213, device="cuda"))
        results.append(inner)
    for other in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(results[0], other))
    # the same rows through the binding: two frames, the parameter rows of frames 0 and 2
    store_form(-1)
    keep = np.array([[v * 3 + 0, v * 3 + 2] for v in range(votes)]).reshape(-1)
    f2, c2, s2 = hip.cylinder_scan_batch(pts, [0, 300, n], params[keep], votes, LO, HI, GRID)
    assert torch.equal(f2, results[0][0]) and torch.equal(c2, results[0][1])


# ---- against the reference's dataset ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "cylinder_batch_golden.npz"))


def _int(a):
    return int(np.asarray(a).reshape(-1)[0])


def _face_case(pts, lo, hi, grid, coord_ref, coord_dev, rows):
    """Every row where the device cell differs from NumPy's must differ by one cell along phi only, with the angle within 2 float32
    ulp of the face between the two cells (tests/test_cylinder_frontend.py's rule, restated)."""
    pol = orc.cylinder_partition(pts, lo, hi, grid)[0]
    interval = (hi[1] - lo[1]) / (grid[1] - 1)
    for r in rows:
        d = coord_dev[r].astype(np.int64) - coord_ref[r].astype(np.int64)
        assert d[0] == 0 and d[2] == 0 and abs(d[1]) == 1, (r, d)
        face = lo[1] + max(coord_dev[r][1], coord_ref[r][1]) * interval
        assert abs(float(pol[r, 1]) - face) <= 2 * np.spacing(np.float32(abs(face))), (r, pol[r, 1], face)


def _against_fixture(gold, prefix, got, scans, rows):
    """got: cylinder.device_batch's dict; scans / rows: per scene the raw frame and its parameter row (for the face-case check)."""
    coord, ref_coord = got["point_coord"].cpu().numpy(), gold[prefix + "point_coord"].T.astype(np.float32)
    assert coord.shape == ref_coord.shape and np.array_equal(coord[:, 3], ref_coord[:, 3])
    differs = (coord != ref_coord).any(axis=1)
    sizes = gold[prefix + "num_points"].reshape(-1).tolist()
    start = 0
    for s, n in enumerate(sizes):
        rows_s = np.nonzero(differs[start:start + n])[0]
        assert rows_s.size <= max(1, int(1e-4 * n)), (s, rows_s.size)
        if rows_s.size:
            aug = transform.transform_scan_host(scans[s], rows[s], 0.05)[0]
            _face_case(aug, LO, HI, GRID, ref_coord[start:start + n, :3], coord[start:start + n, :3], rows_s)
        start += n
    ref_feat = gold[prefix + "point_feature"].T
    tol = 1e-6 * max(1.0, float(np.abs(ref_feat).max()))
    feat = got["point_feature"].cpu().numpy()
    err = float(np.abs(feat[~differs] - ref_feat[~differs]).max())
    print("%s point_feature: max abs error %.3e (bound %.1e), %d rows in a neighbouring cell" % (prefix, err, tol, int(differs.sum())))
    assert err <= tol
    assert np.array_equal(got["point_label"].cpu().numpy(), gold[prefix + "point_label"].astype(np.int64))
    assert np.array_equal(got["num_points"], np.asarray(sizes))
    if not differs.any():   # the voxel set, its order, labels, inverse map and offsets: bit-exact
        for k in ("voxel_coord", "voxel_label", "inverse_map", "offset"):
            assert np.array_equal(got[k].cpu().numpy().astype(np.int64), gold[prefix + k].T.astype(np.int64)), k
        vf = got["voxel_feature"].cpu().numpy()
        assert float(np.abs(vf - gold[prefix + "voxel_feature"].T).max()) <= tol


def _fixture_frames(gold):
    t = np.load(os.path.join(HERE, "golden", "transform_golden.npz"))
    return [t["frame0"].astype(np.float32), t["frame1"].astype(np.float32)], [gold["labels_f0"].astype(np.int64), gold["labels_f1"].astype(np.int64)]


def _raw(frames, labels):
    sizes = [f.shape[0] for f in frames]
    return {"points": torch.from_numpy(np.concatenate(frames)).cuda(), "labels": torch.from_numpy(np.concatenate(labels)).cuda(),
            "num_frames": len(frames), "offsets": [0] + np.cumsum(sizes).tolist()}


def test_training_batch_against_the_reference(hip, gold):
    from openpcseg_amd import cylinder
    frames, labels = _fixture_frames(gold)
    np.random.seed(_int(gold["train_seed"]))
    params = transform.draw_train_params(2, scale_range=tuple(gold["scale_range"]))
    got = cylinder.device_batch(_raw(frames, labels), LO, HI, GRID, _int(gold["num_classes"]), params)
    _against_fixture(gold, "train_", got, frames, params)


def test_tta_batches_against_the_reference(hip, gold):
    """collate_batch_tta holds the ten votes of ONE frame: frame f alone as a raw batch, its ten parameter rows."""
    from openpcseg_amd import cylinder
    frames, labels = _fixture_frames(gold)
    np.random.seed(_int(gold["tta_seed"]))
    params = transform.tta_params(2, 10, scale_range=tuple(gold["scale_range"]))
    for f in range(2):
        mine = params[[v * 2 + f for v in range(10)]]
        got = cylinder.device_batch(_raw([frames[f]], [labels[f]]), LO, HI, GRID, _int(gold["num_classes"]), mine, votes=10)
        _against_fixture(gold, "tta%d_" % f, got, [frames[f]] * 10, mine)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    from openpcseg_amd import cylinder
    host = raw_of(_frames((200, 100), 4, seed=1), labels_seed=1, num_classes=C)
    raw = _cuda(host)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        cylinder.device_batch(host, LO, HI, GRID)
    with pytest.raises(ValueError, match="empty frame"):
        cylinder.device_batch(dict(raw, offsets=[0, 300, 300], num_frames=2), LO, HI, GRID)
    with pytest.raises(ValueError):
        cylinder.device_batch(dict(raw, offsets=[0, 200, 299]), LO, HI, GRID)
    with pytest.raises(RuntimeError, match="grid must be >= 2"):
        cylinder.device_batch(raw, LO, HI, [120, 1, 16])
    with pytest.raises(RuntimeError, match="bad args"):
        hip.cylinder_scan_batch(raw["points"], raw["offsets"], transform.identity_params(34), 17, LO, HI, GRID)
    with pytest.raises(RuntimeError, match="bad args"):
        hip.cylinder_scan_batch(torch.zeros((8, 9), device="cuda"), [0, 8], transform.identity_params(1), 1, LO, HI, GRID)
    bad = dict(raw, labels=torch.full_like(raw["labels"], 25))
    with pytest.raises(IndexError):
        cylinder.device_batch(bad, LO, HI, GRID, C)
    out = cylinder.device_batch(bad, LO, HI, GRID, C, check=False)
    assert int(out["bad"].item()) == 1
    assert int(cylinder.device_batch(raw, LO, HI, GRID, C, check=False)["bad"].item()) == 0
    assert "voxel_label" not in cylinder.device_batch(raw, LO, HI, GRID, C, labels=False)


# ---- voted evaluation ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from openpcseg_amd.workloads.cylinder import CylinderTS
    m = CylinderTS(num_class=C, init_size=8).cuda().eval()
    seeded_state(m)
    return m


@pytest.fixture(scope="module")
def eval_raw():
    from openpcseg_amd.workloads.synthetic import make_scan
    return raw_of([make_scan(1, 2000), make_scan(2, 1913)], labels_seed=9, num_classes=C)


def _keys(coords):
    """One int64 per (cell, scene) row -- the host-built hash of the mapping."""
    c = coords.astype(np.int64)
    return ((c[:, 3] * GRID[0] + c[:, 0]) * GRID[1] + c[:, 1]) * GRID[2] + c[:, 2]


def _float64_votes(raw, out, num_votes):
    """Sum over the votes of softmax(logits row of the point's voxel) in float64: the rows are found on the host, by the cells of
    the points (the kernel's own, recomputed for all votes at once) in the cells of the logits the call handed back."""
    from openpcseg_amd import cylinder
    n = raw["offsets"][-1]
    pc = cylinder.device_batch(_cuda(raw), LO, HI, GRID, C, out["params"], votes=num_votes, labels=False)["point_coord"].cpu().numpy()
    ref = np.zeros((n, C))
    assert len(out["logits"]) == len(out["logit_coords"]) == num_votes
    for v, (lg, lc) in enumerate(zip(out["logits"], out["logit_coords"])):
        lg, lk = lg.cpu().numpy().astype(np.float64), _keys(lc.cpu().numpy())
        order = np.argsort(lk)
        pk = _keys(pc[v * n:(v + 1) * n])
        pos = np.searchsorted(lk[order], pk)
        assert np.array_equal(lk[order][pos], pk)   # every point's cell is a row of this vote's logits
        rows = lg[order[pos]]
        e = np.exp(rows - rows.max(1, keepdims=True))
        ref += e / e.sum(1, keepdims=True)
    return ref


def _check_votes(raw, out, num_votes, evaluator):
    n = raw["offsets"][-1]
    votes = out["votes"].cpu().numpy()
    assert votes.shape == (n, C) and votes.dtype == np.float32
    err = float(np.abs(votes.astype(np.float64) - _float64_votes(raw, out, num_votes)).max())
    print("votes: max abs error %.3e over %d votes (bound %.1e)" % (err, num_votes, num_votes * 1e-6))
    assert err <= num_votes * 1e-6, err
    pred = out["pred"].cpu().numpy()
    assert pred.dtype == np.int64 and np.array_equal(pred, votes.argmax(1))
    assert out["point_offset"] == raw["offsets"] and out["params"].shape == (2 * num_votes, 8)
    hist = evaluator.hist.cpu().numpy()
    assert int(hist.sum()) == n   # every label is in [0, C): counted once, not once per vote
    assert np.array_equal(hist, np.bincount(C * raw["labels"].numpy() + pred, minlength=C * C).reshape(C, C)) and int(evaluator.bad) == 0


@pytest.mark.parametrize("vote_chunk", [None, 1, 4])
@pytest.mark.parametrize("num_votes", [1, 3, 10])
def test_voted_evaluation(model, eval_raw, num_votes, vote_chunk):
    ev = SegEvaluator(C)
    out = model.predict_tta(_cuda(eval_raw), LO, HI, GRID, num_votes=num_votes, evaluator=ev, vote_chunk=vote_chunk,
                            rng=np.random.RandomState(num_votes), return_logits=True)
    _check_votes(eval_raw, out, num_votes, ev)
    plain = model.predict_tta(_cuda(eval_raw), LO, HI, GRID, num_votes=num_votes, vote_chunk=vote_chunk, rng=np.random.RandomState(num_votes))
    assert "logits" not in plain and torch.equal(plain["pred"], out["pred"]) and torch.equal(plain["votes"], out["votes"])


def test_one_identity_vote_is_predict(model, eval_raw):
    from openpcseg_amd import cylinder
    raw = _cuda(eval_raw)
    out = model.predict_tta(raw, LO, HI, GRID, num_votes=1, scale_range=(1.0, 1.0))
    assert np.array_equal(out["params"], transform.identity_params(2))
    want = model.predict(cylinder.device_batch(raw, LO, HI, GRID, C))["point_predict"]
    assert torch.equal(out["pred"], want)


def test_voted_evaluation_refuses_training_mode(model, eval_raw):
    model.train()
    try:
        with pytest.raises(RuntimeError):
            model.predict_tta(_cuda(eval_raw), LO, HI, GRID, num_votes=2)
    finally:
        model.eval()
