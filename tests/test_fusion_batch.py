"""The fusion (RPVNet) dataset's batch on the device: csrc/rangeproj.hip through the raw C ABI,
rangeview.device_batch and RPVNet.predict_tta.

The yardstick is rangeview.range_view_host: get_range_image restated line by line in NumPy (tests/test_fusion_batch_host.py holds
it to the reference's own output bit for bit). Against atan="double" -- the kernel's contract: arctan2 in double, rounded once --
every comparison is EQUALITY: integers, pxpy rows, every pixel of every channel. Against atan="numpy32", the reference's float32
arctan2, one allowance exists (test_full_scan_against_the_reference_arithmetic): rows whose two arctan2 values differ by an ulp AND
whose column flips because of it -- adjacent columns, reproduced exactly by "double", at most 1e-4 of the rows (the cap
tests/test_cylinder_frontend.py uses for the same cause; 200 000 random rows gave 1.5e-5 on the CPU, the test's own scan and cuts
gave 0 of 290 055 rows there)."""
import ctypes

import numpy as np
import pytest
import torch

import fusion_cases as fc
from openpcseg_amd import rangeview
from openpcseg_amd.inference import SegEvaluator
from seeded import seeded_state
from transform_cases import host_batch as host_voxel_batch

pytestmark = pytest.mark.gpu

CUTS = (0.0, 0.5, 0.999999)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_kernels(hip, feats, scenes, cuts, num_scenes, hw):
    """pcs_range_project_f32 + pcs_range_image_fill_f32 on host arrays -> (image, pxpy, bad flag) as host values. Every output
    starts from garbage: the entries own the clearing of `winner` and `bad`."""
    h, w = hw
    n, c = feats.shape
    f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(scenes, dtype=np.int32)).cuda()
    cut = torch.from_numpy(rangeview.cut_value(cuts).reshape(-1)).cuda()
    ws = hip.lib.pcs_range_project_ws_bytes(num_scenes, h, w)
    assert ws == num_scenes * h * w * 4
    winner = torch.full((ws // 4,), 12345, dtype=torch.int32, device="cuda")
    pxpy = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    image = torch.full((num_scenes, 5, h, w), float("nan"), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.lib.pcs_range_project_f32(_ptr(f), n, c, _ptr(s), _ptr(cut), num_scenes, h, w, _ptr(winner), _ptr(pxpy), _ptr(bad), st) == 0
    assert hip.lib.pcs_range_image_fill_f32(_ptr(winner), _ptr(f), n, c, num_scenes, h, w, _ptr(image), st) == 0
    torch.cuda.synchronize()
    win = winner.cpu().numpy()
    assert win.min() >= -1 and win.max() < n
    return image.cpu().numpy(), pxpy.cpu().numpy(), int(bad.item())


def host_view(feats, scenes, cuts, num_scenes, hw, atan="double"):
    """range_view_host per scene + the collates' (scene, px, py) table in float32."""
    image = np.empty((num_scenes, 5) + tuple(hw), dtype=np.float32)
    pxpy = np.empty((feats.shape[0], 3), dtype=np.float32)
    for s in range(num_scenes):
        rows = np.flatnonzero(scenes == s)
        assert rows.size == 0 or np.array_equal(rows, np.arange(rows[0], rows[-1] + 1))   # a scene's rows are contiguous
        image[s], p = rangeview.range_view_host(feats[rows], cuts[s], hw, atan=atan)
        pxpy[rows] = np.pad(p, ((0, 0), (1, 0)), mode="constant", constant_values=s).astype(np.float32)
    return image, pxpy


def random_rows(rng, n, c, h):
    """n rows [x, y, z, reflectivity, ring, extras...]: azimuths all around, rings over the whole image incl. 0 and h - 1."""
    out = rng.uniform(-1, 1, size=(n, c)).astype(np.float32)
    out[:, :2] *= 50
    out[:, 2] *= 3
    out[:, 3] = np.abs(out[:, 3])
    out[:, 4] = rng.integers(0, h, size=n)
    out[0, 4] = h - 1
    out[n - 1, 4] = 0
    return out


def fan_rows(rng, n, c, h):
    """Heavy collisions: four rings, azimuths inside a 2 degree fan -> a few dozen pixels for n rows."""
    out = random_rows(rng, n, c, h)
    az = np.deg2rad(rng.uniform(100, 102, size=n))
    r = rng.uniform(5, 40, size=n)
    out[:, 0], out[:, 1] = (r * np.cos(az)).astype(np.float32), (r * np.sin(az)).astype(np.float32)
    out[:, 4] = rng.integers(0, 4, size=n) * ((h - 1) // 3)
    return out


def assert_equal_view(got_image, got_pxpy, want_image, want_pxpy):
    assert fc.same_bits(got_pxpy, want_pxpy), "pxpy: %d rows differ" % int((got_pxpy != want_pxpy).any(1).sum())
    assert fc.same_bits(got_image, want_image), "image: %d pixels differ" % int((got_image.view(np.uint32) != want_image.view(np.uint32)).any(1).sum())


# ---- a. the kernels through the C ABI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [5, 7])
@pytest.mark.parametrize("hw", [(64, 2048), (64, 512), (4, 126)])
def test_kernels_equal_the_host_contract(hip, hw, c):
    """Scenes of 1, 63, 64, 65, 257, 700 (the fan), 1, 2 (the wrap rows) and 300 rows in one call: one-row scenes, scene boundaries
    inside a workgroup, every cut, rings 0 and H - 1, the yaw that wraps to float32(2 pi)."""
    rng = np.random.default_rng(hw[1] + c)
    sizes = [1, 63, 64, 65, 257, 700, 1, 2, 300]
    parts = [fan_rows(rng, n, c, hw[0]) if n == 700 else random_rows(rng, n, c, hw[0]) for n in sizes]
    parts[7][:, :2] = [[-5.0, -5e-9], [-5.0, 5e-9]]
    feats = np.concatenate(parts)
    scenes = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    cuts = np.array([CUTS[k % 3] for k in range(len(sizes))])
    cuts[7] = 0.5   # no cut: the wrap rows keep their yaw of -+1e-9
    image, pxpy, bad = run_kernels(hip, feats, scenes, cuts, len(sizes), hw)
    want_image, want_pxpy = host_view(feats, scenes, cuts, len(sizes), hw)
    assert bad == 0
    assert_equal_view(image, pxpy, want_image, want_pxpy)
    first = int(np.sum(sizes[:7]))
    assert pxpy[first:first + 2, 1].tolist() == [1.0, -1.0]   # columns W - 1 and 0
    fan = image[5]
    hits = int((fan.reshape(5, -1).T.view(np.uint32) != fc.EMPTY.view(np.uint32)).any(1).sum())
    assert hits * 4 < 700, hits   # most pixels of the fan were hit several times


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("cut", CUTS)
def test_row_counts_around_a_wave(hip, n, cut):
    rng = np.random.default_rng(n)
    feats = random_rows(rng, n, 5, 64)
    scenes = np.zeros(n, dtype=np.int32)
    image, pxpy, bad = run_kernels(hip, feats, scenes, [cut], 1, (64, 512))
    assert bad == 0
    assert_equal_view(image, pxpy, *host_view(feats, scenes, [cut], 1, (64, 512)))


def test_fixture_rows_through_the_kernels(hip):
    gold = fc.load_gold()
    hw = tuple(int(v) for v in gold["hw"])
    for prefix, cuts in (("train_", gold["train_cuts"]), ("tta0_", gold["tta_cuts"][0::2]), ("tta1_", gold["tta_cuts"][1::2])):
        feats = np.ascontiguousarray(gold[prefix + "lidar_F"].T)
        scenes = gold[prefix + "lidar_C"][3].astype(np.int32)
        image, pxpy, bad = run_kernels(hip, feats, scenes, cuts, len(cuts), hw)
        assert bad == 0
        assert_equal_view(image, pxpy, *host_view(feats, scenes, cuts, len(cuts), hw))
        assert fc.same_bits(image, fc.fixture_image(gold, prefix, len(cuts))) and fc.same_bits(pxpy, np.ascontiguousarray(gold[prefix + "range_pxpy"].T))


def test_no_rows_gives_the_empty_image(hip):
    image, pxpy, bad = run_kernels(hip, np.zeros((0, 5), dtype=np.float32), np.zeros(0, dtype=np.int32), [0.3, 0.6], 2, (4, 126))
    assert bad == 0 and pxpy.shape == (0, 3)
    assert np.array_equal(image, np.broadcast_to(fc.EMPTY[None, :, None, None], image.shape))


# ---- b. / c. device_batch ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return fc.load_gold()


def _raw(frames, labels):
    sizes = [f.shape[0] for f in frames]
    return {"points": torch.from_numpy(np.concatenate(frames)).cuda(), "labels": torch.from_numpy(np.concatenate(labels)).cuda(),
            "num_frames": len(frames), "offsets": [0] + np.cumsum(sizes).tolist()}


def test_training_batch_against_the_reference(hip, gold):
    frames, labels = fc.frames_and_labels(gold)
    out = rangeview.device_batch(_raw(frames, labels), fc.scalar(gold["voxel_size"]), gold["train_params"], gold["train_cuts"], eval_maps=True)
    assert "bad" not in out and out["offset"].dtype == torch.int32 and out["range_pxpy"].dtype == torch.float32
    fc.assert_equals_fixture(gold, "train_", fc.device_batch_arrays(out))


def test_tta_batches_against_the_reference(hip, gold):
    """Ten votes of each frame against collate_batch_tta's batch; then both frames in one call (scene v * 2 + f), scene by scene
    equal to the one-frame calls and bit-identical when repeated."""
    frames, labels = fc.frames_and_labels(gold)
    voxel = fc.scalar(gold["voxel_size"])
    single = []
    for f in range(2):
        out = rangeview.device_batch(_raw([frames[f]], [labels[f]]), voxel, gold["tta_params"][f::2], gold["tta_cuts"][f::2], votes=10,
                                     eval_maps=True)
        fc.assert_equals_fixture(gold, "tta%d_" % f, fc.device_batch_arrays(out))
        single.append(out)
    both = [rangeview.device_batch(_raw(frames, labels), voxel, gold["tta_params"], gold["tta_cuts"], votes=10, eval_maps=True) for _ in range(2)]
    for k in ("range_image", "range_pxpy", "offset"):
        assert torch.equal(both[0][k], both[1][k]), k
    assert torch.equal(both[0]["lidar"].F, both[1]["lidar"].F) and torch.equal(both[0]["lidar"].C, both[1]["lidar"].C)
    scene = both[0]["range_pxpy"][:, 0]
    assert torch.equal(scene, both[0]["lidar"].C[:, 3].float())
    for f in range(2):
        assert torch.equal(both[0]["range_image"][f::2], single[f]["range_image"])
        for v in range(10):
            assert torch.equal(both[0]["range_pxpy"][scene == v * 2 + f][:, 1:], single[f]["range_pxpy"][single[f]["range_pxpy"][:, 0] == v][:, 1:])
    assert both[0]["offset"].tolist() == np.cumsum(np.bincount(both[0]["lidar"].C[:, 3].cpu().numpy(), minlength=20)).tolist()


def test_no_cuts_means_no_cut(hip, gold):
    frames, labels = fc.frames_and_labels(gold)
    raw = _raw(frames, labels)
    a = rangeview.device_batch(raw, 0.25, hw=(64, 512))
    b = rangeview.device_batch(raw, 0.25, cuts=[0.5, 0.5], hw=(64, 512))
    assert torch.equal(a["range_image"], b["range_image"]) and torch.equal(a["range_pxpy"], b["range_pxpy"]) and "inverse_map" not in a
    feats, scenes = a["lidar"].F.cpu().numpy(), a["lidar"].C[:, 3].cpu().numpy()
    assert_equal_view(a["range_image"].cpu().numpy(), a["range_pxpy"].cpu().numpy(), *host_view(feats, scenes, [0.5, 0.5], 2, (64, 512)))
    with pytest.raises(ValueError):
        rangeview.device_batch(raw, 0.25, cuts=[0.5])
    with pytest.raises(ValueError):
        rangeview.device_batch({**raw, "points": raw["points"][:, :4].contiguous()}, 0.25)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        rangeview.device_batch({**raw, "points": raw["points"].cpu()}, 0.25)


# ---- d. rows the reference cannot place ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [64.0, -1.0, float("nan")])
def test_bad_rows_are_flagged_and_touch_no_pixel(hip, gold, ring):
    """Row 17 of frame 1 is alone in its voxel (checked on the host), so it reaches the projection whatever its ring says."""
    frames, labels = fc.frames_and_labels(gold)
    frames = [f.copy() for f in frames]
    frames[1][17, 4] = ring
    raw = _raw(frames, labels)
    cuts = [0.25, 0.75]
    with pytest.raises(ValueError, match=r"\[0, 63\]"):
        rangeview.device_batch(raw, 0.25, cuts=cuts)
    out = rangeview.device_batch(raw, 0.25, cuts=cuts, check=False)
    assert int(out["bad"].item()) == 1
    feats, scenes = out["lidar"].F.cpu().numpy(), out["lidar"].C[:, 3].cpu().numpy()
    keep = np.isfinite(feats[:, :2]).all(1) & (feats[:, 4] >= 0) & (feats[:, 4] <= 63)   # NaN compares false
    assert int((~keep).sum()) == 1
    want_image, want_pxpy = host_view(feats[keep], scenes[keep], cuts, 2, (64, 2048))   # as if the row were absent
    assert fc.same_bits(out["range_image"].cpu().numpy(), want_image)
    assert fc.same_bits(out["range_pxpy"].cpu().numpy()[keep], want_pxpy)
    clean = rangeview.device_batch(_raw(fc.frames_and_labels(gold)[0], labels), 0.25, cuts=cuts, check=False)
    assert int(clean["bad"].item()) == 0   # the flag is cleared by every call


def test_rows_that_are_not_finite_or_outside_the_batch_are_flagged(hip):
    """Through the C ABI: NaN / infinite x, y and ring, rings just outside the image, scenes outside [0, S). Rings that ROUND into
    the image (-0.4, H - 0.6) are not bad."""
    rng = np.random.default_rng(3)
    feats = random_rows(rng, 100, 5, 4)
    scenes = np.zeros(100, dtype=np.int32)
    scenes[40], scenes[41] = 1, -1
    feats[10, 0], feats[11, 1], feats[12, 4], feats[13, 0], feats[14, 4] = np.nan, np.inf, np.nan, -np.inf, np.inf
    feats[15, 4], feats[16, 4], feats[17, 4], feats[18, 4] = 4.0, -1.0, 3.6, -0.6
    feats[19, 4], feats[20, 4] = -0.4, 3.4
    image, pxpy, bad = run_kernels(hip, feats, scenes, [0.5], 1, (4, 126))
    keep = scenes == 0
    keep[10:19] = False
    assert bad == 1
    want_image, want_pxpy = host_view(feats[keep], scenes[keep], [0.5], 1, (4, 126))
    assert fc.same_bits(image, want_image) and fc.same_bits(pxpy[keep], want_pxpy)


# ---- e. a whole scan against the reference's own arithmetic: the one allowance ---------------------------------------------------------
def test_full_scan_against_the_reference_arithmetic(hip):
    from openpcseg_amd.workloads.synthetic import make_fusion_raw_batch
    raw = make_fusion_raw_batch([0])
    raw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}
    cuts = np.array([0.137, 0.5, 0.871])
    out = rangeview.device_batch(raw, 0.05, cuts=cuts, votes=3)
    h, w = 64, 2048
    feats, scenes = out["lidar"].F.cpu().numpy(), out["lidar"].C[:, 3].cpu().numpy()
    image, pxpy = out["range_image"].cpu().numpy(), out["range_pxpy"].cpu().numpy()
    assert feats.shape[0] > 3 * 90000
    dbl_image, dbl_pxpy = host_view(feats, scenes, cuts, 3, (h, w), "double")
    assert_equal_view(image, pxpy, dbl_image, dbl_pxpy)   # the kernel's contract: equality everywhere
    ref_image, ref_pxpy = host_view(feats, scenes, cuts, 3, (h, w), "numpy32")
    differ = np.flatnonzero((pxpy.view(np.uint32) != ref_pxpy.view(np.uint32)).any(1))
    print("face cases: %d of %d rows (cap %d)" % (differ.size, feats.shape[0], int(1e-4 * feats.shape[0])))
    assert differ.size <= 1e-4 * feats.shape[0]
    col = lambda p: np.round((p[:, 1].astype(np.float64) / 2 + 0.5) * (w - 1)).astype(np.int64)
    row = lambda p: np.round((p[:, 2].astype(np.float64) / 2 + 0.5) * (h - 1)).astype(np.int64)
    got_c, ref_c = col(pxpy[differ]), col(ref_pxpy[differ])
    assert np.array_equal(pxpy[differ][:, [0, 2]], ref_pxpy[differ][:, [0, 2]])             # scene and image row agree
    assert np.isin((got_c - ref_c) % w, (1, w - 1)).all()                                   # neighbours on the circle
    assert np.array_equal(pxpy[differ].view(np.uint32), dbl_pxpy[differ].view(np.uint32))   # and "double" reproduces them
    exempt = np.zeros((3, h, w), dtype=bool)
    for cols in (got_c, ref_c):
        exempt[scenes[differ], row(pxpy[differ]), cols] = True
    same = (image.view(np.uint32) == ref_image.view(np.uint32)).all(1)
    assert (same | exempt).all(), int((~(same | exempt)).sum())


# ---- f. RPVNet.predict_tta -----------------------------------------------------------------------------------------------------------
C = 20
VOTES = 4
HW_SMALL = (64, 512)


@pytest.fixture(scope="module")
def model(hip):
    from openpcseg_amd.workloads.rpvnet import RPVNet
    m = RPVNet(num_class=C, in_dim=5, num_layer=[2] * 8, cr=0.25).cuda().eval()
    seeded_state(m)
    return m


@pytest.fixture(scope="module")
def eval_raw():
    from openpcseg_amd.workloads.synthetic import make_fusion_raw_batch
    return make_fusion_raw_batch([1, 2], n_points=2000, num_classes=C)


def _cuda(raw):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}


def _float64_votes(raw, out, num_votes, voxel):
    """Sum over the votes of softmax(logits of the point's voxel) in float64, through the HOST-built inverse maps."""
    nf, off = raw["num_frames"], raw["offsets"]
    host = host_voxel_batch(raw, out["params"], num_votes, voxel)
    scene_v, scene_p, inv = host["lidar"].C[:, 3].numpy(), host["inverse_map"].C[:, 3].numpy(), host["inverse_map"].F.numpy()
    ref = np.zeros((off[-1], C))
    assert len(out["logits"]) == num_votes
    for v, lg in enumerate(out["logits"]):
        lg = lg.cpu().numpy().astype(np.float64)
        first = int((scene_v < v * nf).sum())
        assert lg.shape == (int(((scene_v >= v * nf) & (scene_v < (v + 1) * nf)).sum()), C)
        for f in range(nf):
            s = v * nf + f
            rows = lg[int((scene_v < s).sum()) - first + inv[scene_p == s]]
            e = np.exp(rows - rows.max(1, keepdims=True))
            ref[off[f]:off[f + 1]] += e / e.sum(1, keepdims=True)
    return ref


@pytest.mark.parametrize("vote_chunk", [2, 4])
def test_voted_evaluation(model, eval_raw, vote_chunk):
    """Votes within num_votes * 1e-6 of the float64 softmax sum of the returned logits (the bound of tests/test_predict_tta.py);
    the returned logits are point_logits on device_batch of the returned tables; the evaluator counts every point once."""
    ev = SegEvaluator(C)
    raw = _cuda(eval_raw)
    out = model.predict_tta(raw, num_votes=VOTES, evaluator=ev, vote_chunk=vote_chunk, rng=np.random.RandomState(7), hw=HW_SMALL,
                            return_logits=True)
    n, nf = eval_raw["offsets"][-1], eval_raw["num_frames"]
    want_params, want_cuts = rangeview.tta_params(nf, VOTES, rng=np.random.RandomState(7))
    assert np.array_equal(out["params"], want_params) and np.array_equal(out["cuts"], want_cuts) and out["cuts"].shape == (VOTES * nf,)
    votes = out["votes"].cpu().numpy()
    assert votes.shape == (n, C) and votes.dtype == np.float32
    err = float(np.abs(votes.astype(np.float64) - _float64_votes(eval_raw, out, VOTES, model.pres)).max())
    print("votes: max abs error %.3e over %d votes (bound %.1e)" % (err, VOTES, VOTES * 1e-6))
    assert err <= VOTES * 1e-6, err
    pred = out["pred"].cpu().numpy()
    assert pred.dtype == np.int64 and np.array_equal(pred, votes.argmax(1)) and out["point_offset"] == eval_raw["offsets"]
    hist, labels = ev.hist.cpu().numpy(), eval_raw["labels"].numpy()
    assert int(hist.sum()) == n and int(ev.bad) == 0   # once per point, not once per vote
    assert np.array_equal(hist, np.bincount(C * labels + pred, minlength=C * C).reshape(C, C))
    # the logits are those of the batches the returned tables describe
    for v0 in range(0, VOTES, vote_chunk):
        batch = rangeview.device_batch(raw, model.pres, out["params"][v0 * nf:(v0 + vote_chunk) * nf], out["cuts"][v0 * nf:(v0 + vote_chunk) * nf],
                                       votes=vote_chunk, eval_maps=True, hw=HW_SMALL)
        assert batch["range_image"].shape == (vote_chunk * nf, 5) + HW_SMALL
        with torch.inference_mode():
            logits = model.point_logits(batch["lidar"], batch["range_image"], batch["range_pxpy"]).float()
        assert torch.equal(logits, torch.cat(out["logits"][v0:v0 + vote_chunk]))
    plain = model.predict_tta(raw, num_votes=VOTES, vote_chunk=vote_chunk, rng=np.random.RandomState(7), hw=HW_SMALL)
    assert "logits" not in plain and torch.equal(plain["pred"], out["pred"]) and torch.equal(plain["votes"], out["votes"])


def test_training_calls_after_an_evaluation_pass(model, eval_raw):
    """The evaluation runs under inference_mode and makes rangelib's pinned frame-order flags there; they go back to a pool that
    a later call OUTSIDE inference mode draws from, so they must be ordinary tensors (an inference tensor refuses `copy_`)."""
    from openpcseg_amd import rangelib
    model.predict_tta(_cuda(eval_raw), num_votes=2, hw=HW_SMALL)
    rangelib.verify_pending(block=True)   # the pass's flags return to the pool
    fmap = torch.randn(2, 8, 16, 64, device="cuda")
    for _ in range(8):   # more calls than the pass left flags: pooled ones and new ones
        pxpy = torch.tensor([[0, 0.1, 0.2], [1, -0.3, 0.4]], device="cuda")
        assert rangelib.range_to_point(fmap, pxpy).shape == (2, 8)
    rangelib.verify_pending(block=True)


def test_voted_evaluation_refusals(model, eval_raw):
    model.train()
    try:
        with pytest.raises(RuntimeError, match="model.eval"):
            model.predict_tta(_cuda(eval_raw), num_votes=2, hw=HW_SMALL)
    finally:
        model.eval()
    with pytest.raises(ValueError):
        model.predict_tta(_cuda(eval_raw), num_votes=11, hw=HW_SMALL)
