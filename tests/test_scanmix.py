"""PolarMix / LaserMix of raw batches on the device: csrc/scanmix.hip through scanmix.device_mix.

The yardstick is scanmix.mix_scan_host(atan="double") + scanmix.ring_ids_host(atan="double") -- the kernel's contract: arctan2 in
double, rounded once -- and every comparison is EQUALITY: points as bit patterns, labels, the host frame boundaries. There is no
allowance on the device side. tests/test_scanmix_host.py holds the host form to the reference's own output and bounds its one
allowance (atan="numpy32" against "double"); the fixture's frames hold no face case (the maker's seed guard), so the device is also
held to the recorded reference outputs directly."""
import numpy as np
import pytest
import torch

import fusion_cases as fc
import scanmix_cases as sc
from openpcseg_amd import cylinder, rangeview, scanmix, transform
from openpcseg_amd.workloads.synthetic import make_scan

pytestmark = pytest.mark.gpu

OMEGA = (0.7, 3.1)
SIZES = (1, 63, 64, 65, 257, 1025)


def _scan(n, rng, instances=True):
    """n rows, azimuths all around (so every sector holds some and misses some), labels over 0 .. 19 or over 9 .. 19."""
    az = rng.uniform(-np.pi, np.pi, size=n)
    r = rng.uniform(3, 40, size=n)
    pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-3, 1, size=n), rng.uniform(0, 1, size=n)], axis=1).astype(np.float32)
    return pts, rng.integers(0 if instances else 9, 20, size=n).astype(np.int64)


def _raw(frames, labels, device="cuda"):
    sizes = [f.shape[0] for f in frames]
    return {"points": torch.from_numpy(np.ascontiguousarray(np.concatenate(frames), dtype=np.float32)).to(device),
            "labels": torch.from_numpy(np.concatenate(labels).astype(np.int64)).to(device), "num_frames": len(frames),
            "offsets": [0] + np.cumsum(sizes).tolist()}


def _host_mix(scans1, scans2, plan, omega, ring, classes=scanmix.INSTANCE_CLASSES, lasermix="reference"):
    """mix_scan_host + ring_ids_host per frame, atan="double" -> (points, labels, offsets)."""
    pts, labs = [], []
    for (p1, l1), (p2, l2), row in zip(scans1, scans2, plan):
        p, lab = scanmix.mix_scan_host(p1, l1, p2, l2, row, omega, instance_classes=classes, atan="double", lasermix=lasermix)
        if ring:
            p = np.concatenate([p, scanmix.ring_ids_host(p, atan="double")[:, None]], axis=1)
        pts.append(p)
        labs.append(lab)
    return np.concatenate(pts), np.concatenate(labs), [0] + np.cumsum([p.shape[0] for p in pts]).tolist()


def _device_mix(scans1, scans2, plan, omega, ring, **kw):
    raw = _raw([s[0] for s in scans1], [s[1] for s in scans1])
    partner = _raw([s[0] for s in scans2], [s[1] for s in scans2])
    return scanmix.device_mix(raw, partner, plan, omega, ring=ring, **kw)


def _assert_mixed(out, want, what=""):
    pts, labs, off = want
    assert out["offsets"] == off and out["num_frames"] == len(off) - 1, what
    assert out["points"].dtype == torch.float32 and out["labels"].dtype == torch.int64 and out["points"].is_cuda and out["labels"].is_cuda
    got = out["points"].cpu().numpy()
    assert sc.same_bits(got, pts), "%s: %d of %d rows differ" % (what, int((got.view(np.uint32) != pts.view(np.uint32)).any(1).sum())
                                                                  if got.shape == pts.shape else -1, pts.shape[0])
    assert np.array_equal(out["labels"].cpu().numpy(), labs), what


def _check(scans1, scans2, plan, omega=OMEGA, ring=False, what="", instance_classes=scanmix.INSTANCE_CLASSES, lasermix="reference"):
    plan = np.asarray(plan, dtype=np.float64)
    out = _device_mix(scans1, scans2, plan, omega, ring, instance_classes=instance_classes, lasermix=lasermix)
    _assert_mixed(out, _host_mix(scans1, scans2, plan, omega, ring, instance_classes, lasermix), what)
    return out


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("swap", [0, 1])
def test_every_pair_of_row_counts(hip, swap, ring):
    """One batch of 36 frames: every (n1, n2) of SIZES, around the wave (64), the workgroup tile (256) and several tiles."""
    rng = np.random.default_rng(10 + swap)
    scans1, scans2, plan = [], [], []
    for n1 in SIZES:
        for n2 in SIZES:
            scans1.append(_scan(n1, rng))
            p2, l2 = _scan(n2, rng)
            l2[0] = 1   # an instance row: the mixed frame is never empty
            scans2.append((p2, l2))
            plan.append([scanmix.POLARMIX, rng.uniform(-np.pi, 0), swap, 1])
    _check(scans1, scans2, plan, ring=ring)


@pytest.mark.parametrize("frames", [1, 2, 5])
def test_batches_of_unequal_frames_and_every_kind_of_plan_row(hip, frames):
    rng = np.random.default_rng(20 + frames)
    n1 = (513, 64, 1000, 129, 255)[:frames]
    n2 = (300, 1031, 77, 640, 2)[:frames]
    rows = ([scanmix.POLARMIX, -2.1, 1, 1], [scanmix.POLARMIX, -0.4, 0, 1], [scanmix.LASERMIX, 2, 0, 0], [scanmix.NO_MIX, 0, 0, 0],
            [scanmix.POLARMIX, -1.3, 1, 0])[:frames]
    scans1, scans2 = [_scan(n, rng) for n in n1], [_scan(n, rng) for n in n2]
    for ring in (False, True):
        out = _check(scans1, scans2, rows, ring=ring)
        assert out["points"].shape[1] == (5 if ring else 4)
    if frames == 5:   # LaserMix as the reference computes it, and no mixing: scan 1, row for row
        off = out["offsets"]
        assert off[3] - off[2] == n1[2] and off[4] - off[3] == n1[3]
        assert sc.same_bits(out["points"][off[2]:off[3], :4].cpu().numpy(), scans1[2][0])


def test_a_frame_that_spans_many_workgroups(hip):
    """70 000 rows against 70 000: about 270 workgroups share the frame, so the cross-workgroup bases of every bucket matter."""
    p1, p2 = make_scan(5, 70000), make_scan(6, 70000)
    rng = np.random.default_rng(30)
    l1, l2 = rng.integers(0, 20, size=70000), rng.integers(0, 20, size=70000)
    out = _check([(p1, l1)], [(p2, l2)], [[scanmix.POLARMIX, -1.9, 1, 1]], ring=True)
    n_inst = int(np.isin(l2, scanmix.INSTANCE_CLASSES).sum())
    assert out["offsets"][1] > 70000 and n_inst > 20000 and out["points"][:, 4].max().item() == 63.0
    # twice on the same input: identical bits
    again = _device_mix([(p1, l1)], [(p2, l2)], np.array([[scanmix.POLARMIX, -1.9, 1, 1]]), OMEGA, True)
    assert torch.equal(out["points"].view(torch.int32), again["points"].view(torch.int32)) and torch.equal(out["labels"], again["labels"])
    assert out["offsets"] == again["offsets"]


def test_edge_sectors_and_instance_sets(hip):
    rng = np.random.default_rng(40)
    az1 = rng.uniform(0.2, 2.8, size=300)   # scan 1 on the side yaw in (0.2, 2.8)
    p1 = np.stack([10 * np.cos(-az1), 10 * np.sin(-az1), rng.uniform(-1, 1, 300), rng.uniform(0, 1, 300)], axis=1).astype(np.float32)
    l1 = rng.integers(9, 20, size=300).astype(np.int64)
    p2, l2 = _scan(411, rng)
    none = (p2, rng.integers(9, 20, size=411).astype(np.int64))
    one = (p2, np.where(rng.random(411) < 0.4, 5, 12).astype(np.int64))
    assert scanmix.sector_mask(p1, 0.1, "double").all() and not scanmix.sector_mask(p1, -3.0, "double")[az1 > 0.2].any()
    outside = p2[~scanmix.sector_mask(p2, -3.0, "double")]
    empty = (outside, l2[:outside.shape[0]])
    # all of scan 1 inside the sector / nothing of either scan inside it / no instance rows / one class only / classes of the caller
    scans1 = [(p1, l1)] * 5
    scans2 = [(p2, l2), empty, none, one, (p2, l2)]
    plan = [[scanmix.POLARMIX, 0.1, 1, 1], [scanmix.POLARMIX, -3.0, 1, 1], [scanmix.POLARMIX, -1.0, 1, 1], [scanmix.POLARMIX, -1.0, 1, 1],
            [scanmix.POLARMIX, -1.0, 0, 1]]
    for ring in (False, True):
        out = _check(scans1, scans2, plan, ring=ring)
    off = out["offsets"]
    assert off[3] - off[2] == int((~scanmix.sector_mask(p1, -1.0, "double")).sum() + scanmix.sector_mask(p2, -1.0, "double").sum())
    assert off[5] - off[4] == 300 + 3 * int(np.isin(l2, scanmix.INSTANCE_CLASSES).sum())
    _check(scans1, scans2, plan, instance_classes=(7, 3, 250))
    _check(scans1, scans2, plan, instance_classes=())
    # a yaw that IS the float32 edge stays outside (both inequalities are strict)
    p = np.array([[3.0, 3.0, 0.0, 0.5], [3.0, 2.9999, 0.0, 0.6], [-2.0, -7.0, 0.1, 0.7]], dtype=np.float32)
    alpha = float(-scanmix._arctan2_f32(p[:, 1], p[:, 0], "double")[0])
    lab = np.array([11, 12, 13], dtype=np.int64)
    out = _check([(p, lab)], [(p[::-1].copy(), lab[::-1].copy())], [[scanmix.POLARMIX, alpha, 1, 1]])
    assert out["labels"].tolist() == [11, 13, 12]


def test_a_wrap_across_a_frame_boundary_does_not_count(hip):
    """The last row of frame 0 has proj_x > 0.8, the first row of frame 1 proj_x < 0.2: inside one frame that pair advances the ring."""
    yaw = np.array([0.0, 2.9, -2.9, 2.9, 2.9])   # proj_x = 0.5 (yaw / pi + 1); yaw = -arctan2(y, -x)
    p = np.stack([-np.cos(-yaw), np.sin(-yaw), np.zeros(5), np.arange(5) / 10.0], axis=1).astype(np.float32)
    lab = np.arange(5, dtype=np.int64) + 10
    assert scanmix.ring_ids_host(p, "double").tolist() == [0, 0, 1, 1, 1]
    a, b = (p[:2], lab[:2]), (p[2:], lab[2:])   # frame 0 ends on 2.9, frame 1 starts on -2.9
    assert scanmix.ring_ids_host(np.concatenate([a[0], b[0]]), "double")[2] == 1
    out = _check([a, b, a], [b, a, b], [[scanmix.NO_MIX, 0, 0, 0]] * 3, ring=True)
    assert out["points"][:, 4].tolist() == [0, 0, 0, 0, 0, 0, 0]
    # many rings inside the frames, and a boundary in the middle of a sweep
    scans = [(make_scan(7, 3000), np.zeros(3000, dtype=np.int64)), (make_scan(8, 1700), np.zeros(1700, dtype=np.int64))]
    out = _check(scans, scans[::-1], [[scanmix.NO_MIX, 0, 0, 0], [scanmix.POLARMIX, -2.0, 1, 1]], ring=True)
    assert out["points"][:out["offsets"][1], 4].max().item() == 63.0


def test_lasermix_in_radians_against_its_host_form(hip):
    rng = np.random.default_rng(50)
    scans1 = [(make_scan(9 + s, 2000 + 37 * s), rng.integers(0, 20, size=2000 + 37 * s)) for s in range(4)]
    scans2 = [(make_scan(19 + s, 1500 + 111 * s), rng.integers(0, 20, size=1500 + 111 * s)) for s in range(4)]
    plan = [[scanmix.LASERMIX, s, 0, 0] for s in range(4)]
    out = _check(scans1, scans2, plan, ring=True, lasermix="radians")
    off = out["offsets"]
    assert all(off[f + 1] - off[f] != scans1[f][0].shape[0] for f in range(4))   # the bands did mix
    ref = _check(scans1, scans2, plan, ring=False, lasermix="reference")
    assert sc.same_bits(ref["points"].cpu().numpy(), np.concatenate([s[0] for s in scans1]))


def test_fixture_frames_equal_the_recorded_reference_outputs(hip):
    gold = sc.load_gold()
    frames, labels = sc.frames_and_labels(gold)
    for name, seed, index, xyzret, want_labels, after in sc.cases(gold):
        out = _device_mix([(frames[index], labels[index])], [(frames[1 - index], labels[1 - index])], gold[name + "_plan"][None], sc.omega_of(gold), True)
        assert sc.same_bits(out["points"].cpu().numpy(), xyzret), name
        assert np.array_equal(out["labels"].cpu().numpy(), want_labels) and out["offsets"] == [0, xyzret.shape[0]], name


def _gold_mixed(gold, ring):
    frames, labels = sc.frames_and_labels(gold)
    scans = [(frames[0], labels[0]), (frames[1], labels[1])]
    return _device_mix(scans, scans[::-1], gold["batch_plan"], sc.omega_of(gold), ring)


def test_training_batch_equals_the_recorded_one(hip):
    """transform.device_batch takes the mixed dict unchanged; under the recorded seed's tables the batch is the reference's."""
    gold = sc.load_gold()
    seed, scale = sc.scalar(gold["batch_seed"]), tuple(gold["scale_range"])
    plan, params = scanmix.draw_train_plan(2, np.random.RandomState(seed), scale_range=scale)
    assert np.array_equal(plan, gold["batch_plan"])
    out = transform.device_batch(_gold_mixed(gold, False), sc.scalar(gold["voxel_size"]), params, eval_maps=True)
    sc.assert_equals_batch(gold, sc.batch_arrays(out))


def test_cylinder_and_fusion_batches_take_the_mixed_dict(hip):
    gold = sc.load_gold()
    params = gold["batch_params"]
    lo, hi, grid = [0, -180, -4], [50, 180, 2], [120, 90, 16]
    mixed = _gold_mixed(gold, False)
    got = cylinder.device_batch(mixed, lo, hi, grid, 20, params)
    from openpcseg_amd.workloads.cylinder import cylinder_batch
    off = mixed["offsets"]
    feats = hip.scan_transform(mixed["points"], off, params, 1, 0.05)[0]
    samples = [cylinder.cylinder_sample(feats[off[f]:off[f + 1]].contiguous(), mixed["labels"][off[f]:off[f + 1]], lo, hi, grid, 20) for f in (0, 1)]
    want = cylinder_batch(samples)
    for k in ("point_feature", "point_coord", "point_label", "voxel_coord", "voxel_label", "inverse_map"):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert np.array_equal(got["num_points"], [off[1], off[2] - off[1]])
    # the fusion dataset reads the ring from column 4
    ringed = _gold_mixed(gold, True)
    assert ringed["offsets"] == off and torch.equal(ringed["points"][:, :4], mixed["points"])
    cuts, voxel, hw = np.array([0.3, 0.8]), sc.scalar(gold["voxel_size"]), (64, 2048)
    out = rangeview.device_batch(ringed, voxel, params, cuts, eval_maps=True)
    pts, labs = ringed["points"].cpu().numpy(), ringed["labels"].cpu().numpy()
    want = fc.host_batch([pts[off[f]:off[f + 1]] for f in (0, 1)], [labs[off[f]:off[f + 1]] for f in (0, 1)], params, cuts, voxel, hw, "double")
    have = fc.device_batch_arrays(out)
    for k in fc.INT_KEYS:
        assert np.array_equal(np.asarray(have[k]).astype(np.int64).reshape(want[k].shape), want[k].astype(np.int64)), k
    for k in ("lidar_F", "range_pxpy", "range_image"):
        assert fc.same_bits(have[k], want[k]), k


def test_refusals(hip):
    rng = np.random.default_rng(60)
    a, b = _scan(100, rng), _scan(80, rng, instances=False)
    plan = np.array([[scanmix.POLARMIX, -1.0, 1, 1]])
    raw, partner = _raw([a[0]], [a[1]]), _raw([b[0]], [b[1]])
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        scanmix.device_mix(_raw([a[0]], [a[1]], "cpu"), partner, plan, OMEGA)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        scanmix.device_mix(raw, _raw([b[0]], [b[1]], "cpu"), plan, OMEGA)
    with pytest.raises(ValueError, match="as many partner frames"):
        scanmix.device_mix(raw, _raw([b[0], b[0]], [b[1], b[1]]), plan, OMEGA)
    with pytest.raises(ValueError, match="plan"):
        scanmix.device_mix(raw, partner, np.zeros((2, 4)), OMEGA)
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        scanmix.device_mix({**raw, "points": torch.zeros(100, 5, device="cuda")}, partner, plan, OMEGA)
    with pytest.raises(ValueError, match="frame boundaries"):
        scanmix.device_mix({**raw, "offsets": [0, 99]}, partner, plan, OMEGA)
    with pytest.raises(ValueError, match="instance classes"):
        scanmix.device_mix(raw, partner, plan, OMEGA, instance_classes=range(9))
    # a mixed frame with no rows: all of scan 1 inside the sector, nothing of scan 2, no instances
    inside = a[0][scanmix.sector_mask(a[0], -1.0, "double")]
    outside = b[0][~scanmix.sector_mask(b[0], -1.0, "double")]
    assert len(inside) and len(outside)
    with pytest.raises(ValueError, match="no rows"):
        scanmix.device_mix(_raw([a[0], inside], [a[1], a[1][:len(inside)]]), _raw([b[0], outside], [b[1], b[1][:len(outside)]]),
                           np.array([[scanmix.POLARMIX, -1.0, 1, 1]] * 2), OMEGA)
