"""The host contract of PolarMix / LaserMix on raw batches, without a device: the drawers, mix_scan_host and
ring_ids_host against the reference's own output (tests/golden/mix_golden.npz, written by tests/golden/make_mix_golden.py by
RUNNING SemantickittiDataset.__getitem__ and the voxel dataset's collate), hand-made edge cases under both arctan2 rules, the
refusals, and the new C entries' declarations and size-only refusals.

The one allowance against the reference's arithmetic (test_sector_membership_of_the_two_arctan2_rules): NumPy's float32 arctan2
and a double arctan2 rounded once differ by an ulp in about a third of the values; a row changes sides of a sector edge only when
the edge falls between the two. Cap: 1e-6 of the rows tested (2e-8 was seen on random rows). On this test's scans and sectors the
count is 0 of 720 000."""
import os
import re

import numpy as np
import pytest

import scanmix_cases as sc
from openpcseg_amd import native, scanmix
from openpcseg_amd.workloads.synthetic import make_partner_raw_batch, make_raw_batch, make_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcs_scan_mix_ws_bytes", "pcs_scan_mix_count", "pcs_scan_mix_place", "pcs_scan_ring_ws_bytes", "pcs_scan_ring_f32")
ATANS = ("numpy32", "double")
OMEGA = (0.7, 3.1)


@pytest.fixture(scope="module")
def gold():
    return sc.load_gold()


def _polar(alpha, swap=1, paste=1):
    return np.array([scanmix.POLARMIX, alpha, swap, paste], dtype=np.float64)


def _ring_scan(n, rng, r=10.0):
    """n rows on a circle, azimuths all around, z and reflectivity random."""
    az = rng.uniform(-np.pi, np.pi, size=n)
    return np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2, 2, size=n), rng.uniform(0, 1, size=n)], axis=1).astype(np.float32)


# ---- the drawers ---------------------------------------------------------------------------------------------------------------
def test_draw_omega_is_the_modules_omega(gold):
    np.random.seed(sc.scalar(gold["omega_seed"]))
    assert scanmix.draw_omega() == sc.omega_of(gold)
    assert scanmix.draw_omega(np.random.RandomState(sc.scalar(gold["omega_seed"]))) == sc.omega_of(gold)
    a, b = sc.omega_of(gold)
    assert 0 <= a < 2 * np.pi / 3 <= b < 4 * np.pi / 3


def test_draw_mix_plan_gives_the_recorded_rows_and_generator_state(gold):
    kinds = set()
    for name, seed, index, xyzret, labels, after in sc.cases(gold):
        np.random.seed(seed)
        plan = scanmix.draw_mix_plan(1)
        assert plan.dtype == np.float64 and plan.shape == (1, 4) and np.array_equal(plan[0], gold[name + "_plan"])
        assert sc.digest() == after
        rng = np.random.RandomState(seed)
        assert np.array_equal(scanmix.draw_mix_plan(1, rng), plan) and sc.digest(rng) == after
        kinds.add((int(plan[0, 0]), int(plan[0, 2])))
        if plan[0, 0] == scanmix.POLARMIX:
            assert -np.pi <= plan[0, 1] < 0 and plan[0, 3] == 1
        else:
            assert plan[0, 1] in (0, 1, 2, 3)
    assert {k[0] for k in kinds} == {scanmix.POLARMIX, scanmix.LASERMIX} and (scanmix.POLARMIX, 1) in kinds and (scanmix.POLARMIX, 0) in kinds


def test_draw_train_plan_gives_the_recorded_tables_and_generator_state(gold):
    seed, scale = sc.scalar(gold["batch_seed"]), tuple(gold["scale_range"])
    after = (gold["batch_state_after"].tobytes(), sc.scalar(gold["batch_pos_after"]))
    np.random.seed(seed)
    plan, params = scanmix.draw_train_plan(2, scale_range=scale)
    assert np.array_equal(plan, gold["batch_plan"]) and np.array_equal(params, gold["batch_params"]) and sc.digest() == after
    rng = np.random.RandomState(seed)
    plan2, params2 = scanmix.draw_train_plan(2, rng, dataset="cylinder", scale_range=scale)
    assert np.array_equal(plan2, plan) and np.array_equal(params2, params) and sc.digest(rng) == after
    # fusion: one more draw per frame, the cut, behind the frame's augmentation
    rng = np.random.RandomState(seed)
    plan3, params3, cuts = scanmix.draw_train_plan(2, rng, dataset="fusion", scale_range=scale)
    assert np.array_equal(plan3[0], plan[0]) and np.array_equal(params3[0], params[0]) and cuts.shape == (2,) and ((cuts >= 0) & (cuts < 1)).all()
    check = np.random.RandomState(seed)
    scanmix.draw_mix_plan(1, check)
    from openpcseg_amd import transform
    transform.draw_train_params(1, check, scale_range=scale)
    assert cuts[0] == check.rand()
    with pytest.raises(ValueError):
        scanmix.draw_train_plan(2, dataset="range")


def test_without_mixing_one_choice_per_frame_is_consumed():
    rng, check = np.random.RandomState(5), np.random.RandomState(5)
    plan = scanmix.draw_mix_plan(7, rng, mix=False)
    assert (plan[:, 0] == scanmix.NO_MIX).all() and not plan[:, 1:].any()
    for _ in range(7):
        check.choice(2, 1)
    assert sc.digest(rng) == sc.digest(check)
    rng, check = np.random.RandomState(6), np.random.RandomState(6)
    plan, params = scanmix.draw_train_plan(3, rng, mix=False)
    from openpcseg_amd import transform
    for f in range(3):
        check.choice(2, 1)
        assert np.array_equal(params[f], transform.draw_train_params(1, check)[0])
    assert sc.digest(rng) == sc.digest(check) and (plan[:, 0] == scanmix.NO_MIX).all()


# ---- the reference's own output ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atan", ATANS)
def test_recorded_frames_are_reproduced_bit_for_bit(gold, atan):
    """atan="numpy32" is the reference's arithmetic; atan="double" equals it on the fixture by the maker's seed guard: no face case."""
    frames, labels = sc.frames_and_labels(gold)
    for name, seed, index, xyzret, want_labels, after in sc.cases(gold):
        got, got_labels = sc.host_xyzret(frames, labels, index, gold[name + "_plan"], sc.omega_of(gold), atan)
        assert sc.same_bits(got, xyzret), name
        assert got_labels.dtype == np.int64 and np.array_equal(got_labels, want_labels), name
        assert xyzret[:, 4].max() >= 1   # the ring column counts something


@pytest.mark.parametrize("atan", ATANS)
def test_recorded_training_batch_is_reproduced(gold, atan):
    frames, labels = sc.frames_and_labels(gold)
    batch = sc.host_train_batch(frames, labels, gold["batch_plan"], gold["batch_params"], sc.omega_of(gold), sc.scalar(gold["voxel_size"]), atan)
    sc.assert_equals_batch(gold, batch)


def test_fixture_covers_what_it_should(gold):
    frames, labels = sc.frames_and_labels(gold)
    for c in (1, 2, 5):
        assert (labels[0] == c).any() and (labels[1] == c).any()
    assert not (labels[0] == 6).any() and not (labels[1] == 6).any() and (labels[0] == 3).any() and not (labels[1] == 3).any()
    by_name = {c[0]: c for c in sc.cases(gold)}
    laser = by_name["laser"]
    assert np.array_equal(laser[3][:, :4], frames[laser[2]]) and np.array_equal(laser[4], labels[laser[2]])   # scan 1, row for row
    n = frames[by_name["noswap"][2]].shape[0]
    inst = (by_name["noswap"][3].shape[0] - n) // 3
    assert inst > 0 and np.array_equal(by_name["noswap"][3][:n, :4], frames[by_name["noswap"][2]])
    tail = by_name["noswap"][3][n:, :4]
    assert np.array_equal(tail[:inst, 3], tail[inst:2 * inst, 3]) and not np.array_equal(tail[:inst, :2], tail[inst:2 * inst, :2])
    assert ((gold["batch_plan"][:, 0] == scanmix.POLARMIX) & (gold["batch_plan"][:, 2] == 1)).any()


def test_lasermix_as_the_reference_wrote_it_returns_scan_one():
    rng = np.random.default_rng(0)
    p1, p2 = _ring_scan(300, rng), _ring_scan(200, rng)
    l1, l2 = rng.integers(0, 20, size=300), rng.integers(0, 20, size=200)
    for strategy in range(4):
        pts, lab = scanmix.mix_scan_host(p1, l1, p2, l2, [scanmix.LASERMIX, strategy, 0, 0], OMEGA)
        assert sc.same_bits(pts, p1) and np.array_equal(lab, l1)
    pts, lab = scanmix.mix_scan_host(p1, l1, p2, l2, [scanmix.NO_MIX, 0, 0, 0], OMEGA)
    assert sc.same_bits(pts, p1) and np.array_equal(lab, l1)


def test_lasermix_in_radians_alternates_the_bands():
    """One point per band and scan: xyzil_mix_1 takes bands 1, 3, 5 from scan 1 and 2, 4, 6 from scan 2, in band order."""
    degs = {0: (0.0, -10.0, -20.0), 1: (0.0, -7.0, -12.0, -20.0), 2: (0.0, -6.0, -10.0, -14.0, -20.0), 3: (0.0, -5.0, -8.0, -11.0, -15.0, -20.0)}
    for strategy, incs in degs.items():
        inc = np.deg2rad(np.array(incs))
        # scan order is the reverse of band order: the output must be sorted by band, not by row
        rows = lambda tag: np.stack([10 * np.cos(inc), np.zeros_like(inc), 10 * np.sin(inc), tag + np.arange(len(incs)) / 10.0], axis=1)[::-1].astype(np.float32)
        p1, p2 = rows(1.0), rows(2.0)
        l1, l2 = np.arange(len(incs))[::-1] + 10, np.arange(len(incs))[::-1] + 20
        pts, lab = scanmix.mix_scan_host(p1, l1, p2, l2, [scanmix.LASERMIX, strategy, 0, 0], OMEGA, lasermix="radians")
        assert lab.tolist() == [(10 if b % 2 == 0 else 20) + b for b in range(len(incs))]
        assert np.allclose(pts[:, 3], [(1.0 if b % 2 == 0 else 2.0) + b / 10.0 for b in range(len(incs))])
        assert len(scanmix.LASERMIX_BANDS[strategy]) == len(incs) - 1


# ---- hand-made sectors -------------------------------------------------------------------------------------------------------
def _by_hand(p1, l1, p2, l2, alpha, swap, atan, classes=scanmix.INSTANCE_CLASSES):
    """The mixed frame from the documented order, with sector_mask as the only shared piece."""
    in1 = scanmix.sector_mask(p1, alpha, atan) if swap else np.zeros(len(p1), dtype=bool)
    in2 = scanmix.sector_mask(p2, alpha, atan) if swap else np.zeros(len(p2), dtype=bool)
    inst = np.concatenate([np.flatnonzero(l2 == c) for c in classes]).astype(np.int64)
    rot = []
    for w in OMEGA:
        m = np.array([[np.cos(w), np.sin(w), 0], [-np.sin(w), np.cos(w), 0], [0, 0, 1]])
        r = np.zeros_like(p2[inst])
        r[:, :3] = np.dot(p2[inst][:, :3], m)
        r[:, 3] = p2[inst][:, 3]
        rot.append(r)
    return (np.concatenate([p1[~in1], p2[in2], p2[inst]] + rot), np.concatenate([l1[~in1], l2[in2], l2[inst], l2[inst], l2[inst]]))


@pytest.mark.parametrize("atan", ATANS)
def test_hand_made_sectors(atan):
    rng = np.random.default_rng(3)
    # scan 1 on the side yaw in (0.2, 2.8) (y < 0), scan 2 all around
    az1 = rng.uniform(0.2, 2.8, size=90)
    p1 = np.stack([10 * np.cos(-az1), 10 * np.sin(-az1), rng.uniform(-1, 1, 90), rng.uniform(0, 1, 90)], axis=1).astype(np.float32)
    p2 = _ring_scan(70, rng)
    l1 = rng.integers(9, 20, size=90)
    cases = {"no instances": rng.integers(9, 20, size=70), "one class": np.where(rng.random(70) < 0.4, 5, 12), "mixed": rng.integers(0, 10, size=70)}
    for what, l2 in cases.items():
        for alpha, swap in ((-2.0, 1), (-0.5, 1), (0.1, 1), (-np.pi, 1), (-1.0, 0)):
            pts, lab = scanmix.mix_scan_host(p1, l1, p2, l2, _polar(alpha, swap), OMEGA, atan=atan)
            want, want_lab = _by_hand(p1, l1, p2, l2, alpha, swap, atan)
            assert pts.dtype == np.float32 and lab.dtype == np.int64 and np.array_equal(lab, want_lab), (what, alpha)
            assert np.allclose(pts, want, rtol=0, atol=1e-5), (what, alpha)
            n_inst = int(np.isin(l2, scanmix.INSTANCE_CLASSES).sum())
            assert (n_inst == 0) == (what == "no instances")
            if n_inst:
                assert sc.same_bits(pts[-3 * n_inst:-2 * n_inst], np.ascontiguousarray(want[-3 * n_inst:-2 * n_inst]))
    l2 = cases["no instances"]
    # alpha = 0.1: the sector (0.1, 0.1 + pi) holds all of scan 1: only scan 2's sector rows are left
    pts, lab = scanmix.mix_scan_host(p1, l1, p2, l2, _polar(0.1), OMEGA, atan=atan)
    in2 = scanmix.sector_mask(p2, 0.1, atan)
    assert scanmix.sector_mask(p1, 0.1, atan).all() and 0 < in2.sum() < 70 and sc.same_bits(pts, p2[in2])
    # an empty sector: scan 2 has no row inside, scan 1 none either -> scan 1 unchanged
    half = p2[~scanmix.sector_mask(p2, -3.0, atan)]
    p1_out = p1[~scanmix.sector_mask(p1, -3.0, atan)]
    assert len(half) and len(p1_out)
    pts, lab = scanmix.mix_scan_host(p1_out, l1[:len(p1_out)], half, l2[:len(half)], _polar(-3.0), OMEGA, atan=atan)
    assert sc.same_bits(pts, p1_out)
    # paste off
    pts, lab = scanmix.mix_scan_host(p1, l1, p2, cases["mixed"], _polar(-1.0, 0, 0), OMEGA, atan=atan)
    assert sc.same_bits(pts, p1)


@pytest.mark.parametrize("atan", ATANS)
def test_a_yaw_equal_to_the_edge_is_outside(atan):
    """Both inequalities are strict and run in float32: a row whose yaw IS float32(alpha) or float32(beta) stays where it was."""
    p = np.array([[3.0, 3.0, 0.0, 0.5], [3.0, 2.9999, 0.0, 0.6], [-2.0, -7.0, 0.1, 0.7]], dtype=np.float32)
    yaw = -scanmix._arctan2_f32(p[:, 1], p[:, 0], atan)
    alpha = float(yaw[0])
    a32, b32 = scanmix.sector_edges(alpha)
    assert a32 == yaw[0] and yaw[1] > a32 and a32 < yaw[2] < b32
    assert scanmix.sector_mask(p, alpha, atan).tolist() == [False, True, True]
    lab = np.array([11, 12, 13])
    pts, out = scanmix.mix_scan_host(p, lab, p[::-1].copy(), lab[::-1].copy(), _polar(alpha), OMEGA, atan=atan)
    assert out.tolist() == [11, 13, 12] and sc.same_bits(pts, p[[0, 2, 1]])
    # the upper edge: alpha chosen so that float32(alpha + pi) is a row's yaw
    beta_alpha = float(yaw[2]) - np.pi
    while np.float32(beta_alpha + np.pi) > yaw[2]:
        beta_alpha = np.nextafter(beta_alpha, -10.0)
    assert scanmix.sector_edges(beta_alpha)[1] == yaw[2]
    assert scanmix.sector_mask(p, beta_alpha, atan).tolist() == [True, True, False]


def test_sector_membership_of_the_two_arctan2_rules():
    """The one allowance against the reference's arithmetic, bounded: see the module's text."""
    scans = [make_scan(0), make_scan(1)]
    tested = differ = 0
    for alpha in (-3.0, -1.7, -0.25):
        for p in scans:
            differ += int((scanmix.sector_mask(p, alpha, "numpy32") != scanmix.sector_mask(p, alpha, "double")).sum())
            tested += p.shape[0]
    print("sector membership differs in %d of %d rows" % (differ, tested))
    assert tested == 720000 and differ <= 1e-6 * tested
    ulp = np.mean(np.arctan2(scans[0][:, 1], scans[0][:, 0]) != scanmix._arctan2_f32(scans[0][:, 1], scans[0][:, 0], "double"))
    assert 0.05 < ulp < 0.6   # the two rules do differ, often: the sector test just rarely notices


@pytest.mark.parametrize("atan", ATANS)
def test_ring_ids_by_hand(atan):
    """The ring advances where the azimuth wraps from proj_x > 0.8 to proj_x < 0.2; row 0 never advances; 63 is the cap."""
    az = np.tile(np.linspace(-3.0, 3.0, 7), 70)   # 70 sweeps of seven rows
    p = np.stack([np.cos(az), np.sin(az), np.zeros_like(az), np.zeros_like(az)], axis=1).astype(np.float32)
    ring = scanmix.ring_ids_host(p, atan)
    assert ring.dtype == np.float32 and ring.shape == (490,)
    yaw = -np.arctan2(p[:, 1].astype(np.float64), -p[:, 0].astype(np.float64))
    proj = 0.5 * (yaw / np.pi + 1)
    want = np.clip(np.cumsum(np.r_[0, (proj[1:] < 0.2) & (proj[:-1] > 0.8)]), 0, 63)
    assert np.array_equal(ring, want.astype(np.float32)) and ring[0] == 0 and ring.max() == 63 and (np.diff(ring) >= 0).all()
    assert len(np.unique(ring)) == 64
    assert scanmix.ring_ids_host(p[:1], atan).tolist() == [0.0] and scanmix.ring_ids_host(p[:0], atan).shape == (0,)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_host_refusals():
    rng = np.random.default_rng(1)
    p, lab = _ring_scan(20, rng), rng.integers(0, 20, size=20)
    ok = _polar(-1.0)
    for bad in (np.zeros((20, 5), dtype=np.float32), np.zeros((20, 3), dtype=np.float32), np.zeros(20, dtype=np.float32)):
        with pytest.raises(ValueError, match=r"\(n, 4\)"):
            scanmix.mix_scan_host(bad, lab, p, lab, ok, OMEGA)
        with pytest.raises(ValueError, match=r"\(n, 4\)"):
            scanmix.mix_scan_host(p, lab, bad, lab, ok, OMEGA)
    with pytest.raises(ValueError, match="instance classes"):
        scanmix.mix_scan_host(p, lab, p, lab, ok, OMEGA, instance_classes=range(9))
    for classes in ((1, 256), (-1, 2), (3, 3)):
        with pytest.raises(ValueError, match="instance classes"):
            scanmix.mix_scan_host(p, lab, p, lab, ok, OMEGA, instance_classes=classes)
    for row in ([0, -1.0, 1], [0, -1.0, 1, 1, 0], [2, 0, 0, 0], [1, 4, 0, 0]):
        with pytest.raises(ValueError, match="plan"):
            scanmix.mix_scan_host(p, lab, p, lab, row, OMEGA)
    with pytest.raises(ValueError, match="omega"):
        scanmix.mix_scan_host(p, lab, p, lab, ok, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="atan"):
        scanmix.mix_scan_host(p, lab, p, lab, ok, OMEGA, atan="float")
    with pytest.raises(ValueError, match="lasermix"):
        scanmix.mix_scan_host(p, lab, p, lab, ok, OMEGA, lasermix="degrees")
    with pytest.raises(ValueError, match="one label per point"):
        scanmix.mix_scan_host(p, lab[:-1], p, lab, ok, OMEGA)
    # a mixed frame that comes out empty: all of scan 1 inside the sector, nothing of scan 2, no instances
    inside = p[scanmix.sector_mask(p, -1.0)]
    outside = p[~scanmix.sector_mask(p, -1.0)]
    with pytest.raises(ValueError, match="no rows"):
        scanmix.mix_scan_host(inside, np.full(len(inside), 12), outside, np.full(len(outside), 12), ok, OMEGA)
    with pytest.raises(ValueError, match="no rows"):
        scanmix.mix_scan_host(p[:0], lab[:0], p, np.full(20, 12), [scanmix.NO_MIX, 0, 0, 0], OMEGA)
    with pytest.raises(ValueError):
        scanmix.ring_ids_host(np.zeros(5, dtype=np.float32))
    import torch
    raw = {"points": torch.zeros(4, 4), "labels": torch.zeros(4, dtype=torch.int64), "offsets": [0, 4], "num_frames": 1}
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        scanmix.device_mix(raw, raw, [ok], OMEGA)


def test_partner_raw_batch():
    raw, partner = make_raw_batch([1, 2], 500), make_partner_raw_batch([1, 2], 500)
    assert partner["num_frames"] == raw["num_frames"] == 2 and partner["offsets"] == raw["offsets"] and partner["points"].shape == (1000, 4)
    assert not np.array_equal(partner["points"].numpy(), raw["points"].numpy())
    again = make_partner_raw_batch([1, 2], 500)
    assert np.array_equal(again["points"].numpy(), partner["points"].numpy()) and np.array_equal(again["labels"].numpy(), partner["labels"].numpy())
    assert np.array_equal(partner["points"].numpy(), make_raw_batch([1001, 1002], 500)["points"].numpy())
    assert np.isin(partner["labels"].numpy(), scanmix.INSTANCE_CLASSES).any()


def test_device_plan_rows():
    plan = np.array([[scanmix.POLARMIX, -1.25, 1, 1], [scanmix.LASERMIX, 2, 0, 0], [scanmix.NO_MIX, 0, 0, 0]], dtype=np.float64)
    ref = scanmix.device_plan(plan, "reference")
    assert ref.shape == (3, scanmix.PLAN_STRIDE) and ref.dtype == np.float64
    assert ref[0, :5].tolist() == [1.0, float(np.float32(-1.25)), float(np.float32(-1.25 + np.pi)), 1.0, 1.0] and not ref[1:].any()
    rad = scanmix.device_plan(plan, "radians")
    assert rad[1, 0] == 2 and rad[1, 5] == 4 and np.array_equal(rad[1, 6:10], np.array([-4.0, -8.0, -12.0, -16.0]) * np.pi / 180) and not rad[2].any()


# ---- the C entries -----------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    assert re.search(r"\bint64_t pcs_scan_mix_ws_bytes\(int64_t n1, int64_t n2, int32_t num_frames\);", hdr)
    assert re.search(r"\bint pcs_scan_mix_count\(const float \*points1, int64_t n1, const int64_t \*frame_offsets1,", hdr)
    assert re.search(r"\bint pcs_scan_mix_place\(const float \*points1, const int64_t \*labels1, int64_t n1,", hdr)
    assert re.search(r"\bint64_t pcs_scan_ring_ws_bytes\(int64_t m\);", hdr)
    assert re.search(r"\bint pcs_scan_ring_f32\(float \*points, int64_t m, int32_t c, const int64_t \*frame_base,", hdr)
    assert re.search(r"#define PCS_ABI_VERSION 12\b", hdr)
    for name, value in (("PCS_MIX_BUCKETS", 10), ("PCS_MIX_MAX_CLASSES", scanmix.MAX_CLASSES), ("PCS_MIX_PLAN_STRIDE", scanmix.PLAN_STRIDE)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr)
    lib = native.load_library()   # dlopen works without a GPU
    for name in ENTRIES:
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12


def test_size_only_refusals():
    """Sizes are checked before any pointer is looked at, so the refusals need no device."""
    lib = native.load_library()
    assert lib.pcs_scan_mix_ws_bytes(1440000, 1440000, 12) == 12 * (1024 // 12) * 10 * 4
    assert lib.pcs_scan_mix_ws_bytes(1, 0, 1) == 40 and lib.pcs_scan_mix_ws_bytes(0, 0, 3) == 120
    bad_sizes = ((-1, 8, 1), (8, -1, 1), (8, 8, 0), (8, 8, 65536), (2 ** 31, 8, 1), (8, 2 ** 29, 1))
    for n1, n2, f in bad_sizes:
        assert lib.pcs_scan_mix_ws_bytes(n1, n2, f) == -1, (n1, n2, f)
    count = lambda n1, n2, f, k=8: lib.pcs_scan_mix_count(None, n1, None, None, None, n2, None, f, None, None, k, None, 0, None, None, None)
    place = lambda n1, n2, f, k=8, m=8, c=4: lib.pcs_scan_mix_place(None, None, n1, None, None, None, n2, None, f, None, None, k, None, None, 0, None,
                                                                     None, m, c, None, None, None)
    for call in (count, place):
        for n1, n2, f in bad_sizes:
            assert call(n1, n2, f) == -1 and b"bad args" in lib.pcs_last_error(), (n1, n2, f)
        for k in (-1, 9):
            assert call(8, 8, 1, k) == -1 and b"bad args" in lib.pcs_last_error()
        assert call(8, 8, 1) == -1 and b"null pointer" in lib.pcs_last_error()
    for m, c in ((-1, 4), (8 + 4 * 8 + 1, 4), (8, 3), (8, 9)):
        assert place(8, 8, 1, 8, m, c) == -1 and b"bad args" in lib.pcs_last_error(), (m, c)
    ring = lambda m, c, f: lib.pcs_scan_ring_f32(None, m, c, None, f, None, 0, None)
    for m, c, f in ((-1, 5, 1), (2 ** 31, 5, 1), (8, 4, 1), (8, 9, 1), (8, 5, 0), (8, 5, 65536)):
        assert ring(m, c, f) == -1 and b"bad args" in lib.pcs_last_error(), (m, c, f)
    assert ring(8, 5, 1) == -1 and b"null pointer" in lib.pcs_last_error()
    assert ring(0, 5, 1) == 0   # no rows: nothing to do
    assert lib.pcs_scan_ring_ws_bytes(-1) == -1 and lib.pcs_scan_ring_ws_bytes(2 ** 31) == -1 and lib.pcs_scan_ring_ws_bytes(0) == 0
