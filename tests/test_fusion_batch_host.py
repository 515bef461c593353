"""The fusion (RPVNet) dataset's batch on the host: the composition the device path is built from --
transform.transform_scan_host (the float64 affine map, one rounding), hostdata.sparse_quantize, rangeview.range_view_host in the
reference's own arithmetic, concatenation with the scene column -- reproduces tests/golden/fusion_batch_golden.npz bit for bit. The
fixture comes from RUNNING the reference's SemkittiFusionDataset.get_single_sample and collate_batch / collate_batch_tta
(tests/golden/make_fusion_batch_golden.py); the parameter tables and cuts come from rangeview's drawers under its seeds."""
import hashlib
import os
import re

import numpy as np
import pytest

import fusion_cases as fc
from openpcseg_amd import native, rangeview

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcs_range_project_ws_bytes", "pcs_range_project_f32", "pcs_range_image_fill_f32")


@pytest.fixture(scope="module")
def gold():
    return fc.load_gold()


def _digest():
    st = np.random.get_state()
    return hashlib.sha256(np.ascontiguousarray(st[1], dtype=np.uint32).tobytes()).digest(), int(st[2])


def _drawn(gold, which):
    np.random.seed(fc.scalar(gold[which + "_seed"]))
    scale = tuple(gold["scale_range"])
    tables = rangeview.draw_train_params(2, scale_range=scale) if which == "train" else rangeview.tta_params(2, 10, scale_range=scale)
    return tables, _digest()


@pytest.mark.parametrize("which", ["train", "tta"])
def test_drawers_give_the_reference_tables_and_generator_state(gold, which):
    (params, cuts), (sha, pos) = _drawn(gold, which)
    assert params.dtype == cuts.dtype == np.float64
    assert np.array_equal(params, gold[which + "_params"]) and np.array_equal(cuts, gold[which + "_cuts"])
    assert sha == gold[which + "_state_after"].tobytes() and pos == fc.scalar(gold[which + "_pos_after"])
    assert ((cuts >= 0) & (cuts < 1)).all() and len(set(cuts.tolist())) == cuts.shape[0]   # one draw of its own per scene


def test_drawers_accept_a_generator_of_their_own(gold):
    a = rangeview.tta_params(2, 10, scale_range=tuple(gold["scale_range"]), rng=np.random.RandomState(fc.scalar(gold["tta_seed"])))
    assert np.array_equal(a[0], gold["tta_params"]) and np.array_equal(a[1], gold["tta_cuts"])
    with pytest.raises(ValueError):
        rangeview.tta_params(1, 11)


def test_training_batch_reproduces_the_reference(gold):
    scans, labels = fc.frames_and_labels(gold)
    hw = tuple(int(v) for v in gold["hw"])
    batch = fc.host_batch(scans, labels, gold["train_params"], gold["train_cuts"], fc.scalar(gold["voxel_size"]), hw, "numpy32")
    fc.assert_equals_fixture(gold, "train_", batch)
    assert batch["range_image"].shape == (2, 5, 64, 2048)


def test_tta_batches_reproduce_the_reference(gold):
    scans, labels = fc.frames_and_labels(gold)
    hw = tuple(int(v) for v in gold["hw"])
    for f in range(2):   # vote-major tables: row v * 2 + f
        batch = fc.host_batch([scans[f]] * 10, [labels[f]] * 10, gold["tta_params"][f::2], gold["tta_cuts"][f::2], fc.scalar(gold["voxel_size"]),
                              hw, "numpy32")
        fc.assert_equals_fixture(gold, "tta%d_" % f, batch)
        assert len({batch["range_image"][v].tobytes() for v in range(10)}) == 10   # every vote has a view of its own


def test_fixture_has_no_face_case(gold):
    """The kernel's arctan2 (a double one rounded once) gives every recorded scene the reference's bits: the seed guard."""
    scans, labels = fc.frames_and_labels(gold)
    hw = tuple(int(v) for v in gold["hw"])
    batch = fc.host_batch(scans, labels, gold["train_params"], gold["train_cuts"], fc.scalar(gold["voxel_size"]), hw, "double")
    fc.assert_equals_fixture(gold, "train_", batch)


def _rows(xy_ring, z=0.5):
    """rows [x, y, z, reflectivity = row / 100, ring] from (x, y, ring) triples."""
    out = np.zeros((len(xy_ring), 5), dtype=np.float32)
    for i, (x, y, ring) in enumerate(xy_ring):
        out[i] = (x, y, z, i / 100.0, ring)
    return out


@pytest.mark.parametrize("atan", ["numpy32", "double"])
def test_last_row_wins_a_collision(atan):
    pts = _rows([(-10.0, 1.0, 3), (-20.0, 2.0, 3), (-10.0, 1.0, 7), (-30.0, 3.0, 3)])   # rows 0, 1, 3: one azimuth, one ring
    image, pxpy = rangeview.range_view_host(pts, 0.5, atan=atan)
    assert image.shape == (5, 64, 2048) and image.dtype == np.float32 and pxpy.shape == (4, 2) and pxpy.dtype == np.float64
    assert np.array_equal(pxpy[0], pxpy[1]) and np.array_equal(pxpy[0], pxpy[3]) and pxpy[2, 0] == pxpy[0, 0] and pxpy[2, 1] != pxpy[0, 1]
    ix = int(round((pxpy[0, 0] / 2 + 0.5) * 2047))
    assert np.array_equal(image[2:, 3, ix], pts[3, :3]) and np.array_equal(image[2:, 7, ix], pts[2, :3])
    depth = np.linalg.norm(pts[3, :3].astype(np.float32))
    assert image[0, 3, ix] == np.float32(25 * (np.float64(np.float32(1.0) / depth) - 0.4))
    assert image[1, 3, ix] == np.float32(20 * (np.float64(pts[3, 3]) - 0.5))
    hit = (image != fc.EMPTY[:, None, None]).any(0)
    assert int(hit.sum()) == 2 and np.array_equal(image[:, 0, 0], fc.EMPTY)


@pytest.mark.parametrize("atan", ["numpy32", "double"])
def test_yaw_that_wraps_to_two_pi_lands_on_the_last_column(atan):
    """A yaw of -1e-9 in front of the remainder becomes exactly float32(2 pi) (NumPy's remainder adds the divisor to fmodf's
    negative result, and the sum rounds up), so the row lands on column W - 1; its mirror image at +1e-9 lands on column 0."""
    assert np.float32(-1e-9) % np.float32(2 * np.pi) == np.float32(2 * np.pi)
    assert np.float32(2 * np.pi) - np.float32(np.pi) == np.float32(np.pi)
    pts = _rows([(-5.0, -5e-9, 0), (-5.0, 5e-9, 1)])   # atan2(y, -x) = -1e-9 and +1e-9; no cut
    for hw in ((64, 2048), (4, 126)):
        _, pxpy = rangeview.range_view_host(pts, 0.5, hw, atan=atan)
        assert pxpy[:, 0].tolist() == [1.0, -1.0]   # columns W - 1 and 0
        assert pxpy[:, 1].tolist() == [-1.0, 2.0 * (1 / (hw[0] - 1) - 0.5)]


def test_cut_is_rounded_once_from_float64():
    u = 0.123456789
    assert rangeview.cut_value(u) == np.float32((u - 0.5) * 2 * np.pi) and rangeview.cut_value(u).dtype == np.float32
    assert rangeview.cut_value(0.5) == 0 and rangeview.cut_value([0.0])[0] == np.float32(-np.pi)


def test_host_refusals():
    with pytest.raises(ValueError):
        rangeview.range_view_host(np.zeros((3, 4), dtype=np.float32), 0.5)
    for ring in (64.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            rangeview.range_view_host(_rows([(1.0, 2.0, ring)]), 0.5)
    with pytest.raises(ValueError):
        rangeview.range_view_host(_rows([(np.nan, 2.0, 1)]), 0.5)
    import torch
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        rangeview.device_batch({"points": torch.zeros(4, 5), "labels": torch.zeros(4), "offsets": [0, 4], "num_frames": 1})


def test_fusion_raw_batch_carries_the_ring():
    from openpcseg_amd.workloads.synthetic import N_AZ, make_fusion_raw_batch, make_raw_batch
    for n_points in (None, 2000):
        plain, raw = make_raw_batch([1, 2], n_points), make_fusion_raw_batch([1, 2], n_points)
        assert raw["points"].shape[1] == 5 and np.array_equal(raw["points"][:, :4].numpy(), plain["points"].numpy())
        assert raw["offsets"] == plain["offsets"] and np.array_equal(raw["labels"].numpy(), plain["labels"].numpy())
        ring = raw["points"][:, 4].numpy()
        assert ring.min() == 0 and ring.max() == 63 and np.array_equal(ring[:raw["offsets"][1]], ring[raw["offsets"][1]:])
        assert (np.diff(ring[:raw["offsets"][1]]) >= 0).all()
    full = make_fusion_raw_batch([0])["points"].numpy()
    assert np.array_equal(full[:, 4], (np.arange(full.shape[0]) // N_AZ).astype(np.float32))
    # the elevation of a ray decides its ring: z / range is constant along a ring up to the range noise
    el = np.arctan2(full[:, 2], np.hypot(full[:, 0], full[:, 1]))
    assert abs(np.corrcoef(el, full[:, 4])[0, 1]) > 0.99


def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    assert re.search(r"\bint64_t pcs_range_project_ws_bytes\(int32_t num_scenes, int32_t H, int32_t W\);", hdr)
    assert re.search(r"\bint pcs_range_project_f32\(const float \*feats, int64_t n, int32_t c, const int32_t \*scenes, const float \*cuts32,", hdr)
    assert re.search(r"\bint pcs_range_image_fill_f32\(const int32_t \*winner, const float \*feats, int64_t n, int32_t c,", hdr)
    assert re.search(r"#define PCS_ABI_VERSION 12\b", hdr)
    lib = native.load_library()   # dlopen works without a GPU
    for name in ENTRIES:
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12


def test_size_only_refusals():
    """Sizes are checked before any pointer is looked at, so the refusals need no device."""
    lib = native.load_library()
    assert lib.pcs_range_project_ws_bytes(12, 64, 2048) == 12 * 64 * 2048 * 4
    assert lib.pcs_range_project_ws_bytes(1, 4, 126) == 4 * 126 * 4
    for s, h, w in ((0, 64, 2048), (-1, 64, 2048), (1, 1, 2048), (1, 64, 1), (1, 64, 0), (4096, 1024, 1024), (2, 32768, 32768)):
        assert lib.pcs_range_project_ws_bytes(s, h, w) == -1, (s, h, w)
    project = lambda n, c, s, h, w: lib.pcs_range_project_f32(None, n, c, None, None, s, h, w, None, None, None, None)
    fill = lambda n, c, s, h, w: lib.pcs_range_image_fill_f32(None, None, n, c, s, h, w, None, None)
    for call in (project, fill):
        for n, c, s, h, w in ((8, 4, 1, 64, 2048), (8, 5, 0, 64, 2048), (8, 5, 1, 1, 2048), (8, 5, 1, 64, 1), (8, 5, 2, 32768, 32768),
                              (-1, 5, 1, 64, 2048), (2 ** 31, 5, 1, 64, 2048)):
            assert call(n, c, s, h, w) == -1, (n, c, s, h, w)
            assert b"bad args" in lib.pcs_last_error()
        assert call(8, 5, 1, 64, 2048) == -1 and b"null pointer" in lib.pcs_last_error()
        assert call(0, 5, 1, 64, 2048) == -1 and b"null pointer" in lib.pcs_last_error()   # the winner is cleared even for no rows
