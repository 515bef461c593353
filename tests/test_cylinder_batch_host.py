"""The cylinder dataset's batch on the host: the composition the device path is built from --
transform.transform_scan_host (the float64 affine map, one rounding), oracle.cylinder_partition, oracle.voxelize_with_label,
concatenation with the scene column -- reproduces tests/golden/cylinder_batch_golden.npz bit for bit. The fixture comes from RUNNING
the reference's own SemkittiCylinderDataset.get_single_sample and collate_batch / collate_batch_tta
(tests/golden/make_cylinder_batch_golden.py); the parameter tables come from draw_train_params / tta_params under its seeds."""
import os
import re

import numpy as np
import pytest

from openpcseg_amd import native, transform
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KEYS = ("point_feature", "voxel_feature", "point_coord", "voxel_coord", "point_label", "voxel_label", "inverse_map", "num_points",
        "offset")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "cylinder_batch_golden.npz"))


def _int(a):
    return int(np.asarray(a).reshape(-1)[0])


def frames_and_labels(gold):
    """The fixture's input: make_transform_golden.make_frames() restated (the frames are cut from workloads.synthetic.make_scan
    and carry the hand-placed half-voxel rows of tests/golden/transform_golden.npz), and the recorded labels."""
    t = np.load(os.path.join(HERE, "golden", "transform_golden.npz"))
    return [t["frame0"].astype(np.float32), t["frame1"].astype(np.float32)], [gold["labels_f0"].astype(np.int64), gold["labels_f1"].astype(np.int64)]


def host_batch(scans, labels, rows, cfg, num_classes):
    """collate_batch over get_single_sample of `scans[k]` under parameter row `rows[k]`, scene k, on the host."""
    lo, hi, grid = (c.tolist() for c in cfg)
    parts = {k: [] for k in KEYS}
    for s, (pts, lab, row) in enumerate(zip(scans, labels, rows)):
        aug, _ = transform.transform_scan_host(pts, row, 0.05)
        _, coord, feat = orc.cylinder_partition(aug, lo, hi, grid)
        vox, vlab, inds, inv = orc.voxelize_with_label(coord, lab, num_classes)
        scene = lambda a: np.concatenate([a.astype(np.int64), np.full((a.shape[0], 1), s, dtype=np.int64)], axis=1)
        for k, v in (("point_feature", feat), ("voxel_feature", feat[inds]), ("point_coord", scene(coord)), ("voxel_coord", scene(vox)),
                     ("point_label", lab), ("voxel_label", vlab), ("inverse_map", inv), ("num_points", np.array([pts.shape[0]])),
                     ("offset", np.array([vox.shape[0]]))):
            parts[k].append(v)
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out["offset"] = np.cumsum(out["offset"])
    return out


def assert_equals_fixture(gold, prefix, batch):
    for k in KEYS:
        ref = gold[prefix + k].T
        got = batch[k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k.endswith("feature"):
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), k   # bit for bit
        else:
            assert np.array_equal(got.astype(np.int64), ref.astype(np.int64)), k


def test_training_batch_reproduces_the_reference(gold):
    scans, labels = frames_and_labels(gold)
    np.random.seed(_int(gold["train_seed"]))
    rows = transform.draw_train_params(2, scale_range=tuple(gold["scale_range"]))
    assert_equals_fixture(gold, "train_", host_batch(scans, labels, rows, gold["cfg"], _int(gold["num_classes"])))


def test_tta_batches_reproduce_the_reference(gold):
    scans, labels = frames_and_labels(gold)
    np.random.seed(_int(gold["tta_seed"]))
    rows = transform.tta_params(2, 10, scale_range=tuple(gold["scale_range"]))   # vote-major: row v * 2 + f
    for f in range(2):
        batch = host_batch([scans[f]] * 10, [labels[f]] * 10, [rows[v * 2 + f] for v in range(10)], gold["cfg"], _int(gold["num_classes"]))
        assert_equals_fixture(gold, "tta%d_" % f, batch)


def test_fixture_is_data_of_the_expected_shape(gold):
    assert gold["cfg"].tolist() == [[0, -180, -4], [50, 180, 2], [120, 90, 16]]
    assert gold["train_num_points"].tolist() == [512, 301]
    for f, n in enumerate((512, 301)):
        assert gold["tta%d_num_points" % f].tolist() == [n] * 10
        assert gold["tta%d_point_feature" % f].shape == (9, 10 * n)
    assert int((gold["labels_f0"] == 67).sum()) > 0   # the label the vote does not count is present


def test_new_entry_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    assert re.search(r"\bint pcs_cylinder_scan_batch_f32\(const float \*points, int64_t n, int32_t c,", hdr)
    assert re.search(r"#define PCS_ABI_VERSION 12\b", hdr)
    assert "pcs_cylinder_scan_batch_f32" in native.SIGNATURES
    lib = native.load_library()   # dlopen works without a GPU
    assert hasattr(lib, "pcs_cylinder_scan_batch_f32")
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12
    # refusals that need no device: sizes, the cylinder space and null pointers are checked before anything is launched
    import ctypes
    lo, hi, grid = (ctypes.c_double * 3)(0, -180, -4), (ctypes.c_double * 3)(50, 180, 2), (ctypes.c_int32 * 3)(120, 90, 16)
    call = lambda n, c, frames, votes, lo=lo, hi=hi, grid=grid: lib.pcs_cylinder_scan_batch_f32(None, n, c, None, frames, None, votes, lo, hi, grid,
                                                                                              None, None, None, None)
    assert call(0, 4, 1, 1) == 0                      # n == 0: nothing to do
    for n, c, frames, votes in ((-1, 4, 1, 1), (0, 2, 1, 1), (0, 9, 1, 1), (0, 4, 0, 1), (0, 4, 65536, 1), (0, 4, 1, 0), (0, 4, 1, 17)):
        assert call(n, c, frames, votes) != 0, (n, c, frames, votes)
    assert call(0, 4, 1, 1, grid=(ctypes.c_int32 * 3)(120, 1, 16)) != 0
    assert call(0, 4, 1, 1, hi=(ctypes.c_double * 3)(50, -180, 2)) != 0
    assert call(0, 4, 1, 1, lo=None) != 0
    assert call(8, 4, 1, 1) != 0 and b"null pointer" in lib.pcs_last_error()
