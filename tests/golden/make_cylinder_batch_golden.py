"""Generate tests/golden/cylinder_batch_golden.npz: the reference's cylinder dataset on two small frames, training and TTA.

Needs the reference's sources (so it runs where they are present; the .npz is committed). It RUNS, unmodified,
  SemkittiCylinderDataset.get_single_sample   R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:104-174
  collate_batch / collate_batch_tta           R:...semantickitti_cylinder.py:176-265
(and through them aug_points, R:tools/utils/common/seg_utils.py:43-100, and the reference's sparse_quantize). The class is
instantiated without its __init__ (which wants the dataset on disk) and `np.int`, removed from NumPy >= 1.24 and still used by the
reference, is aliased to `int`, as `make_golden.py cylinder` does. The only stand-in is the point-cloud dataset behind it: a list-like
that hands out a fresh copy of a frame on every access, as reading a scan from disk does (get_single_sample augments in place).

Input: the two frames of make_transform_golden.make_frames() (512 and 301 rows, four columns) with random labels, 5 % of them the
label 67 that voxelize_with_label does not count. Grid (120, 90, 16) over [0, -180, -4] .. [50, 180, 2], scale range (0.95, 1.05)
(the cylinder dataset's default), twenty classes.
Recorded, each with the NumPy seed it ran under:
  train_*   collate_batch of the two frames in the training branch (all four augmentations on), one worker seed;
  tta<f>_*  collate_batch_tta of the ten votes of frame f, in __getitem__ order: all votes of frame 0, then all votes of frame 1,
            under ONE seed (the draws run on from frame 0 to frame 1).
Float arrays are stored transposed (column-major packs better), integers as int16 / int8 where they fit. Data only.

    python tests/golden/make_cylinder_batch_golden.py
"""
import importlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, OUT)

LO, HI, GRID = [0, -180, -4], [50, 180, 2], [120, 90, 16]
SCALE_RANGE = [0.95, 1.05]
TRAIN_SEED, TTA_SEED = 31, 41
NUM_CLASSES = 20
FLOATS = ("point_feature", "voxel_feature")
INTS = {"point_coord": np.int16, "voxel_coord": np.int16, "point_label": np.int8, "voxel_label": np.int8,
        "inverse_map": np.int16, "num_points": np.int16, "offset": np.int16}


class FreshFrames:
    """What the reference's SemantickittiDataset is to the cylinder dataset: index -> {"labels", "xyzret", "path"}, read anew."""

    def __init__(self, frames, labels):
        self.frames, self.labels = frames, labels

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return {"labels": self.labels[i].copy(), "xyzret": self.frames[i].copy(), "path": "frame%d" % i}


def make_labels(frames):
    out = []
    for f, frame in enumerate(frames):
        rng = np.random.default_rng(100 + f)
        lab = rng.integers(0, NUM_CLASSES, size=frame.shape[0]).astype(np.int64)
        lab[rng.random(frame.shape[0]) < 0.05] = 67
        out.append(lab)
    return out


def make_dataset(mod, frames, labels, training, tta):
    ds = object.__new__(mod.SemkittiCylinderDataset)
    ds.training, ds.if_tta = training, tta
    ds.class_names = ["c%d" % i for i in range(NUM_CLASSES)]
    ds.cylinder_space_max, ds.cylinder_space_min, ds.grid_size = np.array(HI), np.array(LO), np.array(GRID)
    ds.if_flip = ds.if_scale = ds.if_jitter = ds.if_rotate = True
    ds.scale_axis, ds.scale_range = "xyz", list(SCALE_RANGE)
    ds.point_cloud_dataset = FreshFrames(frames, labels)
    return ds


def pack(prefix, batch, out):
    for k in FLOATS:
        a = batch[k].numpy()
        assert a.dtype == np.float32
        out[prefix + k] = np.ascontiguousarray(a.T)
    for k, dt in INTS.items():
        a = batch[k].numpy()
        assert np.array_equal(a.astype(dt).astype(a.dtype), a), k
        out[prefix + k] = np.ascontiguousarray(a.astype(dt).T)


def main():
    import make_golden
    from make_transform_golden import make_frames, state_digest
    make_golden.import_reference_torchsparse()
    make_golden.import_reference_minkunet()   # import stand-ins + sys.path for the reference tree
    if not hasattr(np, "int"):
        np.int = int
    mod = importlib.import_module("pcseg.data.dataset.semantickitti.semantickitti_cylinder")
    frames = [f.astype(np.float32) for f in make_frames()]
    labels = make_labels(frames)
    out = {"cfg": np.array([LO, HI, GRID], dtype=np.int64), "scale_range": np.array(SCALE_RANGE), "train_seed": np.int64(TRAIN_SEED),
           "tta_seed": np.int64(TTA_SEED), "num_classes": np.int64(NUM_CLASSES), "labels_f0": labels[0].astype(np.int8),
           "labels_f1": labels[1].astype(np.int8)}
    # training: one worker seed, the frames of the batch one after the other
    ds = make_dataset(mod, frames, labels, training=True, tta=False)
    np.random.seed(TRAIN_SEED)
    pack("train_", ds.collate_batch([ds[0], ds[1]]), out)
    out["train_state_after"], out["train_pos_after"] = state_digest()
    # test-time augmentation: __getitem__ runs the ten votes of one index, then the loader moves to the next index
    ds = make_dataset(mod, frames, labels, training=False, tta=True)
    np.random.seed(TTA_SEED)
    for f in range(2):
        votes = ds[f]
        assert len(votes) == 10
        pack("tta%d_" % f, ds.collate_batch_tta([votes]), out)
    out["tta_state_after"], out["tta_pos_after"] = state_digest()
    path = os.path.join(OUT, "cylinder_batch_golden.npz")
    make_golden.save_npz_stable(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
