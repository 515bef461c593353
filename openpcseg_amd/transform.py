"""The dataset transform of the reference's voxel datasets for scans resident in HBM: training
augmentation, the ten votes of test-time augmentation, and the evaluation side of a batch.

  aug_points            R:tools/utils/common/seg_utils.py:43-100 (rotate, scale, flip, jitter)
  get_single_sample     R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:74-142
  collate_batch(_tta)   R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:144-164

All of it is one affine map per (vote, frame), eight numbers (cos, sin, scale, sx, sy, jx, jy, jz), applied in float64 in the
reference's order and association, rounded ONCE to float32 (that value is also the voxel's feature: the reference sets `feat_ =
point` after the augmentation), divided by the voxel size in float32, rounded half to even, cast to int32 and shifted by the
frame's minimum. `draw_train_params` / `tta_params` draw the eight numbers from a NumPy generator in the reference's call order,
`transform_scan_host` is the arithmetic in NumPy (the host path, and the yardstick of csrc/scantransform.hip), `device_batch` runs
it on the device for every vote from one read of the scans and hands back what `collate_batch` / `collate_batch_tta` would.
What a raw batch is, and the host bookkeeping shared with the other device builders (`raw_frames`, `scene_row_offsets`,
`scene_points`, `vote_labels`), is hostdata.py's; `_tta_draws` is the one loop behind this module's and rangeview.py's `tta_params`.

The float64 contract is the reference's arithmetic with the rotation ON (every shipped config): without a rotation aug_points
never leaves float32 (a float32 array times a Python float stays float32 in NumPy), which this module does not restate.
"""
import numpy as np
import torch

from .hostdata import raw_frames, scene_points, scene_row_offsets, sparse_quantize_frames, vote_labels
from .sparse import SparseTensor

__all__ = ["TTA_ANGLES", "identity_params", "draw_train_params", "tta_params", "transform_scan_host", "device_batch"]

# R:tools/utils/common/seg_utils.py:58-60: the rotation of vote k is TTA_ANGLES[k] * pi / 8
TTA_ANGLES = (0, 1, -1, 2, -2, 6, -6, 7, -7, 8)
_FLIPS = ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))   # flip_type 0..3 -> (sx, sy), seg_utils.py:84-89


def identity_params(rows):
    """(rows, 8) float64 parameter rows of the identity map: (1, 0, 1, 1, 1, 0, 0, 0)."""
    out = np.zeros((rows, 8), dtype=np.float64)
    out[:, [0, 2, 3, 4]] = 1.0
    return out


def draw_train_params(num_frames, rng=np.random, rotate=True, scale=True, scale_range=(0.9, 1.1), flip=True, jitter=True):
    """(num_frames, 8) float64: one training augmentation per frame, drawn from `rng` (the `numpy.random` module or a RandomState)
    in exactly aug_points' call order -- uniform(0, 2 pi), uniform(lo, hi), choice(4, 1), three normal(0, 0.1, 1) --, so the seed
    that a worker of the reference's loader runs under gives the same augmentation here."""
    out = identity_params(num_frames)
    for f in range(num_frames):
        if rotate:
            theta = rng.uniform(0, 2 * np.pi)
            out[f, 0], out[f, 1] = np.cos(theta), np.sin(theta)
        if scale:
            out[f, 2] = rng.uniform(scale_range[0], scale_range[1])
        if flip:
            out[f, 3], out[f, 4] = _FLIPS[int(rng.choice(4, 1)[0])]
        if jitter:
            out[f, 5:8] = [rng.normal(0, 0.1, 1)[0], rng.normal(0, 0.1, 1)[0], rng.normal(0, 0.1, 1)[0]]
    return out


def tta_params(num_frames, num_votes=10, scale_range=(0.9, 1.1), rng=np.random):
    """(num_votes * num_frames, 8) float64, vote-major (row v * num_frames + f): vote v rotates by TTA_ANGLES[v] * pi / 8 and
    draws a scale of its own; no flip, no jitter. The draws are consumed frame by frame, a frame's votes in order, as the
    reference's loader visits them (semantickitti_voxel.py:62-69: all votes of one index before the next).
    The TTA branch (semantickitti_voxel.py:94-110) sets `scale_aug_range = [0.95, 1.05]` but passes `scale_range`: the range the
    reference actually scales by is the CONFIGURED one, and that behaviour is kept -- `scale_range` here is that configured range."""
    return _tta_draws(num_frames, num_votes, scale_range, rng, cut=False)[0]


def _tta_draws(num_frames, num_votes, scale_range, rng, cut):
    """The draws of test-time augmentation, for tta_params here and in rangeview.py -> (params, cuts), vote-major. The order is
    the contract: frame by frame, vote by vote, the vote's scale and -- cut: the fusion dataset -- ONE rng.rand() behind it."""
    if not 1 <= num_votes <= len(TTA_ANGLES):
        raise ValueError("openpcseg_amd: test-time augmentation has %d rotations, got num_votes=%d" % (len(TTA_ANGLES), num_votes))
    params = identity_params(num_votes * num_frames)
    cuts = np.empty(num_votes * num_frames if cut else 0, dtype=np.float64)
    for f in range(num_frames):
        for v in range(num_votes):
            theta = TTA_ANGLES[v] * np.pi / 8.0
            row = params[v * num_frames + f]
            row[0], row[1] = np.cos(theta), np.sin(theta)
            row[2] = rng.uniform(scale_range[0], scale_range[1])
            if cut:
                cuts[v * num_frames + f] = rng.rand()
    return params, cuts


def transform_scan_host(points, params_row, voxel_size):
    """One scan under one parameter row, in NumPy: points (n, C >= 3) float32 -> (the augmented points (n, C) float32, the
    shifted voxel coordinates (n, 3) int32). Elementwise float64 in the reference's order (np.dot with the rotation matrix of
    seg_utils.py:64-69 written out: its z column adds exact zeros), one rounding to float32, float32 division, np.round."""
    points = np.asarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("openpcseg_amd: transform_scan_host wants (n, C >= 3) points, got %s" % (points.shape,))
    if points.shape[0] == 0:
        raise ValueError("openpcseg_amd: an empty frame has no minimum to shift by (the reference fails on it too)")
    c, s, scale, sx, sy, jx, jy, jz = (np.float64(v) for v in np.asarray(params_row, dtype=np.float64).reshape(8))
    x, y, z = (points[:, k].astype(np.float64) for k in range(3))
    X = x * c + y * (-s)
    Y = x * s + y * c
    Z = z
    X, Y, Z = X * scale, Y * scale, Z * scale
    X, Y = X * sx, Y * sy
    X, Y, Z = X + jx, Y + jy, Z + jz
    out = points.copy()
    out[:, 0], out[:, 1], out[:, 2] = X, Y, Z   # the one rounding to float32
    pc = np.round(out[:, :3] / np.float32(voxel_size)).astype(np.int32)
    pc -= pc.min(0, keepdims=True)
    return out, pc


def device_batch(raw, voxel_size=0.05, params=None, votes=1, eval_maps=False):
    """Dataset transform + sparse_quantize + collate of a raw batch resident in HBM, for `votes` augmented copies of every frame
    from one read of the scans. raw: a raw batch as hostdata.raw_frames reads it (the dict `workloads.synthetic.make_raw_batch`
    returns, its tensors on the device), labels included; params: host (votes * num_frames, 8) float64, vote-major
    (draw_train_params / tta_params), None = the identity.
    -> {"lidar", "targets"}: SparseTensors over the voxels of votes * num_frames scenes, scene v * num_frames + f = vote v of
    frame f -- what collate_batch (votes = 1) / collate_batch_tta would hand the model. With eval_maps also "targets_mapped" and
    "inverse_map" (SparseTensors over all votes * n points; inverse_map.F = the row of every point inside its own scene) and
    "num_points" (host list, per scene). One host read (the voxel count, inside sparse_quantize_frames)."""
    from . import native
    pts, labels, off, nf, n = raw_frames(raw, "transform.device_batch", "transform_scan_host", need_labels=True)
    v = int(votes)
    if params is None:
        params = identity_params(v * nf)
    be = native.backend()
    feats, coords, mins, off_dev = be.scan_transform(pts, off, params, v, voxel_size)
    scenes = be.scan_shift(coords, mins, off_dev, v)
    vox, index, inverse = sparse_quantize_frames(coords, scenes, v * nf)
    src = index if v == 1 else index % n   # row v * n + i carries the label of point i
    out = {"lidar": SparseTensor(feats[index], vox), "targets": SparseTensor(labels[src], vox)}
    if eval_maps:
        pc = torch.cat([coords, scenes.int()[:, None]], dim=1)
        first = scene_row_offsets(vox[:, 3], v * nf)   # first voxel row of every scene
        out["targets_mapped"] = SparseTensor(vote_labels(labels, v), pc)
        out["inverse_map"] = SparseTensor(inverse - first[scenes], pc)
        out["num_points"] = scene_points(off, v)
    return out
