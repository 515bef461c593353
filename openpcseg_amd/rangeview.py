"""The fusion (RPVNet) dataset's transform for scans resident in HBM: everything `transform.device_batch`
does -- augmentation, votes, the float32 store, voxel dedup, collation, evaluation maps -- plus the range view of every scene.

  get_range_image       R:pcseg/data/dataset/semantickitti/semantickitti_fusion.py:64-114
  get_single_sample     R:...semantickitti_fusion.py:128-196 (aug_points, then get_range_image of lidar.F)
  collate_batch(_tta)   R:...semantickitti_fusion.py:198-245 (the (scene, px, py) table, `offset`)
(waymo_fusion.py follows them.)

The range view projects the frame's DEDUPLICATED voxel rows (lidar.F, not the raw points) onto a 64 x 2048 image: column from the
azimuth shifted by a random cut, row from the ring, pixel collisions resolved by "the last row wins" (NumPy fancy assignment).
`range_view_host` restates get_range_image line by line in NumPy with the cut passed in -- the host path and the yardstick of
csrc/rangeproj.hip --, `draw_train_params` / `tta_params` make the reference's draws in its call order (the cut is the ONE
np.random.rand() behind each frame's augmentation; under TTA the loop is transform._tta_draws), `device_batch` runs the whole
transform on the device, on a raw batch (hostdata.raw_frames) with the ring in column 4.

The kernel's arctan2 is a double one rounded once to float32 (atan="double", the rule of csrc/cyl_cell.h); NumPy's float32
arctan2 (atan="numpy32", the reference's) differs from it by an ulp in about a third of the values, which moves a row to the
neighbouring column about once in 70 000 rows. Everything else is the same arithmetic bit for bit.
"""
import numpy as np

from . import transform
from .hostdata import raw_frames, scene_row_offsets

__all__ = ["HW", "range_view_host", "cut_value", "draw_train_params", "tta_params", "device_batch"]

HW = (64, 2048)   # INIT_HW = UP_HW of get_range_image: the resize between them is a copy


def cut_value(u):
    """The azimuthal cut of np.random.rand() value(s) `u` as the float32 get_range_image adds: (u - 0.5) * 2 * pi in float64,
    rounded once (NumPy adds the Python float to the float32 array as a weak scalar)."""
    return ((np.asarray(u, dtype=np.float64) - 0.5) * 2 * np.pi).astype(np.float32)


def range_view_host(points, cut, hw=HW, atan="numpy32"):
    """get_range_image in NumPy: points (n, >= 5) float32 rows [x, y, z, reflectivity, ring], cut = the float64 value of its
    np.random.rand() -> (image (5, H, W) float32, pxpy (n, 2) float64). atan: "numpy32" = NumPy's float32 arctan2 (the
    reference's), "double" = float32(arctan2 in float64) (the kernel's). A ring outside [0, H - 1] or a row that is not finite
    raises ValueError (the reference asserts on the first and wraps a negative ring)."""
    points = np.asarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] < 5:
        raise ValueError("openpcseg_amd: range_view_host wants (n, C >= 5) rows [x, y, z, reflectivity, ring], got %s" % (points.shape,))
    if atan not in ("numpy32", "double"):
        raise ValueError("openpcseg_amd: atan is 'numpy32' or 'double', got %r" % (atan,))
    h, w = int(hw[0]), int(hw[1])
    depth = np.linalg.norm(points[:, 0:3], 2, axis=1)
    scan_x, scan_y, reflectivity = points[:, 0], points[:, 1], points[:, 3]
    if atan == "numpy32":
        yaw = np.arctan2(scan_y, -scan_x)
    else:
        yaw = np.arctan2(scan_y.astype(np.float64), (-scan_x).astype(np.float64)).astype(np.float32)
    yaw = yaw + cut_value(cut)                                  # random cut
    yaw = yaw % np.float32(2 * np.pi) - np.float32(np.pi)       # (-pi, pi]
    proj_x = np.float32(0.5) * (yaw / np.float32(np.pi) + np.float32(1.0))
    proj_y = points[:, 4]                                       # ring
    proj_x = proj_x * np.float32(w - 1)
    assert yaw.dtype == proj_x.dtype == depth.dtype == np.float32
    rx, ry = np.round(proj_x), np.round(proj_y)
    if not (np.isfinite(scan_x).all() and np.isfinite(scan_y).all() and np.isfinite(ry).all()) or (
            points.shape[0] and (ry.min() < 0 or ry.max() > h - 1)):
        raise ValueError("openpcseg_amd: range_view_host: a row is not finite or its ring is outside [0, %d]" % (h - 1))
    proj_x, proj_y = rx.astype(np.int32), ry.astype(np.int32)

    proj_range = np.zeros((h, w))
    with np.errstate(divide="ignore"):
        proj_range[proj_y, proj_x] = np.float32(1.0) / depth
    proj_reflectivity = np.zeros((h, w))
    proj_reflectivity[proj_y, proj_x] = reflectivity
    proj_xyz = np.zeros((h, w, 3))
    proj_xyz[proj_y, proj_x] = points[:, :3]

    px = 2.0 * (proj_x / (w - 1) - 0.5)
    py = 2.0 * (proj_y / (h - 1) - 0.5)
    proj_range = 25 * (proj_range - 0.4)
    proj_reflectivity = 20 * (proj_reflectivity - 0.5)
    image = np.concatenate([proj_range[np.newaxis, :], proj_reflectivity[np.newaxis, :], proj_xyz.transpose(2, 0, 1)]).astype(np.float32)
    return image, np.hstack([px.reshape(-1, 1), py.reshape(-1, 1)])


def draw_train_params(num_frames, rng=np.random, **aug):
    """(params (num_frames, 8) float64, cuts (num_frames,) float64): per frame transform.draw_train_params' draws for that frame
    (`aug`: its keywords), then ONE rng.rand() -- the order in which get_single_sample calls aug_points and get_range_image."""
    params, cuts = np.empty((num_frames, 8), dtype=np.float64), np.empty(num_frames, dtype=np.float64)
    for f in range(num_frames):
        params[f] = transform.draw_train_params(1, rng=rng, **aug)[0]
        cuts[f] = rng.rand()
    return params, cuts


def tta_params(num_frames, num_votes=10, scale_range=(0.9, 1.1), rng=np.random):
    """(params (num_votes * num_frames, 8), cuts (num_votes * num_frames,)), vote-major (row v * num_frames + f). The draws run in
    __getitem__ order: frame by frame, vote by vote, each vote's scale draw followed by its cut. As in transform.tta_params the
    range the reference scales by is the CONFIGURED one (the TTA branch sets `scale_aug_range` but passes `scale_range`)."""
    return transform._tta_draws(num_frames, num_votes, scale_range, rng, cut=True)


def device_batch(raw, voxel_size=0.05, params=None, cuts=None, votes=1, eval_maps=False, hw=HW, check=True):
    """The fusion dataset's transform + collate of a raw batch resident in HBM: `transform.device_batch` (unchanged: raw, params,
    votes, eval_maps as there; raw["points"] (n, >= 5) with the ring in column 4), then the range view of every scene's voxel rows
    (native range_project on lidar.F / lidar.C[:, 3]). cuts: host (votes * num_frames,) float64 np.random.rand() values, vote-major
    (draw_train_params / tta_params), None = 0.5 for every scene: no cut.
    -> that dict plus "range_image" (votes * num_frames, 5, H, W) fp32, "range_pxpy" (voxels, 3) fp32 = (scene, px, py) and
    "offset" (cumulative voxel rows per scene, int32, as collate_batch adds).
    check: the flag of a ring outside [0, H - 1] / a row that is not finite is read (one extra host read) and raises ValueError;
    check=False hands the device flag back under "bad" (such a row keeps its pxpy row and touches no pixel)."""
    from . import native
    nf = raw_frames(raw, "rangeview.device_batch", "range_view_host", min_columns=5, need_labels=True)[3]
    scenes = int(votes) * nf
    if cuts is None:
        cuts = np.full(scenes, 0.5)
    cuts = np.asarray(cuts, dtype=np.float64).reshape(-1)
    if cuts.shape[0] != scenes:
        raise ValueError("openpcseg_amd: %d cuts for %d votes of %d frames" % (cuts.shape[0], int(votes), nf))
    out = transform.device_batch(raw, voxel_size, params, votes=votes, eval_maps=eval_maps)
    lidar = out["lidar"]
    scene_col = lidar.C[:, 3]
    image, pxpy, bad = native.backend().range_project(lidar.F, scene_col, cuts, scenes, hw)
    out.update(range_image=image, range_pxpy=pxpy, offset=scene_row_offsets(scene_col, scenes)[1:].int())
    if not check:
        out["bad"] = bad
    elif int(bad.item()):
        raise ValueError("rangeview.device_batch: a voxel row is not finite or its ring (column 4) is outside [0, %d]" % (int(hw[0]) - 1))
    return out
