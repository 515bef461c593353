"""The range-view dataset's scan and its KNN label vote for scans resident in HBM.

  LaserScan.do_range_projection / SemLaserScan.do_label_projection   R:pcseg/data/dataset/semantickitti/laserscan.py:174-238, :389-400
  prepare_input_label_semantic_with_mask / generate_label            R:pcseg/data/dataset/semantickitti/semantickitti_rv.py:284-334
  KNN.forward / get_gaussian_kernel / postprocess_knn                R:pcseg/model/segmentor/range/utils.py:209-226, :275-341

The spherical projection is per RAW point, by pitch, "the nearest point wins" a pixel, empty pixels hold -1, and every point keeps
its pixel (`proj_x`, `proj_y`) and its depth (`unproj_range`) for the vote. (rangeview.py is another projection: deduplicated voxel
rows by ring, last row wins, inverse depth, a random cut.)

Host contracts in NumPy -- `range_scan_host`, `input_host`, `knn_vote_host` --, the yardsticks of csrc/rangescan.hip, and the device
forms `device_batch`, `knn_vote`, `predict` on a raw batch (hostdata.raw_frames).

Two orders the reference leaves open are FIXED here, and the kernels follow them:
  collision   a pixel goes to the point with the smallest depth, among equal depths to the smallest point index (the reference's
              np.argsort(depth)[::-1] is not a stable order);
  selection   the vote takes the `knn` candidates that come first in ascending (weighted distance, window position in row-major
              order) (torch's topk(sorted=False) does not say which of two equal distances it keeps).
The kernel's arctan2 / arcsin are double ones rounded once to float32 (atan="double", the rule of csrc/cyl_cell.h); NumPy's float32
functions (atan="numpy32", the reference's) differ from them by an ulp now and then, which can move a point to the neighbouring
pixel. Everything else is the same float32 arithmetic, operation by operation.
"""
import math

import numpy as np

from .hostdata import raw_frames

__all__ = ["HW", "FOV", "range_scan_host", "input_host", "inv_gauss_weights", "knn_vote_host", "device_batch", "knn_vote", "predict", "point_labels"]

HW = (64, 2048)      # R:tools/cfgs/range/*.yaml: 64 x 2048 and 64 x 512
FOV = (3.0, -25.0)   # fov_up, fov_down in degrees, as SemkittiRangeViewDataset passes them
SEARCHES = (3, 5, 7)
MAX_CLASS = 64


def _fov_consts(fov):
    """(float32(|fov_down|), float32(fov)) in radians: do_range_projection computes both as Python floats, and NumPy rounds a Python
    scalar to float32 when it meets a float32 array."""
    fov_up = float(fov[0]) / 180.0 * np.pi
    fov_down = float(fov[1]) / 180.0 * np.pi
    total = abs(fov_down) + abs(fov_up)
    if not (math.isfinite(total) and total > 0):
        raise ValueError("openpcseg_amd: fov = (up, down) in degrees with a positive total, got %r" % (fov,))
    return np.float32(abs(fov_down)), np.float32(total)


def _hw(hw):
    h, w = int(hw[0]), int(hw[1])
    if h < 1 or w < 1:
        raise ValueError("openpcseg_amd: hw = (H >= 1, W >= 1), got %r" % (hw,))
    return h, w


def range_scan_host(points, labels=None, hw=HW, fov=FOV, atan="numpy32", mask="reference"):
    """LaserScan.do_range_projection + SemLaserScan.do_label_projection of ONE scan in NumPy: points (n, >= 4) float32 rows
    [x, y, z, remission], labels (n,) raw ids (semantic id in the low 16 bits) or None
    -> dict: proj_range (H, W), proj_xyz (H, W, 3), proj_remission (H, W) float32 (-1 where empty), proj_idx (H, W) int32 (-1),
       proj_mask (H, W) float32, proj_sem_label (H, W) int32 (0 where empty or without labels); per point proj_x, proj_y (n,) int32
       and unproj_range (n,) float32.
    atan: "numpy32" = NumPy's float32 arctan2 / arcsin (the reference's), "double" = the float64 functions rounded once (the kernel's).
    mask: "reference" = proj_idx > 0 as the reference writes it (the pixel point 0 wins gets mask 0), "hit" = proj_idx >= 0.
    A row whose x, y, z or depth is not finite, whose depth is zero, or whose |z / depth| exceeds 1 (z * z in the subnormals) raises
    ValueError (the reference makes NaN indices of it)."""
    points = np.asarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] < 4:
        raise ValueError("openpcseg_amd: range_scan_host wants (n, C >= 4) rows [x, y, z, remission], got %s" % (points.shape,))
    if atan not in ("numpy32", "double"):
        raise ValueError("openpcseg_amd: atan is 'numpy32' or 'double', got %r" % (atan,))
    if mask not in ("reference", "hit"):
        raise ValueError("openpcseg_amd: mask is 'reference' or 'hit', got %r" % (mask,))
    h, w = _hw(hw)
    n = points.shape[0]
    if labels is not None:
        labels = np.asarray(labels).reshape(-1)
        if labels.shape[0] != n:
            raise ValueError("openpcseg_amd: range_scan_host: %d labels for %d points" % (labels.shape[0], n))
    fov_down_abs, fov_total = _fov_consts(fov)
    one, half = np.float32(1.0), np.float32(0.5)
    scan_x, scan_y, scan_z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        depth = np.sqrt((scan_x * scan_x + scan_y * scan_y) + scan_z * scan_z)   # == np.linalg.norm(points[:, :3], 2, axis=1)
    if not (np.isfinite(points[:, :3]).all() and np.isfinite(depth).all() and (depth > 0).all()):
        raise ValueError("openpcseg_amd: range_scan_host: a row is not finite or has zero depth")
    ratio = scan_z / depth
    if not (np.abs(ratio) <= 1).all():    # z * z in the subnormals (x = y = 0, |z| ~ 1e-20): the reference's arcsin gives NaN there
        raise ValueError("openpcseg_amd: range_scan_host: a row is not finite or has zero depth (|z / depth| > 1: no pitch)")
    if atan == "numpy32":
        yaw = -np.arctan2(scan_y, scan_x)
        pitch = np.arcsin(ratio)
    else:
        yaw = -np.arctan2(scan_y.astype(np.float64), scan_x.astype(np.float64)).astype(np.float32)
        pitch = np.arcsin(ratio.astype(np.float64)).astype(np.float32)
    proj_x = half * (yaw / np.float32(np.pi) + one)
    proj_y = one - (pitch + fov_down_abs) / fov_total
    proj_x = proj_x * np.float32(w)
    proj_y = proj_y * np.float32(h)
    assert depth.dtype == yaw.dtype == pitch.dtype == proj_x.dtype == proj_y.dtype == np.float32
    proj_x = np.maximum(np.float32(0), np.minimum(np.float32(w - 1), np.floor(proj_x))).astype(np.int32)
    proj_y = np.maximum(np.float32(0), np.minimum(np.float32(h - 1), np.floor(proj_y))).astype(np.int32)

    # the contract's order: descending depth, among equal depths descending index, so that the LAST write of a pixel is the nearest
    # point and, among equally near ones, the lowest index
    order = np.lexsort((np.arange(n), depth))[::-1]
    oy, ox = proj_y[order], proj_x[order]
    out = {"proj_range": np.full((h, w), -1, dtype=np.float32), "proj_xyz": np.full((h, w, 3), -1, dtype=np.float32),
           "proj_remission": np.full((h, w), -1, dtype=np.float32), "proj_idx": np.full((h, w), -1, dtype=np.int32)}
    out["proj_range"][oy, ox] = depth[order]
    out["proj_xyz"][oy, ox] = points[order, :3]
    out["proj_remission"][oy, ox] = points[order, 3]
    out["proj_idx"][oy, ox] = order.astype(np.int32)
    idx = out["proj_idx"]
    out["proj_mask"] = ((idx > 0) if mask == "reference" else (idx >= 0)).astype(np.float32)
    sem = np.zeros((h, w), dtype=np.int32)
    if labels is not None:
        hit = idx >= 0
        sem[hit] = (labels.astype(np.int64) & 0xFFFF)[idx[hit]]
    out.update(proj_sem_label=sem, proj_x=proj_x, proj_y=proj_y, unproj_range=depth)
    return out


def _apply_lut(sem, label_lut):
    """generate_label's remap as one lookup: ids inside the table go through it, ids beyond it stay (no key matches them)."""
    sem = np.asarray(sem).astype(np.int64)
    if label_lut is None:
        return sem
    lut = np.asarray(label_lut, dtype=np.int64).reshape(-1)
    inside = (sem >= 0) & (sem < lut.shape[0])
    out = sem.copy()
    out[inside] = lut[sem[inside]]
    return out


def input_host(view, label_lut=None):
    """prepare_input_label_semantic_with_mask + generate_label on a `range_scan_host` dict
    -> (scan (6, H, W) float32 = [x / 50, y / 50, z / 3, remission, range / 80, mask] (float32 divisions), label (H, W) int64
    (through label_lut when given), mask (H, W) float32)."""
    xyz = view["proj_xyz"]
    scale = np.array([50.0, 50.0, 3.0], dtype=np.float32)
    scan = np.concatenate([xyz / scale, view["proj_remission"][..., None], (view["proj_range"] / np.float32(80.0))[..., None],
                           view["proj_mask"][..., None]], axis=-1)
    assert scan.dtype == np.float32
    return np.ascontiguousarray(scan.transpose(2, 0, 1)), _apply_lut(view["proj_sem_label"], label_lut), view["proj_mask"].astype(np.float32)


def inv_gauss_weights(search=5, sigma=1.0):
    """(search * search,) float32, row-major: the vote's weight of every window position, 1 - g / sum(g) with
    g = exp(-(dx^2 + dy^2) / (2 sigma^2)) / (2 pi sigma^2) over the offsets dx, dy from the window's centre. NumPy, float32 step by
    step: the squared offsets and their sum are exact; the quotient is a float32 division; exp is taken in double and rounded once;
    the scale is one float32 product; the normalising sum runs in eight lanes (`_lane_sum`) and the rest is a float32 division and
    a subtraction. These are the bits of the reference's get_gaussian_kernel wherever tests/golden/make_rangescan_golden.py has
    compared them: search 3, 5, 7 at the sigmas its GUARDED_SIGMAS lists (1.0, the shipped one, among them)."""
    search, f32 = int(search), np.float32
    off = np.arange(search, dtype=np.float32) - f32((search - 1) / 2.0)
    r2 = (off * off)[None, :] + (off * off)[:, None]
    var = float(sigma) ** 2.0
    g = f32(1.0 / (2.0 * math.pi * var)) * np.exp((-r2 / f32(2 * var)).astype(np.float64)).astype(np.float32)
    g = g.reshape(-1)
    w = f32(1.0) - g / _lane_sum(g)
    assert w.dtype == np.float32
    return w


def _lane_sum(v, lanes=8, rows=4):
    """Float32 sum of a short vector in a FIXED order: whole rows of `lanes` values go to `rows` interleaved running rows (row r
    takes rows r, r + rows, ... of the first rows * (n_rows // rows)), left-over whole rows to running row 0, the running rows are
    folded into row 0 in order, and the total is the ragged tail summed left to right, then the lanes of row 0 added left to right.
    (The order an eight-lane vector reduction takes; fixing it makes the weights a function of (search, sigma) alone.)"""
    f32 = np.float32
    n_rows = v.shape[0] // lanes
    body, tail = v[:n_rows * lanes].reshape(n_rows, lanes), v[n_rows * lanes:]
    run = np.zeros((rows, lanes), dtype=np.float32)
    whole = n_rows // rows * rows
    for i in range(whole):
        run[i % rows] = run[i % rows] + body[i]
    for i in range(whole, n_rows):
        run[0] = run[0] + body[i]
    for r in range(1, rows):
        run[0] = run[0] + run[r]
    total = f32(0.0)
    for x in tail:
        total = f32(total + x)
    for x in run[0]:
        total = f32(total + x)
    return total


def _vote_args(search, knn, cutoff, num_class):
    search, knn, num_class, cutoff = int(search), int(knn), int(num_class), float(cutoff)
    if search not in SEARCHES:
        raise ValueError("openpcseg_amd: the vote's search window is 3, 5 or 7 (odd, as the reference demands), got %d" % search)
    if not 1 <= knn <= search * search:
        raise ValueError("openpcseg_amd: 1 <= knn <= search^2, got knn = %d for search = %d" % (knn, search))
    if not cutoff >= 0:
        raise ValueError("openpcseg_amd: cutoff >= 0 (0 = off), got %r" % (cutoff,))
    if not 2 <= num_class <= MAX_CLASS:
        raise ValueError("openpcseg_amd: 2 <= num_class <= %d, got %d" % (MAX_CLASS, num_class))
    return search, knn, cutoff, num_class


def knn_vote_host(proj_range, proj_argmax, unproj_range, px, py, knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=20):
    """KNN.forward of ONE scan in NumPy: proj_range (H, W) float32, proj_argmax (H, W) labels in [0, num_class), unproj_range (n,)
    float32, px / py (n,) pixel of every point -> (n,) int64 in [1, num_class - 1].
    Window: search x search around the point's pixel, zero outside the image (range 0, label 0; no azimuthal wrap), negative ranges
    +inf, the centre's range replaced by the point's own; weighted distance |range - own| * (1 - gaussian) in float32. The `knn`
    first candidates in ascending (distance, window position) vote with their pixel's label, those farther than `cutoff` (> 0) for
    an extra bin; the decision is the class of 1 .. num_class - 1 with the most votes, the lowest on equal counts."""
    search, knn, cutoff, num_class = _vote_args(search, knn, cutoff, num_class)
    proj_range = np.asarray(proj_range, dtype=np.float32)
    proj_argmax = np.asarray(proj_argmax).astype(np.int64)
    unproj_range = np.asarray(unproj_range, dtype=np.float32).reshape(-1)
    px, py = np.asarray(px).astype(np.int64).reshape(-1), np.asarray(py).astype(np.int64).reshape(-1)
    if proj_range.ndim != 2 or proj_argmax.shape != proj_range.shape:
        raise ValueError("openpcseg_amd: knn_vote_host wants (H, W) proj_range and proj_argmax, got %s and %s" % (proj_range.shape, proj_argmax.shape))
    h, w = proj_range.shape
    n = unproj_range.shape[0]
    if px.shape[0] != n or py.shape[0] != n:
        raise ValueError("openpcseg_amd: knn_vote_host wants one pixel and one range per point (%d, %d, %d)" % (px.shape[0], py.shape[0], n))
    if n and (px.min() < 0 or px.max() >= w or py.min() < 0 or py.max() >= h):
        raise ValueError("openpcseg_amd: knn_vote_host: a pixel outside the %d x %d image" % (h, w))
    if proj_argmax.size and (proj_argmax.min() < 0 or proj_argmax.max() >= num_class):
        raise ValueError("openpcseg_amd: knn_vote_host: proj_argmax outside [0, %d)" % num_class)
    pad = (search - 1) // 2
    rng_p = np.zeros((h + 2 * pad, w + 2 * pad), dtype=np.float32)
    rng_p[pad:pad + h, pad:pad + w] = proj_range
    lab_p = np.zeros((h + 2 * pad, w + 2 * pad), dtype=np.int64)
    lab_p[pad:pad + h, pad:pad + w] = proj_argmax
    ky, kx = np.divmod(np.arange(search * search), search)
    yy, xx = py[:, None] + ky[None, :], px[:, None] + kx[None, :]      # padded coordinates of every window position
    r = rng_p[yy, xx]
    labs = lab_p[yy, xx]
    r[r < 0] = np.inf
    r[:, (search * search - 1) // 2] = unproj_range
    with np.errstate(invalid="ignore"):
        dist = np.abs(r - unproj_range[:, None]) * inv_gauss_weights(search, sigma)[None, :]
    assert dist.dtype == np.float32
    sel = np.argsort(dist, axis=1, kind="stable")[:, :knn]          # ascending (distance, window position)
    votes = np.take_along_axis(labs, sel, axis=1)
    if cutoff > 0:
        votes[np.take_along_axis(dist, sel, axis=1) > np.float32(cutoff)] = num_class
    counts = np.zeros((n, num_class + 1), dtype=np.int64)
    np.add.at(counts, (np.repeat(np.arange(n), knn), votes.reshape(-1)), 1)
    return counts[:, 1:-1].argmax(axis=1).astype(np.int64) + 1


# ---- the device forms -------------------------------------------------------------------------------------------------------------
def device_batch(raw, hw=HW, fov=FOV, label_lut=None, mask="reference", check=True):
    """The range-view dataset's __getitem__ + collate of a raw batch resident in HBM (hostdata.raw_frames: "points" (n, C >= 4) fp32
    frame after frame, "offsets", "num_frames", optional "labels"), two launches (native range_scan)
    -> {"scan_rv" (B, 6, H, W) fp32, "label_rv" (B, H, W) int64 (0 without labels), "mask_rv" (B, H, W) fp32, "proj_idx" (B, H, W)
        int32 (index within the frame, -1), "proj_x", "proj_y" (n,) int32, "unproj_range" (n,) fp32, "point_offset" (host list)}.
    label_lut: host table of the learning map (ids beyond it stay). mask: as range_scan_host. Equal to range_scan_host(atan="double")
    + input_host of every frame.
    check: the flag of a row that is not finite or has zero depth is read (one host read) and raises ValueError; check=False hands
    the device flag back under "bad" (such a row has proj_x = proj_y = -1 and touches no pixel)."""
    from . import native
    if mask not in ("reference", "hit"):
        raise ValueError("openpcseg_amd: mask is 'reference' or 'hit', got %r" % (mask,))
    pts, labels, off, nf, _ = raw_frames(raw, "rangescan.device_batch", "range_scan_host", min_columns=4)
    out = native.backend().range_scan(pts, off, labels, _hw(hw), _fov_consts(fov), label_lut, mask == "hit")
    bad = out.pop("bad")
    out["point_offset"] = off
    if not check:
        out["bad"] = bad
    elif int(bad.item()):
        raise ValueError("rangescan.device_batch: a row is not finite or has zero depth")
    return out


def knn_vote(proj_range, proj_argmax, unproj_range, proj_x, proj_y, point_offset, knn=5, search=5, sigma=1.0, cutoff=1.0,
             num_class=20, labels=None, hist=None):
    """KNN.forward for a whole batch in one launch (native range_knn_vote): proj_range (B, H, W) fp32, proj_argmax (B, H, W) int64,
    unproj_range (n,) fp32, proj_x / proj_y (n,) int32, point_offset: host list of B + 1 point boundaries -> (n,) int64, per scan
    equal to knn_vote_host. A point with proj_x < 0 (device_batch's bad rows) gets 0 and is not counted.
    labels (n,) int64 + hist (num_class, num_class) int64: hist[label][pred] += 1 for labels in [0, num_class), in the same launch."""
    from . import native
    search, knn, cutoff, num_class = _vote_args(search, knn, cutoff, num_class)
    return native.backend().range_knn_vote(proj_range, proj_argmax, unproj_range, proj_x, proj_y, point_offset, knn, search,
                                           inv_gauss_weights(search, sigma), cutoff, num_class, labels, hist)


def predict(model, raw, evaluator=None, hw=HW, fov=FOV, label_lut=None, mask="reference", knn=5, search=5, sigma=1.0, cutoff=1.0):
    """One evaluation pass of a range-view model on a raw batch, as validate_semkitti + postprocess_knn run it: device_batch ->
    model(scan_rv) -> bilinear resize (align_corners=True) when the logits are smaller than (H, W) -> argmax -> knn_vote with
    proj_range = scan_rv[:, 4] * 80 (the reference's own float32 round trip of the range image).
    model: any eval() module (B, 6, H, W) -> (B, num_class, h, w). evaluator: a SegEvaluator of num_class; with raw["labels"] every
    point is counted once (semantic id = label & 0xFFFF, through label_lut when given) inside the vote's launch.
    -> {"pred" (n,) int64, "point_offset" (host list)}."""
    import torch
    if model.training:
        raise RuntimeError("openpcseg_amd: rangescan.predict wants model.eval()")
    batch = device_batch(raw, hw, fov, label_lut, mask)
    scan = batch["scan_rv"]
    with torch.no_grad():
        logits = model(scan)
        if tuple(logits.shape[-2:]) != tuple(scan.shape[-2:]):
            logits = torch.nn.functional.interpolate(logits, size=tuple(scan.shape[-2:]), mode="bilinear", align_corners=True)
        argmax = logits.argmax(dim=1)
        num_class = int(logits.shape[1])
        labels = hist = None
        if evaluator is not None:
            hist = evaluator.counters(num_class, scan.device, batch["point_offset"], count=raw.get("labels") is not None)
            if hist is not None:
                labels = point_labels(raw["labels"], label_lut)
        pred = knn_vote(scan[:, 4] * 80, argmax, batch["unproj_range"], batch["proj_x"], batch["proj_y"], batch["point_offset"],
                        knn, search, sigma, cutoff, num_class, labels, hist)
    return {"pred": pred, "point_offset": batch["point_offset"]}


def point_labels(labels, label_lut=None):
    """Per-point evaluation labels on the labels' device: the semantic id (low 16 bits), through label_lut when given (ids beyond
    the table stay). The table travels in one pinned asynchronous copy."""
    import torch
    sem = labels.reshape(-1).long() & 0xFFFF
    if label_lut is None:
        return sem
    from . import native
    lut = native._h2d(np.asarray(label_lut, dtype=np.int64).reshape(-1).tolist(), torch.int64, sem.device)   # pinned, asynchronous
    return torch.where(sem < lut.shape[0], lut[sem.clamp(max=lut.shape[0] - 1)], sem)
