"""PolarMix / LaserMix of the reference's SemanticKITTI loader for scans resident in HBM: the mixing of two
scans that `SemkittiDataset.__getitem__` performs under AUGMENT = 'GlobalAugment_LP', ahead of every dataset's own transform.

  __getitem__               R:pcseg/data/dataset/semantickitti/semantickitti.py:98-177 (the draws, the ring column)
  polarmix / swap / rotate_copy   R:pcseg/data/dataset/semantickitti/PolarMix_semantickitti.py
  lasermix_aug              R:pcseg/data/dataset/semantickitti/LaserMix_semantickitti.py
  get_kitti_points_ringID   R:...semantickitti.py:86-96

`draw_omega`, `draw_mix_plan` and `draw_train_plan` make the reference's draws in its call order (`choice(2, 1)` comes first in
EVERY frame, ahead of aug_points' draws), `mix_scan_host` / `ring_ids_host` restate the arithmetic in NumPy -- the host path and
the yardstick of csrc/scanmix.hip --, `device_mix` runs it on the device for a whole batch (two raw batches read by
hostdata.raw_frames: exactly four columns, empty input frames allowed) and hands back a raw batch that
`transform.device_batch`, `cylinder.device_batch` and `rangeview.device_batch` take unchanged.

LaserMix as the reference wrote it returns the first scan unchanged: its band thresholds are degrees (-6.7 / pi * 180 = -383.9)
compared with inclinations in radians, so every point falls into band 1 of the first scan. lasermix="reference" keeps that (it
still consumes the strategy draw); lasermix="radians" is a DEVIATION from the reference, opt-in: the same band tables with the
thresholds converted as the paper means them (deg * pi / 180), held to its own host form only.

The sector test of PolarMix runs in float32 on NumPy's float32 arctan2 (atan="numpy32", the reference's); the kernel's arctan2
is a double one rounded once (atan="double", the rule of csrc/cyl_cell.h and csrc/rangeproj.hip). The two differ by an ulp in
about a third of the values and move a row across a sector edge about twice in 1e8 tests.
"""
import numpy as np

from . import transform
from .hostdata import raw_frames

__all__ = ["INSTANCE_CLASSES", "LASERMIX_BANDS", "POLARMIX", "LASERMIX", "NO_MIX", "draw_omega", "draw_mix_plan", "draw_train_plan",
           "mix_scan_host", "ring_ids_host", "device_mix"]

INSTANCE_CLASSES = (1, 2, 3, 4, 5, 6, 7, 8)   # semantickitti.py:10
# the band thresholds of strategies inc3phi1, inc4phi1, inc5phi1, inc6phi1, in degrees (LaserMix_semantickitti.py:34-109)
LASERMIX_BANDS = ((-6.7, -13.4), (-5.0, -10.0, -15.0), (-4.0, -8.0, -12.0, -16.0), (-3.3, -6.6, -9.9, -13.2, -16.5))
POLARMIX, LASERMIX, NO_MIX = 0, 1, -1         # column 0 of a plan row: the value of choice(2, 1), or "no mixing"
MAX_CLASSES = 8                               # PCS_MIX_MAX_CLASSES of include/pcseg_hip.h
PLAN_STRIDE = 16                              # PCS_MIX_PLAN_STRIDE: float64 words of a frame's row in the device table


def draw_omega(rng=np.random):
    """The reference's module-level `Omega` (semantickitti.py:11), drawn ONCE at import and not part of a frame's draws:
    (random() * 2 pi / 3, (random() + 1) * 2 pi / 3)."""
    return (rng.random() * np.pi * 2 / 3, (rng.random() + 1) * np.pi * 2 / 3)


def draw_mix_plan(num_frames, rng=np.random, mix=True):
    """(num_frames, 4) float64 rows (kind, arg, swap, paste) in __getitem__'s call order: choice(2, 1) first -- 1 = LASERMIX draws
    choice(4, size=1), arg = the strategy index; 0 = POLARMIX draws random() for alpha = (u - 1) pi (arg), random() < 0.5 for the
    swap and random() < 1.0 for the paste (consumed, always true). mix=False (plain GlobalAugment, evaluation): only choice(2, 1)
    is consumed and the row is (NO_MIX, 0, 0, 0)."""
    plan = np.zeros((num_frames, 4), dtype=np.float64)
    for f in range(num_frames):
        prob = int(rng.choice(2, 1)[0])
        if not mix:
            plan[f, 0] = NO_MIX
        elif prob == 1:
            plan[f] = (LASERMIX, int(rng.choice(4, size=1)[0]), 0, 0)
        else:
            alpha = (rng.random() - 1) * np.pi
            swap = rng.random() < 0.5
            paste = rng.random() < 1.0
            plan[f] = (POLARMIX, alpha, swap, paste)
    return plan


def draw_train_plan(num_frames, rng=np.random, dataset="voxel", mix=True, **aug):
    """(plan, params[, cuts]) with the draws interleaved frame by frame as the real loader makes them: the frame's mix draws
    (draw_mix_plan), then transform.draw_train_params(1, rng, **aug), then -- dataset="fusion" -- the cut of the range view
    (rangeview.draw_train_params makes both). dataset: "voxel" | "cylinder" | "fusion"."""
    from . import rangeview
    if dataset not in ("voxel", "cylinder", "fusion"):
        raise ValueError("openpcseg_amd: dataset is 'voxel', 'cylinder' or 'fusion', got %r" % (dataset,))
    plan = np.empty((num_frames, 4), dtype=np.float64)
    params = np.empty((num_frames, 8), dtype=np.float64)
    cuts = np.empty(num_frames, dtype=np.float64)
    for f in range(num_frames):
        plan[f] = draw_mix_plan(1, rng, mix)[0]
        if dataset == "fusion":
            p, c = rangeview.draw_train_params(1, rng, **aug)
            params[f], cuts[f] = p[0], c[0]
        else:
            params[f] = transform.draw_train_params(1, rng, **aug)[0]
    return (plan, params, cuts) if dataset == "fusion" else (plan, params)


# ---- host form ---------------------------------------------------------------------------------------------------------------
def _check_atan(atan):
    if atan not in ("numpy32", "double"):
        raise ValueError("openpcseg_amd: atan is 'numpy32' or 'double', got %r" % (atan,))


def _check_points(points, what):
    points = np.asarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] != 4:
        raise ValueError("openpcseg_amd: %s wants (n, 4) points [x, y, z, reflectivity], got %s" % (what, points.shape))
    return points


def _check_classes(instance_classes):
    classes = [int(c) for c in instance_classes]
    if len(classes) > MAX_CLASSES or any(c < 0 or c > 255 for c in classes) or len(set(classes)) != len(classes):
        raise ValueError("openpcseg_amd: at most %d distinct instance classes inside 0 .. 255, got %r" % (MAX_CLASSES, tuple(instance_classes)))
    return classes


def _check_plan(plan, num_frames):
    plan = np.asarray(plan, dtype=np.float64)
    if plan.shape != (num_frames, 4):
        raise ValueError("openpcseg_amd: a mix plan is (num_frames, 4) rows (kind, arg, swap, paste), got %s for %d frames" % (plan.shape, num_frames))
    for kind, arg in plan[:, :2]:
        if kind not in (POLARMIX, LASERMIX, NO_MIX) or (kind == LASERMIX and arg not in (0, 1, 2, 3)):
            raise ValueError("openpcseg_amd: a plan row is POLARMIX, LASERMIX with a strategy 0 .. 3, or NO_MIX, got (%r, %r)" % (kind, arg))
    return plan


def _check_omega(omega):
    omega = np.asarray(omega, dtype=np.float64)
    if omega.shape != (2,):
        raise ValueError("openpcseg_amd: omega is the two angles of draw_omega, got shape %s" % (omega.shape,))
    return omega


def _check_lasermix(lasermix):
    if lasermix not in ("reference", "radians"):
        raise ValueError("openpcseg_amd: lasermix is 'reference' or 'radians', got %r" % (lasermix,))


def _arctan2_f32(y, x, atan):
    if atan == "numpy32":
        return np.arctan2(y, x)
    return np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)


def sector_edges(alpha):
    """(float32(alpha), float32(alpha + pi)): the edges swap() compares the float32 yaw with (NumPy compares a float32 array with
    a Python float in float32; beta is summed in float64 first, semantickitti.py:158-159)."""
    alpha = float(alpha)
    return np.float32(alpha), np.float32(alpha + np.pi)


def sector_mask(points, alpha, atan="numpy32"):
    """swap()'s membership: yaw = -arctan2(y, x) in float32, yaw > float32(alpha) & yaw < float32(beta), both strict."""
    yaw = -_arctan2_f32(points[:, 1], points[:, 0], atan)
    a, b = sector_edges(alpha)
    return (yaw > a) & (yaw < b)


def omega_params(omega):
    """The parameter rows under which transform_scan_host / affine_row of csrc/raw_scan.h IS rotate_copy's np.dot(float32
    rows, float64 matrix) stored as float32: (cos w, sin w, 1, 1, 1, 0, 0, 0) per angle."""
    out = transform.identity_params(2)
    for j, w in enumerate(_check_omega(omega)):
        out[j, 0], out[j, 1] = np.cos(w), np.sin(w)
    return out


def lasermix_thresholds(strategy):
    """The band thresholds of strategy 0 .. 3 in radians (float64, descending): deg * pi / 180."""
    return np.array([d * np.pi / 180 for d in LASERMIX_BANDS[int(strategy)]], dtype=np.float64)


def lasermix_bands(points, strategy):
    """The band (0 = the highest) of every row under lasermix="radians": inclination = arctan2(z, sqrt(x^2 + y^2)) in float64
    (lasermix_aug's columns are float64 after its concatenate with the labels), band = how many thresholds it is <= ."""
    x, y, z = (points[:, k].astype(np.float64) for k in range(3))
    inc = np.arctan2(z, np.sqrt(x * x + y * y))
    return (inc[:, None] <= lasermix_thresholds(strategy)[None, :]).sum(1)


def mix_scan_host(points1, labels1, points2, labels2, plan_row, omega, instance_classes=INSTANCE_CLASSES, atan="numpy32",
                  lasermix="reference"):
    """polarmix / lasermix_aug of one frame in NumPy: points (n, 4) float32, labels (n,) -> (points (m, 4) float32, labels (m,)
    int64). Row order as the reference's: scan 1 outside the sector (all of it without a swap), scan 2 inside it, the instance rows
    of scan 2 class by class in `instance_classes` order, that list rotated by omega[0], then by omega[1] (column 3 copied).
    atan / lasermix: see the module's text. A mixed frame without rows raises ValueError."""
    _check_atan(atan)
    _check_lasermix(lasermix)
    p1, p2 = _check_points(points1, "mix_scan_host"), _check_points(points2, "mix_scan_host")
    l1, l2 = np.asarray(labels1).reshape(-1).astype(np.int64), np.asarray(labels2).reshape(-1).astype(np.int64)
    if l1.shape[0] != p1.shape[0] or l2.shape[0] != p2.shape[0]:
        raise ValueError("openpcseg_amd: mix_scan_host wants one label per point")
    classes = _check_classes(instance_classes)
    kind, arg, swap, paste = _check_plan(np.asarray(plan_row, dtype=np.float64).reshape(1, -1), 1)[0]
    rot = omega_params(omega)
    if kind == POLARMIX:
        pts, labs = [p1], [l1]
        if swap:
            in1, in2 = sector_mask(p1, arg, atan), sector_mask(p2, arg, atan)
            pts, labs = [p1[~in1], p2[in2]], [l1[~in1], l2[in2]]
        if paste:
            rows = np.concatenate([np.flatnonzero(l2 == c) for c in classes]) if classes else np.zeros(0, dtype=np.int64)
            inst, inst_l = p2[rows], l2[rows]
            pts.append(inst)
            labs.append(inst_l)
            for j in range(2):
                pts.append(transform.transform_scan_host(inst, rot[j], 1.0)[0] if inst.shape[0] else inst)
                labs.append(inst_l)
        out, out_l = np.concatenate(pts), np.concatenate(labs)
    elif kind == LASERMIX and lasermix == "radians":
        b1, b2 = lasermix_bands(p1, arg), lasermix_bands(p2, arg)
        pts, labs = [], []
        for band in range(len(LASERMIX_BANDS[int(arg)]) + 1):   # xyzil_mix_1: bands alternate, the first from scan 1
            p, l, b = (p1, l1, b1) if band % 2 == 0 else (p2, l2, b2)
            pts.append(p[b == band])
            labs.append(l[b == band])
        out, out_l = np.concatenate(pts), np.concatenate(labs)
    else:   # no mixing, and LaserMix as the reference computes it
        out, out_l = p1.copy(), l1.copy()
    if out.shape[0] == 0:
        raise ValueError("openpcseg_amd: the mixed frame has no rows")
    return np.ascontiguousarray(out, dtype=np.float32), out_l


def ring_ids_host(points, atan="numpy32"):
    """get_kitti_points_ringID: points (n, >= 2) float32 -> (n,) float32. yaw = -arctan2(y, -x) in float32, proj_x = 0.5 (yaw / pi
    + 1) in float32, a flag on row i >= 1 where proj_x[i] < 0.2 and proj_x[i - 1] > 0.8, the inclusive sum clipped to 0 .. 63.
    (On a LaserMix frame the reference's columns are float64 by then; the flags agree wherever proj_x is not within an ulp of 0.2
    or 0.8.)"""
    _check_atan(atan)
    points = np.asarray(points, dtype=np.float32)
    if points.ndim != 2 or points.shape[1] < 2:
        raise ValueError("openpcseg_amd: ring_ids_host wants (n, C >= 2) points, got %s" % (points.shape,))
    yaw = -_arctan2_f32(points[:, 1], -points[:, 0], atan)
    proj_x = np.float32(0.5) * (yaw / np.float32(np.pi) + np.float32(1.0))
    flag = np.zeros(points.shape[0], dtype=np.int64)
    flag[1:] = (proj_x[1:] < np.float32(0.2)) & (proj_x[:-1] > np.float32(0.8))
    return np.clip(np.cumsum(flag), 0, 63).astype(np.float32)


# ---- device form -------------------------------------------------------------------------------------------------------------
def device_plan(plan, lasermix="reference"):
    """The (num_frames, PLAN_STRIDE) float64 table csrc/scanmix.hip reads (include/pcseg_hip.h): [mode, alpha32, beta32, swap,
    paste, T, T thresholds]; mode 0 = scan 1 unchanged, 1 = PolarMix, 2 = LaserMix bands."""
    _check_lasermix(lasermix)
    out = np.zeros((plan.shape[0], PLAN_STRIDE), dtype=np.float64)
    for f, (kind, arg, swap, paste) in enumerate(plan):
        if kind == POLARMIX:
            a, b = sector_edges(arg)
            out[f, :5] = (1, a, b, bool(swap), bool(paste))
        elif kind == LASERMIX and lasermix == "radians":
            t = lasermix_thresholds(arg)
            out[f, 0], out[f, 5] = 2, t.shape[0]
            out[f, 6:6 + t.shape[0]] = t
    return out


def device_mix(raw, partner, plan, omega, ring=False, instance_classes=INSTANCE_CLASSES, lasermix="reference"):
    """mix_scan_host(atan="double") of every frame of a raw batch resident in HBM. raw, partner: dicts as
    `workloads.synthetic.make_raw_batch` returns them, tensors on the device, the same number of frames (frame f of `partner` is
    the second scan of frame f; frame lengths are free); plan: host (num_frames, 4) rows of draw_mix_plan / draw_train_plan;
    omega: the two angles of draw_omega.
    -> {"points" (m, 4) fp32 -- (m, 5) with ring=True, column 4 = ring_ids_host(atan="double") of every mixed frame --, "labels"
    (m,) int64, "offsets": host frame boundaries, "num_frames"}: a raw batch again.
    One host read: the ten bucket counts of every frame, which size the output and make `offsets`. The plan, omega, the classes and
    both sets of frame boundaries travel in one pinned asynchronous copy. A mixed frame without rows raises ValueError."""
    from . import native
    form = dict(host_form="mix_scan_host", min_columns=4, exact_columns=True, allow_empty=True, need_labels=True)
    p1, l1, off1, nf, _ = raw_frames(raw, "device_mix's `raw`", **form)
    p2, l2, off2, nf2, _ = raw_frames(partner, "device_mix's `partner`", **form)
    if nf != nf2:
        raise ValueError("openpcseg_amd: device_mix wants as many partner frames as frames, got %d and %d" % (nf2, nf))
    plan = _check_plan(plan, nf)
    classes = _check_classes(instance_classes)
    table = device_plan(plan, lasermix)
    points, labels, offsets = native.backend().scan_mix(p1, l1, off1, p2, l2, off2, table, omega_params(omega), classes, bool(ring))
    empty = [f for f in range(nf) if offsets[f + 1] == offsets[f]]
    if empty:
        raise ValueError("openpcseg_amd: the mixed frame %d has no rows" % empty[0])
    return {"points": points, "labels": labels, "offsets": offsets, "num_frames": nf}
