"""Shared by test_rangescan_host.py and test_rangescan.py: the fixture's reader, the comparison of a host or device result with it,
the constructed inputs of the KNN vote, and a torch restatement of the reference's unfold / topk sequence."""
import os
import zlib

import numpy as np

from openpcseg_amd import rangescan

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangescan_golden.npz")
IMAGE_KEYS = ("proj_range", "proj_xyz", "proj_remission", "proj_idx", "proj_mask", "proj_sem_label")


def load_gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def sizes(gold):
    return [tuple(int(v) for v in hw) for hw in gold["sizes"]]


def frames(gold):
    """[(points (n, 4) float32, raw labels (n,) uint32)] of the fixture's two frames."""
    return [(gold["f%d_points" % i], gold["f%d_labels" % i]) for i in range(gold["frames"].shape[0])]


def prefix(i, hw):
    return "f%d_%dx%d_" % (i, hw[0], hw[1])


def lut(gold):
    return gold["label_lut"].astype(np.int64)


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def assert_view_is_fixture(gold, pre, view):
    """A range_scan_host-shaped dict against the reference's arrays: every full image by its CRC, the hit pixels value by value."""
    for key in IMAGE_KEYS:
        assert crc(view[key]) == gold[pre + "crc_" + key], (pre, key)
    hit = gold[pre + "hit"]
    assert np.array_equal(np.flatnonzero(view["proj_idx"].reshape(-1) >= 0), hit), pre
    assert np.array_equal(view["proj_idx"].reshape(-1)[hit], gold[pre + "hit_idx"]), pre
    assert np.array_equal(view["proj_range"].reshape(-1)[hit], gold[pre + "hit_range"]), pre
    assert np.array_equal(view["proj_mask"].reshape(-1)[hit], gold[pre + "hit_mask"].astype(np.float32)), pre
    assert np.array_equal(view["proj_sem_label"].reshape(-1)[hit], gold[pre + "hit_sem"]), pre
    for key in ("proj_x", "proj_y", "unproj_range"):
        assert view[key].dtype == (np.float32 if key == "unproj_range" else np.int32), (pre, key)
        assert np.array_equal(view[key], gold[pre + key]), (pre, key)


def assert_input_is_fixture(gold, pre, scan, label, mask):
    """The (6, H, W) input tensor, the mapped label and the mask against the reference's."""
    assert scan.dtype == np.float32 and label.dtype == np.int64 and mask.dtype == np.float32
    assert crc(scan) == gold[pre + "crc_scan"] and crc(label) == gold[pre + "crc_label"], pre
    hit = gold[pre + "hit"]
    assert np.array_equal(label.reshape(-1)[hit], gold[pre + "hit_label"]), pre
    assert np.array_equal(mask, scan[5]) and crc(mask) == gold[pre + "crc_proj_mask"], pre


def vote_inputs(gold, i, hw, atan="double"):
    """What postprocess_knn hands the vote for frame i at hw: (range image = channel 4 * 80, proj_argmax, unproj_range, px, py)."""
    pts, labels = frames(gold)[i]
    view = rangescan.range_scan_host(pts, labels, hw, atan=atan)
    scan = rangescan.input_host(view, lut(gold))[0]
    return scan[4] * np.float32(80.0), gold[prefix(i, hw) + "proj_argmax"].astype(np.int64), view["unproj_range"], view["proj_x"], view["proj_y"]


# ---- constructed inputs of the vote at 16 x 64 --------------------------------------------------------------------------------------
VOTE_HW = (16, 64)
VOTE_KINDS = ("border", "empty", "lost", "padding")


def vote_case(kind, num_class, seed=0, hw=VOTE_HW):
    """Seeded inputs of one scan's vote that lean on one edge of the contract:
      border   points in columns 0, 1, W - 2, W - 1 and rows 0, 1, H - 2, H - 1 of a full image (the zero padding, no wrap);
      empty    an image of empty pixels (-1) around a few hit ones: windows full of +inf;
      lost     points whose own range is far from their pixel's (they lost it to a nearer point): the centre's replacement;
      padding  ranges below the cutoff everywhere, so the zero padding (range 0, label 0) is a near neighbour of border points.
    -> dict(proj_range, proj_argmax, unproj_range, px, py)."""
    rng = np.random.default_rng(1000 * seed + VOTE_KINDS.index(kind))
    h, w = hw
    argmax = rng.integers(0, num_class, size=(h, w)).astype(np.int64)
    image = rng.uniform(2.0, 40.0, size=(h, w)).astype(np.float32)
    if kind in ("border", "padding"):
        cols, rows = np.array([0, 1, w - 2, w - 1]), np.array([0, 1, h - 2, h - 1])
        py = np.concatenate([np.repeat(np.arange(h), 4), np.repeat(rows, w)])
        px = np.concatenate([np.tile(cols, h), np.tile(np.arange(w), 4)])
        if kind == "padding":
            image = rng.uniform(0.05, 0.9, size=(h, w)).astype(np.float32)
    else:
        n = 300
        py, px = rng.integers(0, h, size=n), rng.integers(0, w, size=n)
        if kind == "empty":
            keep = rng.uniform(size=(h, w)) < 0.08
            image = np.where(keep, image, np.float32(-1.0)).astype(np.float32)
    unproj = image[py, px].copy()
    unproj = np.where(unproj < 0, np.float32(7.5), unproj).astype(np.float32)     # a point on an empty pixel still has a range
    if kind == "lost":
        unproj = (unproj + rng.uniform(0.5, 6.0, size=unproj.shape).astype(np.float32)).astype(np.float32)
    else:
        jitter = rng.uniform(-0.3, 0.3, size=unproj.shape).astype(np.float32)
        unproj = np.where(rng.uniform(size=unproj.shape) < 0.5, unproj, np.abs(unproj + jitter)).astype(np.float32)
    return {"proj_range": image, "proj_argmax": argmax, "unproj_range": unproj, "px": px.astype(np.int32), "py": py.astype(np.int32)}


def torch_vote(proj_range, proj_argmax, unproj_range, px, py, knn, search, sigma, cutoff, num_class):
    """KNN.forward's sequence of torch operations (unfold, gather, topk, gather, scatter_add_, argmax) restated on host tensors."""
    import torch
    import torch.nn.functional as F
    proj_range, unproj_range = torch.from_numpy(np.asarray(proj_range, dtype=np.float32)), torch.from_numpy(np.asarray(unproj_range, dtype=np.float32))
    proj_argmax = torch.from_numpy(np.asarray(proj_argmax).astype(np.int64))
    px, py = torch.from_numpy(np.asarray(px).astype(np.int64)), torch.from_numpy(np.asarray(py).astype(np.int64))
    h, w = proj_range.shape
    pad = (search - 1) // 2
    unfold_range = F.unfold(proj_range[None, None, ...], kernel_size=(search, search), padding=(pad, pad))
    idx = py * w + px
    window = unfold_range[:, :, idx]
    window[window < 0] = float("inf")
    window[:, (search * search - 1) // 2, :] = unproj_range
    dist = torch.abs(window - unproj_range) * torch.from_numpy(rangescan.inv_gauss_weights(search, sigma)).view(1, -1, 1)
    _, knn_idx = dist.topk(knn, dim=1, largest=False, sorted=False)
    unfold_argmax = F.unfold(proj_argmax[None, None, ...].float(), kernel_size=(search, search), padding=(pad, pad)).long()
    votes = torch.gather(unfold_argmax[:, :, idx], 1, knn_idx)
    if cutoff > 0:
        votes[torch.gather(dist, 1, knn_idx) > cutoff] = num_class
    onehot = torch.zeros((1, num_class + 1, unproj_range.shape[0])).scatter_add_(1, votes, torch.ones_like(votes).float())
    return (onehot[:, 1:-1].argmax(dim=1) + 1).view(-1).numpy()
