"""Inputs, the host yardsticks and the bounds shared by test_rangeloss_host.py and test_rangeloss.py."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from openpcseg_amd import rangeloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "rangeloss_golden.npz")
CLOSE = 1e-5       # two minima of a window within this relative distance: fp32 may pick the other pixel
MASK_CAP = 1e-3    # at most this share of the gradient's elements may be excluded for it
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}


def load_gold():
    return np.load(GOLD)


def gold_case(gold, i):
    """-> logits (B, C, H, W) float32, labels (B, H, W) int64 tensors of fixture case i."""
    return torch.from_numpy(gold["c%d_logits" % i]), torch.from_numpy(gold["c%d_labels" % i].astype(np.int64))


def gold_grad32(gold, i):
    return gold["c%d_grad64" % i].astype(np.float32) + gold["c%d_grad32_delta" % i]


def make_logits(shape, seed, scale=3.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def make_labels(shape, seed, kind="blocks", block=(3, 7)):
    """(B, H, W) int64, constant on blocks. kind: 'blocks' every class may occur, class 0 present; 'absent' the last image draws
    from three classes; 'image0' the first image is all class 0; 'all0' the whole batch is class 0."""
    b, c, h, w = shape
    rng = np.random.default_rng(seed + 1000)
    out = np.zeros((b, h, w), dtype=np.int64)
    if kind == "all0":
        return torch.from_numpy(out)
    bh, bw = block
    for n in range(b):
        if kind == "image0" and n == 0 and b > 1:
            continue
        pool = np.array([0, 1, c - 1]) if (kind == "absent" and n == b - 1) else np.arange(c)
        blocks = rng.choice(pool, size=(-(-h // bh), -(-w // bw)))
        blocks[0, 0] = 0
        out[n] = np.repeat(np.repeat(blocks, bh, axis=0), bw, axis=1)[:h, :w]
    return torch.from_numpy(out)


def tie_logits(shape, seed, block=(2, 5)):
    """Blocks of identical logit vectors: every window inside a block, and many across two, have equal minima."""
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    bh, bw = block
    vec = (rng.standard_normal((b, c, -(-h // bh), -(-w // bw))) * 3.0).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(vec, bh, axis=2), bw, axis=3)[:, :, :h, :w]))


def host(logits, labels, dtype, **opts):
    """range_criterion_host on host tensors -> (total, terms (4), grad) as float64 NumPy; logits are upcast from their dtype."""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    total, terms = rangeloss.range_criterion_host(x, labels.cpu(), dtype=dtype, **opts)
    total.backward()
    return (np.float64(total.item()), np.array([t.item() for t in terms], dtype=np.float64), x.grad.double().numpy())


def close_mask(logits):
    """Elements that are one of the two smallest of a clipped 3 x 3 window whose two smallest float64 probabilities are within
    CLOSE relative of each other -> bool (B, C, H, W)."""
    p = F.softmax(logits.detach().cpu().double(), dim=1).numpy()
    b, c, h, w = p.shape
    pad = np.full((b, c, h + 2, w + 2), np.inf)
    pad[:, :, 1:-1, 1:-1] = p
    win = np.stack([pad[:, :, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=-1)
    order = np.argsort(win, axis=-1, kind="stable")
    v0 = np.take_along_axis(win, order[..., :1], -1)[..., 0]
    v1 = np.take_along_axis(win, order[..., 1:2], -1)[..., 0]
    close = np.isfinite(v1) & ((v1 - v0) <= CLOSE * v1)
    mask = np.zeros((b, c, h + 2, w + 2), dtype=bool)
    for j in range(9):
        dy, dx = divmod(j, 3)
        mask[:, :, dy:dy + h, dx:dx + w] |= close & ((order[..., 0] == j) | (order[..., 1] == j))
    return mask[:, :, 1:-1, 1:-1]


def value_ratio(dev, h64, h32):
    """|dev - h64| over the bound 4 * max(|h32 - h64|, 2^-23 |h64|); <= 1 passes. 0 / 0 (an exact zero on both sides) is 0."""
    bound = 4.0 * max(abs(h32 - h64), 2.0 ** -23 * abs(h64))
    err = abs(float(dev) - h64)
    return 0.0 if err == 0.0 else (np.inf if bound == 0.0 else err / bound)


def half_ulp(values, dtype):
    """Half a unit in the last place of `dtype` at |values| (float64 array); 0 for float32 (the bound has its own floor)."""
    if dtype == torch.float32:
        return np.zeros_like(values)
    a = np.maximum(np.abs(values), 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)
    return 0.5 * 2.0 ** (np.floor(np.log2(a)) - MANT[dtype])


def grad_ratio(dev, g64, g32, dtype=torch.float32, mask=None):
    """Largest |dev - g64| (less half an ulp of a 16-bit output) over max(4 max|g32 - g64|, 2^-22 max|g64|), both sides over the
    elements the mask keeps; <= 1 passes."""
    keep = np.ones(g64.shape, dtype=bool) if mask is None else ~mask
    if not keep.any():
        return 0.0
    bound = max(4.0 * np.abs(g32 - g64)[keep].max(), 2.0 ** -22 * np.abs(g64).max())
    err = np.abs(dev - g64) - half_ulp(np.maximum(np.abs(dev), np.abs(g64)), dtype)
    worst = err[keep].max()
    return 0.0 if worst <= 0.0 else (np.inf if bound == 0.0 else float(worst / bound))
