"""Generate tests/golden/rangeloss_golden.npz: the reference's range-view training criterion on two small inputs.

Needs the reference's sources (so it runs where they are present; the .npz is committed). It RUNS, unmodified,
  CrossEntropyDiceLoss(reduction='none'), Lovasz_softmax(ignore=0), BoundaryLoss()      R:pcseg/model/segmentor/range/utils.py:509-724
composed as the segmentors compose them (R:pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:62-84):
  loss = 1.0 * mean(CE + Dice) + 3.0 * Lovasz + 1.0 * Boundary
on the CPU, in float64 and in float32. utils.py is loaded from its path under the stand-in packages of make_rangescan_golden.py, so
that no package __init__ of the reference runs. One more stand-in, for the float64 run only: lovasz_softmax_flat and lovasz_grad
(utils.py:425-486) cast the foreground with `.float()`, which makes their torch.dot refuse float64 probabilities; while the float64
record is taken, torch.Tensor.float is torch.Tensor.double, so those casts follow the precision of the run. No line of the
reference changes, and the float32 record runs without it.

Inputs: logits (2, 20, 9, 70) and (3, 17, 5, 33), seeded normal times 3; labels constant on blocks of 3 x 7 pixels, class 0
included; the last image of each input draws its blocks from four classes only, so most classes are absent from it.

Recorded per case c<i>_ and precision (64 / 32): ced (the mean of CE + Dice), ls, bd, total and the gradient by the logits (grad64; the float32
one as grad32_delta = grad32 - float32(grad64), an exact difference: grad32 = float32(grad64) + grad32_delta bit for bit); also the
reference's 20 SemanticKITTI class weights (ClassWeightSemikitti.get_weight, utils.py:344-368). Data only.

Seed guards, asserted here (change the seed if one fails):
  * no 3 x 3 window whose two smallest float64 probabilities lie within 1e-5 relative of each other;
  * rangeloss.range_criterion_host in float64 equals the reference's float64 record (terms and gradient, 1e-10 relative).

    python tests/golden/make_rangeloss_golden.py
"""
import importlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, OUT)

CASES = (((2, 20, 9, 70), 11), ((3, 17, 5, 33), 12))   # (shape, seed)
BLOCK = (3, 7)
SCALE = 3.0
WEIGHTS = (1.0, 3.0, 1.0)


def make_case(shape, seed):
    """-> logits float32 (B, C, H, W), labels int64 (B, H, W): block-constant, class 0 present, the last image from four classes."""
    b, c, h, w = shape
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal(shape) * SCALE).astype(np.float32)
    bh, bw = BLOCK
    labels = np.zeros((b, h, w), dtype=np.int64)
    for n in range(b):
        pool = np.arange(c) if n < b - 1 else np.array([0, 2, 5, c - 1])
        blocks = rng.choice(pool, size=(-(-h // bh), -(-w // bw)))
        blocks[0, 0] = 0
        labels[n] = np.repeat(np.repeat(blocks, bh, axis=0), bw, axis=1)[:h, :w]
    return logits, labels


def close_window_share(probas, rel=1e-5):
    """Share of the 3 x 3 windows (clipped) of (B, C, H, W) float64 probabilities whose two smallest values are within `rel`."""
    b, c, h, w = probas.shape
    pad = np.full((b, c, h + 2, w + 2), np.inf)
    pad[:, :, 1:-1, 1:-1] = probas
    win = np.stack([pad[:, :, dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=-1)
    win.sort(axis=-1)
    close = (win[..., 1] - win[..., 0]) <= rel * win[..., 1]
    close &= np.isfinite(win[..., 1])
    return float(close.mean())


class float_is_double:
    """torch.Tensor.float -> torch.Tensor.double while the float64 record is taken (see the module docstring)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import torch
        self.saved = torch.Tensor.float
        if self.on:
            torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        import torch
        torch.Tensor.float = self.saved


def main():
    import torch
    import torch.nn.functional as F
    from stage_reference import reference_root
    from make_golden import save_npz_stable
    from make_rangescan_golden import stand_ins
    from openpcseg_amd import rangeloss
    stand_ins(reference_root())
    utils = importlib.import_module("pcseg.model.segmentor.range.utils")
    torch.set_num_threads(1)
    out = {"weights": np.array(WEIGHTS), "semkitti_weight": np.array(utils.ClassWeightSemikitti.get_weight(), dtype=np.float64),
           "shapes": np.array([s for s, _ in CASES], dtype=np.int64)}
    for i, (shape, seed) in enumerate(CASES):
        logits, labels = make_case(shape, seed)
        pre = "c%d_" % i
        out[pre + "logits"], out[pre + "labels"] = logits, labels.astype(np.int8)
        assert (labels == 0).any() and len(np.unique(labels[-1])) <= 4
        for bits, dtype in ((64, torch.float64), (32, torch.float32)):
            x = torch.from_numpy(logits).to(dtype).requires_grad_(True)
            y = torch.from_numpy(labels)
            wce = utils.CrossEntropyDiceLoss(reduction="none")
            ced = wce(x, y).contiguous().view(-1).mean()
            with float_is_double(bits == 64):
                ls = utils.Lovasz_softmax(ignore=0)(F.softmax(x, dim=1), y).mean()
            bd = utils.BoundaryLoss()(F.softmax(x, dim=1), y)
            total = WEIGHTS[0] * ced + WEIGHTS[1] * ls + WEIGHTS[2] * bd
            with float_is_double(bits == 64):
                total.backward()
            rec = {"ced": ced, "ls": ls, "bd": bd, "total": total}
            for key, val in rec.items():
                out["%s%s%d" % (pre, key, bits)] = np.float64(val.item())
            if bits == 64:
                out[pre + "grad64"] = x.grad.numpy().copy()
            else:   # a few units in the last place around the rounded float64 record: stored as that difference, which compresses
                out[pre + "grad32_delta"] = x.grad.numpy() - out[pre + "grad64"].astype(np.float32)
                assert np.array_equal(out[pre + "grad64"].astype(np.float32) + out[pre + "grad32_delta"], x.grad.numpy())
            if bits == 64:
                share = close_window_share(F.softmax(x.detach(), dim=1).numpy())
                assert share == 0.0, (pre, "a window with two close minima: pick another seed", share)
                xh = torch.from_numpy(logits).double().requires_grad_(True)
                h_total, (h_ce, h_dice, h_ls, h_bd) = rangeloss.range_criterion_host(xh, y, weights=WEIGHTS, dtype=torch.float64)
                h_total.backward()
                for name, a, r in (("ced", h_ce + h_dice, ced), ("ls", h_ls, ls), ("bd", h_bd, bd), ("total", h_total, total)):
                    assert abs(a.item() - r.item()) <= 1e-10 * abs(r.item()), (pre, name, a.item(), r.item())
                gerr = (xh.grad - x.grad).abs().max().item()
                assert gerr <= 1e-10 * x.grad.abs().max().item(), (pre, "host gradient", gerr)
            print("%s float%d: ced %.9g ls %.9g bd %.9g total %.9g" % (pre, bits, ced.item(), ls.item(), bd.item(), total.item()))
    path = os.path.join(OUT, "rangeloss_golden.npz")
    save_npz_stable(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
