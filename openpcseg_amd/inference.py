"""Inference mode: BatchNorm folded into the convolutions, and the prediction tail on the device.

    openpcseg_amd.freeze(model)           # opt-in; model.eval() + torch.no_grad() / inference_mode() then take the folded path
    ev = SegEvaluator(num_class)
    for batch in loader:
        model.predict(batch, evaluator=ev)        # workloads.minkunet.MinkUNet.predict
    hist, iou, miou = ev.compute()                # the only device-to-host copy

In eval mode a BatchNorm is a per-column affine map, so every `conv -> BatchNorm (-> + residual) (-> ReLU)` chain of the
package's own blocks becomes ONE launch of the fused gather-GEMM:

    s  = gamma / sqrt(running_var + eps)      (float64, as FusedBatchNorm's eval branch computes its inverse deviation)
    W' = W * s[None, None, :]  -> fp32        b' = beta - running_mean * s (+ conv.bias * s)  -> fp32
    y  = act(conv(x, W') + b' [+ residual])   bias, addend and ReLU in the write-back (pcs_conv_epilogue, PCS_EP_RELU)

The fold is plain torch arithmetic on the device, done once per weight version (no host read-back); the folded tensors
are ordinary attributes of a record beside the module, so `state_dict()` and the parameter lists are what they were. The
folded path is taken only while the module is frozen, in eval mode and grad mode is off (it has no autograd): `model.train()`
needs no `unfreeze`. A record remembers the version counters (and storage addresses) of the kernel, the conv bias and the
BatchNorm's weight / bias / running statistics and re-folds lazily when any of them changed (`load_state_dict`, an optimizer
step between two evaluations). The half kernels' fragment-ordered copies of W' live in the same record, so a frozen forward
after the first launches no weight preparation.

Cylinder3D's blocks run conv -> LeakyReLU -> BatchNorm (+ residual): the scale sits BEHIND the activation and gamma may be negative,
so it does not commute into the weights (and a fold into the next sparse convolution would carry the shift only to the neighbours
that exist). There the BatchNorm rides in the same launch as a per-column affine map behind the activation (`PostAffineConv`,
PCS_EP_POST_AFFINE): W stays what it is, the write-back computes leaky(conv + bias) * s + t (+ residual), one rounding on the store.
"""
import functools

import numpy as np
import torch
from torch import nn

from . import functional as F
from . import modules as spnn
from . import native
from .fused import FusedBatchNorm
from .hostdata import raw_frames, scene_row_offsets
from .linear import devoxelized_linear
from .sparse import SparseTensor

__all__ = ["freeze", "unfreeze", "FoldedConv", "PostAffineConv", "FoldedDense", "SegEvaluator", "point_predict", "predict_tta"]

_NORMS = (FusedBatchNorm, nn.BatchNorm1d)   # spnn.BatchNorm and the models' _BN / _SyncBN are BatchNorm1d / SyncBatchNorm
_ATTR = "_pcs_folds"


def _is_norm(m):
    return isinstance(m, _NORMS) or isinstance(m, nn.SyncBatchNorm)


def _foldable(conv, bn):
    return (isinstance(conv, spnn.Conv3d) and _is_norm(bn) and getattr(bn, "running_mean", None) is not None and
            getattr(bn, "running_var", None) is not None and conv.out_channels == bn.num_features)


def _stamp_of(tensors):
    """(version, address, device, dtype) of every source tensor, or None where one of them tracks no version counter."""
    stamp = []
    for t in tensors:
        if t is None:
            stamp.append(None)
            continue
        try:
            stamp.append((t._version, t.data_ptr(), t.device, t.dtype))
        except RuntimeError:   # inference tensors track no version counter: fold on every call
            return None
    return tuple(stamp)


def _bn_sources(bn):
    return [getattr(bn, "weight", None), getattr(bn, "bias", None), bn.running_mean, bn.running_var]


def _bn_affine(bn):
    """The eval-mode BatchNorm as y = x * s + t: (s, t) in float64 on the device of the running statistics."""
    gamma, beta, mean, var = _bn_sources(bn)
    s = torch.rsqrt(var.detach().double() + bn.eps)
    if gamma is not None:
        s = gamma.detach().double() * s
    t = -mean.detach().double() * s
    if beta is not None:
        t = t + beta.detach().double()
    return s, t


class _FoldRecord:
    """What a frozen module keeps beside itself for one of its layers, and the one rule for "is it still current": `refresh`
    stamps the tensors `_sources()` names, and where the stamp moved (or cannot be taken) it calls `_fold()` under no_grad, empties
    the dict of derived copies and counts. A subclass supplies `_sources()` and `_fold()`; DERIVED names its dict of copies that
    depend on the sources (None: it keeps none)."""
    DERIVED = None
    COUNTED = True   # `folds`: how often the BatchNorm arithmetic ran (tests); a record without any carries no counter

    def __init__(self):
        self._stamp = None
        if self.DERIVED:
            setattr(self, self.DERIVED, {})
        if self.COUNTED:
            self.folds = 0

    def _fold(self):
        pass

    def refresh(self):
        stamp = _stamp_of(self._sources())
        if stamp is None or stamp != self._stamp:
            with torch.no_grad():
                self._fold()
            if self.DERIVED:
                setattr(self, self.DERIVED, {})
            self._stamp = stamp
            if self.COUNTED:
                self.folds += 1


class FoldedConv(_FoldRecord):
    """conv + the BatchNorm that follows it as one convolution with bias; `relu`: the chain ends in a ReLU. `prepared`: the
    derived copies of `weight` (functional.conv3d_inference), dropped with it."""
    DERIVED = "prepared"

    def __init__(self, conv, bn, relu):
        super().__init__()
        self.conv, self.bn, self.relu = conv, bn, bool(relu)
        self.weight = self.bias = None

    def _sources(self):
        return [self.conv.kernel, self.conv.bias] + _bn_sources(self.bn)

    def _fold(self):
        s, t = _bn_affine(self.bn)
        if self.conv.bias is not None:
            t = t + self.conv.bias.detach().double() * s
        self.weight = (self.conv.kernel.detach().double() * s).float().contiguous()
        self.bias = t.float().contiguous()

    def folded(self):
        """-> (W' fp32, b' fp32, the dict of derived copies), re-folded when a source tensor changed."""
        self.refresh()
        return self.weight, self.bias, self.prepared

    def __call__(self, x, residual=None):
        w, b, prepared = self.folded()
        c = self.conv
        return F.conv3d_inference(x, w, b, c.kernel_size, stride=c.stride, dilation=c.dilation, transposed=c.transposed,
                                  addend=residual, relu=self.relu, prepared=prepared)


class PostAffineConv(_FoldRecord):
    """conv -> LeakyReLU(slope) -> BatchNorm (+ residual) as one launch with the BatchNorm as the affine map behind the activation:
    scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, float64 arithmetic stored as fp32; the kernel
    `W` is used as it is. bn None (UpBlock.up_subm): a plain convolution whose record only keeps the derived weight copies
    (`prepared`, dropped when the kernel changes); the `residual` of such a record is the ordinary addend."""
    DERIVED = "prepared"

    def __init__(self, conv, bn=None, slope=None):
        super().__init__()
        self.conv, self.bn, self.slope = conv, bn, (float(slope) if slope is not None else None)
        self.scale = self.shift = None

    def _sources(self):
        return [self.conv.kernel, self.conv.bias] + (_bn_sources(self.bn) if self.bn is not None else [])

    def _fold(self):
        if self.bn is not None:
            s, t = _bn_affine(self.bn)
            self.scale, self.shift = s.float().contiguous(), t.float().contiguous()

    def folded(self):
        """-> (scale fp32, shift fp32, the dict of derived copies), re-folded when a source tensor changed."""
        self.refresh()
        return self.scale, self.shift, self.prepared

    def __call__(self, x, residual=None):
        scale, shift, prepared = self.folded()
        c = self.conv
        return F.conv3d_inference(x, c.kernel.detach(), c.bias.detach() if c.bias is not None else None, c.kernel_size, stride=c.stride,
                                  dilation=c.dilation, transposed=c.transposed, addend=residual, prepared=prepared,
                                  act_slope=self.slope, post_scale=scale, post_shift=shift)


class FoldedDense(_FoldRecord):
    """nn.Linear with the BatchNorm in front of it (`bn_in`: W diag(s), b + W t) and / or behind it (`bn_out`: diag(s) W, s b + t)
    folded in, float64 arithmetic stored as fp32: the point MLPs of Cylinder3D."""

    def __init__(self, lin, bn_in=None, bn_out=None):
        super().__init__()
        self.lin, self.bn_in, self.bn_out = lin, bn_in, bn_out
        self.weight = self.bias = None

    def _sources(self):
        return [self.lin.weight, self.lin.bias] + [t for bn in (self.bn_in, self.bn_out) if bn is not None for t in _bn_sources(bn)]

    def _fold(self):
        w = self.lin.weight.detach().double()   # (out, in)
        b = self.lin.bias.detach().double() if self.lin.bias is not None else torch.zeros(w.shape[0], dtype=w.dtype, device=w.device)
        if self.bn_in is not None:
            s, t = _bn_affine(self.bn_in)
            b = b + w @ t
            w = w * s[None, :]
        if self.bn_out is not None:
            s, t = _bn_affine(self.bn_out)
            w, b = w * s[:, None], b * s + t
        self.weight, self.bias = w.float().contiguous(), b.float().contiguous()

    def folded(self):
        self.refresh()
        return self.weight, self.bias

    def __call__(self, x):
        w, b = self.folded()
        return torch.nn.functional.linear(x, w, b)


class FoldedLinear(_FoldRecord):
    """The classifier's column blocks (FusedLinear.devoxelized_part) with their (1, cin, cout) gather-GEMM weights and fragment-ordered
    half copies kept per weight version (`parts`) instead of being transposed and prepared on every forward
    (`linear.devoxelized_linear`, memo): the logits are bit-identical to the unfrozen classifier's. No BatchNorm, no arithmetic."""
    DERIVED, COUNTED = "parts", False

    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def _sources(self):
        return [self.lin.weight]

    def devoxelized_part(self, col, xf, idx, wts, cache=None):
        if cache is None:   # no per-forward dict for the identity map: the module's own path
            return self.lin.devoxelized_part(col, xf, idx, wts)
        self.refresh()
        return devoxelized_linear(self.lin.weight, col, xf, idx, wts, cache, memo=self.parts.setdefault((col, xf.shape[1]), {}))


def active(module):
    """The fold records of `module` when the folded path applies to this call (frozen, eval mode, grad mode off), else None."""
    rec = module.__dict__.get(_ATTR)
    if rec is None or module.training or torch.is_grad_enabled():
        return None
    return rec


def _groups(seq):
    """A Sequential made only of [Conv3d, BatchNorm (, ReLU)] groups -> [(conv, bn, relu)], else None."""
    mods, out, i = list(seq), [], 0
    while i < len(mods):
        if i + 1 >= len(mods) or not _foldable(mods[i], mods[i + 1]):
            return None
        relu = i + 2 < len(mods) and isinstance(mods[i + 2], (spnn.ReLU, nn.ReLU)) and not isinstance(mods[i + 2], nn.LeakyReLU)
        out.append((mods[i], mods[i + 1], relu))
        i += 3 if relu else 2
    return out or None


class _SequentialForward:
    """`forward` of a frozen plain Sequential (an instance attribute, so the class and its state_dict stay what they were;
    a class rather than a closure so that the module still pickles)."""

    def __init__(self, seq):
        self.seq = seq

    def __call__(self, x):
        rec = active(self.seq)
        if rec is None or not isinstance(x, SparseTensor):
            return type(self.seq).forward(self.seq, x)
        for f in rec["chain"]:
            x = f(x)
        return x


def freeze(model):
    """Fold every BatchNorm of the package's own blocks (workloads.minkunet, workloads.spvcnn and workloads.rpvnet: the stem, ConvBlock, ResBlock
    incl. its 1x1x1 downsample) and of plain `nn.Sequential(Conv3d, BatchNorm [, ReLU], ...)` chains into its convolution. Of
    workloads.cylinder: the conv -> LeakyReLU -> BatchNorm triples of ResContextBlock / ResBlock / UpBlock become one launch each
    (PostAffineConv), the BatchNorms of the point MLPs fold into their Linear (FoldedDense); ReconNet's three keep running inside
    the gate kernel on the running statistics and are reported as skipped. Anything else is left alone. -> {"folded": number of BatchNorm modules that stop launching, "skipped": [names of BatchNorm modules that keep running]}.
    Changes no parameter, buffer or state_dict entry; takes effect only in eval mode with grad mode off.

    A module with a frozen path says so itself: `fold_records()` -> (the record dict its forward reads through `active`, the
    modules it claims: the BatchNorms that stop launching and any child Sequential the plain-Sequential pass must leave alone),
    or None where its layout is not the expected one."""
    unfreeze(model)
    claimed, folded = set(), 0

    def attach(owner, rec, claims):
        nonlocal folded
        owner.__dict__[_ATTR] = rec
        claimed.update(id(c) for c in claims)
        folded += sum(1 for c in claims if _is_norm(c))

    for m in model.modules():
        plan = m.fold_records() if callable(getattr(m, "fold_records", None)) else None
        if plan:
            attach(m, *plan)
    for m in model.modules():
        if isinstance(m, nn.Sequential) and type(m).forward is nn.Sequential.forward and id(m) not in claimed:
            groups = _groups(m)
            if groups:
                attach(m, {"chain": [FoldedConv(c, b, r) for c, b, r in groups]}, [b for _, b, _ in groups])
                m.__dict__["forward"] = _SequentialForward(m)
    skipped = [name for name, m in model.named_modules() if _is_norm(m) and id(m) not in claimed]
    return {"folded": folded, "skipped": skipped}


def unfreeze(model):
    """Drop every fold record `freeze` attached below `model` (the modules run their BatchNorm layers again). -> how many."""
    n = 0
    for m in model.modules():
        rec = m.__dict__.pop(_ATTR, None)
        if rec is not None:
            n += 1
            if "chain" in rec:
                m.__dict__.pop("forward", None)
    return n


# ---- prediction tail ------------------------------------------------------------------------------------------------
def _scene_offsets(batch_col, n_scenes):
    """hostdata.scene_row_offsets of a batch column that comes from outside: clamped to the scenes the host side of the batch names."""
    return scene_row_offsets(batch_col.long().clamp(0, n_scenes - 1), n_scenes)


def point_predict(logits, batch, votes=None, hist=None, bad=None):
    """The reference's eval tail (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:436-455) for the whole batch in one
    launch: point_predict = logits[rows of scene b][inverse_map of scene b][:num_points[b]].argmax(1), scenes concatenated.
    batch: "lidar" (SparseTensor, coords (m, 4), batch index last, scenes in order as sparse_collate_fn leaves them),
    "inverse_map" (SparseTensor: F (n,) per-scene row of every point, C batch index last), optional "targets_mapped" (F (n,)
    labels), optional "num_points" (host, per scene). The number of scenes comes from the host side of the batch.
    votes (sum kept points, c) fp32: += softmax of every point's row, then decides (the reference's return_tta, summed);
    hist (c, c) int64: += confusion counts of labels in [0, c). -> (pred (sum kept points,) int64 on the device, host list of the
    (n_scenes + 1) offsets into it, bad flag (1,) int32 on the device: an inverse index pointed outside its scene)."""
    logits = logits.float().contiguous()
    maps, labels, kept = _batch_maps(batch, logits.device)
    pred, bad = native.backend().predict_points(logits, labels=labels if hist is not None else None, votes=votes, hist=hist, bad=bad, **maps)
    return pred, kept, bad


def scene_sizes(num_points):
    """A batch's "num_points" (tensor, array, list or None) -> host list of ints, or None."""
    if num_points is None:
        return None
    if isinstance(num_points, torch.Tensor):
        num_points = num_points.cpu()   # host data in every loader of the reference; a device tensor costs a read-back
    return [int(v) for v in np.asarray(num_points).reshape(-1)]


def _batch_maps(batch, dev):
    """The batch of `point_predict` as the tail kernel wants it -> ({"inverse", "point_offset", "row_offset"} on the device, the
    labels of the kept points or None, the host offsets of the kept points or None where no `num_points` says them)."""
    inv = batch["inverse_map"]
    inverse = inv.F.to(dev).long().reshape(-1)
    labels = batch["targets_mapped"].F.to(dev).long().reshape(-1) if batch.get("targets_mapped") is not None else None
    n = inverse.numel()
    num_points = scene_sizes(batch.get("num_points"))
    if num_points is not None:
        ns = len(num_points)
    elif batch.get("offset") is not None:
        ns, num_points = len(batch["offset"]), None
    else:
        raise ValueError("openpcseg_amd: the batch needs `num_points` or `offset` (the number of scenes, known on the host)")
    row_offset = _scene_offsets(batch["lidar"].C.to(dev)[:, -1], ns)
    if num_points is None or sum(num_points) == n:
        # every scene keeps all its points (`[:num_points[idx]]` cuts nothing)
        if num_points is None:
            point_offset = _scene_offsets(inv.C.to(dev)[:, -1], ns)
            kept = None
        else:
            kept = [0] + np.cumsum(num_points).tolist()
            point_offset = native._h2d(kept, torch.int64, dev) if dev.type == "cuda" else torch.tensor(kept, dtype=torch.int64)
    else:
        # shortened spans: point j of scene b's kept prefix is point start[b] + j of the batch; all sizes known on the host
        kept = [0] + np.cumsum(num_points).tolist()
        start = _scene_offsets(inv.C.to(dev)[:, -1], ns)
        scene = torch.repeat_interleave(torch.arange(ns), torch.tensor(num_points)).to(dev)
        kept_dev = torch.tensor(kept, dtype=torch.int64).to(dev)
        src = torch.arange(kept[-1], device=dev) - kept_dev[scene] + start[scene]
        inside = src < start[scene + 1]           # a scene with fewer points than num_points says: refused, not read
        src = src.clamp(max=max(n - 1, 0))
        inverse = torch.where(inside, inverse[src], torch.full_like(src, -1))
        labels = labels[src] if labels is not None else None
        point_offset = kept_dev
    return {"inverse": inverse, "point_offset": point_offset, "row_offset": row_offset}, labels, kept


def predict_output(logits, batch, evaluator=None, votes=None):
    """Eval logits -> what the models' `predict` returns: {"logits" fp32, "point_predict", "point_offset"}, through `evaluator`
    (a SegEvaluator, which also counts) or the plain tail."""
    logits = logits.float()
    if evaluator is not None:
        pred = evaluator.update(logits, batch, votes=votes)
        offsets = evaluator.last_offsets
    else:
        pred, offsets, _ = point_predict(logits, batch, votes=votes)
    return {"logits": logits, "point_predict": pred, "point_offset": offsets}


class SegEvaluator:
    """Confusion matrix of an evaluation run, kept on the device: `update` per batch (no host synchronisation), `compute` once.
    num_class = the width of the logits; unique_label as in the reference's trainer (R:train.py:226-230: class 0 is `ignore`,
    label k + 1 is evaluated class k), default range(num_class - 1)."""

    def __init__(self, num_class, unique_label=None):
        self.num_class = int(num_class)
        self.unique_label = np.asarray(list(range(self.num_class - 1)) if unique_label is None else unique_label, dtype=np.int64)
        if self.unique_label.size == 0 or self.unique_label.min() < 0 or int(self.unique_label.max()) + 2 > self.num_class:
            raise ValueError("openpcseg_amd: unique_label + 1 must index classes of the (num_class, num_class) histogram")
        self.hist = None   # (num_class, num_class) int64 on the device of the first update
        self.bad = None    # (1,) int32: some inverse index pointed outside its scene (that point was not counted)

    def _ensure(self, device):
        if self.hist is None:
            with torch.inference_mode(False):   # ordinary tensors also when first used inside MinkUNet.predict (merge adds in place)
                self.hist = torch.zeros((self.num_class, self.num_class), dtype=torch.int64, device=device)
                self.bad = torch.zeros(1, dtype=torch.int32, device=device)

    def tail(self, logits, labels, offsets, count=True, **maps):
        """One launch of the prediction tail on this evaluator's behalf: native predict_points(logits, **maps), with
        hist[label][pred] += 1 over `labels` when `count`, and the out-of-scene flag OR-ed into `bad`. labels None: nothing to count,
        the evaluator's tensors are neither made nor passed. `offsets` (host) become `last_offsets`. -> pred (or None: want_pred)."""
        if logits.shape[1] != self.num_class:
            raise ValueError("openpcseg_amd: %d logit columns for a %d-class evaluator" % (logits.shape[1], self.num_class))
        if labels is not None:
            self._ensure(logits.device)
        count = count and labels is not None
        pred, _ = native.backend().predict_points(logits.float().contiguous(), labels=labels if count else None,
                                                  hist=self.hist if count else None, bad=self.bad if labels is not None else None, **maps)
        self.last_offsets = offsets
        return pred

    def counters(self, num_class, device, offsets, count=True):
        """For a prediction tail that counts inside its OWN launch (rangescan.predict's KNN vote, where `tail` serves predict_points):
        checks the class count, records `offsets` (host) as `last_offsets` and hands out the (num_class, num_class) int64 histogram
        to add hist[label][pred] into, made on `device` at first use. count=False (nothing to count, e.g. no labels): None, and
        the evaluator's tensors are not made."""
        if int(num_class) != self.num_class:
            raise ValueError("openpcseg_amd: %d classes for a %d-class evaluator" % (int(num_class), self.num_class))
        self.last_offsets = offsets
        if not count:
            return None
        self._ensure(device)
        return self.hist

    def update(self, logits, batch, votes=None):
        """hist[label][pred] += 1 over the batch's points (labels: batch["targets_mapped"]). -> pred (flat, on the device)."""
        if batch.get("targets_mapped") is None:
            raise ValueError("openpcseg_amd: SegEvaluator.update needs batch['targets_mapped']")
        maps, labels, kept = _batch_maps(batch, logits.device)
        return self.tail(logits, labels, kept, votes=votes, **maps)

    def merge(self, other):
        """Add another evaluator's counts (what a multi-rank evaluation would all-reduce)."""
        if other.hist is not None:
            self._ensure(other.hist.device)
            self.hist += other.hist.to(self.hist.device)
            self.bad |= other.bad.to(self.bad.device)
        return self

    @staticmethod
    def metrics(hist, unique_label):
        """(cropped histogram, per-class IoU, mIoU) from a full (c, c) histogram: fast_hist_crop + per_class_iu + nanmean
        (R:infer.py:43-52, R:train.py:459-465), in NumPy on the host."""
        hist = np.asarray(hist)
        n = int(np.max(unique_label)) + 2
        h = hist[:n, :n]
        h = h[unique_label + 1, :]
        h = h[:, unique_label + 1]
        iou = np.diag(h) / (h.sum(1) + h.sum(0) - np.diag(h) + 1e-9)
        return h, iou, float(np.nanmean(iou))

    def compute(self):
        """-> (cropped histogram (int64), per-class IoU, mIoU as a fraction): the one device-to-host copy of the run."""
        if self.hist is None:
            raise RuntimeError("openpcseg_amd: SegEvaluator.compute before any update")
        host = torch.cat([self.hist.reshape(-1), self.bad.long()]).cpu().numpy()
        self.saw_bad = bool(host[-1])
        if self.saw_bad:
            import warnings
            warnings.warn("openpcseg_amd: inverse_map entries pointed outside their scene's rows; those points were not counted")
        return self.metrics(host[:-1].reshape(self.num_class, self.num_class), self.unique_label)


# ---- evaluation with test-time augmentation ---------------------------------------------------------------------------------
def predict_tta(model, raw, num_votes=10, evaluator=None, voxel_size=0.05, rng=np.random, vote_chunk=None, return_logits=False,
                scale_range=(0.9, 1.1)):
    """An evaluation of a raw batch resident in HBM under the reference's test-time augmentation (`TTA: True`:
    R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:62-69 and :94-110, ten rotated and rescaled votes per frame, collated as ten scenes;
    R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:445-446 `return_tta` hands out each scene's softmax rows, which are summed
    here): `transform.tta_params` draws the votes from `rng`, `transform.device_batch` builds them from one read
    of the scans, the model's eval forward (`point_logits`, the call `predict` makes) runs over `vote_chunk` votes at a time (None:
    all votes in one forward), and each vote's softmax is added into ONE (n, num_class) fp32 tensor by the prediction tail
    (native.predict_points on that vote's scenes). The decision is the arg-max after the last vote; `evaluator` (a SegEvaluator)
    gets its confusion counts from that decision only, once per point. raw: the dict of workloads.synthetic.make_raw_batch, on the device.
    -> {"pred" (n,) int64, "votes" (n, num_class) fp32, "point_offset": host frame boundaries, "params": the (num_votes *
    num_frames, 8) table drawn} and with return_logits "logits": per vote the (voxels of that vote's scenes, num_class) fp32 logits."""
    from . import transform
    if model.training:
        raise RuntimeError("predict_tta is an evaluation pass: call model.eval() first")
    fn = getattr(model, "point_logits", None)
    if not callable(fn) or isinstance(fn, nn.Module):
        raise TypeError("openpcseg_amd: predict_tta needs a model with a point_logits(lidar) method (MinkUNet, SPVCNN)")
    return vote_loop(raw, "predict_tta", num_votes, vote_chunk, evaluator, return_logits,
                     lambda nf, nv: {"params": transform.tta_params(nf, nv, scale_range=scale_range, rng=rng)},
                     lambda part, k: transform.device_batch(raw, voxel_size, part["params"], votes=k, eval_maps=True),
                     lambda batch, v0, scene_votes: scene_votes(batch, fn(batch["lidar"])))


def vote_loop(raw, caller, num_votes, vote_chunk, evaluator, return_logits, draw, batch_of, logits_of):
    """The voted evaluation of every model (`predict_tta`, `RPVNet.predict_tta`, `CylinderTS.predict_tta`).
    Per vote one launch of the prediction tail adds the softmax of every point's row into one (n, num_class) tensor; the decision
    and the evaluator's counts come from the last vote's launch only. draw(num_frames, num_votes) -> {name: vote-major table},
    handed back; batch_of(part, k) -> the device batch of k votes from their rows `part` of every table (scene j * num_frames + f
    = the chunk's vote j of frame f); logits_of(batch, v0, scene_votes), under inference_mode -> (fp32 contiguous logits, vote)
    with vote(j) -> (the tail's keywords that find vote v0 + j's points in the logits, keep) and keep() -> {name: tensor}: what
    return_logits keeps of that vote, called after the loop. scene_votes(batch, logits) is that pair for a
    `transform.device_batch(..., eval_maps=True)` dict and logits over batch["lidar"]'s rows.
    -> {"pred", "votes", "point_offset", **the tables drawn} and with return_logits a list per kept name (see predict_tta)."""
    pts, labels, off, nf, n = raw_frames(raw, caller, "a model's `predict` on a host-built batch", need_labels=evaluator is not None)
    nv = int(num_votes)
    chunk = nv if vote_chunk is None else max(1, min(int(vote_chunk), nv))
    drawn = draw(nf, nv)
    be = native.backend()
    dev = pts.device
    labels = labels.long().contiguous() if evaluator is not None else None
    point_offset = functools.lru_cache(None)(lambda: native._h2d(off, torch.int64, dev))   # one upload, for callers of scene_votes

    def scene_votes(batch, logits):
        logits = logits.float().contiguous()
        row_offset = _scene_offsets(batch["lidar"].C[:, -1], len(batch["num_points"]))
        bounds = functools.lru_cache(None)(lambda: row_offset.cpu().tolist())   # asked for explicitly: the chunk's only read-back
        inverse = batch["inverse_map"].F

        def vote(j):
            maps = {"inverse": inverse[j * n:(j + 1) * n], "point_offset": point_offset(), "row_offset": row_offset[j * nf:(j + 1) * nf + 1]}
            return maps, lambda: {"logits": logits[bounds()[j * nf]:bounds()[(j + 1) * nf]]}
        return logits, vote

    votes = pred = bad = None   # bad: the flag of a run without evaluator, made by the first launch
    kept = []
    for v0 in range(0, nv, chunk):
        k = min(chunk, nv - v0)
        batch = batch_of({name: table[v0 * nf:(v0 + k) * nf] for name, table in drawn.items()}, k)
        with torch.inference_mode():
            logits, vote = logits_of(batch, v0, scene_votes)
        if votes is None:
            votes = torch.zeros((n, logits.shape[1]), dtype=torch.float32, device=dev)
        for j in range(k):
            last = v0 + j == nv - 1
            maps, keep = vote(j)
            if evaluator is not None:   # every vote's flag goes to the evaluator, the counts come from the last decision only
                pred = evaluator.tail(logits, labels, off, count=last, votes=votes, want_pred=last, **maps)
            else:
                pred, bad = be.predict_points(logits, votes=votes, want_pred=last, bad=bad, **maps)
            if return_logits:
                kept.append(keep)
    out = {"pred": pred, "votes": votes, "point_offset": off, **drawn}
    for keep in kept:
        for name, t in keep().items():
            out.setdefault(name, []).append(t)
    return out
