"""The training criterion of the range-view segmentors on the device.

RangeNet, SalsaNext, FIDNet and CENet all train on (R:pcseg/model/segmentor/range/fidnet/model/semantic/fidnet.py:62-84,
salsanext.py:250-271, cenet.py:248-318; the classes in R:pcseg/model/segmentor/range/utils.py:509-724)

    loss = 1.0 * mean_pixels(CrossEntropy(reduction='none') + Dice) + 3.0 * Lovasz_softmax(ignore=0) + 1.0 * BoundaryLoss(theta0=3)

`range_criterion_host` is that composition restated line by line in torch: the contract, and the fallback. `RangeCriterion`
runs it on device logits in csrc/rangeloss.hip (two passes over the logits and a fold) around the one-sort Lovasz of
csrc/lovasz.hip. The one extension: a label outside [0, C), where the reference raises, is handled like ignore_index -- CE
term 0 but counted in the mean's divisor, no one-hot row, left out of Dice's denominator.
"""
import os

import torch
import torch.nn.functional as F

from .workloads.losses import lovasz_softmax

MAX_CLASSES = 32   # kMaxC of csrc/rangeloss.hip
_LOSSES = ("dice", "wce")


def _check_options(loss, class_weight):
    if loss not in _LOSSES:
        raise ValueError("openpcseg_amd: loss must be 'dice' or 'wce', got %r" % (loss,))
    if class_weight is not None and loss != "wce":
        raise ValueError("openpcseg_amd: class_weight goes with loss='wce' (the shipped 'dice' configs pass none)")


def _dice_loss_multichannel(predictions, targets, ignore_index=-100):
    """DiceLoss._dice_loss_multichannel with weight None (utils.py:581-624)."""
    eps = 0.0001
    encoded_target = predictions.detach() * 0
    mask = targets == ignore_index
    targets = targets.clone()
    targets[mask] = 0
    encoded_target.scatter_(1, targets.unsqueeze(1), 1)
    mask = mask.unsqueeze(1).expand_as(encoded_target)
    encoded_target[mask] = 0
    intersection = predictions * encoded_target
    numerator = 2 * intersection.sum(0).sum(1).sum(1)
    denominator = predictions + encoded_target
    denominator = denominator.masked_fill(mask, 0)
    denominator = denominator.sum(0).sum(1).sum(1)
    if denominator.sum() == 0:
        return denominator.sum()
    denominator = denominator + eps
    loss_per_channel = 1 - (numerator / denominator)
    return loss_per_channel.sum() / predictions.size(1)


def _boundary_loss(pred, gt, valid, theta0=3):
    """BoundaryLoss.forward (utils.py:678-714) on probabilities; an invalid pixel has no one-hot row. As in the reference's
    one_hot (:717-724) the one-hot map is float32 whatever the probabilities are, so sum(gt_b) + 1e-7 is a float32 sum."""
    n, c, _, _ = pred.shape
    eye = torch.eye(c + 1, device=pred.device)[:, :c]   # row c: the all-zero row of an invalid label
    one_hot_gt = eye[torch.where(valid, gt, torch.full_like(gt, c))].transpose(1, 3).transpose(2, 3)
    gt_b = F.max_pool2d(1 - one_hot_gt, kernel_size=theta0, stride=1, padding=(theta0 - 1) // 2)
    gt_b = gt_b - (1 - one_hot_gt)
    pred_b = F.max_pool2d(1 - pred, kernel_size=theta0, stride=1, padding=(theta0 - 1) // 2)
    pred_b = pred_b - (1 - pred)
    gt_b = gt_b.reshape(n, c, -1)
    pred_b = pred_b.reshape(n, c, -1)
    P = torch.sum(pred_b * gt_b, dim=2) / (torch.sum(pred_b, dim=2) + 1e-7)
    R = torch.sum(pred_b * gt_b, dim=2) / (torch.sum(gt_b, dim=2) + 1e-7)
    BF1 = 2 * P * R / (P + R + 1e-7)
    return torch.mean(1 - BF1)


def _squeeze_labels(logits, labels):
    if labels.dim() == 4 and labels.shape[1] == 1:
        labels = labels.squeeze(1)   # what the models do with (B, 1, H, W)
    if logits.dim() != 4 or tuple(labels.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError("openpcseg_amd: range criterion wants (B, C, H, W) logits and (B, H, W) labels, got %s and %s"
                         % (tuple(logits.shape), tuple(labels.shape)))
    return labels.long()


def range_criterion_host(logits, labels, loss="dice", class_weight=None, lovasz=True, boundary=True, weights=(1.0, 3.0, 1.0),
                         lovasz_ignore=0, top_k_percent_pixels=1.0, dtype=torch.float64):
    """The reference's criterion in torch, in `dtype` -> (total, (ce, dice, ls, bd)), differentiable by `logits`.

    CrossEntropyLoss(reduction='none') [+ _dice_loss_multichannel], the mean (or the top-k mean) over the pixels, the Lovasz of
    workloads/losses.py on flatten_probas' rows, BoundaryLoss. Runs wherever the tensors live."""
    _check_options(loss, class_weight)
    labels = _squeeze_labels(logits, labels)
    x = logits.to(dtype)
    b, c, h, w = x.shape
    valid = (labels >= 0) & (labels < c)
    targets = torch.where(valid, labels, torch.full_like(labels, -100))
    cw = None if class_weight is None else torch.as_tensor(class_weight, device=x.device).to(dtype)
    pixel_ce = F.cross_entropy(x, targets, weight=cw, reduction="none", ignore_index=-100)
    zero = x.new_zeros(())
    dice = _dice_loss_multichannel(F.softmax(x, dim=1), targets) if loss == "dice" else zero
    pixel_losses = (pixel_ce + dice).contiguous().view(-1)
    if top_k_percent_pixels == 1.0:
        loss_ce = pixel_losses.mean()
        ce = pixel_ce.mean()
    else:
        top_k_pixels = int(top_k_percent_pixels * pixel_losses.numel())
        pixel_losses, _ = torch.topk(pixel_losses, top_k_pixels)
        loss_ce = pixel_losses.mean()
        ce = loss_ce - dice   # the mean of the CE terms of the kept pixels
    if lovasz:
        probas = F.softmax(x, dim=1).permute(0, 2, 3, 1).contiguous().view(-1, c)
        ls = lovasz_softmax(probas, labels.reshape(-1), ignore=lovasz_ignore, stable=True)   # ties in point order, as the kernel
    else:
        ls = zero
    bd = _boundary_loss(F.softmax(x, dim=1), labels, valid) if boundary else zero
    total = weights[0] * loss_ce + weights[1] * ls + weights[2] * bd
    return total, (ce.detach(), dice.detach(), ls.detach(), bd.detach())


class _RangeCriterionHip(torch.autograd.Function):
    """Statistics pass -> Lovasz (value and gradient in one call) -> fold -> gradient pass; backward is grad * grad_out."""

    @staticmethod
    def forward(ctx, logits, labels, class_weight, flags, lovasz, lovasz_ignore, weights):
        from . import native
        be = native.backend()
        need_grad = ctx.needs_input_grad[0]
        x = logits.detach()
        ws, probas = be.range_loss_stats(x, labels, class_weight, flags, want_probas=lovasz)
        ls = gls = None
        if lovasz:
            ls, gls = be.lovasz_softmax(probas, labels.reshape(-1), lovasz_ignore, need_grad=need_grad)
        terms = be.range_loss_fold(ws, x.shape, flags, ls, weights)
        ctx.grad = be.range_loss_grad(x, labels, ws, class_weight, gls, flags, weights) if need_grad else None
        ctx.mark_non_differentiable(terms)
        return terms[0].clone(), terms

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return (ctx.grad * grad_out.to(ctx.grad.dtype)), None, None, None, None, None, None


class RangeCriterion(torch.nn.Module):
    """loss = weights[0] * mean_pixels(CE [+ Dice]) + weights[1] * Lovasz_softmax(ignore) + weights[2] * BoundaryLoss.

    loss='dice': CrossEntropyDiceLoss(reduction='none'), what every shipped range config sets; loss='wce': CrossEntropyLoss with
    `class_weight`, no Dice term. forward(logits (B, C, H, W), label_rv (B, H, W) or (B, 1, H, W)) -> the 0-dim loss;
    `.last_terms` holds (ce, dice, ls, bd) as a device tensor. Device logits with C <= 32 run in csrc/rangeloss.hip; host
    tensors, more classes, top_k_percent_pixels != 1.0 or PCS_RANGE_LOSS=0 take `range_criterion_host` in float32."""

    def __init__(self, num_class, loss="dice", class_weight=None, lovasz=True, boundary=True, weights=(1.0, 3.0, 1.0),
                 lovasz_ignore=0, top_k_percent_pixels=1.0):
        super().__init__()
        _check_options(loss, class_weight)
        if len(weights) != 3:
            raise ValueError("openpcseg_amd: weights = (ce + dice, lovasz, boundary)")
        self.num_class = int(num_class)
        self.loss = loss
        self.lovasz, self.boundary = bool(lovasz), bool(boundary)
        self.weights = tuple(float(v) for v in weights)
        self.lovasz_ignore = lovasz_ignore
        self.top_k_percent_pixels = float(top_k_percent_pixels)
        cw = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1)
        if cw is not None and cw.numel() != self.num_class:
            raise ValueError("openpcseg_amd: class_weight must hold %d values, got %d" % (self.num_class, cw.numel()))
        self.register_buffer("class_weight", cw)
        self.last_terms = None

    def uses_kernel(self, logits):
        return (logits.is_cuda and 2 <= logits.shape[1] <= MAX_CLASSES and self.top_k_percent_pixels == 1.0 and
                os.environ.get("PCS_RANGE_LOSS", "1") != "0")

    def forward(self, logits, label_rv):
        labels = _squeeze_labels(logits, label_rv)
        if logits.shape[1] != self.num_class:
            raise ValueError("openpcseg_amd: %d logit channels for %d classes" % (logits.shape[1], self.num_class))
        if not self.uses_kernel(logits):
            total, terms = range_criterion_host(logits, labels, self.loss, self.class_weight, self.lovasz, self.boundary,
                                                self.weights, self.lovasz_ignore, self.top_k_percent_pixels, dtype=torch.float32)
            self.last_terms = torch.stack(terms)
            return total
        flags = (1 if self.loss == "dice" else 0) | (2 if self.boundary else 0)
        cw = None if self.class_weight is None else self.class_weight.to(logits.device)
        total, terms = _RangeCriterionHip.apply(logits.contiguous(), labels.contiguous(), cw, flags, self.lovasz,
                                                self.lovasz_ignore, self.weights)
        self.last_terms = terms[1:]
        return total


def cenet_criterion(criterion, logits, aux_logits, label_rv):
    """CENet with IF_AUX (cenet.py:253-288): 1.25 * main + aux1 + aux2 + aux3, per term -> the 0-dim loss;
    `criterion.last_terms` then holds the four combined terms."""
    heads = [(1.25, logits)] + [(1.0, a) for a in aux_logits]
    total, terms = None, None
    for scale, head in heads:
        value = criterion(head, label_rv) * scale
        total = value if total is None else total + value
        terms = criterion.last_terms * scale if terms is None else terms + criterion.last_terms * scale
    criterion.last_terms = terms
    return total
