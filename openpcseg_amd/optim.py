"""The tail of a training step on the device: unscale, clip and SGD in two launches.

The reference ends every voxel / fusion iteration with (R:train.py:367-372, R:pcseg/optim/__init__.py:15-34)

    scaler.unscale_(optimizer); clip_grad_norm_(params, 10); scaler.step(SGD(momentum, weight_decay, nesterov)); scaler.update()

which torch runs as about seven passes over every parameter behind a Python loop over ~200 tensors, and which under fp16 blocks
the host once per step to read `found_inf`. Here:

    opt = FusedSGD(model.parameters(), lr=0.24, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = LossScaler()                        # fp16 only
    scaler.scale(loss).backward()
    opt.step(max_norm=10, scaler=scaler)         # two launches, no host synchronisation
    opt.total_norm, opt.found_inf                # device tensors: what clip_grad_norm_ would have returned, the overflow flag

`sgd_tail_host` is the contract: the same sequence in fp32 torch operations with one rounding each. The kernels of
csrc/steptail.hip equal it bit for bit whenever they are given the same norm (their norm is a double sum folded in a fixed order, so
it can differ from the host's double sum in the last fp32 bit, and then everything scaled by the clip coefficient follows).

One difference from torch: the gradients are never written. After a step `p.grad` still holds what backward left there, scaled by
the loss scale and unclipped, where torch's `unscale_` and `clip_grad_norm_` overwrite it. Code that reads gradients after the step
(logging their norm, say) reads `opt.total_norm` instead.
"""
import math

import numpy as np
import torch

from . import native

BLOCK_ELEMS = native.STEP_BLOCK_ELEMS   # elements of one parameter tensor a workgroup covers (PCS_STEP_BLOCK_ELEMS)
MAX_GROUPS = native.STEP_MAX_GROUPS

_ROUTE = "; use torch.optim.SGD for this configuration"


def _f32(x):
    return float(np.float32(x))


def ineligible(param_groups, with_grads=False):
    """THE eligibility rule of FusedSGD: None, or the reason the configuration is not served. fp32 contiguous parameters (and,
    `with_grads`, gradients) on one device, dampening 0, not maximize, at most MAX_GROUPS groups."""
    if len(param_groups) > MAX_GROUPS:
        return "%d parameter groups (at most %d)" % (len(param_groups), MAX_GROUPS)
    device, f32, strided = None, torch.float32, torch.strided
    for gi, group in enumerate(param_groups):
        if group.get("dampening", 0) != 0:
            return "group %d: dampening %r (only 0)" % (gi, group["dampening"])
        if group.get("maximize", False):
            return "group %d: maximize" % gi
        for p in group["params"]:
            t, what = p, "parameter"
            while t is not None:
                if t.dtype is not f32:
                    return "group %d: a %s of dtype %s (only float32)" % (gi, what, t.dtype)
                if t.layout is not strided or not t.is_contiguous():
                    return "group %d: a %s that is not dense and contiguous" % (gi, what)
                d = t.device
                if device is None:
                    if d.type not in ("cpu", "cuda"):
                        return "group %d: a %s on a %s device" % (gi, what, d.type)
                    device = d
                elif d != device:
                    return "group %d: a %s on %s beside tensors on %s (one device)" % (gi, what, d, device)
                t, what = (p.grad, "gradient") if with_grads and t is p else (None, None)
    return None


def sgd_tail_host(params, grads, bufs, groups, hyper, *, max_norm=None, scaler=None, total_norm=None):
    """The host form of the step tail, which is the contract of the kernels. In place on `params` and `bufs`.

    params, grads, bufs: lists of fp32 tensors of equal shapes (bufs[i] is None where the group's momentum is 0); groups[i]: the
    index into hyper = [(lr, weight_decay, momentum, nesterov)]. The hyper-parameters are rounded to fp32 once.
    Record, returned as a dict of numpy float32 scalars (found_inf a bool):
        total_norm = float32(sqrt(float64 sum of squares)), or the `total_norm=` override (a norm computed elsewhere, the device's)
        inv_scale  = float32(1 / float64(scale)), 1 without a scaler
        coef       = min(max_norm / (total_norm * inv_scale + 1e-6), 1) in fp32 with a NaN kept, 1 without max_norm
        found_inf  = any gradient value is inf or NaN
        unscaled_norm = total_norm * inv_scale (what clip_grad_norm_ returns after unscale_)
    With a scaler (a LossScaler) torch.amp.GradScaler.update's rule is then applied to it, and a step that found an inf writes
    nothing else. Otherwise per element, as separate fp32 operations (never add(alpha=), which may fuse):
        g1 = g * inv_scale; g2 = g1 * coef; d = g2 + wd * p; buf = mu * buf + d; d = nesterov ? d + mu * buf : buf; p = p + (-lr) * d
    """
    with np.errstate(all="ignore"):
        found_inf = any(not bool(torch.isfinite(g).all()) for g in grads)
        if total_norm is None:
            total = 0.0
            for g in grads:
                total += float(g.double().square().sum())
            total_norm = np.float32(math.sqrt(total))
        else:
            total_norm = np.float32(float(total_norm))
        inv_scale = np.float32(1.0)
        if scaler is not None:
            scale = np.float32(scaler._host_scale())
            inv_scale = np.float32(1.0 / np.float64(scale))
        unscaled = np.float32(total_norm * inv_scale)
        coef = np.float32(1.0)
        if max_norm is not None:
            c = np.float32(np.float32(max_norm) / np.float32(unscaled + np.float32(1e-6)))
            coef = np.float32(1.0) if c > 1.0 else c
        if scaler is not None:
            scaler._host_update(found_inf)
    record = {"total_norm": total_norm, "inv_scale": inv_scale, "coef": coef, "found_inf": found_inf, "unscaled_norm": unscaled}
    if scaler is not None and found_inf:
        return record
    inv, cf = float(inv_scale), float(coef)
    for p, g, buf, gi in zip(params, grads, bufs, groups):
        lr, wd, mu, nesterov = hyper[gi]
        lr, wd, mu = _f32(lr), _f32(wd), _f32(mu)
        g2 = torch.mul(torch.mul(g, inv), cf)
        d = torch.add(g2, torch.mul(p, wd))
        if mu != 0:
            buf.mul_(mu)
            buf.add_(d)
            d = torch.add(d, torch.mul(buf, mu)) if nesterov else buf
        p.add_(torch.mul(d, -lr))
    return record


class LossScaler:
    """torch.amp.GradScaler's loss scale with `scale` and `growth_tracker` resident on the device, updated by the norm launch of
    FusedSGD.step(scaler=...): no `found_inf` read, no host synchronisation per step. The tensors are placed on the device of the
    first loss that is scaled (or of the first step's parameters). state_dict / load_state_dict use GradScaler's keys, so the
    reference's `scaler_state` checkpoints load. get_scale() is the one call that synchronises."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1:
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1 and growth_interval >= 1")
        self._init_scale = float(init_scale)
        self._init_growth_tracker = 0
        self.growth_factor = float(growth_factor)
        self.backoff_factor = float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._scale = None
        self._growth_tracker = None

    def _place(self, device):
        if self._scale is None or self._scale.device != torch.device(device):
            scale, tracker = self._host_scale(), self._host_tracker()
            self._scale = torch.full((), scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((), tracker, dtype=torch.int32, device=device)

    def scale(self, loss):
        """loss * scale, on the loss's device."""
        self._place(loss.device)
        return loss * self._scale

    def _host_scale(self):
        return self._init_scale if self._scale is None else float(self._scale)

    def _host_tracker(self):
        return self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker)

    def _host_update(self, found_inf):
        """GradScaler.update's rule on the host (the host form; the device form is in the norm kernel)."""
        scale, tracker = np.float32(self._host_scale()), self._host_tracker()
        if found_inf:
            scale, tracker = np.float32(np.float64(scale) * self.backoff_factor), 0
        else:
            tracker += 1
            if tracker == self.growth_interval:
                grown = np.float32(np.float64(scale) * self.growth_factor)
                scale, tracker = (grown if np.isfinite(grown) else scale), 0
        self._init_scale, self._init_growth_tracker = float(scale), int(tracker)
        if self._scale is not None:
            self._scale.fill_(float(scale))
            self._growth_tracker.fill_(int(tracker))

    def get_scale(self):
        """The current scale as a Python float: reads the device word, so it waits for the device."""
        return self._host_scale()

    def state_dict(self):
        return {"scale": self._host_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._host_tracker()}

    def load_state_dict(self, state):
        if not state:
            raise RuntimeError("LossScaler.load_state_dict: an empty state (saved by a disabled GradScaler)")
        self._init_scale = float(state["scale"])
        self._init_growth_tracker = int(state["_growth_tracker"])
        self.growth_factor = float(state["growth_factor"])
        self.backoff_factor = float(state["backoff_factor"])
        self.growth_interval = int(state["growth_interval"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


class FusedSGD(torch.optim.Optimizer):
    """torch.optim.SGD (dampening 0) whose step is the device tail of csrc/steptail.hip: gradient norm, clip, loss-scale handling
    and the update in two launches over all parameters, one launch without `max_norm` and `scaler`. A torch.optim.Optimizer, so LR
    schedulers, param_groups (per-group lr, weight_decay, momentum, nesterov: the reference's `sgd_fc`) and step hooks work as
    with SGD, and state_dict() has SGD's layout (`momentum_buffer`) and loads into and from torch.optim.SGD. Parameters on the CPU
    take `sgd_tail_host`. What `ineligible` refuses raises, at construction or at the step."""

    def __init__(self, params, lr, momentum=0, weight_decay=0, nesterov=False, dampening=0, maximize=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: negative lr / momentum / weight_decay")
        if nesterov and momentum <= 0:
            raise ValueError("FusedSGD: Nesterov momentum requires a momentum")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize))
        self._refuse(ineligible(self.param_groups))
        self._cache = {}       # device job table + norm workspace, kept while the pointers stay the same
        self._record = None    # 8 device floats: the norm launch's record (include/pcseg_hip.h)
        self.total_norm = None
        self.found_inf = None

    @staticmethod
    def _refuse(reason):
        if reason is not None:
            raise ValueError("openpcseg_amd.optim.FusedSGD does not serve " + reason + _ROUTE)

    @torch.no_grad()
    def step(self, closure=None, *, max_norm=None, scaler=None):
        """One update. max_norm: clip the global gradient norm as clip_grad_norm_(params, max_norm) does; scaler: a LossScaler
        whose scale the gradients carry -- they are unscaled on the fly, an overflowed step leaves parameters and momentum
        untouched, and the scale is updated. Afterwards self.total_norm (the unscaled norm, before clipping) and self.found_inf
        (1.0 / 0.0) are tensors on the parameters' device, views of one buffer that the next step overwrites; None when the step
        had neither max_norm nor scaler. Parameters without a gradient are left out."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if max_norm is not None and not float(max_norm) >= 0:
            raise ValueError("FusedSGD.step: max_norm must be >= 0")
        if scaler is not None and not isinstance(scaler, LossScaler):
            raise TypeError("FusedSGD.step: scaler must be an openpcseg_amd.optim.LossScaler" + _ROUTE)
        self._refuse(ineligible(self.param_groups, with_grads=True))
        jobs, hyper = [], []
        for gi, group in enumerate(self.param_groups):
            mu = _f32(group["momentum"])
            hyper.append((float(group["lr"]), float(group["weight_decay"]), mu, bool(group["nesterov"])))
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                buf = None
                if mu != 0:
                    state = self.state[p]
                    buf = state.get("momentum_buffer")
                    if buf is None:   # the first step: mu * 0 + d == d, torch's clone of d
                        buf = state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    elif not buf.is_contiguous() or buf.dtype != torch.float32 or buf.device != p.device:
                        buf = state["momentum_buffer"] = buf.to(device=p.device, dtype=torch.float32).contiguous()
                jobs.append((p, g, buf, gi))
        norm = max_norm is not None or scaler is not None
        self.total_norm = self.found_inf = None
        if not jobs:
            return loss
        dev = jobs[0][0].device
        if scaler is not None:
            scaler._place(dev)
        if dev.type == "cpu":
            rec = sgd_tail_host([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], hyper,
                                max_norm=max_norm, scaler=scaler)
            if norm:
                self.total_norm = torch.tensor(float(rec["unscaled_norm"]), dtype=torch.float32)
                self.found_inf = torch.tensor(float(rec["found_inf"]), dtype=torch.float32)
            return loss
        if norm and (self._record is None or self._record.device != dev):
            self._record = torch.zeros(8, dtype=torch.float32, device=dev)
        native.backend().step_tail(self._cache, jobs, hyper, record=self._record if norm else None, max_norm=max_norm,
                                   scaler=None if scaler is None else (scaler._scale, scaler._growth_tracker, scaler.growth_factor,
                                                                       scaler.backoff_factor, scaler.growth_interval))
        if norm:
            self.total_norm, self.found_inf = self._record[4], self._record[3]
        return loss
