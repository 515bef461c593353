"""Shared by tests/test_steptail_host.py and tests/test_steptail_kernels.py: the float64 reference of the training-step tail
(torch.optim.SGD + clip_grad_norm_ + torch.amp.GradScaler("cpu"), the reference's optimiser stack of R:train.py:367-372, run in
float64) and the per-element error bound of the fp32 forms against it.

The bound. The fp32 forms (openpcseg_amd.optim.sgd_tail_host and the kernels of csrc/steptail.hip) run, per element,

    g1 = g * inv_scale;  g2 = g1 * coef;  wp = wd * p;  d = g2 + wp;  mb = mu * buf;  buf' = mb + d;
    nesterov:  nb = mu * buf';  d2 = d + nb      else  d2 = buf'
    u = (-lr) * d2;  p' = p + u

with ONE fp32 rounding per operation. A rounding to nearest errs by at most EPS = 2^-24 times the magnitude of the value it rounds,
so with e_x the bound on |x_fp32 - x_float64| every operation contributes EPS * (|x_float64| + e_x before rounding) on top of what
its operands carry (a product carries operand error times the other factor, a sum the sum of its operands' errors). Two inputs are
themselves rounded: inv_scale = float32(1 / scale) (relative EPS; none without a scaler) and coef, which the fp32 forms compute as
max_norm / (float32(norm) * inv_scale + 1e-6f): the norm's one rounding, the product, the sum and the quotient each add a relative
EPS and the constant's own rounding is smaller still, so coef carries at most 5 EPS relative (min(., 1) does not enlarge an error;
none without max_norm). The hyper-parameters of the cases are fp32-representable, so both sides use the same numbers. The errors
e_p and e_buf are carried from step to step. This bounds operand magnitudes, not ulps of the result: where p + u nearly cancels the
bound is many ulps of the result, and it has to be -- torch's own fp32 CPU SGD fuses some of these pairs into FMAs and differs from
the float64 run by thousands of ulps of such a result, while staying inside this bound (fewer roundings, never more), which the
host test asserts. The float64 side's own rounding (2^-53 relative) is 2^-29 of the bound and is not counted.
"""
import numpy as np
import torch

EPS = 2.0 ** -24


def f32r(x):
    """x rounded to fp32, as a Python float: a hyper-parameter both precisions can hold."""
    return float(np.float32(x))


def make_tensors(sizes, seed, scale=1.0, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        return [torch.randint(-8, 9, (n,), generator=g).to(torch.float32) for n in sizes]
    return [torch.randn(n, generator=g, dtype=torch.float32) * scale for n in sizes]


class Float64Tail:
    """torch.optim.SGD + clip_grad_norm_ + GradScaler("cpu") in float64 over copies of `params`; `step(grads)` runs one tail and
    advances the error bounds e_p / e_buf of an fp32 form that started from the same state and saw the same gradients."""

    def __init__(self, params, groups, hyper, max_norm=None, scaler=None):
        self.params = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in params]
        self.groups, self.hyper, self.max_norm = list(groups), list(hyper), max_norm
        self.opt = torch.optim.SGD([{"params": [p for p, g in zip(self.params, groups) if g == gi], "lr": lr, "weight_decay": wd,
                                     "momentum": mu, "nesterov": nesterov} for gi, (lr, wd, mu, nesterov) in enumerate(hyper)], lr=1.0)
        self.scaler = None
        if scaler is not None:
            self.scaler = torch.amp.GradScaler("cpu", **scaler)
            self.scaler.scale(torch.zeros((), dtype=torch.float64))   # places the scale (GradScaler is lazy)
        self.e_p = [np.zeros(p.numel()) for p in params]
        self.e_buf = [np.zeros(p.numel()) for p in params]
        self.total_norm = None

    def scale(self):
        return 1.0 if self.scaler is None else float(self.scaler.get_scale())

    def tracker(self):
        return int(self.scaler._get_growth_tracker())

    def bufs(self):
        return [self.opt.state[p].get("momentum_buffer") for p in self.params]

    def step(self, grads):
        """grads: fp32 tensors as the fp32 form sees them (scaled, under a scaler; None: no gradient). Returns found_inf."""
        from torch.nn.utils import clip_grad_norm_
        scale = self.scale()
        before = [(p.detach().numpy().copy().ravel(), None if b is None else b.numpy().copy().ravel())
                  for p, b in zip(self.params, self.bufs())]
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.detach().cpu().double().clone()
        found = any(g is not None and not bool(torch.isfinite(g).all()) for g in grads)
        if self.scaler is not None:
            self.scaler.unscale_(self.opt)
        coef = 1.0
        if self.max_norm is not None:
            self.total_norm = float(clip_grad_norm_(self.params, self.max_norm))
            coef = min(self.max_norm / (self.total_norm + 1e-6), 1.0)
        else:
            self.total_norm = float(np.sqrt(sum(float(p.grad.square().sum()) for p in self.params if p.grad is not None)))
        if self.scaler is not None:
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            self.opt.step()
        if self.scaler is not None and found:
            return True      # a skipped step: nothing moved, the bounds stay
        for i, (g, gi) in enumerate(zip(grads, self.groups)):
            if g is None:
                continue
            lr, wd, mu, nesterov = self.hyper[gi]
            p, buf = before[i]
            buf = np.zeros_like(p) if buf is None else buf
            self.e_p[i], self.e_buf[i] = _advance(g.detach().cpu().double().numpy().ravel(), p, buf, 1.0 / scale, coef, lr, wd, mu, nesterov,
                                                  self.e_p[i], self.e_buf[i], self.scaler is not None, self.max_norm is not None)
        return False


def _rounded(x, e):
    """(magnitude, error) of a value after its one rounding: e in, e + EPS * (|x| + e) out."""
    return e + EPS * (np.abs(x) + e)


def _advance(g, p, buf, inv_scale, coef, lr, wd, mu, nesterov, e_p, e_buf, has_scaler, has_clip):
    g1 = g * inv_scale
    e = _rounded(g1, np.abs(g1) * (EPS if has_scaler else 0.0))
    g2 = g1 * coef
    e = _rounded(g2, e * coef + (np.abs(g1) + e) * (5 * EPS * coef if has_clip else 0.0))
    wp = wd * p
    e_wp = _rounded(wp, wd * e_p)
    d = g2 + wp
    e_d = _rounded(d, e + e_wp)
    if mu != 0:
        mb = mu * buf
        e_mb = _rounded(mb, mu * e_buf)
        nbuf = mb + d
        e_buf = _rounded(nbuf, e_mb + e_d)
        if nesterov:
            nb = mu * nbuf
            e_nb = _rounded(nb, mu * e_buf)
            d, e_d = d + nb, _rounded(d + nb, e_d + e_nb)
        else:
            d, e_d = nbuf, e_buf
    u = lr * d
    e_u = _rounded(u, lr * e_d)
    e_p = _rounded(p - u, e_p + e_u)
    return e_p, e_buf


def assert_within(ref, params, bufs, what):
    """Every element of the fp32 state within the carried bound of the float64 state. Prints the worst ratio."""
    worst = 0.0
    for i, (p64, p32) in enumerate(zip(ref.params, params)):
        pairs = [(p64.detach().numpy().ravel(), p32.detach().cpu().double().numpy().ravel(), ref.e_p[i], "p")]
        b64 = ref.bufs()[i]
        if b64 is not None and bufs[i] is not None:
            pairs.append((b64.numpy().ravel(), bufs[i].detach().cpu().double().numpy().ravel(), ref.e_buf[i], "buf"))
        for a, b, e, name in pairs:
            if a.size == 0:
                continue
            err = np.abs(a - b)
            k = int(np.argmax(err - e))
            assert err[k] <= e[k], "%s: tensor %d %s[%d]: |%.9g - %.9g| = %.3g > bound %.3g" % (what, i, name, k, b[k], a[k], err[k], e[k])
            worst = max(worst, float((err / np.maximum(e, 1e-300)).max()))
    return worst
