"""CPU tests of the training-step tail (openpcseg_amd/optim.py, csrc/steptail.hip): the C ABI is declared and exported, the host
form -- reached through FusedSGD on CPU parameters -- follows the reference's optimiser stack run in float64 within the bound
derived in tests/steptail_cases.py, equals torch.optim.SGD bit for bit where every value is exactly representable, trades
state_dicts with torch.optim.SGD / torch.amp.GradScaler, and refuses what it does not serve."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.nn.utils import clip_grad_norm_

import steptail_cases as sc
from openpcseg_amd import native, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 7, 64, 129, 500, 1000, 33, 2048, 5, 4097, 260]   # 12 tensors of mixed sizes


def test_step_symbols():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    lib = native.load_library()
    for name in ("pcs_step_plan", "pcs_step_norm", "pcs_step_apply"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"\}\s*pcs_step_job\s*;", hdr) and ctypes.sizeof(native._StepJob) == 48
    assert int(re.search(r"#define PCS_STEP_BLOCK_ELEMS (\d+)", hdr).group(1)) == native.STEP_BLOCK_ELEMS == optim.BLOCK_ELEMS
    assert int(re.search(r"#define PCS_STEP_MAX_GROUPS (\d+)", hdr).group(1)) == native.STEP_MAX_GROUPS == optim.MAX_GROUPS
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12


def test_step_plan_on_the_host():
    """pcs_step_plan needs no device: first_block, the block count at the edges of the block constant, and its refusals."""
    lib, E = native.load_library(), native.STEP_BLOCK_ELEMS
    hy = native._StepHyper()
    hy.n_groups, hy.mu[0], hy.mu[1] = 2, 0.9, 0.0
    numels = [0, 1, E - 1, E, E + 1, 3 * E + 1, 0]
    arr = (native._StepJob * len(numels))()
    for j, n in zip(arr, numels):
        j.p, j.g, j.buf, j.numel, j.group = 4096, 8192, 12288, n, 0
    assert lib.pcs_step_plan(ctypes.byref(arr), len(numels), ctypes.byref(hy)) == 0 + 1 + 1 + 1 + 2 + 4 + 0
    assert [j.first_block for j in arr] == [0, 0, 1, 2, 3, 5, 9]

    def refused(**kw):
        one = (native._StepJob * 1)()
        one[0].p, one[0].g, one[0].buf, one[0].numel, one[0].group = 4096, 8192, 12288, 10, 0
        for k, v in kw.items():
            setattr(one[0], k, v)
        rc = lib.pcs_step_plan(ctypes.byref(one), 1, ctypes.byref(hy))
        return rc == -1 and b"pcs_step_plan" in lib.pcs_last_error()
    assert not refused()
    assert refused(numel=-1) and refused(group=2) and refused(group=-1) and refused(p=None) and refused(g=None)
    assert refused(buf=None)             # group 0 has momentum: it needs its buffer
    assert refused(group=1)              # group 1 has none: a buffer does not go with it
    assert not refused(group=1, buf=None)
    assert refused(p=4098)               # not 4-byte aligned
    hy.n_groups = 9
    assert refused()


def _hyper(nesterov, momentum, two_groups):
    hy = [(sc.f32r(0.24), sc.f32r(1e-4), sc.f32r(momentum), nesterov)]
    if two_groups:
        hy.append((sc.f32r(0.024), sc.f32r(5e-4), sc.f32r(momentum), nesterov))
    return hy


def _grads_of_step(step, scale):
    """Six steps: the clip (max_norm 10) is active on the large ones and idle on the small ones; step 2 carries an inf."""
    mag = [1.0, 0.02, 1.0, 0.5, 0.01, 2.0][step]
    grads = sc.make_tensors(SIZES, 100 + step, scale=mag * scale)
    if step == 2:
        grads[4][17] = float("inf")
    return grads


CASES = {"nesterov": (True, 0.9, False), "plain-momentum-two-groups": (False, 0.9, True), "no-momentum": (False, 0.0, False),
         "nesterov-two-groups": (True, 0.5, True)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("with_scaler", [False, True], ids=["noscaler", "scaler"])
def test_host_form_follows_the_float64_stack(case, with_scaler):
    nesterov, momentum, two = CASES[case]
    hyper = _hyper(nesterov, momentum, two)
    groups = [(i % 2 if two else 0) for i in range(len(SIZES))]
    cfg = dict(init_scale=8.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2) if with_scaler else None
    start = sc.make_tensors(SIZES, 7)
    ref = sc.Float64Tail(start, groups, hyper, max_norm=10.0, scaler=cfg)

    def grouped(params):
        return [{"params": [p for p, g in zip(params, groups) if g == gi], "lr": lr, "weight_decay": wd, "momentum": mu, "nesterov": nv}
                for gi, (lr, wd, mu, nv) in enumerate(hyper)]
    mine = [torch.nn.Parameter(p.clone()) for p in start]
    opt = optim.FusedSGD(grouped(mine), lr=1.0)
    scaler = optim.LossScaler(**cfg) if with_scaler else None
    # torch's own fp32 CPU stack: it must stay inside the same bound, or the bound would be a convenient one
    theirs = [torch.nn.Parameter(p.clone()) for p in start]
    topt = torch.optim.SGD(grouped(theirs), lr=1.0)
    tscaler = None
    if with_scaler:
        tscaler = torch.amp.GradScaler("cpu", **cfg)
        tscaler.scale(torch.zeros(()))
    skipped = []
    for step in range(6):
        scale = ref.scale()
        grads = _grads_of_step(step, scale)
        if not with_scaler and step == 2:
            grads[4][17] = 1.0      # without a scaler nothing skips a step: torch itself would write NaNs
        before = [p.detach().clone() for p in mine]
        found = ref.step(grads)
        for p, g in zip(mine, grads):
            p.grad = g.clone()
        opt.step(max_norm=10.0, scaler=scaler)
        for p, g in zip(theirs, grads):
            p.grad = g.clone()
        if tscaler is not None:
            tscaler.unscale_(topt)
        clip_grad_norm_(theirs, 10.0)
        if tscaler is not None:
            tscaler.step(topt)
            tscaler.update()
        else:
            topt.step()
        for p, g in zip(mine, grads):
            assert torch.equal(p.grad, g)       # the documented difference from torch: gradients are never written
        if with_scaler:
            assert bool(opt.found_inf) == found
            assert scaler.get_scale() == ref.scale() == tscaler.get_scale()
            assert scaler.state_dict()["_growth_tracker"] == ref.tracker()
        if found:
            skipped.append(step)
            assert all(torch.equal(a, b) for a, b in zip(before, mine))
            assert ref.scale() == scale * 0.5 and ref.tracker() == 0
        else:
            assert abs(float(opt.total_norm) / ref.total_norm - 1) <= 2 * sc.EPS
        bufs = [opt.state[p].get("momentum_buffer") for p in mine]
        w1 = sc.assert_within(ref, mine, bufs, "host form, step %d" % step)
        w2 = sc.assert_within(ref, theirs, [topt.state[p].get("momentum_buffer") for p in theirs], "torch fp32, step %d" % step)
        print("step %d: worst error / bound: host form %.3f, torch fp32 %.3f" % (step, w1, w2))
    assert skipped == ([2] if with_scaler else [])
    if with_scaler:     # 8 -> (two clean steps) 16 -> (inf) 8 -> (two clean steps) 16, tracker 1 after the sixth
        assert scaler.get_scale() == 16.0 and scaler.state_dict()["_growth_tracker"] == 1


def _integer_problem():
    sizes = [1, 5, 64, 129, 300]
    return sc.make_tensors(sizes, 3, integer=True), [sc.make_tensors(sizes, 10 + s, integer=True) for s in range(3)]


def test_host_form_equals_torch_sgd_on_representable_data():
    """Integers, lr 0.5, mu 0.5, wd 0.25, the norm below max_norm (coef == 1.0): every intermediate is exact in fp32, fused or
    not, so the host form and fp32 torch.optim.SGD agree bit for bit over three steps."""
    start, grads = _integer_problem()
    for nesterov in (False, True):
        mine = [torch.nn.Parameter(p.clone()) for p in start]
        theirs = [torch.nn.Parameter(p.clone()) for p in start]
        kw = dict(lr=0.5, momentum=0.5, weight_decay=0.25, nesterov=nesterov)
        opt, topt = optim.FusedSGD(mine, **kw), torch.optim.SGD(theirs, **kw)
        for gs in grads:
            for p, q, g in zip(mine, theirs, gs):
                p.grad, q.grad = g.clone(), g.clone()
            opt.step(max_norm=1e4)
            assert float(clip_grad_norm_(theirs, 1e4)) < 1e4
            topt.step()
            assert float(opt.total_norm) < 1e4
            for p, q in zip(mine, theirs):
                assert torch.equal(p, q)
                assert torch.equal(opt.state[p]["momentum_buffer"], topt.state[q]["momentum_buffer"])
        # the function itself, on plain tensors, gives what the optimizer gave
        ps, bs = [p.clone() for p in start], [torch.zeros_like(p) for p in start]
        for gs in grads:
            rec = optim.sgd_tail_host(ps, gs, bs, [0] * len(ps), [(0.5, 0.25, 0.5, nesterov)], max_norm=1e4)
            assert rec["coef"] == 1.0 and not rec["found_inf"] and rec["inv_scale"] == 1.0
        assert all(torch.equal(a, b) for a, b in zip(ps, mine))
        # total_norm= overrides the norm: a tenth of max_norm / norm scales the step
        ps2 = [p.clone() for p in start]
        rec = optim.sgd_tail_host(ps2, grads[0], [torch.zeros_like(p) for p in start], [0] * len(ps2), [(0.5, 0.25, 0.5, nesterov)],
                                  max_norm=1.0, total_norm=4.0)
        assert rec["total_norm"] == 4.0 and rec["coef"] == np.float32(1.0) / np.float32(np.float32(4.0) + np.float32(1e-6))


def test_state_dict_round_trip_with_torch_sgd():
    start, grads = _integer_problem()
    kw = dict(lr=0.5, momentum=0.5, weight_decay=0.25, nesterov=True)

    def run(make_first, make_second):
        ps = [torch.nn.Parameter(p.clone()) for p in start]
        first = make_first(ps, **kw)
        for gs in grads[:2]:
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            first.step()
        second = make_second(ps, lr=0.125)       # the loaded state brings its own hyper-parameters
        second.load_state_dict(first.state_dict())
        assert second.param_groups[0]["lr"] == 0.5 and second.param_groups[0]["nesterov"] is True
        for p, g in zip(ps, grads[2]):
            p.grad = g.clone()
        second.step()
        return ps, [second.state[p]["momentum_buffer"] for p in ps]
    want = run(torch.optim.SGD, torch.optim.SGD)
    for a, b in ((optim.FusedSGD, torch.optim.SGD), (torch.optim.SGD, optim.FusedSGD), (optim.FusedSGD, optim.FusedSGD)):
        got = run(a, b)
        for x, y in zip(want[0] + want[1], got[0] + got[1]):
            assert torch.equal(x, y), (a.__name__, b.__name__)
    sd = optim.FusedSGD([torch.nn.Parameter(torch.ones(3))], lr=0.1, momentum=0.9).state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["param_groups"][0]["dampening"] == 0


def test_loss_scaler_state_dict_trades_with_gradscaler():
    mine = optim.LossScaler(init_scale=1024.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7)
    p = torch.nn.Parameter(torch.ones(4))
    opt = optim.FusedSGD([p], lr=0.1)
    p.grad = torch.ones(4)
    assert float(mine.scale(torch.tensor(2.0))) == 2048.0
    opt.step(scaler=mine)                                   # one clean step: tracker 1
    theirs = torch.amp.GradScaler("cpu")
    theirs.load_state_dict(mine.state_dict())
    assert set(mine.state_dict()) == set(torch.amp.GradScaler("cpu").state_dict())
    assert theirs.state_dict() == mine.state_dict() == {"scale": 1024.0, "growth_factor": 4.0, "backoff_factor": 0.25,
                                                        "growth_interval": 7, "_growth_tracker": 1}
    back = optim.LossScaler()
    ref = torch.amp.GradScaler("cpu", init_scale=32.0, growth_interval=3)
    back.load_state_dict(ref.state_dict())
    assert back.state_dict() == ref.state_dict() and back.get_scale() == 32.0
    p.grad = torch.full((4,), float("nan"))
    keep = p.detach().clone()
    opt.step(scaler=back)
    assert back.get_scale() == 16.0 and torch.equal(p, keep) and float(opt.found_inf) == 1.0


def test_parameter_without_gradient_is_untouched():
    a, b, c = (torch.nn.Parameter(torch.full((5,), v)) for v in (1.0, 2.0, 3.0))
    opt = optim.FusedSGD([a, b, c], lr=0.5, momentum=0.5)
    a.grad, c.grad = torch.ones(5), torch.ones(5)
    opt.step(max_norm=100.0)
    assert torch.equal(b, torch.full((5,), 2.0)) and "momentum_buffer" not in opt.state[b]
    assert torch.equal(a, torch.full((5,), 0.5)) and torch.equal(c, torch.full((5,), 2.5))
    assert float(opt.total_norm) == float(np.float32(np.sqrt(10.0)))
    opt.zero_grad()
    opt.step()                                              # no gradient anywhere: nothing to do
    assert torch.equal(a, torch.full((5,), 0.5)) and opt.total_norm is None


def test_ineligible_configurations_raise():
    def p(dtype=torch.float32):
        return torch.nn.Parameter(torch.ones(4, 6, dtype=dtype))
    route = "use torch.optim.SGD"
    for make in (lambda: optim.FusedSGD([p(torch.float64)], lr=0.1),
                 lambda: optim.FusedSGD([p(torch.bfloat16)], lr=0.1),
                 lambda: optim.FusedSGD([torch.nn.Parameter(torch.ones(6, 4).t())], lr=0.1),
                 lambda: optim.FusedSGD([p()], lr=0.1, momentum=0.9, dampening=0.1),
                 lambda: optim.FusedSGD([p()], lr=0.1, maximize=True),
                 lambda: optim.FusedSGD([{"params": [p()]} for _ in range(optim.MAX_GROUPS + 1)], lr=0.1),
                 lambda: optim.FusedSGD([p(), torch.nn.Parameter(torch.ones(3, device="meta"))], lr=0.1)):
        with pytest.raises(ValueError, match=route):
            make()
    assert optim.FusedSGD([{"params": [p()]} for _ in range(optim.MAX_GROUPS)], lr=0.1) is not None
    # at the step: what arrived after construction
    w = p()
    opt = optim.FusedSGD([w], lr=0.1)
    w.grad = torch.ones(6, 4).t()
    assert not w.grad.is_contiguous()
    with pytest.raises(ValueError, match=route):
        opt.step()
    w.grad = torch.ones(4, 6)
    opt.param_groups[0]["dampening"] = 0.5
    with pytest.raises(ValueError, match=route):
        opt.step()
    opt.param_groups[0]["dampening"] = 0
    with pytest.raises(TypeError, match=route):
        opt.step(scaler=torch.amp.GradScaler("cpu"))
    with pytest.raises(ValueError):
        opt.step(max_norm=-1.0)
    with pytest.raises(ValueError):
        optim.FusedSGD([p()], lr=0.1, nesterov=True)
    assert torch.equal(w, torch.ones(4, 6))                 # nothing above moved it
    opt.step()
    assert torch.equal(w, torch.full((4, 6), np.float32(1.0) + np.float32(-0.1) * np.float32(1.0)))
