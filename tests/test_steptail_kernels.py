"""`-m gpu`: the kernels of csrc/steptail.hip behind openpcseg_amd.optim.FusedSGD against the host form (bit for bit wherever both are
given the same norm), against the float64 optimiser stack of tests/steptail_cases.py (its derived bound), against
torch.amp.GradScaler, without host synchronisation, and in place of clip_grad_norm_ + torch.optim.SGD on the ten-iteration
reference trajectory of tests/test_trajectory.py."""
import numpy as np
import pytest
import torch

import steptail_cases as sc
from openpcseg_amd import optim

E = optim.BLOCK_ELEMS
# every path of a job: empty, shorter than a 16-byte access, ragged ends, whole sweeps of the 256 lanes, the block edges, several blocks
NUMELS = [0, 1, 3, 4, 5, 255, 256, 257, E - 1, E, E + 1, 3 * E + 1]
# ... then a tensor that ends exactly on a block boundary followed by a one-element tensor (the workgroup -> job search), and two
# tensors that are views at a one-element offset (4-byte aligned only: the element-wise path)
AFTER = [2 * E, 1]
UNALIGNED = [1000, E + 3]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def device_tensors(host, dev):
    """Device copies of the host tensors; the last len(UNALIGNED) of them as views one element into a larger allocation."""
    out = []
    for i, t in enumerate(host):
        if i >= len(host) - len(UNALIGNED):
            base = torch.zeros(t.numel() + 8, device=dev)
            assert base.data_ptr() % 16 == 0
            view = base[1:1 + t.numel()]
            view.copy_(t)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            out.append(view)
        else:
            out.append(t.to(dev))
    return out


def problem(dev, seed=5, grad_scale=1.0, steps=3):
    sizes = NUMELS + AFTER + UNALIGNED
    start = sc.make_tensors(sizes, seed)
    grads = [sc.make_tensors(sizes, seed + 50 + s, scale=grad_scale) for s in range(steps)]
    params = [torch.nn.Parameter(t) for t in device_tensors(start, dev)]
    return sizes, start, grads, params


def set_grads(params, grads, dev):
    for p, g in zip(params, device_tensors(grads, dev)):
        p.grad = g


CASES = {"nesterov": ([(0.24, 1e-4, 0.9, True)], False), "momentum": ([(0.24, 1e-4, 0.9, False)], False),
         "no-momentum": ([(0.24, 1e-4, 0.0, False)], False),
         "two-groups": ([(0.24, 1e-4, 0.9, True), (0.024, 5e-4, 0.5, False)], True),
         "two-groups-one-without-momentum": ([(0.24, 1e-4, 0.0, False), (0.024, 5e-4, 0.5, True)], True)}


def grouped(params, groups, hyper):
    return [{"params": [p for p, g in zip(params, groups) if g == gi], "lr": lr, "weight_decay": wd, "momentum": mu, "nesterov": nv}
            for gi, (lr, wd, mu, nv) in enumerate(hyper)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_equals_host_form_bit_for_bit(case, hip):
    """coef == 1 and no scaler: nothing depends on the last bit of the norm, so p and buf equal sgd_tail_host bit for bit over three
    steps -- the apply launch alone (steps 0 and 2) and behind a norm launch whose clip is idle (step 1)."""
    hyper, two = CASES[case]
    hyper = [(sc.f32r(lr), sc.f32r(wd), sc.f32r(mu), nv) for lr, wd, mu, nv in hyper]
    dev = torch.device("cuda:0")
    sizes, start, grads, params = problem(dev)
    groups = [(i % 2 if two else 0) for i in range(len(sizes))]
    opt = optim.FusedSGD(grouped(params, groups, hyper), lr=1.0)
    hp = [t.clone() for t in start]
    hb = [torch.zeros_like(t) if hyper[g][2] != 0 else None for t, g in zip(start, groups)]
    for step in range(3):
        set_grads(params, grads[step], dev)
        kw = {"max_norm": 1e9} if step == 1 else {}
        opt.step(**kw)
        rec = optim.sgd_tail_host(hp, grads[step], hb, groups, hyper, **kw)
        if step == 1:
            assert rec["coef"] == 1.0 and float(opt._record[2]) == 1.0
            assert abs(float(opt.total_norm) / float(rec["total_norm"]) - 1) <= 2 * sc.EPS
        else:
            assert opt.total_norm is None
        for i, p in enumerate(params):
            assert same_bits(p, hp[i]), "step %d: parameter %d (numel %d)" % (step, i, sizes[i])
            if hb[i] is not None:
                assert same_bits(opt.state[p]["momentum_buffer"], hb[i]), "step %d: buffer %d (numel %d)" % (step, i, sizes[i])
            else:
                assert "momentum_buffer" not in opt.state[p]
            assert same_bits(p.grad, grads[step][i])       # gradients are never written


def _clip_run(dev, steps=2):
    hyper = [(sc.f32r(0.24), sc.f32r(1e-4), sc.f32r(0.9), True)]
    sizes, start, grads, params = problem(dev, seed=9, steps=steps)
    opt = optim.FusedSGD(params, lr=hyper[0][0], weight_decay=hyper[0][1], momentum=hyper[0][2], nesterov=True)
    norms, states = [], []
    for step in range(steps):
        set_grads(params, grads[step], dev)
        opt.step(max_norm=10.0)
        norms.append(opt._record.clone())
        states.append(([p.detach().clone() for p in params], [opt.state[p]["momentum_buffer"].clone() for p in params]))
    return hyper, sizes, start, grads, norms, states


@pytest.mark.gpu
def test_clip_active(hip):
    dev = torch.device("cuda:0")
    hyper, sizes, start, grads, records, states = _clip_run(dev)
    _, _, _, _, records2, states2 = _clip_run(dev)
    groups = [0] * len(sizes)
    ref = sc.Float64Tail(start, groups, hyper, max_norm=10.0)
    hp, hb = [t.clone() for t in start], [torch.zeros_like(t) for t in start]
    for step in range(len(grads)):
        ref.step(grads[step])
        rec = records[step].cpu().numpy()
        total_norm, coef = rec[0], rec[2]
        assert ref.total_norm > 10.0 and coef < 1.0          # the clip is active
        # the norm: within 1 ulp (fp32) of the float64 norm
        exact = np.float64(ref.total_norm)
        assert abs(np.float64(total_norm) - exact) <= np.spacing(np.float32(exact)), (total_norm, exact)
        assert rec[1] == 1.0 and rec[3] == 0.0 and rec[4] == total_norm
        # two runs: identical bits, the record included (a fixed fold order, no float atomics)
        assert same_bits(records[step], records2[step])
        for a, b in zip(states[step][0] + states[step][1], states2[step][0] + states2[step][1]):
            assert same_bits(a, b)
        # the host form fed with the device's norm: equal bit for bit
        got = optim.sgd_tail_host(hp, grads[step], hb, groups, hyper, max_norm=10.0, total_norm=float(total_norm))
        assert got["coef"] == coef and got["total_norm"] == total_norm
        for i in range(len(sizes)):
            assert same_bits(states[step][0][i], hp[i]), "step %d: parameter %d (numel %d)" % (step, i, sizes[i])
            assert same_bits(states[step][1][i], hb[i]), "step %d: buffer %d (numel %d)" % (step, i, sizes[i])
        # and against the float64 stack the derived bound holds
        worst = sc.assert_within(ref, states[step][0], states[step][1], "device, step %d" % step)
        print("step %d: total_norm %.9g (float64 %.17g), worst error / bound %.3f" % (step, total_norm, exact, worst))


@pytest.mark.gpu
def test_more_work_blocks_than_norm_workgroups(hip):
    """The norm launch has at most 2048 workgroups (8 on each of 256 CUs), each sweeping work blocks b, b + 2048, ...: 2400 tiny
    tensors and one of 3 E + 1 elements make 2404 work blocks, so 356 workgroups take a second one. The norm, the overflow flag
    (an inf in the LAST tensor, a work block only a second sweep reaches) and the update are held as in the other tests."""
    dev = torch.device("cuda:0")
    hyper = [(sc.f32r(0.24), sc.f32r(1e-4), sc.f32r(0.9), True)]
    sizes = [1 + i % 5 for i in range(1200)] + [3 * E + 1] + [1 + i % 3 for i in range(1200)]
    assert sum(-(-n // E) for n in sizes) == 2404
    start, grads = sc.make_tensors(sizes, 31), sc.make_tensors(sizes, 32)
    flat_p, flat_g = torch.cat(start).to(dev), torch.cat(grads).to(dev)     # one allocation each: tensors at every 4-byte alignment
    params = [torch.nn.Parameter(t) for t in flat_p.split(sizes)]
    for p, g in zip(params, flat_g.split(sizes)):
        p.grad = g
    opt = optim.FusedSGD(params, lr=hyper[0][0], weight_decay=hyper[0][1], momentum=hyper[0][2], nesterov=True)
    opt.step(max_norm=10.0)
    exact = np.sqrt(sum(float(g.double().square().sum()) for g in grads))
    total_norm = float(opt.total_norm)
    assert exact > 10.0 and abs(total_norm - exact) <= np.spacing(np.float32(exact)) and float(opt.found_inf) == 0.0
    hp, hb = [t.clone() for t in start], [torch.zeros_like(t) for t in start]
    optim.sgd_tail_host(hp, grads, hb, [0] * len(sizes), hyper, max_norm=10.0, total_norm=total_norm)
    assert same_bits(flat_p, torch.cat(hp))
    assert same_bits(torch.cat([opt.state[p]["momentum_buffer"] for p in params]), torch.cat(hb))
    # an overflow that only a second sweep sees
    scaler = optim.LossScaler(init_scale=4.0)
    flat_g[-1] = float("inf")
    keep = flat_p.clone()
    opt.step(max_norm=10.0, scaler=scaler)
    assert float(opt.found_inf) == 1.0 and scaler.get_scale() == 2.0 and same_bits(flat_p, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["nan-first", "inf-last"])
def test_scaler_skips_and_updates_like_gradscaler(poison, hip):
    dev = torch.device("cuda:0")
    hyper = [(sc.f32r(0.24), sc.f32r(1e-4), sc.f32r(0.9), True)]
    cfg = dict(init_scale=64.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    sizes, start, grads, params = problem(dev, seed=13, grad_scale=64.0, steps=4)
    groups = [0] * len(sizes)
    if poison == "nan-first":
        first = next(i for i, n in enumerate(sizes) if n > 0)      # the table's first tensor with an element
        grads[1][first][0] = float("nan")
    else:
        grads[1][-1][-1] = float("inf")
    opt = optim.FusedSGD(params, lr=hyper[0][0], weight_decay=hyper[0][1], momentum=hyper[0][2], nesterov=True)
    scaler = optim.LossScaler(**cfg)
    ref = sc.Float64Tail(start, groups, hyper, max_norm=10.0, scaler=cfg)
    want_scale = [64.0, 32.0, 32.0, 64.0]      # clean (tracker 1), poisoned (halved, 0), clean (1), clean (doubled, 0)
    want_tracker = [1, 0, 1, 0]
    for step in range(4):
        before = [bits(p) for p in params], [bits(opt.state[p]["momentum_buffer"]) for p in params if opt.state[p]]
        found = ref.step(grads[step])
        set_grads(params, grads[step], dev)
        opt.step(max_norm=10.0, scaler=scaler)
        assert bool(opt.found_inf) == found == (step == 1)
        assert scaler.get_scale() == ref.scale() == want_scale[step]
        assert scaler.state_dict()["_growth_tracker"] == ref.tracker() == want_tracker[step]
        if found:
            after = [bits(p) for p in params], [bits(opt.state[p]["momentum_buffer"]) for p in params]
            assert len(before[1]) == len(params)
            for a, b in zip(before[0] + before[1], after[0] + after[1]):
                assert torch.equal(a, b)                       # p and buf keep their bits
        else:
            assert abs(float(opt.total_norm) / ref.total_norm - 1) <= 3 * sc.EPS     # the unscaled norm, as clip_grad_norm_ returns it
        sc.assert_within(ref, params, [opt.state[p]["momentum_buffer"] for p in params], "device, step %d" % step)


@pytest.mark.gpu
def test_step_does_not_synchronise_the_host(hip):
    dev = torch.device("cuda:0")
    sizes, start, grads, params = problem(dev, seed=21)
    opt = optim.FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = optim.LossScaler(init_scale=4.0)
    set_grads(params, grads[0], dev)
    loss = scaler.scale(torch.ones((), device=dev))
    opt.step(max_norm=10.0, scaler=scaler)           # builds the table
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(max_norm=10.0, scaler=scaler)
        opt.step(max_norm=10.0)
        opt.step()
        norm, flag = opt.total_norm, opt.found_inf
        loss = scaler.scale(loss)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert norm is None and flag is None and float(loss) == 16.0
    assert all(bool(torch.isfinite(p).all()) for p in params)


@pytest.mark.gpu
def test_trajectory_with_the_fused_tail(hip):
    """tests/test_trajectory.py's `workload` route with FusedSGD.step(max_norm=clip) in place of clip_grad_norm_ + torch.optim.SGD,
    held to that test's bounds. The fp32 backward reads _WeightPrep's transposed copies of the weights, so this also shows that
    they are refreshed after a step that wrote the weights through raw pointers."""
    import test_trajectory as tt
    from openpcseg_amd.sparse import SparseTensor
    fs = tt.fs
    g = tt._fixture()
    T = fs.TRAJ
    dev = torch.device("cuda:0")
    feats, coords, labels = (t.to(dev) for t in tt._batch_arrays(g))
    model = tt._model("workload", dev)
    opt = optim.FusedSGD(model.parameters(), lr=T["lr"], momentum=T["momentum"], weight_decay=T["weight_decay"])
    losses, norms = [], []
    for _ in range(T["steps"]):
        model.train()
        opt.zero_grad()
        ret = model({"lidar": SparseTensor(feats.clone(), coords), "targets": SparseTensor(labels, coords), "offset": None})
        loss = ret["loss"].mean()
        loss.backward()
        opt.step(max_norm=T["clip"])
        norms.append(float(opt.total_norm))
        losses.append(float(loss.detach()))
    losses, norms = np.array(losses), np.array(norms)
    loss_err = np.abs(losses / g["losses"] - 1)
    norm_err = np.abs(norms / g["grad_norms"] - 1)
    state = [(n, t) for n, t in model.state_dict().items() if t.dtype.is_floating_point]
    mine = fs.grad_fingerprint(state)
    assert [str(n) for n in mine["grad_names"]] == [str(n) for n in g["state_names"]]
    rs, ms = g["state_stats"], mine["grad_stats"]
    e_abs = np.abs(ms[:, 1] / rs[:, 1] - 1)
    e_smp = np.abs(mine["grad_samples"] - g["state_samples"]).max(1) / rs[:, 2]
    tw = np.concatenate([g["twin_losses"], g["losses"][None]], 0)
    twin_loss = np.max([np.abs(tw[i] / tw[j] - 1) for i in range(len(tw)) for j in range(i)], axis=0)
    t_abs = np.abs(g["twin_state_stats"][:, :, 1] / rs[None, :, 1] - 1).max(0)
    t_smp = (np.abs(g["twin_state_samples"] - g["state_samples"][None]).max(2) / rs[None, :, 2]).max(0)
    m = {"loss_rel_err": [float("%.3g" % v) for v in loss_err], "grad_norm_rel_err": [float("%.3g" % v) for v in norm_err],
         "twin_loss_rel_drift": [float("%.3g" % v) for v in twin_loss], "weights_abssum_rel_err_max": float(e_abs.max()),
         "weights_sample_err_rel_max": float(e_smp.max())}
    print("\n[trajectory] fused tail: %s" % m)
    assert (loss_err <= np.maximum(tt.LOSS_REL, 3 * twin_loss)).all(), m
    assert loss_err[:2].max() < tt.LOSS_REL, m
    assert m["weights_abssum_rel_err_max"] < max(tt.WEIGHT_REL, 3 * float(t_abs.max())), m
    assert m["weights_sample_err_rel_max"] < max(tt.WEIGHT_REL, 3 * float(t_smp.max())), m
    nominal = 3 * twin_loss <= tt.LOSS_REL
    assert nominal[:2].all() and (norm_err[nominal] <= 1e-3).all(), m
