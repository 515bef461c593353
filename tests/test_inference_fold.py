"""Inference mode (openpcseg_amd.freeze): BatchNorm folded into the convolutions, bias + residual + ReLU in the write-back.

CPU part (-m "not gpu"): the fold arithmetic per block and for a whole small model on the pure-PyTorch backend against float64 /
the oracle backend; freeze leaves state_dict alone, is ignored in train / grad mode, re-folds when a source tensor changes
(the one currency rule, held once per record class and source tensor).
GPU part (-m gpu): every layer shape of the MinkUNet workload in one launch against the oracle's conv_fwd on the folded weights;
model level: no BatchNorm call is left, fp32 / bf16 / fp16 errors of the frozen model are bounded by those of the unfrozen one.

Bounds. Folding adds ONE rounding per weight and per bias to a contraction that already has K * cin of them, so the frozen
result is as far from an exact evaluation as the unfrozen one up to sample noise: err(frozen) <= 2 * err(unfrozen) + floor, the
floor being the project's fp32 kernel bound (2e-5 of the tensor maximum, test_dense_parity.close), which keeps a lucky unfrozen
run from failing the test. Half precision at model level: one rounding FEWER per layer, so mean error <= 1.5x, max <= 2x.
"""
import json
import os

import numpy as np
import pytest
import torch

import openpcseg_amd
from openpcseg_amd import cpu_fallback, native
from openpcseg_amd import functional as F
from openpcseg_amd.hostdata import sparse_collate_fn
from openpcseg_amd.sparse import SparseTensor
from openpcseg_amd.workloads import minkunet as mk
from openpcseg_amd.workloads.synthetic import make_batch, make_scan, voxelize_scan
from seeded import seeded_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "inference_parity.json")


# ---- float64 yardstick of one conv -> BatchNorm (-> + residual) (-> ReLU) chain ---------------------------------------
def _kmap_of(x, conv):
    """The kernel map `conv` used on SparseTensor x (already run, so x.kmaps holds it); None for a 1x1x1 convolution."""
    ks, st = tuple(conv.kernel_size), tuple(conv.stride)
    if ks == (1, 1, 1):
        return None
    if conv.transposed:
        out_stride = tuple(x.stride[k] // st[k] for k in range(3))
        return x.kmaps[(out_stride, ks, st, (1, 1, 1))].rev
    return x.kmaps[(tuple(x.stride), ks, st, (1, 1, 1))].fwd


def _chain64(x64, conv, bn, kmap, residual=None, relu=True):
    w = conv.kernel.detach().double()
    w = w if w.dim() == 3 else w[None]
    if kmap is None:
        out = x64 @ w[0]
    else:
        out = torch.zeros((kmap.n_dst, w.shape[2]), dtype=torch.float64)
        pairs, ko = kmap.pairs.long(), kmap.koff_host
        for k in range(kmap.K):
            p = pairs[ko[k]:ko[k + 1]]
            out.index_add_(0, p[:, 1], x64[p[:, 0]] @ w[k])
    if conv.bias is not None:
        out = out + conv.bias.detach().double()
    out = (out - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.detach().double() + bn.bias.detach().double()
    if residual is not None:
        out = out + residual
    return out.clamp_(min=0) if relu else out


def _bound(frozen, unfrozen, ref):
    ref = np.asarray(ref, np.float64)
    ef = float(np.abs(np.asarray(frozen, np.float64) - ref).max())
    eu = float(np.abs(np.asarray(unfrozen, np.float64) - ref).max())
    return ef, eu, 2.0 * eu + 2e-5 * float(np.abs(ref).max())


def _scan_tensor(channels, seed=0, n_points=2000):
    lidar = make_batch([seed], n_points=n_points)["lidar"]
    g = torch.Generator().manual_seed(100 + channels)
    x = SparseTensor(torch.randn(lidar.C.shape[0], channels, generator=g), lidar.C.int().contiguous())
    x.cmaps[x.stride] = x.C   # as initial_voxelize leaves it: a transposed convolution finds its output coordinates here
    return x


def _run(block, x, *args):
    with torch.no_grad():
        return block(x, *args)


@pytest.fixture()
def cpu_be():
    with cpu_fallback.enabled() as b:
        yield b


def test_fold_arithmetic_blocks_cpu(cpu_be):
    """Stem, ConvBlock (strided and transposed), ResBlock with and without downsample on the pure-PyTorch backend: frozen and
    unfrozen against the float64 evaluation of the block's formula."""
    model = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5).eval()
    down, up = mk.ConvBlock(16, 16, 2, 2, False).eval(), mk.ConvBlock(16, 24, 2, 2, False, transposed=True).eval()
    res_same, res_ds = mk.ResBlock(16, 16, False).eval(), mk.ResBlock(16, 32, False).eval()
    holder = torch.nn.ModuleDict({"model": model, "down": down, "up": up, "a": res_same, "b": res_ds})
    seeded_state(holder)
    results = {}

    def both(name, fn):
        openpcseg_amd.unfreeze(holder)
        results[name] = [fn()]
        assert openpcseg_amd.freeze(holder)["skipped"] == []
        results[name].append(fn())

    # stem: 4 -> 16 -> 16
    def stem():
        x = _scan_tensor(4)
        y = _run(model._stem, x)
        h = _chain64(x.F.double(), model.stem[0], model.stem[1], _kmap_of(x, model.stem[0]))
        return y.F, _chain64(h, model.stem[3], model.stem[4], _kmap_of(x, model.stem[3]))
    both("stem", stem)

    def updown():
        x = _scan_tensor(16)
        d = _run(down, x)
        u = _run(up, d)
        rd = _chain64(x.F.double(), down.net[0], down.net[1], _kmap_of(x, down.net[0]))
        ru = _chain64(d.F.double(), up.net[0], up.net[1], _kmap_of(d, up.net[0]))   # the up-conv alone, on the block's own input
        assert u.F.shape == (x.F.shape[0], 24) and d.stride == (2, 2, 2)
        return torch.cat([d.F.reshape(-1), u.F.reshape(-1)]), torch.cat([rd.reshape(-1), ru.reshape(-1)])
    both("convblock", updown)

    def res(block):
        def fn():
            x = _scan_tensor(16)
            y = _run(block, x)
            km = _kmap_of(x, block.net[0])
            h = _chain64(x.F.double(), block.net[0], block.net[1], km)
            r = x.F.double()
            if not isinstance(block.downsample, torch.nn.Identity):
                r = _chain64(r, block.downsample[0], block.downsample[1], None, relu=False)
            return y.F, _chain64(h, block.net[3], block.net[4], km, residual=r)
        return fn
    both("res_same", res(res_same))
    both("res_downsample", res(res_ds))

    for name, ((yu, ref_u), (yf, ref_f)) in results.items():
        # each run against the float64 evaluation on ITS OWN inputs (the up-conv's input is the down-conv's output)
        ef, eu = float((yf.double() - ref_f).abs().max()), float((yu.double() - ref_u).abs().max())
        bound = 2.0 * eu + 2e-5 * float(ref_f.abs().max())
        print("%s: frozen %.3e unfrozen %.3e bound %.3e" % (name, ef, eu, bound))
        assert ef <= bound, (name, ef, eu, bound)
        assert float(yf.min()) >= 0.0   # every one of these chains ends in a ReLU


def _small_batch(n_points=2000):
    b = make_batch([0], n_points=n_points)
    return b["lidar"].F.clone(), b["lidar"].C.int().contiguous()


def _logits(model, feats, coords):
    with torch.no_grad():
        return model({"lidar": SparseTensor(feats.clone(), coords)})["logits"].float()


def _count_calls(monkeypatch, be, names):
    counts = {n: 0 for n in names}
    for n in names:
        if not hasattr(be, n):
            continue
        orig = getattr(be, n)

        def wrapped(*a, _o=orig, _n=n, **kw):
            counts[_n] += 1
            return _o(*a, **kw)
        monkeypatch.setattr(be, n, wrapped, raising=False)
    return counts


def test_fold_whole_model_cpu(monkeypatch):
    """MinkUNet-18 (cr 0.5) on the ~2 000-point scan. Reference: the UNFROZEN model on the oracle backend (the C restatement of the
    reference, another summation order). The frozen model on a backend without the ReLU epilogue (the oracle) takes the torch
    add_ / relu_ fallback; its distance from the unfrozen run on the same backend is fold rounding alone, bounded the same way."""
    from oracle.adapter import OracleBackend
    model = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5).eval()
    seeded_state(model)
    feats, coords = _small_batch()
    monkeypatch.setattr(native, "_BACKEND", OracleBackend())
    assert not getattr(native.backend(), "conv_epilogue_relu", False)
    ref = _logits(model, feats, coords).numpy()
    assert openpcseg_amd.freeze(model) == {"folded": 49, "skipped": []}
    calls = _count_calls(monkeypatch, native.backend(), ["bn_apply"])
    frozen_oracle = _logits(model, feats, coords).numpy()
    assert calls["bn_apply"] == 0
    with cpu_fallback.enabled():
        frozen_cpu = _logits(model, feats, coords).numpy()
        openpcseg_amd.unfreeze(model)
        unfrozen_cpu = _logits(model, feats, coords).numpy()
    ef, eu, bound = _bound(frozen_cpu, unfrozen_cpu, ref)
    eo = float(np.abs(frozen_oracle - ref).max())
    print("whole model: frozen %.3e unfrozen %.3e frozen-on-oracle %.3e bound %.3e" % (ef, eu, eo, bound))
    assert ef <= bound, (ef, eu, bound)
    assert eo <= bound, (eo, eu, bound)


def test_freeze_is_opt_in_and_tracks_the_weights(cpu_be, monkeypatch):
    model = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5).eval()
    twin = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=0.5).eval()   # never frozen
    seeded_state(model)
    seeded_state(twin)
    feats, coords = _small_batch()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = [id(p) for p in model.parameters()]
    plain = _logits(model, feats, coords)
    assert openpcseg_amd.freeze(model) == {"folded": 49, "skipped": []}
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys()) and all(torch.equal(after[k], before[k]) for k in before)
    assert [id(p) for p in model.parameters()] == params

    calls = _count_calls(monkeypatch, cpu_be, ["bn_apply", "bn_stats"])
    frozen = _logits(model, feats, coords)
    assert calls["bn_apply"] == 0 and calls["bn_stats"] == 0
    assert float((frozen - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    # grad mode on: today's path, BatchNorm layers and all, bit for bit
    out = model({"lidar": SparseTensor(feats.clone(), coords)})["logits"]
    assert calls["bn_apply"] == 49 and torch.equal(out.detach(), plain)
    # train mode: today's path (batch statistics), no unfreeze needed
    calls["bn_apply"] = 0
    model.train()
    with torch.no_grad():
        model({"lidar": SparseTensor(feats.clone(), coords)})
    assert calls["bn_apply"] == 49
    model.load_state_dict(before)   # the training pass moved the running statistics
    model.eval()

    # re-fold after load_state_dict and after an in-place change of running_var
    folds = lambda: sum(f.folds for m in model.modules() for f in _records(m))
    n0 = folds()
    sd = {k: (v * 1.25 if k.endswith("kernel") else v) for k, v in before.items()}
    model.load_state_dict(sd)
    twin.load_state_dict(sd)
    a, b = _logits(model, feats, coords), _logits(twin, feats, coords)
    assert folds() == n0 + 49
    assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) and float((a - frozen).abs().max()) > 1e-3
    for m in (model, twin):
        m.stem[1].running_var.mul_(4.0)
    a2, b2 = _logits(model, feats, coords), _logits(twin, feats, coords)
    assert folds() == n0 + 50
    assert float((a2 - b2).abs().max()) <= 1e-4 * float(b2.abs().max()) and float((a2 - a).abs().max()) > 1e-3
    _logits(model, feats, coords)
    assert folds() == n0 + 50   # nothing changed: nothing folded

    calls["bn_apply"] = 0
    assert openpcseg_amd.unfreeze(model) > 0
    assert torch.equal(_logits(model, feats, coords), b2) and calls["bn_apply"] == 49


def _records(module):
    rec = module.__dict__.get("_pcs_folds") or {}
    for v in rec.values():
        for f in (v if isinstance(v, list) else [v]):
            if hasattr(f, "folds"):
                yield f


def _tiny_records():
    """One record of each class on 8 -> 16 channels, with the call that uses it."""
    from openpcseg_amd import inference, linear
    from openpcseg_amd import modules as spnn
    from openpcseg_amd.fused import FusedBatchNorm
    conv = lambda: spnn.Conv3d(8, 16, 3, bias=True)
    g = torch.Generator().manual_seed(1)
    xf, idx, wts = torch.randn(30, 8, generator=g), torch.randint(0, 30, (50, 8), generator=g).int(), torch.rand(50, 8, generator=g)
    folded = lambda rec: rec.folded()
    return [(inference.FoldedConv(conv(), FusedBatchNorm(16), True), folded),
            (inference.PostAffineConv(conv(), FusedBatchNorm(16), 0.01), folded),
            (inference.FoldedDense(torch.nn.Linear(8, 16), bn_in=FusedBatchNorm(8), bn_out=FusedBatchNorm(16)), folded),
            (inference.FoldedLinear(linear.FusedLinear(8, 16)), lambda rec: rec.devoxelized_part(0, xf, idx, wts, cache={}))]


def _fold_token(rec):
    """What changes exactly when the record folded: its counter, or for FoldedLinear (not counted) a mark in its `parts` memo."""
    return rec.folds if hasattr(rec, "folds") else rec.parts.setdefault("mark", object())


def test_one_currency_rule_for_every_record_class(cpu_be):
    """FoldedConv, PostAffineConv, FoldedDense, FoldedLinear, and every source tensor each of them names: an in-place change and a
    new storage re-fold exactly once at the next use; sources without a version counter fold on every use; a re-fold empties
    `prepared` (FoldedLinear: drops `parts`)."""
    seen = 0
    for rec, use in _tiny_records():
        sources = [t for t in rec._sources() if t is not None]
        assert len(sources) == {"FoldedConv": 6, "PostAffineConv": 6, "FoldedDense": 10, "FoldedLinear": 1}[type(rec).__name__]
        assert hasattr(rec, "folds") == (type(rec).__name__ != "FoldedLinear")
        use(rec)
        for t in sources:
            for change in ("in place", "storage"):
                before = _fold_token(rec)
                use(rec)
                assert _fold_token(rec) is before or _fold_token(rec) == before   # current: nothing folds
                if hasattr(rec, "prepared"):
                    rec.prepared["copy"] = "stale"
                if change == "in place":
                    with torch.no_grad():
                        t.mul_(1.5)
                else:
                    t.data = t.data.clone()
                use(rec)
                after = _fold_token(rec)
                assert (after == before + 1) if hasattr(rec, "folds") else (after is not before), (type(rec).__name__, change)
                assert getattr(rec, "prepared", {}) == {}
                use(rec)
                assert _fold_token(rec) is after or _fold_token(rec) == after   # and not again
                seen += 1
    assert seen == 2 * (6 + 6 + 10 + 1)
    with torch.inference_mode():
        made = _tiny_records()
    for rec, use in made:   # inference tensors track no version: every use folds
        tokens = []
        for _ in range(3):
            use(rec)
            tokens.append(_fold_token(rec))
        if hasattr(rec, "folds"):
            assert tokens == [1, 2, 3], type(rec).__name__
        else:
            assert tokens[0] is not tokens[1] and tokens[1] is not tokens[2]


def test_freeze_plain_sequential_and_unknown_modules(cpu_be):
    """A plain Sequential(Conv3d, BatchNorm, ReLU) folds (FusedBatchNorm or spnn.BatchNorm); a BatchNorm freeze cannot place
    is left alone and reported."""
    from openpcseg_amd import modules as spnn
    from openpcseg_amd.fused import FusedBatchNorm

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Sequential(spnn.Conv3d(8, 16, 3), spnn.BatchNorm(16), spnn.ReLU(True))
            self.b = torch.nn.Sequential(spnn.Conv3d(16, 16, 3, bias=True), FusedBatchNorm(16))
            self.odd = torch.nn.Sequential(spnn.Conv3d(16, 16, 3), spnn.LeakyReLU(0.1), spnn.BatchNorm(16))

        def forward(self, x):
            h = self.b(self.a(x))
            return self.odd(h)

    net = Net().eval()
    seeded_state(net)
    x = _scan_tensor(8)
    plain = _run(net, x).F
    assert openpcseg_amd.freeze(net) == {"folded": 2, "skipped": ["odd.2"]}
    frozen = _run(net, _scan_tensor(8)).F
    assert float((frozen - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    assert openpcseg_amd.unfreeze(net) == 2
    assert torch.equal(_run(net, _scan_tensor(8)).F, plain)


def test_cpu_backend_conv_write_back_order(cpu_be):
    """cpu_fallback.conv_gather_gemm: bias, then addend, then the activation, like pcs_conv_epilogue."""
    x = _scan_tensor(8)
    entry = F.build_kernel_map(x.C, x.C, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    g = torch.Generator().manual_seed(3)
    w, bias, add = torch.randn(27, 8, 12, generator=g) * 0.1, torch.randn(12, generator=g), torch.randn(x.C.shape[0], 12, generator=g)
    base = cpu_be.conv_gather_gemm(x.F, w, entry.fwd)
    assert torch.equal(cpu_be.conv_gather_gemm(x.F, w, entry.fwd, bias=bias, addend=add, relu=True), torch.relu(base + bias + add))
    leaky = cpu_be.conv_gather_gemm(x.F, w, entry.fwd, addend=add, act_slope=0.1)
    assert torch.equal(leaky, torch.where(base + add < 0, (base + add) * 0.1, base + add))
    assert torch.equal(cpu_be.conv_gather_gemm(x.F, w, entry.fwd, act_slope=0.0), base)   # 0 and 1 = no activation


# =====================================================================================================================
# GPU
# =====================================================================================================================
def _dense():
    import test_dense_parity as dp
    return dp


@pytest.fixture(scope="module")
def levels():
    return _dense().scan_levels([0, 1])


_ORACLE = {}


def _oracle_conv(key, x, w, nbmaps, nbsizes, sizes, transposed=False):
    from oracle import oracle as orc
    if key not in _ORACLE:
        _ORACLE.clear()   # one entry: the cases of a shape run back to back
        _ORACLE[key] = orc.conv_fwd(x, w, nbmaps, nbsizes, sizes, transposed=transposed).astype(np.float64)
    return _ORACLE[key]


def _check_layer(y, ref, dtype, relu):
    dp = _dense()
    if dtype is None:
        assert y.dtype == torch.float32
        dp.close(y, ref, 2e-5)
    else:
        assert y.dtype == dtype
        dp.close_half(y, ref, dtype)
    if relu:
        assert float(y.float().min()) >= 0.0   # -0.0 compares equal to 0


def _operands(rng, n_in, n_out, k, cin, cout, dtype):
    dp = _dense()
    x = rng.normal(size=(n_in, cin)).astype(np.float32)
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(cin * k) * rng.uniform(0.5, 1.5, size=cout)).astype(np.float32)   # W * s
    b = rng.normal(size=cout).astype(np.float32) * 0.3
    add = rng.normal(size=(n_out, cout)).astype(np.float32)
    if dtype is not None:
        x, w, add = dp._round_half(x, dtype), dp._round_half(w, dtype), dp._round_half(add, dtype)
    return x, w, b, add


LAYER_CASES = [(1, 96, 96), (1, 4, 32), (2, 64, 64), (4, 128, 128), (8, 256, 256), (8, 384, 256), (2, 112, 112)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [None, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("stride,cin,cout", LAYER_CASES)
def test_layer_one_launch_dense_map(hip, levels, monkeypatch, stride, cin, cout, dtype):
    """conv + b' + addend + ReLU through functional.conv3d_inference on the BASELINE-density maps: ONE backend call, against the
    oracle's conv_fwd on W' followed by the same steps in float64 (half: on half-rounded x, W', addend). 4 -> 32 (the stem)
    runs on the fp32 kernel also under autocast and is rounded afterwards."""
    dp = _dense()
    entry, nbmaps, nbsizes, n = dp.level_map(levels, stride)
    rng = np.random.default_rng(stride * 100000 + cin * 100 + cout + 11)
    x, w, b, add = _operands(rng, n, n, 27, cin, cout, dtype)
    conv = _oracle_conv((stride, cin, cout, dtype), x, w, nbmaps, nbsizes, (n, n))
    calls = _count_calls(monkeypatch, native.backend(), ["conv_gather_gemm", "conv_gather_gemm_h", "bn_apply"])
    dx, dw, db, dadd = dp.t(x), dp.t(w), dp.t(b), dp.t(add)
    for addend in (None, dadd):
        for relu in (True, False):
            xs = SparseTensor(dx if dtype is None else dx.to(dtype), dp.t(levels[stride]), stride)
            xs.kmaps[((stride,) * 3, (3, 3, 3), (1, 1, 1), (1, 1, 1))] = entry
            before = dict(calls)
            with torch.no_grad(), torch.autocast("cuda", dtype=dtype or torch.bfloat16, enabled=dtype is not None):
                y = F.conv3d_inference(xs, dw, db, 3, addend=addend if addend is None or dtype is None else addend.to(dtype), relu=relu)
            assert sum(calls.values()) - sum(before.values()) == 1 and calls["bn_apply"] == 0
            half = dtype is not None and native.backend().conv_h_applies(cin, cout, 27)
            assert calls["conv_gather_gemm_h"] - before["conv_gather_gemm_h"] == (1 if half else 0)
            ref = conv + b[None, :].astype(np.float64) + (add.astype(np.float64) if addend is not None else 0.0)
            _check_layer(y.F, np.maximum(ref, 0.0) if relu else ref, dtype, relu)
            if relu:
                assert float((y.F == 0).float().mean()) > 0.2   # the activation did cut


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [None, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_layer_strided_transposed_pointwise(hip, levels, dtype):
    """K = 8 strided (stride 4 -> 8, 128 -> 128) and transposed (256 -> 128) convolutions and K = 1 over the identity map
    (64 -> 128, the residual blocks' downsample), with and without addend, ReLU on."""
    from oracle import oracle as orc
    dp = _dense()
    c4, c8 = levels[4], levels[8]
    n_in, n_out = c4.shape[0], c8.shape[0]
    nbmaps, nbsizes = orc.build_kmap(c4, c8, 2, 4)
    rng = np.random.default_rng(77)
    ctx = lambda: torch.autocast("cuda", dtype=dtype or torch.bfloat16, enabled=dtype is not None)
    cast = lambda a: dp.t(a) if dtype is None else dp.t(a).to(dtype)
    # strided
    x, w, b, add = _operands(rng, n_in, n_out, 8, 128, 128, dtype)
    xs = SparseTensor(cast(x), dp.t(c4), 4)
    xs.cmaps[(4, 4, 4)], xs.cmaps[(8, 8, 8)] = xs.C, dp.t(c8)
    conv = orc.conv_fwd(x, w, nbmaps, nbsizes, (n_in, n_out)).astype(np.float64)
    down = None
    for addend in (None, add):
        with torch.no_grad(), ctx():
            down = F.conv3d_inference(xs, dp.t(w), dp.t(b), 2, stride=2, addend=None if addend is None else cast(addend), relu=True)
        assert down.stride == (8, 8, 8) and np.array_equal(down.C.cpu().numpy(), c8)
        _check_layer(down.F, np.maximum(conv + b + (0.0 if addend is None else addend), 0.0), dtype, True)
    # transposed, on the maps the strided convolution left in the shared cache
    xu, wu, bu, addu = _operands(rng, n_out, n_in, 8, 256, 128, dtype)
    conv = orc.conv_fwd(xu, wu, nbmaps, nbsizes, (n_in, n_out), transposed=True).astype(np.float64)
    for addend in (None, addu):
        with torch.no_grad(), ctx():
            up = F.conv3d_inference(down._like(cast(xu)), dp.t(wu), dp.t(bu), 2, stride=2, transposed=True,
                                    addend=None if addend is None else cast(addend), relu=True)
        assert up.stride == (4, 4, 4) and up.F.shape == (n_in, 128)
        _check_layer(up.F, np.maximum(conv + bu + (0.0 if addend is None else addend), 0.0), dtype, True)
    # K = 1: the downsample branch (no ReLU) and with addend + ReLU
    x1, w1, b1, add1 = _operands(rng, n_in, n_in, 1, 64, 128, dtype)
    ref = x1.astype(np.float64) @ w1[0].astype(np.float64) + b1
    for addend, relu in ((None, False), (add1, True)):
        with torch.no_grad(), ctx():
            y = F.conv3d_inference(SparseTensor(cast(x1), dp.t(c4), 4), dp.t(w1[0]), dp.t(b1), 1,
                                   addend=None if addend is None else cast(addend), relu=relu)
        r = ref + (0.0 if addend is None else addend)
        _check_layer(y.F, np.maximum(r, 0.0) if relu else r, dtype, relu)


@pytest.mark.gpu
def test_epilogue_flags_abi(hip, levels):
    """PCS_EP_RELU clear + act_slope = 0 still means no activation; an unknown flag bit is PCS_EINVAL (both entries)."""
    import ctypes
    dp = _dense()
    entry, _, _, n = dp.level_map(levels, 8)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(n, 64, device="cuda", generator=g)
    w = torch.randn(27, 64, 64, device="cuda", generator=g) / np.sqrt(64 * 27)
    plain = hip.conv_gather_gemm(x, w, entry.fwd)
    assert torch.equal(hip.conv_gather_gemm(x, w, entry.fwd, act_slope=0.0), plain) and float(plain.min()) < 0
    assert torch.equal(hip.conv_gather_gemm(x, w, entry.fwd, relu=True), torch.relu(plain))
    assert torch.equal(hip.conv_gather_gemm(x, w, entry.fwd, relu=True, act_slope=0.1), torch.relu(plain))   # the flag wins
    km = entry.fwd
    t = hip.tile_rows(64, 64, km)
    seg = hip._segments(km, t)
    dst = torch.empty_like(plain)
    for flags, want in ((native.HipBackend.EP_RELU, 0), (native.HipBackend.EP_RELU | 2, -1), (4, -1)):
        ep = hip._Epilogue(None, 0.0, flags)
        rc = hip.lib.pcs_conv_gather_gemm_f32_ex(native._ptr(x), n, 64, native._ptr(w), 27, 64, native._ptr(km._pairs_raw), 0,
                                                 native._ptr(seg), t, km.n_dst, None, ctypes.byref(ep), native._ptr(dst), None, None,
                                                 native._stream())
        assert rc == want, (flags, rc)
    xh = x.to(torch.bfloat16)
    wp = hip.prepare_weights_h(w, torch.bfloat16, transpose=False)
    th = hip.tile_rows(64, 64, km, 1)
    segh = hip._segments(km, th)
    dsth = torch.empty((n, 64), dtype=torch.bfloat16, device="cuda")
    for flags, want in ((native.HipBackend.EP_RELU, 0), (native.HipBackend.EP_RELU | 8, -1)):
        ep = hip._Epilogue(None, 0.0, flags)
        rc = hip.lib.pcs_conv_gather_gemm_h_ex(native._ptr(xh), n, 64, native._ptr(wp), 27, 64, native._ptr(km._pairs_raw), 0,
                                               native._ptr(segh), th, km.n_dst, None, ctypes.byref(ep), native._ptr(dsth), 1, None, None,
                                               native._stream())
        assert rc == want, (flags, rc)
    torch.cuda.synchronize()
    assert float(dsth.float().min()) >= 0.0


# ---- model level ------------------------------------------------------------------------------------------------------
def _device_batch(frames):
    b = sparse_collate_fn(frames)
    return b["lidar"].F.cuda(), b["lidar"].C.int().cuda().contiguous()


def _scans(kind):
    if kind == "one":
        return [voxelize_scan(make_scan(0, 20000), seed=0)]
    return [voxelize_scan(make_scan(s, n), seed=s) for s, n in ((1, 12000), (2, 20000), (3, 16000))]


def _record_parity(key, value):
    data = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as f:
            data = json.load(f)
    data[key] = value
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    with open(PARITY_JSON, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)


def _public_methods(be):
    return [n for n in dir(be) if not n.startswith("_") and callable(getattr(be, n)) and not isinstance(getattr(type(be), n, None), type)]


@pytest.mark.gpu
@pytest.mark.parametrize("scans", ["one", "three"])
@pytest.mark.parametrize("layers,pairs", [(mk.MK18_LAYERS, 49), (mk.MK34_LAYERS, 63)], ids=["mk18", "mk34"])
def test_frozen_model_makes_no_batchnorm_call(hip, monkeypatch, layers, pairs, scans):
    """(a) zero bn_apply / bn_stats / _FusedBN calls, fewer backend calls in total, no weight preparation after the first frozen
    forward (fp32 and bf16 autocast); (d) two frozen forwards are bit-identical."""
    from openpcseg_amd import fused
    model = mk.MinkUNet(num_class=20, num_layer=layers, cr=1.0).cuda().eval()
    seeded_state(model)
    feats, coords = _device_batch(_scans(scans))
    be = native.backend()
    counts = _count_calls(monkeypatch, be, _public_methods(be))
    fbn = {"n": 0}
    orig_apply = fused._FusedBN.apply
    monkeypatch.setattr(fused._FusedBN, "apply", staticmethod(lambda *a, **k: (fbn.__setitem__("n", fbn["n"] + 1), orig_apply(*a, **k))[1]))

    def run(amp):
        for k in counts:
            counts[k] = 0
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            y = _logits(model, feats, coords)
        return y, dict(counts)

    for amp in (False, True):
        openpcseg_amd.unfreeze(model)
        _, plain = run(amp)
        assert plain["bn_apply"] == pairs
        assert openpcseg_amd.freeze(model) == {"folded": pairs, "skipped": []}
        y1, first = run(amp)
        y2, second = run(amp)
        for c in (first, second):
            assert c["bn_apply"] == 0 and c["bn_stats"] == 0 and c.get("bn_finalize", 0) == 0 and fbn["n"] == 0
        assert sum(second.values()) < sum(plain.values()), (sum(second.values()), sum(plain.values()))
        assert second["prepare_weights_h"] == 0 and second["weights_multi"] == 0 and second["transpose_weights"] == 0
        if amp:
            assert first["prepare_weights_h"] > 0 and second["conv_gather_gemm_h"] > 0
        assert torch.equal(y1, y2)
        print("backend calls (amp=%s): unfrozen %d, frozen %d" % (amp, sum(plain.values()), sum(second.values())))


@pytest.mark.gpu
def test_frozen_model_fp32_error_vs_oracle_backend(hip, monkeypatch):
    """(b) MinkUNet-18, one 20 000-point scan: reference = the unfrozen model on the oracle backend with host tensors;
    max|frozen_hip - ref| <= 2 * max|unfrozen_hip - ref| + 2e-5 * max|ref|."""
    from oracle.adapter import OracleBackend
    model = mk.MinkUNet(num_class=20, num_layer=mk.MK18_LAYERS, cr=1.0).eval()
    seeded_state(model)
    frames = _scans("one")
    b = sparse_collate_fn(frames)
    hf, hc = b["lidar"].F.clone(), b["lidar"].C.int().contiguous()
    with monkeypatch.context() as mp:
        mp.setattr(native, "_BACKEND", OracleBackend())
        ref = _logits(model, hf, hc).numpy()
    model.cuda()
    feats, coords = hf.cuda(), hc.cuda()
    unfrozen = _logits(model, feats, coords).cpu().numpy()
    openpcseg_amd.freeze(model)
    frozen = _logits(model, feats, coords).cpu().numpy()
    ef, eu, bound = _bound(frozen, unfrozen, ref)
    _record_parity("mk18_fp32_vs_oracle_backend", {"max_err_frozen": ef, "max_err_unfrozen": eu, "max_abs_ref": float(np.abs(ref).max()),
                                                   "bound": bound, "points": int(ref.shape[0])})
    print("fp32 model: frozen %.3e unfrozen %.3e bound %.3e" % (ef, eu, bound))
    assert ef <= bound, (ef, eu, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("layers", [mk.MK18_LAYERS, mk.MK34_LAYERS], ids=["mk18", "mk34"])
def test_frozen_model_autocast_error(hip, layers, dtype):
    """(c) errors of the frozen and the unfrozen half runs against the unfrozen fp32 HIP logits, over the logit RMS:
    frozen <= 1.5 * unfrozen for the mean, 2 * for the max. Arg-max agreement is recorded, not asserted."""
    model = mk.MinkUNet(num_class=20, num_layer=layers, cr=1.0).cuda().eval()
    seeded_state(model)
    feats, coords = _device_batch(_scans("three"))
    ref = _logits(model, feats, coords).double()
    rms = float(ref.pow(2).mean().sqrt())
    out = {}
    for name in ("unfrozen", "frozen"):
        if name == "frozen":
            openpcseg_amd.freeze(model)
        with torch.autocast("cuda", dtype=dtype):
            y = _logits(model, feats, coords).double()
        err = (y - ref).abs()
        out[name] = {"max_err_over_rms": float(err.max()) / rms, "mean_err_over_rms": float(err.mean()) / rms,
                     "argmax_agreement": float((y.argmax(1) == ref.argmax(1)).double().mean())}
    out["logit_rms"] = rms
    _record_parity("mk%d_%s_vs_fp32_hip" % (18 if layers is mk.MK18_LAYERS else 34, str(dtype).split(".")[1]), out)
    print(out)
    assert out["frozen"]["mean_err_over_rms"] <= 1.5 * out["unfrozen"]["mean_err_over_rms"], out
    assert out["frozen"]["max_err_over_rms"] <= 2.0 * out["unfrozen"]["max_err_over_rms"], out
