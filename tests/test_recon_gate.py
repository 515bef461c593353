"""The ReconBlock (DDCM) gate of Cylinder3D (csrc/recongate.hip, fused.recon_gate;
R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:337-384) through the C ABI, against tests/recon_reference.py (float64).

Bounds (stated before any kernel ran; y64 = the float64 formula from the inputs as stored):

    forward, fp32     |out - out64| <= 2e-5 max |out64|: the project's fp32 kernel bound. On the data of these tests the roundings on
                      the path are far inside it: bn_k(a) = fma(a, sc, sh) carries at most 10 u (|a sc| + |mean sc| + |beta|) (the
                      apply bound of tests/bn_reference.py, u = 2^-24; |mean sc| <= 75 here, so < 1e-4 absolute), a sigmoid has
                      slope <= 1/4, expf / the sum 1 + e / the division a few u each, two additions and the product a few u more.
    forward, 16 bits  that plus half an ulp of the storage format at out64 (the one rounding of the store): the exact half ulp
                      2^(floor(log2 |y|) - p - 1), p = 7 (bf16) / 10 (fp16), floored at the smallest normal exponent
    backward apply    the same two bounds on dx_gate and on every da_k, each relative to its own tensor's maximum; the float64
                      sums are handed to the kernel, so the bound is that of the apply pass alone
    backward stats    the relative bound tests/bn_reference.py derives for pcs_bn_bwd_stats_*, with g_k in place of dy * gate:
                          |S_k0 - S_k0_64| <= (L + 6) u sum |g_k|,   |S_k1 - S_k1_64| <= (L + 6) u sum |g_k| (|a_k| + |mean_k|) invstd_k
                      L = ceil(n / 1024) + 256: recon_gate_partial_kernel runs 1024 workgroups of TY <= 256 row lanes, a lane adds
                      ceil(n / (1024 TY)) terms in fp32, the workgroup adds its TY lane sums in fp32, everything after that is
                      double -- the chain of bn_partial_kernel. xhat carries the same 4 roundings and the product 1. g_k itself
                      is computed here (dy * x, the sigmoid, s (1 - s): about 8 roundings and the BatchNorm term's error through
                      a slope <= 0.1), where the BatchNorm pass reads it exactly; that is not allowed for separately: it is
                      charged to the 256 of L, which no single chain of these shapes comes near (TY = 64 at c = 16, 16 at c = 64).
    exact data        equality. mean, invstd, gamma powers of two, beta 0, every a_k element either mean (bn = 0, gate exactly
                      0.5) or mean + 32 / (invstd gamma) (bn = 32, expf(-32) < 2^-25, gate exactly 1.0 in fp32), x small integers:
                      out = x * {1.5, 2, 2.5, 3} with no rounding anywhere, in all three storage types.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_reference as BR
import recon_reference as R
from openpcseg_amd import build as pcs_build
from openpcseg_amd import cpu_fallback, fused, native
from openpcseg_amd.fused import FusedBatchNorm

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
FMT = {"bf16": (7, -126), "fp16": (10, -14)}   # mantissa bits, smallest normal exponent
ENTRIES = ["pcs_recon_gate_f32", "pcs_recon_gate_h", "pcs_recon_gate_bwd_stats_f32", "pcs_recon_gate_bwd_stats_h",
           "pcs_recon_gate_bwd_apply_f32", "pcs_recon_gate_bwd_apply_h"]


def half_ulp(y, name):
    """Half an ulp of the storage format at y (0 for fp32: the fp32 bound holds its store)."""
    if name == "fp32":
        return np.zeros_like(y)
    p, emin = FMT[name]
    a = np.abs(y)
    e = np.full(a.shape, float(emin))
    nz = a > 0
    e[nz] = np.maximum(np.floor(np.log2(a[nz])), emin)
    return 0.5 * 2.0 ** (e - p)


def stored(a, name):
    """-> (host tensor in the storage type, the stored values in float64)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[name])
    return t, t.float().numpy().astype(np.float64)


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(got, ref64, name, what):
    bound = 2e-5 * float(np.abs(ref64).max()) + half_ulp(ref64, name)
    err = np.abs(host(got) - ref64)
    print("[recon gate] %-28s %s: worst error / bound = %.4f" % (what, name, float((err / bound).max())))
    assert (err <= bound).all(), (what, name, float((err / bound).max()))


# ---- cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_case(n, c, name):
    """Unit-scale data, the mean of a channel up to 50 standard deviations off zero; distinct statistics, gamma and beta per branch.
    -> dict of float64 arrays of the values AS STORED in the storage type + the host tensors."""
    rng = np.random.default_rng(1000 * n + c)
    q = {"t": {}}
    std = rng.uniform(0.5, 1.5, size=(3, c))
    mean = rng.uniform(-50.0, 50.0, size=(3, c)) * std
    for k in range(3):
        q["t"]["a%d" % k], q["a%d" % k] = stored(mean[k] + std[k] * rng.normal(size=(n, c)), name)
    q["t"]["x"], q["x"] = stored(rng.normal(size=(n, c)), name)
    q["t"]["dy"], q["dy"] = stored(rng.normal(size=(n, c)), name)
    q["stat3"] = np.concatenate([np.concatenate([mean[k], 1.0 / std[k]]) for k in range(3)])
    q["gamma3"] = rng.uniform(0.5, 1.5, size=3 * c).astype(np.float32)
    q["beta3"] = rng.uniform(-0.5, 0.5, size=3 * c).astype(np.float32)
    q["a3"] = [q["a0"], q["a1"], q["a2"]]
    return q


def exact_case(n, c, name):
    """The exact data of the module docstring -> (a3, x tensors in the storage type, stat3, gamma3, expected out in float64)."""
    ch = np.arange(c)
    a3, stat3, gamma3 = [], [], []
    for k in range(3):
        mean = np.where((ch + k) % 2 == 0, 1.0, -1.0) * 2.0 ** ((ch + k) % 3)
        invstd = 2.0 ** (((ch + 2 * k) % 3) - 1)
        gamma = 2.0 ** (1 - ((ch + k) % 3))
        hot = ((ch % 8) >> k) & 1                          # bit k of channel % 8: this branch's gate is 1.0, else 0.5
        row = mean + hot * 32.0 / (invstd * gamma)
        BR.assert_representable(row, name, "a%d" % k)
        a3.append(stored(np.broadcast_to(row, (n, c)), name)[0])
        stat3 += [mean, invstd]
        gamma3.append(gamma)
    rng = np.random.default_rng(n + c)
    x = rng.integers(-6, 7, size=(n, c)).astype(np.float64)
    pop = sum(((ch % 8) >> k) & 1 for k in range(3))
    want = x * (1.5 + 0.5 * pop)
    BR.assert_representable(want, name, "out")
    return a3, stored(x, name)[0], np.concatenate(stat3), np.concatenate(gamma3).astype(np.float32), want


# ---- raw entries ----------------------------------------------------------------------------------------------------------
def raw_forward(hip, name, a3, x, stat3, gamma3, beta3, n, c, out, dtype=None):
    p = native._ptr
    args = [p(a3[0]), p(a3[1]), p(a3[2]), p(x), p(stat3), p(gamma3), p(beta3), n, c]
    if name == "fp32":
        return hip.lib.pcs_recon_gate_f32(*args, p(out), native._stream())
    return hip.lib.pcs_recon_gate_h(*args, CODE[name] if dtype is None else dtype, p(out), native._stream())


def raw_bwd_stats(hip, name, dy, x, a3, stat3, gamma3, beta3, n, c, ws, sums2, doubles):
    p = native._ptr
    args = [p(dy), p(x), p(a3[0]), p(a3[1]), p(a3[2]), p(stat3), p(gamma3), p(beta3), n, c]
    tail = [p(ws), p(sums2), doubles, native._stream()]
    if name == "fp32":
        return hip.lib.pcs_recon_gate_bwd_stats_f32(*args, *tail)
    return hip.lib.pcs_recon_gate_bwd_stats_h(*args, CODE[name], *tail)


def raw_bwd_apply(hip, name, dy, x, a3, stat3, gamma3, beta3, sums2, count, n, c, dx, da):
    p = native._ptr
    args = [p(dy), p(x), p(a3[0]), p(a3[1]), p(a3[2]), p(stat3), p(gamma3), p(beta3), p(sums2), float(count), None, n, c]
    tail = [p(dx), p(da[0]), p(da[1]), p(da[2]), native._stream()]
    if name == "fp32":
        return hip.lib.pcs_recon_gate_bwd_apply_f32(*args, *tail)
    return hip.lib.pcs_recon_gate_bwd_apply_h(*args, CODE[name], *tail)


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_gate_entries():
    lib = ctypes.CDLL(pcs_build.LIB_PATH)
    assert all(hasattr(lib, e) for e in ENTRIES) and all(e in native.SIGNATURES for e in ENTRIES)
    lib.pcs_abi_version.restype = ctypes.c_int32
    assert lib.pcs_abi_version() == 12 == native.ABI_VERSION


@pytest.mark.parametrize("n,c", [(2, 4), (37, 8), (500, 16)])
def test_reference_equals_torch_autograd_in_float64(n, c):
    """The float64 reference of the three formulas against autograd over batch_norm, sigmoid, add and mul in float64."""
    rng = np.random.default_rng(n + c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    a3 = [t(3.0 * (k + 1) + (0.5 + k) * rng.normal(size=(n, c))).requires_grad_() for k in range(3)]
    x, dy = t(rng.normal(size=(n, c))).requires_grad_(), t(rng.normal(size=(n, c)))
    w3 = [t(rng.uniform(0.5, 1.5, size=c)).requires_grad_() for _ in range(3)]
    b3 = [t(rng.uniform(-0.5, 0.5, size=c)).requires_grad_() for _ in range(3)]
    eps = 1e-5
    gates = [torch.sigmoid(torch.nn.functional.batch_norm(a, None, None, w, b, True, 0.0, eps)) for a, w, b in zip(a3, w3, b3)]
    out = ((gates[0] + gates[1]) + gates[2]) * x
    out.backward(dy)
    an = [a.detach().numpy() for a in a3]
    stat3 = np.concatenate([np.concatenate([a.mean(0), 1.0 / np.sqrt(a.var(0) + eps)]) for a in an])
    g3, be3 = np.concatenate([w.detach().numpy() for w in w3]), np.concatenate([b.detach().numpy() for b in b3])
    xn, dyn = x.detach().numpy(), dy.numpy()
    close = lambda got, ref: np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(ref).max())))
    close(R.forward(an, xn, stat3, g3, be3), out.detach().numpy())
    s2 = R.bwd_stats(dyn, xn, an, stat3, g3, be3)
    dx, da = R.bwd_apply(dyn, xn, an, stat3, g3, be3, s2, n)
    close(dx, x.grad.numpy())
    for k in range(3):
        close(da[k], a3[k].grad.numpy())
        close(s2[(2 * k + 1) * c:(2 * k + 2) * c], w3[k].grad.numpy())
        close(s2[2 * k * c:(2 * k + 1) * c], b3[k].grad.numpy())


def test_cpu_fallback_methods_against_float64():
    n, c = 300, 12
    q = real_case(n, c, "fp32")
    be = cpu_fallback.TorchCpuBackend()
    t = q["t"]
    a3 = [t["a0"], t["a1"], t["a2"]]
    stat3, g3, b3 = torch.from_numpy(q["stat3"]), torch.from_numpy(q["gamma3"]), torch.from_numpy(q["beta3"])
    within(be.recon_gate(a3, t["x"], stat3, g3, b3), R.forward(q["a3"], q["x"], q["stat3"], q["gamma3"], q["beta3"]), "fp32", "cpu forward")
    s64 = R.bwd_stats(q["dy"], q["x"], q["a3"], q["stat3"], q["gamma3"], q["beta3"])
    s2 = be.recon_gate_bwd_stats(t["dy"], t["x"], a3, stat3, g3, b3)
    assert s2.dtype == torch.float64 and s2.shape == (6 * c,)
    assert np.abs(s2.numpy() - s64).max() <= 1e-4 * np.abs(s64).max()
    dx, da = be.recon_gate_bwd_apply(t["dy"], t["x"], a3, stat3, g3, b3, torch.from_numpy(s64), n)
    dx64, da64 = R.bwd_apply(q["dy"], q["x"], q["a3"], q["stat3"], q["gamma3"], q["beta3"], s64, n)
    within(dx, dx64, "fp32", "cpu dx_gate")
    for k in range(3):
        within(da[k], da64[k], "fp32", "cpu da%d" % k)


def _seeded_bns(c, sync=False):
    bns = [FusedBatchNorm(c, sync=sync) for _ in range(3)]
    rng = np.random.default_rng(c)
    with torch.no_grad():
        for bn in bns:
            bn.weight.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, size=c).astype(np.float32)))
            bn.bias.copy_(torch.from_numpy(rng.uniform(-0.5, 0.5, size=c).astype(np.float32)))
            bn.running_mean.copy_(torch.from_numpy(rng.normal(size=c).astype(np.float32)))
            bn.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, size=c).astype(np.float32)))
    return bns


def _autograd_run(device, switch, monkeypatch, n=1000, c=16):
    monkeypatch.setenv("PCS_RECON_GATE", switch)
    q = real_case(n, c, "fp32")
    bns = [bn.to(device).train() for bn in _seeded_bns(c)]
    leaves = [q["t"][k].to(device).clone().requires_grad_() for k in ("x", "a0", "a1", "a2")]
    out = fused.recon_gate(bns, leaves[1:], leaves[0])
    out.backward(q["t"]["dy"].to(device))
    res = {"out": out.detach(), "dx": leaves[0].grad, "da0": leaves[1].grad, "da1": leaves[2].grad, "da2": leaves[3].grad}
    for k, bn in enumerate(bns):
        res.update({"dw%d" % k: bn.weight.grad, "db%d" % k: bn.bias.grad})
    run = {"rm%d" % k: bn.running_mean.clone() for k, bn in enumerate(bns)}
    run.update({"rv%d" % k: bn.running_var.clone() for k, bn in enumerate(bns)})
    assert all(int(bn.num_batches_tracked) == 1 for bn in bns)
    for bn in bns:
        bn.eval()
    with torch.no_grad():
        res["eval"] = fused.recon_gate(bns, leaves[1:], leaves[0])
    return {k: v.cpu() for k, v in res.items()}, {k: v.cpu() for k, v in run.items()}, bns


def _autograd_compare(device, monkeypatch, be):
    calls = []
    for name in ("recon_gate", "recon_gate_bwd_stats", "recon_gate_bwd_apply"):
        orig = getattr(be, name)
        monkeypatch.setattr(be, name, (lambda o, k: lambda *a, **kw: (calls.append(k), o(*a, **kw))[1])(orig, name))
    f, frun, bns = _autograd_run(device, "1", monkeypatch)
    assert calls == ["recon_gate", "recon_gate_bwd_stats", "recon_gate_bwd_apply", "recon_gate"]
    del calls[:]
    l, lrun, _ = _autograd_run(device, "0", monkeypatch)
    assert calls == []
    for k in f:
        scale = float(l[k].abs().max())
        assert float((f[k] - l[k]).abs().max()) <= 1e-5 * scale, (k, float((f[k] - l[k]).abs().max()) / scale)
    for k in frun:
        assert torch.allclose(frun[k], lrun[k], rtol=1e-6, atol=0.0), k
    # eval mode reads the running statistics: the float64 formula on them
    q = real_case(1000, 16, "fp32")
    stat3 = np.concatenate([np.concatenate([host(bn.running_mean), 1.0 / np.sqrt(host(bn.running_var) + bn.eps)]) for bn in bns])
    g3, b3 = np.concatenate([host(bn.weight) for bn in bns]), np.concatenate([host(bn.bias) for bn in bns])
    within(f["eval"], R.forward(q["a3"], q["x"], stat3, g3, b3), "fp32", "eval mode")


def test_autograd_against_the_literal_sequence_on_the_cpu_backend(monkeypatch):
    with cpu_fallback.enabled() as be:
        _autograd_compare("cpu", monkeypatch, be)


def test_empty_input_is_a_no_op_without_a_device():
    """n == 0 returns PCS_OK before any pointer is looked at: every entry, with NULL everywhere, on a host without a GPU."""
    lib = native.load_library()
    z = [None] * 8
    assert lib.pcs_recon_gate_f32(*z[:7], 0, 16, None, None) == 0
    assert lib.pcs_recon_gate_h(*z[:7], 0, 16, 1, None, None) == 0
    assert lib.pcs_recon_gate_bwd_stats_f32(*z, 0, 16, None, None, 0, None) == 0
    assert lib.pcs_recon_gate_bwd_stats_h(*z, 0, 16, 2, None, None, 0, None) == 0
    assert lib.pcs_recon_gate_bwd_apply_f32(*z, None, 0.0, None, 0, 16, None, None, None, None, None) == 0
    assert lib.pcs_recon_gate_bwd_apply_h(*z, None, 0.0, None, 0, 16, 1, None, None, None, None, None) == 0
    assert lib.pcs_recon_gate_h(*z[:7], 0, 16, 3, None, None) == -1          # the dtype is looked at first


# ---- GPU: exact data ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [(d, c) for d in DT for c in (8, 16, 64, 96, 256)] + [("fp32", 4), ("fp32", 12)])
def test_exact_data(hip, name, c):
    for n in (1, 63, 257, 4099):
        a3, x, stat3, gamma3, want = exact_case(n, c, name)
        out = hip.recon_gate([dev(a) for a in a3], dev(x), dev(stat3), dev(gamma3), None)
        assert out.dtype == DT[name] and np.array_equal(host(out), want), (name, n, c)


# ---- GPU: random data -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DT))
@pytest.mark.parametrize("n,c", [(20011, 16), (257, 64)])
def test_real_data_against_float64(hip, n, c, name):
    """Forward, backward statistics (twice: bit-identical) and backward apply; the three branches carry distinct statistics, gamma
    and beta and every da_k is checked on its own, so a mixed-up branch cannot pass."""
    q = real_case(n, c, name)
    a3 = [dev(q["t"]["a%d" % k]) for k in range(3)]
    x, dy = dev(q["t"]["x"]), dev(q["t"]["dy"])
    stat3, g3, b3 = dev(q["stat3"]), dev(q["gamma3"]), dev(q["beta3"])
    ref = (q["a3"], q["stat3"], q["gamma3"], q["beta3"])
    tag = "n=%d c=%d" % (n, c)
    within(hip.recon_gate(a3, x, stat3, g3, b3), R.forward(ref[0], q["x"], *ref[1:]), name, "forward " + tag)
    s64 = R.bwd_stats(q["dy"], q["x"], *ref)
    s2 = hip.recon_gate_bwd_stats(dy, x, a3, stat3, g3, b3)
    again = hip.recon_gate_bwd_stats(dy, x, a3, stat3, g3, b3)
    assert torch.equal(s2, again) and torch.equal(s2._pcs_f32, again._pcs_f32)
    assert torch.equal(s2._pcs_f32, s2.float())
    g64 = R.grads_of_gates(q["dy"], q["x"], *ref)
    got = s2.cpu().numpy()
    for k in range(3):
        b0, b1 = BR.bwd_stats_bound(g64[k], q["a3"][k], q["stat3"][2 * k * c:(2 * k + 2) * c])
        e0 = np.abs(got[2 * k * c:(2 * k + 1) * c] - s64[2 * k * c:(2 * k + 1) * c])
        e1 = np.abs(got[(2 * k + 1) * c:(2 * k + 2) * c] - s64[(2 * k + 1) * c:(2 * k + 2) * c])
        print("[recon gate] bwd stats %s %s branch %d: worst error / bound = %.4f, %.4f" % (tag, name, k, (e0 / b0).max(), (e1 / b1).max()))
        assert (e0 <= b0).all() and (e1 <= b1).all(), (k, float((e0 / b0).max()), float((e1 / b1).max()))
    dx, da = hip.recon_gate_bwd_apply(dy, x, a3, stat3, g3, b3, dev(s64), n)
    dx64, da64 = R.bwd_apply(q["dy"], q["x"], *ref, s64, n)
    within(dx, dx64, name, "dx_gate " + tag)
    for k in range(3):
        within(da[k], da64[k], name, "da%d %s" % (k, tag))


@pytest.mark.gpu
def test_autograd_against_the_literal_sequence(hip, monkeypatch):
    _autograd_compare("cuda", monkeypatch, native.backend())


# ---- GPU: contract --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,c", [("fp32", 6), ("bf16", 12)])
def test_unsupported_widths(hip, monkeypatch, name, c):
    n = 100
    t = lambda: torch.ones((n, c), dtype=DT[name], device="cuda")
    a3, x, out = [t(), t(), t()], t(), torch.full((n, c), 7.0, dtype=DT[name], device="cuda")
    stat3, g3, b3 = torch.ones(6 * c, dtype=torch.float64, device="cuda"), torch.ones(3 * c, device="cuda"), torch.zeros(3 * c, device="cuda")
    assert raw_forward(hip, name, a3, x, stat3, g3, b3, n, c, out) == -4 and b"16-byte pieces" in hip.lib.pcs_last_error()
    ws = torch.zeros(hip.lib.pcs_bn_num_partials() * 6 * c, device="cuda")
    s2 = torch.full((9 * c,), 7.0, dtype=torch.float64, device="cuda")
    assert raw_bwd_stats(hip, name, x, x, a3, stat3, g3, b3, n, c, ws, s2, 9 * c) == -4
    da = [torch.full((n, c), 7.0, dtype=DT[name], device="cuda") for _ in range(3)]
    assert raw_bwd_apply(hip, name, x, x, a3, stat3, g3, b3, s2, n, n, c, out, da) == -4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((s2 == 7.0).all()) and all(bool((d == 7.0).all()) for d in da)
    # the Python entry takes the literal sequence and never asks the kernel
    monkeypatch.setattr(native.backend(), "recon_gate", lambda *a: pytest.fail("recon_gate called for c = %d" % c))
    bns = [bn.cuda().train() for bn in _seeded_bns(c)]
    y = fused.recon_gate(bns, a3, x)
    assert y.shape == (n, c) and y.dtype == DT[name] and bool(torch.isfinite(y).all())


@pytest.mark.gpu
def test_contract(hip):
    """A row pointer 4 bytes off alignment, a null pointer with n > 0, dtype 3, a short sums2."""
    n, c = 64, 16
    q = real_case(257, 64, "fp32")
    a3 = [dev(q["t"]["a%d" % k][:n, :c].contiguous()) for k in range(3)]
    x = dev(q["t"]["x"][:n, :c].contiguous())
    stat3, g3, b3 = torch.ones(6 * c, dtype=torch.float64, device="cuda"), torch.ones(3 * c, device="cuda"), torch.zeros(3 * c, device="cuda")
    buf = torch.zeros(n * c + 4, device="cuda")
    skew = buf[1:1 + n * c].view(n, c)
    assert skew.data_ptr() % 16 == 4
    out = torch.full((n, c), 7.0, device="cuda")
    for args in (([skew, a3[1], a3[2]], x), ([a3[0], a3[1], skew], x), (a3, skew)):
        assert raw_forward(hip, "fp32", args[0], args[1], stat3, g3, b3, n, c, out) == -4 and b"16-byte" in hip.lib.pcs_last_error()
    assert raw_forward(hip, "fp32", a3, x, stat3, g3, b3, n, c, skew) == -4
    ws = torch.zeros(hip.lib.pcs_bn_num_partials() * 6 * c, device="cuda")
    s2 = torch.full((9 * c,), 7.0, dtype=torch.float64, device="cuda")
    da = [torch.full((n, c), 7.0, device="cuda") for _ in range(3)]
    assert raw_bwd_stats(hip, "fp32", skew, x, a3, stat3, g3, b3, n, c, ws, s2, 9 * c) == -4
    assert raw_bwd_apply(hip, "fp32", x, x, a3, stat3, g3, b3, s2, n, n, c, out, [da[0], skew, da[2]]) == -4
    # null pointers with n > 0
    p = native._ptr
    assert hip.lib.pcs_recon_gate_f32(p(a3[0]), None, p(a3[2]), p(x), p(stat3), p(g3), p(b3), n, c, p(out), native._stream()) == -1
    assert hip.lib.pcs_recon_gate_f32(p(a3[0]), p(a3[1]), p(a3[2]), p(x), p(stat3), p(g3), p(b3), n, c, None, native._stream()) == -1
    assert hip.lib.pcs_recon_gate_bwd_stats_f32(p(x), p(x), p(a3[0]), p(a3[1]), p(a3[2]), p(stat3), p(g3), p(b3), n, c, None, p(s2), 9 * c,
                                                native._stream()) == -1
    # a dtype outside {1, 2}
    h = [a.bfloat16() for a in a3]
    oh = torch.full((n, c), 7.0, dtype=torch.bfloat16, device="cuda")
    assert raw_forward(hip, "bf16", h, x.bfloat16(), stat3, g3, b3, n, c, oh, dtype=3) == -1 and b"dtype" in hip.lib.pcs_last_error()
    assert raw_forward(hip, "bf16", h, x.bfloat16(), stat3, g3, b3, n, c, oh, dtype=0) == -1
    # a short sums2: 9c - 1 doubles
    assert raw_bwd_stats(hip, "fp32", x, x, a3, stat3, g3, b3, n, c, ws, s2, 9 * c - 1) == -2 and b"9c doubles" in hip.lib.pcs_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((oh == 7.0).all()) and bool((buf == 0).all()) and bool((s2 == 7.0).all())
    assert all(bool((d == 7.0).all()) for d in da)
    # n == 0 through the backend: outputs of the right shapes, zero sums
    e = torch.empty((0, c), device="cuda")
    assert hip.recon_gate([e, e, e], e, stat3, g3, b3).shape == (0, c)
    z = hip.recon_gate_bwd_stats(e, e, [e, e, e], stat3, g3, b3)
    assert z.shape == (6 * c,) and bool((z == 0).all()) and bool((z._pcs_f32 == 0).all())
    dx, d3 = hip.recon_gate_bwd_apply(e, e, [e, e, e], stat3, g3, b3, z, 0.0)
    assert dx.shape == (0, c) and all(d.shape == (0, c) for d in d3)
