"""SPVCNN's point-branch merge (csrc/pointmerge.hip, fused.point_merge):

    out[i, j] = ( sum_{k<8, idx8[i,k] >= 0} w8[i,k] * vox[idx8[i,k], j] ) + max(0, bn(lin[i, j])),   mask bit (i, j) = [bn > 0]

Bounds (derived, not measured). y64 = the formula in float64 from the inputs as stored, bn64 its BatchNorm term,
A = sum_k |w_k vox_k| + (|lin| + |mean|) |invstd gamma| + |beta|:

    fp32:    |out - y64| <= 16 * 2^-24 * A      nine roundings in the gather sum (eight fused multiply-adds and the final add), the
                                                double -> float conversions of mean and invstd, the products and sums of the affine map
    16 bit:  that plus half an ulp of the storage format at the float64 result, ulp_h(y) = 2^(floor(log2 |y|) - p), p = 7 (bf16) /
             10 (fp16), floored at the smallest normal exponent -- the one rounding of the store. Relative to |y64| half an ulp
             lies between 2^-9 and 2^-8 (bf16), 2^-12 and 2^-11 (fp16), depending on where in its binade the result sits: the
             lower figures are reached only at the top of a binade, and a correctly rounded store exceeds them by up to 2x
             (measured on MI355X: worst error 1.62x of 16 * 2^-24 * A + 2^-9 |y64| at the first bf16 case, the stored value being
             the nearest bf16 number), so the bound is the exact half ulp, not a fixed fraction of |y64|
    mask:    the bit is the gate of the BatchNorm term AS pcs_bn_apply_* WOULD STORE IT, [round_storage(bn) > 0] (fp16 rounds a
             term in (0, 2^-25] to 0: bit clear), so the backward passes see the gate they see after the literal sequence;
             equals [bn64 > 0] wherever |bn64| exceeds the fp32 bound; at most 0.1 % of the elements may be excluded that way

In fp32 the kernel must also reproduce the three operations it replaces bit for bit (same summation order)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from openpcseg_amd import build as pcs_build
from openpcseg_amd import cpu_fallback, fused, native
from openpcseg_amd import functional as F
from openpcseg_amd.fused import FusedBatchNorm

U24 = 2.0 ** -24
FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}   # mantissa bits, smallest normal exponent
NS = [1, 7, 63, 64, 65, 1000]
MS = [1, 50]
CS = [32, 64, 96, 128, 256]


# ---- cases and the float64 side ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, m, c):
    """About 30 % of the corners -1; row 0 without any corner, row 1 with zero weights (n >= 3); the last row reaches voxel m - 1."""
    rng = np.random.default_rng(7 * n + 13 * m + c)
    idx8 = rng.integers(0, m, size=(n, 8)).astype(np.int32)
    idx8[rng.uniform(size=(n, 8)) < 0.3] = -1
    w8 = rng.uniform(0, 1, size=(n, 8)).astype(np.float32)
    if n >= 3:
        idx8[0] = -1
        w8[1] = 0.0
        if n >= 100:
            idx8[n // 2] = -1
    idx8[n - 1, 0] = m - 1
    vox = rng.normal(size=(m, c)).astype(np.float32)
    lin = rng.normal(size=(n, c)).astype(np.float32)
    stat = np.concatenate([0.3 * rng.normal(size=c), rng.uniform(0.5, 2.0, size=c)])   # mean | invstd, float64
    gamma = rng.uniform(0.5, 1.5, size=c).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, size=c).astype(np.float32)
    return idx8, w8, vox, lin, stat, gamma, beta


def stored(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)
    return t, t.float().numpy().astype(np.float64)


def oracle(idx8, w8, vox64, lin64, stat, gamma, beta):
    """-> (y64, bn64, A) of the module docstring."""
    c = vox64.shape[1]
    ok = idx8 >= 0
    term = np.where(ok, w8.astype(np.float64), 0.0)[:, :, None] * vox64[np.maximum(idx8, 0)]
    mean, invstd = stat[:c], stat[c:]
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    bn = (lin64 - mean) * invstd * g64 + b64
    A = np.abs(term).sum(1) + (np.abs(lin64) + np.abs(mean)) * np.abs(invstd * g64) + np.abs(b64)
    return term.sum(1) + np.maximum(bn, 0.0), bn, A


def half_ulp(y, dtype):
    """Half an ulp of the storage format at y (0 for fp32: the fp32 bound already holds its store)."""
    if dtype == torch.float32:
        return np.zeros_like(y)
    p, emin = FMT[dtype]
    a = np.abs(y)
    e = np.full(a.shape, float(emin))
    nz = a > 0
    e[nz] = np.maximum(np.floor(np.log2(a[nz])), emin)
    return 0.5 * 2.0 ** (e - p)


def mask_bits(mask, c):
    m = mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return ((m[:, :, None] >> np.arange(32)) & 1).reshape(mask.shape[0], c).astype(bool)


def check_forward(out, mask, y64, bn64, A, dtype, what):
    o = out.detach().float().cpu().numpy().astype(np.float64)
    bound = 16 * U24 * A + half_ulp(y64, dtype)
    err = np.abs(o - y64)
    worst = float((err / bound).max())
    print("[point merge] %s %s: worst error / bound = %.3f" % (what, dtype, worst))
    assert (err <= bound).all(), (what, worst)
    sure = np.abs(bn64) > 16 * U24 * A
    assert (~sure).mean() <= 1e-3, (what, float((~sure).mean()))
    assert (mask_bits(mask, y64.shape[1])[sure] == (bn64 > 0)[sure]).all(), what


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_merge_entries():
    lib = ctypes.CDLL(pcs_build.LIB_PATH)
    assert hasattr(lib, "pcs_point_merge_f32") and hasattr(lib, "pcs_point_merge_h")
    lib.pcs_abi_version.restype = ctypes.c_int32
    assert lib.pcs_abi_version() == 12 == native.ABI_VERSION
    assert "pcs_point_merge_f32" in native.SIGNATURES and "pcs_point_merge_h" in native.SIGNATURES


def _autograd64(idx8, w8, vox64, lin64, gamma, beta, gout64, eps):
    """Training-mode formula in float64 torch autograd -> (y, bn, grads of vox / lin / gamma / beta, mean, biased var)."""
    vox = torch.from_numpy(vox64).requires_grad_(True)
    lin = torch.from_numpy(lin64).requires_grad_(True)
    g = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    ok = torch.from_numpy(idx8 >= 0)
    w = torch.where(ok, torch.from_numpy(w8.astype(np.float64)), torch.zeros(()).double())
    gather = (w.unsqueeze(-1) * vox[torch.from_numpy(np.maximum(idx8, 0)).long()]).sum(1)
    mean, var = lin.mean(0), lin.var(0, unbiased=False)
    bn = (lin - mean) * torch.rsqrt(var + eps) * g + b
    y = gather + torch.relu(bn)
    y.backward(torch.from_numpy(gout64))
    return (y.detach().numpy(), bn.detach().numpy(), vox.grad.numpy(), lin.grad.numpy(), g.grad.numpy(), b.grad.numpy(),
            mean.detach().numpy(), var.detach().numpy())


def _run_merge(bn, lin, vox, idx8, w8, gout):
    lin, vox = lin.clone().requires_grad_(True), vox.clone().requires_grad_(True)
    bn.zero_grad(set_to_none=True)
    out = fused.point_merge(bn, lin, vox, idx8, w8)
    out.backward(gout)
    return out.detach(), vox.grad, lin.grad, bn.weight.grad.clone(), bn.bias.grad.clone()


def _seeded_bn(c, gamma, beta):
    bn = FusedBatchNorm(c).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
    return bn


@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("c", [32, 24])
def test_point_merge_autograd_on_the_cpu_backend(monkeypatch, c, switch):
    """fused.point_merge on the pure-PyTorch backend (c = 32: its `point_merge`; c = 24 and PCS_POINT_MERGE=0: the literal
    sequence) against float64 autograd. Forward: the fp32 bound of the module docstring with the batch statistics in place of
    mean / invstd. Gradients: sums of fp32 terms, (terms + 2) * 2^-23 * sum |term| for the voxel gradient as
    tests/test_pointvoxel_half.py takes it; the BatchNorm gradients pass two reductions over the n = 257 rows and a handful of
    products per element: 4 n 2^-24 of the largest gradient element, away from gates the forward bound cannot decide."""
    monkeypatch.setenv("PCS_POINT_MERGE", switch)
    n, m = 257, 40
    idx8, w8, vox, lin, _, gamma, beta = case(n, m, c)
    gout = np.random.default_rng(c).normal(size=(n, c)).astype(np.float32)
    y, bn64, gv, gl, gg, gb, mean, var = _autograd64(idx8, w8, vox.astype(np.float64), lin.astype(np.float64), gamma, beta,
                                                     gout.astype(np.float64), 1e-5)
    _, _, A = oracle(idx8, w8, vox.astype(np.float64), lin.astype(np.float64), np.concatenate([mean, 1 / np.sqrt(var + 1e-5)]), gamma, beta)
    with cpu_fallback.enabled() as be:
        calls = []
        orig = be.point_merge
        monkeypatch.setattr(be, "point_merge", lambda *a: (calls.append(1), orig(*a))[1])
        bn = _seeded_bn(c, gamma, beta)
        out, dvox, dlin, dw, db = _run_merge(bn, torch.from_numpy(lin), torch.from_numpy(vox), torch.from_numpy(idx8),
                                             torch.from_numpy(w8), torch.from_numpy(gout))
    assert len(calls) == (1 if (c == 32 and switch == "1") else 0)
    bound = 16 * U24 * A
    assert (np.abs(out.numpy() - y) <= bound).all()
    ok = idx8 >= 0
    S = np.zeros((m, c))
    np.add.at(S, idx8[ok], (w8[ok].astype(np.float64)[:, None] * np.abs(gout.astype(np.float64))[np.nonzero(ok)[0]]))
    terms = np.bincount(idx8[ok], minlength=m).reshape(-1, 1)
    assert (np.abs(dvox.numpy() - gv) <= (terms + 2) * 2.0 ** -23 * S).all()
    sure = np.abs(bn64) > bound
    assert sure.mean() > 0.999
    tol = 4 * n * U24
    assert (np.abs(dlin.numpy() - gl)[sure] <= tol * np.abs(gl).max()).all()
    assert (np.abs(dw.numpy() - gg) <= tol * np.abs(gg).max()).all() and (np.abs(db.numpy() - gb) <= tol * np.abs(gb).max()).all()
    assert np.allclose(bn.running_mean.numpy(), 0.1 * mean, atol=1e-6)
    assert np.allclose(bn.running_var.numpy(), 0.9 + 0.1 * var * n / (n - 1), rtol=1e-5)
    assert int(bn.num_batches_tracked) == 1


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _shapes(c):
    return [(n, m) for n in NS + ([70000] if c == 32 else []) for m in MS]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("c", CS)
def test_kernel_against_float64(hip, c, dtype):
    for n, m in _shapes(c):
        idx8, w8, vox, lin, stat, gamma, beta = case(n, m, c)
        vt, v64 = stored(vox, dtype)
        lt, l64 = stored(lin, dtype)
        y64, bn64, A = oracle(idx8, w8, v64, l64, stat, gamma, beta)
        out, mask = hip.point_merge(dev(vt), dev(idx8), dev(w8), dev(lt), dev(stat), dev(gamma), dev(beta))
        assert out.dtype == dtype and out.shape == (n, c) and mask.shape == (n, c // 32) and mask.dtype == torch.int32
        check_forward(out, mask, y64, bn64, A, dtype, "n=%d m=%d c=%d" % (n, m, c))


@pytest.mark.gpu
@pytest.mark.parametrize("c", CS)
def test_fp32_is_bit_identical_to_the_three_operations(hip, c):
    for n, m in _shapes(c):
        idx8, w8, vox, lin, stat, gamma, beta = (dev(a) for a in case(n, m, c))
        out, mask = hip.point_merge(vox, idx8, w8, lin, stat, gamma, beta)
        y, ymask = hip.bn_apply(lin, None, stat, gamma, beta, True, want_mask=True)
        ref = hip.devoxelize_fwd(vox, idx8, w8) + y
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), (n, m, c)
        assert torch.equal(mask, ymask), (n, m, c)


def test_empty_input_is_a_no_op_without_a_device():
    """n == 0 returns 0 before any pointer is looked at; a dtype outside {1, 2} is PCS_EINVAL; c % 32 != 0 is PCS_EUNSUPPORTED."""
    lib = native.load_library()
    assert lib.pcs_point_merge_f32(None, None, None, None, None, None, None, 0, 64, None, None, None) == 0
    assert lib.pcs_point_merge_h(None, None, None, None, None, None, None, 0, 64, 1, None, None, None) == 0
    assert lib.pcs_point_merge_h(None, None, None, None, None, None, None, 0, 64, 3, None, None, None) == -1
    assert lib.pcs_point_merge_f32(None, None, None, None, None, None, None, 0, 24, None, None, None) == -4
    assert b"pcs_point_merge_f32" in lib.pcs_last_error()


def _float64_side(idx8, w8, v64, l64, gamma, beta, g64):
    return _autograd64(idx8, w8, v64, l64, gamma, beta, g64, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,c", [(1000, 50, 96), (4097, 300, 256)])
def test_autograd_fp32_is_bit_identical_to_the_literal_sequence(hip, monkeypatch, n, m, c):
    idx8, w8, vox, lin, _, gamma, beta = case(n, m, c)
    gout = dev(np.random.default_rng(n).normal(size=(n, c)).astype(np.float32))
    got = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("PCS_POINT_MERGE", switch)
        calls = []
        be = native.backend()
        orig = be.point_merge
        monkeypatch.setattr(be, "point_merge", lambda *a: (calls.append(1), orig(*a))[1])
        bn = _seeded_bn(c, gamma, beta).cuda()
        got[switch] = _run_merge(bn, dev(lin), dev(vox), dev(idx8), dev(w8), gout) + (bn.running_mean.clone(), bn.running_var.clone())
        monkeypatch.setattr(be, "point_merge", orig)
        assert len(calls) == int(switch)
    for a, b, what in zip(got["1"], got["0"], ("out", "dvox", "dlin", "dgamma", "dbeta", "running_mean", "running_var")):
        assert torch.equal(a, b), what
    # and the values against float64 autograd. The batch statistics are sums of n fp32 terms here (fp32 partials per workgroup),
    # so the mean / invstd the apply pass reads carry up to n more roundings than the 16 of the kernel bound
    y, bn64, gv, gl, gg, gb, mean, var = _float64_side(idx8, w8, vox.astype(np.float64), lin.astype(np.float64), gamma, beta,
                                                       gout.cpu().numpy().astype(np.float64))
    out, dvox, dlin, dw, db, rm, rv = (t.cpu().numpy() for t in got["1"])
    _, _, A = oracle(idx8, w8, vox.astype(np.float64), lin.astype(np.float64), np.concatenate([mean, 1 / np.sqrt(var + 1e-5)]), gamma, beta)
    assert (np.abs(out - y) <= (16 + n) * U24 * A).all()
    sure = np.abs(bn64) > (16 + n) * U24 * A
    tol = 4 * n * U24
    assert (np.abs(dlin - gl)[sure] <= tol * np.abs(gl).max()).all()
    assert np.abs(dvox - gv).max() <= tol * np.abs(gv).max()
    assert np.abs(dw - gg).max() <= tol * np.abs(gg).max() and np.abs(db - gb).max() <= tol * np.abs(gb).max()
    assert np.allclose(rm, 0.1 * mean, atol=1e-6) and np.allclose(rv, 0.9 + 0.1 * var * n / (n - 1), rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("n,m,c", [(1000, 50, 96), (4097, 300, 256)])
def test_autograd_bf16_against_float64(hip, monkeypatch, n, m, c, switch):
    """16-bit leaves outside autocast, the merge kernel and the literal sequence alike. Voxel gradient: the bound
    tests/test_pointvoxel_half.py takes for the spdevoxelize backward (half an ulp of the stored value plus (terms + 2) 2^-23
    sum |term|). Remaining gradients: the bounds of test_hip_parity.test_fused_batchnorm_half_io (eps = 2^-8: 2 eps of the
    largest element for dx away from undecided gates, 2e-2 for the parameter gradients, 1e-4 / 1e-5 for the running statistics)."""
    from test_pointvoxel_half import check, devox_bwd_oracle
    dtype, eps = torch.bfloat16, 2.0 ** -8
    monkeypatch.setenv("PCS_POINT_MERGE", switch)
    idx8, w8, vox, lin, _, gamma, beta = case(n, m, c)
    vt, v64 = stored(vox, dtype)
    lt, l64 = stored(lin, dtype)
    gt, g64 = stored(np.random.default_rng(n).normal(size=(n, c)).astype(np.float32), dtype)
    y, bn64, gv, gl, gg, gb, mean, var = _float64_side(idx8, w8, v64, l64, gamma, beta, g64)
    bn = _seeded_bn(c, gamma, beta).cuda()
    out, dvox, dlin, dw, db = _run_merge(bn, dev(lt), dev(vt), dev(idx8), dev(w8), dev(gt))
    assert out.dtype == dtype and dvox.dtype == dtype and dlin.dtype == dtype and dw.dtype == torch.float32
    _, _, A = oracle(idx8, w8, v64, l64, np.concatenate([mean, 1 / np.sqrt(var + 1e-5)]), gamma, beta)
    # forward: one rounding fused, three in the literal sequence (each half an ulp of a value no larger than the sum of the parts)
    roundings = 1 if switch == "1" else 3
    o = out.float().cpu().numpy().astype(np.float64)
    assert (np.abs(o - y) <= 16 * U24 * A + roundings * 2.0 ** -8 * A).all()   # half a bf16 ulp is at most 2^-8 of the value
    yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w8.astype(np.float64), m)
    assert np.abs(yb - gv).max() < 1e-9
    check(dvox, yb, Sb, ntb, dtype, "merge dvox n=%d c=%d" % (n, c))
    live = np.abs(bn64) > 4 * eps
    d = np.abs(dlin.float().cpu().numpy() - gl)
    assert d[live].max() <= 2 * eps * np.abs(gl).max() + 1e-6
    for got, ref in ((dw, gg), (db, gb)):
        assert np.allclose(got.cpu().numpy(), ref, rtol=2e-2, atol=2e-2 * np.abs(ref).max())
    assert np.allclose(bn.running_var.cpu().numpy(), 0.9 + 0.1 * var * n / (n - 1), rtol=1e-4)
    assert np.allclose(bn.running_mean.cpu().numpy(), 0.1 * mean, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [24, 48])
def test_unsupported_widths(hip, monkeypatch, c):
    n, m = 300, 20
    idx8, w8, vox, lin, stat, gamma, beta = (dev(a) for a in case(n, m, c))
    out = torch.full((n, c), 7.0, device="cuda")
    mask = torch.zeros((n, c // 32 + 1), dtype=torch.int32, device="cuda")
    p = native._ptr
    rc = hip.lib.pcs_point_merge_f32(p(vox), p(idx8), p(w8), p(lin), p(stat), p(gamma), p(beta), n, c, p(out), p(mask), native._stream())
    assert rc == -4 and b"multiple of 32" in hip.lib.pcs_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the Python entry: the literal sequence, the kernel is not asked
    be = native.backend()
    monkeypatch.setattr(be, "point_merge", lambda *a: pytest.fail("point_merge called for c = %d" % c))
    res = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("PCS_POINT_MERGE", switch)
        bn = _seeded_bn(c, gamma.cpu().numpy(), beta.cpu().numpy()).cuda()
        res[switch] = _run_merge(bn, lin, vox, idx8, w8, torch.ones((n, c), device="cuda"))
    for a, b in zip(res["1"], res["0"]):
        assert torch.equal(a, b)
    bn = _seeded_bn(c, gamma.cpu().numpy(), beta.cpu().numpy()).cuda()
    ref = F.spdevoxelize(vox, idx8, w8) + torch.relu(torch.nn.functional.batch_norm(lin, None, None, bn.weight, bn.bias, True, 0.1, 1e-5))
    assert torch.allclose(res["1"][0], ref, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_misaligned_rows_are_rejected_not_read(hip):
    """A row pointer 4 bytes off a 16-byte boundary: PCS_EUNSUPPORTED from the entry, nothing launched, `out` untouched."""
    n, m, c = 64, 10, 32
    idx8, w8, vox, lin, stat, gamma, beta = (dev(a) for a in case(n, m, c))
    buf = torch.zeros(n * c + 4, device="cuda")
    skew = buf[1:1 + n * c].view(n, c)
    assert skew.data_ptr() % 16 == 4
    out = torch.full((n, c), 7.0, device="cuda")
    mask = torch.zeros((n, 1), dtype=torch.int32, device="cuda")
    p = native._ptr
    for args in ((p(vox), p(idx8), p(w8), p(skew)), (p(skew[:m]), p(idx8), p(w8), p(lin))):
        rc = hip.lib.pcs_point_merge_f32(*args, p(stat), p(gamma), p(beta), n, c, p(out), p(mask), native._stream())
        assert rc == -4 and b"16-byte" in hip.lib.pcs_last_error()
    rc = hip.lib.pcs_point_merge_f32(p(vox), p(idx8), p(w8), p(lin), p(stat), p(gamma), p(beta), n, c, p(skew), p(mask), native._stream())
    assert rc == -4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 0).all())


@pytest.mark.gpu
def test_mixed_dtypes_and_eval_mode(hip):
    """A 16-bit operand beside an fp32 one is cast up (fp32 entry, fp32 out); eval mode reads the running statistics."""
    n, m, c = 500, 30, 64
    idx8, w8, vox, lin, stat, gamma, beta = case(n, m, c)
    lt, l64 = stored(lin, torch.bfloat16)
    y64, bn64, A = oracle(idx8, w8, vox.astype(np.float64), l64, stat, gamma, beta)
    out, mask = hip.point_merge(dev(vox), dev(idx8), dev(w8), dev(lt), dev(stat), dev(gamma), dev(beta))
    assert out.dtype == torch.float32
    check_forward(out, mask, y64, bn64, A, torch.float32, "mixed")
    bn = _seeded_bn(c, gamma, beta).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(dev(stat[:c]).float())
        bn.running_var.copy_((1.0 / dev(stat[c:]) ** 2 - bn.eps).float())
        got = fused.point_merge(bn, dev(lin), dev(vox), dev(idx8), dev(w8))
    rm, rv = bn.running_mean.double().cpu().numpy(), bn.running_var.double().cpu().numpy()
    y64, bn64, A = oracle(idx8, w8, vox.astype(np.float64), lin.astype(np.float64), np.concatenate([rm, 1 / np.sqrt(rv + bn.eps)]), gamma, beta)
    assert (np.abs(got.cpu().numpy() - y64) <= 16 * U24 * A).all()
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.gpu
def test_mask_bit_is_the_gate_of_the_stored_batchnorm_term(hip):
    """One fp16 element whose BatchNorm term is positive in fp32 and would store as 0 (lin = mean = 0, beta = 2^-26): its mask
    bit is clear, as in the mask pcs_bn_apply_h writes for the same input; the merged output still adds the unrounded term
    (one rounding). In fp32 and bf16 the term survives the store and the bit is set."""
    n, m, c = 4, 3, 32
    idx8 = np.full((n, 8), -1, dtype=np.int32)
    idx8[:, 0] = [0, 1, 2, 0]
    w8 = np.full((n, 8), 0.5, dtype=np.float32)
    vox = np.arange(m * c, dtype=np.float32).reshape(m, c) / 8
    lin = np.zeros((n, c), dtype=np.float32)
    stat = np.concatenate([np.zeros(c), np.ones(c)])
    beta = np.ones(c, dtype=np.float32)
    beta[:4] = [2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -25]   # fp16: 0, 0 (tie to even), 2^-24, 2^-24
    for dtype, on in [(torch.float16, [False, False, True, True]), (torch.float32, [True] * 4), (torch.bfloat16, [True] * 4)]:
        vt, v64 = stored(vox, dtype)
        lt, l64 = stored(lin, dtype)
        out, mask = hip.point_merge(dev(vt), dev(idx8), dev(w8), dev(lt), dev(stat), None, dev(beta))
        y, ymask = hip.bn_apply(dev(lt), None, dev(stat), None, dev(beta), True, want_mask=True)
        assert torch.equal(mask, ymask), dtype
        bits = mask_bits(mask, c)
        assert np.array_equal(bits, y.float().cpu().numpy() > 0), dtype
        assert bits[:, :4].tolist() == [on] * n and bits[:, 4:].all(), dtype
        y64, bn64, A = oracle(idx8, w8, v64, l64, stat, np.ones(c, dtype=np.float32), beta)
        assert (np.abs(out.float().cpu().numpy() - y64) <= 16 * U24 * A + half_ulp(y64, dtype)).all(), dtype
