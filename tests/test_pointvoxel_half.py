"""spvoxelize / spdevoxelize with 16-bit features (the bf16 / fp16 instances of csrc/pointvoxel.hip) against a float64 oracle.

The features arrive as bf16 / fp16 and leave in the same format; the kernels accumulate in fp32 registers and round once on the
store. Bound (derived, not measured): with y the float64 result computed from the STORED inputs (already rounded to 16 bits,
weights as passed), S the same sum over absolute values, n_terms the number of terms of that output row, p = 7 (bf16) / 10
(fp16) and ulp_h(x) = 2^(floor(log2 |x|) - p) floored at the format's smallest normal exponent (-126 / -14):

    |out - y| <= 0.5 * ulp_h(max(|y|, |out|)) + (n_terms + 2) * 2^-23 * S

-- one rounding to storage plus the standard fp32 summation bound with a factor 2 of slack. The voxelize backward is one fp32
division: 0.5 * ulp_h + 2 * 2^-23 * |y|.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from openpcseg_amd import functional as F
from openpcseg_amd import native

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}   # mantissa bits, smallest normal exponent
CODE = {torch.bfloat16: 1, torch.float16: 2}
U23 = 2.0 ** -23


# ---- oracle side ---------------------------------------------------------------------------------------------------------
def stored(a, dtype):
    """fp32 host array -> (tensor rounded to the 16-bit format, the stored values as float64)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)
    return t, t.float().numpy().astype(np.float64)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def ulp_h(x, dtype):
    p, emin = FMT[dtype]
    x = np.abs(np.asarray(x, np.float64))
    e = np.full(x.shape, float(emin))
    nz = x > 0
    e[nz] = np.maximum(np.floor(np.log2(x[nz])), emin)
    return 2.0 ** (e - p)


def check(out, y, S, n_terms, dtype, what):
    """Asserts the bound of the module docstring; n_terms per output row."""
    out = f64(out) if isinstance(out, torch.Tensor) else out
    assert out.shape == y.shape, (what, out.shape, y.shape)
    bound = 0.5 * ulp_h(np.maximum(np.abs(y), np.abs(out)), dtype) + (np.asarray(n_terms, np.float64).reshape(-1, 1) + 2) * U23 * S
    err = np.abs(out - y)
    worst = float((err / bound).max()) if err.size else 0.0
    print("[pointvoxel half] %s %s: worst error / bound = %.3f" % (what, dtype, worst))
    assert (err <= bound).all(), (what, worst)


@functools.lru_cache(maxsize=None)
def vox_case(c, n=3000, m=300):
    """idx: 17 rows of -1, voxel 0 without a point, voxel 1 with one point, voxel 2 with 130, the rest spread over 3..m-1."""
    rng = np.random.default_rng(1000 + c)
    idx = np.empty(n, np.int32)
    idx[:17] = -1
    idx[17] = 1
    idx[18:148] = 2
    idx[148:] = rng.integers(3, m, size=n - 148)
    idx = idx[rng.permutation(n)]
    counts = np.bincount(idx[idx >= 0], minlength=m).astype(np.int32)
    assert counts[0] == 0 and counts[1] == 1 and counts[2] == 130 and (counts[3:] % 2 == 0).any() and (counts[3:] % 2 == 1).any()
    feats = rng.normal(size=(n, c)).astype(np.float32)
    gout = rng.normal(size=(m, c)).astype(np.float32)
    return idx, counts, feats, gout


def vox_oracle(feats64, idx, counts):
    m = counts.shape[0]
    ok = idx >= 0
    term = feats64[ok] / counts[idx[ok]].astype(np.float64)[:, None]
    y = np.zeros((m, feats64.shape[1]))
    S = np.zeros_like(y)
    np.add.at(y, idx[ok], term)
    np.add.at(S, idx[ok], np.abs(term))
    return y, S


def vox_bwd_oracle(gout64, idx, counts):
    y = np.zeros((idx.shape[0], gout64.shape[1]))
    ok = (idx >= 0) & (counts[np.maximum(idx, 0)] > 0)
    y[ok] = gout64[idx[ok]] / counts[idx[ok]].astype(np.float64)[:, None]
    return y


@functools.lru_cache(maxsize=None)
def devox_case(c, m, n=3000):
    """idx8 drawn from [-1, m); row 0 has no corner at all, row 1 only zero weights."""
    rng = np.random.default_rng(2000 + c + m)
    idx8 = rng.integers(-1, m, size=(n, 8)).astype(np.int32)
    idx8[0] = -1
    w8 = rng.uniform(0, 1, size=(n, 8)).astype(np.float32)
    w8[1] = 0.0
    feat = rng.normal(size=(m, c)).astype(np.float32)
    gout = rng.normal(size=(n, c)).astype(np.float32)
    return idx8, w8, feat, gout


def devox_oracle(feat64, idx8, w64):
    ok = idx8 >= 0
    term = np.where(ok, w64, 0.0)[:, :, None] * feat64[np.maximum(idx8, 0)]
    return term.sum(1), np.abs(term).sum(1), ok.sum(1)


def devox_bwd_oracle(gout64, idx8, w64, m):
    ok = (idx8 >= 0).reshape(-1)
    rows = np.repeat(np.arange(idx8.shape[0]), 8)[ok]
    term = w64.reshape(-1)[ok][:, None] * gout64[rows]
    y = np.zeros((m, gout64.shape[1]))
    S = np.zeros_like(y)
    np.add.at(y, idx8.reshape(-1)[ok], term)
    np.add.at(S, idx8.reshape(-1)[ok], np.abs(term))
    return y, S, np.bincount(idx8.reshape(-1)[ok], minlength=m)


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


# ---- CPU cases -------------------------------------------------------------------------------------------------------------
def test_pointvoxel_policy_api():
    assert F.get_pointvoxel_policy() == "fp32"
    try:
        F.set_pointvoxel_policy("keep")
        assert F.get_pointvoxel_policy() == "keep"
        F.set_pointvoxel_policy("fp32")
        assert F.get_pointvoxel_policy() == "fp32"
        for bad in ("half", "bf16", None, ""):
            with pytest.raises(ValueError):
                F.set_pointvoxel_policy(bad)
        assert F.get_pointvoxel_policy() == "fp32"
    finally:
        F.set_pointvoxel_policy("fp32")


@pytest.mark.parametrize("dtype", [0, 3])
def test_half_entries_refuse_other_dtypes_without_a_device(dtype):
    """The argument checks of the four _h entries run before any HIP call: dtype other than 1 / 2 is PCS_EINVAL."""
    lib = native.load_library()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    calls = {
        "pcs_voxelize_fwd_csr_h": lambda: lib.pcs_voxelize_fwd_csr_h(p, p, p, p, 8, 4, dtype, p, None),
        "pcs_voxelize_bwd_h": lambda: lib.pcs_voxelize_bwd_h(p, p, p, 8, 4, dtype, p, None),
        "pcs_devoxelize_fwd_h": lambda: lib.pcs_devoxelize_fwd_h(p, p, p, 8, 4, dtype, p, None),
        "pcs_devoxelize_bwd_csr_h": lambda: lib.pcs_devoxelize_bwd_csr_h(p, p, p, p, 8, 4, dtype, p, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.pcs_last_error()
        assert msg and name.encode() in msg, (name, msg)
    assert lib.pcs_abi_version() == 12


# ---- GPU cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [3, 4, 12, 32, 96, 520])
def test_voxelize_half(hip, c, dtype):
    """c = 3 scalar, 4 / 12 the 8-byte accesses, 32 / 96 the 16-byte ones, 520 more than one pass of the lane row."""
    idx, counts, feats, gout = vox_case(c)
    ft, f64s = stored(feats, dtype)
    y, S = vox_oracle(f64s, idx, counts)
    di, dc = dev(idx), dev(counts)
    out = hip.voxelize_fwd(dev(ft), di, dc)
    assert out.dtype == dtype and out.shape == (counts.shape[0], c)
    check(out, y, S, counts, dtype, "voxelize fwd c=%d" % c)
    assert torch.equal(out.view(torch.int16), hip.voxelize_fwd(dev(ft), di, dc).view(torch.int16))   # run-to-run identical
    assert (out[dev(counts == 0)].view(torch.int16) == 0).all()                                         # empty voxels: exact zeros
    gt, g64 = stored(gout, dtype)
    yb = vox_bwd_oracle(g64, idx, counts)
    gin = hip.voxelize_bwd(dev(gt), di, dc, idx.shape[0])
    assert gin.dtype == dtype
    check(gin, yb, np.abs(yb), np.zeros(idx.shape[0]), dtype, "voxelize bwd c=%d" % c)   # (0 + 2) * 2^-23 * |y|
    assert (gin[dev(idx < 0)].view(torch.int16) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,m", [(5, 400), (8, 37), (20, 400), (32, 400), (96, 400), (520, 50), (8, 20000)])
def test_devoxelize_half(hip, c, m, dtype):
    """(5, 400) scalar; (8, 37) the wave-per-voxel backward with ~650 entries per voxel; (20, 400) c % 4 but not % 8; (96, 400)
    and (520, 50) the lane-row backward; (8, 20000) mostly empty and one-entry voxels."""
    idx8, w8, feat, gout = devox_case(c, m)
    w64 = w8.astype(np.float64)
    ft, f64s = stored(feat, dtype)
    y, S, nt = devox_oracle(f64s, idx8, w64)
    di, dw = dev(idx8), dev(w8)
    out = hip.devoxelize_fwd(dev(ft), di, dw)
    assert out.dtype == dtype
    check(out, y, S, nt, dtype, "devoxelize fwd c=%d m=%d" % (c, m))
    assert (out[0].view(torch.int16) == 0).all() and (out[1].view(torch.int16) == 0).all()
    gt, g64 = stored(gout, dtype)
    yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w64, m)
    gfeat = hip.devoxelize_bwd(dev(gt), di, dw, m)
    assert gfeat.dtype == dtype
    check(gfeat, yb, Sb, ntb, dtype, "devoxelize bwd c=%d m=%d" % (c, m))
    assert (gfeat[dev(ntb == 0)].view(torch.int16) == 0).all()
    assert torch.equal(gfeat.view(torch.int16), hip.devoxelize_bwd(dev(gt), di, dw, m).view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_output_row_is_written(hip, dtype):
    """The two segmented entries on NaN-prefilled outputs: every row is stored, empty ones included."""
    lib = native.load_library()
    for c in (3, 12, 32, 520):
        idx, counts, feats, _ = vox_case(c)
        m = counts.shape[0]
        order, rowptr = hip._csr(dev(idx), m)
        ft, dc = dev(stored(feats, dtype)[0]), dev(counts)
        out = torch.full((m, c), float("nan"), dtype=dtype, device=DEV)
        rc = lib.pcs_voxelize_fwd_csr_h(native._ptr(ft), native._ptr(order), native._ptr(rowptr), native._ptr(dc), m, c, CODE[dtype],
                                        native._ptr(out), native._stream())
        assert rc == 0 and not torch.isnan(out).any(), c
    for c, m in ((5, 400), (8, 37), (20, 400), (96, 400), (8, 20000)):
        idx8, w8, _, gout = devox_case(c, m)
        order, rowptr = hip._csr(dev(idx8), m)
        gt, dw = dev(stored(gout, dtype)[0]), dev(w8)
        gfeat = torch.full((m, c), float("nan"), dtype=dtype, device=DEV)
        rc = lib.pcs_devoxelize_bwd_csr_h(native._ptr(gt), native._ptr(order), native._ptr(rowptr), native._ptr(dw), m, c, CODE[dtype],
                                          native._ptr(gfeat), native._stream())
        assert rc == 0 and not torch.isnan(gfeat).any(), (c, m)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_segmented_forms(hip, dtype):
    """The lane-row kernels keep 4 row loads in flight on levels of at most 400 000 voxels and 2 above; a narrow row above that
    size leaves the wave-per-voxel form. One level just above the threshold through the default dispatch, and both forms forced
    on the small cases: inside the bound and bit-identical to each other (same summation order)."""
    m = 400001
    idx, counts, feats, _ = vox_case(12, 3000, m)
    ft, f64s = stored(feats, dtype)
    y, S = vox_oracle(f64s, idx, counts)
    out = hip.voxelize_fwd(dev(ft), dev(idx), dev(counts))
    check(out, y, S, counts, dtype, "voxelize fwd m=%d" % m)
    idx8, w8, _, gout = devox_case(8, m)
    gt, g64 = stored(gout, dtype)
    yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w8.astype(np.float64), m)
    check(hip.devoxelize_bwd(dev(gt), dev(idx8), dev(w8), m), yb, Sb, ntb, dtype, "devoxelize bwd c=8 m=%d" % m)
    force = native.load_library().pcs_debug_pointvoxel_h_inflight
    try:
        for c in (3, 12, 96, 520):
            idx, counts, feats, _ = vox_case(c)
            ft, f64s = stored(feats, dtype)
            y, S = vox_oracle(f64s, idx, counts)
            got = []
            for loads in (2, 4):
                force(loads)
                got.append(hip.voxelize_fwd(dev(ft), dev(idx), dev(counts)))
                check(got[-1], y, S, counts, dtype, "voxelize fwd c=%d, %d loads" % (c, loads))
            assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16)), c
        for c, m in ((5, 400), (96, 400), (520, 50)):
            idx8, w8, _, gout = devox_case(c, m)
            gt, g64 = stored(gout, dtype)
            yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w8.astype(np.float64), m)
            got = []
            for loads in (2, 4):
                force(loads)
                got.append(hip.devoxelize_bwd(dev(gt), dev(idx8), dev(w8), m))
                check(got[-1], yb, Sb, ntb, dtype, "devoxelize bwd c=%d m=%d, %d loads" % (c, m, loads))
            assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16)), (c, m)
    finally:
        force(0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_sizes(hip, dtype):
    def e(*shape, dt=dtype):
        return torch.empty(shape, dtype=dt, device=DEV)
    out = hip.voxelize_fwd(e(0, 6), e(0, dt=torch.int32), e(0, dt=torch.int32))
    assert out.shape == (0, 6) and out.dtype == dtype
    gin = hip.voxelize_bwd(e(5, 6), e(0, dt=torch.int32), torch.ones(5, dtype=torch.int32, device=DEV), 0)
    assert gin.shape == (0, 6) and gin.dtype == dtype
    out = hip.devoxelize_fwd(e(5, 6), e(0, 8, dt=torch.int32), e(0, 8, dt=torch.float32))
    assert out.shape == (0, 6) and out.dtype == dtype
    gfeat = hip.devoxelize_bwd(e(0, 6), e(0, 8, dt=torch.int32), e(0, 8, dt=torch.float32), 0)
    assert gfeat.shape == (0, 6) and gfeat.dtype == dtype
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_outside_autocast(hip, dtype):
    """16-bit leaves: the output and .grad keep the dtype, values inside the kernels' bounds."""
    c = 12
    idx, counts, feats, gout = vox_case(c)
    ft, f64s = stored(feats, dtype)
    gt, g64 = stored(gout, dtype)
    leaf = dev(ft).requires_grad_(True)
    out = F.spvoxelize(leaf, dev(idx), dev(counts))
    out.backward(dev(gt))
    assert out.dtype == dtype and leaf.grad.dtype == dtype
    y, S = vox_oracle(f64s, idx, counts)
    check(out, y, S, counts, dtype, "spvoxelize")
    yb = vox_bwd_oracle(g64, idx, counts)
    check(leaf.grad, yb, np.abs(yb), np.zeros(idx.shape[0]), dtype, "spvoxelize grad")

    c, m = 20, 400
    idx8, w8, feat, gout = devox_case(c, m)
    ft, f64s = stored(feat, dtype)
    gt, g64 = stored(gout, dtype)
    leaf = dev(ft).requires_grad_(True)
    out = F.spdevoxelize(leaf, dev(idx8), dev(w8))
    out.backward(dev(gt))
    assert out.dtype == dtype and leaf.grad.dtype == dtype
    w64 = w8.astype(np.float64)
    y, S, nt = devox_oracle(f64s, idx8, w64)
    check(out, y, S, nt, dtype, "spdevoxelize")
    yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w64, m)
    check(leaf.grad, yb, Sb, ntb, dtype, "spdevoxelize grad")
    # weights that arrive in 16 bits are computed with in fp32
    wt, w64h = stored(w8, dtype)
    out = F.spdevoxelize(dev(ft), dev(idx8), dev(wt))
    y, S, nt = devox_oracle(f64s, idx8, w64h)
    assert out.dtype == dtype
    check(out, y, S, nt, dtype, "spdevoxelize, 16-bit weights")


def _far_points(n=6000):
    """Points whose voxel coordinates reach beyond 2048 (fp16 holds integers exactly only up to 2048, bf16 up to 256), several
    points per voxel, two frames."""
    rng = np.random.default_rng(7)
    cells = rng.integers(0, 6000, size=(n // 4, 3))
    xyz = np.repeat(cells, 4, axis=0) + rng.uniform(0.05, 0.95, size=(n // 4 * 4, 3))
    b = rng.integers(0, 2, size=(xyz.shape[0], 1))
    coords = np.concatenate([xyz, b], 1).astype(np.float32)
    return torch.from_numpy(coords).to(DEV), torch.from_numpy(rng.normal(size=(xyz.shape[0], 4)).astype(np.float32)).to(DEV)


@pytest.mark.gpu
def test_policy_under_autocast(hip):
    from openpcseg_amd.sparse import PointTensor
    from openpcseg_amd.workloads.pointvoxel import initial_voxelize
    dtype = torch.bfloat16
    idx, counts, feats, _ = vox_case(32)
    idx8, w8, feat, _ = devox_case(32, 400)
    xv, xd = dev(stored(feats, dtype)[0]), dev(stored(feat, dtype)[0])
    di, dc, d8, dw = dev(idx), dev(counts), dev(idx8), dev(w8)
    want_v, want_d = F.spvoxelize(xv.float(), di, dc), F.spdevoxelize(xd.float(), d8, dw)
    coords, pf = _far_points()

    def voxel_coords():
        return initial_voxelize(PointTensor(pf, coords.clone()), 1.0, 1.0).C

    plain = voxel_coords()
    assert int(plain[:, :3].max()) > 2048
    assert F.get_pointvoxel_policy() == "fp32"
    try:
        with torch.autocast("cuda", dtype=dtype):
            got_v, got_d = F.spvoxelize(xv, di, dc), F.spdevoxelize(xd, d8, dw)
            c_fp32 = voxel_coords()
        assert got_v.dtype == torch.float32 and torch.equal(got_v, want_v)      # the default: today's behaviour, bit for bit
        assert got_d.dtype == torch.float32 and torch.equal(got_d, want_d)
        F.set_pointvoxel_policy("keep")
        with torch.autocast("cuda", dtype=dtype):
            keep_v, keep_d = F.spvoxelize(xv, di, dc), F.spdevoxelize(xd, d8, dw)
            keep_v32, keep_d32 = F.spvoxelize(xv.float(), di, dc), F.spdevoxelize(xd.float(), d8, dw)
            c_keep = voxel_coords()
        assert keep_v.dtype == dtype and keep_d.dtype == dtype
        assert keep_v32.dtype == torch.float32 and torch.equal(keep_v32, want_v)
        assert keep_d32.dtype == torch.float32 and torch.equal(keep_d32, want_d)
        assert torch.equal(keep_v.view(torch.int16), hip.voxelize_fwd(xv, di, dc).view(torch.int16))
        # voxel coordinates are averaged through spvoxelize: "keep" never rounds them to 16 bits
        assert c_keep.dtype == torch.int32 and torch.equal(c_keep, c_fp32) and torch.equal(c_keep, plain)
    finally:
        F.set_pointvoxel_policy("fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_backend_shim_takes_half(hip, dtype):
    """The reference's nn/functional hands the four *_cuda functions half tensors under autocast, the weight included."""
    from openpcseg_amd import backend_shim as shim
    c = 12
    idx, counts, feats, gout = vox_case(c)
    ft, f64s = stored(feats, dtype)
    gt, g64 = stored(gout, dtype)
    out = shim.voxelize_forward_cuda(dev(ft), dev(idx), dev(counts))
    y, S = vox_oracle(f64s, idx, counts)
    assert out.dtype == dtype
    check(out, y, S, counts, dtype, "shim voxelize fwd")
    gin = shim.voxelize_backward_cuda(dev(gt), dev(idx), dev(counts), idx.shape[0])
    yb = vox_bwd_oracle(g64, idx, counts)
    assert gin.dtype == dtype
    check(gin, yb, np.abs(yb), np.zeros(idx.shape[0]), dtype, "shim voxelize bwd")

    c, m = 20, 400
    idx8, w8, feat, gout = devox_case(c, m)
    ft, f64s = stored(feat, dtype)
    gt, g64 = stored(gout, dtype)
    wt, w64 = stored(w8, dtype)          # the oracle uses the rounded weights
    out = shim.devoxelize_forward_cuda(dev(ft), dev(idx8), dev(wt))
    y, S, nt = devox_oracle(f64s, idx8, w64)
    assert out.dtype == dtype
    check(out, y, S, nt, dtype, "shim devoxelize fwd")
    gfeat = shim.devoxelize_backward_cuda(dev(gt), dev(idx8), dev(wt), m)
    yb, Sb, ntb = devox_bwd_oracle(g64, idx8, w64, m)
    assert gfeat.dtype == dtype
    check(gfeat, yb, Sb, ntb, dtype, "shim devoxelize bwd")


@pytest.mark.gpu
def test_point_branch_hop_chain(hip):
    """A point-branch chain of four hops, forward and backward, three ways with the same weights: (a) fp32, (b) bf16 autocast with
    the default policy, (c) bf16 autocast with "keep". Yardstick (a): the output error and the largest parameter-gradient error
    of (c) are at most 2x those of (b) -- the hops add four roundings of the size every conv / BatchNorm output of the path already
    carries, and errors of that kind grow like the square root of their number.
    Measured on MI355X: both ratios 1.000 (output error 4.3e-3, gradient error 3.9e-3 of the tensor maximum either way). The
    points of a synthetic batch are its voxel centres, so most trilinear weights are 0 or 1 and most voxels hold one point: the
    hops mostly copy rows that are bf16 values already, which the rounding on the store leaves alone."""
    from openpcseg_amd import modules as spnn
    from openpcseg_amd.fused import FusedBatchNorm
    from openpcseg_amd.sparse import PointTensor
    from openpcseg_amd.workloads import synthetic
    from openpcseg_amd.workloads.pointvoxel import initial_voxelize, point_to_voxel, voxel_to_point

    torch.manual_seed(0)
    conv1, bn, lin, conv2 = spnn.Conv3d(4, 32, 3), FusedBatchNorm(32), torch.nn.Linear(32, 32), spnn.Conv3d(32, 32, 2, stride=2)
    mods = torch.nn.ModuleList([conv1, bn, lin, conv2]).to(DEV).train()
    lidar = synthetic.make_batch([0, 1], n_points=4000)["lidar"]
    feats, coords = lidar.F.to(DEV), lidar.C.to(DEV).float()

    def run(amp, policy):
        mods.zero_grad(set_to_none=True)
        hops = []
        F.set_pointvoxel_policy(policy)
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                z = PointTensor(feats, coords.clone())
                x0 = initial_voxelize(z, 1.0, 1.0)
                x1 = bn(conv1(x0), relu=True)
                z1 = voxel_to_point(x1, z)
                hops.append((x1.F.dtype, z1.F.dtype))
                z1.F = z1.F + lin(z1.F)
                x2 = point_to_voxel(x1, z1)
                hops.append((z1.F.dtype, x2.F.dtype))
                x3 = conv2(x2)
                z2 = voxel_to_point(x3, z1)
                hops.append((x3.F.dtype, z2.F.dtype))
                out = z2.F
                out.float().pow(2).sum().backward()
        finally:
            F.set_pointvoxel_policy("fp32")
        return out.detach().double(), [p.grad.detach().double() for p in mods.parameters()], hops

    def errors(got, ref):
        out_err = float((got[0] - ref[0]).abs().max() / ref[0].abs().max())
        grad_err = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got[1], ref[1]))
        return out_err, grad_err

    a, b, c = run(False, "fp32"), run(True, "fp32"), run(True, "keep")
    assert all(d == torch.float32 for pair in a[2] for d in pair)
    assert all(d == torch.bfloat16 for pair in c[2] for d in pair), c[2]   # the three hops after the first stay in 16 bits
    (b_out, b_grad), (c_out, c_grad) = errors(b, a), errors(c, a)
    rec = {"out_err_fp32_policy": b_out, "out_err_keep": c_out, "out_ratio": c_out / b_out,
           "grad_err_fp32_policy": b_grad, "grad_err_keep": c_grad, "grad_ratio": c_grad / b_grad}
    print("\n[pointvoxel half] hop chain: %s" % json.dumps(rec))
    out_dir = os.environ.get("PCS_MEASURED_DIR", "")   # where a run keeps its measured records, if it keeps any
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "pointvoxel_half_measured.json"), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    assert c_out <= 2.0 * b_out and c_grad <= 2.0 * b_grad, rec
