"""Convolution geometries that no shipped model uses, on the HIP path (-m gpu): kernel volumes 2 .. 125 (K > 32 leaves the MFMA wave
kernels for conv_block, K > 64 leaves the wave scan of the weight-gradient split lookup), even kernels at stride 1 (up to 8 pairs per
row at K = 8), dilation, strides 3 and (2, 1, 2), the tensor-stride-2 level, negative coordinates, and maps in which output rows have
no pair at all. The case table is tests/geometry_cases.py.

Two scene families: the golden scene (expected values = outputs of the reference, tests/golden/geometry_golden.npz) and random
dense scene `random_scene(rng, 40000, 60, 3)` of test_hip_parity.py (38 811 voxels, 8 pairs per row at K = 125, and the same
scene shifted to negative coordinates; expected values = the oracle, which tests/test_oracle_pinning.py pins to the same fixture).

Which kernel a call reaches is asserted, not assumed: through the plan the library launches from (pcs_debug_conv_plan: family, waves,
column tiles), its shape queries (pcs_conv_h_applies, pcs_conv_x3_applies, pcs_conv_emits_bn_partials -- fields of the same plan)
and through call counters on the backend entries. Bounds are the suite's: 2e-5 of the tensor maximum for
fp32 against the oracle, close_half for 16-bit outputs, 40 half-ulps of the maximum under autocast (test_conv3d_under_autocast)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import geometry_cases as gc
from oracle import oracle as orc
from test_dense_parity import _HALF_TOL, _round_half, _ws_mode, close_half
from test_hip_parity import random_scene
from test_host_api import PLAN_EXTRAS, PLAN_ORDER, PLAN_STATS, conv_plan

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS, GEO = gc.load()
IDS = [c[0] for c in gc.CASES]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close32(a, b, what, rtol=2e-5):
    """fp32 bound of the suite (MFMA vs scalar summation order, relative to the tensor maximum); the figure is printed first."""
    a = a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-6) if b.size else 0.0
    print("geometry %s: %.3g" % (what, err))
    assert err <= rtol, (what, err)


# ---- scenes and maps ---------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene(which, tensor_stride=1):
    """(N, 4) int32 input coordinates of a scene family at a tensor stride."""
    key = (which, tensor_stride)
    if key not in _SCENES:
        if which == "golden":
            c = gc.input_coords(OPS, tensor_stride)
        elif which == "golden_neg":
            c = GEO["neg_coords"]
        elif which == "small":   # one batch, about 1500 of the 1728 cells of a 12^3 box: 6 row tiles at 288 rows, ~20 pairs per row at k3
            c = random_scene(np.random.default_rng(12), 3500, 12, 1)
        else:
            c = random_scene(np.random.default_rng(4), 40000, 60, 3)
            c[:, :3] *= tensor_stride   # a level at tensor stride s holds multiples of s
            if which.endswith("_neg"):
                c[:, :3] -= c[:, :3].max(axis=0, keepdims=True) // 2
        _SCENES[key] = np.ascontiguousarray(c, dtype=np.int32)
    return _SCENES[key]


class Case:
    pass


_CASES = {}


def build_case(which, name, table=gc.CASES):
    """The HIP output coordinates and kernel map of one case on one scene, each asserted bit-equal (order included) to the expected
    ones -- the reference's on the golden scenes, the oracle's on the random ones -- before anything is computed on them."""
    key = (which, name)
    if key in _CASES:
        return _CASES[key]
    from openpcseg_amd import functional as F
    _, ks, st, ts_, dil = gc.case(name, table)
    ks3, st3, ts3, dil3 = gc.tup3(ks), gc.tup3(st), gc.tup3(ts_), gc.tup3(dil)
    inc = scene(which, ts_)
    golden = which.startswith("golden")
    prefix = "neg_" if which == "golden_neg" else ""
    d_in = t(inc)
    c = Case()
    c.general_downsample = gc.is_strided(st) and not all(st3[k] in (1, ks3[k]) for k in range(3))
    if gc.is_strided(st):
        outc = GEO["%sds_%s" % (prefix, name)] if golden else orc.spdownsample(inc, st, ks, ts_)
        d_out = F.spdownsample(d_in, st, ks, ts_)
        assert d_out.dtype == torch.int32 and tuple(d_out.shape) == outc.shape and (d_out.cpu().numpy() == outc).all()
    else:
        outc, d_out = inc, d_in
    if golden:
        nbmaps, nbsizes = GEO["%skmap_%s_nbmaps" % (prefix, name)].astype(np.int64), GEO["%skmap_%s_nbsizes" % (prefix, name)]
    else:
        nbmaps, nbsizes = orc.build_kmap(inc, outc, ks, ts_, dil)
    entry = F.build_kernel_map(d_in, d_out, ks3, ts3, dil3)
    assert (entry[1].cpu().numpy() == nbsizes).all()
    assert (entry[0].cpu().numpy().astype(np.int64) == nbmaps).all()
    assert entry[2] == (inc.shape[0], outc.shape[0]) and entry.fwd.K == gc.volume(ks)
    c.entry, c.nbmaps, c.nbsizes, c.n_in, c.n_out, c.K = entry, nbmaps, nbsizes, inc.shape[0], outc.shape[0], gc.volume(ks)
    c.d_in, c.d_out, c.strided, c.ts3 = d_in, d_out, gc.is_strided(st), ts3
    c.ks, c.st, c.dil = ks, st, dil
    _CASES[key] = c
    return c


def check_rev(entry):
    """entry.rev holds the pair set of entry.fwd, (out_row, in_row), sorted by input row within each offset (test_kmap_golden)."""
    fwd, rev = entry.fwd, entry.rev
    assert rev.koff_host == fwd.koff_host and (rev.n_src, rev.n_dst) == (fwd.n_dst, fwd.n_src) and rev.K == fwd.K
    fp, rp = fwd.pairs.cpu().numpy(), rev.pairs.cpu().numpy()
    assert fp.shape == rp.shape
    for k in range(fwd.K):
        a, b = fwd.koff_host[k], fwd.koff_host[k + 1]
        f, r = fp[a:b], rp[a:b]
        assert (np.diff(r[:, 1]) > 0).all()
        order = np.argsort(f[:, 0], kind="stable")
        assert (f[order][:, [1, 0]] == r).all(), k


RULEBOOK_PARAMS = ([("golden", c[0]) for c in gc.CASES] + [("dense", c[0]) for c in gc.CASES] +
                   [("golden_neg", c[0]) for c in gc.NEG_CASES] + [("dense_neg", c[0]) for c in gc.NEG_CASES])


@pytest.mark.parametrize("which,name", RULEBOOK_PARAMS, ids=["%s-%s" % p for p in RULEBOOK_PARAMS])
def test_coordinates_and_rulebooks(hip, which, name):
    """F.spdownsample (fast branch: k3 s3, k2 s2; general branch ds_pack_general_kernel: k4 s2, k5 s2, k5 s3, k3 s(2,1,2), k3 s2)
    and F.build_kernel_map, bit-exact with order (build_case asserts it); the input-sorted map; and for odd, point-symmetric
    kernels at stride 1 (K = 125, 75, 15, dilated 27) the mirrored half-probe: entry._mirror is set and fwd.mirror() is the map a
    probe of the negated offsets builds."""
    table = gc.NEG_CASES if which.endswith("_neg") else gc.CASES
    c = build_case(which, name, table)
    _, ks, st, ts_, dil = gc.case(name, table)
    assert c.general_downsample == (name in ("k4s2", "k5s2", "k5s3", "k3s212", "k3s2_l2", "k3s2"))
    entry = c.entry
    symmetric = c.K % 2 == 1 and not c.strided
    assert bool(entry._mirror) == symmetric
    check_rev(entry)
    if symmetric:
        assert c.K >= 3 and torch.equal(entry._ctx[2].flip(0), -entry._ctx[2])
        built = hip.build_kmap(c.d_in, c.d_in, -entry._ctx[2])
        assert torch.equal(entry.rev.pairs, built.pairs) and torch.equal(entry.rev.koff, built.koff)
        assert entry.rev.koff_host == built.koff_host and torch.equal(entry.rev.nbsizes, built.nbsizes)
        assert (entry.rev.n_src, entry.rev.n_dst) == (built.n_src, built.n_dst)
        # and the half-probe itself against a full probe of the same offsets
        full = hip.build_kmap(c.d_in, c.d_in.clone(), entry._ctx[2])
        assert torch.equal(full.pairs, entry.fwd.pairs) and full.koff_host == entry.fwd.koff_host


# ---- fp32: conv_wave5 / conv_wave4 / conv_block ------------------------------------------------------------------------------------------
FP32_SHAPES = {(32, 32): "wave5", (64, 96): "wave5", (96, 128): "wave5", (16, 32): "wave4", (8, 16): "wave4", (5, 33): "block"}
# dgrad contracts over cout and writes cin columns: 32 -> 16 and 16 -> 8 have an odd count of 16-column tiles
DGRAD_FAMILY = {(32, 32): "wave5", (64, 96): "wave5", (96, 128): "wave5", (16, 32): "wave4", (8, 16): "wave4", (5, 33): "block"}


def fp32_family(lib, cin, cout, k):
    """Which of the three fused fp32 kernels pcs_conv_gather_gemm_f32 launches for a shape on aligned tensors: the plan's family (it
    does not depend on the tile height)."""
    return conv_plan(lib, "fp32", cin, cout, k, 128)["family"]


def operands(rng, c, cin, cout, transposed=False):
    n_src, n_dst = (c.n_out, c.n_in) if transposed else (c.n_in, c.n_out)
    x = rng.normal(size=(n_src, cin)).astype(np.float32)
    w = (rng.normal(size=(c.K, cin, cout)) / np.sqrt(cin * 8.0)).astype(np.float32)
    gy = rng.normal(size=(n_dst, cout)).astype(np.float32)
    return x, w, gy


@pytest.mark.parametrize("cin,cout", list(FP32_SHAPES), ids=["%dx%d" % s for s in FP32_SHAPES])
@pytest.mark.parametrize("name", IDS)
def test_fp32_forward_dgrad_wgrad(hip, name, cin, cout):
    """pcs_conv_gather_gemm_f32 forward and dgrad (the input-sorted map, transposed weights) at tile heights 64, 128 and the default
    pick, and pcs_conv_wgrad_f32, against the oracle; each launch repeated bit-identically. K > 32 must run conv_block whatever the
    channel counts (no tile order, no write-back extras, no BatchNorm partials, 128-row tiles); K <= 32 the family of the shape."""
    c = build_case("dense", name)
    lib, k = hip.lib, c.K
    want = "block" if k > 32 else FP32_SHAPES[(cin, cout)]
    assert fp32_family(lib, cin, cout, k) == want
    assert fp32_family(lib, cout, cin, k) == ("block" if k > 32 else DGRAD_FAMILY[(cin, cout)])
    if want != "wave5":
        assert hip.tile_rows(cin, cout, c.entry.fwd) == 128 and not lib.pcs_conv_emits_bn_partials(cin, cout, k, 256, 0)
    if k > 32:
        assert not lib.pcs_conv_emits_bn_partials(cin, cout, k, 128, 0) and not hip.conv_supports_addend(cin, cout, k, 0)
        assert not hip.conv_emits_stats(cin, cout, k, c.entry.fwd)
    rng = np.random.default_rng(k * 1000 + cin * 10 + cout)
    x, w, gy = operands(rng, c, cin, cout)
    ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out))
    ogx, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    dx, dw, dgy = t(x), t(w), t(gy)
    wt = hip.transpose_weights(dw)
    for tile in (64, 128, None):
        y = hip.conv_gather_gemm(dx, dw, c.entry.fwd, tile_rows=tile)
        close32(y, ref, "%s %dx%d fwd tile %s" % (name, cin, cout, tile))
        assert torch.equal(y, hip.conv_gather_gemm(dx, dw, c.entry.fwd, tile_rows=tile))
        gx = hip.conv_gather_gemm(dgy, wt, c.entry.rev, tile_rows=tile)
        close32(gx, ogx, "%s %dx%d dgrad tile %s" % (name, cin, cout, tile))
        assert torch.equal(gx, hip.conv_gather_gemm(dgy, wt, c.entry.rev, tile_rows=tile))
    gw = hip.conv_wgrad(dx, dgy, c.entry.fwd, 0)
    close32(gw, ogw, "%s %dx%d wgrad" % (name, cin, cout))
    assert torch.equal(gw, hip.conv_wgrad(dx, dgy, c.entry.fwd, 0))


@pytest.mark.parametrize("name", ["k2s1", "k442", "k4s1", "k4s2", "k553", "k5s1"])
def test_fp32_wgrad_three_plane_split(hip, name):
    """pcs_conv_wgrad_f32_bf16x3 (wgrad3 on three bf16 planes) at K = 8, 32, 64, 75, 125 on 96 x 96: K > 64 takes the serial split
    lookup. The fp32 bound, bit-reproducible, and not the fp32-MFMA kernel's bits."""
    c = build_case("dense", name)
    assert c.K in (8, 32, 64, 75, 125)
    rng = np.random.default_rng(c.K + 17)
    x, w, gy = operands(rng, c, 96, 96)
    _, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    dx, dgy = t(x), t(gy)
    gws = hip.conv_wgrad(dx, dgy, c.entry.fwd, 0, split=True)
    close32(gws, ogw, "%s 96x96 wgrad split" % name)
    assert torch.equal(gws, hip.conv_wgrad(dx, dgy, c.entry.fwd, 0, split=True))
    gw = hip.conv_wgrad(dx, dgy, c.entry.fwd, 0)
    close32(gw, ogw, "%s 96x96 wgrad" % name)
    assert not torch.equal(gw, gws)


# ---- 16-bit kernels ------------------------------------------------------------------------------------------------------------------------
def _interleave(hip, mode):
    f = hip.lib.pcs_debug_wgrad_interleave
    f.restype, f.argtypes = None, [ctypes.c_int32]
    f(mode)


def wgrad_h_all_orders(hip, fa, fb, kmap, a_col):
    """pcs_conv_wgrad_h under the default launch order and the forced orders 0, 1, 2 of the splits: one result, bit for bit."""
    try:
        outs = []
        for mode in (-1, 0, 1, 2):
            _interleave(hip, mode)
            outs.append(hip.conv_wgrad_h(fa, fb, kmap, a_col))
    finally:
        _interleave(hip, -1)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0]


HALF_SHAPES = [(64, 64), (96, 96), (128, 128), (384, 256)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", HALF_SHAPES, ids=["%dx%d" % s for s in HALF_SHAPES])
@pytest.mark.parametrize("name", ["k211", "k2s1", "k323", "k3d2", "k442"])
def test_half_forward_dgrad_wgrad(hip, dtype, name, cin, cout):
    """pcs_conv_gather_gemm_h forward and dgrad at K = 2, 8 (k2 at stride 1: up to 8 pairs per row, where the weight-stationary kernel
    picks its configuration for one pair per row), 18, dilated 27 and 32, under the default kernel choice and with conv_wave5h /
    conv_wave6h forced; pcs_conv_wgrad_h under every launch order. Against the oracle on the half-rounded operands."""
    c = build_case("dense", name)
    assert c.K in (2, 8, 18, 27, 32) and hip.conv_h_applies(cin, cout, c.K) and hip.conv_h_applies(cout, cin, c.K)
    assert hip.lib.pcs_conv_uses_tile_order(cin, cout, c.K, hip._HALF[dtype])
    rng = np.random.default_rng(c.K * 1000 + cin + cout + 7)
    x, w, gy = (_round_half(v, dtype) for v in operands(rng, c, cin, cout))
    ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out))
    ogx, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    dx, dgy = t(x).to(dtype), t(gy).to(dtype)
    wp = hip.prepare_weights_h(t(w), dtype, transpose=False)
    wpt = hip.prepare_weights_h(t(w), dtype, transpose=True)
    try:
        for mode in (-1, 0, 3):   # the shape policy's own pick, conv_wave5h, conv_wave6h wherever it has an instance
            _ws_mode(hip, mode)
            y = hip.conv_gather_gemm_h(dx, wp, c.K, cout, c.entry.fwd)
            assert y.dtype == dtype and tuple(y.shape) == (c.n_out, cout)
            close_half(y, ref, dtype)
            assert torch.equal(y, hip.conv_gather_gemm_h(dx, wp, c.K, cout, c.entry.fwd))
            close_half(hip.conv_gather_gemm_h(dx, wp, c.K, cout, c.entry.fwd, tile_rows=128, ordered="force"), ref, dtype)
            close_half(hip.conv_gather_gemm_h(dgy, wpt, c.K, cin, c.entry.rev), ogx, dtype)
    finally:
        _ws_mode(hip, -1)
    gw = wgrad_h_all_orders(hip, dx, dgy, c.entry.fwd, 0)
    assert gw.dtype == torch.float32
    close32(gw, ogw, "%s %dx%d %s wgrad_h" % (name, cin, cout, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("cin,cout", [(128, 128), (32, 32)], ids=["128x128", "32x32"])
@pytest.mark.parametrize("name", ["k4s1", "k4s2", "k553", "k5s1"])
def test_half_wgrad_large_kernel_volume(hip, dtype, name, cin, cout):
    """pcs_conv_wgrad_h at K = 64 (the last volume of the 64-lane split scan), 75 and 125 (the serial lookup, which ignores the
    launch order while the grid stays padded to 8 ceil(ns / 8) workgroups at the half default, order 2): 128 x 128 on wgrad3,
    32 x 32 on its thin one-wave instance. fp32 accumulation of exact products: the fp32 bound; every launch order the same bits."""
    c = build_case("dense", name)
    assert c.K in (64, 75, 125)
    rng = np.random.default_rng(c.K * 1000 + cin + 11)
    x, w, gy = (_round_half(v, dtype) for v in operands(rng, c, cin, cout))
    _, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    gw = wgrad_h_all_orders(hip, t(x).to(dtype), t(gy).to(dtype), c.entry.fwd, 0)
    close32(gw, ogw, "%s %dx%d %s wgrad_h" % (name, cin, cout, dtype))
    if c.strided:   # the transposed convolution's weight gradient: its input lives on the output rows (column 1)
        xt, _, gyt = (_round_half(v, dtype) for v in operands(rng, c, cin, cout, transposed=True))
        _, ogwt = orc.conv_bwd(xt, gyt, w, c.nbmaps, c.nbsizes, transposed=True)
        close32(wgrad_h_all_orders(hip, t(xt).to(dtype), t(gyt).to(dtype), c.entry.fwd, 1), ogwt, "%s transposed wgrad_h" % name)


@pytest.mark.parametrize("name", ["k2s1", "k323", "k442", "k3d2"])
def test_x3_forward_dgrad(hip, name):
    """pcs_conv_gather_gemm_f32_bf16x3 at K = 8 (stride 1), 18, 32 and dilated 27 on 96 x 96: the bound of
    test_conv_x3_forward_dense_map (2e-5 against the oracle, bit-reproducible, at most twice the fp32 MFMA kernel's error against
    float64), forward and dgrad."""
    c = build_case("dense", name)
    cin = cout = 96
    assert c.K in (8, 18, 32, 27) and hip.conv_x3_applies(cin, cout, c.K)
    rng = np.random.default_rng(c.K + 23)
    x, w, gy = operands(rng, c, cin, cout)
    dx, dw, dgy = t(x), t(w), t(gy)
    ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out))
    ogx, _ = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    wp = hip.prepare_weights_x3(dw, transpose=False)
    for tile in (None, 128):
        y = hip.conv_gather_gemm_x3(dx, wp, c.K, cout, c.entry.fwd, tile_rows=tile)
        close32(y, ref, "%s x3 fwd tile %s" % (name, tile))
        assert torch.equal(y, hip.conv_gather_gemm_x3(dx, wp, c.K, cout, c.entry.fwd, tile_rows=tile))
    gx = hip.conv_gather_gemm_x3(dgy, hip.prepare_weights_x3(dw, transpose=True), c.K, cin, c.entry.rev)
    close32(gx, ogx, "%s x3 dgrad" % name)
    pairs, koff = c.entry.fwd.pairs.long(), c.entry.fwd.koff_host
    y64 = torch.zeros(c.n_out, cout, dtype=torch.float64, device=DEV)
    x64, w64 = dx.double(), dw.double()
    for k in range(c.K):
        pk = pairs[koff[k]:koff[k + 1]]
        if pk.numel():
            y64.index_add_(0, pk[:, 1], x64[pk[:, 0]] @ w64[k])
    y32 = hip.conv_gather_gemm(dx, dw, c.entry.fwd)
    e3, e32 = float((y.double() - y64).abs().max()), float((y32.double() - y64).abs().max())
    assert e3 <= 2.0 * e32 + 1e-7 * float(y64.abs().max()), (e3, e32)


# ---- destination rows without a pair -----------------------------------------------------------------------------------------------------
def poison(n, c, dtype):
    """Fill and free a NaN tensor of the output's size: the allocator hands the block to the next torch.empty of that size."""
    p = torch.full((n, c), float("nan"), dtype=dtype, device=DEV)
    del p


def stats_match(hip, got, y, cout):
    assert len(got) == 1
    yd = y.double()
    assert float(got[0][-1]) == y.shape[0]
    assert torch.allclose(got[0][:cout], yd.sum(0), rtol=0, atol=1e-6 * float(yd.abs().sum(0).max()))
    assert torch.allclose(got[0][cout:2 * cout], (yd * yd).sum(0), rtol=1e-6)
    sums = hip.bn_stats(y.float())
    assert torch.allclose(hip.bn_finalize(got[0], float(y.shape[0]), 1e-5, 0.1, None, None),
                          hip.bn_finalize(sums, float(y.shape[0]), 1e-5, 0.1, None, None), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("direction", ["fwd", "rev"])
@pytest.mark.parametrize("name", ["k4s2", "k3s3"])
def test_rows_without_pairs(hip, name, direction):
    """k4 s2 and k3 s3 on the golden scene (the reference's own maps): 59 % / 43 % of the output rows have no pair, and in the
    transposed direction 35 % of the k3 s3 input rows (every voxel lies in some k4 window, so k4 s2 has none there: it runs all the
    same). The entries write into torch.empty, poisoned with NaN before each call. Every kernel family -- conv_wave5, conv_wave4,
    conv_block, the 16-bit kernels conv_wave5h / conv_wave6h, bf16x3 -- must leave exact zeros on those rows, exactly the bias with a
    bias, relu(bias) with relu=True, exactly the addend with an addend, and BatchNorm partials that are those of the result."""
    c = build_case("golden", name)
    transposed = direction == "rev"
    kmap = c.entry.rev if transposed else c.entry.fwd
    n_src, n_dst = (c.n_out, c.n_in) if transposed else (c.n_in, c.n_out)
    hit = np.zeros(n_dst, bool)
    hit[c.nbmaps[:, 0 if transposed else 1]] = True
    empty = t(~hit)
    frac = 1.0 - hit.mean()
    if (name, direction) == ("k4s2", "rev"):
        assert frac == 0.0
    else:
        assert frac >= 0.10, frac
    k = c.K
    fams = set()
    for cin, cout in ((32, 32), (16, 32), (5, 33), (64, 64), (96, 96)):
        rng = np.random.default_rng(k * 100 + cin + cout)
        x, w, _ = operands(rng, c, cin, cout, transposed)
        bias = (rng.normal(size=cout) + 0.25).astype(np.float32)
        add = rng.normal(size=(n_dst, cout)).astype(np.float32)
        ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out), transposed)
        assert ref.shape == (n_dst, cout) and not ref[~hit].any()
        dx, dw, dbias, dadd = t(x), t(w), t(bias), t(add)
        fam = fp32_family(hip.lib, cin, cout, k)
        fams.add(fam)
        for tile in ((64, 128, None) if cin < 64 else (None,)):
            poison(n_dst, cout, torch.float32)
            y = hip.conv_gather_gemm(dx, dw, kmap, tile_rows=tile)
            assert not bool(y[empty].any()) and bool(torch.isfinite(y).all())
            close32(y, ref, "%s %s %dx%d %s tile %s" % (name, direction, cin, cout, fam, tile))
            poison(n_dst, cout, torch.float32)
            got = []
            yb = hip.conv_gather_gemm(dx, dw, kmap, bias=dbias, tile_rows=tile, bn_sums=got)
            assert torch.equal(yb[empty], dbias.expand(int(empty.sum()), cout))
            close32(yb, ref + bias[None, :], "%s %s %dx%d bias" % (name, direction, cin, cout))
            emits = bool(hip.lib.pcs_conv_emits_bn_partials(cin, cout, k, tile or hip.tile_rows(cin, cout, kmap), 0))
            assert emits == (len(got) == 1)
            if got:
                stats_match(hip, got, yb, cout)
            if fam == "block":   # no write-back extras on the generic kernel: the callers fall back
                assert not hip.conv_supports_addend(cin, cout, k, 0)
                with pytest.raises(RuntimeError):
                    hip.conv_gather_gemm(dx, dw, kmap, bias=dbias, tile_rows=tile, relu=True)
                continue
            poison(n_dst, cout, torch.float32)
            yr = hip.conv_gather_gemm(dx, dw, kmap, bias=dbias, tile_rows=tile, relu=True)
            assert torch.equal(yr[empty], torch.relu(dbias).expand(int(empty.sum()), cout)) and torch.equal(yr, torch.relu(yb))
            poison(n_dst, cout, torch.float32)
            ya = hip.conv_gather_gemm(dx, dw, kmap, tile_rows=tile, addend=dadd)
            assert torch.equal(ya[empty], dadd[empty]) and torch.equal(ya, y + dadd)
        if k > 32 or cin < 64:
            continue
        # 16-bit kernels (K <= 32): conv_wave5h and conv_wave6h
        for dtype in (torch.bfloat16, torch.float16):
            assert hip.conv_h_applies(cin, cout, k)
            xh, wh = _round_half(x, dtype), _round_half(w, dtype)
            refh = orc.conv_fwd(xh, wh, c.nbmaps, c.nbsizes, (c.n_in, c.n_out), transposed)
            dxh, wp, addh = t(xh).to(dtype), hip.prepare_weights_h(t(wh), dtype, transpose=False), dadd.to(dtype)
            try:
                for mode in (0, 3):
                    _ws_mode(hip, mode)
                    poison(n_dst, cout, dtype)
                    yh = hip.conv_gather_gemm_h(dxh, wp, k, cout, kmap)
                    assert not bool(yh[empty].any())
                    close_half(yh, refh, dtype)
                    poison(n_dst, cout, dtype)
                    got = []
                    yhb = hip.conv_gather_gemm_h(dxh, wp, k, cout, kmap, bias=dbias, bn_sums=got)
                    assert torch.equal(yhb[empty], dbias.to(dtype).expand(int(empty.sum()), cout))
                    if got:
                        stats_match(hip, got, yhb, cout)
                    poison(n_dst, cout, dtype)
                    yhr = hip.conv_gather_gemm_h(dxh, wp, k, cout, kmap, bias=dbias, relu=True)
                    assert torch.equal(yhr[empty], torch.relu(dbias).to(dtype).expand(int(empty.sum()), cout))
                    poison(n_dst, cout, dtype)
                    yha = hip.conv_gather_gemm_h(dxh, wp, k, cout, kmap, addend=addh)
                    assert torch.equal(yha[empty], addh[empty])
            finally:
                _ws_mode(hip, -1)
        assert hip.conv_x3_applies(cin, cout, k)
        wp3 = hip.prepare_weights_x3(dw, transpose=False)
        poison(n_dst, cout, torch.float32)
        y3 = hip.conv_gather_gemm_x3(dx, wp3, k, cout, kmap)
        assert not bool(y3[empty].any())
        close32(y3, ref, "%s %s %dx%d x3" % (name, direction, cin, cout))
        poison(n_dst, cout, torch.float32)
        got = []
        y3b = hip.conv_gather_gemm_x3(dx, wp3, k, cout, kmap, bias=dbias, bn_sums=got)
        assert torch.equal(y3b[empty], dbias.expand(int(empty.sum()), cout))
        if got:
            stats_match(hip, got, y3b, cout)
    assert fams == ({"block"} if k > 32 else {"wave5", "wave4", "block"})


# ---- the boundaries the plan owns --------------------------------------------------------------------------------------------------------
# (entry, cin, cout, case of NEG_CASES on the small scene, [(tile_rows, family, waves, 16-column tiles per column tile, kc)])
PLAN_BOUNDARIES = [
    # 4-wave workgroups while two tiles fit a CU's LDS (conv_nw8): 128 columns 144 | 160, 96 columns 192 | 208, 64 columns 288 | 304;
    # fp32 128 -> 128 narrows to 64-column tiles from 176 rows on (conv5_nctt), which fit twice again
    ("fp32", 128, 128, "k3s1", [(144, "wave5", 4, 8, 0), (160, "wave5", 8, 8, 0), (176, "wave5", 4, 4, 0)]),
    ("bf16", 128, 128, "k3s1", [(144, "wave6h", 4, 8, 1), (160, "wave6h", 8, 8, 1)]),
    ("fp16", 128, 128, "k3s1", [(144, "wave6h", 4, 8, 1), (160, "wave6h", 8, 8, 1)]),
    ("fp32", 96, 96, "k3s1", [(192, "wave5", 4, 6, 0), (208, "wave5", 8, 6, 0)]),
    ("bf16", 96, 96, "k3s1", [(192, "wave6h", 4, 6, 1), (208, "wave6h", 8, 6, 1)]),
    ("x3", 96, 96, "k3s1", [(192, "wave5x", 4, 6, 0), (208, "wave5x", 8, 6, 0)]),
    ("fp32", 64, 64, "k3s1", [(288, "wave5", 4, 4, 0), (304, "wave5", 8, 4, 0)]),
    ("bf16", 64, 64, "k3s1", [(288, "wave6h", 4, 4, 1), (304, "wave6h", 8, 4, 1)]),
    ("x3", 64, 64, "k3s1", [(288, "wave5x", 4, 4, 0), (304, "wave5x", 8, 4, 0)]),
    # the chunked weight-stationary instances stop above 160 rows
    ("bf16", 256, 256, "k3s1", [(160, "wave6h", 8, 8, 2), (176, "wave5h", 8, 8, 0)]),
    # K <= 8 (one pair per row and offset): the weight-stationary kernel from 16 fragments per step on
    ("bf16", 96, 96, "k2s2", [(128, "wave6h", 4, 6, 1)]),
    ("bf16", 64, 64, "k2s2", [(128, "wave5h", 4, 4, 0)]),
    # 32 columns on 256 threads: 32 row groups, the statistics need 64 rows of scratch (48: the query says no, no partials come back)
    ("fp32", 32, 32, "k3s1", [(48, "wave5", 4, 2, 0), (64, "wave5", 4, 2, 0)]),
    ("bf16", 32, 32, "k3s1", [(48, "wave5h", 4, 2, 0), (64, "wave5h", 4, 2, 0)]),
    ("x3", 32, 32, "k3s1", [(48, "wave5x", 4, 2, 0), (64, "wave5x", 4, 2, 0)]),
]
_PLAN_REFS = {}


def plan_reference(c, name, cin, cout, half):
    """Operands (rounded to `half` where given) and the oracle's output for them, computed once per (map, shape, storage).
    The features are scaled by 0.2: operands() sizes the weights for ~8 pairs per row and this k3 map has ~20, and the last check of
    stats_match is absolute (1e-7 on the mean) while the write-back sums in fp32 about the tile's first row -- at worst an error of
    2^-24 n |x - pivot| in a column sum, 3.6e-4 sigma over these 1510 rows with a pivot 4 sigma out. At sigma = 0.32 that is 7.6e-8 on
    the mean: inside the bound for any pivot, not by the luck of the draw (at sigma = 1.6 a 176-row tile measured 1.3e-7)."""
    key = (name, cin, cout, half)
    if key not in _PLAN_REFS:
        rng = np.random.default_rng(c.K * 1000 + cin + cout)
        x, w, _ = operands(rng, c, cin, cout)
        x *= np.float32(0.2)
        add = rng.normal(size=(c.n_out, cout)).astype(np.float32)
        if half is not None:
            x, w, add = (_round_half(v, half) for v in (x, w, add))
        _PLAN_REFS[key] = (x, w, add, orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out)))
    return _PLAN_REFS[key]


@pytest.mark.parametrize("entry,cin,cout,name,heights", PLAN_BOUNDARIES,
                         ids=["%s-%dx%d-%s" % b[:4] for b in PLAN_BOUNDARIES])
def test_plan_boundaries(hip, entry, cin, cout, name, heights):
    """The three entries with tile_rows forced to both sides of every boundary conv_route owns, on a small dense cloud (about 1500
    voxels in a 12^3 box: the k3 map has ~20 pairs per row, so the heaviest-first order is launched; 6 row tiles at 288 rows) and its
    k2 stride-2 map. The family, wave count, column-tile width and contraction chunks are read from the plan of that very call
    (statistics + order + extras flags as the call carries them); the output, the BatchNorm sums of the write-back and the output
    with an addend are held to the file's bounds on every side."""
    c = build_case("small", name, gc.NEG_CASES)
    assert 1400 <= c.n_in <= 1600 and c.K == (27 if name == "k3s1" else 8)
    kmap, lib = c.entry.fwd, hip.lib
    ordered = hip._wants_order(kmap)
    if name == "k3s1":
        assert ordered and c.nbmaps.shape[0] > 6 * c.n_out and (c.n_out + 287) // 288 >= 5
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(entry)
    x, w, add, ref = plan_reference(c, name, cin, cout, half)
    dx, dw, dadd = t(x), t(w), t(add)
    if half is not None:
        dx, dadd, wp = dx.to(half), dadd.to(half), hip.prepare_weights_h(dw, half, transpose=False)
        run = lambda **kw: hip.conv_gather_gemm_h(dx, wp, c.K, cout, kmap, **kw)
    elif entry == "x3":
        wp = hip.prepare_weights_x3(dw, transpose=False)
        run = lambda **kw: hip.conv_gather_gemm_x3(dx, wp, c.K, cout, kmap, **kw)
    else:
        run = lambda **kw: hip.conv_gather_gemm(dx, dw, kmap, **kw)
    close = (lambda y, r, what: close_half(y, r, half)) if half is not None else close32
    for tile, family, waves, nctt, kc in heights:
        what = "%s %dx%d %s tile %d" % (entry, cin, cout, name, tile)
        flags = PLAN_ORDER if ordered else 0
        p = conv_plan(lib, entry, cin, cout, c.K, tile, flags | PLAN_STATS)
        assert (p["family"], p["waves"], p["nctt"], p["kc"]) == (family, waves, nctt, kc), (what, p)
        assert p["ncoltiles"] == -(-cout // (16 * nctt)) and p["reads_order"]
        assert p["emits_stats"] == (tile >= 64 or cout > 32), (what, p)
        got = []
        y = run(tile_rows=tile, bn_sums=got)
        assert len(got) == (1 if p["emits_stats"] else 0), what
        close(y, ref, what)
        if got:
            stats_match(hip, got, y, cout)
        assert torch.equal(y, run(tile_rows=tile)), what   # the statistics change nothing in the output; bit-reproducible
        if entry == "x3":
            assert not p["takes_extras"]
            continue
        pa = conv_plan(lib, entry, cin, cout, c.K, tile, flags | PLAN_EXTRAS)
        assert pa["takes_extras"] and (pa["family"], pa["waves"], pa["nctt"]) == (family, waves, nctt), (what, pa)
        ya = run(tile_rows=tile, addend=dadd)
        if half is None:
            assert torch.equal(ya, y + dadd), what
        else:
            close_half(ya, ref + add, half)


# ---- functional.conv3d: which backend entry ran, and what it returned ----------------------------------------------------------------------
ENTRIES = ("conv_gather_gemm", "conv_gather_gemm_h", "conv_gather_gemm_x3", "conv_wgrad", "conv_wgrad_h", "_tile_order")


@contextlib.contextmanager
def counted(hip):
    """`hip` as the process-wide backend with every convolution entry counted: seen[name] = [(args, kwargs), ...]."""
    from openpcseg_amd import native
    seen = {n: [] for n in ENTRIES}
    orig = {n: getattr(hip, n) for n in ENTRIES}

    def wrap(n):
        return lambda *a, **k: (seen[n].append((a, k)), orig[n](*a, **k))[1]
    prev = native._BACKEND
    for n in ENTRIES:
        setattr(hip, n, wrap(n))
    native._BACKEND = hip
    try:
        yield seen
    finally:
        native._BACKEND = prev
        for n in ENTRIES:
            delattr(hip, n)   # back to the class's methods


ENTRY_OF = {"fp32": "conv_gather_gemm", "half": "conv_gather_gemm_h", "x3": "conv_gather_gemm_x3"}


def test_conv3d_reaches_the_entry_the_route_names(hip, monkeypatch):
    """functional.conv3d, forward and dgrad, calls the backend entry functional._conv_family names for that direction (the dgrad with
    (cout, cin) swapped), once each, and an addend reaches the dgrad entry exactly when the runner reports that the kernel took it.
    K = 27 on the smallest submanifold geometry of the case table (k3d2_l2) and the strided / transposed pair k3s3; 4 -> 32 (thin:
    fp32 in every mode), 32 -> 32, 64 -> 64, 96 -> 96; fp32, bf16 autocast on bf16 features, the bf16x3 convolution policy; plain,
    with_skip, and act_slope = 0.1 where conv_act_fusable says so.
    CONDITION: over these cases each of the three entries must be the expected one at least once, forward and dgrad, and the
    addend must both ride and not ride; otherwise the test says nothing and fails as vacuous."""
    from openpcseg_amd import functional as F
    from openpcseg_amd.sparse import SparseTensor
    records = []
    run = F._run_conv

    def spy(be, fam, *a, **kw):
        res = run(be, fam, *a, **kw)
        records.append((fam, bool(kw.get("transpose", False)), bool(res[2])))
        return res
    monkeypatch.setattr(F, "_run_conv", spy)
    fwd_seen, dgrad_seen, rode = set(), set(), set()
    rng = np.random.default_rng(27)
    try:
        for name, transposed in (("k3d2_l2", False), ("k3s3", False), ("k3s3", True)):
            c = build_case("golden", name)
            assert c.K == 27
            for cin, cout in ((4, 32), (32, 32), (64, 64), (96, 96)):
                x, w, _ = operands(rng, c, cin, cout, transposed)
                for mode in ("fp32", "autocast_bf16", "conv_bf16x3"):
                    hd = torch.bfloat16 if mode == "autocast_bf16" else None
                    F.set_conv_policy("bf16x3" if mode == "conv_bf16x3" else "fp32")
                    for variant in ("plain", "with_skip", "act_slope"):
                        dx, dw = t(x).to(hd or torch.float32).requires_grad_(True), t(w).requires_grad_(True)
                        if transposed:   # the level and its map, as the encoder's strided convolution leaves them
                            fine = SparseTensor(torch.zeros(c.n_in, 4, device=DEV), c.d_in, c.ts3)
                            fine.cmaps[c.ts3] = c.d_in
                            down = F.conv3d(fine, torch.zeros(c.K, 4, 4, device=DEV), c.ks, stride=c.st, dilation=c.dil)
                            st = SparseTensor(dx, down.C, down.s)
                            st.cmaps, st.kmaps = down.cmaps, down.kmaps
                        else:
                            st = SparseTensor(dx, c.d_in, c.ts3)
                        del records[:]
                        with counted(hip) as seen, torch.autocast("cuda", dtype=torch.bfloat16, enabled=hd is not None):
                            kw = {}
                            if variant == "act_slope":
                                if not F.conv_act_fusable(dx, dw):
                                    continue
                                kw["act_slope"] = 0.1
                            fam_f = F._conv_family(hip, hd, True, cin, cout, 27)
                            fam_d = F._conv_family(hip, hd, True, cout, cin, 27)
                            if variant == "with_skip":
                                out, skip = F.conv3d(st, dw, c.ks, stride=c.st, dilation=c.dil, transposed=transposed, with_skip=True)
                                (out.F.float().sum() + torch.tanh(skip.F.float()).sum()).backward()
                            else:
                                F.conv3d(st, dw, c.ks, stride=c.st, dilation=c.dil, transposed=transposed, **kw).F.float().sum().backward()
                        what = (name, transposed, cin, cout, mode, variant)
                        (rf, tf, took_f), (rd, td, took) = records
                        assert (rf, tf, took_f, rd, td) == (fam_f, False, False, fam_d, True), (what, records)
                        calls = {n: len(seen[n]) for n in ENTRY_OF.values()}
                        want = {n: [ENTRY_OF[fam_f], ENTRY_OF[fam_d]].count(n) for n in ENTRY_OF.values()}
                        assert calls == want, (what, calls, want)
                        fwd_kw, dgrad_kw = seen[ENTRY_OF[fam_f]][0][1], seen[ENTRY_OF[fam_d]][-1][1]
                        assert fwd_kw.get("addend") is None and fwd_kw.get("act_slope") == kw.get("act_slope"), (what, fwd_kw)
                        assert (dgrad_kw.get("addend") is not None) == took and (variant == "with_skip" or not took), (what, took)
                        assert dx.grad is not None and dw.grad is not None
                        fwd_seen.add(fam_f)
                        dgrad_seen.add(fam_d)
                        if variant == "with_skip":
                            rode.add(took)
    finally:
        F.set_conv_policy("fp32")
    assert fwd_seen == dgrad_seen == set(ENTRY_OF) and rode == {True, False}, (fwd_seen, dgrad_seen, rode)   # the CONDITION above


def assert_fp32_entries_only(seen, k):
    """K > 32: the fp32 kernel served forward and dgrad -- no 16-bit, bf16x3 or tile-order call, and (K > 32 has none of them) no
    BatchNorm partials or write-back extras were asked of it."""
    assert len(seen["conv_gather_gemm"]) >= 1
    assert not seen["conv_gather_gemm_h"] and not seen["conv_gather_gemm_x3"] and not seen["_tile_order"] and not seen["conv_wgrad_h"]
    for a, kw in seen["conv_gather_gemm"]:
        assert a[1].shape[0] == k and a[0].dtype == torch.float32
        assert kw.get("addend") is None and kw.get("act_slope") is None and not kw.get("relu")


def run_conv3d(c, x, w, transposed, **kw):
    """functional.conv3d over the geometry of case `c` (its levels and maps are built by conv3d itself) -> output SparseTensor."""
    from openpcseg_amd import functional as F
    from openpcseg_amd.sparse import SparseTensor
    if not transposed:
        return F.conv3d(SparseTensor(x, c.d_in, c.ts3), w, c.ks, stride=c.st, dilation=c.dil, **kw)
    fine = SparseTensor(torch.zeros(c.n_in, 4, device=DEV), c.d_in, c.ts3)
    fine.cmaps[c.ts3] = c.d_in
    down = F.conv3d(fine, torch.zeros(c.K, 4, 4, device=DEV), c.ks, stride=c.st, dilation=c.dil)
    assert torch.equal(down.C, c.d_out)
    inp = SparseTensor(x, down.C, down.s)
    inp.cmaps, inp.kmaps = down.cmaps, down.kmaps
    return F.conv3d(inp, w, c.ks, stride=c.st, dilation=c.dil, transposed=True, **kw)


CONV_IDS = ["%s_%s" % (c[0], "T" if c[1] else "N") for c in gc.CONV_CASES]


@pytest.mark.parametrize("mode", ["fp32", "autocast_bf16", "wgrad_bf16x3", "conv_bf16x3"])
@pytest.mark.parametrize("name,transposed,cin,cout", gc.CONV_CASES, ids=CONV_IDS)
def test_conv3d_autograd_vs_reference_golden(hip, name, transposed, cin, cout, mode):
    """functional.conv3d (y, gx, gw) against the reference's ConvolutionFunction vectors, transposed included: fp32 at 2e-5; under
    bf16 autocast against the fp32 golden at the suite's autocast bound; and under the bf16x3 policies (which these thin layers do not
    meet: the fp32 kernels must serve them, at the fp32 bound). K > 32: the call counter shows the fp32 entry and nothing else."""
    from openpcseg_amd import functional as F
    c = build_case("golden", name)
    tag = "conv_%s_%s" % (name, "T" if transposed else "N")
    x = t(GEO[tag + "_x"]).requires_grad_(True)
    w = t(GEO[tag + "_w"]).requires_grad_(True)
    assert tuple(w.shape) == (c.K, cin, cout) and F.get_wgrad_policy() == "fp32" and F.get_conv_policy() == "fp32"
    amp = mode == "autocast_bf16"
    try:
        if mode == "wgrad_bf16x3":
            F.set_wgrad_policy("bf16x3")
        if mode == "conv_bf16x3":
            F.set_conv_policy("bf16x3")
        with counted(hip) as seen:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                out = run_conv3d(c, x, w, transposed)
            out.F.backward(t(GEO[tag + "_gy"]).to(out.F.dtype))
    finally:
        F.set_wgrad_policy("fp32")
        F.set_conv_policy("fp32")
    assert out.F.dtype == (torch.bfloat16 if amp else torch.float32) and x.grad.dtype == torch.float32 and w.grad.dtype == torch.float32
    # thin layers (4 .. 12 channels): the fp32 entries at every K; for K > 32 that is the claim under test
    assert_fp32_entries_only(seen, c.K)
    assert len(seen["conv_gather_gemm"]) >= 2 and len(seen["conv_wgrad"]) == 1 and not seen["conv_wgrad"][0][1].get("split")
    for got, key in ((out.F, "_y"), (x.grad, "_gx"), (w.grad, "_gw")):
        ref = GEO[tag + key]
        if amp:
            err = float((got.float().cpu() - torch.from_numpy(ref)).abs().max()) / float(np.abs(ref).max())
            print("geometry %s %s autocast: %.3g" % (tag, key, err))
            assert err <= 40 * _HALF_TOL[torch.bfloat16], (key, err)
        else:
            close32(got, ref, "%s %s %s" % (tag, key, mode))


@pytest.mark.parametrize("mode", ["fp32", "autocast_bf16", "autocast_fp16", "wgrad_bf16x3", "conv_bf16x3"])
@pytest.mark.parametrize("name,transposed", [("k5s1", False), ("k4s1", False), ("k4s2", False), ("k4s2", True), ("k2s1", False)],
                         ids=["k5s1", "k4s1", "k4s2_N", "k4s2_T", "k2s1"])
def test_conv3d_wide_layers_pick_their_entries(hip, name, transposed, mode):
    """functional.conv3d on 96 x 96 channels over the dense scene, against the oracle. K = 125 / 64: every mode lands on the fp32
    kernel for forward and dgrad (autocast rounds its output to the half dtype; the bf16x3 convolution policy does not apply), with
    no tile-order call; the bf16x3 weight-gradient policy does reach the three-plane split at K > 64. K = 8 at stride 1: autocast
    takes the 16-bit entries, the bf16x3 policy the split entry."""
    from openpcseg_amd import functional as F
    c = build_case("dense", name)
    cin = cout = 96
    rng = np.random.default_rng(c.K + 31)
    x, w, gy = operands(rng, c, cin, cout, transposed)
    amp = {"autocast_bf16": torch.bfloat16, "autocast_fp16": torch.float16}.get(mode)
    if amp is not None:
        x, w, gy = (_round_half(v, amp) for v in (x, w, gy))
    ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out), transposed)
    ogx, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes, transposed)
    dx, dw = t(x).requires_grad_(True), t(w).requires_grad_(True)
    try:
        if mode == "wgrad_bf16x3":
            F.set_wgrad_policy("bf16x3")
        if mode == "conv_bf16x3":
            F.set_conv_policy("bf16x3")
        with counted(hip) as seen:
            with torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
                out = run_conv3d(c, dx, dw, transposed)
            out.F.backward(t(gy).to(out.F.dtype))
    finally:
        F.set_wgrad_policy("fp32")
        F.set_conv_policy("fp32")
    if c.K > 32:
        assert not hip.conv_h_applies(cin, cout, c.K) and not hip.conv_x3_applies(cin, cout, c.K)
        assert_fp32_entries_only(seen, c.K)
        assert len(seen["conv_gather_gemm"]) == (3 if transposed else 2)   # (+ the level-building convolution of the transposed case)
        assert len(seen["conv_wgrad"]) == 1 and bool(seen["conv_wgrad"][0][1].get("split")) == (mode == "wgrad_bf16x3")
    elif amp is not None:
        assert len(seen["conv_gather_gemm_h"]) == 2 and len(seen["conv_wgrad_h"]) == 1 and not seen["conv_gather_gemm"]
    elif mode == "conv_bf16x3":
        assert len(seen["conv_gather_gemm_x3"]) == 2 and not seen["conv_gather_gemm"] and not seen["conv_gather_gemm_h"]
    else:
        assert len(seen["conv_gather_gemm"]) == 2 and not seen["conv_gather_gemm_x3"] and not seen["conv_gather_gemm_h"]
    if amp is None:
        assert out.F.dtype == torch.float32
        close32(out.F, ref, "%s conv3d y %s" % (name, mode))
        close32(dx.grad, ogx, "%s conv3d gx %s" % (name, mode))
    else:
        assert out.F.dtype == amp and dx.grad.dtype == torch.float32
        close_half(out.F, ref, amp)
        close_half(dx.grad.to(amp), ogx, amp)
    close32(dw.grad, ogw, "%s conv3d gw %s" % (name, mode))


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["k5s1", "k4s2", "k442"])
def test_conv3d_fusion_extras_fall_back_above_32_offsets(hip, name, amp):
    """What the fused blocks ask of conv3d -- BatchNorm statistics from the write-back (bn_stats), the skip gradient riding in the
    dgrad write-back (with_skip), LeakyReLU in the write-back (conv_act_fusable) -- at K = 125 and 64, where the kernel has none of
    them: no statistics are attached (the BatchNorm runs its own pass), no addend reaches the kernel, _SparseConv adds the skip
    gradient itself, and the gradients are those of the unfused graph and of the oracle. K = 32 (4, 4, 2) as the control: there the
    statistics are attached and the addend rides."""
    from openpcseg_amd import functional as F
    from openpcseg_amd.sparse import SparseTensor
    c = build_case("dense", name)
    cin = cout = 64
    rng = np.random.default_rng(c.K + 41)
    x, w, gy = operands(rng, c, cin, cout)
    gs = rng.normal(size=x.shape).astype(np.float32)
    if amp is not None:
        x, w, gy, gs = (_round_half(v, amp) for v in (x, w, gy, gs))
    ogx, ogw = orc.conv_bwd(x, gy, w, c.nbmaps, c.nbsizes)
    want_gx = ogx + gs * (1.0 - np.tanh(x.astype(np.float64)) ** 2)
    dw = t(w).requires_grad_(True)
    assert F.conv_act_fusable(t(x), dw) == (c.K <= 32)
    res = []
    for fused in (False, True):
        dx = t(x).requires_grad_(True)
        dw.grad = None
        with counted(hip) as seen:
            with torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
                st = SparseTensor(dx if amp is None else dx.to(amp), c.d_in, c.ts3)
                if fused:
                    out, skip = F.conv3d(st, dw, c.ks, stride=c.st, dilation=c.dil, bn_stats=True, with_skip=True)
                else:
                    out, skip = F.conv3d(st, dw, c.ks, stride=c.st, dilation=c.dil), st
                loss = (out.F.float() * t(gy)).sum() + (torch.tanh(skip.F.float()) * t(gs)).sum()
            loss.backward()
        if c.K > 32:
            assert_fp32_entries_only(seen, c.K)
            assert not hasattr(out, "bn_sums") and len(seen["conv_gather_gemm"]) == 2
        elif fused:
            assert hasattr(out, "bn_sums") == (amp is None or hip.conv_h_applies(cin, cout, c.K))
            last = (seen["conv_gather_gemm_h"] if amp is not None else seen["conv_gather_gemm"])[-1]
            assert last[1].get("addend") is not None   # the skip gradient rode in the dgrad launch
        res.append((dx.grad.clone(), dw.grad.clone()))
    (gx0, gw0), (gx1, gw1) = res
    tol = 1e-6 if amp is None else 2.0 ** -7
    assert float((gx1 - gx0).abs().max()) <= tol * float(gx0.abs().max())
    assert float((gw1 - gw0).abs().max()) <= 1e-6 * float(gw0.abs().max())
    close32(gw1, ogw, "%s fused extras gw" % name)
    if amp is None:
        close32(gx1, want_gx, "%s fused extras gx" % name)
    else:
        err = float((gx1.double().cpu() - torch.from_numpy(want_gx)).abs().max()) / float(np.abs(want_gx).max())
        assert err <= 40 * _HALF_TOL[amp], err


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout", [(32, 32), (96, 96), (5, 33)], ids=["32x32", "96x96", "5x33"])
def test_conv3d_inference_k5(hip, cin, cout, amp):
    """conv3d_inference on a k5 convolution + bias + ReLU (+ residual): K = 125 has no write-back epilogue, so the kernel adds the
    bias and torch adds / clamps -- no error, the same values as conv3d followed by the separate ops, and no epilogue flag reaches the
    fp32 entry. The prepared-weights dict is reused by a second call."""
    from openpcseg_amd import functional as F
    from openpcseg_amd.sparse import SparseTensor
    c = build_case("dense", "k5s1")
    rng = np.random.default_rng(cin + cout)
    x, w, _ = operands(rng, c, cin, cout)
    bias = t(rng.normal(size=cout).astype(np.float32))
    res = t(rng.normal(size=(c.n_out, cout)).astype(np.float32))
    dx, dw = t(x), t(w)
    assert not hip.conv_supports_addend(cin, cout, 125, 0)
    prepared = {}
    with counted(hip) as seen, torch.no_grad(), torch.autocast("cuda", dtype=amp or torch.bfloat16, enabled=amp is not None):
        plain = F.conv3d(SparseTensor(dx, c.d_in), dw, 5, bias=bias.to(amp) if amp is not None else bias)
        want_relu = torch.relu(plain.F)
        want_res = torch.relu(plain.F + res.to(plain.F.dtype))
        n0 = len(seen["conv_gather_gemm"])
        got_relu = F.conv3d_inference(SparseTensor(dx, c.d_in), dw, bias, 5, relu=True, prepared=prepared)
        got_res = F.conv3d_inference(SparseTensor(dx, c.d_in), dw, bias, 5, relu=True, addend=res, prepared=prepared)
        got_lin = F.conv3d_inference(SparseTensor(dx, c.d_in), dw, bias, 5, prepared=prepared)
    assert_fp32_entries_only(seen, 125)
    assert len(seen["conv_gather_gemm"]) == n0 + 3 and all(kw.get("bias") is not None for _, kw in seen["conv_gather_gemm"][n0:])
    assert torch.equal(got_relu.C, plain.C) and got_relu.F.dtype == plain.F.dtype
    tol = 1e-6 if amp is None else 2.0 * _HALF_TOL[amp]
    for got, want in ((got_relu.F, want_relu), (got_res.F, want_res), (got_lin.F, plain.F)):
        assert float((got.float() - want.float()).abs().max()) <= tol * float(want.float().abs().max())
    ref = orc.conv_fwd(x, w, c.nbmaps, c.nbsizes, (c.n_in, c.n_out)) + bias.cpu().numpy()[None, :]
    if amp is None:
        close32(got_lin.F, ref, "k5s1 %dx%d inference" % (cin, cout))
        assert float(got_relu.F.min()) == 0.0
