"""PCS_EP_POST_AFFINE at kernel level (-m gpu): the write-back order bias, activation, per-column affine map, addend, store of the
fused convolution (include/pcseg_hip.h, pcs_conv_epilogue) at each of its write-back sites:

    fp32  conv_os5 (ConvStoreF32)                      32 -> 32, 64 -> 96 (K = 27), 128 -> 128 (K = 8 strided / transposed)
    fp32  conv_os4 (ConvStoreF32)                      16 -> 32
    half  conv_os6h, 8-wide vector commit              64 -> 64, 128 -> 128 (K = 27), 128 -> 128 (K = 8 strided / transposed)
    half  conv_os6h, fall-back store (ConvStoreHalf)   64 -> 20 with the weight-stationary kernel forced on (cout % 8 != 0)
    half  conv_os5h (its inline lambda), TAIL          40 -> 56
    half  conv_os5h, straight instance                 256 -> 20, and 64 -> 64 with the weight-stationary kernel switched off

256 -> 20 of tests/test_dense_parity.py::HALF_CASES has no weight-stationary instance (2 column tiles x 8 steps), so it runs on
conv_os5h; the fall-back store of conv_os6h is reached by a shape it does serve whose width is no multiple of 8.
Maps: the k = 3 submanifold map and the k = 2 stride-2 map (forward and transposed) of ONE 20 000-point synthetic scan, each with
a tail tile. Exactness on operands whose every sum is exact in fp32; random data against the oracle's conv_fwd followed by the
same steps in float64 under the project's bounds (close 2e-5 for fp32, close_half for 16 bits)."""
import ctypes

import numpy as np
import pytest
import torch

from openpcseg_amd import functional as F
from openpcseg_amd import native
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
EP_POST = native.HipBackend.EP_POST_AFFINE
EINVAL, EUNSUPPORTED = -1, -4
CODE = {None: 0, torch.bfloat16: 1, torch.float16: 2}


def _dp():
    import test_dense_parity as dp
    return dp


def _inference_operands(*a):
    import test_inference_fold as tif
    return tif._operands(*a)


@pytest.fixture(scope="module")
def maps(hip):
    """{"sub" | "down" | "up": (HIP kernel map, oracle nbmaps, nbsizes, (n_in, n_out) as the oracle wants them, transposed, K,
    rows in, rows out)} of one 20 000-point scan; the rulebooks are asserted equal to the oracle's before use."""
    from openpcseg_amd.workloads.synthetic import make_batch
    dp = _dp()
    c = make_batch([0], n_points=20000)["lidar"].C.numpy()
    c1 = np.ascontiguousarray(c[np.argsort(orc.sphash(c), kind="stable")])
    c2 = orc.spdownsample(c1, 2, 2, 1)
    d1, d2 = dp.t(c1), dp.t(c2)
    sub = F.build_kernel_map(d1, d1, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    nbm, nbs = orc.build_kmap(c1, c1, 3, 1)
    assert np.array_equal(sub[1].cpu().numpy(), nbs) and np.array_equal(sub[0].cpu().numpy().astype(np.int64), nbm)
    down = F.build_kernel_map(d1, d2, (2, 2, 2), (1, 1, 1), (1, 1, 1))
    nbm2, nbs2 = orc.build_kmap(c1, c2, 2, 1)
    assert np.array_equal(down[1].cpu().numpy(), nbs2) and np.array_equal(down[0].cpu().numpy().astype(np.int64), nbm2)
    wide = F.build_kernel_map(d1, d1, (5, 3, 3), (1, 1, 1), (1, 1, 1))   # K = 45: the generic kernel, no write-back extras
    n1, n2 = c1.shape[0], c2.shape[0]
    return {"sub": (sub.fwd, nbm, nbs, (n1, n1), False, 27, n1, n1), "down": (down.fwd, nbm2, nbs2, (n1, n2), False, 8, n1, n2),
            "up": (down.rev, nbm2, nbs2, (n1, n2), True, 8, n2, n1), "wide": wide.fwd}


# (id, map, cin, cout, weight-stationary mode or None = the default policy)
F32_CASES = [("os5-32x32", "sub", 32, 32), ("os5-64x96", "sub", 64, 96), ("os4-16x32", "sub", 16, 32),
             ("os5-down-128x128", "down", 128, 128), ("os5-up-128x128", "up", 128, 128)]
HALF_SHAPES = [("os6h-vec-64x64", "sub", 64, 64, None), ("os6h-vec-128x128", "sub", 128, 128, None),
               ("os5h-256x20", "sub", 256, 20, None), ("os5h-tail-40x56", "sub", 40, 56, None),
               ("os6h-fallback-64x20", "sub", 64, 20, 3), ("os5h-64x64", "sub", 64, 64, 0),
               ("os6h-vec-down-128x128", "down", 128, 128, None), ("os6h-vec-up-128x128", "up", 128, 128, None)]
IDS = lambda cases: [c[0] for c in cases]


def test_shapes_come_from_the_dense_parity_cases():
    shapes = {(cin, cout) for _, cin, cout, _ in _dp().HALF_CASES}
    assert {(64, 64), (128, 128), (256, 20), (40, 56)} <= shapes


def _ws(hip, mode):
    f = hip.lib.pcs_debug_convh_ws
    f.restype, f.argtypes = None, [ctypes.c_int32] * 3
    f(-1 if mode is None else mode, 0, 0)


def _tail_tile(hip, km, cin, cout, code):
    t = hip.tile_rows(cin, cout, km, code)
    assert km.n_dst % t != 0, "the map needs a tail tile (%d rows, tiles of %d)" % (km.n_dst, t)
    return t


def _assert_site(hip, name, cin, cout, k, half):
    """The entry / kernel family the case is meant for."""
    lib = hip.lib
    if half:
        assert hip.conv_h_applies(cin, cout, k)
        assert ("tail" in name) == (cin % 32 != 0)
    else:
        assert lib.pcs_conv_supports_epilogue(cin, cout, k, 0) == 1
        assert lib.pcs_conv_uses_tile_order(cin, cout, k, 0) == (1 if name.startswith("os5") else 0)   # conv_os5 against conv_os4


def _seq(v, b, slope, relu, s, t, r):
    """bias, activation, affine map, addend -- torch, on the device, in the dtype of v."""
    v = v + b
    v = torch.relu(v) if relu else torch.where(v < 0, v * slope, v)
    v = v * s + t
    return v + r if r is not None else v


def _exact_operands(rng, n_in, n_out, k, cin, cout):
    dp = _dp()
    x = rng.integers(-2, 3, size=(n_in, cin)).astype(np.float32)
    w = rng.integers(-1, 2, size=(k, cin, cout)).astype(np.float32)
    b = rng.integers(-3, 4, size=cout).astype(np.float32)
    r = rng.integers(-4, 5, size=(n_out, cout)).astype(np.float32)
    s = rng.choice(np.array([0.5, 1.0, 2.0, -1.0], dtype=np.float32), size=cout)
    s[:4] = [0.5, 1.0, 2.0, -1.0]
    t = rng.integers(-3, 4, size=cout).astype(np.float32)
    return [dp.t(a) for a in (x, w, b, r, s, t)]


@pytest.mark.parametrize("name,mp,cin,cout", F32_CASES, ids=IDS(F32_CASES))
def test_fp32_one_launch_is_the_torch_sequence_exactly(hip, maps, name, mp, cin, cout):
    """Every sum exact in fp32: the one-launch result is torch.equal to the sequence applied to the plain kernel's output."""
    km, _, _, _, _, k, n_in, n_out = maps[mp]
    _assert_site(hip, name, cin, cout, k, False)
    _tail_tile(hip, km, cin, cout, 0)
    x, w, b, r, s, t = _exact_operands(np.random.default_rng(cin * 1000 + cout), n_in, n_out, k, cin, cout)
    plain = hip.conv_gather_gemm(x, w, km)
    assert float(plain.abs().max()) < 2 ** 23 and float(plain.min()) < 0
    for addend in (None, r):
        for relu in (False, True):
            y = hip.conv_gather_gemm(x, w, km, bias=b, addend=addend, act_slope=0.5, relu=relu, post_scale=s, post_shift=t)
            assert torch.equal(y, _seq(plain, b, 0.5, relu, s, t, addend)), (name, addend is not None, relu)
    # not the order of the call without the bit
    assert not torch.equal(y, torch.relu(plain + b + r) * s + t)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,mp,cin,cout,ws", HALF_SHAPES, ids=IDS(HALF_SHAPES))
def test_half_rounds_once_on_the_store(hip, maps, name, mp, cin, cout, ws, dtype):
    """Same exact operands: the half kernel's result is torch.equal to the fp32 kernel's post-affine result cast to the half dtype
    -- a second rounding (of the activation's or the affine map's result) would show wherever a value leaves the format."""
    km, _, _, _, _, k, n_in, n_out = maps[mp]
    _assert_site(hip, name, cin, cout, k, True)
    _tail_tile(hip, km, cin, cout, CODE[dtype])
    x, w, b, r, s, t = _exact_operands(np.random.default_rng(cin * 1000 + cout + 1), n_in, n_out, k, cin, cout)
    wp = hip.prepare_weights_h(w, dtype, transpose=False)
    xh, rh = x.to(dtype), r.to(dtype)
    assert torch.equal(xh.float(), x) and torch.equal(rh.float(), r)
    try:
        _ws(hip, ws)
        for addend, addend_h in ((None, None), (r, rh)):
            for relu in (False, True):
                want = hip.conv_gather_gemm(x, w, km, bias=b, addend=addend, act_slope=0.5, relu=relu, post_scale=s, post_shift=t)
                y = hip.conv_gather_gemm_h(xh, wp, k, cout, km, bias=b, addend=addend_h, act_slope=0.5, relu=relu, post_scale=s, post_shift=t)
                assert y.dtype == dtype and torch.equal(y, want.to(dtype)), (name, addend is not None, relu)
    finally:
        _ws(hip, None)


_ORACLE = {}


def _oracle_conv(key, x, w, nbm, nbs, sizes, transposed):
    if key not in _ORACLE:
        _ORACLE.clear()   # one entry: the variants of a case run back to back
        _ORACLE[key] = orc.conv_fwd(x, w, nbm, nbs, sizes, transposed=transposed).astype(np.float64)
    return _ORACLE[key]


def _random_case(hip, maps, name, mp, cin, cout, dtype, ws=None):
    dp = _dp()
    km, nbm, nbs, sizes, transposed, k, n_in, n_out = maps[mp]
    _assert_site(hip, name, cin, cout, k, dtype is not None)
    rng = np.random.default_rng(cin * 1000 + cout + 7 + CODE[dtype])
    x, w, b, add = _inference_operands(rng, n_in, n_out, k, cin, cout, dtype)
    s = (rng.uniform(0.5, 1.5, size=cout) * np.where(np.arange(cout) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    assert (s > 0).any() and (s < 0).any()
    t = (0.3 * rng.normal(size=cout)).astype(np.float32)
    conv = _oracle_conv((name, dtype), x, w, nbm, nbs, sizes, transposed)
    dx, dw, db, dadd, ds, dt_ = [dp.t(a) for a in (x, w, b, add, s, t)]
    if dtype is not None:
        wp, dx, dadd = hip.prepare_weights_h(dw, dtype, transpose=False), dx.to(dtype), dadd.to(dtype)
    try:
        _ws(hip, ws)
        for addend in (None, add):
            for relu in (False, True):
                kw = dict(bias=db, addend=None if addend is None else dadd, act_slope=0.01, relu=relu, post_scale=ds, post_shift=dt_)
                y = hip.conv_gather_gemm(dx, dw, km, **kw) if dtype is None else hip.conv_gather_gemm_h(dx, wp, k, cout, km, **kw)
                v = conv + b.astype(np.float64)
                v = np.maximum(v, 0.0) if relu else np.where(v < 0, v * np.float64(np.float32(0.01)), v)
                v = v * s.astype(np.float64) + t.astype(np.float64)
                if addend is not None:
                    v = v + add.astype(np.float64)
                if dtype is None:
                    assert y.dtype == torch.float32
                    dp.close(y, v, 2e-5)
                else:
                    assert y.dtype == dtype
                    dp.close_half(y, v, dtype)
    finally:
        _ws(hip, None)


@pytest.mark.parametrize("name,mp,cin,cout", F32_CASES, ids=IDS(F32_CASES))
def test_fp32_random_data_against_the_oracle(hip, maps, name, mp, cin, cout):
    _random_case(hip, maps, name, mp, cin, cout, None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,mp,cin,cout,ws", HALF_SHAPES, ids=IDS(HALF_SHAPES))
def test_half_random_data_against_the_oracle(hip, maps, name, mp, cin, cout, ws, dtype):
    _random_case(hip, maps, name, mp, cin, cout, dtype, ws)


def _raw(hip, x, w, km, cin, cout, k, ep, code=0, part=None, tile=None):
    """One call of the _ex entry with a caller-made pcs_conv_epilogue -> (return code, dst)."""
    t = tile or hip.tile_rows(cin, cout, km, code)
    seg = hip._segments(km, t)
    dst = torch.zeros((km.n_dst, cout), dtype=x.dtype, device="cuda")
    fn = hip.lib.pcs_conv_gather_gemm_h_ex if code else hip.lib.pcs_conv_gather_gemm_f32_ex
    rc = fn(native._ptr(x), x.shape[0], cin, native._ptr(w), k, cout, native._ptr(km._pairs_raw), 0, native._ptr(seg), t, km.n_dst, None,
            ctypes.byref(ep), native._ptr(dst), *((code,) if code else ()), native._ptr(part), None, native._stream())
    torch.cuda.synchronize()
    return rc, dst


def test_flag_clear_is_the_call_of_before_bit_for_bit(hip, maps):
    """The extended struct with the bit clear -- its trailing fields holding addresses nobody may read -- against
    hip.conv_gather_gemm(..., addend=, act_slope=): bias-less, addend, then LeakyReLU, on both entries."""
    km, _, _, _, _, k, n, _ = maps["sub"]
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(n, 64, device="cuda", generator=g)
    w = torch.randn(27, 64, 64, device="cuda", generator=g) / np.sqrt(64 * 27)
    add = torch.randn(n, 64, device="cuda", generator=g)
    for code, dtype in ((0, None), (1, torch.bfloat16)):
        xx, aa = (x, add) if dtype is None else (x.to(dtype), add.to(dtype))
        ww = w if dtype is None else hip.prepare_weights_h(w, dtype, transpose=False)
        want = hip.conv_gather_gemm(xx, ww, km, addend=aa, act_slope=0.1) if dtype is None else \
            hip.conv_gather_gemm_h(xx, ww, 27, 64, km, addend=aa, act_slope=0.1)
        ep = hip._Epilogue(aa.data_ptr(), 0.1, 0, 0x10, 0x14)
        rc, dst = _raw(hip, xx, ww, km, 64, 64, 27, ep, code)
        assert rc == 0 and torch.equal(dst, want)
    ep3 = hip._Epilogue(None, 0.0, native.HipBackend.EP_RELU)   # positional three-argument construction keeps working
    assert ep3.post_scale is None and ep3.post_shift is None and ctypes.sizeof(ep3) == 32
    assert hip.lib.pcs_abi_version() == 12


def test_abi_rejections(hip, maps):
    """Bit 16 with a null scale, with a misaligned pointer and together with bn_partial: PCS_EINVAL on both _ex entries; a generic
    shape (K > 32): PCS_EUNSUPPORTED; bits 2, 4, 8 and 32 stay PCS_EINVAL."""
    km, _, _, _, _, k, n, _ = maps["sub"]
    g = torch.Generator(device="cuda").manual_seed(10)
    x = torch.randn(n, 64, device="cuda", generator=g)
    w = torch.randn(27, 64, 64, device="cuda", generator=g) / np.sqrt(64 * 27)
    s = torch.ones(64 + 4, device="cuda")
    t = torch.zeros(64 + 4, device="cuda")
    assert s.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    for code, dtype in ((0, None), (1, torch.bfloat16), (2, torch.float16)):
        xx = x if dtype is None else x.to(dtype)
        ww = w if dtype is None else hip.prepare_weights_h(w, dtype, transpose=False)
        tile = hip.tile_rows(64, 64, km, code)
        assert hip.lib.pcs_conv_emits_bn_partials(64, 64, 27, tile, code) == 1
        part = torch.zeros(((n + tile - 1) // tile) * 2 * 64, dtype=torch.float64, device="cuda")
        E = lambda flags, ps, pt: hip._Epilogue(None, 0.01, flags, ps, pt)
        ok = E(EP_POST, s.data_ptr(), t.data_ptr())
        rc, dst = _raw(hip, xx, ww, km, 64, 64, 27, ok, code)
        # scale 1, shift 0, no addend: the LeakyReLU call of before
        leaky = hip.conv_gather_gemm(xx, ww, km, act_slope=0.01) if dtype is None else hip.conv_gather_gemm_h(xx, ww, 27, 64, km, act_slope=0.01)
        assert rc == 0 and torch.equal(dst, leaky) and float(leaky.float().min()) < 0
        for bad in (E(EP_POST, None, t.data_ptr()), E(EP_POST, s.data_ptr(), None), E(EP_POST, None, None),
                    E(EP_POST, s.data_ptr() + 4, t.data_ptr()), E(EP_POST, s.data_ptr(), t.data_ptr() + 8),
                    E(EP_POST | 2, s.data_ptr(), t.data_ptr()), E(EP_POST | 4, s.data_ptr(), t.data_ptr()),
                    E(EP_POST | 8, s.data_ptr(), t.data_ptr()), E(32, s.data_ptr(), t.data_ptr()), E(2, None, None)):
            assert _raw(hip, xx, ww, km, 64, 64, 27, bad, code)[0] == EINVAL, (code, bad.flags)
        assert _raw(hip, xx, ww, km, 64, 64, 27, ok, code, part=part)[0] == EINVAL          # not together with bn_partial
        assert _raw(hip, xx, ww, km, 64, 64, 27, E(0, None, None), code, part=part)[0] == 0   # the partials alone are fine
    wide = maps["wide"]
    assert wide.K == 45
    w45 = torch.randn(45, 64, 64, device="cuda", generator=g) / np.sqrt(64 * 45)
    ok = hip._Epilogue(None, 0.01, EP_POST, s.data_ptr(), t.data_ptr())
    assert hip.lib.pcs_conv_supports_epilogue(64, 64, 45, 0) == 0
    assert _raw(hip, x, w45, wide, 64, 64, 45, ok, 0, tile=128)[0] == EUNSUPPORTED
    assert _raw(hip, x.to(torch.bfloat16), w45, wide, 64, 64, 45, ok, 1, tile=128)[0] == EUNSUPPORTED
    with pytest.raises(ValueError):
        hip.conv_gather_gemm(x, w, km, post_scale=s[:64])
    with pytest.raises(ValueError):
        hip.conv_gather_gemm(x, w, km, post_scale=s[:32], post_shift=t[:32])


@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_conv3d_inference_is_one_launch(hip, maps, monkeypatch, dtype):
    """functional.conv3d_inference with act_slope / post_scale / post_shift / addend: ONE backend call where the shape's kernel
    takes the mode (64 -> 64: the half entry under autocast, 16 -> 32: the fp32 kernel, rounded afterwards), and the torch steps
    behind the kernel -- the same values within the output format -- where the bf16x3 policy leaves no epilogue."""
    from openpcseg_amd.sparse import SparseTensor
    dp = _dp()
    km, _, _, _, _, k, n, _ = maps["sub"]
    be = native.backend()
    counts = {"conv_gather_gemm": 0, "conv_gather_gemm_h": 0, "conv_gather_gemm_x3": 0}
    for nme in counts:
        orig = getattr(be, nme)

        def wrapped(*a, _o=orig, _n=nme, **kw):
            counts[_n] += 1
            return _o(*a, **kw)
        monkeypatch.setattr(be, nme, wrapped, raising=False)
    coords = None
    for cin, cout in ((64, 64), (16, 32)):
        rng = np.random.default_rng(cin + cout)
        x, w, b, add = _inference_operands(rng, n, n, 27, cin, cout, dtype)
        s = (rng.uniform(0.5, 1.5, size=cout) * np.where(np.arange(cout) % 2 == 0, 1.0, -1.0)).astype(np.float32)
        t = (0.3 * rng.normal(size=cout)).astype(np.float32)
        dx, dw, db, dadd, ds, dt_ = [dp.t(a) for a in (x, w, b, add, s, t)]
        if dtype is not None:
            dx, dadd = dx.to(dtype), dadd.to(dtype)
        if coords is None:
            from openpcseg_amd.workloads.synthetic import make_batch
            c = make_batch([0], n_points=20000)["lidar"].C.numpy()
            coords = dp.t(np.ascontiguousarray(c[np.argsort(orc.sphash(c), kind="stable")]))

        def run():
            xs = SparseTensor(dx, coords, 1)
            with torch.no_grad(), torch.autocast("cuda", dtype=dtype or torch.bfloat16, enabled=dtype is not None):
                return F.conv3d_inference(xs, dw, db, 3, addend=dadd, act_slope=0.01, post_scale=ds, post_shift=dt_).F
        before = dict(counts)
        y = run()
        assert sum(counts.values()) - sum(before.values()) == 1
        half = dtype is not None and be.conv_h_applies(cin, cout, 27)
        assert counts["conv_gather_gemm_h"] - before["conv_gather_gemm_h"] == (1 if half else 0)
        assert y.dtype == (dtype or torch.float32)
        if dtype is None and cin == 64:
            F.set_conv_policy("bf16x3")
            try:
                before = dict(counts)
                y3 = run()
                assert counts["conv_gather_gemm_x3"] - before["conv_gather_gemm_x3"] == 1
            finally:
                F.set_conv_policy("fp32")
            dp.close(y3, y.cpu().numpy(), 2e-5)
