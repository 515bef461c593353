"""The fused BatchNorm kernels (csrc/norm.hip) against the float64 reference of tests/bn_reference.py, every pass in
isolation: the test chooses stat, sums2 and count and feeds them in, so one pass's error is never forgiven by another's.

  exact cases   small-integer data for which every intermediate and result is representable in fp32, bf16 and fp16: the
                kernels must EQUAL the reference, on both vector paths, across the launch geometry (lanes tx = min(c / V, 64),
                TY = 256 / tx rows per workgroup, 1024 workgroups in the statistics passes, min(ceil(n / 4 TY), 2048) in the
                apply passes, row loops unrolled by 4)
  real cases    random normal data, per-element bounds derived in bn_reference's docstring
  SyncBN        the arithmetic of a sharded run on one device; empty and single-row tensors; the fp16 ReLU gate; the three
                statistics producers under |mean| >> std and an outlying pivot row

The first tests need no GPU: they pin the reference itself against torch.nn.functional.batch_norm in float64."""
import numpy as np
import pytest
import torch

import bn_reference as R

# No module-level pytestmark: the reference-pinning tests below must run under -m "not gpu". Every test that touches the
# device therefore carries @gpu itself -- a new GPU test without it would run, and fail, on a machine without one.
gpu = pytest.mark.gpu
DT = ["fp32", "bf16", "fp16"]
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
EPS, MOM = 1e-5, 0.1
PCS_EINVAL, PCS_EUNSUPPORTED = -1, -4


# ---- the reference, pinned on the CPU -----------------------------------------------------------------------------------
def _close64(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(b).max()) if b.size else 1.0)), what


@pytest.mark.parametrize("n,c", [(2, 3), (37, 20), (300, 32)])
@pytest.mark.parametrize("relu,with_res", [(True, True), (False, False)])
def test_reference_equals_torch_batch_norm_in_float64(n, c, relu, with_res):
    rng = np.random.default_rng(n + c)
    x, dy, res = (rng.normal(size=(n, c)) * 1.7 + 0.3, rng.normal(size=(n, c)), rng.normal(size=(n, c)))
    w, b = rng.uniform(0.5, 1.5, size=c) * rng.choice([-1.0, 1.0], size=c), rng.uniform(-0.5, 0.5, size=c)
    xt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
    rt = torch.from_numpy(res).requires_grad_(True)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    y = torch.nn.functional.batch_norm(xt, rm, rv, wt, bt, True, MOM, EPS)
    if with_res:
        y = y + rt
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(dy))

    s = R.sums(x)
    assert s[2 * c] == n
    stat, rm64, rv64 = R.finalize(s, n, EPS, MOM, np.zeros(c), np.ones(c))
    y64 = R.apply(x, stat, w, b, res if with_res else None, relu)
    gate = y64 if relu else None
    s2 = R.bwd_stats(dy, x, stat, gate)
    dx, dres = R.bwd_apply(dy, x, stat, s2, n, w, gate)
    _close64(y64, y.detach().numpy(), "y")
    _close64(rm64, rm.numpy(), "running_mean")
    _close64(rv64, rv.numpy(), "running_var")
    _close64(dx, xt.grad.numpy(), "dx")
    _close64(s2[c:], wt.grad.numpy(), "dw")
    _close64(s2[:c], bt.grad.numpy(), "db")
    if with_res:
        _close64(dres, rt.grad.numpy(), "dres")


@pytest.mark.parametrize("n,c", [(2, 3), (37, 20), (300, 32)])
def test_reference_leaky_relu_input_equals_autograd(n, c):
    """bwd_apply(in_slope) is the gradient of the PRE-activation of leaky_relu -> batch_norm -> relu."""
    rng = np.random.default_rng(7 * n + c)
    pre, dy = rng.normal(size=(n, c)) * 1.7 + 0.3, rng.normal(size=(n, c))
    w, b, slope = rng.uniform(0.5, 1.5, size=c), rng.uniform(-0.5, 0.5, size=c), 0.1
    pt, wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (pre, w, b))
    y = torch.relu(torch.nn.functional.batch_norm(torch.nn.functional.leaky_relu(pt, slope), None, None, wt, bt, True, MOM, EPS))
    y.backward(torch.from_numpy(dy))
    x = np.where(pre > 0, pre, slope * pre)
    stat, _, _ = R.finalize(R.sums(x), n, EPS)
    y64 = R.apply(x, stat, w, b, None, True)
    s2 = R.bwd_stats(dy, x, stat, y64)
    dx, _ = R.bwd_apply(dy, x, stat, s2, n, w, y64, in_slope=slope)
    _close64(y64, y.detach().numpy(), "y")
    _close64(dx, pt.grad.numpy(), "dx")
    _close64(s2[c:], wt.grad.numpy(), "dw")


def test_reference_helpers_on_the_cpu():
    """Mask packing round-trips; finalize's count guards; the exact cases are exactly representable in every storage type; with
    continuous data the share of elements whose ReLU gate is undecided at the bound is around 1e-6, far below the 0.1 % allowed."""
    rng = np.random.default_rng(0)
    y = rng.normal(size=(9, 96))
    words = R.mask_words(y)
    assert words.shape == (9, 3) and words.dtype == np.int32 and np.array_equal(R.mask_bits(words, 96), y > 0)
    assert int(R.mask_words(np.eye(1, 32, 31))[0, 0]) == -2 ** 31 and int(R.mask_words(np.eye(1, 32, 0))[0, 0]) == 1
    stat, rm, rv = R.finalize(np.array([3.0, 9.0, 1.0]), 1, EPS, MOM, np.zeros(1), np.ones(1))   # one row: biased variance
    assert stat[0] == 3.0 and stat[1] == 1.0 / np.sqrt(EPS) and rv[0] == 0.9
    stat, _, _ = R.finalize(np.zeros(3), 0, EPS)                                                # count 0 is read as 1
    assert stat[0] == 0.0 and np.isfinite(stat).all()
    for n, c in [(37, 20), (1000, 409)]:
        for name in DT:
            _exact_references(_exact_case(n, c), name)
    for name in DT:
        k = _real_case(20000, 32, name, 1)
        assert R.unsure(k["x"], k["stat"], k["w"], k["b"], k["res"], name).mean() <= 1e-4


# ---- helpers ------------------------------------------------------------------------------------------------------------
def dev(a, name="fp32"):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(R.torch_dtype(name)).cuda()


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def devmask(y64):
    return torch.from_numpy(R.mask_words(y64)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def same(t, ref64, name, what):
    """Bit for bit: ref64 is representable in the storage type (asserted by the caller), so equality there is equality."""
    assert torch.equal(t, dev(ref64, name)), what


RATIOS = {}


def within(got, ref64, bound, key, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref64)
    ratio = float(np.max(np.divide(err, bound, out=np.where(err > 0, np.inf, 0.0), where=bound > 0))) if err.size else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print("[bn] %-22s %-28s worst error / bound = %.4f (so far %.4f)" % ("%s %s" % key, what, ratio, RATIOS[key]))
    assert (err <= bound).all(), (key, what, ratio)


def _exact_case(n, c):
    """|x| <= 8, |dy|, |res| <= 4, mean in {-1, 0, 1}, invstd 0.5, w in {1, 2, -1}, b in {-1, 0, 0.5, 1}; sums2 for count = 2:
    sums2[:c] / 2 a multiple of 0.5, sums2[c:] / 2 in {-1, 0, 1}."""
    rng = np.random.default_rng(131 * c + n)

    def ints(lo, hi, shape):
        return rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    return dict(n=n, c=c, x=ints(-8, 8, (n, c)), dy=ints(-4, 4, (n, c)), res=ints(-4, 4, (n, c)),
                stat=np.concatenate([rng.choice([-1.0, 0.0, 1.0], size=c), np.full(c, 0.5)]),
                w=rng.choice([1.0, 2.0, -1.0], size=c), b=rng.choice([-1.0, 0.0, 0.5, 1.0], size=c),
                s2=np.concatenate([ints(-4, 4, c), 2.0 * rng.choice([-1.0, 0.0, 1.0], size=c)]))


def _exact_references(k, name, stats=True):
    """The float64 results of the exact case; asserts (a condition on the INPUTS) that all of them survive `name` unchanged."""
    x, dy, res, stat, w, b, s2 = (k[a] for a in ("x", "dy", "res", "stat", "w", "b", "s2"))
    r = {}
    r["y"] = R.apply(x, stat, w, b, res, True)
    r["y_plain"] = R.apply(x, stat)
    r["dx"], r["dres"] = R.bwd_apply(dy, x, stat, s2, 2, w, r["y"])
    r["dx_slope"], _ = R.bwd_apply(dy, x, stat, s2, 2, w, r["y"], in_slope=0.5)
    r["dx_plain"], _ = R.bwd_apply(dy, x, stat, s2, 2)
    for a in ("x", "dy", "res"):
        R.assert_representable(k[a], name, a)
    for a, v in r.items():
        R.assert_representable(v, name, a)
    if stats:
        r["sums"] = R.sums(x)
        r["sums2"] = R.bwd_stats(dy, x, stat, r["y"])
        r["sums2_plain"] = R.bwd_stats(dy, x, stat)
        for a in ("sums2", "sums2_plain"):
            R.assert_representable(r[a], "fp32", a)   # the fp32 copy of the backward sums must equal them too
    return r


def _params(k):
    return dev64(k["stat"]), dev(k["w"]), dev(k["b"]), dev64(k["s2"])


def _exact_apply(hip, n, c, names=DT, plain=True):
    k = _exact_case(n, c)
    stat, w, b, s2 = _params(k)
    for name in names:
        r = _exact_references(k, name, stats=False)
        x, dy, res, yg = dev(k["x"], name), dev(k["dy"], name), dev(k["res"], name), dev(r["y"], name)
        tag = "n=%d c=%d %s" % (n, c, name)
        same(hip.bn_apply(x, res, stat, w, b, True), r["y"], name, tag + " y")
        dx, dres = hip.bn_bwd_apply(dy, x, yg, stat, s2, 2.0, w, True, True)
        same(dx, r["dx"], name, tag + " dx")
        same(dres, r["dres"], name, tag + " dres")
        dxs, none = hip.bn_bwd_apply(dy, x, yg, stat, s2, 2.0, w, True, False, in_slope=0.5)
        assert none is None
        same(dxs, r["dx_slope"], name, tag + " dx (in_slope)")
        if c % 32 == 0:
            y, mask = hip.bn_apply(x, res, stat, w, b, True, want_mask=True)
            same(y, r["y"], name, tag + " y (mask launch)")
            assert torch.equal(mask, devmask(r["y"])), tag + " mask words"
            for got, ref in zip(hip.bn_bwd_apply(dy, x, mask, stat, s2, 2.0, w, True, True), (dx, dres)):
                assert torch.equal(got, ref), tag + " backward apply from the mask"
            assert torch.equal(hip.bn_bwd_apply(dy, x, mask, stat, s2, 2.0, w, True, False, in_slope=0.5)[0], dxs), tag
        if plain:
            same(hip.bn_apply(x, None, stat, None, None, False), r["y_plain"], name, tag + " y (plain)")
            same(hip.bn_bwd_apply(dy, x, None, stat, s2, 2.0, None, False, False)[0], r["dx_plain"], name, tag + " dx (plain)")


def _exact_stats(hip, n, c, names=DT):
    k = _exact_case(n, c)
    stat = dev64(k["stat"])
    for name in names:
        r = _exact_references(k, name)
        x, dy, yg = dev(k["x"], name), dev(k["dy"], name), dev(r["y"], name)
        tag = "n=%d c=%d %s" % (n, c, name)
        assert np.array_equal(host(hip.bn_stats(x)), r["sums"]), tag + " sums"
        s2 = hip.bn_bwd_stats(dy, x, yg, stat, True)
        assert np.array_equal(host(s2), r["sums2"]), tag + " sums2"
        assert s2._pcs_f32.dtype == torch.float32 and np.array_equal(host(s2._pcs_f32), r["sums2"]), tag + " sums2 in fp32"
        if c % 32 == 0:
            assert torch.equal(hip.bn_bwd_stats(dy, x, devmask(r["y"]), stat, True), s2), tag + " sums2 from the mask"
        assert np.array_equal(host(hip.bn_bwd_stats(dy, x, None, stat, False)), r["sums2_plain"]), tag + " sums2 (no ReLU)"


# ---- 2. exact cases -----------------------------------------------------------------------------------------------------
C_V4 = [4, 20, 32, 64, 96, 204, 256, 260, 288, 384]
C_V1 = [1, 3, 5, 65, 409]


@gpu
@pytest.mark.parametrize("c", C_V4 + C_V1)
def test_exact_every_channel_class(hip, c):
    """Each lane geometry (tx = c / V up to 64, partial second passes of the channel loop at 260 / 288 / 409, the scalar path)
    at one row, a row count that is no multiple of anything, and several trips of every row loop."""
    for n in (1, 37, 1000):
        _exact_apply(hip, n, c)
        _exact_stats(hip, n, c)


@gpu
@pytest.mark.parametrize("c,n", [(c, n) for c in (256, 409) for n in (1, 2, 3, 4, 5, 4095, 4096, 4097, 16384, 16385, 20481)] +
                         [(32, n) for n in (31, 32, 33, 32767, 32769)] + [(1, 255), (1, 257)])
def test_exact_statistics_across_the_sweep(hip, c, n):
    """One sweep of the 1024 workgroups is 1024 * TY rows (4096 at c = 256 / 409, 32 768 at c = 32, 262 144 at c = 1): row
    counts on either side of one sweep, of the four-sweep unroll and of its remainder."""
    _exact_stats(hip, n, c)


@gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 32767, 32768, 32769, 40961])
def test_exact_apply_across_the_grid(hip, n):
    """c = 256: TY = 4, a workgroup's unrolled trip is 16 rows, the grid stops growing at 2048 workgroups = 32 768 rows;
    40 961 rows give a fifth trip (the remainder loop)."""
    _exact_apply(hip, n, 256, plain=n < 5000)


@gpu
def test_exact_apply_at_the_grid_cap_of_the_narrowest_tensor(hip):
    """c = 4: TY = 256, the 2048-workgroup cap is reached at 2 097 152 rows; one more."""
    _exact_apply(hip, 2097153, 4, plain=False)


def _raw_apply(hip, name, x, res, stat, w, b, n, c, relu, y, mask, ldy, tail, ctail):
    from openpcseg_amd import native
    p = native._ptr
    head = [p(x), p(res), p(stat), p(w), p(b), n, c, int(relu)]
    rest = [p(y), p(mask), ldy, p(tail), ctail, native._stream()]
    if name == "fp32":
        return hip.lib.pcs_bn_apply_f32(*head, *rest)
    return hip.lib.pcs_bn_apply_h(*head, CODE[name], *rest)


def _raw_bwd_stats(hip, name, dy, x, y, mask, stat, n, c, relu, lddy):
    from openpcseg_amd import native
    p = native._ptr
    ws = torch.empty(hip.lib.pcs_bn_num_partials() * 2 * c, dtype=torch.float32, device="cuda")
    buf = torch.empty(3 * c, dtype=torch.float64, device="cuda")
    head = [p(dy), p(x), p(y), p(mask), p(stat), n, c, int(relu)]
    rest = [p(ws), p(buf), buf.numel(), lddy, native._stream()]
    rc = hip.lib.pcs_bn_bwd_stats_f32(*head, *rest) if name == "fp32" else hip.lib.pcs_bn_bwd_stats_h(*head, CODE[name], *rest)
    return rc, buf[:2 * c]


def _raw_bwd_apply(hip, name, dy, x, y, mask, stat, s2, count, w, n, c, relu, dx, dres, lddy, in_slope=1.0):
    from openpcseg_amd import native
    p = native._ptr
    return hip.lib.pcs_bn_bwd_apply_act(p(dy), p(x), p(y), p(mask), p(stat), p(s2), float(count), None, p(w), n, c, int(relu),
                                        CODE[name], float(in_slope), p(dx), p(dres), lddy, native._stream())


@gpu
@pytest.mark.parametrize("c,ct", [(4, 256), (256, 4), (20, 12), (96, 132)])
def test_exact_concat_layout(hip, c, ct):
    """apply writes y into the left c columns of an (n, c + ct) buffer and copies `tail` right of it; the backward passes read
    dy out of the gradient of that buffer through the row stride."""
    for n in (37, 1000):
        k = _exact_case(n, c)
        stat, w, b, s2 = _params(k)
        tail64 = np.random.default_rng(ct).integers(-8, 9, size=(n, ct)).astype(np.float64)
        grad64 = np.concatenate([k["dy"], tail64[:, ::-1]], axis=1)
        for name in DT:
            r = _exact_references(k, name)
            x, res, yg = dev(k["x"], name), dev(k["res"], name), dev(r["y"], name)
            out = hip.bn_apply(x, res, stat, w, b, True, tail=dev(tail64, name))
            same(out, np.concatenate([r["y"], tail64], axis=1), name, "concat n=%d %s" % (n, name))
            grad = dev(grad64, name)
            dy = grad[:, :c]
            assert dy.stride(0) == c + ct
            assert np.array_equal(host(hip.bn_bwd_stats(dy, x, yg, stat, True)), r["sums2"])
            dx, dres = hip.bn_bwd_apply(dy, x, yg, stat, s2, 2.0, w, True, True)
            same(dx, r["dx"], name, "concat dx")
            same(dres, r["dres"], name, "concat dres")
            assert torch.equal(grad, dev(grad64, name))


@gpu
@pytest.mark.parametrize("name", DT)
def test_exact_row_strides_through_the_raw_entries(hip, name):
    """ldy > c + ctail: the gap columns keep what they held. lddy % 4 != 0: the scalar path, the same values."""
    n, c, ct, ldy = 1000, 20, 12, 40
    k = _exact_case(n, c)
    stat, w, b, s2 = _params(k)
    r = _exact_references(k, name)
    x, res = dev(k["x"], name), dev(k["res"], name)
    tail64 = np.random.default_rng(1).integers(-8, 9, size=(n, ct)).astype(np.float64)
    tail = dev(tail64, name)
    buf = torch.full((n, ldy), -77.0, dtype=x.dtype, device="cuda")
    assert _raw_apply(hip, name, x, res, stat, w, b, n, c, True, buf, None, ldy, tail, ct) == 0
    want = np.concatenate([r["y"], tail64, np.full((n, ldy - c - ct), -77.0)], axis=1)
    same(buf, want, name, "gap columns")
    assert _raw_apply(hip, name, x, res, stat, w, b, n, c, True, buf, None, c + ct - 1, tail, ct) == PCS_EINVAL   # stride too small

    n, c, lddy = 1000, 32, 35
    k = _exact_case(n, c)
    stat, w, b, s2 = _params(k)
    r = _exact_references(k, name)
    x, yg = dev(k["x"], name), dev(r["y"], name)
    grad64 = np.concatenate([k["dy"], np.full((n, lddy - c), 99.0)], axis=1)
    grad = dev(grad64, name)
    rc, sums2 = _raw_bwd_stats(hip, name, grad, x, yg, None, stat, n, c, True, lddy)
    assert rc == 0 and np.array_equal(host(sums2), r["sums2"])
    dx, dres = torch.empty_like(x), torch.empty_like(x)
    assert _raw_bwd_apply(hip, name, grad, x, yg, None, stat, s2, 2.0, w, n, c, True, dx, dres, lddy) == 0
    same(dx, r["dx"], name, "dx, lddy = 35")
    same(dres, r["dres"], name, "dres, lddy = 35")
    # the bit mask needs the vector path: refused on this stride
    rc, _ = _raw_bwd_stats(hip, name, grad, x, None, devmask(r["y"]), stat, n, c, True, lddy)
    assert rc == PCS_EUNSUPPORTED
    assert _raw_bwd_stats(hip, name, grad, x, yg, None, stat, n, c, True, c - 1)[0] == PCS_EINVAL


def _off_by_one(t):
    """The same (n, c) values on a view that starts one element into a flat buffer: rows no longer 16 / 8-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) != 0
    return v


@gpu
@pytest.mark.parametrize("name", DT)
def test_alignment_fallback(hip, name):
    """c = 32 with misaligned rows takes the scalar path in every pass: equal to the reference on the exact data, and on real
    data the apply passes are bit-identical to the aligned call. A mask request there is refused and writes nothing."""
    n, c = 1000, 32
    k = _exact_case(n, c)
    stat, w, b, s2 = _params(k)
    r = _exact_references(k, name)
    x, dy, res, yg = (_off_by_one(dev(a, name)) for a in (k["x"], k["dy"], k["res"], r["y"]))
    assert np.array_equal(host(hip.bn_stats(x)), r["sums"])
    same(hip.bn_apply(x, res, stat, w, b, True), r["y"], name, "y")
    assert np.array_equal(host(hip.bn_bwd_stats(dy, x, yg, stat, True)), r["sums2"])
    dx, dres = hip.bn_bwd_apply(dy, x, yg, stat, s2, 2.0, w, True, True, in_slope=0.5)
    same(dx, r["dx_slope"], name, "dx")
    same(dres, r["dres"], name, "dres")

    q = _real_case(n, c, name, 3)
    stat, w, b, s2 = dev64(q["stat"]), dev(q["w"]), dev(q["b"]), dev64(q["s2"])
    xa, dya, resa = dev(q["x"], name), dev(q["dy"], name), dev(q["res"], name)
    xm, resm = _off_by_one(xa), _off_by_one(resa)
    ya = hip.bn_apply(xa, resa, stat, w, b, True)
    assert torch.equal(hip.bn_apply(xm, resm, stat, w, b, True), ya)
    for a, m in zip(hip.bn_bwd_apply(dya, xa, ya, stat, s2, float(n), w, True, True),
                    hip.bn_bwd_apply(dya, xm, _off_by_one(ya), stat, s2, float(n), w, True, True)):
        assert torch.equal(a, m)
    # the statistics passes sum in another order on the scalar path (TY = 8 rows per workgroup, not 32): both calls within
    # the bound of the float64 sums, hence within twice the bound of each other
    b0, b1 = R.stats_bound(q["x"])
    sm, sa, s64 = host(hip.bn_stats(xm)), host(hip.bn_stats(xa)), R.sums(q["x"])
    assert sm[2 * c] == sa[2 * c] == n
    for got, tag in ((sm, "misaligned"), (sa, "aligned")):
        within(got[:c], s64[:c], b0, ("stats", name), tag + " sum x")
        within(got[c:2 * c], s64[c:2 * c], b1, ("stats", name), tag + " sum x^2")
    assert (np.abs(sm[:c] - sa[:c]) <= 2 * b0).all() and (np.abs(sm[c:2 * c] - sa[c:2 * c]) <= 2 * b1).all()
    gate64 = host(ya)                                # the gate both calls are handed: y as the aligned apply stored it
    g0, g1 = R.bwd_stats_bound(q["dy"], q["x"], q["stat"], gate64)
    t64 = R.bwd_stats(q["dy"], q["x"], q["stat"], gate64)
    ta = hip.bn_bwd_stats(dya, xa, ya, stat, True)
    tm = hip.bn_bwd_stats(_off_by_one(dya), xm, _off_by_one(ya), stat, True)
    for got, tag in ((tm, "misaligned"), (ta, "aligned")):
        within(host(got)[:c], t64[:c], g0, ("bwd_stats", name), tag + " sum g")
        within(host(got)[c:], t64[c:], g1, ("bwd_stats", name), tag + " sum g xhat")
        assert torch.equal(got._pcs_f32, got.float())
    assert (np.abs(host(tm)[:c] - host(ta)[:c]) <= 2 * g0).all() and (np.abs(host(tm)[c:] - host(ta)[c:]) <= 2 * g1).all()
    assert torch.equal(hip.bn_bwd_stats(dya, xa, devmask(gate64), stat, True), ta)   # and the mask form of the aligned call

    y = torch.full((n, c), -77.0, dtype=xm.dtype, device="cuda")
    mask = torch.full((n, 1), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert _raw_apply(hip, name, xm, None, stat, w, b, n, c, True, y, mask, c, None, 0) == PCS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == -77.0).all()) and bool((mask == 0x5A5A5A5A).all())


# ---- 3. real-valued cases -----------------------------------------------------------------------------------------------
def _real_case(n, c, name, seed):
    rng = np.random.default_rng(1000003 * seed + 131 * c + n)
    x = R.rounded(rng.normal(size=(n, c)) * 1.7 + 0.3, name)
    dy, res = R.rounded(rng.normal(size=(n, c)), name), R.rounded(rng.normal(size=(n, c)), name)
    stat = np.concatenate([0.3 + 0.2 * rng.normal(size=c), rng.uniform(0.4, 0.8, size=c)])
    w = (rng.uniform(0.5, 1.5, size=c) * rng.choice([-1.0, 1.0], size=c)).astype(np.float32).astype(np.float64)
    b = rng.uniform(-0.5, 0.5, size=c).astype(np.float32).astype(np.float64)
    return dict(n=n, c=c, x=x, dy=dy, res=res, stat=stat, w=w, b=b, s2=rng.normal(size=2 * c) * np.sqrt(n))


VARIANTS = [(True, True, True), (True, False, True), (False, False, False), (False, True, True)]   # relu, residual, w and b
REAL_APPLY = [(4, 1000), (20, 37), (32, 32769), (96, 37), (204, 1000), (256, 17), (256, 32769), (260, 1000), (288, 1000),
              (384, 37), (1, 1000), (3, 37), (5, 1000), (65, 37), (409, 1000)]


@gpu
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("c,n", REAL_APPLY)
def test_real_apply_passes(hip, c, n, name):
    relu, with_res, affine = VARIANTS[REAL_APPLY.index((c, n)) % 4]
    k = _real_case(n, c, name, 1)
    x64, res64 = k["x"], k["res"] if with_res else None
    w64, b64 = (k["w"], k["b"]) if affine else (None, None)
    stat, w, b, s2 = dev64(k["stat"]), dev(w64), dev(b64), dev64(k["s2"])
    x, dy, res = dev(x64, name), dev(k["dy"], name), dev(res64, name)
    y64 = R.apply(x64, k["stat"], w64, b64, res64, relu)
    tag = "n=%d c=%d" % (n, c)
    want_mask = relu and c % 32 == 0
    out = hip.bn_apply(x, res, stat, w, b, relu, want_mask=want_mask)
    y = out[0] if want_mask else out
    within(host(y), y64, R.apply_bound(x64, k["stat"], w64, b64, res64, y64, name), ("apply", name), tag)
    if relu:
        unsure = R.unsure(x64, k["stat"], w64, b64, res64, name)
        assert unsure.mean() <= 1e-3
        if want_mask:   # the bit of the stored y, wherever the float64 pre-activation decides it
            stored_gate = R.rounded(y64, name) > 0
            assert np.array_equal(R.mask_bits(out[1].cpu().numpy(), c)[~unsure], stored_gate[~unsure]), tag
    # backward apply, the gate handed in (the float64 result as stored): nothing of the forward kernel in it
    gate64 = R.rounded(y64, name) if relu else None
    for slope in (None, 0.1):
        dx64, dres64 = R.bwd_apply(k["dy"], x64, k["stat"], k["s2"], n, w64, gate64, in_slope=slope)
        dx, dres = hip.bn_bwd_apply(dy, x, dev(gate64, name), stat, s2, float(n), w, relu, with_res, in_slope=slope)
        within(host(dx), dx64, R.bwd_apply_bound(k["dy"], x64, k["stat"], k["s2"], n, w64, gate64, slope, dx64, name),
               ("bwd_apply", name), tag + (" in_slope" if slope else ""))
        if with_res:
            assert np.array_equal(host(dres), dres64), tag + " dres"
        if want_mask:
            for a, m in zip((dx, dres), hip.bn_bwd_apply(dy, x, devmask(gate64), stat, s2, float(n), w, relu, with_res, in_slope=slope)):
                assert (a is None and m is None) or torch.equal(a, m), tag


REAL_STATS = [(256, 4097), (256, 16385), (409, 4096), (409, 20481), (32, 33), (32, 32769), (1, 257), (1, 262145), (260, 1000),
              (204, 37), (96, 1000), (5, 1000), (20, 4097), (65, 1000)]


@gpu
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("c,n", REAL_STATS)
def test_real_statistics_passes(hip, c, n, name):
    relu = REAL_STATS.index((c, n)) % 2 == 0
    k = _real_case(n, c, name, 2)
    x64, dy64 = k["x"], k["dy"]
    x, dy, stat = dev(x64, name), dev(dy64, name), dev64(k["stat"])
    tag = "n=%d c=%d" % (n, c)
    s, s64 = host(hip.bn_stats(x)), R.sums(x64)
    assert s[2 * c] == n
    b0, b1 = R.stats_bound(x64)
    within(s[:c], s64[:c], b0, ("stats", name), tag + " sum x")
    within(s[c:2 * c], s64[c:2 * c], b1, ("stats", name), tag + " sum x^2")
    gate64 = R.rounded(R.apply(x64, k["stat"], k["w"], k["b"], None, True), name) if relu else None
    s2 = hip.bn_bwd_stats(dy, x, dev(gate64, name), stat, relu)
    s2_64 = R.bwd_stats(dy64, x64, k["stat"], gate64)
    g0, g1 = R.bwd_stats_bound(dy64, x64, k["stat"], gate64)
    within(host(s2)[:c], s2_64[:c], g0, ("bwd_stats", name), tag + " sum g")
    within(host(s2)[c:], s2_64[c:], g1, ("bwd_stats", name), tag + " sum g xhat")
    assert torch.equal(s2._pcs_f32, s2.float())
    if relu and c % 32 == 0:
        assert torch.equal(hip.bn_bwd_stats(dy, x, devmask(gate64), stat, relu), s2)


# ---- 4. SyncBN arithmetic on one device ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["fp32", "bf16"])
@pytest.mark.parametrize("c", [32, 20])
def test_syncbn_arithmetic_over_shards(hip, c, name):
    """Shards of 700, 1 and 0 rows: the summed `sums` with the device-resident global count give the statistics of the whole
    tensor; the backward of a shard with the summed sums2 is the whole tensor's backward restricted to its rows."""
    n = 701
    k = _real_case(n, c, name, 4)
    x64, dy64, w64, b64 = k["x"], k["dy"], k["w"], k["b"]
    cuts = [(0, 700), (700, 701), (701, 701)]
    xs = [dev(x64[a:e], name) for a, e in cuts]
    dys = [dev(dy64[a:e], name) for a, e in cuts]
    parts = [hip.bn_stats(t) for t in xs]
    assert [float(p[2 * c]) for p in parts] == [700.0, 1.0, 0.0] and not bool(parts[2].any())
    total = parts[0] + parts[1] + parts[2]
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    stat = hip.bn_finalize(total, 0.0, EPS, MOM, rm, rv, count_dev=total[2 * c:])
    # statistics of the whole tensor: the error of the summed sums is at most the shards' bounds added
    b0 = sum(R.stats_bound(x64[a:e])[0] for a, e in cuts)
    b1 = sum(R.stats_bound(x64[a:e])[1] for a, e in cuts)
    s64 = R.sums(x64)
    within(host(total)[:c], s64[:c], b0, ("stats", name), "shards sum x")
    within(host(total)[c:2 * c], s64[c:2 * c], b1, ("stats", name), "shards sum x^2")
    stat64, rm64, rv64 = R.finalize(s64, n, EPS, MOM, np.zeros(c), np.ones(c))
    mean64, var64 = stat64[:c], 1.0 / stat64[c:] ** 2 - EPS
    dmean = b0 / n
    dvar = b1 / n + (2 * np.abs(mean64) + dmean) * dmean
    got = host(stat)
    assert (np.abs(got[:c] - mean64) <= dmean + 1e-15).all()
    lo, hi = 1.0 / np.sqrt(var64 + dvar + EPS), 1.0 / np.sqrt(np.maximum(var64 - dvar, 0.0) + EPS)
    assert ((got[c:] >= lo * (1 - 1e-15)) & (got[c:] <= hi * (1 + 1e-15))).all()
    # finalize itself is double arithmetic on the vector it was given: exact against the reference on the SAME sums, global count
    same_stat, rm_s, rv_s = R.finalize(host(total), n, EPS, MOM, np.zeros(c), np.ones(c))
    assert np.allclose(got, same_stat, rtol=1e-14, atol=0)
    assert np.array_equal(host(rm), rm_s.astype(np.float32).astype(np.float64))
    assert np.allclose(host(rv), rv_s, rtol=2.0 ** -23, atol=0)
    assert np.abs(host(rv) - rv64).max() <= MOM * (dvar * n / (n - 1)).max() + 2.0 ** -23 * np.abs(rv64).max()

    # backward: the gate of every shard is the whole tensor's float64 result as stored
    stat_h = got
    y64 = R.rounded(R.apply(x64, stat_h, w64, b64, None, True), name)
    s2_parts = [hip.bn_bwd_stats(dys[i], xs[i], dev(y64[a:e], name), stat, True) for i, (a, e) in enumerate(cuts)]
    assert not bool(s2_parts[2].any())
    s2 = s2_parts[0] + s2_parts[1] + s2_parts[2]
    s2_64 = R.bwd_stats(dy64, x64, stat_h, y64)
    g0 = sum(R.bwd_stats_bound(dy64[a:e], x64[a:e], stat_h, y64[a:e])[0] for a, e in cuts)
    g1 = sum(R.bwd_stats_bound(dy64[a:e], x64[a:e], stat_h, y64[a:e])[1] for a, e in cuts)
    within(host(s2)[:c], s2_64[:c], g0, ("bwd_stats", name), "shards sum g")
    within(host(s2)[c:], s2_64[c:], g1, ("bwd_stats", name), "shards sum g xhat")
    w = dev(w64)
    for slope in (None, 0.1):
        # the float64 backward of the whole tensor with the sums this pass is handed, restricted to the shard's rows
        dx64, dres64 = R.bwd_apply(dy64, x64, stat_h, host(s2), n, w64, y64, in_slope=slope)
        bound = R.bwd_apply_bound(dy64, x64, stat_h, host(s2), n, w64, y64, slope, dx64, name)
        for i, (a, e) in enumerate(cuts):
            dx, dres = hip.bn_bwd_apply(dys[i], xs[i], dev(y64[a:e], name), stat, s2, 0.0, w, True, True,
                                        count_dev=total[2 * c:], in_slope=slope)
            assert dx.shape == (e - a, c) and dres.shape == (e - a, c)
            within(host(dx), dx64[a:e], bound[a:e], ("bwd_apply", name), "shard %d" % i + (" in_slope" if slope else ""))
            assert np.array_equal(host(dres), dres64[a:e])


# ---- 5. empty and single-row tensors ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("c", [32, 5])
def test_empty_tensor_through_every_wrapper(hip, c, name):
    from openpcseg_amd import native
    dt = R.torch_dtype(name)
    x = torch.empty(0, c, dtype=dt, device="cuda")
    w, b = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    s = hip.bn_stats(x)
    assert s.shape == (2 * c + 1,) and not bool(s.any())
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    stat = hip.bn_finalize(s, 0.0, EPS, MOM, rm, rv, count_dev=s[2 * c:])
    assert bool(torch.isfinite(stat).all()) and not bool(stat[:c].any())     # count 0 read as 1
    assert np.allclose(host(stat[c:]), 1.0 / np.sqrt(EPS), rtol=1e-14)
    assert bool(torch.isfinite(rm).all()) and bool(torch.isfinite(rv).all())
    if c % 32 == 0:
        y, gate = hip.bn_apply(x, x, stat, w, b, True, want_mask=True)
        assert gate.shape == (0, c // 32)
    else:
        y = gate = hip.bn_apply(x, x, stat, w, b, True)
    assert y.shape == (0, c) and y.dtype == dt
    if c % 4 == 0:
        assert hip.bn_apply(x, None, stat, None, None, False, tail=torch.empty(0, 8, dtype=dt, device="cuda")).shape == (0, c + 8)
    s2 = hip.bn_bwd_stats(x, x, gate, stat, True)
    assert s2.shape == (2 * c,) and not bool(s2.any()) and not bool(s2._pcs_f32.any())
    for slope in (None, 0.1):
        dx, dres = hip.bn_bwd_apply(x, x, gate, stat, s2, 0.0, w, True, True, count_dev=s[2 * c:], in_slope=slope)
        assert dx.shape == (0, c) and dres.shape == (0, c)
        dx, dres = hip.bn_bwd_apply(x, x, gate, stat, s2, 0.0, w, True, True, in_slope=slope)   # no rows: the count is not looked at
        assert dx.shape == (0, c) and dres.shape == (0, c)
    # the convolution write-back of an empty output has no tiles: no partial rows
    none = torch.empty(0, dtype=torch.float64, device="cuda")
    r = hip.bn_reduce_partials(none, c, 0)
    assert r.shape == (2 * c + 1,) and not bool(r.any())
    rm2, rv2 = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    stat2 = hip.bn_reduce_finalize(none, c, 0, EPS, MOM, rm2, rv2)                              # n == 0 read as count 1
    assert torch.equal(stat2, stat) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
    # a null tensor with rows to read is still refused
    ws = torch.empty(hip.lib.pcs_bn_num_partials() * 2 * c, dtype=torch.float32, device="cuda")
    p = native._ptr
    if name == "fp32":
        assert hip.lib.pcs_bn_stats_f32(None, 5, c, p(ws), p(s), native._stream()) == PCS_EINVAL
    else:
        assert hip.lib.pcs_bn_stats_h(None, 5, c, CODE[name], p(ws), p(s), native._stream()) == PCS_EINVAL
    one = torch.zeros(5, c, dtype=dt, device="cuda")
    assert _raw_bwd_stats(hip, name, None, one, None, None, stat, 5, c, False, c)[0] == PCS_EINVAL
    assert _raw_bwd_stats(hip, name, one, None, None, None, stat, 5, c, False, c)[0] == PCS_EINVAL
    assert _raw_bwd_stats(hip, name, one, one, None, None, stat, 5, c, True, c)[0] == PCS_EINVAL    # ReLU without a gate
    assert hip.lib.pcs_bn_reduce_partials(None, 3, c, 5, p(s), native._stream()) == PCS_EINVAL
    assert hip.lib.pcs_bn_reduce_partials_finalize(None, 3, c, 5, EPS, MOM, None, None, None, p(stat2), native._stream()) == PCS_EINVAL
    assert _raw_bwd_apply(hip, name, one, one, None, None, stat, s2, 0.0, w, 5, c, False, one.clone(), None, c) == PCS_EINVAL   # rows, no count


@gpu
@pytest.mark.parametrize("name", DT)
def test_empty_tensor_through_the_module(hip, name):
    """FusedBatchNorm in training mode on an empty tensor: forward and backward run (under SyncBN a rank that raised here
    would leave the others waiting in the all-reduce), the gradients are zero."""
    from openpcseg_amd.fused import FusedBatchNorm
    from openpcseg_amd.sparse import SparseTensor
    for c in (32, 20):
        bn = FusedBatchNorm(c).cuda().train()
        x = torch.empty(0, c, dtype=R.torch_dtype(name), device="cuda", requires_grad=True)
        r = torch.empty(0, c, dtype=R.torch_dtype(name), device="cuda", requires_grad=True)
        coords = torch.empty(0, 4, dtype=torch.int32, device="cuda")
        y = bn(SparseTensor(x, coords), residual=SparseTensor(r, coords), relu=True).F
        assert y.shape == (0, c)
        y.sum().backward()
        assert x.grad.shape == (0, c) and r.grad.shape == (0, c)
        assert not bool(bn.weight.grad.any()) and not bool(bn.bias.grad.any())
        assert bool(torch.isfinite(bn.running_mean).all()) and bool(torch.isfinite(bn.running_var).all())


@gpu
@pytest.mark.parametrize("name", DT)
@pytest.mark.parametrize("c", [32, 5])
def test_single_row(hip, c, name):
    """n = 1: variance 0, invstd = 1 / sqrt(eps), running_var updated with the biased value (count > 1 guards the n / (n - 1))."""
    x64 = R.rounded(np.random.default_rng(c).normal(size=(1, c)) * 1.7 + 0.3, name)
    s = hip.bn_stats(dev(x64, name))
    assert np.array_equal(host(s), R.sums(x64))     # the pivot IS the row: x and x^2 un-shifted in double
    rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
    stat = hip.bn_finalize(s, 1.0, EPS, MOM, rm, rv)
    stat64, rm64, rv64 = R.finalize(R.sums(x64), 1, EPS, MOM, np.zeros(c), np.ones(c))
    assert np.array_equal(host(stat)[:c], x64[0]) and np.allclose(host(stat)[c:], 1.0 / np.sqrt(EPS), rtol=1e-15, atol=0)
    assert np.array_equal(host(rv), np.full(c, np.float32(0.9), dtype=np.float64))
    assert np.array_equal(host(rm), rm64.astype(np.float32).astype(np.float64))
    b64, y64 = np.full(c, 0.25), np.full((1, c), 0.25)
    y = hip.bn_apply(dev(x64, name), None, stat, None, dev(b64), False)
    within(host(y), y64, R.apply_bound(x64, host(stat), None, b64, None, y64, name), ("apply", name), "n=1 c=%d" % c)


# ---- 6. the fp16 gate ---------------------------------------------------------------------------------------------------
@gpu
def test_mask_bit_is_the_gate_of_the_stored_value(hip):
    """A pre-activation in (0, 2^-25] is positive in fp32 and stores as 0 in fp16. The mask bit is [y > 0] of the STORED y, so
    the mask form and the y form of backward agree and a layer's gradient does not depend on c % 32."""
    n, c = 4, 32
    x64 = np.zeros((n, c))
    stat64 = np.concatenate([np.zeros(c), np.ones(c)])            # x = mean = 0: the pre-activation is b
    b64 = np.ones(c)
    b64[:4] = [2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -25]   # stores as 0, 0 (tie to even), 2^-24, 2^-24
    dy64 = np.arange(1, n * c + 1, dtype=np.float64).reshape(n, c) / 64
    stat, b = dev64(stat64), dev(b64)
    s2 = dev64(np.zeros(2 * c))
    for name, on in [("fp16", [False, False, True, True]), ("fp32", [True] * 4), ("bf16", [True] * 4)]:
        x, dy = dev(x64, name), dev(dy64, name)
        y, mask = hip.bn_apply(x, None, stat, None, b, True, want_mask=True)
        bits = R.mask_bits(mask.cpu().numpy(), c)
        assert np.array_equal(bits, host(y) > 0), name
        assert bits[:, :4].tolist() == [on] * n and bits[:, 4:].all(), name
        assert torch.equal(mask, devmask(host(y)))
        assert torch.equal(hip.bn_bwd_stats(dy, x, mask, stat, True), hip.bn_bwd_stats(dy, x, y, stat, True)), name
        for a, m in zip(hip.bn_bwd_apply(dy, x, y, stat, s2, float(n), None, True, True),
                        hip.bn_bwd_apply(dy, x, mask, stat, s2, float(n), None, True, True)):
            assert torch.equal(a, m), name
        dres = host(hip.bn_bwd_apply(dy, x, mask, stat, s2, float(n), None, True, True)[1])
        assert np.array_equal(dres[:, :4] != 0, np.array([on] * n)), name


# ---- 7. statistics producers under |mean| >> std and an outlying pivot ------------------------------------------------------
def _check_stat(stat, x64, what, mean_tol):
    c = x64.shape[1]
    mean, var = x64.mean(0), x64.var(0)
    got = host(stat)
    merr = np.abs(got[:c] - mean)
    ierr = np.abs(got[c:] * np.sqrt(var + EPS) - 1.0)
    print("[bn] %-40s mean err / tol = %.3g, invstd rel err = %.3g" % (what, float((merr / mean_tol).max()), float(ierr.max())))
    assert (merr <= mean_tol).all(), what
    assert (ierr <= 2e-4).all(), what


@gpu
@pytest.mark.parametrize("n,c", [(262144, 4), (16385, 256)])
@pytest.mark.parametrize("d", [0.0, 10.0, 30.0])
def test_stats_pass_with_an_outlying_pivot_row(hip, n, c, d):
    """The pivot of the shifted sums is row 0 of the tensor: d standard deviations off the mean."""
    x = np.random.default_rng(n + c).normal(size=(n, c)).astype(np.float32)
    x[0] = d
    s = hip.bn_stats(torch.from_numpy(x).cuda())
    _check_stat(hip.bn_finalize(s, float(n), EPS, MOM, None, None), x.astype(np.float64), "bn_stats n=%d c=%d d=%g" % (n, c, d), 1e-6)


@gpu
@pytest.mark.parametrize("c", [1, 3, 4, 5, 96])
def test_reduce_partials_alone(hip, c):
    for nrows in (1, 255, 256, 257, 2047, 2048, 2049, 4097):
        p = np.random.default_rng(nrows + c).integers(-1000, 1001, size=(nrows, 2, c)).astype(np.float64)
        s = host(hip.bn_reduce_partials(dev64(p), c, 12345))
        assert np.array_equal(s[:2 * c], p.sum(0).reshape(-1)) and s[2 * c] == 12345, (nrows, c)


def _scene(rng, n, extent):
    c = np.concatenate([rng.integers(0, extent, size=(n, 3)), np.zeros((n, 1), dtype=np.int64)], axis=1)
    c = np.unique(c.astype(np.int32), axis=0)
    return c[rng.permutation(c.shape[0])]


@gpu
@pytest.mark.parametrize("kind,cin,cout,mean", [("fp32", 64, 96, 300.0), ("fp32", 64, 96, -300.0), ("fp32", 4, 32, 300.0),
                                                ("fp32", 4, 32, -300.0), ("bf16", 64, 64, 30.0), ("bf16", 64, 64, -30.0),
                                                ("fp16", 64, 64, 30.0), ("fp16", 64, 64, -30.0)])
@pytest.mark.parametrize("lonely_first", [False, True], ids=["dense", "lonely-row-first"])
def test_conv_write_back_partials_under_a_large_mean(hip, kind, cin, cout, mean, lonely_first):
    """The convolution leaves per-tile sums about the tile's first row. A bias puts the output at |mean| >> std; with
    lonely_first the first row of the first tile has no pair at all (its value is the bias alone). Both reductions against the
    float64 statistics of the STORED output, and bit-identical to each other."""
    from openpcseg_amd import functional as F
    rng = np.random.default_rng(cin + cout)
    coords = _scene(rng, 4000, 16)
    out_coords = np.concatenate([np.array([[200, 200, 200, 0]], dtype=np.int32), coords]) if lonely_first else coords
    cin_t, cout_t = torch.from_numpy(coords).cuda(), torch.from_numpy(out_coords).cuda()
    km = F.build_kernel_map(cin_t, cout_t if lonely_first else cin_t, (3, 3, 3), (1, 1, 1), (1, 1, 1)).fwd
    n = out_coords.shape[0]
    pairs_per_row = max(km.num_pairs / n, 1.0)
    x = torch.from_numpy(rng.normal(size=(coords.shape[0], cin)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.normal(size=(27, cin, cout)) / np.sqrt(cin * pairs_per_row)).astype(np.float32)).cuda()
    bias = torch.full((cout,), mean, device="cuda") + torch.linspace(-1, 1, cout, device="cuda")
    got = []
    if kind == "fp32":
        out = hip.conv_gather_gemm(x, w, km, bias=bias, tile_rows=64, bn_sums=got, bn_raw=True)
    else:
        dt = R.torch_dtype(kind)
        out = hip.conv_gather_gemm_h(x.to(dt), hip.prepare_weights_h(w, dt, transpose=False), 27, cout, km, bias=bias, tile_rows=64,
                                     bn_sums=got, bn_raw=True)
    assert len(got) == 1 and got[0].numel() == -(-n // 64) * 2 * cout
    o64 = host(out)
    assert out.shape == (n, cout) and 0.3 < float(o64.std(0).mean()) < 3.0
    if lonely_first:
        assert np.array_equal(o64[0], host(bias.to(out.dtype)))
    rm_a, rv_a = torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")
    rm_b, rv_b = rm_a.clone(), rv_a.clone()
    stat_a = hip.bn_reduce_finalize(got[0], cout, n, EPS, MOM, rm_a, rv_a)
    sums = hip.bn_reduce_partials(got[0], cout, n)
    stat_b = hip.bn_finalize(sums, float(n), EPS, MOM, rm_b, rv_b)
    assert torch.equal(stat_a, stat_b) and torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b)
    assert float(sums[2 * cout]) == n
    tol = (1e-6 + (R.U_S[kind] if kind != "fp32" else 0.0)) * np.abs(o64.mean(0))
    _check_stat(stat_a, o64, "conv %s %d->%d mean %g%s" % (kind, cin, cout, mean, " lonely" if lonely_first else ""), tol)
