"""RPVNet's range-point-voxel merge (csrc/rangemerge.hip, fused.range_point_merge):

    out = ( devoxelize(vox, idx8, w8) + range_sample(img, pxpy) ) + third,    third = relu(bn(lin)) (bn mode) or lin (add mode)

Checks (bounds derived, not measured; tests/range_merge_reference.py is the float64 side and states the bound):
  1. fp32: out and mask bit for bit what pcs_devoxelize_fwd_f32, pcs_range_sample_fwd_f32, an add, pcs_bn_apply_f32 (relu), an add give.
  2. every storage format: |out - ref64| <= ulp_storage(|ref64| + e) / 2 + e, e = 32 * 2^-24 * T, nothing excluded, on the (4, 8)
     image at dyadic coordinates (x = (2 ix + 1) / W - 1 with ix a multiple of 1/8: ix is exact whether or not the compiler
     contracts the expression, so the float32 weights of the reference are the kernel's).
  3. the mask is exact on representable data (small-integer lin, power-of-two gamma / invstd / mean / beta), c = 32 and 96.
  4. return codes.  5. autograd through fused.range_point_merge, switch on against off.  6. routing.
Shapes: n in {1, 63, 64, 65, 257} (one workgroup owns 64 points), m = 37 voxels, B = 2, (H, W) in {(4, 8), (5, 7)},
c in {4, 12} (fp32 only), {8, 24, 56, 168} (add mode), {32, 96, 448} (both modes; 96 = a chunk with a tail, 448 = seven chunks)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import range_merge_reference as R
from openpcseg_amd import build as pcs_build
from openpcseg_amd import cpu_fallback, fused, native
from openpcseg_amd.fused import FusedBatchNorm

NS = [1, 63, 64, 65, 257]
M, B = 37, 2
HWS = [(4, 8), (5, 7)]
C_F32_ONLY, C_ADD, C_BN = [4, 12], [8, 24, 56, 168], [32, 96, 448]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["fp32", "bf16", "fp16"]
NAME = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}


def widths(dtype):
    return (C_F32_ONLY if dtype == torch.float32 else []) + C_ADD + C_BN


# ---- cases -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, c, hw, off_frames=False):
    """About a quarter of the corners -1 and (n >= 3) one point without any; frames non-decreasing in {0, 1}; coordinates: on (4, 8)
    dyadic (ix, iy multiples of 1/8 between -2.5 and size + 1.5), on (5, 7) uniform in [-1.3, 1.3]; both include x or y at exactly
    -1 and +1 and points with all four corners outside. off_frames (backend level only): a frame of B and a frame of 0.5."""
    h, w = hw
    rng = np.random.default_rng(1000 * n + 10 * c + h)
    idx8 = rng.integers(0, M, size=(n, 8)).astype(np.int32)
    idx8[rng.uniform(size=(n, 8)) < 0.25] = -1
    if n >= 3:
        idx8[1] = -1
    idx8[n - 1, 0] = M - 1
    w8 = rng.uniform(0, 1, size=(n, 8)).astype(np.float32)
    frame = np.sort(rng.integers(0, B, size=n)).astype(np.float32)
    if hw == (4, 8):
        ix = rng.integers(-20, 8 * w + 12, size=n) / 8.0
        iy = rng.integers(-20, 8 * h + 12, size=n) / 8.0
        x, y = (2 * ix + 1) / w - 1, (2 * iy + 1) / h - 1
    else:
        x, y = rng.uniform(-1.3, 1.3, size=n), rng.uniform(-1.3, 1.3, size=n)
    for i, (vx, vy) in enumerate([(-1.0, 0.25), (1.0, -0.5), (0.5, -1.0), (-0.25, 1.0), (1.0, 1.0), (-1.5, 0.0), (0.0, 1.75)]):
        if i + 2 < n:
            x[i + 2], y[i + 2] = vx, vy
    pxpy = np.stack([frame, x, y], axis=1).astype(np.float32)
    if off_frames and n >= 12:
        pxpy[10, 0], pxpy[11, 0] = float(B), 0.5
    assert (pxpy[:, 1:].astype(np.float64) == np.stack([x, y], axis=1)).all() or hw != (4, 8)   # dyadic: exact in float32
    vox = rng.normal(size=(M, c)).astype(np.float32)
    lin = rng.normal(size=(n, c)).astype(np.float32)
    img = rng.normal(size=(B, c, h, w)).astype(np.float32)
    stat = np.concatenate([0.3 * rng.normal(size=c), rng.uniform(0.5, 2.0, size=c)])   # mean | invstd, float64
    gamma = rng.uniform(0.5, 1.5, size=c).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, size=c).astype(np.float32)
    return dict(idx8=idx8, w8=w8, pxpy=pxpy, vox=vox, lin=lin, img=img, stat=stat, gamma=gamma, beta=beta)


def stored(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)
    return t, t.float().numpy().astype(np.float64)


def dev(a):
    if a is None:
        return None
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def mask_bits(mask, c):
    m = mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return ((m[:, :, None] >> np.arange(32)) & 1).reshape(mask.shape[0], c).astype(bool)


def run_backend(be, k, dtype, bn, to=lambda a: a):
    vt, v64 = stored(k["vox"], dtype)
    lt, l64 = stored(k["lin"], dtype)
    t = lambda a: to(torch.from_numpy(np.ascontiguousarray(a)))
    st = (t(k["stat"]), t(k["gamma"]), t(k["beta"])) if bn else (None, None, None)
    out, mask = be.range_point_merge(to(vt), t(k["idx8"]), t(k["w8"]), t(k["img"]), t(k["pxpy"]), to(lt), *st)
    ref, bn64, T = R.merge64(v64, k["idx8"], k["w8"], k["img"], k["pxpy"], l64, *((k["stat"], k["gamma"], k["beta"]) if bn else ()))
    return out, mask, ref, bn64, T


def check_bound(out, ref, T, dtype, what):
    o = out.detach().float().cpu().numpy().astype(np.float64)
    lim = R.bound(ref, T, NAME[dtype])
    err = np.abs(o - ref)
    print("[range merge] %s %s: worst error / bound = %.3f" % (what, NAME[dtype], float((err / lim).max())))
    assert (err <= lim).all(), (what, float((err / lim).max()))


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_merge_entries():
    lib = ctypes.CDLL(pcs_build.LIB_PATH)
    assert hasattr(lib, "pcs_range_point_merge_f32") and hasattr(lib, "pcs_range_point_merge_h")
    lib.pcs_abi_version.restype = ctypes.c_int32
    assert lib.pcs_abi_version() == 12 == native.ABI_VERSION
    assert "pcs_range_point_merge_f32" in native.SIGNATURES and "pcs_range_point_merge_h" in native.SIGNATURES
    assert hasattr(native.HipBackend, "range_point_merge") and hasattr(cpu_fallback.TorchCpuBackend, "range_point_merge")


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("bn", [True, False], ids=["bn", "add"])
def test_reference_is_grid_sample_index_arithmetic_and_batch_norm_in_float64(hw, bn):
    """The float64 side against torch in float64: grid_sample(bilinear, zeros, align_corners=False) per frame, the corner gather
    as index arithmetic, batch_norm with given statistics. Dyadic coordinates (4, 8): the float32 corner weights are exact, 1e-12 T;
    (5, 7): they carry float32 roundings of ix and of the products (2^-21 of a weight's scale), 1e-5 (1 + max |img|)."""
    n, c, eps = 65, 32, 1e-5
    k = case(n, c, hw)
    v64, l64 = k["vox"].astype(np.float64), k["lin"].astype(np.float64)
    var = np.random.default_rng(5).uniform(0.3, 2.0, size=c)
    stat = np.concatenate([k["stat"][:c], 1.0 / np.sqrt(var + eps)])
    ref, bn64, T = R.merge64(v64, k["idx8"], k["w8"], k["img"], k["pxpy"], l64, *((stat, k["gamma"], k["beta"]) if bn else ()))
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    idx = torch.from_numpy(k["idx8"]).long()
    w = torch.where(idx >= 0, t64(k["w8"]), torch.zeros((), dtype=torch.float64))
    gather = (w.unsqueeze(-1) * t64(v64)[idx.clamp(min=0)]).sum(1)
    img, p = t64(k["img"]), t64(k["pxpy"])
    samp = torch.zeros((n, c), dtype=torch.float64)
    for b in range(B):
        sel = p[:, 0] == b
        s = torch.nn.functional.grid_sample(img[b:b + 1], p[sel][:, 1:].reshape(1, 1, -1, 2), mode="bilinear", padding_mode="zeros",
                                            align_corners=False)
        samp[sel] = s.reshape(c, -1).t()
    if bn:
        third = torch.relu(torch.nn.functional.batch_norm(t64(l64), t64(stat[:c]), t64(var), t64(k["gamma"]), t64(k["beta"]), False, 0.0, eps))
    else:
        third = t64(l64)
    want = (gather + samp + third).numpy()
    tol = 1e-12 * T if hw == (4, 8) else 1e-5 * (1 + np.abs(k["img"]).max())
    assert (np.abs(ref - want) <= tol).all(), float(np.abs(ref - want).max())
    if bn:   # the term before the ReLU, the quantity the mask checks read
        pre = torch.nn.functional.batch_norm(t64(l64), t64(stat[:c]), t64(var), t64(k["gamma"]), t64(k["beta"]), False, 0.0, eps).numpy()
        assert (np.abs(bn64 - pre) <= 1e-12 * T).all()


@pytest.mark.parametrize("c,bn", [(32, True), (96, True), (24, False), (4, False)])
def test_cpu_backend_against_float64(c, bn):
    """cpu_fallback's restatement (fp32 torch arithmetic, its own order of operations): within the bound of the fp32 kernel; the mask
    bits away from undecided gates."""
    be = cpu_fallback.TorchCpuBackend()
    for n in (1, 65):
        k = case(n, c, (4, 8), off_frames=True)
        out, mask, ref, bn64, T = run_backend(be, k, torch.float32, bn)
        check_bound(out, ref, T, torch.float32, "cpu n=%d c=%d" % (n, c))
        if bn:
            sure = np.abs(bn64) > 32 * 2.0 ** -24 * T
            assert (mask_bits(mask, c)[sure] == (bn64 > 0)[sure]).all()
        else:
            assert mask is None


def test_empty_input_and_argument_checks_without_a_device():
    """n == 0 returns 0 before any pointer is looked at; a dtype outside {1, 2} is PCS_EINVAL; c % 4 (fp32) / c % 8 (16 bits) and bn mode
    with c % 32 != 0 are PCS_EUNSUPPORTED; add mode with a gamma is PCS_EINVAL."""
    lib = native.load_library()
    N = None
    one = ctypes.c_void_p(16)   # a non-null `stat`: never dereferenced, the width check comes first
    assert lib.pcs_range_point_merge_f32(N, N, N, N, N, 2, 4, 8, N, N, N, N, 0, 64, N, N, N) == 0
    assert lib.pcs_range_point_merge_h(N, N, N, N, N, 2, 4, 8, N, N, N, N, 0, 64, 1, N, N, N) == 0
    assert lib.pcs_range_point_merge_h(N, N, N, N, N, 2, 4, 8, N, N, N, N, 0, 64, 3, N, N, N) == -1
    assert lib.pcs_range_point_merge_f32(N, N, N, N, N, 2, 4, 8, N, N, N, N, 0, 6, N, N, N) == -4
    assert b"pcs_range_point_merge_f32" in lib.pcs_last_error()
    assert lib.pcs_range_point_merge_h(N, N, N, N, N, 2, 4, 8, N, N, N, N, 0, 12, 2, N, N, N) == -4
    assert lib.pcs_range_point_merge_f32(N, N, N, N, N, 2, 4, 8, N, one, N, N, 0, 56, N, N, N) == -4
    assert b"multiple of 32" in lib.pcs_last_error()
    assert lib.pcs_range_point_merge_f32(N, N, N, N, N, 2, 4, 8, N, N, one, N, 0, 64, N, N, N) == -1
    assert lib.pcs_range_point_merge_f32(N, N, N, N, N, 0, 4, 8, N, N, N, N, 0, 64, N, N, N) == -1


def _seeded_bn(c, gamma, beta):
    bn = FusedBatchNorm(c)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
    return bn.train()


def _run_merge(bn, lin, vox, idx8, w8, img, pxpy, gout):
    lin, vox, img = (t.detach().clone().requires_grad_(True) for t in (lin, vox, img))
    out = fused.range_point_merge(bn, lin, vox, idx8, w8, img, pxpy)
    out.backward(gout)
    return out.detach(), lin.grad, vox.grad, img.grad, bn.weight.grad, bn.bias.grad


def _record_calls(monkeypatch, be, calls):
    orig = be.range_point_merge
    monkeypatch.setattr(be, "range_point_merge", lambda *a: (calls.append((a[5].shape[1], "bn" if a[6] is not None else "add")), orig(*a))[1])
    return orig


@pytest.mark.parametrize("c,mode", [(32, "bn"), (24, "add")])
def test_autograd_on_the_cpu_backend(monkeypatch, c, mode):
    """fused.range_point_merge on the pure-PyTorch backend, switch on against off: the same function (torch's own float32 order of
    operations differs between the routes: 1e-5), routed as the width says; eval mode reads the running statistics."""
    n = 65
    k = case(n, c, (5, 7))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    gout = t(np.random.default_rng(3).normal(size=(n, c)).astype(np.float32))
    got = {}
    with cpu_fallback.enabled() as be:
        for switch in ("1", "0"):
            monkeypatch.setenv("PCS_RANGE_MERGE", switch)
            calls = []
            orig = _record_calls(monkeypatch, be, calls)
            bn = _seeded_bn(c, k["gamma"], k["beta"])
            got[switch] = _run_merge(bn, t(k["lin"]), t(k["vox"]), t(k["idx8"]), t(k["w8"]), t(k["img"]), t(k["pxpy"]), gout) + (
                bn.running_mean.clone(), bn.running_var.clone())
            monkeypatch.setattr(be, "range_point_merge", orig)
            assert calls == ([(c, mode)] if switch == "1" else []) and int(bn.num_batches_tracked) == 1
        for a, b, what in zip(got["1"], got["0"], ("out", "dlin", "dvox", "dimg", "dgamma", "dbeta", "running_mean", "running_var")):
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-5), what
        monkeypatch.setenv("PCS_RANGE_MERGE", "1")
        bn = _seeded_bn(c, k["gamma"], k["beta"]).eval()
        with torch.no_grad():
            bn.running_mean.copy_(t(k["stat"][:c]).float())
            bn.running_var.copy_((1.0 / t(k["stat"][c:]) ** 2 - bn.eps).float())
            out = fused.range_point_merge(bn, t(k["lin"]), t(k["vox"]), t(k["idx8"]), t(k["w8"]), t(k["img"]), t(k["pxpy"]))
        rm, rv = bn.running_mean.double().numpy(), bn.running_var.double().numpy()
        ref, _, T = R.merge64(k["vox"].astype(np.float64), k["idx8"], k["w8"], k["img"], k["pxpy"], k["lin"].astype(np.float64),
                              np.concatenate([rm, 1 / np.sqrt(rv + bn.eps)]), k["gamma"], k["beta"])
        assert (np.abs(out.numpy() - ref) <= 1e-5 * (1 + T)).all() and int(bn.num_batches_tracked) == 0


# ---- GPU: the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hw", HWS, ids=["4x8", "5x7"])
@pytest.mark.parametrize("n", NS)
def test_fp32_is_bit_identical_to_the_five_kernel_sequence(hip, n, hw):
    for c in C_F32_ONLY + C_ADD + C_BN:
        k = {name: dev(a) for name, a in case(n, c, hw, off_frames=True).items()}
        base = hip.devoxelize_fwd(k["vox"], k["idx8"], k["w8"]) + hip.range_sample_fwd(k["img"], k["pxpy"])
        out, mask = hip.range_point_merge(k["vox"], k["idx8"], k["w8"], k["img"], k["pxpy"], k["lin"], None, None, None)
        assert mask is None and torch.equal(out.view(torch.int32), (base + k["lin"]).view(torch.int32)), ("add", n, c, hw)
        if c % 32 == 0:
            y, ymask = hip.bn_apply(k["lin"], None, k["stat"], k["gamma"], k["beta"], True, want_mask=True)
            out, mask = hip.range_point_merge(k["vox"], k["idx8"], k["w8"], k["img"], k["pxpy"], k["lin"], k["stat"], k["gamma"], k["beta"])
            assert torch.equal(out.view(torch.int32), (base + y).view(torch.int32)), ("bn", n, c, hw)
            assert mask.shape == (n, c // 32) and mask.dtype == torch.int32 and torch.equal(mask, ymask), ("mask", n, c, hw)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", NS)
def test_kernel_against_float64(hip, n, dtype):
    """Check 2 of the module docstring, every element: dyadic coordinates on the (4, 8) image, frames of B and 0.5 included."""
    for c in widths(dtype):
        k = case(n, c, (4, 8), off_frames=True)
        for bn in ([False, True] if c % 32 == 0 else [False]):
            out, mask, ref, bn64, T = run_backend(hip, k, dtype, bn, to=dev)
            assert out.dtype == dtype and out.shape == (n, c)
            check_bound(out, ref, T, dtype, "n=%d c=%d %s" % (n, c, "bn" if bn else "add"))
        if n >= 12:   # the rows of no frame (frames B and 0.5): the sample is 0 -- the same bits as with an image of zeros
            with_img = run_backend(hip, k, dtype, False, to=dev)[0]
            without = run_backend(hip, dict(k, img=np.zeros_like(k["img"])), dtype, False, to=dev)[0]
            assert torch.equal(with_img[10:12], without[10:12]) and not torch.equal(with_img, without)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [32, 96])
def test_mask_is_exact_on_representable_data(hip, c, dtype):
    """Small-integer lin, power-of-two gamma / invstd / mean / beta: bn(lin) is exact in fp32 (and its sign survives any storage
    rounding), so every mask bit is [bn64 > 0]; c = 96 crosses a channel chunk (64 + a tail of 32)."""
    for n in (65, 257):
        k = dict(case(n, c, (4, 8)))
        rng = np.random.default_rng(n + c)
        k["lin"] = rng.integers(-8, 9, size=(n, c)).astype(np.float32)
        k["stat"] = np.concatenate([rng.choice([-2.0, -0.5, 0.0, 0.5, 1.0], size=c), rng.choice([0.5, 1.0, 2.0], size=c)])
        k["gamma"] = rng.choice([-1.0, 0.5, 1.0, 2.0], size=c).astype(np.float32)
        k["beta"] = rng.choice([-1.0, -0.25, 0.0, 0.5], size=c).astype(np.float32)
        out, mask, ref, bn64, T = run_backend(hip, k, dtype, True, to=dev)
        assert (bn64 == 0).any() and (bn64 > 0).any() and (bn64 < 0).any()
        assert np.array_equal(mask_bits(mask, c), bn64 > 0), (n, c)
        check_bound(out, ref, T, dtype, "representable n=%d c=%d" % (n, c))


@pytest.mark.gpu
def test_return_codes(hip):
    n, c = 64, 32
    k = {name: dev(a) for name, a in case(n, c, (4, 8)).items()}
    p, lib = native._ptr, hip.lib
    out = torch.full((n, 64), 7.0, device="cuda")
    mask = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    head = (p(k["vox"]), p(k["idx8"]), p(k["w8"]), p(k["img"]), p(k["pxpy"]), B, 4, 8)

    def f32(head, lin, stat, gamma, beta, c, out_, mask_):
        return lib.pcs_range_point_merge_f32(*head, lin, stat, gamma, beta, n, c, out_, mask_, native._stream())

    assert f32(head, p(k["lin"]), None, None, None, 6, p(out), None) == -4 and b"multiple of 4" in lib.pcs_last_error()
    assert lib.pcs_range_point_merge_h(*head, p(k["lin"]), None, None, None, n, 12, 1, p(out), None, native._stream()) == -4
    assert lib.pcs_range_point_merge_h(*head, p(k["lin"]), None, None, None, n, 32, 3, p(out), None, native._stream()) == -1
    assert f32(head, p(k["lin"]), p(k["stat"]), p(k["gamma"]), p(k["beta"]), 56, p(out), p(mask)) == -4
    assert b"multiple of 32" in lib.pcs_last_error()
    assert f32(head, p(k["lin"]), p(k["stat"]), p(k["gamma"]), p(k["beta"]), 32, p(out), None) == -1     # bn mode without a mask
    assert f32(head, p(k["lin"]), None, p(k["gamma"]), None, 32, p(out), None) == -1                     # add mode with a gamma
    # a row pointer 4 bytes off a 16-byte boundary: nothing launched
    buf = torch.zeros(n * c + 4, device="cuda")
    skew = buf[1:1 + n * c].view(n, c)
    assert skew.data_ptr() % 16 == 4
    assert f32(head, p(skew), None, None, None, c, p(out), None) == -4 and b"16-byte" in lib.pcs_last_error()
    assert f32((p(skew[:M]),) + head[1:], p(k["lin"]), None, None, None, c, p(out), None) == -4
    assert f32(head, p(k["lin"]), None, None, None, c, p(skew), None) == -4
    assert lib.pcs_range_point_merge_f32(*([None] * 5), B, 4, 8, None, None, None, None, 0, c, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 0).all()) and bool((mask == 0).all())
    with pytest.raises(RuntimeError):   # the Python entry refuses bn mode at c = 56 as the C entry does
        k56 = {name: dev(a) for name, a in case(n, 56, (4, 8)).items()}
        hip.range_point_merge(k56["vox"], k56["idx8"], k56["w8"], k56["img"], k56["pxpy"], k56["lin"], k56["stat"], k56["gamma"], k56["beta"])


# ---- GPU: autograd and routing ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c,mode", [(32, "bn"), (24, "add")])
def test_autograd_fp32_is_bit_identical_to_the_literal_sequence(hip, monkeypatch, c, mode):
    n, hw = 257, (5, 7)
    k = case(n, c, hw)
    gout = dev(np.random.default_rng(n).normal(size=(n, c)).astype(np.float32))
    got = {}
    be = native.backend()
    for switch in ("1", "0"):
        monkeypatch.setenv("PCS_RANGE_MERGE", switch)
        calls = []
        orig = _record_calls(monkeypatch, be, calls)
        bn = _seeded_bn(c, k["gamma"], k["beta"]).cuda()
        got[switch] = _run_merge(bn, dev(k["lin"]), dev(k["vox"]), dev(k["idx8"]), dev(k["w8"]), dev(k["img"]), dev(k["pxpy"]), gout) + (
            bn.running_mean.clone(), bn.running_var.clone())
        monkeypatch.setattr(be, "range_point_merge", orig)
        assert calls == ([(c, mode)] if switch == "1" else [])
    for a, b, what in zip(got["1"], got["0"], ("out", "dlin", "dvox", "dimg", "dgamma", "dbeta", "running_mean", "running_var")):
        assert a is not None and torch.equal(a, b), what
    # eval mode: the running statistics
    monkeypatch.setenv("PCS_RANGE_MERGE", "1")
    bn = _seeded_bn(c, k["gamma"], k["beta"]).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(dev(k["stat"][:c]).float())
        bn.running_var.copy_((1.0 / dev(k["stat"][c:]) ** 2 - bn.eps).float())
        out = fused.range_point_merge(bn, dev(k["lin"]), dev(k["vox"]), dev(k["idx8"]), dev(k["w8"]), dev(k["img"]), dev(k["pxpy"]))
    rm, rv = bn.running_mean.double().cpu().numpy(), bn.running_var.double().cpu().numpy()
    k4 = case(n, c, hw)
    ref, _, T = R.merge64(k4["vox"].astype(np.float64), k4["idx8"], k4["w8"], k4["img"], k4["pxpy"], k4["lin"].astype(np.float64),
                          np.concatenate([rm, 1 / np.sqrt(rv + bn.eps)]), k4["gamma"], k4["beta"])
    # general coordinates: the float32 weights may differ from the reference's by a contraction (2^-21 of a weight's scale)
    assert (np.abs(out.cpu().numpy() - ref) <= 32 * 2.0 ** -24 * T + 1e-5 * (1 + np.abs(k4["img"]).max())).all()
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("c", [32, 24])
def test_autograd_bf16(hip, monkeypatch, c):
    """bf16 leaves outside autocast on the dyadic image: every gradient finite and in the dtype of its leaf; the output inside the
    bound of check 2, the reference taking the batch statistics of the stored rows in float64. c = 24 (add mode): the fused
    BatchNorm pass stores its bf16 result before the kernel adds it, so half an ulp of that term joins the bound."""
    monkeypatch.setenv("PCS_RANGE_MERGE", "1")
    n, dtype = 257, torch.bfloat16
    k = case(n, c, (4, 8))
    vt, v64 = stored(k["vox"], dtype)
    lt, l64 = stored(k["lin"], dtype)
    gt, _ = stored(np.random.default_rng(n).normal(size=(n, c)).astype(np.float32), dtype)
    it, i64 = stored(k["img"], dtype)
    bn = _seeded_bn(c, k["gamma"], k["beta"]).cuda()
    calls = []
    _record_calls(monkeypatch, native.backend(), calls)
    out, dlin, dvox, dimg, dw, db = _run_merge(bn, dev(lt), dev(vt), dev(k["idx8"]), dev(k["w8"]), dev(it), dev(k["pxpy"]), dev(gt))
    assert calls == [(c, "bn" if c % 32 == 0 else "add")]
    assert out.dtype == dtype and dlin.dtype == dtype and dvox.dtype == dtype and dimg.dtype == dtype and dw.dtype == torch.float32
    assert all(bool(torch.isfinite(g).all()) for g in (out, dlin, dvox, dimg, dw, db))
    stat = np.concatenate([l64.mean(0), 1 / np.sqrt(l64.var(0) + bn.eps)])
    ref, bn64, T = R.merge64(v64, k["idx8"], k["w8"], i64.astype(np.float32), k["pxpy"], l64, stat, k["gamma"], k["beta"])
    lim = R.bound(ref, T, "bfloat16")
    if c % 32:
        lim = lim + R.ulp(np.maximum(bn64, 0.0) + 32 * 2.0 ** -24 * T, "bfloat16") / 2
    err = np.abs(out.float().cpu().numpy().astype(np.float64) - ref)
    print("[range merge] autograd bf16 c=%d: worst error / bound = %.3f" % (c, float((err / lim).max())))
    assert (err <= lim).all()


@pytest.mark.gpu
def test_routing(hip, monkeypatch):
    """(bn | add | literal) per width and switch; host tensors, another sampling mode, differing row dtypes and refused widths: literal."""
    n = 65
    be = native.backend()
    calls = []
    _record_calls(monkeypatch, be, calls)

    def route(c, switch="1", mode="bilinear", lin_dtype=torch.float32, host=False):
        k = case(n, c, (5, 7))
        to = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if host else dev
        monkeypatch.setenv("PCS_RANGE_MERGE", switch)
        del calls[:]
        bn = _seeded_bn(c, k["gamma"], k["beta"])
        bn = bn if host else bn.cuda()
        try:
            fused.range_point_merge(bn, to(k["lin"]).to(lin_dtype), to(k["vox"]), to(k["idx8"]), to(k["w8"]), to(k["img"]), to(k["pxpy"]), mode)
        except RuntimeError:
            assert host   # the HIP backend has no host path: the literal sequence was taken and refused the tensors
        return list(calls)

    assert route(32) == [(32, "bn")] and route(96) == [(96, "bn")] and route(448) == [(448, "bn")]
    assert route(24) == [(24, "add")] and route(56) == [(56, "add")] and route(4) == [(4, "add")]
    assert route(32, switch="0") == [] and route(24, switch="0") == []
    assert route(32, mode="nearest") == []
    assert route(32, lin_dtype=torch.bfloat16) == []   # lin bf16 beside fp32 vox
    assert route(32, host=True) == []
    k = case(n, 12, (5, 7))                              # 16-bit rows of 12 channels: the kernel refuses c % 8 != 0
    monkeypatch.setenv("PCS_RANGE_MERGE", "1")
    del calls[:]
    bn = _seeded_bn(12, k["gamma"], k["beta"]).cuda()
    with torch.no_grad():
        out = fused.range_point_merge(bn, dev(k["lin"]).half(), dev(k["vox"]).half(), dev(k["idx8"]), dev(k["w8"]), dev(k["img"]), dev(k["pxpy"]))
    assert calls == [] and bool(torch.isfinite(out).all())
