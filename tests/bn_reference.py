"""Plain float64 NumPy for every pass of the fused BatchNorm (include/pcseg_hip.h, the BatchNorm section), and the
elementwise error bounds the kernels of csrc/norm.hip are held to by tests/test_batchnorm_kernels.py.

Passes (x, res, dy: (n, c) float64; stat = mean | invstd, 2c; sums = sum x | sum x^2 | n; sums2 = sum g | sum g xhat):

    sums      the vector pcs_bn_stats_* leaves
    finalize  mean = S0 / count, var = max(S1 / count - mean^2, 0), invstd = 1 / sqrt(var + eps); running statistics with the
              unbiased variance var * count / (count - 1) when count > 1, the biased one otherwise; count <= 0 is read as 1
    apply     y = act((x - mean) * invstd * w + b [+ res]); mask bit (i, j) = [y > 0] of the STORED y, word i * c/32 + j/32,
              bit j % 32; concat: cat([y, tail], 1)
    bwd_stats g = dy * gate;  sums2 = sum g | sum g * xhat,  xhat = (x - mean) * invstd
    bwd_apply dx = (g - S0'/count - xhat * S1'/count) * invstd * w [* (x > 0 ? 1 : in_slope)], dres = g

Bounds, derived from the roundings on the kernels' paths (never from what the kernels give). u = 2^-24; u_s the unit
roundoff of the storage type as the tests state it: u (fp32), 2^-8 (bf16), 2^-11 (fp16), plus 2^-25 absolute in fp16 for a
result below the smallest subnormal's half; sc = invstd * w in float64.

  apply      the kernel forms sc = fl(fl(invstd) * w) (2 roundings), sh = fl(b - fl(fl(mean) * sc)) (mean's conversion, a
             product, a difference), t = fma(x, sc, sh) (1) and t + res (1). To first order the error is at most
             |x sc| (2 + 1 + 1) u + |mean sc| (1 + 2 + 1 + 1 + 1 + 1) u + |b| (1 + 1 + 1) u + |res| u, every coefficient <= 8
             once the later roundings are charged to each term; 10 u covers the second-order terms. The store adds
             u_s |y64|:
                 |y - y64| <= 10 u (|x sc| + |mean sc| + |b| + |res|) + u_s |y64|
  bwd_apply  xhat = fl(fl(x - fl(mean)) * fl(invstd)) (4), k1, k2 one conversion each, xhat * k2 (1), two subtractions (2),
             ws = fl(fl(invstd) * w) (2), the product (1), in_slope (1): at most 8 on any term,
                 |dx - dx64| <= 10 u (|g| + |k1| + (|x| + |mean|) invstd |k2|) |invstd w| [* max(1, in_slope)] + u_s |dx64|
             dres is g copied: exact.
  stats      a workgroup row-lane adds ceil(n / (1024 TY)) <= ceil(n / 1024) terms in fp32, the workgroup adds its TY <= 256
             lane sums in fp32, the rest is double: the longest fp32 chain is L = ceil(n / 1024) + 256 additions, plus the
             subtraction of the pivot p = row 0 (1) and the square (1, twice the relative error of x - p: 2 more):
                 |S0 - S0_64| <= (L + 2) u sum |x - p|
                 |S1 - S1_64| <= (L + 4) u sum (x - p)^2 + 2 |p| (bound on S0)
             for the RAW sums sum x, sum x^2: the un-shift S0 + n p, S1 + 2 p S0 + n p^2 is done in double.
  bwd_stats  the same chains over g and g * xhat; xhat carries 4 roundings and the product 1, the conversions of mean and
             invstd are charged to |mean| and invstd:
                 |s0 - s0_64| <= (L + 6) u sum |g|,   |s1 - s1_64| <= (L + 6) u sum |g| (|x| + |mean|) invstd

An element whose float64 pre-activation lies within its own apply bound of zero may take either ReLU gate: `unsure`.
"""
import numpy as np

U = 2.0 ** -24
U_S = {"fp32": U, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
ABS_S = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _split(stat):
    stat = _f64(stat)
    c = stat.size // 2
    return stat[:c], stat[c:]


# ---- the passes ---------------------------------------------------------------------------------------------------------
def sums(x):
    x = _f64(x)
    return np.concatenate([x.sum(0), (x * x).sum(0), [float(x.shape[0])]])


def finalize(sums_, count, eps, momentum=0.1, running_mean=None, running_var=None):
    """-> (stat, running_mean, running_var); the running statistics in float64 (the kernel stores them as fp32)."""
    s = _f64(sums_)
    c = s.size // 2
    count = float(count) if count > 0 else 1.0
    mean = s[:c] / count
    var = np.maximum(s[c:2 * c] / count - mean * mean, 0.0)
    stat = np.concatenate([mean, 1.0 / np.sqrt(var + eps)])
    if running_mean is None:
        return stat, None, None
    unb = var * count / (count - 1.0) if count > 1.0 else var
    return (stat, (1.0 - momentum) * _f64(running_mean) + momentum * mean,
            (1.0 - momentum) * _f64(running_var) + momentum * unb)


def preact(x, stat, w=None, b=None, res=None):
    x, w, b, res = _f64(x), _f64(w), _f64(b), _f64(res)
    mean, invstd = _split(stat)
    t = (x - mean) * invstd
    if w is not None:
        t = t * w
    if b is not None:
        t = t + b
    if res is not None:
        t = t + res
    return t


def apply(x, stat, w=None, b=None, res=None, relu=False, tail=None):
    y = preact(x, stat, w, b, res)
    if relu:
        y = np.maximum(y, 0.0)
    return y if tail is None else np.concatenate([y, _f64(tail)], axis=1)


def mask_words(y):
    """[y > 0] of an (n, c) array, c % 32 == 0, packed as the apply pass packs it: (n, c / 32) int32 words."""
    n, c = y.shape
    assert c % 32 == 0
    bits = (np.asarray(y) > 0).reshape(n, c // 32, 32).astype(np.uint64)
    return (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


def mask_bits(words, c):
    m = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    return ((m[:, :, None] >> np.arange(32)) & 1).reshape(m.shape[0], c).astype(bool)


def _gated(dy, gate):
    dy = _f64(dy)
    return dy if gate is None else dy * (np.asarray(gate) > 0)


def bwd_stats(dy, x, stat, gate=None):
    """gate: the ReLU output y (or anything whose sign pattern is [y > 0]); None without ReLU."""
    mean, invstd = _split(stat)
    g = _gated(dy, gate)
    return np.concatenate([g.sum(0), (g * ((_f64(x) - mean) * invstd)).sum(0)])


def bwd_apply(dy, x, stat, sums2, count, w=None, gate=None, in_slope=None):
    """-> (dx, dres)."""
    x, s2 = _f64(x), _f64(sums2)
    mean, invstd = _split(stat)
    c = mean.size
    count = float(count) if count > 0 else 1.0
    g = _gated(dy, gate)
    dx = (g - s2[:c] / count - (x - mean) * invstd * (s2[c:2 * c] / count)) * invstd
    if w is not None:
        dx = dx * _f64(w)
    if in_slope is not None:
        dx = dx * np.where(x > 0, 1.0, float(in_slope))
    return dx, g


# ---- storage types ------------------------------------------------------------------------------------------------------
def torch_dtype(name):
    import torch
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[name]


def rounded(a, name):
    """a (float64) rounded to the storage type and widened again."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch_dtype(name)).double().numpy()


def assert_representable(a, name, what=""):
    """A condition on the inputs of the exact cases: 100 % of the float64 values survive the storage type unchanged."""
    a = _f64(a)
    assert np.array_equal(rounded(a, name), a), "%s: not exactly representable in %s" % (what, name)


# ---- bounds -------------------------------------------------------------------------------------------------------------
def _absw(stat, w):
    _, invstd = _split(stat)
    return np.abs(invstd if w is None else invstd * _f64(w))


def apply_bound(x, stat, w, b, res, y64, name):
    mean, _ = _split(stat)
    sc = _absw(stat, w)
    a = np.abs(_f64(x)) * sc + np.abs(mean) * sc
    if b is not None:
        a = a + np.abs(_f64(b))
    if res is not None:
        a = a + np.abs(_f64(res))
    return 10 * U * a + U_S[name] * np.abs(y64) + ABS_S[name]


def unsure(x, stat, w, b, res, name):
    """Elements whose float64 pre-activation lies within its own bound of zero: either ReLU gate is right there."""
    t = preact(x, stat, w, b, res)
    return np.abs(t) <= apply_bound(x, stat, w, b, res, t, name)


def bwd_apply_bound(dy, x, stat, sums2, count, w, gate, in_slope, dx64, name):
    x, s2 = _f64(x), _f64(sums2)
    mean, invstd = _split(stat)
    c = mean.size
    g = np.abs(_gated(dy, gate))
    a = (g + np.abs(s2[:c] / count) + (np.abs(x) + np.abs(mean)) * invstd * np.abs(s2[c:2 * c] / count)) * _absw(stat, w)
    if in_slope is not None:
        a = a * max(1.0, float(in_slope))
    return 10 * U * a + U_S[name] * np.abs(dx64) + ABS_S[name]


def chain(n):
    """An upper bound on the longest fp32 addition chain of the statistics passes, every geometry."""
    return -(-n // 1024) + 256


def stats_bound(x):
    """-> bounds on |sum x - sum x_64| and |sum x^2 - sum x^2_64|, (c,) each."""
    x = _f64(x)
    n = x.shape[0]
    p = x[0] if n > 0 else np.zeros(x.shape[1])
    L = chain(n)
    b0 = (L + 2) * U * np.abs(x - p).sum(0)
    b1 = (L + 4) * U * ((x - p) ** 2).sum(0) + 2 * np.abs(p) * b0
    return b0, b1


def bwd_stats_bound(dy, x, stat, gate=None):
    mean, invstd = _split(stat)
    g = np.abs(_gated(dy, gate))
    L = chain(g.shape[0])
    return (L + 6) * U * g.sum(0), (L + 6) * U * (g * (np.abs(_f64(x)) + np.abs(mean)) * invstd).sum(0)
