"""NumPy float64 restatement of RPVNet's range-point-voxel merge (csrc/rangemerge.hip, fused.range_point_merge):

    out[i, j] = sum_{k<8, idx8[i,k] >= 0} w8[i,k] vox[idx8[i,k], j]  +  sum_{corner q inside} w_q(i) img[b_i, j, y_q, x_q]  +  third[i, j]
    third     = max(0, (lin - mean) invstd gamma + beta)   (bn mode: stat given)      or      lin      (add mode: stat None)

The four bilinear corner weights are computed in float32 exactly as `corners_of` (csrc/range_corners.h) computes them --
ix = ((x + 1) W - 1) / 2 with every operation rounded to float32, the weights as products of two float32 differences -- and then
taken as exact numbers; everything else is float64. Also returned: the BatchNorm term before the ReLU (bn mode) and

    T = sum |w8 vox| + sum |w img| + |lin sc| + |mean sc| + |beta|          sc = invstd gamma      (add mode: T's third part is |lin|)

the magnitude the fp32 roundings of the chain are relative to. Not a test module: tests/test_range_merge.py imports it."""
import numpy as np

F32 = np.float32


def corner_table(pxpy, B, H, W):
    """-> (pixel (n, 4) int64 = (b H + y) W + x of the nw, ne, sw, se corner or -1 when the corner is outside the image or the frame
    is no integer in [0, B); weight (n, 4) float32)."""
    pxpy = np.asarray(pxpy, dtype=F32)
    fb, x, y = pxpy[:, 0], pxpy[:, 1], pxpy[:, 2]
    with np.errstate(invalid="ignore"):
        b = np.where(np.isfinite(fb), fb, -1).astype(np.int64)
        okf = (fb >= 0) & (b < B) & (b.astype(F32) == fb)
    ix = ((x + F32(1)) * F32(W) - F32(1)) / F32(2)
    iy = ((y + F32(1)) * F32(H) - F32(1)) / F32(2)
    assert ix.dtype == F32 and iy.dtype == F32
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + F32(1), y0 + F32(1)
    wts = np.stack([(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)], axis=1)
    assert wts.dtype == F32
    pix = np.full((len(fb), 4), -1, dtype=np.int64)
    for q, (xx, yy) in enumerate(((x0, y0), (x1, y0), (x0, y1), (x1, y1))):
        ok = okf & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        pix[ok, q] = (b[ok] * H + yy[ok].astype(np.int64)) * W + xx[ok].astype(np.int64)
    return pix, wts


def merge64(vox64, idx8, w8, img, pxpy, lin64, stat=None, gamma=None, beta=None):
    """vox64 (m, c), lin64 (n, c): the row tensors as stored, in float64; img (B, c, H, W), w8, pxpy, gamma, beta float32;
    stat = mean | invstd (2c float64) or None -> (out64 (n, c), bn64 (n, c) or None, T (n, c))."""
    B, c, H, W = img.shape
    ok = idx8 >= 0
    term = np.where(ok, w8.astype(np.float64), 0.0)[:, :, None] * vox64[np.maximum(idx8, 0)]
    pix, wts = corner_table(pxpy, B, H, W)
    rows = img.astype(np.float64).transpose(0, 2, 3, 1).reshape(B * H * W, c)
    samp = np.where(pix >= 0, wts.astype(np.float64), 0.0)[:, :, None] * rows[np.maximum(pix, 0)]
    T = np.abs(term).sum(1) + np.abs(samp).sum(1)
    base = term.sum(1) + samp.sum(1)
    if stat is None:
        return base + lin64, None, T + np.abs(lin64)
    mean, invstd = stat[:c], stat[c:]
    sc = invstd * (gamma.astype(np.float64) if gamma is not None else 1.0)
    b64 = beta.astype(np.float64) if beta is not None else np.zeros(c)
    bn = (lin64 - mean) * sc + b64
    T = T + np.abs(lin64 * sc) + np.abs(mean * sc) + np.abs(b64)
    return base + np.maximum(bn, 0.0), bn, T


FMT = {"float32": (23, -126), "bfloat16": (7, -126), "float16": (10, -14)}   # mantissa bits, smallest normal exponent


def ulp(v, fmt):
    """The spacing of the storage format `fmt` at |v| (subnormal spacing below the smallest normal)."""
    p, emin = FMT[fmt]
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.full(a.shape, float(emin))
    nz = a > 0
    e[nz] = np.maximum(np.floor(np.log2(a[nz])), emin)
    return 2.0 ** (e - p)


def bound(ref64, T, fmt):
    """|out - ref64| <= ulp_storage(|ref64| + e) / 2 + e, e = 32 * 2^-24 * T: 32 bounds the fp32 roundings of the chain (8 corner
    fused multiply-adds, at most 11 for the sample and its weights, 6 for the BatchNorm term, 2 adds); the store rounds the fp32
    value, which lies within e of ref64, to the nearest number of the storage format."""
    e = 32 * 2.0 ** -24 * T
    return ulp(np.abs(ref64) + e, fmt) / 2 + e
