"""Linear over tall rows: y = x W^T + b where x is (N, C) with N in the millions and C, the output width, in the tens or hundreds --
the classifier, the point MLPs of SPVCNN / RPVNet / Cylinder3D, the re-classed stock nn.Linear of a fused model. hipBLASLt serves
these shapes badly (a handful of workgroups for the (C_in, C_out) weight gradient, 32x32x256 macro-tiles for the 480 -> 20
classifier), so they run on this package's convolution and weight-gradient kernels over the identity map. The 1x1x1 convolution is
the same idea inside conv3d's own autograd node (functional._PointwiseConv); the two share functional._rows_weight_grad, where their
padding policies stand side by side.

One owner for what every site needs ("Linear over tall rows"):
  tall_rows      which (N, C) rows the family serves; the width rules stand with the Function they belong to (`widths_ok`);
  half_dtype     which half dtype a call computes in;
  row_linear     dense forward and input gradient, split-reduction weight gradient (`_PointLinear`), or NOT_SERVED;
  parts_linear   the Linear over cat(parts, 1) as column blocks on the gather-GEMM (`_SkinnyLinearParts`), or NOT_SERVED;
  weight_block   a column block of a Linear weight as the (1, cin, cout) fp32 weights the gather-GEMM reads;
  FusedLinear    nn.Linear on the gather-GEMM (`_SkinnyLinear`), whole, in parts, or commuted in front of the devoxelisation
                 (`devoxelized_linear`).
`_SkinnyLinear` and `_SkinnyLinearParts` stay two Functions: under autocast with fp32 input they compute different things on
purpose -- the first casts and runs the 16-bit kernel, the second keeps an fp32 part in fp32 and sums in fp32."""
import torch
from torch import nn
from torch.autograd import Function

from . import functional as F
from . import native

MIN_ROWS = 4096
_ROW_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
NOT_SERVED = None   # what row_linear / parts_linear return for inputs they leave to the caller's own Linear

_POINT_MAPS = {}   # identity maps (row count, device) for callers with no cache of their own (re-classed stock modules, the
#                    workloads' point MLPs): one per step, shared by all of them
_POINT_MAPS_LIMIT, _MODULE_MAPS_LIMIT = 4, 8   # entries past which functional._identity_map starts the cache afresh


def tall_rows(x, min_rows=MIN_ROWS):
    """THE rule for "(N, C) rows this family serves": a 2-D device tensor of fp32 / bf16 / fp16 with rows >= 4096 (min_rows).
    min_rows=0 is passed by the two `_merge` sites of workloads/spvcnn.py and rpvnet.py alone, whose point MLPs have always taken
    `_PointLinear` at any row count (their small test shapes run the split-reduction weight gradient because of it)."""
    return isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 2 and x.dtype in _ROW_DTYPES and x.shape[0] >= min_rows


def half_dtype(tensors, autocast=True):
    """The half dtype a call over these tensors computes in, or None for fp32: the first dtype among them that is not fp32, else
    functional._amp_dtype of the first (the autocast dtype while autocast is on). autocast=False: `devoxelized_linear` and the
    frozen classifier compute in whatever dtype the voxel features arrive in -- the convolution that produced them has already
    followed autocast, and an fp32 tensor there is one its producer chose to keep in fp32."""
    for t in tensors:
        if t.dtype != torch.float32:
            return t.dtype
    return F._amp_dtype(tensors[0]) if autocast else None


def weight_block(weight, col=0, cin=None):
    """The column block [col, col + cin) of an nn.Linear weight (out, in) -- default: all of it -- as the (1, cin, out) fp32 weights
    of a K = 1 convolution."""
    w = weight.detach()
    if cin is not None:
        w = w[:, col:col + cin]
    return w.float().t().contiguous().unsqueeze(0)


class _PointLinear(Function):
    """y = x W^T + b over ~2 M point rows: forward and input gradient stay dense GEMMs (hipBLASLt through torch), the weight gradient
    x^T dy -- (C_in, C_out), contracted over every point -- runs on the split-reduction wgrad kernel (as functional._PointwiseConv)."""

    @staticmethod
    def widths_ok(cin, cout):
        """Any input width (the weight gradient zero-pads it: Cylinder_TS's first point layer is Linear(9, 64)); the output width
        in whole 16-byte pieces."""
        return cout % 4 == 0

    @staticmethod
    def forward(ctx, x, weight, bias):
        hd = F._amp_dtype(x)
        ctx.hd, ctx.has_bias, ctx.in_dtype = hd, bias is not None, x.dtype
        if hd is None:
            ctx.save_for_backward(x, weight)
            return torch.nn.functional.linear(x.float(), weight.float(), bias.float() if bias is not None else None)
        xh = x.to(hd)   # kept for the weight gradient: one conversion of the (N, C_in) rows instead of one per direction
        ctx.save_for_backward(xh, weight)
        return torch.nn.functional.linear(xh, weight.to(hd), bias.to(hd) if bias is not None else None)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        hd = ctx.hd
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = (dy.float().matmul(weight.float()) if hd is None else dy.to(hd).matmul(weight.to(hd))).to(ctx.in_dtype)
        if ctx.needs_input_grad[1]:
            gw = F._rows_weight_grad(x, dy, hd, _POINT_MAPS, _POINT_MAPS_LIMIT, pad_in=True).t().to(weight.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = dy.float().sum(0).to(weight.dtype)
        return gx, gw, gb


def row_linear(x, weight, bias, min_rows=MIN_ROWS):
    """x W^T + b through `_PointLinear`, or NOT_SERVED -- the caller then runs its own Linear (the re-classed stock module of a
    fused model cannot be called from here: it would come straight back)."""
    if not (tall_rows(x, min_rows) and _PointLinear.widths_ok(weight.shape[1], weight.shape[0])):
        return NOT_SERVED
    return _PointLinear.apply(x, weight, bias)


def _gather_gemm(be, x, w1, km, hd, kept=F._per_call, **kw):
    """x over the identity map km with the (1, cin, cout) weights w1 on the kernel family of this shape -> functional._run_conv's."""
    fam = F._conv_family(be, hd, x.is_cuda, w1.shape[1], w1.shape[2], 1, x3=False)
    return F._run_conv(be, fam, x, w1, km, hd, kept, **kw)


class _SkinnyLinear(Function):
    """y = x @ W^T + b for a tall-skinny problem (1.2 M rows, 480 -> 20 classes): hipBLASLt picks 32x32x256 /
    256x256x16 macro-tiles for it (forward 1.05 ms, dgrad 1.82 ms at 12-21 TFLOP/s). The fused conv kernels treat it
    as a K = 1 convolution over the identity map: forward + dgrad on the gather-GEMM, dW on the split-reduction wgrad."""

    @staticmethod
    def widths_ok(cin, cout):
        """The gather-GEMM moves rows in 16-byte pieces, in both directions: both widths (of every part, for the parts form)."""
        return cin % 4 == 0 and cout % 4 == 0

    @staticmethod
    def forward(ctx, x, weight, bias, km, hd=None):
        """km: the identity map of x's rows. hd: the half dtype of the call (`half_dtype`; the 16-bit MFMA kernel serves the forward
        when its shape rules allow)."""
        y, x, _ = _gather_gemm(native.backend(), x, weight_block(weight), km, hd, bias=bias.float() if bias is not None else None)
        ctx.save_for_backward(x, weight)
        ctx.km, ctx.hd, ctx.in_dtype = km, hd, x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        be = native.backend()
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = be.conv_gather_gemm(dy.float(), weight.detach().float().contiguous().unsqueeze(0), ctx.km)
        if ctx.needs_input_grad[1]:
            dw = F._weight_grad(be, x, dy, ctx.km, 0, x.dtype)[0].t().to(weight.dtype)
        if ctx.needs_input_grad[2]:
            db = dy.float().sum(0)
        return dx, dw, db, None, None


class _SkinnyLinearParts(Function):
    """y = cat(parts, 1) @ W^T + b without the concatenation: one gather-GEMM per column block of W, summed -- the
    classifier over [z1 | z2 | z3] (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:415-417) never materialises the
    (N, 480) tensor (2.8 GB written and read back per step at 1.4 M points) nor, in backward, the contiguous copies of
    its sliced gradient: every d(part) is written once, by its own launch."""

    @staticmethod
    def forward(ctx, weight, bias, km, hd, *parts):
        be = native.backend()
        wt = weight_block(weight)   # (1, in, out)
        saved, y, col = [], None, 0
        for i, x in enumerate(parts):
            cin = x.shape[1]
            b = bias.float() if (bias is not None and i == 0) else None
            # a part that ARRIVES in half runs on the 16-bit kernel; an fp32 part stays fp32 even under autocast: the
            # pass is HBM-bound, and casting first (read 4 + write 2 + read 2 bytes per element) costs twice the fp32 read
            hx = half_dtype((x,), autocast=False)
            # (1, cin, out): a contiguous row block; the sum stays fp32
            t, x, _ = _gather_gemm(be, x, wt[:, col:col + cin], km, hx, bias=b, rounded=False)
            y = t.float() if y is None else y.add_(t.float())
            saved.append(x)
            col += cin
        ctx.save_for_backward(weight, *saved)
        ctx.km, ctx.hd, ctx.has_bias = km, hd, bias is not None
        return y.to(hd) if hd is not None else y

    @staticmethod
    def backward(ctx, dy):
        be = native.backend()
        weight, parts = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dy32 = dy.contiguous().float()
        w = weight.detach().float()  # (out, in)
        grads, dws, col = [], [], 0
        for i, x in enumerate(parts):
            cin = x.shape[1]
            dx = None
            if ctx.needs_input_grad[4 + i]:
                dx = be.conv_gather_gemm(dy32, w[:, col:col + cin].contiguous().unsqueeze(0), ctx.km)
            grads.append(dx)
            if ctx.needs_input_grad[0]:
                dws.append(F._weight_grad(be, x, dy32, ctx.km, 0, x.dtype)[0].t())
            col += cin
        dw = torch.cat(dws, dim=1).to(weight.dtype) if ctx.needs_input_grad[0] else None
        db = dy32.sum(0) if (ctx.has_bias and ctx.needs_input_grad[1]) else None
        return (dw, db, None, None) + tuple(grads)


def parts_linear(weight, bias, parts, cache=None):
    """cat(parts, 1) W^T + b through `_SkinnyLinearParts`, or NOT_SERVED: every part a served tensor of a served width (the row floor
    on the first), the widths summing to the weight's. cache: a module's own dict of identity maps (FusedLinear._maps), default the
    process-wide one."""
    cout, cin = weight.shape
    if not (all(tall_rows(x, 0 if i else MIN_ROWS) and _SkinnyLinear.widths_ok(x.shape[1], cout) for i, x in enumerate(parts)) and
            sum(x.shape[1] for x in parts) == cin):
        return NOT_SERVED
    cache, limit = (_POINT_MAPS, _POINT_MAPS_LIMIT) if cache is None else (cache, _MODULE_MAPS_LIMIT)
    km = F._identity_map(parts[0].shape[0], parts[0].device, cache, limit)
    return _SkinnyLinearParts.apply(weight, bias, km, half_dtype(parts), *parts)


def devoxelized_linear(weight, col, xf, idx, wts, cache, memo=None, limit=None):
    """devoxelize(xf) @ W_i^T computed as devoxelize(xf @ W_i^T), W_i = weight[:, col : col + C_i] of an nn.Linear weight:
    trilinear devoxelisation is linear over the voxel features (fixed per-point weights), so it commutes with the classifier --
    the class scores are formed on the VOXELS (36 k / 329 k / 1.16 M rows of 256 / 128 / 96 channels -> num_class) and only
    num_class channels per point are interpolated, instead of interpolating 480 channels per point and contracting them there
    (2.7 GB of point features written, read by the classifier, and the same again as gradients in backward). Same function; the
    fp32 rounding order differs. xf (V, C_i) voxel features, idx / wts (N, 8) the points' corner map. The bias is added on the
    points by the caller: the weights of a point with missing corners do not sum to one. cache: dict that keeps the identity map
    of this row count (pass the tensor's per-forward `kmaps`: built once per level and step, freed with the step; a dict that
    outlives the step comes with its size `limit`).
    memo: forward only (inference.FoldedLinear) -- a dict the caller keeps for as long as this weight block is current; the
    (1, cin, cout) weights and their prepared half copies are made once in it. Same kernels on the same values."""
    cin, cout = xf.shape[1], weight.shape[0]
    if not (tall_rows(xf) and _SkinnyLinear.widths_ok(cin, cout)):
        v = torch.nn.functional.linear(xf.float(), weight[:, col:col + cin].float())
        return F.spdevoxelize(v.float(), idx, wts)
    km = F._identity_map(xf.shape[0], xf.device, cache, limit)
    hd = half_dtype((xf,), autocast=False)
    if memo is None:
        v = _SkinnyLinear.apply(xf, weight[:, col:col + cin], None, km, hd)
    else:
        w1 = F._memo(memo, "w", lambda: weight_block(weight, col, cin))
        v = _gather_gemm(native.backend(), xf, w1, km, hd, F._kept_in(memo))[0]
    return F.spdevoxelize(v.float(), idx, wts)


class FusedLinear(nn.Linear):
    """nn.Linear (same parameters / state_dict keys) whose fp32 device path runs on the fused conv kernels when the
    row count dwarfs the feature sizes and the shapes are 16-byte granular; anything else is nn.Linear."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__(in_features, out_features, bias)
        self._maps = {}  # identity maps by row count (a handful of distinct batch sizes per run)

    def forward(self, x):
        if not (tall_rows(x) and _SkinnyLinear.widths_ok(self.in_features, self.out_features)):
            return super().forward(x)
        km = F._identity_map(x.shape[0], x.device, self._maps, _MODULE_MAPS_LIMIT)
        return _SkinnyLinear.apply(x, self.weight, self.bias, km, half_dtype((x,)))

    def devoxelized_part(self, col, xf, idx, wts, cache=None):
        """One term of forward(cat([devoxelize(x_i) for i], 1)) = sum_i devoxelize(x_i @ W_i^T) + b, W_i = the column
        block [col, col + C_i) of the weight (`devoxelized_linear`). cache: a per-forward dict for the identity map of this row
        count (the tensor's `kmaps`); default: the module's own small cache."""
        if cache is None:
            return devoxelized_linear(self.weight, col, xf, idx, wts, self._maps, limit=_MODULE_MAPS_LIMIT)
        return devoxelized_linear(self.weight, col, xf, idx, wts, cache)

    def sum_devoxelized(self, terms):
        y = terms[0]
        for t in terms[1:]:
            y = y + t
        return y + self.bias if self.bias is not None else y

    def forward_parts(self, parts):
        """forward(torch.cat(parts, 1)) without building the concatenation (column blocks of the weight)."""
        parts = list(parts)
        y = parts_linear(self.weight, self.bias, parts, self._maps)
        return self.forward(torch.cat(parts, dim=1)) if y is NOT_SERVED else y
