"""Block fusion above the op boundary: BatchNorm + residual add + ReLU of the
reference's conv blocks as ONE forward apply pass and ONE backward apply pass over the voxel features.

`FusedBatchNorm` has the parameters / buffers / state_dict keys of nn.BatchNorm1d (and nn.SyncBatchNorm), so
reference checkpoints load; `sync=True` all-reduces the (sum, sum^2, count) vector over the default process group
between the statistics and the apply kernels -- SyncBatchNorm semantics, ONE small collective per layer and
direction on a dedicated process group, the global row count travelling inside the vector and staying on the device (R:pcseg/model/segmentor/voxel/minkunet/minkunet.py:23-25)."""
import torch
import torch.distributed as dist
from torch import nn
from torch.autograd import Function

from . import functional as F_
from . import native
from .sparse import SparseTensor
# Linear over tall rows lives in linear.py; these names stay importable from here, where they lived before (callers' imports, checkpoints'
# tooling): aliases, nothing is defined here
from .linear import FusedLinear, _SkinnyLinear, _SkinnyLinearParts, devoxelized_linear  # noqa: F401,E402


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _syncing(sync):
    """True when a sync-mode layer must exchange its statistics. PCS_SYNC_WORLD1=1 (test rig): also in a one-rank process
    group, so that the whole collective path -- dedicated communicator, all-reduce, device-resident count -- runs over
    RCCL on a box with a single GPU."""
    if not sync or not (dist.is_available() and dist.is_initialized()):
        return False
    import os
    return dist.get_world_size() > 1 or os.environ.get("PCS_SYNC_WORLD1") == "1"


_STATS_GROUP = {}


def _stats_group():
    """A process group of its own for the BatchNorm statistics. On the default group the tiny (<= 6 KB) statistics
    all-reduces of backward queue FIFO behind DDP's 25 MB gradient buckets on the same RCCL communicator and stream
    -- each of the 63 BN layers then waits for a bucket to cross the xGMI ring before it can normalise its gradient.
    A second communicator (high-priority stream on RCCL) lets them overtake. Two communicators issued concurrently
    rely on every rank issuing its collectives in the same order: graphs that differ per rank (find_unused_parameters,
    data-dependent branches) should set PCS_BN_GROUP=0, the safe fallback, which keeps everything on the default group."""
    import os
    if os.environ.get("PCS_BN_GROUP", "1") == "0":
        return None
    # bound to the default group OBJECT (held in the cache entry and compared with `is`: after destroy_process_group() +
    # re-init CPython may hand the new group the old one's address, so an id() key could return a dead communicator)
    default = dist.distributed_c10d._get_default_group()
    key = (dist.get_world_size(), dist.get_backend())
    hit = _STATS_GROUP.get(key)
    g = hit[1] if hit is not None and hit[0] is default else None
    if g is None:
        _STATS_GROUP.clear()
        kw = {}
        if dist.get_backend() == "nccl":
            try:
                kw["pg_options"] = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
            except Exception:
                pass
        try:
            g = dist.new_group(backend=dist.get_backend(), **kw)  # collective: every rank reaches its first BN layer
        except Exception:  # an older / stricter torch.distributed: the statistics stay on the default group
            try:
                g = dist.new_group(backend=dist.get_backend())
            except Exception:
                g = False
        _STATS_GROUP[key] = (default, g)
    return g or None


def _train_stat(be, x, pre, sync, eps, momentum, running_mean, running_var):
    """Training-mode statistics of one BatchNorm over the contiguous (n, c) tensor x -> (stat = mean | invstd, host count, device
    count or None); the running statistics are updated. pre: what the producing convolution handed over, or None."""
    n, c = x.shape
    # [sum x | sum x^2 | n]: handed over by the producing convolution (its write-back computed them), else one pass
    syncing = _syncing(sync)
    # an empty tensor (a rank without voxels): count read as 1, as the kernels read a zero device count
    count, count_dev, stat = float(max(n, 1)), None, None
    raw = pre is not None and pre.numel() != 2 * c + 1 and pre.numel() > 0 and pre.numel() % (2 * c) == 0
    if raw and not syncing and n > 0:
        # the producing convolution's per-tile partials: reduction and finalize in one launch (nothing to all-reduce)
        stat = be.bn_reduce_finalize(pre, c, n, eps, momentum, running_mean, running_var)
    elif raw:
        sums = be.bn_reduce_partials(pre, c, n)
    elif pre is not None and pre.numel() == 2 * c + 1:
        sums = pre.clone() if syncing else pre  # the all-reduce below works in place
    else:
        sums = be.bn_stats(x)
    if syncing:
        # ONE collective per layer and direction: the row count rides in the statistics vector and the global
        # count stays on the device (finalize / bwd_apply read it there) -- no count all-reduce, no host sync
        dist.all_reduce(sums, group=_stats_group())
        count_dev = sums[2 * c:]
    if stat is None:
        stat = be.bn_finalize(sums, count, eps, momentum, running_mean, running_var, count_dev=count_dev)
    return stat, count, count_dev


def _bn_sync(bn):
    return bool(getattr(bn, "sync", isinstance(bn, nn.SyncBatchNorm)))


def _running_stat(bn):
    """Eval mode's [mean | invstd] double vector, as the apply kernels read it."""
    inv = torch.rsqrt(bn.running_var.double() + bn.eps)
    return torch.cat([bn.running_mean.double(), inv]).contiguous()


def _handed_over(t):
    """(features, statistics the producing convolution handed over for exactly this tensor or None) of a SparseTensor / tensor.
    The statistics are used only for the very tensor they describe (same object, untouched since): `x.F = dropout(x.F)`,
    `x.feats += b` in between fall back to the statistics pass."""
    if not isinstance(t, SparseTensor):
        return t, None
    x, pre = t.feats, getattr(t, "bn_sums", None)
    if pre is not None:
        sums, of, ver = pre
        pre = sums if (of is x and x._version == ver) else None
    return x, pre


def _count_step(bn):
    """One training step on bn's num_batches_tracked, unless somebody counted it already: a model that bumps all its counters
    with one _foreach_add_ per step marks its layers `counted_by_parent` for good; block_fusion's root pre-forward hook marks
    the layers it counted `_pcs_bumped` for this one step, and the mark is taken off here."""
    if bn.__dict__.get("_pcs_bumped", False):
        bn.__dict__["_pcs_bumped"] = False
    elif not getattr(bn, "counted_by_parent", False):
        bn.num_batches_tracked.add_(1)


def _reduced(local, sync):
    """The backward sums the apply pass divides by the global count: the local ones, or in sync mode a copy all-reduced
    (the local ones stay as they are: DDP averages the parameter gradients formed from them)."""
    if not _syncing(sync):
        return local
    sums = local.clone()
    dist.all_reduce(sums, group=_stats_group())
    return sums


def _param_sums(local, dtype):
    """The local backward sums in the parameters' dtype (the HIP reduction leaves them in fp32 as well; else one cast)."""
    lw = getattr(local, "_pcs_f32", None)
    return lw if lw is not None and lw.dtype == dtype else local.to(dtype)


def _bn_backward(cfg, saved, dy, relu=True, has_res=False, in_slope=None):
    """The two backward passes of a BatchNorm [+ residual] [+ ReLU] -> (dx, dres, dweight, dbias). cfg = (count, sync);
    saved = (x, gate, stat, weight, count_dev); dy contiguous, or the left columns of a wider buffer (read through its row stride)."""
    be = native.backend()
    x, gate, stat, weight, count_dev = saved
    count, sync = cfg
    c = x.shape[1]
    local = be.bn_bwd_stats(dy, x, gate, stat, relu)
    kw = {} if in_slope is None else {"in_slope": in_slope}
    dx, dres = be.bn_bwd_apply(dy, x, gate, stat, _reduced(local, sync), count, weight, relu, has_res, count_dev=count_dev, **kw)
    dw = db = None
    if weight is not None:
        lw = _param_sums(local, weight.dtype)
        dw, db = lw[c:], lw[:c]
    return dx, dres, dw, db


class _FusedBN(Function):
    """Feature tensors may be fp32, bf16 or fp16 (mixed precision: the half convolutions hand on halfs); statistics,
    scale / shift and running stats are fp32 / double whatever the storage format."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, running_mean, running_var, eps, momentum, relu, sync, pre=None, tail=None, in_slope=None):
        """in_slope: x is the output of a LeakyReLU that the producing convolution applied in its write-back; the gradient this
        node returns for x is then the gradient of the PRE-activation (the derivative rides in the backward apply pass), which is
        what that convolution's backward expects (functional._SparseConv, act_slope).
        tail (n, ct): concat fusion -- the output is cat([bn(x), tail], 1), the BN result written straight into the left
        columns and `tail` copied to the right ones by the apply launch (no torch.cat pass); backward reads its dy out of
        the gradient of that buffer through a row stride and hands the right columns on as tail's gradient."""
        be = native.backend()
        x = x.contiguous()
        res = res.contiguous() if res is not None else None
        n, c = x.shape
        stat, count, count_dev = _train_stat(be, x, pre, sync, eps, momentum, running_mean, running_var)
        # c % 32 == 0: the backward passes read the ReLU gate as a bit mask (1/32 of a tensor) instead of y
        if relu and c % 32 == 0 and c % 4 == 0:
            y, gate = be.bn_apply(x, res, stat, weight, bias, relu, want_mask=True, tail=tail)
        else:
            y = be.bn_apply(x, res, stat, weight, bias, relu, tail=tail)
            gate = (y if tail is None else y[:, :c].contiguous()) if relu else None
        ctx.save_for_backward(x, gate, stat, weight, count_dev)
        ctx.cfg = (count, sync)
        ctx.flags = (relu, res is not None, tail is not None, in_slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        relu, has_res, has_tail, in_slope = ctx.flags
        dtail = None
        if has_tail:
            c = ctx.saved_tensors[0].shape[1]
            dtail = dy[:, c:]   # the skip tensor's gradient: a view, summed into its other gradients by autograd
            dy = dy[:, :c]      # read in place through the row stride
        else:
            dy = dy.contiguous()
        dx, dres, dw, db = _bn_backward(ctx.cfg, ctx.saved_tensors, dy, relu, has_res, in_slope)
        return dx, dres, dw, db, None, None, None, None, None, None, None, dtail, None


def bn_rows(bn, x, residual=None, relu=False, tail=None, pre=None, in_slope=None):
    """`relu(bn(x) + residual)` [with `tail` concatenated on the right] over plain (N, C) tensors, on the parameters / buffers of
    any BatchNorm1d-shaped module: the ONE way into the fused passes. Training mode counts the step (`_count_step`) and uses
    the batch statistics -- `pre`: what the producing convolution handed over for x -- all-reduced for a sync layer (`_bn_sync`);
    eval mode applies the running statistics. in_slope, tail: `_FusedBN.forward`."""
    if bn.training:
        _count_step(bn)
        return _FusedBN.apply(x, residual, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu,
                              _bn_sync(bn), pre, tail, in_slope)
    return native.backend().bn_apply(x.contiguous(), residual.contiguous() if residual is not None else None, _running_stat(bn),
                                     bn.weight, bn.bias, relu, tail=tail.contiguous() if tail is not None else None)


def bn_forward(bn, input, residual=None, relu=False, cat_with=None, in_slope=None):
    """`relu(bn(input) + residual)` [concatenated with cat_with] over SparseTensor features as one fused pass, on the parameters /
    buffers of `bn`: a FusedBatchNorm (whose forward this is) or the caller's own nn.BatchNorm1d / nn.SyncBatchNorm
    (block_fusion; BatchNorm1d semantics in train and eval mode, SyncBatchNorm: the statistics are all-reduced over the whole job).
    cat_with: a SparseTensor / tensor on the same coordinates; the result then carries cat([bn(x), cat_with], 1) (torchsparse.cat
    of the reference's decoder, fused into the apply pass). in_slope: the input is the output of a LeakyReLU that the producing
    convolution applied in its write-back (`_FusedBN.forward`). A residual of another dtype is cast to the features'."""
    x, pre = _handed_over(input)
    r = residual.feats if isinstance(residual, SparseTensor) else residual
    tail = cat_with.feats if isinstance(cat_with, SparseTensor) else cat_with
    if tail is not None and (x.shape[1] % 4 or tail.shape[1] % 4 or tail.shape[0] != x.shape[0] or tail.dtype != x.dtype):
        # the concat-fused apply pass moves 16-byte pieces of one dtype: other widths (the cr 1.6 configs: 409 + 204 ...) concatenate with torch
        y = bn_forward(bn, input, residual=residual, relu=relu)
        return y._like(torch.cat([y.feats, tail.to(y.feats.dtype)], dim=1))
    if r is not None and r.dtype != x.dtype:
        r = r.to(x.dtype)
    return input._like(bn_rows(bn, x, r, relu, tail, pre, in_slope))


class FusedBatchNorm(nn.Module):
    """BatchNorm over SparseTensor features with optional fused residual add and ReLU:
    `bn(x)`, `bn(x, relu=True)`, `bn(x, residual=r, relu=True)`, `bn(x, cat_with=skip)` (`bn_forward`)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, sync=False):
        super().__init__()
        self.num_features, self.eps, self.momentum, self.sync = num_features, eps, momentum, sync
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.counted_by_parent = False   # a model may bump all its counters with one _foreach_add_ per step

    def extra_repr(self):
        return "%d, eps=%g, momentum=%g, sync=%s" % (self.num_features, self.eps, self.momentum, self.sync)

    forward = bn_forward


# ---- the point-branch merges: SPVCNN's (voxel + point) and RPVNet's (voxel + range + point) ---------------------------------
_ROW_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _merge_enabled():
    import os
    return os.environ.get("PCS_POINT_MERGE", "1") != "0"   # A/B switch: 0 = the literal three-op sequence


def _range_merge_enabled():
    import os
    return os.environ.get("PCS_RANGE_MERGE", "1") != "0"   # A/B switch: 0 = the literal sequence of the existing passes


def _grid_sample_rows(feature_map, pxpy, grid_sample_mode="bilinear"):
    """range_to_point for inputs the kernels do not serve (host tensors, other sampling modes): torch's grid_sample frame by
    frame, rows grouped by ascending frame (what R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:31-51 computes)."""
    rows = []
    for b in range(feature_map.shape[0]):
        grid = pxpy[pxpy[:, 0] == b][:, 1:].to(feature_map.dtype).reshape(1, 1, -1, 2)
        s = torch.nn.functional.grid_sample(feature_map[b:b + 1], grid, mode=grid_sample_mode, padding_mode="zeros", align_corners=False)
        rows.append(s.reshape(feature_map.shape[1], -1).t())
    return torch.cat(rows, dim=0)


class _Merge(Function):
    """out = devoxelize(vox) [+ range_sample(img, pxpy)] + third in ONE kernel: csrc/pointmerge.hip without an image (SPVCNN,
    R:pcseg/model/segmentor/fusion/spvcnn/spvcnn.py:417-418, 430-431, 443-444), csrc/rangemerge.hip with one (RPVNet,
    R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:648-651, 665-668, 683-686, 701-704). bn_mode: third = relu(bn(lin)) with
    training-mode statistics -- statistics, all-reduce and running statistics as `_FusedBN`, the gate the bit mask the kernel
    wrote; otherwise (range kernel only) third = lin, the finished term. No backward kernel: the gradient of `out` is the dy of
    the BatchNorm backward passes (bn mode; else lin's gradient itself), the gout of the devoxelize backward through the CSR
    cached on the corner map, and the gout of the range_sample backward through the pixel CSR cached on pxpy."""

    @staticmethod
    def forward(ctx, lin, vox, idx8, w8, img, pxpy, weight, bias, running_mean, running_var, eps, momentum, sync, bn_mode):
        be = native.backend()
        lin, vox = lin.contiguous(), vox.contiguous()
        idx8, w8 = idx8.contiguous().int(), w8.contiguous().float()
        stat = None
        if bn_mode:
            stat, count, count_dev = _train_stat(be, lin, None, sync, eps, momentum, running_mean, running_var)
            ctx.cfg = (count, sync)
        if img is None:
            out, mask = be.point_merge(vox, idx8, w8, lin, stat, weight, bias)
            ctx.maps = (idx8, w8, vox.shape[0], vox.dtype, None, None, None, lin.dtype)
        else:
            pxpy = pxpy.float().contiguous()
            # the image is sampled in fp32 (rangelib._RangeToPoint)
            out, mask = be.range_point_merge(vox, idx8, w8, img.float().contiguous(), pxpy, lin, stat, weight, bias)
            ctx.maps = (idx8, w8, vox.shape[0], vox.dtype, pxpy, tuple(img.shape), img.dtype, lin.dtype)
        if bn_mode:
            ctx.save_for_backward(lin, mask, stat, weight, count_dev)
        ctx.bn_mode = bn_mode
        return out

    @staticmethod
    def backward(ctx, g):
        be = native.backend()
        g = g.contiguous()
        idx8, w8, m, vox_dtype, pxpy, img_shape, img_dtype, lin_dtype = ctx.maps
        dlin = dvox = dimg = dw = db = None
        if ctx.bn_mode:
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[6] or ctx.needs_input_grad[7]:
                dlin, _, dw, db = _bn_backward(ctx.cfg, ctx.saved_tensors, g)
        elif ctx.needs_input_grad[0]:
            dlin = g if g.dtype == lin_dtype else g.to(lin_dtype)
        if ctx.needs_input_grad[1]:
            dvox = be.devoxelize_bwd(g, idx8, w8, m)
            if dvox.dtype != vox_dtype:
                dvox = dvox.to(vox_dtype)
        if ctx.needs_input_grad[4]:
            from . import rangelib
            if rangelib._PENDING:
                rangelib.verify_pending()
            dimg = be.range_sample_bwd(g.float().contiguous(), pxpy, img_shape[0], img_shape[2], img_shape[3])
            if dimg.dtype != img_dtype:
                dimg = dimg.to(img_dtype)
        return dlin, dvox, None, None, dimg, None, dw, db, None, None, None, None, None, None


def _merge_kernel_serves(be, lin_out, vox_feats, idx8, w8, feature_map=None, pxpy=None, grid_sample_mode="bilinear"):
    """The inputs csrc/pointmerge.hip (feature_map None) or csrc/rangemerge.hip (or the backend's restatement of them) takes;
    everything else is the literal sequence. The two kernels differ, and the differences are stated here and nowhere else:
      * each has its own switch (PCS_POINT_MERGE, PCS_RANGE_MERGE);
      * the point kernel has no add mode: it needs c % 32 == 0 (the ReLU mask is made of whole words), where the range kernel
        takes any width of whole 16-byte pieces and `_merge` runs the BatchNorm pass first when c % 32 != 0;
      * the point kernel takes vox and lin in differing row dtypes (the backend casts up to fp32); the range kernel refuses them,
        and the literal sequence promotes as torch does.
    Both take host tensors on the CPU backend and device tensors on the HIP backend, never a mixture, and no empty input (the
    literal sequence reads an empty shard's count as 1, `_train_stat`)."""
    ranged = feature_map is not None
    if ranged:
        if not (_range_merge_enabled() and hasattr(be, "range_point_merge") and grid_sample_mode == "bilinear"):
            return False
    elif not (_merge_enabled() and hasattr(be, "point_merge")):
        return False
    cpu = getattr(be, "name", "") == "torch-cpu"
    tensors = (lin_out, vox_feats, idx8, w8) + ((feature_map, pxpy) if ranged else ())
    if not (all(not t.is_cuda for t in tensors) if cpu else all(t.is_cuda for t in tensors)):
        return False   # host tensors on the HIP backend, or a mixture
    if lin_out.dim() != 2 or vox_feats.dim() != 2:
        return False
    n, c = lin_out.shape
    if n == 0 or vox_feats.shape[1] != c or lin_out.dtype not in _ROW_DTYPES or vox_feats.dtype not in _ROW_DTYPES:
        return False
    if not ranged:
        return c % 32 == 0
    if feature_map.dim() != 4 or pxpy.dim() != 2 or pxpy.shape[1] != 3:
        return False
    if feature_map.shape[1] != c or pxpy.shape[0] != n or not pxpy.is_floating_point():
        return False
    if lin_out.dtype != vox_feats.dtype or feature_map.dtype not in _ROW_DTYPES:
        return False   # row dtypes that differ: the literal sequence promotes them as torch does
    if c % (4 if lin_out.dtype == torch.float32 else 8):
        return False   # the widths the kernel refuses (rows move in 16-byte pieces)
    from . import rangelib
    return rangelib._frames_in_order(pxpy, feature_map.shape[0])


def _merge(bn, lin_out, vox_feats, idx8, w8, feature_map=None, pxpy=None, grid_sample_mode="bilinear"):
    """`point_merge` (feature_map None) and `range_point_merge`."""
    be = native.backend()
    fused = _merge_kernel_serves(be, lin_out, vox_feats, idx8, w8, feature_map, pxpy, grid_sample_mode)
    if fused and lin_out.shape[1] % 32 == 0:   # BatchNorm apply, ReLU and mask inside the kernel
        if bn.training:
            _count_step(bn)
            return _Merge.apply(lin_out, vox_feats, idx8, w8, feature_map, pxpy, bn.weight, bn.bias, bn.running_mean,
                                bn.running_var, bn.eps, bn.momentum, _bn_sync(bn), True)
        maps = (vox_feats.contiguous(), idx8.contiguous().int(), w8.contiguous().float())
        if feature_map is None:
            return be.point_merge(*maps, lin_out.contiguous(), _running_stat(bn), bn.weight, bn.bias)[0]
        return be.range_point_merge(*maps, feature_map.float().contiguous(), pxpy.float().contiguous(), lin_out.contiguous(),
                                    _running_stat(bn), bn.weight, bn.bias)[0]
    if feature_map is None and not fused and not bn.training:   # this route has always gathered first in eval mode
        return F_.spdevoxelize(vox_feats, idx8, w8) + bn_rows(bn, lin_out, relu=True)
    y = bn_rows(bn, lin_out, relu=True)
    if fused:   # the range kernel's add mode
        return _Merge.apply(y, vox_feats, idx8, w8, feature_map, pxpy, None, None, None, None, None, None, False, False)
    if feature_map is None:
        return F_.spdevoxelize(vox_feats, idx8, w8) + y
    from . import rangelib
    r = rangelib.range_to_point(feature_map, pxpy, grid_sample_mode, fallback=_grid_sample_rows)
    return F_.spdevoxelize(vox_feats, idx8, w8) + r + y


def point_merge(bn, lin_out, vox_feats, idx8, w8):
    """`spdevoxelize(vox_feats, idx8, w8) + relu(bn(lin_out))`: SPVCNN's point-branch merge. bn: a FusedBatchNorm (or any
    BatchNorm1d-shaped module: weight, bias, running statistics, eps, momentum); lin_out (N, C) the point Linear's output;
    vox_feats (M, C); idx8 / w8 (N, 8) the points' corner map. One kernel when the backend has `point_merge`, C % 32 == 0 and
    the tensors are on the device (PCS_POINT_MERGE=0 switches it off); otherwise the literal sequence through the existing
    fused passes -- same function, and in fp32 the same bits. Eval mode: the running statistics."""
    return _merge(bn, lin_out, vox_feats, idx8, w8)


def range_point_merge(bn, lin_out, vox_feats, idx8, w8, feature_map, pxpy, grid_sample_mode="bilinear"):
    """`spdevoxelize(vox_feats, idx8, w8) + range_to_point(feature_map, pxpy) + relu(bn(lin_out))`: RPVNet's merge of its voxel,
    range and point branches. bn: a FusedBatchNorm (or any BatchNorm1d-shaped module); lin_out (N, C) the point Linear's output;
    vox_feats (M, C); idx8 / w8 (N, 8) the points' corner map; feature_map (B, C, H, W); pxpy (N, 3) = (frame, x, y), the frames
    non-decreasing integers in [0, B) (`rangelib.range_to_point`'s contract, verified the same way). One kernel when the backend
    has `range_point_merge` and serves the inputs: BatchNorm apply, ReLU and mask inside it when C % 32 == 0, otherwise the
    fused BatchNorm pass first and the kernel adds its output. PCS_RANGE_MERGE=0, a backend without the op, host tensors on the
    HIP backend, other sampling modes, differing row dtypes and refused widths take the literal sequence of the existing
    passes -- same function, and in fp32 the same bits. Eval mode: the running statistics."""
    return _merge(bn, lin_out, vox_feats, idx8, w8, feature_map, pxpy, grid_sample_mode)


# ---- Cylinder3D's ReconBlock gate ------------------------------------------------------------------------------------------
def _gate_enabled():
    import os
    return os.environ.get("PCS_RECON_GATE", "1") != "0"   # A/B switch: 0 = the literal sequence


class _ReconGate(Function):
    """out = x * (sigmoid(bn0(a0)) + sigmoid(bn1(a1)) + sigmoid(bn2(a2))) with training-mode statistics
    (R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:368-384): the three apply passes, the sigmoids, the adds and the
    multiply in ONE kernel per direction (csrc/recongate.hip). Statistics, all-reduce and running statistics per branch as
    `_FusedBN`; backward all-reduces the three branches' sums as one 6c vector. Only the forward's inputs are saved. The gradient
    returned for x is the one through the product; the one through the convolutions arrives by a0..a2."""

    @staticmethod
    def forward(ctx, x, a0, a1, a2, w0, b0, w1, b1, w2, b2, bns, pres):
        be = native.backend()
        x = x.contiguous()
        a3 = [a0.contiguous(), a1.contiguous(), a2.contiguous()]
        stats, count, count_dev = [], float(max(x.shape[0], 1)), None
        for bn, a, pre in zip(bns, a3, pres):
            stat, count, cd = _train_stat(be, a, pre, _bn_sync(bn), bn.eps, bn.momentum, bn.running_mean, bn.running_var)
            stats.append(stat)
            count_dev = cd if count_dev is None else count_dev   # the same global row count in every branch
        stat3 = torch.cat(stats)
        gamma3, beta3 = torch.cat([w0, w1, w2]).float(), torch.cat([b0, b1, b2]).float()
        out = be.recon_gate(a3, x, stat3, gamma3, beta3)
        ctx.save_for_backward(x, a3[0], a3[1], a3[2], stat3, gamma3, beta3, count_dev)
        ctx.cfg = (count, any(_bn_sync(bn) for bn in bns), w0.dtype, (x.dtype, a0.dtype, a1.dtype, a2.dtype))
        return out

    @staticmethod
    def backward(ctx, dy):
        be = native.backend()
        x, a0, a1, a2, stat3, gamma3, beta3, count_dev = ctx.saved_tensors
        count, sync, wdtype, in_dtypes = ctx.cfg
        c = x.shape[1]
        a3 = [a0, a1, a2]
        dy = dy.contiguous()
        local = be.recon_gate_bwd_stats(dy, x, a3, stat3, gamma3, beta3)
        sums2 = _reduced(local, sync)   # ONE collective for the three BatchNorms
        dx, da = be.recon_gate_bwd_apply(dy, x, a3, stat3, gamma3, beta3, sums2, count, count_dev=count_dev)
        lw = _param_sums(local, wdtype)
        wb = []
        for k in range(3):
            wb += [lw[(2 * k + 1) * c:(2 * k + 2) * c], lw[2 * k * c:(2 * k + 1) * c]]
        grads = [g if g.dtype == d else g.to(d) for g, d in zip([dx] + list(da), in_dtypes)]
        return (*grads, *wb, None, None)


def recon_gate(bns, conv_outs, x):
    """`x * (sigmoid(bns[0](conv_outs[0])) + sigmoid(bns[1](conv_outs[1])) + sigmoid(bns[2](conv_outs[2])))`: the ReconBlock gate of
    Cylinder3D -> (N, C) features. bns: three FusedBatchNorm (or BatchNorm1d-shaped) modules; conv_outs: the three convolutions'
    outputs, SparseTensors (whose write-back statistics are used where present) or (N, C) tensors; x: SparseTensor or tensor.
    One kernel per direction when the backend has `recon_gate`, the width is a multiple of 4 (fp32) / 8 (16 bits) and the rows
    are 16-byte aligned (PCS_RECON_GATE=0 switches it off); otherwise the literal sequence: three fused BatchNorm applies,
    torch.sigmoid, adds, multiply. Eval mode: the running statistics, same kernel."""
    be = native.backend()
    xf = x.feats if isinstance(x, SparseTensor) else x
    got = [_handed_over(t) for t in conv_outs]
    feats = [xf] + [a for a, _ in got]
    halfs = (torch.bfloat16, torch.float16)
    dt = xf.dtype if all(t.dtype == xf.dtype for t in feats) else torch.float32
    fused = (_gate_enabled() and hasattr(be, "recon_gate") and len(bns) == 3 and len(got) == 3 and
             all(t.dim() == 2 and t.shape == xf.shape and t.dtype in (torch.float32,) + halfs for t in feats) and
             xf.shape[1] % (8 if dt in halfs else 4) == 0 and
             (all(t.is_cuda for t in feats) or getattr(be, "name", "") == "torch-cpu") and
             all(t.data_ptr() % 16 == 0 or not t.is_contiguous() for t in feats) and
             all(bn.weight is not None and bn.bias is not None for bn in bns) and
             all(bn.training == bns[0].training for bn in bns))
    if fused and bns[0].training:
        for bn in bns:
            _count_step(bn)
        return _ReconGate.apply(xf, got[0][0], got[1][0], got[2][0], bns[0].weight, bns[0].bias, bns[1].weight, bns[1].bias,
                                bns[2].weight, bns[2].bias, list(bns), [pre for _, pre in got])
    if fused:
        stat3 = torch.cat([_running_stat(bn) for bn in bns])
        return be.recon_gate([a.contiguous() for a, _ in got], xf.contiguous(), stat3,
                             torch.cat([bn.weight for bn in bns]).float(), torch.cat([bn.bias for bn in bns]).float())
    gate = None
    for bn, (a, pre) in zip(bns, got):
        s = torch.sigmoid(bn_rows(bn, a, pre=pre))
        gate = s if gate is None else gate + s
    return gate * xf
