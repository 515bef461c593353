"""Cylinder3D (Cylinder_TS) workload on the HIP operator API.

Architecture and state_dict layout of R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py:387-588 (so reference
checkpoints load): point MLP `PPmodel` (BatchNorm over the raw 9 point features, three Linear-BatchNorm-ReLU, a Linear) ->
scatter-max voxelisation (R:tools/utils/common/seg_utils.py:172-188) -> `fea_compression` -> ResContextBlock `downCntx` ->
four ResBlocks with a strided k3 `pool` (stride 2, 2, then (2, 2, 1) twice) -> four UpBlocks (`trans_dilao`, transposed
`up_subm`, skip add, three asymmetric convs) -> ReconBlock `ReconNet` -> concat -> k3 `logits` conv with bias -> point
refinement (`change_dim`, `point_logits`). Every block convolution is conv -> LeakyReLU -> BatchNorm: the slope rides in
the convolution's write-back and in the BatchNorm backward (`in_slope`), and the statistics come from the write-back where
the kernel emits them -- the fusions block_fusion.py applies to the reference's own blocks. The ReconBlock gate

    out = x * (sigmoid(bn0(conv3x1x1(x))) + sigmoid(bn0_2(conv1x3x1(x))) + sigmoid(bn0_3(conv1x1x3(x))))      (cylinder_ts.py:368-384)

is one kernel per direction behind the three convolutions (fused.recon_gate, csrc/recongate.hip); PCS_RECON_GATE=0 and widths
the kernel does not serve take the literal sequence. cy480 = init_size 32 (R:tools/cfgs/voxel/semantic_kitti/cylinder_cy480_cr10.yaml).
Inference: after `openpcseg_amd.freeze(model)` every block triple is ONE launch -- the BatchNorm's running statistics ride as a
per-column affine map behind the LeakyReLU, the residual behind that (inference.PostAffineConv) -- `up_subm` takes `+ skip` as
its addend and the point MLPs run with their BatchNorms folded into the Linear layers (inference.FoldedDense).
"""
import os

import numpy as np
import torch
from torch import nn

from .. import functional as F
from .. import fused, inference, native
from .. import modules as spnn
from ..fused import FusedBatchNorm
from ..hostdata import raw_frames
from ..linear import NOT_SERVED, row_linear
from ..scatter import scatter_max
from ..sparse import SparseTensor
from .losses import SegLoss

SLOPE = 0.01   # nn.LeakyReLU() of the reference's blocks
CYL_FUSED = os.environ.get("PCS_CYL_FUSED", "1") != "0"    # LeakyReLU in the convolution's write-back (A/B switch of block_fusion)
SKIP_FUSED = os.environ.get("PCS_SKIP_FUSED", "1") != "0"  # a block input's two gradients added in the dgrad write-back


def _linear(lin, x):
    """nn.Linear over point / voxel rows; on the device the weight gradient runs on the split-reduction kernel."""
    y = row_linear(x, lin.weight, lin.bias)
    return lin(x) if y is NOT_SERVED else y


def _dense_bn(bn, h, relu=False):
    """A FusedBatchNorm over plain (N, C) rows (the point MLPs): the fused statistics / apply passes."""
    return fused.bn_rows(bn, h, relu=relu)


def _cab(conv, bn, x, residual=None, want_skip=False, frozen=None):
    """conv -> LeakyReLU -> BatchNorm (+ residual) on a SparseTensor; -> (result, x routed through conv when want_skip).
    frozen: the triple's inference.PostAffineConv while the owner's folded path applies -- one launch, no BatchNorm."""
    if frozen is not None:
        y = frozen(x, residual=residual)
        return (y, x) if want_skip else y
    if CYL_FUSED and conv.bias is None and conv.kernel.dim() == 3 and F.conv_act_fusable(x.feats, conv.kernel):
        skip = want_skip and SKIP_FUSED and torch.is_grad_enabled() and x.feats.requires_grad
        out = F.conv3d(x, conv.kernel, kernel_size=conv.kernel_size, stride=conv.stride, dilation=conv.dilation,
                       transposed=conv.transposed, bn_stats=bn.training, with_skip=skip, act_slope=SLOPE)
        h, xs = out if skip else (out, x)
        y = bn(h, residual=residual, in_slope=SLOPE)
    else:
        h, xs = conv(x), x
        h.F = torch.nn.functional.leaky_relu(h.F, SLOPE)
        y = bn(h, residual=residual)
    return (y, xs) if want_skip else y


def _fold_triples(block):
    """openpcseg_amd.freeze: {conv name: inference.PostAffineConv} over the block's TRIPLES (conv, LeakyReLU, BatchNorm names), the
    record `_cab(frozen=)` reads. The ABI reads a slope of 0 as "no activation": only finite slopes > 0 are claimed."""
    rec = {}
    for cname, aname, bname in block.TRIPLES:
        conv, act, bn = getattr(block, cname), getattr(block, aname), getattr(block, bname)
        slope = float(act.negative_slope) if isinstance(act, nn.LeakyReLU) else float("nan")
        if inference._foldable(conv, bn) and np.isfinite(slope) and slope > 0:
            rec[cname] = inference.PostAffineConv(conv, bn, slope)
    return rec


def _conv(cin, cout, ks, stride=1, transposed=False, bias=False):
    return spnn.Conv3d(cin, cout, kernel_size=ks, stride=stride, bias=bias, transposed=transposed)


class ResContextBlock(nn.Module):       # cylinder_ts.py:88-155
    first, second = (1, 3, 3), (3, 1, 3)
    TRIPLES = (("conv1", "act1", "bn0"), ("conv1_2", "act1_2", "bn0_2"), ("conv2", "act2", "bn1"), ("conv3", "act3", "bn2"))

    def __init__(self, cin, cout, dist):
        super().__init__()
        self.conv1, self.act1, self.bn0 = _conv(cin, cout, self.first), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv1_2, self.act1_2, self.bn0_2 = _conv(cout, cout, self.second), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv2, self.act2, self.bn1 = _conv(cin, cout, self.second), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv3, self.act3, self.bn2 = _conv(cout, cout, self.first), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)

    def fold_records(self):
        rec = _fold_triples(self)
        return (rec, [f.bn for f in rec.values()]) if rec else None

    def forward(self, x):
        fz = (inference.active(self) or {}).get
        shortcut, xs = _cab(self.conv1, self.bn0, x, want_skip=True, frozen=fz("conv1"))
        shortcut = _cab(self.conv1_2, self.bn0_2, shortcut, frozen=fz("conv1_2"))
        res_a = _cab(self.conv2, self.bn1, xs, frozen=fz("conv2"))
        return _cab(self.conv3, self.bn2, res_a, residual=shortcut, frozen=fz("conv3"))


class ResBlock(ResContextBlock):        # cylinder_ts.py:158-250: the other order of the asymmetric pair, then `pool`
    first, second = (3, 1, 3), (1, 3, 3)

    def __init__(self, cin, cout, dist, height_pooling):
        super().__init__(cin, cout, dist)
        self.pool = _conv(cout, cout, 3, stride=2 if height_pooling else (2, 2, 1))

    def forward(self, x):
        res_a = super().forward(x)
        return self.pool(res_a), res_a


class UpBlock(nn.Module):               # cylinder_ts.py:253-334
    TRIPLES = (("trans_dilao", "trans_act", "trans_bn"), ("conv1", "act1", "bn1"), ("conv2", "act2", "bn2"), ("conv3", "act3", "bn3"))

    def __init__(self, cin, cout, dist, height_pooling):
        super().__init__()
        self.trans_dilao, self.trans_act, self.trans_bn = _conv(cin, cout, 3), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv1, self.act1, self.bn1 = _conv(cout, cout, (1, 3, 3)), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv2, self.act2, self.bn2 = _conv(cout, cout, (3, 1, 3)), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.conv3, self.act3, self.bn3 = _conv(cout, cout, 3), nn.LeakyReLU(), FusedBatchNorm(cout, sync=dist)
        self.up_subm = _conv(cout, cout, 3, stride=2 if height_pooling else (2, 2, 1), transposed=True)

    def fold_records(self):
        rec = _fold_triples(self)
        if isinstance(self.up_subm, spnn.Conv3d):
            rec["up_subm"] = inference.PostAffineConv(self.up_subm)   # + skip.F rides as the addend
        return (rec, [f.bn for f in rec.values() if f.bn is not None]) if rec else None

    def forward(self, x, skip):
        fz = (inference.active(self) or {}).get
        up_a = _cab(self.trans_dilao, self.trans_bn, x, frozen=fz("trans_dilao"))
        if fz("up_subm") is not None:
            up_a = fz("up_subm")(up_a, residual=skip.F)   # + skip in the convolution's write-back
        else:
            up_a = self.up_subm(up_a)
            up_a.F = up_a.F + skip.F
        up_e = _cab(self.conv1, self.bn1, up_a, frozen=fz("conv1"))
        up_e = _cab(self.conv2, self.bn2, up_e, frozen=fz("conv2"))
        return _cab(self.conv3, self.bn3, up_e, frozen=fz("conv3"))


class ReconBlock(nn.Module):            # cylinder_ts.py:337-384
    def __init__(self, cin, cout, dist):
        super().__init__()
        self.conv1, self.bn0, self.act1 = _conv(cin, cout, (3, 1, 1)), FusedBatchNorm(cout, sync=dist), nn.Sigmoid()
        self.conv1_2, self.bn0_2, self.act1_2 = _conv(cin, cout, (1, 3, 1)), FusedBatchNorm(cout, sync=dist), nn.Sigmoid()
        self.conv1_3, self.bn0_3, self.act1_3 = _conv(cin, cout, (1, 1, 3)), FusedBatchNorm(cout, sync=dist), nn.Sigmoid()
        for conv in (self.conv1, self.conv1_2, self.conv1_3):   # the statistics of the three conv outputs from their write-back
            conv.emit_bn_stats = os.environ.get("PCS_CONV_BN_STATS", "1") != "0"

    def forward(self, x):
        outs = [self.conv1(x), self.conv1_2(x), self.conv1_3(x)]
        return outs[0]._like(fused.recon_gate([self.bn0, self.bn0_2, self.bn0_3], outs, x))


def voxelize(z_feats, z_coords):
    """`voxelize(z)` of R:tools/utils/common/seg_utils.py:172-188: hash of the points' integer cells, unique with first index and
    inverse, count, scatter_max -> SparseTensor whose rows follow the sorted unique hashes. z_coords (N, 4) float, batch last."""
    icoords = z_coords.int()
    pc_hash = F.sphash(icoords)
    be = native.backend()
    if icoords.is_cuda and hasattr(be, "unique_inverse_csr"):
        sparse_hash, idx_query, _ = be.unique_inverse_csr(pc_hash)   # unique + inverse + count from one stable sort
    else:
        sparse_hash, idx_query = torch.unique(pc_hash, return_inverse=True)
    m, n = sparse_hash.shape[0], pc_hash.shape[0]
    # a voxel's representative: its first point (every point of a voxel carries the same integer coordinates)
    inds = torch.full((m,), n, dtype=torch.int64, device=pc_hash.device).scatter_reduce(
        0, idx_query, torch.arange(n, device=pc_hash.device), "amin")
    x = SparseTensor(scatter_max(z_feats, idx_query, dim=0, dim_size=m)[0], icoords[inds].contiguous(), 1)
    x.cmaps.setdefault(x.stride, x.coords)
    return x


class CylinderTS(nn.Module):
    def __init__(self, num_class=20, in_dim=9, init_size=32, point_refinement=True, dist=False, label_smoothing=0.0, ignore_label=0):
        super().__init__()
        s = init_size
        self.num_class, self.in_dim, self.init_size, self.point_refinement = num_class, in_dim, init_size, point_refinement
        norm = lambda c: FusedBatchNorm(c, sync=dist)
        self.PPmodel = nn.Sequential(norm(in_dim), nn.Linear(in_dim, 64), norm(64), nn.ReLU(), nn.Linear(64, 128), norm(128), nn.ReLU(),
                                     nn.Linear(128, 256), norm(256), nn.ReLU(), nn.Linear(256, 256))
        self.fea_compression = nn.Sequential(nn.Linear(256, 16), nn.ReLU())
        self.downCntx = ResContextBlock(16, s, dist)
        self.resBlock2 = ResBlock(s, 2 * s, dist, height_pooling=True)
        self.resBlock3 = ResBlock(2 * s, 4 * s, dist, height_pooling=True)
        self.resBlock4 = ResBlock(4 * s, 8 * s, dist, height_pooling=False)
        self.resBlock5 = ResBlock(8 * s, 16 * s, dist, height_pooling=False)
        self.upBlock0 = UpBlock(16 * s, 16 * s, dist, height_pooling=False)
        self.upBlock1 = UpBlock(16 * s, 8 * s, dist, height_pooling=False)
        self.upBlock2 = UpBlock(8 * s, 4 * s, dist, height_pooling=True)
        self.upBlock3 = UpBlock(4 * s, 2 * s, dist, height_pooling=True)
        self.ReconNet = ReconBlock(2 * s, 2 * s, dist)
        self.logits = _conv(4 * s, num_class, 3, bias=True)
        if point_refinement:
            self.change_dim = nn.Sequential(nn.Linear(4 * s, 256), norm(256), nn.LeakyReLU())
            self.point_logits = nn.Linear(256, num_class)
        self.criterion = SegLoss(ignore_index=ignore_label, label_smoothing=label_smoothing)          # CE + Lovasz on the voxels
        self.loss_funs = nn.CrossEntropyLoss(ignore_index=ignore_label, label_smoothing=label_smoothing)  # the point term
        # num_batches_tracked of all BatchNorm layers: one _foreach_add_ per training step
        self._bn_layers = [m for m in self.modules() if isinstance(m, FusedBatchNorm)]
        for m in self._bn_layers:
            m.counted_by_parent = True

    def fold_records(self):
        """openpcseg_amd.freeze: {"pp": PPmodel's three Linear layers with the four BatchNorms around them folded in (`_point_mlp`),
        "cd": change_dim's Linear with its BatchNorm (`forward`)}, each where the layout is the constructor's."""
        pp, cd, dense = self.PPmodel, getattr(self, "change_dim", None), inference.FoldedDense
        rec, norms = {}, []
        tracked = lambda bn: getattr(bn, "running_mean", None) is not None
        layout = [FusedBatchNorm, nn.Linear] + [FusedBatchNorm, nn.ReLU, nn.Linear] * 3
        if [type(l) for l in pp] == layout and all(tracked(pp[i]) for i in (0, 2, 5, 8)):
            rec["pp"] = [dense(pp[1], bn_in=pp[0], bn_out=pp[2]), dense(pp[4], bn_out=pp[5]), dense(pp[7], bn_out=pp[8])]
            norms += [pp[0], pp[2], pp[5], pp[8]]
        if cd is not None and len(cd) == 3 and isinstance(cd[0], nn.Linear) and inference._is_norm(cd[1]) and tracked(cd[1]) \
                and isinstance(cd[2], nn.LeakyReLU):
            rec["cd"] = dense(cd[0], bn_out=cd[1])
            norms.append(cd[1])
        return (rec, norms) if rec else None

    def _point_mlp(self, x):
        pp = self.PPmodel
        rec = inference.active(self)
        if rec is not None and "pp" in rec:   # the four BatchNorms folded into the three Linear layers they surround
            h = x
            for lin in rec["pp"]:
                h = torch.relu(lin(h))
            return _linear(pp[10], h)
        h = _dense_bn(pp[0], x)
        for i in (1, 4, 7):
            h = _dense_bn(pp[i + 1], _linear(pp[i], h), relu=True)
        return _linear(pp[10], h)

    def _refine_rows(self, batch, up0e, voxel_hash):
        """The row of the voxel features every point receives in the point refinement, as cylinder_ts.py:539-542 takes it: the
        position of the point's voxel in `voxel_coord`, used as a row of the output tensor. The two orders differ (the dataset's
        quantisation order against the sorted hashes), so a point reads the features of ANOTHER voxel, possibly of another frame
        of the batch; the fixtures and the reference's checkpoints were made with exactly this pairing, and it is kept."""
        return F.sphashquery(F.sphash(batch["point_coord"].int()), voxel_hash)

    def forward(self, batch):
        """batch: the dict of the reference's collate_batch (point_feature (N, in_dim), point_coord (N, 4), voxel_coord (M, 4),
        voxel_label (M,), point_label (N,), offset) -> {"logits": voxel logits in the output tensor's row order, "logit_coords",
        "point_logits", and in train mode "loss"}."""
        if self.training and self._bn_layers:
            torch._foreach_add_([m.num_batches_tracked for m in self._bn_layers], 1)
        point_feature = self._point_mlp(batch["point_feature"])
        ret = voxelize(point_feature, batch["point_coord"].float())
        ret.F = torch.relu(_linear(self.fea_compression[0], ret.F))
        ret = self.downCntx(ret)
        down1c, down1b = self.resBlock2(ret)
        down2c, down2b = self.resBlock3(down1c)
        down3c, down3b = self.resBlock4(down2c)
        down4c, down4b = self.resBlock5(down3c)
        up4e = self.upBlock0(down4c, down4b)
        up3e = self.upBlock1(up4e, down3b)
        up2e = self.upBlock2(up3e, down2b)
        up1e = self.upBlock3(up2e, down1b)
        up0e = self.ReconNet(up1e)
        up0e.F = torch.cat((up0e.F, up1e.F.to(up0e.F.dtype)), 1)
        logits = self.logits(up0e).F
        out = {"logits": logits, "logit_coords": up0e.C}
        voxel_hash = None
        if self.point_refinement:
            voxel_hash = F.sphash(batch["voxel_coord"].int())
            from_voxel = up0e.F[self._refine_rows(batch, up0e, voxel_hash)]
            cd, rec = self.change_dim, inference.active(self)
            if rec is not None and "cd" in rec:
                from_voxel = torch.nn.functional.leaky_relu(rec["cd"](from_voxel), cd[2].negative_slope)
            else:
                from_voxel = torch.nn.functional.leaky_relu(_dense_bn(cd[1], _linear(cd[0], from_voxel)), cd[2].negative_slope)
            out["point_logits"] = _linear(self.point_logits, point_feature + from_voxel.to(point_feature.dtype))
        if self.training:
            if voxel_hash is None:
                voxel_hash = F.sphash(batch["voxel_coord"].int())
            target = batch["voxel_label"][F.sphashquery(F.sphash(up0e.C), voxel_hash)]
            loss = self.criterion(logits.float(), target.long())
            if self.point_refinement:
                loss = loss + self.loss_funs(out["point_logits"].float(), batch["point_label"].long())
            out["loss"] = loss
        return out

    def predict(self, batch, evaluator=None):
        """Evaluation forward + the voxel -> point mapping of cylinder_ts.py:572-586 for the whole batch at once: the batch index is
        part of the hash, so ONE query of the points against the logits' coordinates gives every point its row, and the arg-max of
        that row is taken by the prediction tail kernel (no per-frame host loop, no gathered (N, C) tensor). ->
        {"logits", "logit_coords", "point_predict": flat int64 device tensor, frame after frame, each cut to batch["num_points"]
        where given, "point_offset": its host offsets}. evaluator: a SegEvaluator that also counts batch["point_label"]."""
        if self.training:
            raise RuntimeError("CylinderTS.predict is an evaluation pass: call model.eval() first")
        with torch.inference_mode():
            out = self.forward(batch)
            logits = out["logits"].float().contiguous()
            pc = batch["point_coord"]
            rows = F.sphashquery(F.sphash(pc.int()), F.sphash(out["logit_coords"]))
            labels = batch["point_label"].long() if (evaluator is not None and batch.get("point_label") is not None) else None
            frame = pc[:, -1].long()
            num_points = inference.scene_sizes(batch.get("num_points"))
            if num_points is not None:
                counts = torch.bincount(frame, minlength=len(num_points))
                if sum(num_points) != pc.shape[0]:   # `[:num_points[idx]]`: a frame keeps the head of its points
                    start = torch.cumsum(counts, 0) - counts
                    keep = (torch.arange(pc.shape[0], device=pc.device) - start[frame]) < torch.tensor(num_points, device=pc.device)[frame]
                    rows = rows[keep]
                    labels = labels[keep] if labels is not None else None
                offsets = [0] + np.cumsum(num_points).tolist()
            else:
                offsets = [0] + torch.cumsum(torch.bincount(frame), 0).cpu().tolist()   # the one read-back of a batch without num_points
            be = native.backend()
            if not (logits.is_cuda and hasattr(be, "predict_points")):   # a backend without the tail kernel: the rows' arg-max on the host path
                pred = logits[rows].argmax(1)
                if evaluator is not None:
                    evaluator.last_offsets = offsets
            elif evaluator is not None:
                pred = evaluator.tail(logits, labels, offsets, inverse=rows.contiguous())
            else:
                pred, _ = be.predict_points(logits, inverse=rows.contiguous())
        return {"logits": logits, "logit_coords": out["logit_coords"], "point_predict": pred, "point_offset": offsets}


    def predict_tta(self, raw, space_min, space_max, grid_size, num_votes=10, evaluator=None, vote_chunk=None,
                    scale_range=(0.95, 1.05), rng=np.random, return_logits=False):
        """An evaluation of a raw batch resident in HBM under the reference's test-time augmentation of the cylinder dataset
        (`TTA: True`: R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:92-99 and :126-142, ten rotated and rescaled
        votes per frame, collated as ten scenes by collate_batch_tta). `transform.tta_params` draws the votes from `rng`,
        `cylinder.device_batch(labels=False)` builds `vote_chunk` of them at a time from one read of the scans (None: all votes in
        one forward), the eval forward runs over the chunk, ONE hash query of the chunk's points against `logit_coords` gives
        every point its global row (as `predict` does), and per vote one launch of the prediction tail adds softmax(that row)
        into ONE (n, num_class) fp32 tensor (`inference.vote_loop`, the loop of every model's voted evaluation). The reference's forward_ensemble hands out raw per-scene logits and leaves the summing
        to its caller; summing softmax rows is the rule `inference.predict_tta` follows, and it is kept here. The decision is the
        arg-max after the last vote; `evaluator` (a SegEvaluator) gets its confusion counts from that decision only, once per
        point. -> the keys of inference.predict_tta: {"pred" (n,) int64, "votes" (n, num_class) fp32, "point_offset": host frame
        boundaries, "params": the (num_votes * num_frames, 8) table drawn}, and with return_logits "logits": per vote the
        (voxels of that vote's scenes, num_class) fp32 logits, with "logit_coords": their (voxels, 4) cells, the scene
        vote * num_frames + frame in the last column."""
        from .. import cylinder, transform
        if self.training:
            raise RuntimeError("CylinderTS.predict_tta is an evaluation pass: call model.eval() first")
        nf, n = raw_frames(raw, "CylinderTS.predict_tta", "`predict` on a host-built batch")[3:]

        def logits_of(batch, v0, _):
            out = self.forward(batch)
            logits, lc = out["logits"].float().contiguous(), out["logit_coords"]
            rows = F.sphashquery(F.sphash(batch["point_coord"].int()), F.sphash(lc)).contiguous()

            def vote(j):
                def keep():   # the vote's logits by mask, their scene re-based from the chunk to the evaluation
                    mine = (lc[:, -1] >= j * nf) & (lc[:, -1] < (j + 1) * nf)
                    coords = lc[mine].clone()
                    coords[:, -1] += v0 * nf
                    return {"logits": logits[mine], "logit_coords": coords}
                return {"inverse": rows[j * n:(j + 1) * n]}, keep   # global rows of the logits: no offsets
            return logits, vote

        return inference.vote_loop(
            raw, "CylinderTS.predict_tta", num_votes, vote_chunk, evaluator, return_logits,
            lambda nf, nv: {"params": transform.tta_params(nf, nv, scale_range=scale_range, rng=rng)},
            lambda part, k: cylinder.device_batch(raw, space_min, space_max, grid_size, self.num_class, part["params"], votes=k, labels=False),
            logits_of)


def cylinder_batch(samples):
    """collate_batch of the reference's cylinder dataset (R:pcseg/data/dataset/semantickitti/semantickitti_cylinder.py:176-213)
    over the dicts `openpcseg_amd.cylinder.cylinder_sample` returns: the frame index becomes the last coordinate column."""
    def with_frame(key):
        return torch.cat([torch.cat([s[key], torch.full((s[key].shape[0], 1), i, dtype=s[key].dtype, device=s[key].device)], 1)
                          for i, s in enumerate(samples)])
    batch = {"point_feature": torch.cat([s["point_feature"] for s in samples]), "point_coord": with_frame("point_coord"),
             "voxel_coord": with_frame("voxel_coord"), "voxel_label": torch.cat([s["voxel_label"] for s in samples]),
             "point_label": torch.cat([s["point_label"] for s in samples]),
             "offset": torch.cumsum(torch.tensor([s["voxel_coord"].shape[0] for s in samples]), 0).int(),
             "num_points": np.array([int(s["point_feature"].shape[0]) for s in samples])}
    if all("inverse_map" in s for s in samples):
        batch["inverse_map"] = torch.cat([s["inverse_map"] for s in samples])
    return batch
