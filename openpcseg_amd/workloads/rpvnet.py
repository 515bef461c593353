"""RPVNet (ResBlock variant) workload on the HIP operator API.

Architecture and state_dict layout of R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py:94-707 (so reference checkpoints
load): the MinkUNet trunk of workloads.minkunet (stem, stage1..4, up1..4, classifier), a point branch -- four
Linear-BatchNorm-ReLU point MLPs (`point_transforms.{0..3}`, widths in -> 32 -> 256 -> 128 -> 96 times cr) -- and a
SalsaNext range branch over the (B, 5, H, W) range image (`range_branch.{stem, stage1..4, mid_stage, up1..4}`). The three
branches meet four times per forward,

    z_next.F = voxel_to_point(x, z).F + range_to_point(r, pxpy) + ReLU(BatchNorm(Linear(z.F)))   (rpvnet.py:648-651, 665-668,
                                                                                                   683-686, 701-704)

each of them one kernel (fused.range_point_merge, csrc/rangemerge.hip) behind the point Linear: BatchNorm apply, ReLU and
gate mask inside it at widths that are multiples of 32, the fused BatchNorm pass first and its output added by the kernel at
the others; PCS_RANGE_MERGE=0 takes the literal sequence. The merged point features go back to the voxels (point_to_voxel)
and to the range image (rangelib.point_to_range). The range branch stays on torch's dense modules (Conv2d, BatchNorm2d,
LeakyReLU, AvgPool2d, PixelShuffle: MIOpen's path, not this package's) and keeps the reference's Dropout2d(0.2) modules.
mk34 = NUM_LAYER [2, 3, 4, 6, 2, 2, 2, 2], cr 1.75, IN_FEATURE_DIM 5 (R:tools/cfgs/fusion/semantic_kitti/rpvnet_mk34_cr17_5.yaml).
"""
import numpy as np
import torch
from torch import nn

from .. import functional as F
from .. import fused, inference, rangelib
from ..linear import NOT_SERVED, FusedLinear, row_linear
from ..sparse import PointTensor
from .minkunet import MK34_LAYERS, PLANES, PREBUILD, MinkUNet, _norm
from .pointvoxel import initial_voxelize, point_maps, point_to_voxel

RANGE_DROPOUT = 0.2   # hard-coded in the reference's range branch (rpvnet.py:220-230)


def _conv_act_bn(cin, cout, dilation=1):
    """The range branch's unit: 3x3 conv (same size) -> LeakyReLU -> BatchNorm2d; returns (conv, bn)."""
    return nn.Conv2d(cin, cout, 3, padding=dilation, dilation=dilation), nn.BatchNorm2d(cout)


class _RangeContext(nn.Module):
    """1x1 conv -> LeakyReLU = s; s + bn2(lrelu(conv3_dilated(bn1(lrelu(conv2(s))))))   (`conv1..3`, `bn1..2`)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 1)
        self.conv2, self.bn1 = _conv_act_bn(cout, cout)
        self.conv3, self.bn2 = _conv_act_bn(cout, cout, dilation=2)
        self.act = nn.LeakyReLU()

    def forward(self, x):
        s = self.act(self.conv1(x))
        h = self.bn1(self.act(self.conv2(s)))
        return s + self.bn2(self.act(self.conv3(h)))


class _RangeDown(nn.Module):
    """a = lrelu(conv1_1x1(x)) + bn1(lrelu(conv2_3x3(x))); pooled: -> (avgpool(dropout(a)), a), else dropout(a)."""

    def __init__(self, cin, cout, pooled=True, drop=True):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 1)
        self.conv2, self.bn1 = _conv_act_bn(cin, cout)
        self.act = nn.LeakyReLU()
        self.dropout = nn.Dropout2d(RANGE_DROPOUT)
        self.pool = nn.AvgPool2d(3, stride=2, padding=1) if pooled else None
        self.drop = drop

    def forward(self, x):
        a = self.act(self.conv1(x)) + self.bn1(self.act(self.conv2(x)))
        d = self.dropout(a) if self.drop else a
        return d if self.pool is None else (self.pool(d), a)


class _RangeUp(nn.Module):
    """bn1(lrelu(conv1(cat(pixel_shuffle(x, 2), skip)))) with the reference's three dropouts around it (`conv1`, `bn1`)."""

    def __init__(self, cin, cskip, cout, drop=True):
        super().__init__()
        self.conv1, self.bn1 = _conv_act_bn(cin // 4 + cskip, cout)
        self.act = nn.LeakyReLU()
        self.shuffle = nn.PixelShuffle(2)
        self.dropout1, self.dropout2, self.dropout3 = (nn.Dropout2d(RANGE_DROPOUT) for _ in range(3))
        self.drop = drop

    def forward(self, x, skip):
        up = self.shuffle(x)
        if self.drop:
            up = self.dropout1(up)
        h = torch.cat([up, skip], dim=1)
        if self.drop:
            h = self.dropout2(h)
        h = self.bn1(self.act(self.conv1(h)))
        return self.dropout3(h) if self.drop else h


class SalsaNext(nn.Module):
    """The range branch's encoder / decoder (rpvnet.py:205-232); RPVNet.point_logits drives its stages one by one."""

    def __init__(self, in_channels=5, planes=PLANES, cr=1.75):
        super().__init__()
        cs = [int(cr * c) for c in planes]
        self.stem = nn.Sequential(_RangeContext(in_channels, cs[0]), _RangeContext(cs[0], cs[0]), _RangeContext(cs[0], cs[0]))
        self.stage1 = _RangeDown(cs[0], cs[1], drop=False)
        self.stage2 = _RangeDown(cs[1], cs[2])
        self.stage3 = _RangeDown(cs[2], cs[3])
        self.stage4 = _RangeDown(cs[3], cs[4])
        self.mid_stage = _RangeDown(cs[4], cs[4], pooled=False)
        self.up1 = _RangeUp(cs[4], cs[4], cs[5])
        self.up2 = _RangeUp(cs[5], cs[3], cs[6])
        self.up3 = _RangeUp(cs[6], cs[2], cs[7])
        self.up4 = _RangeUp(cs[7], cs[1], cs[8], drop=False)


class RPVNet(MinkUNet):
    point_branch = True

    def __init__(self, num_class=20, in_dim=5, num_layer=MK34_LAYERS, planes=PLANES, cr=1.75, pres=0.05, vres=0.05,
                 dist=False, ignore_label=0, label_smoothing=0.0, dropout=0.3):
        super().__init__(num_class=num_class, in_dim=in_dim, num_layer=num_layer, planes=planes, cr=cr, pres=pres,
                         vres=vres, dist=dist, ignore_label=ignore_label, label_smoothing=label_smoothing, dropout=dropout)
        cs = [int(cr * c) for c in planes]
        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cin, cout), _norm(cout, dist), nn.ReLU(True))
            for cin, cout in ((in_dim, cs[0]), (cs[0], cs[4]), (cs[4], cs[6]), (cs[6], cs[8]))])
        self.range_branch = SalsaNext(5, planes, cr)   # depth, intensity, x, y, z: the reference's range image
        if dist:
            self.range_branch = nn.SyncBatchNorm.convert_sync_batchnorm(self.range_branch)
        self.grid_sample_mode = "bilinear"
        self._bn_layers = [m for m in self.modules() if isinstance(m, fused.FusedBatchNorm)]
        for m in self._bn_layers:
            m.counted_by_parent = True

    def _merge(self, i, x, z, r, pxpy):
        """Hop i: the point tensor after `voxel_to_point(x, z)` and `.F = .F + range_to_point(r, pxpy) + point_transforms[i](z.F)`."""
        lin, bn = self.point_transforms[i][0], self.point_transforms[i][1]
        idx8, w8 = point_maps(x, z)
        h = row_linear(z.F, lin.weight, lin.bias, min_rows=0)   # weight gradient on the split-reduction kernel, at any row count
        if h is NOT_SERVED:
            h = lin(z.F)
        feats = fused.range_point_merge(bn, h, x.F, idx8, w8, r, pxpy, self.grid_sample_mode)
        out = PointTensor(feats, z.C, idx_query=z.idx_query, weights=z.weights)
        out.additional_features = z.additional_features
        return out

    def _point_dropout(self, feats):
        # the module's own flag: fullsize.freeze_dropout switches the dropout MODULES to eval inside a training model
        return torch.nn.functional.dropout(feats, self.dropout.p, self.dropout.training, False)

    def point_logits(self, x, range_image, range_pxpy):
        """x: SparseTensor (feats (N, >= in_dim), coords (N, 4) int), range_image (B, 5, H, W), range_pxpy (N, 3) = (frame, x, y)
        in [-1, 1] -> per-point logits (N, num_class)."""
        if self.training and self._bn_layers:
            torch._foreach_add_([m.num_batches_tracked for m in self._bn_layers], 1)
        rb, pxpy = self.range_branch, range_pxpy
        b, h, w = range_image.shape[0], range_image.shape[2], range_image.shape[3]
        x.F = x.F[:, :self.in_dim]
        z = PointTensor(x.F, x.C.float())
        x0 = initial_voxelize(z, self.pres, self.vres)
        if PREBUILD:
            F.prebuild_coords(x0, [(2, 2)] * 4)
        r0 = rb.stem(range_image)
        x0 = self._stem(x0)
        z0 = self._merge(0, x0, z, r0, pxpy)

        x1 = self.stage1(point_to_voxel(x0, z0))
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        r1, s1 = rb.stage1(rangelib.point_to_range(z0.F, pxpy, b, h, w))
        r2, s2 = rb.stage2(r1)
        r3, s3 = rb.stage3(r2)
        r4, s4 = rb.stage4(r3)
        r4 = rb.mid_stage(r4)
        z1 = self._merge(1, x4, z0, r4, pxpy)

        y1 = point_to_voxel(x4, z1)
        q1 = rangelib.point_to_range(z1.F, pxpy, b, r4.shape[2], r4.shape[3])
        y1.F = self._point_dropout(y1.F)
        y1 = self.up1[1](self.up1[0](y1, cat_with=x3))  # torchsparse.cat([up(y1), x3]) fused into the BN apply pass
        y2 = self.up2[1](self.up2[0](y1, cat_with=x2))
        q2 = rb.up2(rb.up1(q1, s4), s3)
        z2 = self._merge(2, y2, z1, q2, pxpy)

        y3 = point_to_voxel(y2, z2)
        q3 = rangelib.point_to_range(z2.F, pxpy, b, q2.shape[2], q2.shape[3])
        y3.F = self._point_dropout(y3.F)
        y3 = self.up3[1](self.up3[0](y3, cat_with=x1))
        y4 = self.up4[1](self.up4[0](y3, cat_with=x0))
        q4 = rb.up4(rb.up3(q3, s2), s1)
        z3 = self._merge(3, y4, z2, q4, pxpy)

        lin = self.classifier[0]
        if isinstance(lin, FusedLinear):
            return lin.forward_parts([z1.F, z2.F, z3.F])  # Linear over [z1 | z2 | z3] without the concat
        return self.classifier(torch.cat([z1.F, z2.F, z3.F], dim=1))

    def predict(self, batch, evaluator=None, votes=None):
        if self.training:
            raise RuntimeError("RPVNet.predict is an evaluation pass: call model.eval() first")
        with torch.inference_mode():
            return inference.predict_output(self.point_logits(batch["lidar"], batch["range_image"], batch["range_pxpy"]), batch, evaluator, votes)

    def predict_tta(self, raw, num_votes=10, evaluator=None, vote_chunk=None, scale_range=(0.9, 1.1), rng=np.random, hw=(64, 2048),
                    return_logits=False):
        """An evaluation of a raw batch resident in HBM under the fusion dataset's test-time augmentation (`TTA: True`:
        R:pcseg/data/dataset/semantickitti/semantickitti_fusion.py:116-126 and :148-164, ten rotated and rescaled votes per frame,
        each with a range view under a cut of its own, collated as ten scenes by collate_batch_tta). `rangeview.tta_params` draws
        the votes and their cuts from `rng` in the reference's order, `rangeview.device_batch(..., eval_maps=True)` builds
        `vote_chunk` of them at a time from one read of the scans (None: all votes in one forward; voxel size = the model's
        `pres`), and the loop of `inference.predict_tta` sums every vote's softmax rows and decides after the last one; `evaluator`
        (a SegEvaluator) counts that decision once per point. raw: the dict of workloads.synthetic.make_fusion_raw_batch, on the
        device. -> the keys of inference.predict_tta plus "cuts": the (num_votes * num_frames,) np.random.rand() values drawn."""
        from .. import rangeview
        if self.training:
            raise RuntimeError("RPVNet.predict_tta is an evaluation pass: call model.eval() first")
        return inference.vote_loop(
            raw, "RPVNet.predict_tta", num_votes, vote_chunk, evaluator, return_logits,
            lambda nf, nv: dict(zip(("params", "cuts"), rangeview.tta_params(nf, nv, scale_range=scale_range, rng=rng))),
            lambda part, k: rangeview.device_batch(raw, self.pres, part["params"], part["cuts"], votes=k, eval_maps=True, hw=hw),
            lambda batch, v0, scene_votes: scene_votes(batch, self.point_logits(batch["lidar"], batch["range_image"], batch["range_pxpy"])))

    def forward(self, batch):
        logits = self.point_logits(batch["lidar"], batch["range_image"], batch["range_pxpy"])
        out = {"logits": logits}
        if self.training and "targets" in batch:
            out["loss"] = self.criterion(logits, batch["targets"].F.long())
        return out
