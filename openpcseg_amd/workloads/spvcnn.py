"""SPVCNN (ResBlock variant) workload on the HIP operator API.

Architecture and state_dict layout of R:pcseg/model/segmentor/fusion/spvcnn/spvcnn.py:189-456 (so reference
checkpoints load): the MinkUNet trunk of workloads.minkunet (stem, stage1..4, up1..4, classifier) plus a point branch
-- three Linear-BatchNorm-ReLU point MLPs (`point_transforms.{0,1,2}`, widths 32 -> 256 -> 128 -> 96 times cr) whose
output is added to the devoxelised voxel features at strides 16, 4 and 1, and fed back into the voxels by
point_to_voxel. Each of the three merges

    z_next.F = voxel_to_point(x, z).F + ReLU(BatchNorm(Linear(z.F)))        (spvcnn.py:417-418, 430-431, 443-444)

is one kernel (fused.point_merge, csrc/pointmerge.hip) behind the point Linear; widths that are no multiple of 32 and
PCS_POINT_MERGE=0 take the literal sequence. mk18 = NUM_LAYER [2] * 8 (R:tools/cfgs/fusion/semantic_kitti/spvcnn_mk18_cr10.yaml).
"""
import torch
from torch import nn

from .. import functional as F
from .. import fused
from ..linear import NOT_SERVED, FusedLinear, row_linear
from ..sparse import PointTensor
from .minkunet import MK18_LAYERS, PLANES, PREBUILD, MinkUNet, _norm
from .pointvoxel import initial_voxelize, point_maps, point_to_voxel, voxel_to_point


class SPVCNN(MinkUNet):
    point_branch = True

    def __init__(self, num_class=20, in_dim=4, num_layer=MK18_LAYERS, planes=PLANES, cr=1.0,
                 pres=0.05, vres=0.05, dist=False, ignore_label=0, label_smoothing=0.1, dropout=0.0):
        super().__init__(num_class=num_class, in_dim=in_dim, num_layer=num_layer, planes=planes, cr=cr, pres=pres,
                         vres=vres, dist=dist, ignore_label=ignore_label, label_smoothing=label_smoothing, dropout=dropout)
        cs = [int(cr * c) for c in planes]
        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cin, cout), _norm(cout, dist), nn.ReLU(True))
            for cin, cout in ((cs[0], cs[4]), (cs[4], cs[6]), (cs[6], cs[8]))])
        self._bn_layers = [m for m in self.modules() if isinstance(m, fused.FusedBatchNorm)]
        for m in self._bn_layers:
            m.counted_by_parent = True

    def _merge(self, i, x, z):
        """Hop i: the point tensor after `voxel_to_point(x, z)` and `.F += point_transforms[i](z.F)`."""
        lin, bn = self.point_transforms[i][0], self.point_transforms[i][1]
        idx8, w8 = point_maps(x, z)
        h = row_linear(z.F, lin.weight, lin.bias, min_rows=0)   # weight gradient on the split-reduction kernel, at any row count
        if h is NOT_SERVED:
            h = lin(z.F)
        out = PointTensor(fused.point_merge(bn, h, x.F, idx8, w8), z.C, idx_query=z.idx_query, weights=z.weights)
        out.additional_features = z.additional_features
        return out

    def point_logits(self, x):
        """x: SparseTensor (feats (N,>=in_dim), coords (N,4) int) -> per-point logits (N, num_class)."""
        if self.training and self._bn_layers:
            torch._foreach_add_([m.num_batches_tracked for m in self._bn_layers], 1)
        x.F = x.F[:, :self.in_dim]
        z = PointTensor(x.F, x.C.float())
        x0 = initial_voxelize(z, self.pres, self.vres)
        if PREBUILD:
            F.prebuild_coords(x0, [(2, 2)] * 4)
        x0 = self._stem(x0)
        z0 = voxel_to_point(x0, z)
        x1 = self.stage1(point_to_voxel(x0, z0))
        x2 = self.stage2(x1)
        x3 = self.stage3(x2)
        x4 = self.stage4(x3)
        z1 = self._merge(0, x4, z0)
        y1 = point_to_voxel(x4, z1)
        y1.F = self._dropout(y1.F, True)
        y1 = self.up1[1](self.up1[0](y1, cat_with=x3))  # torchsparse.cat([up(y1), x3]) fused into the BN apply pass
        y2 = self.up2[1](self.up2[0](y1, cat_with=x2))
        z2 = self._merge(1, y2, z1)
        y3 = point_to_voxel(y2, z2)
        y3.F = self._dropout(y3.F, True)
        y3 = self.up3[1](self.up3[0](y3, cat_with=x1))
        y4 = self.up4[1](self.up4[0](y3, cat_with=x0))
        z3 = self._merge(2, y4, z2)
        lin = self.classifier[0]
        if isinstance(lin, FusedLinear):
            return lin.forward_parts([z1.F, z2.F, z3.F])  # Linear over [z1 | z2 | z3] without the (N, 480) concat
        return self.classifier(torch.cat([z1.F, z2.F, z3.F], dim=1))

    def predict(self, batch, evaluator=None, votes=None):
        if self.training:
            raise RuntimeError("SPVCNN.predict is an evaluation pass: call model.eval() first")
        return super().predict(batch, evaluator=evaluator, votes=votes)
