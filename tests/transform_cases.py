"""Shared by the dataset-transform tests: the reference fixture (tests/golden/transform_golden.npz, written by
tests/golden/make_transform_golden.py) and the host composition a device batch is held to."""
import hashlib
import os

import numpy as np
import torch

from openpcseg_amd import transform as T
from openpcseg_amd.hostdata import sparse_collate_fn, sparse_quantize
from openpcseg_amd.sparse import SparseTensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform_golden.npz")
N_TRAIN, N_VOTES = 3, 10


class Fixture:
    """The recorded cases: 0..2 the seeded training draws, 3..12 votes 0..9 of test-time augmentation, for two frames."""

    def __init__(self):
        g = np.load(GOLDEN)
        self.g = g
        self.voxel = float(g["voxel_size"])
        self.scale_range = tuple(float(v) for v in g["scale_range"])
        self.frames = [g["frame0"], g["frame1"]]
        self.half_rows = int(g["half_rows"])
        self.train_seeds = [int(s) for s in g["train_seeds"]]
        self.tta_seed = int(g["tta_seed"])

    def recorded(self, case, f):
        """-> (xyz float32, pc int32, inds, inverse) the reference produced for `case` of frame f."""
        g = self.g
        ends = np.cumsum(g["inds_len_f%d" % f])
        inds = g["inds_f%d" % f][ends[case] - g["inds_len_f%d" % f][case]:ends[case]]
        return (g["xyz_f%d" % f][case], g["pc_f%d" % f][case].T.astype(np.int32), inds.astype(np.int64),
                g["inverse_f%d" % f][case].astype(np.int64))

    def train_params(self, k):
        """The parameters of training draw k, drawn from the global generator under the fixture's seed -> (params (2, 8), the
        generator's state after the draw)."""
        np.random.seed(self.train_seeds[k])
        p = T.draw_train_params(2, scale_range=self.scale_range)
        return p, np.random.get_state()

    def tta_params(self):
        np.random.seed(self.tta_seed)
        p = T.tta_params(2, N_VOTES, scale_range=self.scale_range)
        return p, np.random.get_state()

    def state_matches(self, state, tag):
        digest = np.frombuffer(hashlib.sha256(np.ascontiguousarray(state[1], dtype=np.uint32).tobytes()).digest(), dtype=np.uint8)
        return np.array_equal(digest, self.g["%s_state_after" % tag]) and int(state[2]) == int(self.g["%s_pos_after" % tag])


def host_batch(raw, params, votes, voxel):
    """The host composition: transform_scan_host per (vote, frame), host sparse_quantize, sparse_collate_fn -- the batch
    collate_batch / collate_batch_tta hand the model, scene v * num_frames + f = vote v of frame f."""
    pts, labels, off, nf = raw["points"].cpu().numpy(), raw["labels"].cpu().numpy(), raw["offsets"], raw["num_frames"]
    samples = []
    for v in range(votes):
        for f in range(nf):
            p, lab = pts[off[f]:off[f + 1]], labels[off[f]:off[f + 1]]
            feat, pc = T.transform_scan_host(p, params[v * nf + f], voxel)
            _, inds, inverse = sparse_quantize(pc, return_index=True, return_inverse=True)
            samples.append({"lidar": SparseTensor(feat[inds], pc[inds]), "targets": SparseTensor(lab[inds], pc[inds]),
                            "targets_mapped": SparseTensor(lab, pc), "inverse_map": SparseTensor(np.asarray(inverse, dtype=np.int64), pc),
                            "num_points": np.array([p.shape[0]])})
    return sparse_collate_fn(samples)


def raw_of(frames, labels_seed=0, num_classes=20, device="cpu"):
    """A raw batch (the dict of workloads.synthetic.make_raw_batch) from given (n_i, C) float32 frames."""
    rng = np.random.default_rng(labels_seed)
    sizes = [f.shape[0] for f in frames]
    labels = rng.integers(0, num_classes, size=sum(sizes)).astype(np.int64)
    ids = np.concatenate([np.full(n, i, dtype=np.int32) for i, n in enumerate(sizes)])
    return {"points": torch.from_numpy(np.concatenate(frames)).to(device), "frames": torch.from_numpy(ids).to(device),
            "labels": torch.from_numpy(labels).to(device), "num_frames": len(frames), "offsets": [0] + np.cumsum(sizes).tolist()}
