"""Generate tests/golden/transform_golden.npz: the reference's dataset transform on two small frames.

Needs the reference's sources (so it runs where they are present; the .npz is committed). It imports, unmodified,
  aug_points        R:tools/utils/common/seg_utils.py:43-100
  sparse_quantize   TS:torchsparse/utils/quantize.py:24-46 (from the reference's package/torchsparse.zip)
and restates only the four lines of get_single_sample between them (R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:
83-120): the float32 store of the augmented xyz, pc_ = round(xyz / voxel_size) as int32, pc_ -= pc_.min(0), sparse_quantize(pc_).
seg_utils imports torch_scatter and the whole torchsparse package at module level although aug_points uses neither: those
imports are served by empty stand-ins (and the real torchsparse.utils.quantize).

Input: frames of 512 and 301 rows, four columns, cut from workloads.synthetic.make_scan, plus hand-placed rows whose coordinates
are exact odd multiples of half a voxel (voxel 0.25: multiples of 0.125 are exact in float32), of both signs.
Recorded, each with the NumPy seed it ran under: three training draws (all four augmentations on, scale range 0.9 .. 1.1) and
the ten votes of test-time augmentation, stored case-major (cases 0..2 = the training draws, 3..12 = votes 0..9) as one array
per frame and quantity: xyz (aug_points' output as float32), pc (rounded and shifted), inverse, inds (concatenated, with their
lengths). Data only.

    python tests/golden/make_transform_golden.py
"""
import hashlib
import importlib.util
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, OUT)

VOXEL = 0.25
SCALE_RANGE = [0.9, 1.1]
TRAIN_SEEDS = (11, 12, 13)
TTA_SEED = 21
HALF_ROWS = 8   # the first rows of frame 0 are the hand-placed ones


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def state_digest():
    """The global generator's position: (sha256 of the 624 Mersenne-Twister words, index into them) as bytes + int."""
    st = np.random.get_state()
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(st[1], dtype=np.uint32).tobytes()).digest(), dtype=np.uint8), np.int64(st[2])


def import_reference():
    from stage_reference import TS_ZIP, reference_root
    root = reference_root()
    if root is None:
        raise RuntimeError("the reference's sources are not present")
    tmp = tempfile.mkdtemp(prefix="pcs_transform_golden_")
    member = "torchsparse/torchsparse/utils/quantize.py"
    with zipfile.ZipFile(TS_ZIP) as zf:
        zf.extract(member, tmp)
    for name in ("torch_scatter", "torchsparse", "torchsparse.nn", "torchsparse.nn.functional", "torchsparse.nn.utils",
                 "torchsparse.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchsparse"].nn = sys.modules["torchsparse.nn"]
    sys.modules["torchsparse.nn"].functional = sys.modules["torchsparse.nn.functional"]
    sys.modules["torchsparse.nn.utils"].get_kernel_offsets = None
    sys.modules["torchsparse"].PointTensor = sys.modules["torchsparse"].SparseTensor = None
    quantize = _load("torchsparse.utils.quantize", os.path.join(tmp, member))
    seg_utils = _load("pcs_reference_seg_utils", os.path.join(root, "tools", "utils", "common", "seg_utils.py"))
    return seg_utils.aug_points, quantize.sparse_quantize


def make_frames():
    from openpcseg_amd.workloads.synthetic import make_scan
    a = make_scan(3, 512).copy()
    b = make_scan(4, 301).copy()
    # odd multiples of half a voxel (k + 1/2) * VOXEL, both signs: k even and odd decide which way half-to-even goes
    # |x| != |y| in every row: under the votes that rotate by an odd multiple of pi / 4 the two products of a row with |x| = |y|
    # cancel to ~1e-16, and what is left then depends on whether the BLAS behind np.dot fuses its multiply-adds (OpenBLAS picks
    # its kernel by the CPU it runs on) -- a value the reference itself does not reproduce from machine to machine
    half = np.array([[0.5, -1.5, 1.5], [-1.5, 2.5, -2.5], [3.5, -4.5, 0.5], [-0.5, 1.5, -1.5],
                     [6.5, -7.5, 2.5], [-8.5, 9.5, -0.5], [10.5, 11.5, -3.5], [-12.5, -13.5, 1.5]]) * VOXEL
    assert half.shape[0] == HALF_ROWS
    a[:HALF_ROWS, :3] = half.astype(np.float32)
    assert np.array_equal(a[:HALF_ROWS, :3].astype(np.float64), half)
    return a, b


def dataset_transform(aug_points, sparse_quantize, frame, **aug):
    """get_single_sample's lines between the scan and the SparseTensors, for one frame."""
    point = frame.copy()
    point[:, 0:3] = aug_points(xyz=point[:, :3], scale_axis="xyz", scale_range=SCALE_RANGE, **aug)
    pc_ = np.round(point[:, :3] / VOXEL).astype(np.int32)
    pc_ -= pc_.min(0, keepdims=1)
    _, inds, inverse_map = sparse_quantize(pc_, return_index=True, return_inverse=True)
    return point[:, :3].copy(), pc_, np.asarray(inds, dtype=np.int32), np.asarray(inverse_map, dtype=np.int32)


def main():
    aug_points, sparse_quantize = import_reference()
    frames = make_frames()
    out = {"voxel_size": np.float64(VOXEL), "scale_range": np.array(SCALE_RANGE), "train_seeds": np.array(TRAIN_SEEDS),
           "tta_seed": np.int64(TTA_SEED), "half_rows": np.int64(HALF_ROWS), "frame0": frames[0], "frame1": frames[1]}

    cases = {0: [], 1: []}   # per frame: the 13 recorded cases in the order train0..2, tta0..9

    def keep(tag, f, res):
        cases[f].append(res)

    # plain transform (no augmentation): the half-voxel rows round as NumPy rounds them
    for f, frame in enumerate(frames):
        out["plain_pc_f%d" % f] = dataset_transform(aug_points, sparse_quantize, frame)[1].astype(np.int16)
    # training: one worker seed per draw, the frames of the batch one after the other
    for k, seed in enumerate(TRAIN_SEEDS):
        np.random.seed(seed)
        for f, frame in enumerate(frames):
            keep("train%d" % k, f, dataset_transform(aug_points, sparse_quantize, frame, if_flip=True, if_scale=True,
                                                     if_jitter=True, if_rotate=True, if_tta=False))
        out["train%d_state_after" % k], out["train%d_pos_after" % k] = state_digest()
    # test-time augmentation: __getitem__ runs the ten votes of one index, then the next index
    np.random.seed(TTA_SEED)
    for f, frame in enumerate(frames):
        for v in range(10):
            keep("tta%d" % v, f, dataset_transform(aug_points, sparse_quantize, frame, if_flip=False, if_scale=True,
                                                   if_jitter=False, if_rotate=True, if_tta=True, num_vote=v))
    out["tta_state_after"], out["tta_pos_after"] = state_digest()
    # one array per frame and quantity (case-major); int16 holds every coordinate (< 2^15 voxels of 0.25) and row number
    for f in (0, 1):
        assert len(cases[f]) == len(TRAIN_SEEDS) + 10 and max(int(c[1].max()) for c in cases[f]) < 2 ** 15
        out["xyz_f%d" % f] = np.stack([c[0] for c in cases[f]])
        out["pc_f%d" % f] = np.stack([c[1].T for c in cases[f]]).astype(np.int16)   # (case, axis, row): packs better
        out["inverse_f%d" % f] = np.stack([c[3] for c in cases[f]]).astype(np.int16)
        out["inds_f%d" % f] = np.concatenate([c[2] for c in cases[f]]).astype(np.int16)
        out["inds_len_f%d" % f] = np.array([c[2].shape[0] for c in cases[f]])
    path = os.path.join(OUT, "transform_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
