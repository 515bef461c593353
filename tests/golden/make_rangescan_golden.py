"""Generate tests/golden/rangescan_golden.npz: the reference's range-view scan, input tensors and KNN label vote on two small frames.

Needs the reference's sources (so it runs where they are present; the .npz is committed). It RUNS, unmodified,
  SemLaserScan.set_points / set_label                          R:pcseg/data/dataset/semantickitti/laserscan.py:148-238, :358-400
  SemkittiRangeViewDataset.prepare_input_label_semantic_with_mask / generate_label (with LEARNING_MAP)
                                                               R:pcseg/data/dataset/semantickitti/semantickitti_rv.py:284-334
  KNN.forward, get_gaussian_kernel                             R:pcseg/model/segmentor/range/utils.py:275-341
on the inputs postprocess_knn (:209-216) hands the vote: the range image as channel 4 of the input tensor times 80.
The three files are loaded from their paths under bare stand-in packages, so that no package __init__ of the reference runs, behind
  * an empty `cv2` module (semantickitti_rv.py imports it for fill_spherical, which is not called),
  * `torchvision.transforms.functional` with `to_tensor` only (imported by both files, called by neither function run here),
  * `np.float = float` (laserscan.py:302 spells the float64 dtype that way; NumPy dropped the alias).
None of the three changes a value. The dataset is instantiated without its __init__ (which wants the dataset on disk).

Inputs: frame 0 = make_scan(3, 3000), frame 1 = make_scan(5, 2117) (workloads.synthetic), each recorded at 16 x 64 (3 000 points on
1 024 pixels: collisions dominate, and point 0 wins a pixel, which the reference's mask then drops) and at 64 x 512; seeded raw
SemanticKITTI ids with instance bits set; a seeded block-constant proj_argmax, under which the vote changes the pixel's label for
several percent of the points, so a kernel that copies the pixel label fails.

Recorded per (frame, size) under the prefix f<i>_<H>x<W>_: the hit pixels (flat index) with the winner's index, range, mask, raw and
mapped label; CRC-32 of every full array (proj_range, proj_xyz, proj_remission, proj_idx, proj_mask, proj_sem_label, the (6, H, W)
input tensor, the mapped label); per point proj_x, proj_y, unproj_range; proj_argmax and the vote's output. Data only.

Seed guards, asserted here (change the seed if one fails):
  * range_scan_host(atan="double") -- the kernel's arctan2 / arcsin -- equals atan="numpy32" -- the reference's -- bit for bit;
  * no pixel whose two nearest depths are equal (the reference leaves that order open; the contract fixes it);
  * range_scan_host + input_host equal the reference's arrays, knn_vote_host equals the reference's vote on every row;
  * inv_gauss_weights equals 1 - get_gaussian_kernel bit for bit at search 3, 5, 7 for every sigma of GUARDED_SIGMAS (the
    weights at sigma 1.0 are recorded as inv_gauss_3, inv_gauss, inv_gauss_7).
With those, a device test needs no allowance on the fixture.

    python tests/golden/make_rangescan_golden.py
"""
import importlib
import os
import sys
import types
import zlib

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, OUT)

FRAMES = ((3, 3000), (5, 2117))            # (make_scan seed, rows)
SIZES = ((16, 64), (64, 512))
LABEL_SEED, ARGMAX_SEED = 77, 91
BLOCK = (4, 8)                             # proj_argmax is constant on blocks of 4 x 8 pixels
NUM_CLASS = 20
KNN_PARAMS = {"knn": 5, "search": 5, "sigma": 1.0, "cutoff": 1.0}
GUARDED_SIGMAS = (0.3, 0.5, 0.7, 1.0, 1.3, 1.5, 2.0, 3.0, 4.0)   # at search 3, 5 and 7 each: inv_gauss_weights == the reference's bits


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def stand_ins(ref_root):
    import torch
    sys.modules["cv2"] = types.ModuleType("cv2")
    tv, tvt, tvf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))

    def to_tensor(pic):
        assert isinstance(pic, np.ndarray) and pic.dtype != np.uint8
        pic = pic[:, :, None] if pic.ndim == 2 else pic
        return torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1)))

    tvf.to_tensor = to_tensor
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    if not hasattr(np, "float"):
        np.float = float
    # bare packages over the reference's directories: their modules load from their own files, no __init__ runs
    for name in ("pcseg", "pcseg.data", "pcseg.data.dataset", "pcseg.data.dataset.semantickitti", "pcseg.model", "pcseg.model.segmentor",
                 "pcseg.model.segmentor.range"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref_root, *name.split("."))]
        sys.modules[name] = pkg


def make_labels(rng, n, keys):
    sem = rng.choice(np.asarray(keys, dtype=np.uint32), size=n)
    inst = rng.integers(0, 1000, size=n).astype(np.uint32)
    return (sem | (inst << np.uint32(16))).astype(np.uint32)


def block_argmax(rng, h, w):
    bh, bw = BLOCK
    blocks = rng.integers(0, NUM_CLASS, size=(-(-h // bh), -(-w // bw)))
    return np.repeat(np.repeat(blocks, bh, axis=0), bw, axis=1)[:h, :w].astype(np.int64)


def main():
    import torch
    from stage_reference import reference_root
    from make_golden import save_npz_stable
    from openpcseg_amd import rangescan
    from openpcseg_amd.workloads.synthetic import make_scan
    stand_ins(reference_root())
    rv = importlib.import_module("pcseg.data.dataset.semantickitti.semantickitti_rv")
    utils = importlib.import_module("pcseg.model.segmentor.range.utils")
    learning_map = rv.LEARNING_MAP
    lut = np.arange(max(learning_map) + 1, dtype=np.int64)
    for key, value in learning_map.items():
        lut[key] = value
    out = {"frames": np.array(FRAMES, dtype=np.int64), "sizes": np.array(SIZES, dtype=np.int64), "label_lut": lut.astype(np.int16),
           "num_class": np.int64(NUM_CLASS), "fov": np.array(rangescan.FOV)}
    out.update({"knn_" + k: np.float64(v) for k, v in KNN_PARAMS.items()})
    # the weights: rangescan.inv_gauss_weights (NumPy, its own float32 steps) against the reference's kernel, bit for bit
    for search in (3, 5, 7):
        for sigma in GUARDED_SIGMAS:
            ref_w = (1 - utils.get_gaussian_kernel(search, sigma, 1)).reshape(-1).numpy()
            assert ref_w.dtype == np.float32 and np.array_equal(ref_w.view(np.uint32), rangescan.inv_gauss_weights(search, sigma).view(np.uint32)), \
                (search, sigma, "inv_gauss_weights is not the reference's kernel")
            if sigma == KNN_PARAMS["sigma"]:
                out["inv_gauss" if search == KNN_PARAMS["search"] else "inv_gauss_%d" % search] = ref_w
    out["guarded_sigmas"] = np.array(GUARDED_SIGMAS)
    lrng, arng = np.random.default_rng(LABEL_SEED), np.random.default_rng(ARGMAX_SEED)
    knn = utils.KNN(dict(KNN_PARAMS), NUM_CLASS)
    for i, (seed, rows) in enumerate(FRAMES):
        pts = make_scan(seed, rows)
        assert pts.shape == (rows, 4) and pts.dtype == np.float32
        labels = make_labels(lrng, rows, sorted(learning_map))
        out["f%d_points" % i], out["f%d_labels" % i] = pts, labels
        for h, w in SIZES:
            pre = "f%d_%dx%d_" % (i, h, w)
            scan = rv.SemLaserScan(nclasses=34, sem_color_dict=rv.color_map, project=True, H=h, W=w, fov_up=3.0, fov_down=-25.0)
            scan.set_points(pts[:, :3].copy(), pts[:, 3].copy())
            scan.set_label(labels.copy())
            ds = object.__new__(rv.SemkittiRangeViewDataset)
            ds.H, ds.W, ds.label_transfer_dict = h, w, learning_map
            sample = {"xyz": scan.proj_xyz, "intensity": scan.proj_remission, "range_img": scan.proj_range, "xyz_mask": scan.proj_mask,
                      "semantic_label": ds.generate_label(scan.proj_sem_label)}
            tensor, label, mask = ds.prepare_input_label_semantic_with_mask(sample)
            tensor = np.ascontiguousarray(tensor.transpose(2, 0, 1))       # what to_tensor makes of it
            assert tensor.dtype == np.float32 and tensor.shape == (6, h, w) and mask.dtype == np.float32

            # guards: the host contract is the reference, the two arctangents agree, no depth tie decides a pixel
            views = {a: rangescan.range_scan_host(pts, labels, (h, w), atan=a) for a in ("numpy32", "double")}
            for key in views["numpy32"]:
                assert np.array_equal(views["numpy32"][key], views["double"][key]), (pre, key, "a face case: pick another seed")
            view = views["numpy32"]
            for key in ("proj_range", "proj_xyz", "proj_remission", "proj_idx", "proj_mask", "proj_sem_label", "proj_x", "proj_y",
                        "unproj_range"):
                ref = getattr(scan, key)
                assert view[key].dtype == ref.dtype and np.array_equal(view[key], ref), (pre, key, "range_scan_host is not the reference")
            pix = view["proj_y"].astype(np.int64) * w + view["proj_x"]
            order = np.lexsort((view["unproj_range"], pix))
            same = (pix[order][1:] == pix[order][:-1]) & (view["unproj_range"][order][1:] == view["unproj_range"][order][:-1])
            first = np.ones(rows, dtype=bool)
            first[1:] = pix[order][1:] != pix[order][:-1]
            assert not (same & first[:-1]).any(), (pre, "two nearest depths of a pixel are equal: pick another seed")
            h_scan, h_label, h_mask = rangescan.input_host(view, lut)
            assert np.array_equal(h_scan.view(np.uint32), tensor.view(np.uint32)) and np.array_equal(h_label, label) and np.array_equal(h_mask, mask)
            if (h, w) == SIZES[0] and i == 0:
                assert (view["proj_idx"] == 0).sum() == 1 and view["proj_mask"][view["proj_idx"] == 0] == 0   # the mask quirk is in
                assert (view["proj_idx"] >= 0).sum() < rows // 2                                              # collisions dominate

            # the vote, on postprocess_knn's inputs
            argmax = block_argmax(arng, h, w)
            t_range = torch.from_numpy(tensor[4]) * 80.0
            ref_vote = knn(t_range, torch.from_numpy(scan.unproj_range), torch.from_numpy(argmax),
                           torch.from_numpy(scan.proj_x.astype(np.int64)), torch.from_numpy(scan.proj_y.astype(np.int64))).numpy()
            vote = rangescan.knn_vote_host(h_scan[4] * np.float32(80.0), argmax, view["unproj_range"], view["proj_x"], view["proj_y"],
                                           num_class=NUM_CLASS, **KNN_PARAMS)
            assert np.array_equal(vote, ref_vote), (pre, "knn_vote_host is not the reference", int((vote != ref_vote).sum()))
            changed = float((vote != argmax[view["proj_y"], view["proj_x"]]).mean())
            assert changed > 0.03, (pre, changed)

            hit = np.flatnonzero(view["proj_idx"].reshape(-1) >= 0).astype(np.int32)
            out.update({pre + "hit": hit, pre + "hit_idx": view["proj_idx"].reshape(-1)[hit], pre + "hit_range": view["proj_range"].reshape(-1)[hit],
                        pre + "hit_mask": mask.reshape(-1)[hit].astype(np.int8), pre + "hit_sem": view["proj_sem_label"].reshape(-1)[hit],
                        pre + "hit_label": label.reshape(-1)[hit].astype(np.int16)})
            for key in ("proj_range", "proj_xyz", "proj_remission", "proj_idx", "proj_mask", "proj_sem_label"):
                out[pre + "crc_" + key] = crc(getattr(scan, key))
            out[pre + "crc_scan"], out[pre + "crc_label"] = crc(tensor), crc(label.astype(np.int64))
            out.update({pre + "proj_x": scan.proj_x.astype(np.int16), pre + "proj_y": scan.proj_y.astype(np.int16),
                        pre + "unproj_range": scan.unproj_range, pre + "proj_argmax": argmax.astype(np.int8),
                        pre + "vote": ref_vote.astype(np.int8), pre + "vote_changed": np.float64(changed)})
            print("%s %d hit pixels of %d, the vote changes %.1f %% of the points" % (pre, hit.shape[0], h * w, 100 * changed))
    path = os.path.join(OUT, "rangescan_golden.npz")
    save_npz_stable(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
