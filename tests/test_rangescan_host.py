"""The range-view scan and its KNN vote on the host: rangescan.range_scan_host / input_host / knn_vote_host
reproduce tests/golden/rangescan_golden.npz -- the output of RUNNING the reference's SemLaserScan, its dataset's input builder and
its KNN module (tests/golden/make_rangescan_golden.py) -- by equality; the two orders the contract fixes hold on constructed ties;
the new C entries are declared, exported and refuse bad sizes without a device."""
import os
import re

import numpy as np
import pytest

import rangescan_cases as rc
from openpcseg_amd import native, rangescan
from openpcseg_amd.workloads.synthetic import make_raw_batch, make_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcs_range_scan_ws_bytes", "pcs_range_scan_f32", "pcs_range_knn_vote")


@pytest.fixture(scope="module")
def gold():
    return rc.load_gold()


@pytest.mark.parametrize("atan", ["numpy32", "double"])
def test_scan_and_input_reproduce_the_reference(gold, atan):
    for i, (pts, labels) in enumerate(rc.frames(gold)):
        for hw in rc.sizes(gold):
            pre = rc.prefix(i, hw)
            view = rangescan.range_scan_host(pts, labels, hw, tuple(gold["fov"]), atan=atan)
            rc.assert_view_is_fixture(gold, pre, view)
            rc.assert_input_is_fixture(gold, pre, *rangescan.input_host(view, rc.lut(gold)))
            raw = rangescan.input_host(view)[1]                       # without the table: the raw semantic ids
            assert np.array_equal(raw.reshape(-1)[gold[pre + "hit"]], gold[pre + "hit_sem"]) and raw.dtype == np.int64


def test_vote_reproduces_the_reference(gold):
    for search, key in ((3, "inv_gauss_3"), (5, "inv_gauss"), (7, "inv_gauss_7")):        # the reference's kernels, recorded
        w = rangescan.inv_gauss_weights(search, 1.0)
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), gold[key].view(np.uint32)), search
        assert np.array_equal(w.reshape(search, search), w.reshape(search, search).T) and w.argmin() == (search * search - 1) // 2
    for i in range(2):
        for hw in rc.sizes(gold):
            vote = rangescan.knn_vote_host(*rc.vote_inputs(gold, i, hw, "numpy32"), knn=5, search=5, sigma=1.0, cutoff=1.0, num_class=20)
            assert vote.dtype == np.int64 and np.array_equal(vote, gold[rc.prefix(i, hw) + "vote"])
            assert float(gold[rc.prefix(i, hw) + "vote_changed"].reshape(-1)[0]) > 0.03     # copying the pixel's label would fail


def test_mask_rules(gold):
    pts, labels = rc.frames(gold)[0]
    ref = rangescan.range_scan_host(pts, labels, (16, 64))
    hit = rangescan.range_scan_host(pts, labels, (16, 64), mask="hit")
    zero = ref["proj_idx"] == 0
    assert zero.sum() == 1 and ref["proj_mask"][zero] == 0 and hit["proj_mask"][zero] == 1     # point 0 wins a pixel of this scan
    assert np.array_equal(ref["proj_mask"][~zero], hit["proj_mask"][~zero])
    assert np.array_equal(hit["proj_mask"], (hit["proj_idx"] >= 0).astype(np.float32))
    assert all(np.array_equal(ref[k], hit[k]) for k in ref if k != "proj_mask")


def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    assert re.search(r"\bint64_t pcs_range_scan_ws_bytes\(int32_t num_frames, int32_t H, int32_t W\);", hdr)
    assert re.search(r"\bint pcs_range_scan_f32\(const float \*points, int64_t n, int32_t c, const int64_t \*frame_offsets, int32_t num_frames,", hdr)
    assert re.search(r"\bint pcs_range_knn_vote\(const float \*proj_range, const int64_t \*proj_argmax, int32_t num_scenes, int32_t H, int32_t W,", hdr)
    assert re.search(r"#define PCS_ABI_VERSION 12\b", hdr)
    lib = native.load_library()   # dlopen works without a GPU
    for name in ENTRIES:
        assert name in native.SIGNATURES and hasattr(lib, name), name
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12


def test_size_only_refusals():
    """Sizes are checked before any pointer is looked at, so the refusals need no device."""
    lib = native.load_library()
    assert lib.pcs_range_scan_ws_bytes(12, 64, 2048) == 12 * 64 * 2048 * 8
    assert lib.pcs_range_scan_ws_bytes(1, 1, 1) == 8
    for s, h, w in ((0, 64, 2048), (-1, 64, 2048), (1, 0, 2048), (1, 64, 0), (4096, 1024, 1024), (2, 32768, 32768)):
        assert lib.pcs_range_scan_ws_bytes(s, h, w) == -1, (s, h, w)
    scan = lambda n, c, f, h, w, fov=0.5: lib.pcs_range_scan_f32(None, n, c, None, f, None, None, 0, h, w, 0.4, fov, 0, *([None] * 10))
    for n, c, f, h, w in ((8, 3, 1, 64, 2048), (8, 4, 0, 64, 2048), (8, 4, 1, 0, 2048), (8, 4, 2, 32768, 32768), (-1, 4, 1, 64, 2048),
                          (2 ** 31, 4, 1, 64, 2048)):
        assert scan(n, c, f, h, w) == -1 and b"bad args" in lib.pcs_last_error(), (n, c, f, h, w)
    assert scan(8, 4, 1, 64, 2048, fov=0.0) == -1 and b"bad args" in lib.pcs_last_error()
    assert scan(8, 4, 1, 64, 2048) == -1 and b"null pointer" in lib.pcs_last_error()
    vote = lambda search, knn, cutoff, nc, b=1, n=8: lib.pcs_range_knn_vote(None, None, b, 16, 64, None, None, None, n, None, search, knn, cutoff,
                                                                            None, nc, None, None, None, None)
    for args, word in (((4, 5, 1.0, 20), b"search"), ((9, 5, 1.0, 20), b"search"), ((1, 1, 1.0, 20), b"search"), ((5, 0, 1.0, 20), b"knn"),
                       ((5, 26, 1.0, 20), b"knn"), ((3, 10, 1.0, 20), b"knn"), ((5, 5, -1.0, 20), b"cutoff"), ((5, 5, float("nan"), 20), b"cutoff"),
                       ((5, 5, 1.0, 65), b"num_class"), ((5, 5, 1.0, 1), b"num_class"), ((5, 5, 1.0, 20, 0), b"bad sizes"),
                       ((5, 5, 1.0, 20, 1, -1), b"bad sizes"), ((5, 5, 1.0, 20, 1, 2 ** 31), b"bad sizes")):
        assert vote(*args) == -1 and word in lib.pcs_last_error(), args
    assert vote(5, 5, 1.0, 20) == -1 and b"null pointer" in lib.pcs_last_error()


@pytest.mark.parametrize("hw", [(64, 2048), (64, 512)])
def test_the_two_arctangents_agree_on_a_full_scan(hw):
    """DESIGN.md section 7j's cap: the rows whose pixel differs between the kernel's functions and NumPy's stay at or below 1e-4."""
    pts = make_scan(3)
    a, b = (rangescan.range_scan_host(pts, None, hw, atan=t) for t in ("numpy32", "double"))
    moved = int(((a["proj_x"] != b["proj_x"]) | (a["proj_y"] != b["proj_y"])).sum())
    print("rows on another pixel at %s: %d of %d" % (hw, moved, pts.shape[0]))
    assert moved <= 1e-4 * pts.shape[0]
    assert np.array_equal(a["unproj_range"], b["unproj_range"])
    assert np.array_equal(a["unproj_range"], np.linalg.norm(pts[:, :3], 2, axis=1))


def test_collision_rule_on_constructed_ties():
    """Equal depths: the lower index wins; otherwise the nearer point, wherever it stands in the scan."""
    p = np.array([[10.0, 1.0, -1.0, 0.1], [5.0, 0.5, -0.5, 0.2], [5.0, 0.5, -0.5, 0.3], [10.0, 1.0, -1.0, 0.4], [5.0, 0.5, -0.5, 0.5]], dtype=np.float32)
    v = rangescan.range_scan_host(p, np.array([10, 11, 13, 15, 16]), (16, 64))
    assert len(set(zip(v["proj_x"].tolist(), v["proj_y"].tolist()))) == 1          # one ray, one pixel
    y, x = int(v["proj_y"][0]), int(v["proj_x"][0])
    assert v["proj_idx"][y, x] == 1 and v["proj_remission"][y, x] == np.float32(0.2) and v["proj_sem_label"][y, x] == 11
    assert (v["proj_idx"] >= 0).sum() == 1 and v["proj_range"][y, x] == v["unproj_range"][1]
    v = rangescan.range_scan_host(p[::-1].copy(), None, (16, 64))                  # reversed: rows 0, 2, 3 are the near ones
    assert v["proj_idx"][y, x] == 0 and v["proj_mask"][y, x] == 0 and (v["proj_sem_label"] == 0).all()


def test_selection_rule_on_a_constructed_boundary_tie():
    """Two candidates at the same weighted distance compete for the last of the knn places: the lower window position takes it."""
    h, w = 16, 64
    image = np.full((h, w), -1.0, dtype=np.float32)
    argmax = np.zeros((h, w), dtype=np.int64)
    py, px, u = 8, 30, np.float32(10.0)
    image[py, px] = u
    image[py, px - 1], image[py, px + 1] = np.float32(10.25), np.float32(10.25)     # mirror positions: equal gaussian weights
    argmax[py, px], argmax[py, px - 1], argmax[py, px + 1] = 3, 7, 5
    args = (image, argmax, np.array([u]), np.array([px]), np.array([py]))
    # knn = 2: the centre (distance 0) and ONE of the two neighbours; with knn = 1 class 3 alone, with knn = 3 classes 3, 5, 7 tie -> 3
    assert rangescan.knn_vote_host(*args, knn=1, search=3, cutoff=1.0).tolist() == [3]
    argmax[py, px] = 0                                                              # the centre votes for the ignored class
    assert rangescan.knn_vote_host(*args, knn=2, search=3, cutoff=1.0).tolist() == [7]   # position 3 (left) before position 5 (right)
    assert rangescan.knn_vote_host(*args, knn=3, search=3, cutoff=1.0).tolist() == [5]   # both in: the lowest class on equal counts
    assert rangescan.knn_vote_host(*args, knn=3, search=3, cutoff=0.1).tolist() == [1]   # both beyond the cutoff: no class has a vote


@pytest.mark.parametrize("search", [3, 5, 7])
def test_vote_equals_the_torch_sequence(search):
    rng = np.random.default_rng(search)
    h, w, n, nc = 16, 64, 700, 20
    image = rng.uniform(2.0, 40.0, size=(h, w)).astype(np.float32)
    image[rng.uniform(size=(h, w)) < 0.15] = -1.0
    argmax = rng.integers(0, nc, size=(h, w))
    py, px = rng.integers(0, h, size=n), rng.integers(0, w, size=n)
    u = (np.abs(image[py, px]) + rng.uniform(0.0, 0.5, size=n)).astype(np.float32)
    for knn in (1, 5, search * search // 2):
        mine = rangescan.knn_vote_host(image, argmax, u, px, py, knn=knn, search=search, sigma=1.0, cutoff=1.0, num_class=nc)
        assert np.array_equal(mine, rc.torch_vote(image, argmax, u, px, py, knn, search, 1.0, 1.0, nc)), (search, knn)


def test_refusals():
    raw = make_raw_batch([0, 1], n_points=64)
    with pytest.raises(RuntimeError, match="range_scan_host"):                     # host tensors: pointed at the host form
        rangescan.device_batch(raw)
    with pytest.raises(ValueError, match="C >= 4"):
        rangescan.device_batch({**raw, "points": raw["points"][:, :3]})
    with pytest.raises(ValueError, match="mask"):
        rangescan.device_batch(raw, mask="any")
    pts = make_scan(0, 32)
    for bad in (pts[:, :3], pts.reshape(-1)):
        with pytest.raises(ValueError, match="C >= 4"):
            rangescan.range_scan_host(bad)
    with pytest.raises(ValueError, match="atan"):
        rangescan.range_scan_host(pts, atan="float")
    with pytest.raises(ValueError, match="labels"):
        rangescan.range_scan_host(pts, np.zeros(3))
    for row in ([np.nan, 1, 1, 0], [0, 0, 0, 0.5], [np.inf, 1, 1, 0], [3e38, 3e38, 0, 0], [0, 0, 1e-20, 0.5]):   # the last: z / depth > 1
        with pytest.raises(ValueError, match="not finite or has zero depth"):
            rangescan.range_scan_host(np.concatenate([pts, np.array([row], dtype=np.float32)]))
    image, argmax = np.ones((16, 64), dtype=np.float32), np.zeros((16, 64), dtype=np.int64)
    one = (np.ones(1, dtype=np.float32), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))
    for kw, word in (({"search": 4}, "search"), ({"search": 9}, "search"), ({"knn": 0}, "knn"), ({"knn": 26}, "knn"), ({"cutoff": -1.0}, "cutoff"),
                     ({"num_class": 65}, "num_class")):
        with pytest.raises(ValueError, match=word):
            rangescan.knn_vote_host(image, argmax, *one, **kw)
        with pytest.raises(ValueError, match=word):                                 # the device form refuses before it touches a tensor
            rangescan.knn_vote(None, None, None, None, None, [0, 1], **kw)
    with pytest.raises(ValueError, match="outside the 16 x 64 image"):
        rangescan.knn_vote_host(image, argmax, one[0], np.array([64]), one[2])
    with pytest.raises(ValueError, match="proj_argmax outside"):
        rangescan.knn_vote_host(image, argmax + 20, *one)
    with pytest.raises(ValueError, match="proj_range and proj_argmax"):
        rangescan.knn_vote_host(image, argmax[:8], *one)
