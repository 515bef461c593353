"""csrc/scantransform.hip (pcs_scan_transform, pcs_scan_shift) and transform.device_batch on the MI355X, held to
transform.transform_scan_host -- which tests/test_transform_host.py holds to the reference's recorded outputs. Every result is an
integer or a float32 that both sides round once from the same float64 value: the bound is equality."""
import ctypes

import numpy as np
import pytest
import torch

from openpcseg_amd import native
from openpcseg_amd import transform as T
from openpcseg_amd.sparse import SparseTensor
from transform_cases import N_TRAIN, N_VOTES, Fixture, host_batch, raw_of

pytestmark = pytest.mark.gpu

SIX = [1, 63, 64, 65, 255, 257]      # below, at and above a wave; below and above a workgroup
FIVE = [257, 1, 65, 255, 63]
ONE = [300]
MAXV = native.HipBackend.MAX_VOTES


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def make_frames(sizes, c, seed):
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.normal(0, 20, size=(n, 3)), rng.uniform(0, 1, size=(n, c - 3))], 1).astype(np.float32) for n in sizes]


def make_params(votes, nf, seed):
    """Training draws (rotation, scale, flip, jitter) for every (vote, frame); vote 0 of frame 0 is the identity."""
    p = T.draw_train_params(votes * nf, rng=np.random.RandomState(seed))
    p[0] = T.identity_params(1)[0]
    return p


def host_reference(frames, params, votes, voxel):
    """-> feats (V n, C), shifted coords (V n, 3), mins (V F, 3), scenes (V n,) as the kernels lay them out."""
    nf = len(frames)
    feats, coords, mins, scenes = [], [], [], []
    for v in range(votes):
        for f, fr in enumerate(frames):
            out, pc = T.transform_scan_host(fr, params[v * nf + f], voxel)
            feats.append(out)
            coords.append(pc)
            mins.append(np.round(out[:, :3] / np.float32(voxel)).astype(np.int32).min(0))
            scenes.append(np.full(fr.shape[0], v * nf + f, dtype=np.int64))
    return np.concatenate(feats), np.concatenate(coords), np.stack(mins), np.concatenate(scenes)


def device_points(frames, unaligned):
    pts = np.concatenate(frames)
    if not unaligned:
        return torch.from_numpy(pts).cuda()
    # the same rows starting one row of a 3-column view into the allocation: 12 bytes past a 16-byte boundary
    flat = torch.empty(pts.size + 3, dtype=torch.float32, device="cuda")
    view = flat.view(-1)[3:].view(pts.shape)
    view.copy_(torch.from_numpy(pts))
    assert view.data_ptr() % 16 == 12 and view.is_contiguous()
    return view


def run_kernels(hip, pts, offsets, params, votes, voxel):
    feats, coords, mins, off = hip.scan_transform(pts, offsets, params, votes, voxel)
    unshifted = coords.clone()
    scenes = hip.scan_shift(coords, mins, off, votes)
    return feats.cpu().numpy(), unshifted.cpu().numpy(), coords.cpu().numpy(), mins.cpu().numpy(), scenes.cpu().numpy()


def check_equal(got, frames, params, votes, voxel):
    feats, unshifted, coords, mins, scenes = got
    w_feats, w_coords, w_mins, w_scenes = host_reference(frames, params, votes, voxel)
    assert feats.dtype == np.float32 and coords.dtype == np.int32 and mins.dtype == np.int32 and scenes.dtype == np.int64
    assert np.array_equal(feats.view(np.int32), w_feats.view(np.int32)), int((feats != w_feats).sum())
    assert np.array_equal(mins, w_mins)
    assert np.array_equal(coords, w_coords), int((coords != w_coords).sum())
    assert np.array_equal(scenes, w_scenes)
    assert np.array_equal(unshifted - coords, w_mins[w_scenes])


@pytest.mark.parametrize("sizes", [SIX, FIVE, ONE], ids=["six", "five", "one"])
@pytest.mark.parametrize("votes", [1, 10, MAXV])
@pytest.mark.parametrize("cols", [3, 4, "4-unaligned", 5])
def test_kernels_equal_the_host_transform(hip, sizes, votes, cols):
    c = 4 if cols == "4-unaligned" else cols
    frames = make_frames(sizes, c, seed=len(sizes) * 100 + votes)
    params = make_params(votes, len(sizes), seed=votes + c)
    offsets = [0] + np.cumsum(sizes).tolist()
    voxel = 0.05
    got = run_kernels(hip, device_points(frames, cols == "4-unaligned"), offsets, params, votes, voxel)
    check_equal(got, frames, params, votes, voxel)
    n = offsets[-1]
    assert np.array_equal(got[0][:n].view(np.int32)[:sizes[0]], frames[0].view(np.int32))   # the identity row: bit for bit


@pytest.mark.parametrize("votes", [1, 4])
def test_hundreds_of_workgroups_per_frame(hip, votes):
    """Enough rows that every frame's partial minima come from a few hundred workgroups spread over the chip (the fold by the
    workgroup that draws the frame's last ticket), each with its minimum in a random row."""
    sizes = [50000, 30001]
    frames = make_frames(sizes, 4, seed=5)
    params = make_params(votes, 2, seed=8)
    got = run_kernels(hip, device_points(frames, False), [0, 50000, 80001], params, votes, 0.05)
    check_equal(got, frames, params, votes, 0.05)


@pytest.mark.parametrize("votes", [1, 4])
def test_minimum_in_the_last_and_in_the_first_row(hip, votes):
    """Frame 0 (257 rows: its last row is alone in the second workgroup) has its minimum in its LAST row, frame 1 in its FIRST;
    z keeps its place under every vote (rotation about z, positive scale, jitter ~0.1), all three axes under the identity."""
    sizes = [257, 300]
    frames = make_frames(sizes, 4, seed=77)
    frames[0][-1, :3] = -500.0
    frames[1][0, :3] = -700.0
    params = make_params(votes, 2, seed=3)
    offsets = [0, 257, 557]
    got = run_kernels(hip, device_points(frames, False), offsets, params, votes, 0.05)
    check_equal(got, frames, params, votes, 0.05)
    feats, unshifted, coords, mins, _ = got
    n = 557
    assert np.array_equal(unshifted[256], mins[0]) and np.array_equal(coords[256], [0, 0, 0])
    for v in range(votes):
        assert unshifted[v * n + 256, 2] == mins[v * 2 + 0, 2] and unshifted[v * n + 257, 2] == mins[v * 2 + 1, 2]
        assert (unshifted[v * n:v * n + 256, 2] > mins[v * 2, 2]).all() and (unshifted[v * n + 258:(v + 1) * n, 2] > mins[v * 2 + 1, 2]).all()


def test_fixture_cases_on_the_device(hip, fx):
    """The reference's recorded outputs, straight from the kernels: the three training draws (one vote each), the ten votes in one
    call, and the half-voxel rows under the identity at a voxel of 0.25 (ties to even, both signs)."""
    pts = device_points(fx.frames, False)
    offsets = [0, 512, 813]
    for k in range(N_TRAIN):
        params, _ = fx.train_params(k)
        feats, _, coords, _, _ = run_kernels(hip, pts, offsets, params, 1, fx.voxel)
        for f in range(2):
            xyz, pc, _, _ = fx.recorded(k, f)
            rows = slice(offsets[f], offsets[f + 1])
            assert np.array_equal(feats[rows, :3], xyz) and np.array_equal(coords[rows], pc)
    params, _ = fx.tta_params()
    feats, _, coords, _, _ = run_kernels(hip, pts, offsets, params, N_VOTES, fx.voxel)
    for v in range(N_VOTES):
        for f in range(2):
            xyz, pc, _, _ = fx.recorded(N_TRAIN + v, f)
            rows = slice(v * 813 + offsets[f], v * 813 + offsets[f + 1])
            assert np.array_equal(feats[rows, :3], xyz) and np.array_equal(coords[rows], pc)
            assert np.array_equal(feats[rows, 3], fx.frames[f][:, 3])
    feats, _, coords, _, _ = run_kernels(hip, pts, offsets, T.identity_params(2), 1, fx.voxel)
    assert np.array_equal(feats.view(np.int32), np.concatenate(fx.frames).view(np.int32))
    for f in range(2):
        assert np.array_equal(coords[offsets[f]:offsets[f + 1]], fx.g["plain_pc_f%d" % f].astype(np.int32))


def test_bad_arguments_are_refused(hip):
    """PCS_EINVAL before anything is launched: the outputs keep what they held."""
    lib = native.load_library()
    n, c, nf, v = 8, 4, 1, 1
    pts = torch.zeros(n, c, device="cuda")
    off = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    par = torch.from_numpy(T.identity_params(1)).cuda()
    feats = torch.full((n, c), 7.0, device="cuda")
    coords = torch.full((n, 3), 7, dtype=torch.int32, device="cuda")
    mins = torch.full((1, 3), 7, dtype=torch.int32, device="cuda")
    scenes = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    null = ctypes.c_void_p(0)
    st = native._stream()

    need = lib.pcs_scan_transform_ws_bytes(n, nf, v)
    assert need > 0 and lib.pcs_scan_transform_ws_bytes(-1, nf, v) < 0 and lib.pcs_scan_transform_ws_bytes(n, nf, MAXV + 1) < 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def transform(points=p(pts), n=n, c=c, off=p(off), nf=nf, par=p(par), v=v, voxel=0.05, feats=p(feats), coords=p(coords), mins=p(mins),
                  ws=p(ws), ws_bytes=need):
        return lib.pcs_scan_transform(points, n, c, off, nf, par, v, voxel, feats, coords, mins, ws, ws_bytes, st)

    def shift(coords=p(coords), n=n, off=p(off), nf=nf, mins=p(mins), v=v, scenes=p(scenes)):
        return lib.pcs_scan_shift(coords, n, off, nf, mins, v, scenes, st)

    bad = [transform(points=null), transform(off=null), transform(par=null), transform(feats=null), transform(coords=null),
           transform(mins=null), transform(ws=null), transform(n=-1), transform(c=2), transform(c=native.HipBackend.MAX_COLUMNS + 1), transform(v=0),
           transform(v=MAXV + 1), transform(nf=0), transform(voxel=0.0),
           shift(coords=null), shift(off=null), shift(mins=null), shift(scenes=null), shift(n=-1), shift(v=0), shift(v=MAXV + 1), shift(nf=0)]
    assert bad == [-1] * len(bad), bad     # PCS_EINVAL
    assert b"pcs_scan_shift" in lib.pcs_last_error()
    assert transform(ws_bytes=need - 1) == -2     # PCS_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((feats == 7).all()) and bool((coords == 7).all()) and bool((mins == 7).all()) and bool((scenes == 7).all())
    with pytest.raises(ValueError):
        hip.scan_transform(pts, [0, n], T.identity_params(2), 1, 0.05)    # two parameter rows for one (vote, frame)
    with pytest.raises(RuntimeError, match="pcs_scan_transform"):
        hip.scan_transform(pts, [0, n], T.identity_params(MAXV + 1), MAXV + 1, 0.05)
    assert transform() == 0 and shift() == 0


# ---- batch level ---------------------------------------------------------------------------------------------------------
def _cuda(raw):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}


def _same(a, b):
    assert isinstance(a, SparseTensor) and isinstance(b, SparseTensor)
    assert a.F.dtype == b.F.dtype and a.C.dtype == b.C.dtype, (a.F.dtype, b.F.dtype, a.C.dtype, b.C.dtype)
    assert torch.equal(a.F.cpu(), b.F.cpu()) and torch.equal(a.C.cpu(), b.C.cpu())


@pytest.mark.parametrize("n_points", [3000, None], ids=["equal-lengths", "unequal-lengths"])
def test_identity_batch_equals_device_collate(hip, n_points):
    from openpcseg_amd.workloads import synthetic
    if n_points is None:
        raw = _cuda(raw_of([synthetic.make_scan(0, 3000), synthetic.make_scan(1, 1777), synthetic.make_scan(2, 2500)]))
    else:
        raw = _cuda(synthetic.make_raw_batch([0, 1], n_points=n_points))
    got, want = T.device_batch(raw), synthetic.device_collate(raw)
    assert set(got) == {"lidar", "targets"}
    _same(got["lidar"], want["lidar"])
    _same(got["targets"], want["targets"])


@pytest.mark.parametrize("mode", ["train", "tta"])
def test_eval_batch_equals_the_host_composition(hip, fx, mode):
    """device_batch(eval_maps=True) = transform_scan_host -> host sparse_quantize -> sparse_collate_fn, tensor by tensor; on the
    fixture's frames also the reference's recorded inds / inverse_map."""
    raw = raw_of(fx.frames, labels_seed=5)
    if mode == "train":
        params, votes = fx.train_params(1)[0], 1
    else:
        params, votes = fx.tta_params()[0], N_VOTES
    got = T.device_batch(_cuda(raw), voxel_size=fx.voxel, params=params, votes=votes, eval_maps=True)
    want = host_batch(raw, params, votes, fx.voxel)
    for name in ("lidar", "targets", "targets_mapped", "inverse_map"):
        _same(got[name], want[name])
    assert got["num_points"] == want["num_points"].reshape(-1).tolist()
    scene_v, scene_p = got["lidar"].C[:, 3].cpu().numpy(), got["inverse_map"].C[:, 3].cpu().numpy()
    for v in range(votes):
        for f in range(2):
            xyz, pc, inds, inverse = fx.recorded((1 if mode == "train" else N_TRAIN + v), f)
            s = v * 2 + f
            assert np.array_equal(got["inverse_map"].F.cpu().numpy()[scene_p == s], inverse)
            assert np.array_equal(got["lidar"].C.cpu().numpy()[scene_v == s][:, :3], pc[inds])
            assert np.array_equal(got["lidar"].F.cpu().numpy()[scene_v == s][:, :3], xyz[inds])


def test_empty_frame_raises_on_the_host(hip):
    raw = _cuda(raw_of([np.ones((5, 4), dtype=np.float32), np.zeros((0, 4), dtype=np.float32)]))
    with pytest.raises(ValueError, match="empty frame"):
        T.device_batch(raw)
