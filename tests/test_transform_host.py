"""The dataset transform on the host: openpcseg_amd.transform against the reference's recorded outputs
(tests/golden/transform_golden.npz: aug_points of R:tools/utils/common/seg_utils.py:43-100, the rounding and shift of
R:pcseg/data/dataset/semantickitti/semantickitti_voxel.py:112-113 and the reference's sparse_quantize, on two frames of 512 and
301 rows). The restatement is elementwise float64 in the reference's order, so the bound is equality: float32 equality of the
augmented points, integer equality of the voxel coordinates."""
import os
import re

import numpy as np
import pytest
import torch

from openpcseg_amd import native
from openpcseg_amd import transform as T
from openpcseg_amd.hostdata import raw_frames, sparse_quantize
from transform_cases import N_TRAIN, N_VOTES, Fixture, host_batch, raw_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return Fixture()


def _check_case(fx, case, f, params_row):
    xyz, pc, inds, inverse = fx.recorded(case, f)
    got, got_pc = T.transform_scan_host(fx.frames[f], params_row, fx.voxel)
    assert got.dtype == np.float32 and got_pc.dtype == np.int32
    assert np.array_equal(got[:, :3], xyz), "case %d frame %d: %d float32 mismatches" % (case, f, int((got[:, :3] != xyz).sum()))
    assert np.array_equal(got[:, 3], fx.frames[f][:, 3])
    assert np.array_equal(got_pc, pc), "case %d frame %d: %d voxel mismatches" % (case, f, int((got_pc != pc).sum()))
    _, i2, inv2 = sparse_quantize(got_pc, return_index=True, return_inverse=True)
    assert np.array_equal(i2, inds) and np.array_equal(inv2, inverse)


@pytest.mark.parametrize("k", range(N_TRAIN))
def test_training_draws_equal_the_reference(fx, k):
    """Same NumPy seed -> the augmentation the reference's worker drew: outputs equal, and the generator left in the same state."""
    params, state = fx.train_params(k)
    assert params.shape == (2, 8) and fx.state_matches(state, "train%d" % k)
    assert set(np.abs(params[:, 3:5]).ravel()) == {1.0}
    for f in range(2):
        _check_case(fx, k, f, params[f])


def test_tta_votes_equal_the_reference(fx):
    params, state = fx.tta_params()
    assert params.shape == (2 * N_VOTES, 8) and fx.state_matches(state, "tta")
    theta = np.array(T.TTA_ANGLES) * np.pi / 8.0
    assert np.array_equal(params[0::2, 0], np.cos(theta)) and np.array_equal(params[1::2, 1], np.sin(theta))
    assert np.array_equal(params[:, 3:], T.identity_params(20)[:, 3:])          # no flip, no jitter
    assert params[:, 2].min() >= fx.scale_range[0] and params[:, 2].max() <= fx.scale_range[1] and len(set(params[:, 2])) == 20
    for v in range(N_VOTES):
        for f in range(2):
            _check_case(fx, N_TRAIN + v, f, params[v * 2 + f])
    with pytest.raises(ValueError):
        T.tta_params(1, 11)


def test_draws_take_any_generator_and_switches(fx):
    """A RandomState of its own is consumed like the module; a switched-off augmentation draws nothing and stays the identity."""
    a = T.draw_train_params(3, rng=np.random.RandomState(5))
    np.random.seed(5)
    assert np.array_equal(a, T.draw_train_params(3))
    rs = np.random.RandomState(5)
    before = rs.get_state()[1].copy()
    assert np.array_equal(T.draw_train_params(2, rng=rs, rotate=False, scale=False, flip=False, jitter=False), T.identity_params(2))
    assert np.array_equal(rs.get_state()[1], before)
    only_scale = T.draw_train_params(2, rng=np.random.RandomState(7), rotate=False, flip=False, jitter=False, scale_range=(0.95, 1.05))
    assert np.array_equal(only_scale[:, 2], np.random.RandomState(7).uniform(0.95, 1.05, size=2))


def test_identity_returns_the_input_bit_for_bit(fx):
    for f in range(2):
        got, pc = T.transform_scan_host(fx.frames[f], T.identity_params(1)[0], fx.voxel)
        assert np.array_equal(got.view(np.int32), fx.frames[f].view(np.int32))
        assert np.array_equal(pc, fx.g["plain_pc_f%d" % f].astype(np.int32))     # what the reference's rounding gave, un-augmented
    # the hand-placed rows sit exactly between two voxels, with both signs: np.round decides half to even
    q = fx.frames[0][:fx.half_rows, :3] / np.float32(fx.voxel)
    assert np.array_equal(np.abs(q - np.trunc(q)), np.full_like(q, 0.5)) and (q < 0).any() and (q > 0).any()
    assert (np.trunc(q) % 2 == 0).any() and (np.trunc(q) % 2 != 0).any()     # ties that go towards and away from zero


def test_empty_frame_raises():
    with pytest.raises(ValueError, match="empty frame"):
        T.transform_scan_host(np.zeros((0, 4), dtype=np.float32), T.identity_params(1)[0], 0.05)
    raw = raw_of([np.ones((5, 4), dtype=np.float32), np.zeros((0, 4), dtype=np.float32), np.ones((3, 4), dtype=np.float32)])
    with pytest.raises(ValueError, match="empty frame"):
        raw_frames(raw, "transform.device_batch", "transform_scan_host")


def test_host_batch_layout(fx):
    """The host composition the device batch is held to: scene v * F + f = vote v of frame f, per-scene inverse maps."""
    raw = raw_of(fx.frames)
    params, _ = fx.tta_params()
    b = host_batch(raw, params[:6], 3, fx.voxel)
    assert b["lidar"].C[:, 3].unique().tolist() == list(range(6)) and b["inverse_map"].F.shape[0] == 3 * (512 + 301)
    assert b["num_points"].reshape(-1).tolist() == [512, 301] * 3
    _, _, _, inverse = fx.recorded(N_TRAIN + 1, 1)                       # vote 1 of frame 1 = scene 3
    assert np.array_equal(b["inverse_map"].F[b["inverse_map"].C[:, 3] == 3].numpy(), inverse)


def test_symbols_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    lib = native.load_library()
    for name in ("pcs_scan_transform", "pcs_scan_shift", "pcs_scan_transform_ws_bytes"):
        assert re.search(r"\bint(64_t)? %s\(" % name, hdr) and name in native.SIGNATURES and hasattr(lib, name)
    assert lib.pcs_scan_transform_ws_bytes(1440000, 12, 1) == 4 * 12 * (1 + (1024 // 12) * 3)   # tickets + partial minima per frame
    assert "seg_utils.py:43-100" in hdr and "semantickitti_voxel.py" in hdr     # the reference lines they replace
    assert int(re.search(r"#define PCS_ABI_VERSION (\d+)", hdr).group(1)) == 12 == native.ABI_VERSION == lib.pcs_abi_version()
    assert int(re.search(r"#define PCS_SCAN_MAX_VOTES (\d+)", hdr).group(1)) == native.HipBackend.MAX_VOTES
    assert int(re.search(r"#define PCS_SCAN_MAX_COLUMNS (\d+)", hdr).group(1)) == native.HipBackend.MAX_COLUMNS


def test_device_batch_refuses_host_tensors(fx):
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        T.device_batch(raw_of(fx.frames), voxel_size=fx.voxel)
    be = native.HipBackend()
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        be.scan_transform(torch.zeros(4, 4), [0, 4], T.identity_params(1), 1, 0.05)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        be.scan_shift(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int32), torch.tensor([0, 4]), 1)
