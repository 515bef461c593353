"""The host side every device input builder shares: hostdata.raw_frames, the one reader of a raw batch,
hostdata.scene_row_offsets, and the one loop behind transform.tta_params and rangeview.tta_params. No GPU: the refusals come before
any launch, the prefix runs on host tensors, the draws are NumPy."""
import numpy as np
import pytest
import torch

from openpcseg_amd import rangeview, transform
from openpcseg_amd.hostdata import raw_frames, scene_row_offsets


def _raw(sizes=(5, 3), columns=4, **changes):
    n = sum(sizes)
    raw = {"points": torch.zeros(n, columns), "labels": torch.zeros(n, dtype=torch.int64), "num_frames": len(sizes),
           "offsets": [0] + np.cumsum(sizes).tolist()}
    raw.update(changes)
    return raw


def _read(raw, **kw):
    return raw_frames(raw, "a_builder", "a_host_form", **kw)


def test_raw_frames_refuses_host_tensors_last():
    """A well-formed batch of host tensors gets as far as the device check, and the message names the caller and the host form."""
    with pytest.raises(RuntimeError, match="HIP device tensor") as e:
        _read(_raw())
    assert "a_builder" in str(e.value) and "a_host_form" in str(e.value)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        _read(_raw(points=np.zeros((8, 4), dtype=np.float32)))


def test_raw_frames_column_requirement():
    with pytest.raises(ValueError, match=r"\(n, C >= 3\)"):
        _read(_raw(columns=2))
    with pytest.raises(ValueError, match=r"\(n, C >= 5\)"):
        _read(_raw(columns=4), min_columns=5)
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        _read(_raw(columns=5), min_columns=4, exact_columns=True)
    with pytest.raises(ValueError, match=r"\(n, 4\)"):
        _read(_raw(columns=3), min_columns=4, exact_columns=True)
    with pytest.raises(ValueError):
        _read(_raw(points=torch.zeros(8)))


@pytest.mark.parametrize("changes", [{"num_frames": 3}, {"offsets": [1, 5, 8]}, {"offsets": [0, 5, 7]}, {"offsets": [0, 5, 9]},
                                     {"offsets": [0, 5, 4, 8], "num_frames": 3}, {"labels": torch.zeros(7, dtype=torch.int64)}])
@pytest.mark.parametrize("allow_empty", [False, True])
def test_raw_frames_refuses_bad_boundaries(changes, allow_empty):
    """len(offsets) != num_frames + 1, offsets[0] != 0, offsets[-1] != n (both sides), a decreasing boundary, labels of another length."""
    with pytest.raises(ValueError, match="frame boundaries"):
        _read(_raw(**changes), allow_empty=allow_empty)


def test_raw_frames_empty_frame_depends_on_the_caller():
    raw = _raw(sizes=(5, 0, 3))
    with pytest.raises(ValueError, match="empty frame"):
        _read(raw)
    with pytest.raises(RuntimeError, match="HIP device tensor"):   # the mixer's setting lets it pass, up to the device check
        _read(raw, allow_empty=True)


def test_raw_frames_labels():
    raw = _raw()
    del raw["labels"]
    with pytest.raises(ValueError, match="labels"):
        _read(raw, need_labels=True)
    with pytest.raises(RuntimeError, match="HIP device tensor"):   # optional otherwise
        _read(raw)


@pytest.mark.parametrize("col,scenes", [([0, 0, 0], 1), ([0, 0, 1, 3, 3, 3], 5), ([], 4)])
def test_scene_row_offsets(col, scenes):
    """Against np.bincount + cumsum: one scene; five with an empty scene in the middle and one at the end; no rows at all."""
    for dtype in (torch.int32, torch.int64):
        got = scene_row_offsets(torch.tensor(col, dtype=dtype), scenes)
        want = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(col, dtype=np.int64), minlength=scenes))])
        assert got.dtype == torch.int64 and got.shape == (scenes + 1,) and np.array_equal(got.numpy(), want)
    if not col:
        assert not got.any()


def test_fusion_draws_walk_frame_vote_scale_cut():
    """The reference's order restated HERE: frame by frame, vote by vote, uniform for the scale, then rand for the cut."""
    nf, nv = 2, 3
    rng = np.random.RandomState(7)
    want, want_cuts = transform.identity_params(nv * nf), np.empty(nv * nf)
    for f in range(nf):
        for v in range(nv):
            theta = transform.TTA_ANGLES[v] * np.pi / 8.0
            want[v * nf + f, :3] = (np.cos(theta), np.sin(theta), rng.uniform(0.9, 1.1))
            want_cuts[v * nf + f] = rng.rand()
    params, cuts = rangeview.tta_params(nf, nv, rng=np.random.RandomState(7))
    assert params.dtype == np.float64 and params.shape == (nv * nf, 8) and cuts.dtype == np.float64 and cuts.shape == (nv * nf,)
    assert np.array_equal(params, want) and np.array_equal(cuts, want_cuts)


def test_voxel_draws_consume_no_cut():
    """transform.tta_params draws the scales alone: its scale column is that of a walk without the rand() calls."""
    nf, nv = 2, 3
    rng = np.random.RandomState(7)
    want = np.empty(nv * nf)
    for f in range(nf):
        for v in range(nv):
            want[v * nf + f] = rng.uniform(0.9, 1.1)
    rs = np.random.RandomState(7)
    params = transform.tta_params(nf, nv, rng=rs)
    assert isinstance(params, np.ndarray) and params.shape == (nv * nf, 8) and np.array_equal(params[:, 2], want)
    assert rs.rand() == rng.rand()   # both generators stand at the same place
    assert not np.array_equal(params[:, 2], rangeview.tta_params(nf, nv, rng=np.random.RandomState(7))[0][:, 2])


@pytest.mark.parametrize("num_votes", [0, 11])
def test_draws_refuse_vote_counts(num_votes):
    with pytest.raises(ValueError, match="num_votes"):
        transform.tta_params(2, num_votes)
    with pytest.raises(ValueError, match="num_votes"):
        rangeview.tta_params(2, num_votes)
