"""inference.predict_tta: an evaluation under the reference's test-time augmentation, from raw scans in HBM to voted predictions.

The votes are held to the float64 softmax sum of the logits the call itself used, mapped to the points through HOST-built inverse
maps (transform_cases.host_batch: transform_scan_host, host sparse_quantize, sparse_collate_fn), within num_votes * 1e-6: the
per-pass bound tests/test_predict_tail.py::test_tail_softmax_votes derives for the tail kernel (per pass < 5e-7 for c = 20 and a
running sum <= 4; here the sum reaches num_votes <= 10, half an ulp of which is 4.8e-7: the same margin of two holds)."""
import numpy as np
import pytest
import torch

from openpcseg_amd.inference import SegEvaluator, predict_tta
from seeded import seeded_state
from transform_cases import host_batch, raw_of

pytestmark = pytest.mark.gpu

C = 20
VOXEL = 0.05


@pytest.fixture(scope="module")
def model(hip):
    from openpcseg_amd.workloads import minkunet as mk
    m = mk.MinkUNet(num_class=C, num_layer=mk.MK18_LAYERS, cr=0.25).cuda().eval()
    seeded_state(m)
    return m


@pytest.fixture(scope="module")
def raw():
    from openpcseg_amd.workloads.synthetic import make_scan
    return raw_of([make_scan(1, 2000), make_scan(2, 1913)], labels_seed=9, num_classes=C)


def _cuda(raw):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}


def float64_votes(raw, out, num_votes):
    """Sum over the votes of softmax(logits of the point's voxel) in float64, through the host-built batch."""
    nf, off = raw["num_frames"], raw["offsets"]
    host = host_batch(raw, out["params"], num_votes, VOXEL)
    scene_v, scene_p, inv = host["lidar"].C[:, 3].numpy(), host["inverse_map"].C[:, 3].numpy(), host["inverse_map"].F.numpy()
    ref = np.zeros((off[-1], C))
    assert len(out["logits"]) == num_votes
    for v, lg in enumerate(out["logits"]):
        lg = lg.cpu().numpy().astype(np.float64)
        first = int((scene_v < v * nf).sum())
        assert lg.shape == (int(((scene_v >= v * nf) & (scene_v < (v + 1) * nf)).sum()), C)
        for f in range(nf):
            s = v * nf + f
            rows = lg[int((scene_v < s).sum()) - first + inv[scene_p == s]]
            e = np.exp(rows - rows.max(1, keepdims=True))
            ref[off[f]:off[f + 1]] += e / e.sum(1, keepdims=True)
    return ref


def check(raw, out, num_votes, evaluator=None):
    n = raw["offsets"][-1]
    votes = out["votes"].cpu().numpy()
    assert votes.shape == (n, C) and votes.dtype == np.float32
    err = float(np.abs(votes.astype(np.float64) - float64_votes(raw, out, num_votes)).max())
    print("votes: max abs error %.3e over %d votes (bound %.1e)" % (err, num_votes, num_votes * 1e-6))
    assert err <= num_votes * 1e-6, err
    assert np.allclose(votes.sum(1), num_votes, atol=1e-4)
    pred = out["pred"].cpu().numpy()
    assert pred.dtype == np.int64 and np.array_equal(pred, votes.argmax(1))
    assert out["point_offset"] == raw["offsets"]
    if evaluator is not None:
        hist = evaluator.hist.cpu().numpy()
        labels = raw["labels"].numpy()
        assert int(hist.sum()) == n                                   # every label is in [0, C): counted once, not once per vote
        want = np.bincount(C * labels + pred, minlength=C * C).reshape(C, C)
        assert np.array_equal(hist, want) and int(evaluator.bad) == 0


@pytest.mark.parametrize("num_votes", [3, 10])
def test_votes_prediction_and_histogram(model, raw, num_votes):
    ev = SegEvaluator(C)
    out = predict_tta(model, _cuda(raw), num_votes=num_votes, evaluator=ev, voxel_size=VOXEL, rng=np.random.RandomState(num_votes),
                      return_logits=True)
    check(raw, out, num_votes, ev)
    theta = np.array([0, 1, -1, 2, -2, 6, -6, 7, -7, 8][:num_votes]) * np.pi / 8.0
    assert np.array_equal(out["params"][0::2, 0], np.cos(theta)) and out["params"].shape == (2 * num_votes, 8)
    plain = predict_tta(model, _cuda(raw), num_votes=num_votes, voxel_size=VOXEL, rng=np.random.RandomState(num_votes))
    assert "logits" not in plain and torch.equal(plain["pred"], out["pred"]) and torch.equal(plain["votes"], out["votes"])


def test_vote_chunks(model, raw):
    """One vote per forward and all votes in one forward: each within the bound of its own logits; a chunk that does not divide
    the votes; the same draws either way."""
    outs = {}
    for chunk in (1, None, 2):
        ev = SegEvaluator(C)
        outs[chunk] = predict_tta(model, _cuda(raw), num_votes=3, evaluator=ev, voxel_size=VOXEL, rng=np.random.RandomState(4),
                                  vote_chunk=chunk, return_logits=True)
        check(raw, outs[chunk], 3, ev)
    assert np.array_equal(outs[1]["params"], outs[None]["params"])


def test_refusals(model, raw):
    model.train()
    try:
        with pytest.raises(RuntimeError):
            predict_tta(model, _cuda(raw), num_votes=2)
    finally:
        model.eval()
    with pytest.raises(TypeError):
        predict_tta(torch.nn.Linear(4, C).cuda().eval(), _cuda(raw), num_votes=2)
    with pytest.raises(ValueError):
        predict_tta(model, _cuda(raw), num_votes=11)
