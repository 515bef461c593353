"""The package's own RPVNet graph (openpcseg_amd/workloads/rpvnet.py) against the fixtures the REFERENCE's RPVNet wrote
(R:pcseg/model/segmentor/fusion/rpvnet/rpvnet.py run on its own CPU backend by tests/golden/make_golden.py), without the reference's
sources: state_dict layout, the two small train-mode fixtures on the pure-PyTorch path, and on the GPU config 5 at full size (fp32
and bf16 autocast) and the inference mode. Bounds are those the existing tests hold the reference's own graph to on the same
fixtures (tests/test_reference_models.py, tests/test_fullsize_parity.py, tests/test_inference_fold.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fullsize as fs  # noqa: E402

import openpcseg_amd  # noqa: E402
from openpcseg_amd import cpu_fallback, native  # noqa: E402
from openpcseg_amd.sparse import SparseTensor  # noqa: E402
from openpcseg_amd.workloads.rpvnet import RPVNet  # noqa: E402
from seeded import seeded_state  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
POINT_NORMS = ["point_transforms.%d.1" % i for i in range(4)]


def _record_merges(monkeypatch, be, calls):
    orig = be.range_point_merge
    monkeypatch.setattr(be, "range_point_merge", lambda *a: (calls.append((a[5].shape[1], "bn" if a[6] is not None else "add")), orig(*a))[1])


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_parameter_names_are_the_references():
    g = np.load(os.path.join(GOLDEN, "config5_golden.npz"))
    cfg = fs.MODEL_CFG["config5"]
    model = RPVNet(in_dim=cfg["IN_FEATURE_DIM"], num_layer=cfg["NUM_LAYER"], cr=cfg["cr"])
    names = [name for name, _ in model.named_parameters()]
    assert len(names) == 283 == len(g["grad_names"]) and set(names) == set(str(n) for n in g["grad_names"])
    assert sum(n.startswith("range_branch.") for n in names) == 76
    assert [n for n in names if n.startswith("point_transforms.3.")] == [
        "point_transforms.3.0.weight", "point_transforms.3.0.bias", "point_transforms.3.1.weight", "point_transforms.3.1.bias"]
    assert [tuple(model.point_transforms[i][0].weight.shape) for i in range(4)] == [(56, 5), (448, 56), (224, 448), (168, 224)]
    small = dict(num_layer=[2] * 8, cr=0.25)
    model = RPVNet(**small)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    seeded_state(model)
    for k, v in model.state_dict().items():
        if v.dtype.is_floating_point:
            assert v.shape == before[k].shape and not torch.equal(v, before[k]), k
    twin = RPVNet(**small)
    twin.load_state_dict(model.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))


@pytest.mark.parametrize("switch", ["1", "0"])
@pytest.mark.parametrize("tag,in_dim,num_class,smoothing", [("rpv", 4, 20, 0.1), ("rpw", 5, 23, 0.0)])
def test_small_fixtures_on_the_pytorch_cpu_path(monkeypatch, tag, in_dim, num_class, smoothing, switch):
    """rpv_* / rpw_* of models_e2e_golden.npz (cr 0.25, mk18, train mode with the dropouts frozen as the fixture froze them): logits
    and loss within the 1e-3 tests/test_reference_models.py allows the reference's own graph. Widths 8 / 64 / 32 / 24: hops 0 and 3
    run the fused BatchNorm pass first and the merge adds its output."""
    monkeypatch.setenv("PCS_RANGE_MERGE", switch)
    gold = np.load(os.path.join(GOLDEN, "models_e2e_golden.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with cpu_fallback.enabled() as be:
        calls = []
        _record_merges(monkeypatch, be, calls)
        model = RPVNet(num_class=num_class, in_dim=in_dim, num_layer=[2] * 8, cr=0.25, label_smoothing=smoothing)
        seeded_state(model)
        model.train()
        fs.freeze_dropout(model)
        coords = t(gold[tag + "_coords"])
        out = model({"lidar": SparseTensor(t(gold[tag + "_feats"]), coords), "targets": SparseTensor(t(gold[tag + "_labels"]), coords),
                     "range_image": t(gold[tag + "_range_image"]), "range_pxpy": t(gold[tag + "_range_pxpy"])})
        out["loss"].backward()
    assert calls == ([(8, "add"), (64, "bn"), (32, "bn"), (24, "add")] if switch == "1" else [])
    ref = gold[tag + "_logits"]
    assert out["logits"].shape == ref.shape and ref.shape[1] == num_class
    assert np.abs(out["logits"].detach().numpy() - ref).max() < 1e-3
    assert abs(float(out["loss"].detach()) - float(gold[tag + "_loss"])) < 1e-3
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(int(m.num_batches_tracked) == 1 for m in model.modules() if hasattr(m, "num_batches_tracked"))


# ---- GPU: config 5 at full size, reference-free ------------------------------------------------------------------------------
# (logit max-abs err, loss abs err, matrix abs-sum rel, matrix sample / abs-max, any abs-sum rel, any sample / abs-max):
# tests/test_fullsize_parity.py BOUNDS["config5/reference+fuse"], the project's bound for the reference's graph on these kernels
BOUNDS_CONFIG5 = (8e-4, 2e-5, 4e-4, 6e-4, 1e-3, 4e-3)
# (max err / rms, mean err / rms, gradient abs-sum rel, arg-max agreement): tests/test_fullsize_parity.py REF_AMP_BOUNDS["config5"]
REF_AMP_BOUNDS_CONFIG5 = (0.32, 0.016, 0.20, 0.982)
_MEASURED = {}


def _record(name, m):
    _MEASURED[name] = m
    print("\n[rpvnet parity] %s: %s" % (name, json.dumps(m)))
    out = os.environ.get("PCS_MEASURED_DIR", "")   # where a run keeps its measured records, if it keeps any
    if out and os.path.isdir(out):
        with open(os.path.join(out, "rpvnet_parity_measured.json"), "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def config5():
    g = np.load(os.path.join(GOLDEN, "config5_golden.npz"))
    assert int(g["n_points"]) == -1
    batch = fs.build_inputs("config5", SparseTensor)
    crcs = fs.input_crcs("config5", batch)
    assert len(crcs) == 5
    for k, v in crcs.items():
        assert int(v) == int(g[k]), "input %s differs from the frame the reference ran on" % k
    return g, batch


def _step(g, host_batch, amp=None):
    dev = torch.device("cuda:0")
    batch = fs.to_device("config5", host_batch, dev, SparseTensor)
    cfg = fs.MODEL_CFG["config5"]
    model = RPVNet(num_class=20, in_dim=cfg["IN_FEATURE_DIM"], num_layer=cfg["NUM_LAYER"], cr=cfg["cr"],
                   label_smoothing=cfg["LABEL_SMOOTHING"], dropout=cfg["DROPOUT_P"])
    seeded_state(model)
    fs.freeze_dropout(model.to(dev).train())
    if amp is None:
        out = model(batch)
    else:
        with torch.autocast("cuda", dtype=amp):
            out = model(batch)
    out["loss"].backward()
    logits, loss = out["logits"].detach().float().cpu().numpy(), float(out["loss"].detach())
    m = fs.compare(g, logits, loss, fs.model_grads(model))
    m["loss_ref"] = float(g["loss"])
    return logits, loss, m


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["1", "0"])
def test_config5_fullsize_fp32(hip, monkeypatch, config5, switch):
    """One training step of RPVNet-34 cr 1.75 on the full frame of config5_golden.npz: logits, loss and the 283 gradient fingerprints."""
    monkeypatch.setenv("PCS_RANGE_MERGE", switch)
    g, batch = config5
    calls = []
    _record_merges(monkeypatch, native.backend(), calls)
    _, _, m = _step(g, batch)
    assert calls == ([(56, "add"), (448, "bn"), (224, "bn"), (168, "add")] if switch == "1" else [])
    _record("config5/workload" + ("" if switch == "1" else "/literal"), m)
    lo, ls, gm, gms, ga, gas = BOUNDS_CONFIG5
    assert m["logit_max_abs_err"] < lo, m
    assert m["colsum_err_per_row"] < lo, m
    assert m["abssum_rel_err"] < 1e-4, m
    assert m["loss_abs_err"] < ls * max(1.0, abs(m["loss_ref"])), m
    assert m["grad_matrix_abssum_rel_err"] < gm and m["grad_matrix_sample_err_rel_max"] < gms, m
    assert m["grad_abssum_rel_err"] < ga and m["grad_sample_err_rel_max"] < gas, m
    assert m["grad_dead_max_over_G"] < 1e-3, m


@pytest.mark.gpu
def test_config5_fullsize_bf16_autocast(hip, monkeypatch, config5):
    """Against the fp32 fixture under bf16 autocast: the bounds the reference's own graph is held to."""
    monkeypatch.setenv("PCS_RANGE_MERGE", "1")
    g, batch = config5
    calls = []
    _record_merges(monkeypatch, native.backend(), calls)
    logits, loss, m = _step(g, batch, amp=torch.bfloat16)
    step, ref = int(g["row_step"]), g["logits_rows"]
    rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    err = np.abs(logits[::step] - ref)
    m.update({"logit_rms": rms, "logit_max_err_over_rms": float(err.max() / rms), "logit_mean_err_over_rms": float(err.mean() / rms),
              "argmax_agreement": float((logits[::step].argmax(1) == ref.argmax(1)).mean()), "merge_calls": [list(c) for c in calls]})
    _record("config5/workload/bf16", m)
    assert np.isfinite(logits).all() and np.isfinite(loss)
    bmax, bmean, bgrad, bagree = REF_AMP_BOUNDS_CONFIG5
    assert m["logit_max_err_over_rms"] < bmax, m
    assert m["logit_mean_err_over_rms"] < bmean, m
    assert m["argmax_agreement"] > bagree, m
    assert m["grad_abssum_rel_err"] < bgrad, m


# ---- GPU: inference ------------------------------------------------------------------------------------------------------
def _eval_frame():
    from openpcseg_amd.hostdata import sparse_collate_fn, sparse_quantize
    from openpcseg_amd.workloads.synthetic import make_scan
    pts = make_scan(0, 20000)
    pc = np.round(pts[:, :3] / 0.05).astype(np.int32)
    pc -= pc.min(0, keepdims=1)
    _, inds, inverse = sparse_quantize(pc, return_index=True, return_inverse=True)
    labels = np.random.default_rng(0).integers(0, 20, size=pts.shape[0]).astype(np.int64)
    b = sparse_collate_fn([{"lidar": SparseTensor(pts[inds], pc[inds]), "targets_mapped": SparseTensor(labels, pc),
                            "inverse_map": SparseTensor(np.asarray(inverse).astype(np.int64), pc),
                            "num_points": np.array([pts.shape[0]])}])
    b["range_image"], b["range_pxpy"] = fs.range_view(b["lidar"].F, h=64, w=512)   # the range view of the voxelised points
    return b


def _logits(model, feats, coords, image, pxpy):
    with torch.no_grad():
        return model({"lidar": SparseTensor(feats.clone(), coords), "range_image": image, "range_pxpy": pxpy})["logits"].float()


@pytest.mark.gpu
def test_inference_freeze_and_predict(hip, monkeypatch):
    """freeze folds the 63 conv + BatchNorm pairs of the mk34 trunk and leaves the four point-MLP norms running (on the merge
    kernel, with the running statistics; cr 1.0: every hop a multiple of 32 wide). Frozen vs unfrozen: the bound of
    tests/test_inference_fold.py, reference = the unfrozen model on the oracle backend with host tensors:
    err(frozen) <= 2 err(unfrozen) + 2e-5 max |ref|."""
    from oracle.adapter import OracleBackend
    from openpcseg_amd.inference import SegEvaluator
    from test_predict_tail import fast_hist_crop, per_class_iu, reference_tail
    monkeypatch.setenv("PCS_RANGE_MERGE", "1")
    model = RPVNet(num_class=20, in_dim=4, cr=1.0).eval()
    seeded_state(model)
    host = _eval_frame()
    hf, hc = host["lidar"].F.clone(), host["lidar"].C.int().contiguous()
    hi, hp = host["range_image"], host["range_pxpy"]
    with monkeypatch.context() as mp_:
        mp_.setattr(native, "_BACKEND", OracleBackend())
        ref = _logits(model, hf, hc, hi, hp).numpy()
    model.cuda()
    feats, coords, image, pxpy = hf.cuda(), hc.cuda(), hi.cuda(), hp.cuda()
    unfrozen = _logits(model, feats, coords, image, pxpy).cpu().numpy()
    report = openpcseg_amd.freeze(model)
    assert report == {"folded": 63, "skipped": POINT_NORMS}
    be = native.backend()
    calls = {"range_point_merge": 0, "bn_apply": 0}
    for name in calls:
        orig = getattr(be, name)
        monkeypatch.setattr(be, name, (lambda o, k: lambda *a, **kw: (calls.__setitem__(k, calls[k] + 1), o(*a, **kw))[1])(orig, name))
    frozen = _logits(model, feats, coords, image, pxpy).cpu().numpy()
    assert calls == {"range_point_merge": 4, "bn_apply": 0}
    ef = float(np.abs(frozen.astype(np.float64) - ref).max())
    eu = float(np.abs(unfrozen.astype(np.float64) - ref).max())
    bound = 2.0 * eu + 2e-5 * float(np.abs(ref).max())
    print("rpvnet fp32: frozen %.3e unfrozen %.3e bound %.3e" % (ef, eu, bound))
    assert ef <= bound, (ef, eu, bound)
    batch = {k: (SparseTensor(v.F.cuda(), v.C.int().cuda()) if isinstance(v, SparseTensor) else v) for k, v in host.items()}
    batch["range_image"], batch["range_pxpy"] = image, pxpy
    ev = SegEvaluator(20)
    out = model.predict(batch, evaluator=ev)
    preds, labels = reference_tail(out["logits"].cpu().numpy(), batch)
    assert np.array_equal(out["point_predict"].cpu().numpy(), np.concatenate(preds)) and out["point_offset"] == [0, 20000]
    hist, iou, miou = ev.compute()
    want = sum(fast_hist_crop(p, l, np.arange(19)) for p, l in zip(preds, labels))
    assert np.array_equal(hist, want) and miou == float(np.nanmean(per_class_iu(want)))
    model.train()
    with pytest.raises(RuntimeError):
        model.predict(batch)
