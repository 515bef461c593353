"""`openpcseg_amd.freeze` on workloads.cylinder.CylinderTS: every conv -> LeakyReLU -> BatchNorm (+ residual) triple as ONE launch
with the BatchNorm as a per-column affine map behind the activation (pcs_conv_epilogue, PCS_EP_POST_AFFINE), `up_subm` with the
skip as its addend, the point MLPs with their BatchNorms folded into the Linear layers.

CPU part (torch-cpu backend): the report, frozen against unfrozen logits, unfreeze, state_dict, the lazy re-fold and the order of
the write-back. GPU part (-m gpu): the 20 000-point scan of test_cylinder_workload.test_eval_and_predict against the unfrozen
model on the oracle backend in fp32, the unfrozen bf16 run of the same session under autocast, and predict on a frozen model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import openpcseg_amd
from openpcseg_amd import cpu_fallback, native
from openpcseg_amd import functional as F
from openpcseg_amd.inference import FoldedDense, PostAffineConv, SegEvaluator
from openpcseg_amd.sparse import SparseTensor
from openpcseg_amd.workloads.cylinder import CylinderTS, cylinder_batch
from openpcseg_amd.workloads.synthetic import make_batch, make_scan
from seeded import seeded_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)   # fullsize.py: the cylinder partition of the full-size fixtures
KEYS = ["point_feature", "point_coord", "voxel_coord", "voxel_label", "point_label", "offset"]
PARITY_JSON = os.path.join(ROOT, "profiles", "cylinder_freeze_parity.json")
REPORT = {"folded": 41, "skipped": ["ReconNet.bn0", "ReconNet.bn0_2", "ReconNet.bn0_3"]}
N_CONVS = 48   # 4 (downCntx) + 4 x 5 (ResBlock: 4 + pool) + 4 x 5 (UpBlock: 4 + up_subm) + 3 (ReconNet) + 1 (logits)


def _small_batch():
    """The batch test_cylinder_workload.test_small_fixture_on_the_pytorch_cpu_path builds (2 500 points)."""
    gold = np.load(os.path.join(GOLDEN, "models_e2e_golden.npz"))
    return {k: torch.from_numpy(np.ascontiguousarray(gold["cyl_" + k])) for k in KEYS}


def _small_model():
    model = CylinderTS(num_class=20, in_dim=9, init_size=8).eval()
    seeded_state(model)
    return model


def _forward(model, batch):
    with torch.no_grad():
        return model(dict(batch))


def _count_calls(monkeypatch, be, names):
    counts = {n: 0 for n in names}
    for n in names:
        if not hasattr(be, n):
            continue
        orig = getattr(be, n)

        def wrapped(*a, _o=orig, _n=n, **kw):
            counts[_n] += 1
            return _o(*a, **kw)
        monkeypatch.setattr(be, n, wrapped, raising=False)
    return counts


def _records(model):
    for m in model.modules():
        rec = m.__dict__.get("_pcs_folds") or {}
        for v in rec.values():
            for f in (v if isinstance(v, list) else [v]):
                if hasattr(f, "folds"):
                    yield f


@pytest.fixture()
def cpu_be():
    with cpu_fallback.enabled() as b:
        yield b


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_report_full_width():
    """cy480 (init_size 32): 36 block triples + 5 dense norms of the model's 44 stop launching; ReconNet's three stay."""
    model = CylinderTS(num_class=20, init_size=32).eval()
    assert sum(1 for m in model.modules() if hasattr(m, "running_mean")) == 44
    assert openpcseg_amd.freeze(model) == REPORT
    recs = list(_records(model))
    assert sum(isinstance(f, PostAffineConv) and f.bn is not None for f in recs) == 36
    assert sum(isinstance(f, PostAffineConv) and f.bn is None for f in recs) == 4      # the four up_subm
    assert sum(isinstance(f, FoldedDense) for f in recs) == 4                          # PPmodel's first Linear takes two norms
    assert openpcseg_amd.unfreeze(model) > 0 and not list(_records(model))


def test_only_positive_finite_slopes_are_claimed():
    """The ABI reads a slope of 0 as "no activation": such a triple keeps its BatchNorm and is reported."""
    model = CylinderTS(num_class=20, init_size=8).eval()
    model.downCntx.act1.negative_slope = 0.0
    model.upBlock0.act2.negative_slope = float("nan")
    rep = openpcseg_amd.freeze(model)
    assert rep["folded"] == 39 and rep["skipped"] == ["downCntx.bn0", "upBlock0.bn2"] + REPORT["skipped"]


def test_frozen_against_unfrozen(cpu_be, monkeypatch):
    """Eval forward on the small batch: logits within the fp32 kernel bound 2e-5 max |unfrozen|, no bn_apply, 48 conv calls."""
    batch, model = _small_batch(), _small_model()
    twin = _small_model()   # never frozen
    plain = _forward(model, batch)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    params = [id(p) for p in model.parameters()]
    assert openpcseg_amd.freeze(model) == REPORT
    after = model.state_dict()
    assert list(after.keys()) == list(before.keys()) and all(torch.equal(after[k], before[k]) for k in before)
    assert [id(p) for p in model.parameters()] == params

    calls = _count_calls(monkeypatch, cpu_be, ["bn_apply", "bn_stats", "conv_gather_gemm"])
    frozen = _forward(model, batch)
    assert calls["bn_apply"] == 0 and calls["bn_stats"] == 0
    assert calls["conv_gather_gemm"] == N_CONVS
    assert torch.equal(frozen["logit_coords"], plain["logit_coords"]) and "loss" not in frozen
    for key in ("logits", "point_logits"):
        scale = float(plain[key].abs().max())
        err = float((frozen[key] - plain[key]).abs().max())
        print("cylinder freeze cpu %s: err %.3e of max %.3e" % (key, err, scale))
        assert err <= 2e-5 * scale, (key, err, scale)

    # the unfrozen forward makes the same 48 convolution calls and 41 bn_apply launches more
    calls.update({k: 0 for k in calls})
    assert openpcseg_amd.unfreeze(model) > 0
    again = _forward(model, batch)
    assert calls["conv_gather_gemm"] == N_CONVS and calls["bn_apply"] == 41
    assert torch.equal(again["logits"], _forward(twin, batch)["logits"]) and torch.equal(again["logits"], plain["logits"])


def test_grad_mode_and_train_mode_take_the_unfrozen_path(cpu_be, monkeypatch):
    batch, model = _small_batch(), _small_model()
    plain = _forward(model, batch)["logits"]
    openpcseg_amd.freeze(model)
    calls = _count_calls(monkeypatch, cpu_be, ["bn_apply"])
    out = model(dict(batch))["logits"]          # grad mode on: BatchNorm layers and all, bit for bit
    assert calls["bn_apply"] == 41 and torch.equal(out.detach(), plain)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()                               # no unfreeze needed: batch statistics
    out = model(dict(batch))
    assert "loss" in out and all(int(m.num_batches_tracked) == 1 for m in model.modules() if hasattr(m, "num_batches_tracked"))
    model.load_state_dict(sd)
    model.eval()
    assert float((_forward(model, batch)["logits"] - plain).abs().max()) <= 2e-5 * float(plain.abs().max())


def test_refold_after_a_change_of_the_running_statistics(cpu_be):
    batch, model, twin = _small_batch(), _small_model(), _small_model()
    openpcseg_amd.freeze(model)
    a = _forward(model, batch)["logits"]
    folds = lambda: sum(f.folds for f in _records(model))
    rec = model.upBlock3.__dict__["_pcs_folds"]["conv3"]
    assert rec.bn is model.upBlock3.bn3
    n_all, n_rec = folds(), rec.folds
    _forward(model, batch)
    assert folds() == n_all   # nothing changed: nothing folded
    for m in (model, twin):
        m.upBlock3.bn3.running_var.mul_(4)
    a2, b2 = _forward(model, batch)["logits"], _forward(twin, batch)["logits"]
    assert rec.folds == n_rec + 1 and folds() == n_all + 1
    assert float((a2 - a).abs().max()) > 100 * 2e-5 * float(a.abs().max())   # the output moved, far beyond the bound it is matched to
    assert float((a2 - b2).abs().max()) <= 2e-5 * float(b2.abs().max())
    # load_state_dict writes every tensor in place: every record folds again (36 + 4 + 4)
    sd = {k: (v * 1.25 if k.endswith("kernel") else v) for k, v in twin.state_dict().items()}
    model.load_state_dict(sd)
    twin.load_state_dict(sd)
    a3, b3 = _forward(model, batch)["logits"], _forward(twin, batch)["logits"]
    assert folds() == n_all + 1 + 44
    assert float((a3 - b3).abs().max()) <= 2e-5 * float(b3.abs().max())
    assert openpcseg_amd.unfreeze(model) > 0
    assert torch.equal(_forward(model, batch)["logits"], b3)


def test_frozen_model_on_a_backend_without_the_mode(monkeypatch):
    """The oracle backend has no `conv_epilogue_post_affine`: the kernel adds the bias, torch does leaky_relu_, mul_, add_, add_
    -- still no BatchNorm launch, the same 48 convolution calls."""
    from oracle.adapter import OracleBackend
    batch, model = _small_batch(), _small_model()
    monkeypatch.setattr(native, "_BACKEND", OracleBackend())
    be = native.backend()
    assert not getattr(be, "conv_epilogue_post_affine", False)
    plain = _forward(model, batch)["logits"]
    openpcseg_amd.freeze(model)
    calls = _count_calls(monkeypatch, be, ["bn_apply", "conv_gather_gemm"])
    frozen = _forward(model, batch)["logits"]
    assert calls["conv_gather_gemm"] == N_CONVS
    # ReconNet's three norms run in the literal gate sequence on this backend (it has no gate op): those are the `skipped` ones
    assert calls["bn_apply"] == 3
    assert float((frozen - plain).abs().max()) <= 2e-5 * float(plain.abs().max())


def test_cpu_backend_post_affine_write_back_order(cpu_be):
    """conv_gather_gemm(act_slope, post_scale, post_shift, addend) = leaky(conv + b) * s + t + r. s has negative entries, so neither
    "affine before the activation" nor "addend before the activation" passes."""
    lidar = make_batch([0], n_points=2000)["lidar"]
    coords = lidar.C.int().contiguous()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(coords.shape[0], 8, generator=g)
    entry = F.build_kernel_map(coords, coords, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    w, b = torch.randn(27, 8, 12, generator=g) * 0.1, torch.randn(12, generator=g)
    r = torch.randn(coords.shape[0], 12, generator=g)
    s = (0.5 + torch.rand(12, generator=g)) * torch.tensor([1.0, -1.0] * 6)
    t = torch.randn(12, generator=g) * 0.3
    base = cpu_be.conv_gather_gemm(x, w, entry.fwd) + b
    leaky = torch.where(base < 0, base * 0.5, base)
    want = leaky * s + t + r
    got = cpu_be.conv_gather_gemm(x, w, entry.fwd, bias=b, act_slope=0.5, post_scale=s, post_shift=t, addend=r)
    assert torch.equal(got, want)
    affine_first = base * s + t
    assert not torch.allclose(got, torch.where(affine_first < 0, affine_first * 0.5, affine_first) + r, atol=1e-3)
    addend_first = torch.where(base + r < 0, (base + r) * 0.5, base + r) * s + t
    assert not torch.allclose(got, addend_first, atol=1e-3)
    assert torch.equal(cpu_be.conv_gather_gemm(x, w, entry.fwd, bias=b, relu=True, post_scale=s, post_shift=t), torch.relu(base) * s + t)
    with pytest.raises(ValueError):
        cpu_be.conv_gather_gemm(x, w, entry.fwd, post_scale=s)
    # the same order through functional.conv3d_inference, with the backend's mode and with the torch steps behind the kernel
    xs = SparseTensor(x, coords, 1)
    xs.kmaps[((1, 1, 1), (3, 3, 3), (1, 1, 1), (1, 1, 1))] = entry
    with torch.no_grad():
        y1 = F.conv3d_inference(xs, w, b, 3, addend=r, act_slope=0.5, post_scale=s, post_shift=t).F
        assert torch.equal(y1, want)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(type(cpu_be), "conv_epilogue_post_affine", False)
            y2 = F.conv3d_inference(xs, w, b, 3, addend=r, act_slope=0.5, post_scale=s, post_shift=t).F
    assert float((y2 - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _record_parity(key, value):
    data = {}
    if os.path.exists(PARITY_JSON):
        with open(PARITY_JSON) as f:
            data = json.load(f)
    data[key] = value
    try:
        with open(PARITY_JSON, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:   # a read-only checkout: the figures are in the test's output
        pass


_SCAN = {}


def _scan():
    """The set-up of test_cylinder_workload.test_eval_and_predict, built once: a 20 000-point scan through cylinder_sample on the
    device, and the logits of the UNFROZEN model on the oracle backend with host tensors."""
    if not _SCAN:
        import fullsize as fs
        from oracle.adapter import OracleBackend
        from openpcseg_amd import cylinder as front
        pts = torch.from_numpy(make_scan(0, 20000).astype(np.float32)).cuda()
        labels = torch.from_numpy(np.random.default_rng(0).integers(0, 20, size=pts.shape[0]).astype(np.int64)).cuda()
        batch = cylinder_batch([front.cylinder_sample(pts, labels, fs.CYL_LO, fs.CYL_HI, fs.CYL_GRID, 20)])
        host = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        model = CylinderTS(num_class=20, init_size=32).eval()
        seeded_state(model)
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            mp.setattr(native, "_BACKEND", OracleBackend())
            ro = model(host)
        _SCAN.update(batch=batch, host=host, ref=ro["logits"].numpy().astype(np.float64), ref_coords=ro["logit_coords"].numpy(),
                     ref_points=ro["point_logits"].numpy().astype(np.float64))
    return _SCAN


def _device_model():
    model = CylinderTS(num_class=20, init_size=32).eval()
    seeded_state(model)
    return model.cuda()


@pytest.mark.gpu
def test_frozen_model_fp32_error_vs_oracle_backend(hip, monkeypatch):
    """ef / eu: the largest logit error of the frozen / unfrozen HIP run against the unfrozen model on the oracle backend:
    ef <= 2 eu + 2e-5 max |ref| (the bound of every other model's freeze test). No bn_apply, 48 convolution launches."""
    s = _scan()
    model = _device_model()
    err = lambda o, key="logits", ref="ref": float(np.abs(o[key].float().cpu().numpy().astype(np.float64) - s[ref]).max())
    unfrozen = _forward(model, s["batch"])
    assert np.array_equal(unfrozen["logit_coords"].cpu().numpy(), s["ref_coords"])
    assert openpcseg_amd.freeze(model) == REPORT
    be = native.backend()
    _forward(model, s["batch"])   # folds and prepares
    calls = _count_calls(monkeypatch, be, ["bn_apply", "bn_stats", "conv_gather_gemm", "conv_gather_gemm_h", "conv_gather_gemm_x3"])
    frozen = _forward(model, s["batch"])
    assert calls["bn_apply"] == 0 and calls["bn_stats"] == 0
    assert calls["conv_gather_gemm"] + calls["conv_gather_gemm_h"] == N_CONVS and calls["conv_gather_gemm_x3"] == 0
    assert np.array_equal(frozen["logit_coords"].cpu().numpy(), s["ref_coords"])
    ef, eu, scale = err(frozen), err(unfrozen), float(np.abs(s["ref"]).max())
    print("cylinder freeze fp32: frozen %.3e unfrozen %.3e of max |ref| %.3e" % (ef, eu, scale))
    _record_parity("fp32", {"frozen_max_err": ef, "unfrozen_max_err": eu, "ref_max": scale, "bound": 2.0 * eu + 2e-5 * scale})
    assert ef <= 2.0 * eu + 2e-5 * scale, (ef, eu, scale)
    pf, pu, pscale = err(frozen, "point_logits", "ref_points"), err(unfrozen, "point_logits", "ref_points"), float(np.abs(s["ref_points"]).max())
    print("cylinder freeze fp32 point logits: frozen %.3e unfrozen %.3e of max |ref| %.3e" % (pf, pu, pscale))
    assert pf <= 2.0 * pu + 2e-5 * pscale, (pf, pu, pscale)   # the same bound on the point refinement's output


@pytest.mark.gpu
def test_frozen_model_bf16_autocast(hip):
    """No bound exists for this regime: the yardstick is the unfrozen bf16 run of the same session against the same fp32 oracle
    logits. The frozen run's max / mean logit error over the RMS and its arg-max disagreement may not exceed 1.25x the unfrozen
    run's (the margin test_config4_fullsize_bf16_autocast grants for summation-order noise)."""
    s = _scan()
    ref = s["ref"]
    rms = float(np.sqrt((ref ** 2).mean()))
    model = _device_model()
    runs = {}
    for name in ("unfrozen", "frozen"):
        if name == "frozen":
            assert openpcseg_amd.freeze(model) == REPORT
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            o = model(dict(s["batch"]))
        logits = o["logits"].float().cpu().numpy().astype(np.float64)
        assert np.isfinite(logits).all() and np.array_equal(o["logit_coords"].cpu().numpy(), s["ref_coords"])
        e = np.abs(logits - ref)
        runs[name] = {"logit_rms": rms, "logit_max_err_over_rms": float(e.max() / rms), "logit_mean_err_over_rms": float(e.mean() / rms),
                      "argmax_disagreement": float((logits.argmax(1) != ref.argmax(1)).mean())}
        print("cylinder freeze bf16 %s: %s" % (name, json.dumps(runs[name])))
    _record_parity("bf16_autocast", runs)
    f, u = runs["frozen"], runs["unfrozen"]
    assert f["logit_max_err_over_rms"] <= 1.25 * u["logit_max_err_over_rms"], (f, u)
    assert f["logit_mean_err_over_rms"] <= 1.25 * u["logit_mean_err_over_rms"], (f, u)
    assert f["argmax_disagreement"] <= 1.25 * u["argmax_disagreement"], (f, u)


@pytest.mark.gpu
def test_predict_on_a_frozen_model(hip):
    """point_predict = the per-frame NumPy loop of the reference on the frozen model's own logits; the evaluator's histogram matches."""
    from test_cylinder_workload import _reference_predict
    s = _scan()
    model = _device_model()
    openpcseg_amd.freeze(model)
    batch, host = s["batch"], s["host"]
    for num_points in (None, [19000]):
        b = dict(batch)
        b["num_points"] = np.array(num_points) if num_points is not None else batch["num_points"]
        ev = SegEvaluator(20)
        out = model.predict(b, evaluator=ev)
        want = _reference_predict(out["logits"].cpu().numpy(), out["logit_coords"].cpu().numpy(), host["point_coord"].numpy(),
                                  [int(v) for v in b["num_points"]])
        assert np.array_equal(out["point_predict"].cpu().numpy(), np.concatenate(want))
        kept = int(b["num_points"][0])
        assert out["point_offset"] == [0, kept]
        hist = torch.zeros(20, 20, dtype=torch.int64)
        hist.index_put_((host["point_label"][:kept], torch.from_numpy(want[0])), torch.ones(kept, dtype=torch.int64), accumulate=True)
        assert torch.equal(ev.hist.cpu(), hist)
