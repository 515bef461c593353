"""The package's own SPVCNN graph (openpcseg_amd/workloads/spvcnn.py) against the fixtures the REFERENCE's SPVCNN wrote
(R:pcseg/model/segmentor/fusion/spvcnn/spvcnn.py run on its own CPU backend by tests/golden/make_golden.py), without the reference's
sources: state_dict layout, the small train-mode fixture on the pure-PyTorch path, two ranks over gloo, and on the GPU config 3 at
full size (fp32 and bf16 autocast) and the inference mode. Bounds are those the existing tests hold the reference's own graph to on
the same fixtures (tests/test_reference_models.py, tests/test_fullsize_parity.py, tests/test_inference_fold.py)."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import fullsize as fs  # noqa: E402

import openpcseg_amd  # noqa: E402
from openpcseg_amd import cpu_fallback, native  # noqa: E402
from openpcseg_amd import functional as pcsF  # noqa: E402
from openpcseg_amd.sparse import SparseTensor  # noqa: E402
from openpcseg_amd.workloads.spvcnn import SPVCNN  # noqa: E402
from seeded import seeded_state  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_parameter_names_are_the_references():
    g = np.load(os.path.join(GOLDEN, "config3_golden.npz"))
    model = SPVCNN(num_layer=[2] * 8)
    assert set(name for name, _ in model.named_parameters()) == set(str(n) for n in g["grad_names"])
    assert [n for n, _ in model.named_parameters() if n.startswith("point_transforms.1.")] == [
        "point_transforms.1.0.weight", "point_transforms.1.0.bias", "point_transforms.1.1.weight", "point_transforms.1.1.bias"]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    seeded_state(model)
    for k, v in model.state_dict().items():
        if v.dtype.is_floating_point:
            assert v.shape == before[k].shape and not torch.equal(v, before[k]), k
    twin = SPVCNN(num_layer=[2] * 8)
    twin.load_state_dict(model.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))


@pytest.mark.parametrize("switch", ["1", "0"])
def test_small_fixture_on_the_pytorch_cpu_path(monkeypatch, switch):
    """spv_* of models_e2e_golden.npz (2 000 points, cr 0.25, mk18, train mode, dropout 0, label smoothing 0.1): logits and loss
    within the 1e-3 tests/test_reference_models.py allows the reference's own graph. Widths 64 / 32 / 24: hop 3 takes the
    literal sequence whatever the switch says."""
    monkeypatch.setenv("PCS_POINT_MERGE", switch)
    gold = np.load(os.path.join(GOLDEN, "models_e2e_golden.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with cpu_fallback.enabled() as be:
        calls = []
        orig = be.point_merge
        monkeypatch.setattr(be, "point_merge", lambda *a: (calls.append(a[3].shape[1]), orig(*a))[1])
        model = SPVCNN(num_class=20, num_layer=[2] * 8, cr=0.25, label_smoothing=0.1, dropout=0.0)
        seeded_state(model)
        model.train()
        coords = t(gold["spv_coords"])
        out = model({"lidar": SparseTensor(t(gold["spv_feats"]), coords), "targets": SparseTensor(t(gold["spv_labels"]), coords)})
        out["loss"].backward()
    assert calls == ([64, 32] if switch == "1" else [])
    assert np.abs(out["logits"].detach().numpy() - gold["spv_logits"]).max() < 1e-3
    assert abs(float(out["loss"].detach()) - float(gold["spv_loss"])) < 1e-3
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    assert all(int(m.num_batches_tracked) == 1 for m in model.modules() if hasattr(m, "num_batches_tracked"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_RANK_FRAMES = {0: [0], 1: [1, 2]}   # unequal shards, whole frames per rank


def _ddp_model(dist_mode):
    model = SPVCNN(num_class=20, num_layer=[1] * 8, cr=0.25, dist=dist_mode, label_smoothing=0.0, dropout=0.0)
    seeded_state(model)
    return model.train()


def _ddp_frames():
    from openpcseg_amd.workloads.synthetic import make_batch
    return make_batch([41, 42, 43], n_points=1200)


def _spv_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    sys.path.insert(0, ROOT)
    cpu_fallback.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    b = _ddp_frames()
    fid = b["lidar"].C[:, 3]
    sel = torch.zeros_like(fid, dtype=torch.bool)
    coords = b["lidar"].C.clone()
    for local, f in enumerate(_RANK_FRAMES[rank]):
        sel |= fid == f
        coords[fid == f, 3] = local
    coords = coords[sel].contiguous()
    model = _ddp_model(True)
    out = model({"lidar": SparseTensor(b["lidar"].F[sel].clone(), coords), "targets": SparseTensor(b["targets"].F[sel], coords)})
    out["loss"].backward()
    for p in model.parameters():    # what DistributedDataParallel does to the gradients (it refuses host modules in sync mode)
        dist.all_reduce(p.grad)
        p.grad /= world
    if rank == 0:
        q.put(({n: p.grad.numpy().copy() for n, p in model.named_parameters()},
               {n: t.numpy().copy() for n, t in model.named_buffers() if t.dtype.is_floating_point}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_match_the_concatenated_batch():
    """SPVCNN(dist=True) on two gloo ranks with one and two frames: gradients averaged over the ranks = the gradients of one process
    on the three-frame batch with the per-rank losses averaged; running statistics agree. Tolerance of
    test_distributed.test_fused_reference_minkunet_under_ddp_matches_the_concatenated_batch at world 2."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_spv_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    grads, bufs = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    b = _ddp_frames()
    with cpu_fallback.enabled():
        ref = _ddp_model(False)
        logits = ref.point_logits(SparseTensor(b["lidar"].F.clone(), b["lidar"].C))
        tgt, fid = b["targets"].F.long(), b["lidar"].C[:, 3]
        loss = 0.0
        for r in range(2):
            mine = torch.zeros_like(fid, dtype=torch.bool)
            for f in _RANK_FRAMES[r]:
                mine |= fid == f
            loss = loss + ref.criterion(logits[mine], tgt[mine]) / 2
        loss.backward()
    G = float(np.median([float(p.grad.abs().max()) for p in ref.parameters()]))
    for n, p in ref.named_parameters():
        scale = max(float(p.grad.abs().max()), 1e-3 * G)
        assert np.abs(grads[n] - p.grad.numpy()).max() <= 2e-3 * scale, n
    for n, t in ref.named_buffers():
        if t.dtype.is_floating_point:
            assert np.allclose(bufs[n], t.numpy(), rtol=1e-4, atol=1e-6), n


# ---- GPU: config 3 at full size, reference-free ------------------------------------------------------------------------------
# (logit max-abs err, loss abs err, matrix abs-sum rel, matrix sample / abs-max, any abs-sum rel, any sample / abs-max):
# tests/test_fullsize_parity.py BOUNDS["config3/reference"], at most 2x what the reference's own graph measured on these kernels
BOUNDS_CONFIG3 = (4e-4, 1e-5, 3e-4, 7e-4, 5e-4, 3e-3)
# (max err / rms, mean err / rms, gradient abs-sum rel, arg-max agreement): tests/test_fullsize_parity.py REF_AMP_BOUNDS["config3"]
REF_AMP_BOUNDS_CONFIG3 = (0.38, 0.019, 0.15, 0.975)
_MEASURED = {}


def _record(name, m):
    _MEASURED[name] = m
    print("\n[spvcnn parity] %s: %s" % (name, json.dumps(m)))
    out = os.environ.get("PCS_MEASURED_DIR", "")   # where a run keeps its measured records, if it keeps any
    if out and os.path.isdir(out):
        with open(os.path.join(out, "spvcnn_parity_measured.json"), "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def config3():
    g = np.load(os.path.join(GOLDEN, "config3_golden.npz"))
    assert int(g["n_points"]) == -1
    batch = fs.build_inputs("config3", SparseTensor)
    for k, v in fs.input_crcs("config3", batch).items():
        assert int(v) == int(g[k]), "input %s differs from the frame the reference ran on" % k
    return g, batch


def _step(g, host_batch, amp=None):
    dev = torch.device("cuda:0")
    batch = fs.to_device("config3", host_batch, dev, SparseTensor)
    model = SPVCNN(num_class=20, num_layer=fs.MODEL_CFG["config3"]["NUM_LAYER"], cr=1.0, label_smoothing=0.1, dropout=0.0)
    seeded_state(model)
    model.to(dev).train()
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
def test_config3_fullsize_fp32(hip, monkeypatch, config3, switch):
    """One training step of SPVCNN-18 on the full frame of config3_golden.npz: logits, loss and the 161 gradient fingerprints."""
    monkeypatch.setenv("PCS_POINT_MERGE", switch)
    g, batch = config3
    _, _, m = _step(g, batch)
    _record("config3/workload" + ("" if switch == "1" else "/literal"), m)
    lo, ls, gm, gms, ga, gas = BOUNDS_CONFIG3
    assert m["logit_max_abs_err"] < lo, m
    assert m["colsum_err_per_row"] < lo, m
    assert m["abssum_rel_err"] < 1e-4, m
    assert m["loss_abs_err"] < ls * max(1.0, abs(m["loss_ref"])), m
    assert m["grad_matrix_abssum_rel_err"] < gm and m["grad_matrix_sample_err_rel_max"] < gms, m
    assert m["grad_abssum_rel_err"] < ga and m["grad_sample_err_rel_max"] < gas, m
    assert m["grad_dead_max_over_G"] < 1e-3, m


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["fp32", "keep"])
def test_config3_fullsize_bf16_autocast(hip, config3, policy):
    """Against the fp32 fixture under bf16 autocast. Default point <-> voxel policy: the bounds the reference's own graph is held to.
    "keep" (16-bit point <-> voxel hops): finite, and the same four quantities recorded -- no bound exists for that regime yet."""
    g, batch = config3
    pcsF.set_pointvoxel_policy(policy)
    try:
        logits, loss, m = _step(g, batch, amp=torch.bfloat16)
    finally:
        pcsF.set_pointvoxel_policy("fp32")
    step, ref = int(g["row_step"]), g["logits_rows"]
    rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    err = np.abs(logits[::step] - ref)
    m.update({"logit_rms": rms, "logit_max_err_over_rms": float(err.max() / rms), "logit_mean_err_over_rms": float(err.mean() / rms),
              "argmax_agreement": float((logits[::step].argmax(1) == ref.argmax(1)).mean())})
    _record("config3/workload/bf16" + ("" if policy == "fp32" else "/keep"), m)
    assert np.isfinite(logits).all() and np.isfinite(loss)
    if policy == "fp32":
        bmax, bmean, bgrad, bagree = REF_AMP_BOUNDS_CONFIG3
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
    return sparse_collate_fn([{"lidar": SparseTensor(pts[inds], pc[inds]), "targets_mapped": SparseTensor(labels, pc),
                               "inverse_map": SparseTensor(np.asarray(inverse).astype(np.int64), pc),
                               "num_points": np.array([pts.shape[0]])}])


def _logits(model, feats, coords):
    with torch.no_grad():
        return model({"lidar": SparseTensor(feats.clone(), coords)})["logits"].float()


@pytest.mark.gpu
def test_inference_freeze_and_predict(hip, monkeypatch):
    """freeze folds the 49 conv + BatchNorm pairs of the mk18 trunk and leaves the three point-MLP norms running (on the merge
    kernel, with the running statistics). Frozen vs unfrozen: the bound of tests/test_inference_fold.py for MinkUNet-18, reference =
    the unfrozen model on the oracle backend with host tensors: err(frozen) <= 2 err(unfrozen) + 2e-5 max |ref|."""
    from oracle.adapter import OracleBackend
    from openpcseg_amd.inference import SegEvaluator
    from test_predict_tail import fast_hist_crop, per_class_iu, reference_tail
    model = SPVCNN(num_class=20, cr=1.0).eval()
    seeded_state(model)
    host = _eval_frame()
    hf, hc = host["lidar"].F.clone(), host["lidar"].C.int().contiguous()
    with monkeypatch.context() as mp_:
        mp_.setattr(native, "_BACKEND", OracleBackend())
        ref = _logits(model, hf, hc).numpy()
    model.cuda()
    feats, coords = hf.cuda(), hc.cuda()
    unfrozen = _logits(model, feats, coords).cpu().numpy()
    report = openpcseg_amd.freeze(model)
    assert report == {"folded": 49, "skipped": ["point_transforms.0.1", "point_transforms.1.1", "point_transforms.2.1"]}
    be = native.backend()
    calls = {"point_merge": 0, "bn_apply": 0}
    for name in calls:
        orig = getattr(be, name)
        monkeypatch.setattr(be, name, (lambda o, k: lambda *a, **kw: (calls.__setitem__(k, calls[k] + 1), o(*a, **kw))[1])(orig, name))
    frozen = _logits(model, feats, coords).cpu().numpy()
    assert calls == {"point_merge": 3, "bn_apply": 0}
    ef = float(np.abs(frozen.astype(np.float64) - ref).max())
    eu = float(np.abs(unfrozen.astype(np.float64) - ref).max())
    bound = 2.0 * eu + 2e-5 * float(np.abs(ref).max())
    print("spvcnn fp32: frozen %.3e unfrozen %.3e bound %.3e" % (ef, eu, bound))
    assert ef <= bound, (ef, eu, bound)
    batch = {k: (SparseTensor(v.F.cuda(), v.C.int().cuda()) if isinstance(v, SparseTensor) else v) for k, v in host.items()}
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
