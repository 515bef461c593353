"""The package's own Cylinder3D graph (openpcseg_amd/workloads/cylinder.py) against the fixtures the REFERENCE's Cylinder_TS wrote
(R:pcseg/model/segmentor/voxel/cylinder3d/cylinder_ts.py run on its own CPU backend by tests/golden/make_golden.py), without the
reference's sources: state_dict layout, the small train-mode fixture on the pure-PyTorch path, two ranks over gloo, and on the GPU
config 4 at full size (fp32 and bf16 autocast), eval mode and `predict`. Bounds are those the existing tests hold the reference's
own graph to on the same fixtures (tests/test_reference_models.py, tests/test_fullsize_parity.py). The config-4 frame is rebuilt
with the NumPy restatement of the reference's cylinder dataset transform (oracle.oracle.cylinder_partition /
voxelize_with_label) and must reproduce the six input CRCs of the fixture before anything runs."""
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

from openpcseg_amd import cpu_fallback, native  # noqa: E402
from openpcseg_amd import functional as pcsF  # noqa: E402
from openpcseg_amd.workloads.cylinder import CylinderTS, cylinder_batch  # noqa: E402
from openpcseg_amd.workloads.synthetic import make_scan  # noqa: E402
from oracle import oracle as host_oracle  # noqa: E402
from seeded import seeded_state  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ["point_feature", "point_coord", "voxel_coord", "voxel_label", "point_label", "offset"]


def host_frames(seeds, n_points, label_seed_offset=100):
    """collate_batch of the reference's cylinder dataset over synthetic scans, in NumPy: one dict of host tensors."""
    feats, pcs, vcs, vls, pls = [], [], [], [], []
    for i, seed in enumerate(seeds):
        pts = make_scan(seed, n_points).astype(np.float32)
        labels = np.random.default_rng(seed + label_seed_offset).integers(0, 20, size=pts.shape[0]).astype(np.int64)
        _, coord, feat = host_oracle.cylinder_partition(pts, fs.CYL_LO, fs.CYL_HI, fs.CYL_GRID)
        vox, vlab, _, _ = host_oracle.voxelize_with_label(coord, labels, 20)
        col = lambda a: np.concatenate([a.astype(np.int64), np.full((a.shape[0], 1), i, dtype=np.int64)], 1)
        feats.append(feat), pcs.append(col(coord)), vcs.append(col(vox)), vls.append(vlab.astype(np.int64)), pls.append(labels)
    t = lambda parts: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts)))
    return {"point_feature": t(feats), "point_coord": t(pcs), "voxel_coord": t(vcs), "voxel_label": t(vls), "point_label": t(pls),
            "offset": torch.from_numpy(np.cumsum([v.shape[0] for v in vcs]).astype(np.int32))}


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_parameter_names_are_the_references():
    g = np.load(os.path.join(GOLDEN, "config4_golden.npz"))
    model = CylinderTS()
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 151 and set(names) == set(str(n) for n in g["grad_names"])
    assert tuple(model.ReconNet.conv1.kernel.shape) == (3, 64, 64) and tuple(model.logits.kernel.shape) == (27, 128, 20)
    assert tuple(model.resBlock2.pool.kernel.shape) == (27, 64, 64) and tuple(model.PPmodel[1].weight.shape) == (64, 9)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    seeded_state(model)
    for k, v in model.state_dict().items():
        if v.dtype.is_floating_point:
            assert v.shape == before[k].shape and not torch.equal(v, before[k]), k
    twin = CylinderTS()
    twin.load_state_dict(model.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))


@pytest.mark.parametrize("switch", ["1", "0"])
def test_small_fixture_on_the_pytorch_cpu_path(monkeypatch, switch):
    """cyl_* of models_e2e_golden.npz (2 500 points, init_size 8, train mode): voxel order equal, logits and loss within the 1e-3
    tests/test_reference_models.py allows the reference's own graph; the gate runs once, at width 16, when the switch is on."""
    monkeypatch.setenv("PCS_RECON_GATE", switch)
    gold = np.load(os.path.join(GOLDEN, "models_e2e_golden.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with cpu_fallback.enabled() as be:
        calls = []
        orig = be.recon_gate
        monkeypatch.setattr(be, "recon_gate", lambda *a: (calls.append(a[1].shape[1]), orig(*a))[1])
        model = CylinderTS(num_class=20, in_dim=9, init_size=8)
        seeded_state(model)
        model.train()
        out = model({k: t(gold["cyl_" + k]) for k in KEYS})
        out["loss"].backward()
    assert calls == ([16] if switch == "1" else [])
    assert np.array_equal(out["logit_coords"].numpy(), gold["cyl_logit_coords"])     # voxel order incl. the scatter / unique path
    assert np.abs(out["logits"].detach().numpy() - gold["cyl_logits"]).max() < 1e-3
    assert abs(float(out["loss"].detach()) - float(gold["cyl_loss"])) < 1e-3
    assert out["point_logits"].shape == (2500, 20)
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
    model = CylinderTS(num_class=20, init_size=8, dist=dist_mode)
    seeded_state(model)
    return model.train()


def _ddp_frames():
    return host_frames([41, 42, 43], 1200)


def _shard(b, frames):
    """The frames of one rank out of the concatenated batch, renumbered from 0."""
    out = {}
    for ck, keys in (("point_coord", ("point_feature", "point_label")), ("voxel_coord", ("voxel_label",))):
        fid = b[ck][:, 3]
        sel = torch.zeros_like(fid, dtype=torch.bool)
        coords = b[ck].clone()
        for local, f in enumerate(frames):
            sel |= fid == f
            coords[fid == f, 3] = local
        out[ck] = coords[sel].contiguous()
        for k in keys:
            out[k] = b[k][sel].clone()
    out["offset"] = None
    return out


def _cyl_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    sys.path.insert(0, ROOT)
    cpu_fallback.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model = _ddp_model(True)
    out = model(_shard(_ddp_frames(), _RANK_FRAMES[rank]))
    out["loss"].backward()
    for p in model.parameters():    # what DistributedDataParallel does to the gradients (it refuses host modules in sync mode)
        dist.all_reduce(p.grad)
        p.grad /= world
    if rank == 0:
        q.put(({n: p.grad.numpy().copy() for n, p in model.named_parameters()},
               {n: t.numpy().copy() for n, t in model.named_buffers() if t.dtype.is_floating_point}))
    dist.barrier()
    dist.destroy_process_group()


def _rank_pairing(b, up0e):
    """The point refinement of the reference pairs a point with the output row whose NUMBER is the position of the point's voxel
    in `voxel_coord` (CylinderTS._refine_rows): a pairing that depends on the batch a frame travels in. For the one-process run
    to compute what the two ranks compute, it takes each rank's pairing, restated on the rows of the three-frame batch: position
    j in the rank's voxel_coord -> the rank's j-th smallest voxel hash (its output row j) -> that voxel's row in this run."""
    rows = torch.empty(b["point_coord"].shape[0], dtype=torch.int64)
    global_hash = pcsF.sphash(up0e.C)
    for frames in _RANK_FRAMES.values():
        sh = _shard(b, frames)
        local_hash = pcsF.sphash(sh["voxel_coord"].int())
        receives = torch.argsort(local_hash)[pcsF.sphashquery(pcsF.sphash(sh["point_coord"].int()), local_hash)]
        mv, mp_ = torch.zeros(b["voxel_coord"].shape[0], dtype=torch.bool), torch.zeros(rows.shape[0], dtype=torch.bool)
        for f in frames:
            mv |= b["voxel_coord"][:, 3] == f
            mp_ |= b["point_coord"][:, 3] == f
        rows[mp_] = pcsF.sphashquery(pcsF.sphash(b["voxel_coord"][mv][receives].int()), global_hash)
    return rows


def test_two_ranks_match_the_concatenated_batch():
    """CylinderTS(dist=True) on two gloo ranks with one and two frames: gradients averaged over the ranks = the gradients of one
    process on the three-frame batch with the per-rank losses averaged; running statistics agree. Tolerances of
    test_spvcnn_workload.test_two_ranks_match_the_concatenated_batch. The one-process run uses the ranks' point-refinement
    pairing (`_rank_pairing`); everything else, the SyncBatchNorm of `change_dim` included, is the plain model."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cyl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    grads, bufs = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    b = _ddp_frames()
    with cpu_fallback.enabled():
        ref = _ddp_model(False)
        ref._refine_rows = lambda batch, up0e, voxel_hash: _rank_pairing(b, up0e)
        out = ref(b)                    # its own loss (one batch-wide mean) is not used: the per-rank losses are formed below
        target = b["voxel_label"][pcsF.sphashquery(pcsF.sphash(out["logit_coords"]), pcsF.sphash(b["voxel_coord"].int()))]
        vf, pf = out["logit_coords"][:, 3], b["point_coord"][:, 3]
        loss = 0.0
        for r in range(2):
            mv, mp_ = torch.zeros_like(vf, dtype=torch.bool), torch.zeros_like(pf, dtype=torch.bool)
            for f in _RANK_FRAMES[r]:
                mv |= vf == f
                mp_ |= pf == f
            loss = loss + (ref.criterion(out["logits"][mv], target[mv]) + ref.loss_funs(out["point_logits"][mp_], b["point_label"][mp_])) / 2
        loss.backward()
    G = float(np.median([float(p.grad.abs().max()) for p in ref.parameters()]))
    # a Linear bias in front of a train-mode BatchNorm has a gradient that is ZERO by construction (the normalisation removes the
    # bias): rounding noise on both sides, which no relative tolerance can compare. They must stay noise, by the rule of
    # fullsize.compare (below 1e-3 G); every other parameter is held to the tolerance named above.
    dead = {"PPmodel.1.bias", "PPmodel.4.bias", "PPmodel.7.bias", "change_dim.0.bias"}
    for n, p in ref.named_parameters():
        if n in dead:
            assert float(p.grad.abs().max()) < 1e-3 * G and float(np.abs(grads[n]).max()) < 1e-3 * G, n
            continue
        scale = max(float(p.grad.abs().max()), 1e-3 * G)
        assert np.abs(grads[n] - p.grad.numpy()).max() <= 2e-3 * scale, n
    for n, t in ref.named_buffers():
        if t.dtype.is_floating_point:
            assert np.allclose(bufs[n], t.numpy(), rtol=1e-4, atol=1e-6), n


# ---- GPU: config 4 at full size, reference-free ------------------------------------------------------------------------------
_MEASURED = {}


def _record(name, m):
    _MEASURED[name] = m
    print("\n[cylinder parity] %s: %s" % (name, json.dumps(m)))
    out = os.environ.get("PCS_MEASURED_DIR", "")   # where a run keeps its measured records, if it keeps any
    if out and os.path.isdir(out):
        with open(os.path.join(out, "cylinder_parity_measured.json"), "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def config4():
    """make_scan(2) through the NumPy restatement of the reference's cylinder transform; the six CRCs of the fixture must match."""
    g = np.load(os.path.join(GOLDEN, "config4_golden.npz"))
    assert int(g["n_points"]) == -1
    batch = host_frames([fs.FRAME_SEED["config4"]], None)
    assert batch["voxel_coord"].shape[0] == 40482
    crcs = fs.input_crcs("config4", batch)
    assert len(crcs) == 6
    for k, v in crcs.items():
        assert int(v) == int(g[k]), "input %s differs from the frame the reference ran on" % k
    return g, batch


def _step(g, host_batch, amp=None):
    dev = torch.device("cuda:0")
    batch = {k: v.to(dev) for k, v in host_batch.items()}
    model = CylinderTS(num_class=20, in_dim=9, init_size=32, label_smoothing=0.0)
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
def test_config4_fullsize_fp32(hip, monkeypatch, config4, switch):
    """One training step of Cylinder_TS cy480 on the full frame of config4_golden.npz: logits, loss and the 151 gradient
    fingerprints inside BOUNDS["config4/reference"] of tests/test_fullsize_parity.py, with the gate kernel and without."""
    from test_fullsize_parity import BOUNDS, _assert_bounds
    assert BOUNDS["config4/reference"] == (1e-3, 1e-5, 3e-3, 3.6e-2, 1.8e-2, 5.5e-2)
    monkeypatch.setenv("PCS_RECON_GATE", switch)
    calls = []
    be = native.backend()
    orig = be.recon_gate
    monkeypatch.setattr(be, "recon_gate", lambda *a: (calls.append(tuple(a[1].shape)), orig(*a))[1])
    g, batch = config4
    _, _, m = _step(g, batch)
    _record("config4/workload" + ("" if switch == "1" else "/literal"), m)
    assert calls == ([(40482, 64)] if switch == "1" else [])
    _assert_bounds("config4/reference", m)


@pytest.mark.gpu
def test_config4_fullsize_bf16_autocast(hip, monkeypatch, config4):
    """Against the fp32 fixture under bf16 autocast: finite, and four quantities recorded -- logit max and mean error over the RMS,
    arg-max DISagreement, worst gradient abs-sum error. No bound exists for this regime; the yardstick is the literal run
    (PCS_RECON_GATE=0) of the same session: the fused run may not exceed 1.25x its figures (the margin is summation-order noise)."""
    g, batch = config4
    step, ref = int(g["row_step"]), g["logits_rows"]
    rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
    runs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("PCS_RECON_GATE", switch)
        logits, loss, m = _step(g, batch, amp=torch.bfloat16)
        err = np.abs(logits[::step] - ref)
        m.update({"logit_rms": rms, "logit_max_err_over_rms": float(err.max() / rms), "logit_mean_err_over_rms": float(err.mean() / rms),
                  "argmax_agreement": float((logits[::step].argmax(1) == ref.argmax(1)).mean())})
        _record("config4/workload/bf16" + ("" if switch == "1" else "/literal"), m)
        assert np.isfinite(logits).all() and np.isfinite(loss)
        runs[switch] = m
    f, l = runs["1"], runs["0"]
    assert f["logit_max_err_over_rms"] <= 1.25 * l["logit_max_err_over_rms"], (f, l)
    assert f["logit_mean_err_over_rms"] <= 1.25 * l["logit_mean_err_over_rms"], (f, l)
    assert 1.0 - f["argmax_agreement"] <= 1.25 * (1.0 - l["argmax_agreement"]), (f, l)
    assert f["grad_abssum_rel_err"] <= 1.25 * l["grad_abssum_rel_err"], (f, l)


# ---- GPU: eval mode and predict --------------------------------------------------------------------------------------------
def _reference_predict(logits, coords, point_coord, num_points):
    """cylinder_ts.py:572-586 in NumPy: per frame, the arg-max of the logits row whose coordinates equal the point's."""
    preds = []
    for idx in range(int(point_coord[:, -1].max()) + 1):
        mask_point, mask_logits = point_coord[:, -1] == idx, coords[:, -1] == idx
        out_i = logits[mask_logits].argmax(1)
        key = lambda c: (c[:, 0].astype(np.int64) * 4096 + c[:, 1]) * 4096 + c[:, 2]
        lk = key(coords[mask_logits])
        order = np.argsort(lk)
        idx_query = order[np.searchsorted(lk[order], key(point_coord[mask_point]))]
        preds.append(out_i[idx_query][:num_points[idx]])
    return preds


@pytest.mark.gpu
def test_eval_and_predict(hip, monkeypatch):
    """Eval mode (running statistics) on a 20 000-point scan built on the device by cylinder.cylinder_sample. Reference: the same
    model on the oracle backend with host tensors (no gate op there: the literal sequence). With e1 / e0 the largest logit error of
    the HIP run with the gate kernel / with PCS_RECON_GATE=0: e1 <= 2 e0 + 2e-5 max |ref| (the pattern of
    test_spvcnn_workload.test_inference_freeze_and_predict: the new path against twice the established one plus the fp32 kernel
    bound), and e0 itself within 1e-3 max |ref|. predict = the per-frame loop of cylinder_ts.py:572-586; it raises in train mode."""
    from oracle.adapter import OracleBackend
    from openpcseg_amd import cylinder as front
    from openpcseg_amd.inference import SegEvaluator
    pts = torch.from_numpy(make_scan(0, 20000).astype(np.float32)).cuda()
    labels = torch.from_numpy(np.random.default_rng(0).integers(0, 20, size=pts.shape[0]).astype(np.int64)).cuda()
    batch = cylinder_batch([front.cylinder_sample(pts, labels, fs.CYL_LO, fs.CYL_HI, fs.CYL_GRID, 20)])
    host = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    model = CylinderTS(num_class=20, init_size=32).eval()
    seeded_state(model)
    with monkeypatch.context() as mp_, torch.no_grad():
        mp_.setattr(native, "_BACKEND", OracleBackend())
        ro = model(host)
    ref, ref_coords = ro["logits"].numpy().astype(np.float64), ro["logit_coords"].numpy()
    assert "loss" not in ro
    model.cuda()
    errs = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("PCS_RECON_GATE", switch)
        with torch.no_grad():
            o = model(batch)
        assert np.array_equal(o["logit_coords"].cpu().numpy(), ref_coords) and "loss" not in o
        errs[switch] = float(np.abs(o["logits"].float().cpu().numpy().astype(np.float64) - ref).max())
    scale = float(np.abs(ref).max())
    print("cylinder eval fp32: gate %.3e literal %.3e of max |ref| %.3e" % (errs["1"], errs["0"], scale))
    assert errs["0"] <= 1e-3 * scale and errs["1"] <= 2.0 * errs["0"] + 2e-5 * scale, (errs, scale)
    for num_points in (None, [19000]):
        b = dict(batch)
        b["num_points"] = np.array(num_points) if num_points is not None else batch["num_points"]
        ev = SegEvaluator(20)
        out = model.predict(b, evaluator=ev)
        want = _reference_predict(out["logits"].cpu().numpy(), out["logit_coords"].cpu().numpy(), host["point_coord"].numpy(),
                                  [int(v) for v in b["num_points"]])
        assert np.array_equal(out["point_predict"].cpu().numpy(), np.concatenate(want))
        assert out["point_offset"] == [0, int(b["num_points"][0])]
        kept = int(b["num_points"][0])
        hist = torch.zeros(20, 20, dtype=torch.int64)
        hist.index_put_((host["point_label"][:kept], torch.from_numpy(want[0])), torch.ones(kept, dtype=torch.int64), accumulate=True)
        assert torch.equal(ev.hist.cpu(), hist)
    model.train()
    with pytest.raises(RuntimeError):
        model.predict(batch)
