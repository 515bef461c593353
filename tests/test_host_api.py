"""Host-side logic without a GPU: the C-ABI library loads and exports what the header
declares, the reference import names resolve, containers share their caches, the conv3d
dispatcher / autograd wiring reproduces the reference's outputs when the native backend is
replaced (monkeypatch, test only) by the CPU oracle."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import openpcseg_amd
from openpcseg_amd import functional as F
from openpcseg_amd import hostdata, native
from openpcseg_amd.sparse import PointTensor, SparseTensor, cat, fapply, get_kernel_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    declared = set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(native.SIGNATURES), declared ^ set(native.SIGNATURES)
    lib = native.load_library()  # dlopen works without a GPU
    for name in declared:
        assert hasattr(lib, name), name
    # and the other way round: nothing named pcs_* leaves the library without a declaration in the header
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH if hasattr(native, "LIB_PATH") else lib._name],
                          capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pcs_[a-z0-9_]+)$", syms, re.M))
    assert exported and exported <= declared, exported - declared
    assert lib.pcs_abi_version() == native.ABI_VERSION == 12
    assert lib.pcs_hashtable_capacity(1000) == 2048
    assert lib.pcs_hashtable_bytes(2048) == 2048 * 12
    assert lib.pcs_conv_tile_rows(32, 32) in (64, 128)


def test_no_cpu_fallback():
    be = native.HipBackend()
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        be.hash(torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        F.spvoxelize(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "openpcseg_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "pcs_oracle" not in src, f
    # the measurement / analysis tools are not checkers either: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
    # worker may touch oracle/ (bench.py: inside _cpu_baseline_worker only)
    for f in sorted(os.listdir(os.path.join(ROOT, "tools"))):
        if f.endswith((".py", ".sh")):
            src = open(os.path.join(ROOT, "tools", f)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M) and "pcs_oracle" not in src, f
    bench = open(os.path.join(ROOT, "bench.py")).read()
    body = bench[bench.index("def _cpu_baseline_worker"):]
    body = body[:body.index("\ndef ", 1)]
    assert len(re.findall(r"^\s*(?:from|import)\s+oracle\b", bench, re.M)) == len(re.findall(r"^\s*(?:from|import)\s+oracle\b", body, re.M)) > 0


def test_product_sources_hold_no_retired_kernels():
    """The column-parallel "ring" kernels of round 4 (0.47-0.70x the wave kernels, profiles/round4_ring.md) are retired: no
    hook, stub header or export of them is left in the product sources, the C ABI or the built library, and their parked text
    is gone (git history keeps it). So are the variants that lost their A/B: the ds_add_f32 / fenced / interleaved commits of
    the wave kernels (profiles/round3_commit_ab.txt) and the BatchNorm backward statistics in the dgrad write-back
    (profiles/round6_bn_link_ab.txt)."""
    import subprocess
    pkg = os.path.join(ROOT, "openpcseg_amd")
    csrc = os.path.join(pkg, "csrc")
    for f in os.listdir(csrc):
        assert not f.startswith("conv_ring"), f
        assert "conv_ring" not in open(os.path.join(csrc, f)).read() and "PCS_WITH_RING" not in open(os.path.join(csrc, f)).read(), f
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(d, f)).read()
                for name in ("PCS_COMMIT_", "gs_x", "BNLink"):
                    assert name not in src, (f, name)
    hdr = open(os.path.join(ROOT, "include", "pcseg_hip.h")).read()
    assert "pcs_conv_ring_enable(" not in hdr and "pcs_conv_ring_applies(" not in hdr
    assert "bn_x" not in hdr and "pcs_bn_bwd_reduce_partials" not in hdr
    assert not os.path.exists(os.path.join(ROOT, "tools", "experimental"))
    lib = os.path.join(pkg, "lib", "libpcseg_hip.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", lib], capture_output=True, text=True).stdout
        assert "pcs_conv_ring" not in syms and "conv_ring6" not in syms
        assert "pcs_bn_bwd_reduce_partials" not in syms


def test_reference_import_names():
    openpcseg_amd.install_as_torchsparse()
    import torchsparse
    import torchsparse.nn as spnn
    import torchsparse.nn.functional as TF
    from torchsparse import PointTensor as PT, SparseTensor as ST  # noqa: F401
    from torchsparse.nn.utils import fapply as fa, get_kernel_offsets as gko  # noqa: F401
    from torchsparse.utils.collate import sparse_collate_fn  # noqa: F401
    from torchsparse.utils.quantize import sparse_quantize  # noqa: F401
    assert torchsparse.__version__ == "1.4.0"
    for n in ["sphash", "sphashquery", "spcount", "spvoxelize", "spdevoxelize", "calc_ti_weights",
              "spdownsample", "conv3d"]:
        assert callable(getattr(TF, n))
    conv = spnn.Conv3d(4, 8, kernel_size=3, stride=1)
    assert conv.kernel.shape == (27, 4, 8) and conv.bias is None
    assert spnn.Conv3d(4, 8, kernel_size=1).kernel.shape == (4, 8)
    assert torchsparse.cat is cat


def test_kernel_offsets_order():
    assert get_kernel_offsets(3)[:4].tolist() == [[-1, -1, -1], [0, -1, -1], [1, -1, -1], [-1, 0, -1]]
    assert get_kernel_offsets(2).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1],
                                              [1, 1, 0], [1, 1, 1]]
    assert get_kernel_offsets((1, 3, 3))[:4].tolist() == [[0, -1, -1], [0, 0, -1], [0, 1, -1], [0, -1, 0]]
    assert (get_kernel_offsets(3, stride=2) == 2 * get_kernel_offsets(3)).all()
    assert get_kernel_offsets(2).dtype == torch.int32


def test_cache_sharing_semantics():
    x = SparseTensor(torch.zeros(3, 2), torch.zeros(3, 4, dtype=torch.int32), 2)
    assert x.s == (2, 2, 2) and x.F is x.feats and x.C is x.coords
    y = fapply(x, torch.relu)
    z = cat([x, y])
    w = x + y
    for t in (y, z, w):
        assert t.cmaps is x.cmaps and t.kmaps is x.kmaps and t.stride == x.stride
    assert z.F.shape == (3, 4)
    p = PointTensor(torch.zeros(3, 2), torch.zeros(3, 4))
    q = p + p
    assert q.idx_query is p.idx_query and q.additional_features is p.additional_features


def test_sparse_quantize_matches_reference(golden):
    for b in range(2):
        vox, idx = hostdata.sparse_quantize(golden["quant_in_%d" % b], return_index=True)
        assert (vox == golden["quant_out_%d" % b]).all() and (idx == golden["quant_idx_%d" % b]).all()
    a = SparseTensor(np.zeros((2, 1), np.float32), np.array([[0, 0, 0], [1, 1, 1]], np.int32))
    b = SparseTensor(np.zeros((1, 1), np.float32), np.array([[2, 2, 2]], np.int32))
    out = hostdata.sparse_collate_fn([{"lidar": a, "n": 1}, {"lidar": b, "n": 2}])
    assert out["lidar"].C.tolist() == [[0, 0, 0, 0], [1, 1, 1, 0], [2, 2, 2, 1]] and out["n"] == [1, 2]


def test_sparse_quantize_host_path_properties():
    """The NumPy path is a stable sort + run flags (like the device path), not np.unique: same outputs as np.unique over the
    ravel hash -- first occurrence, ascending hash order, inverse -- on random clouds with many duplicates, anisotropic voxel
    sizes, negative coordinates, one row and no rows; ravel_hash itself against the mixed-radix definition."""
    rng = np.random.default_rng(7)
    for n, vs in [(0, 1), (1, 0.5), (7, (0.5, 0.25, 1.0)), (5000, 0.37), (5000, (2, 3, 1))]:
        pts = rng.integers(-40, 40, size=(n, 3)).astype(np.float64) * 0.21
        vox, idx, inv = hostdata.sparse_quantize(pts, vs, return_index=True, return_inverse=True)
        cells = np.floor(pts / np.array(vs if isinstance(vs, tuple) else (vs,) * 3)).astype(np.int32)
        if n == 0:
            assert vox.shape == (0, 3) and idx.shape == (0,) and inv.shape == (0,)
            continue
        rel = (cells - cells.min(0)).astype(np.uint64)
        ext = rel.max(0) + np.uint64(1)
        h = (rel[:, 0] * ext[1] + rel[:, 1]) * ext[2] + rel[:, 2]
        assert (hostdata.ravel_hash(cells) == h).all()
        _, i2, v2 = np.unique(h, return_index=True, return_inverse=True)
        assert (idx == i2).all() and (inv == v2).all() and (vox == cells[i2]).all()
        assert (vox[inv] == cells).all()
        only = hostdata.sparse_quantize(pts, vs)
        assert isinstance(only, np.ndarray) and (only == vox).all()
    mixed = hostdata.sparse_collate([SparseTensor(torch.zeros(2, 3), torch.zeros(2, 3)), SparseTensor(torch.ones(1, 3), torch.ones(1, 3))])
    assert mixed.C.dtype == torch.float32 and mixed.C[:, 3].tolist() == [0.0, 0.0, 1.0] and mixed.F.shape == (3, 3)


def test_sparse_quantize_tensor_input_goes_to_the_backend(oracle_backend):
    """torch tensor in -> tensors out through backend().quantize (HIP in the product; the oracle here)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "quantize_golden.npz"))
    vox, idx, inv = hostdata.sparse_quantize(torch.from_numpy(g["scan_in"]), float(g["scan_vs"]), return_index=True,
                                             return_inverse=True)
    assert torch.equal(vox, torch.from_numpy(g["scan_vox"])) and torch.equal(idx, torch.from_numpy(g["scan_idx"]))
    assert torch.equal(inv, torch.from_numpy(g["scan_inv"]))
    only = hostdata.sparse_quantize(torch.from_numpy(g["ints_in"]), 3)
    assert torch.equal(only, torch.from_numpy(g["ints_vox"]))


# ---- dispatcher + autograd on the oracle backend vs the reference's outputs ---------------------------
@pytest.mark.parametrize("tag,name,ks,stride,transposed", [
    ("conv_k3s1_N", "k3s1", 3, 1, False), ("conv_k2s2_N", "k2s2", 2, 2, False), ("conv_k2s2_T", "k2s2", 2, 2, True)])
def test_conv3d_dispatch_matches_reference(golden, oracle_backend, tag, name, ks, stride, transposed):
    coords = torch.from_numpy(golden["scene_coords"])
    x = torch.from_numpy(golden[tag + "_x"]).requires_grad_(True)
    w = torch.from_numpy(golden[tag + "_w"]).requires_grad_(True)
    if not transposed:
        inp = SparseTensor(x, coords, 1)
        out = F.conv3d(inp, w, ks, stride=stride)
        key = ((1, 1, 1), (ks,) * 3, (stride,) * 3, (1, 1, 1))
        entry = inp.kmaps[key]
        assert (entry[0].long().numpy() == golden["kmap_%s_nbmaps" % name]).all()
        assert (entry[1].numpy() == golden["kmap_%s_nbsizes" % name]).all()
        if stride > 1:
            assert (out.C.numpy() == golden["ds_" + name]).all() and out.s == (2, 2, 2)
    else:
        # a transposed conv reuses the map its down conv built (conv.py:184-192)
        fine = SparseTensor(torch.zeros(coords.shape[0], 8), coords, 1)
        fine.cmaps[(1, 1, 1)] = coords
        down = F.conv3d(fine, torch.zeros(8, 8, 12), ks, stride=stride)
        inp = SparseTensor(x, down.C, down.s)
        inp.cmaps, inp.kmaps = down.cmaps, down.kmaps
        out = F.conv3d(inp, w, ks, stride=stride, transposed=True)
        assert out.s == (1, 1, 1) and out.C is coords
    assert np.allclose(out.F.detach().numpy(), golden[tag + "_y"], rtol=1e-4, atol=1e-5)
    out.F.backward(torch.from_numpy(golden[tag + "_gy"]))
    assert np.allclose(x.grad.numpy(), golden[tag + "_gx"], rtol=1e-4, atol=1e-5)
    assert np.allclose(w.grad.numpy(), golden[tag + "_gw"], rtol=1e-4, atol=1e-4)
    assert out.kmaps is inp.kmaps and out.cmaps is inp.cmaps


@pytest.mark.parametrize("ks", [3, (1, 3, 3), (3, 1, 3)])
def test_submanifold_reverse_map_is_a_mirror(golden, oracle_backend, ks):
    """Submanifold conv + point-symmetric offsets: the input-sorted map comes from the forward map's slices
    (offset k <- offset K-1-k), and equals the map a second probe pass builds."""
    from openpcseg_amd import functional as F
    from openpcseg_amd.sparse import make_ntuple
    c = torch.from_numpy(golden["scene_coords"])
    entry = F.build_kernel_map(c, c, make_ntuple(ks, ndim=3), (1, 1, 1), (1, 1, 1))
    assert entry._mirror
    built = oracle_backend.build_kmap(c, c, -entry._ctx[2])
    assert torch.equal(entry.rev.pairs, built.pairs) and torch.equal(entry.rev.nbsizes, built.nbsizes)
    assert entry.rev.koff_host == built.koff_host
    # a distinct coordinate tensor or an even kernel does not qualify
    assert not F.build_kernel_map(c, c.clone(), (3, 3, 3), (1, 1, 1), (1, 1, 1))._mirror
    assert not F.build_kernel_map(c, c, (2, 2, 2), (1, 1, 1), (1, 1, 1))._mirror


def test_conv3d_channel_mismatch_raises(golden, oracle_backend):
    coords = torch.from_numpy(golden["scene_coords"])
    with pytest.raises(ValueError, match="mismatch"):
        F.conv3d(SparseTensor(torch.zeros(coords.shape[0], 5), coords, 1), torch.zeros(27, 4, 8), 3)


def test_pointwise_conv_bypasses_backend(oracle_backend):
    x = SparseTensor(torch.ones(3, 2), torch.zeros(3, 4, dtype=torch.int32))
    out = F.conv3d(x, torch.ones(2, 5), 1)
    assert out.F.shape == (3, 5) and out.C is x.C and not x.kmaps


def test_minkunet_e2e_matches_reference_logits(golden_e2e, oracle_backend):
    """Our MinkUNet workload (same state_dict layout) on the oracle backend reproduces the
    reference's MinkUNet + reference backend logits: proves the dispatcher, the map reuse by
    transposed convs, initial_voxelize and voxel_to_point follow the reference."""
    from seeded import seeded_state
    from openpcseg_amd.workloads.minkunet import MinkUNet
    torch.manual_seed(0)
    model = MinkUNet(num_class=20, cr=0.25)
    ref_keys = [k for k in golden_e2e["state_keys"].tolist()]
    assert sorted(model.state_dict().keys()) == sorted(ref_keys)
    seeded_state(model)
    model.train()
    batch = {"lidar": SparseTensor(torch.from_numpy(golden_e2e["feats"]), torch.from_numpy(golden_e2e["coords"])),
             "targets": SparseTensor(torch.from_numpy(golden_e2e["labels"]), torch.from_numpy(golden_e2e["coords"]))}
    out = model(batch)
    diff = (out["logits"].detach().numpy() - golden_e2e["logits"])
    assert np.abs(diff).max() < 1e-3, np.abs(diff).max()
    assert abs(float(out["loss"]) - float(golden_e2e["loss"])) < 1e-3
    out["loss"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


# the reference's own MinkUNet source on this API: tests/test_reference_models.py (CPU oracle and, under -m gpu, HIP)


def test_batched_lovasz_equals_the_per_class_loop():
    """workloads/losses.py: the (C', n)-batched Lovasz-softmax == the reference's per-class loop
    (R:tools/utils/common/lovasz_losses.py:176-204, classes='present'), value and gradient, with an ignored label
    and an absent class."""
    import torch
    from openpcseg_amd.workloads.losses import lovasz_softmax, lovasz_softmax_per_class
    torch.manual_seed(0)
    for n in (1, 7, 5000):
        logits = torch.randn(n, 20, requires_grad=True)
        lab = torch.randint(0, 20, (n,))
        if n > 7:
            lab[lab == 7] = 3
        p = logits.softmax(1)
        a, b = lovasz_softmax(p, lab, ignore=0), lovasz_softmax_per_class(p, lab, ignore=0)
        ga, = torch.autograd.grad(a, logits, retain_graph=True)
        gb, = torch.autograd.grad(b, logits)
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-6 and (ga - gb).abs().max() <= 1e-7
    empty = torch.zeros(4, 20).softmax(1)
    assert float(lovasz_softmax(empty, torch.zeros(4, dtype=torch.long), ignore=0)) == 0.0
    # ignore labels OUTSIDE [0, nc): the ignored points must not make a clamped class "present"
    for ign in (255, -100, -1):
        logits = torch.randn(4000, 20, requires_grad=True)
        lab = torch.randint(0, 18, (4000,))      # classes 18, 19 absent: 19 is where a clamped 255 would land, 0 for negatives
        lab[lab == 0] = 5
        lab[torch.rand(4000) < 0.1] = ign
        p = logits.softmax(1)
        a, b = lovasz_softmax(p, lab, ignore=ign), lovasz_softmax_per_class(p, torch.where(lab == ign, lab, lab), ignore=ign)
        ga, = torch.autograd.grad(a, logits, retain_graph=True)
        gb, = torch.autograd.grad(b, logits)
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-6 and (ga - gb).abs().max() <= 1e-7, (ign, float(a), float(b))


def test_cpu_baseline_worker_times_one_frame():
    """bench.py's cpu_baseline leg (the reference's compiled CPU backend under the workload model, one frame, no
    extrapolation) on a shrunken frame: the record carries value = 1 / (fwd + bwd), cores, kind and the sample text."""
    import json
    import subprocess
    import sys as _sys
    env = dict(os.environ, PCS_CPU_BASELINE_RAYS="1200", OMP_NUM_THREADS="8")
    out = subprocess.run([_sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-baseline-worker", "1"], env=env,
                         capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["kind"] in ("reference", "port") and rec["unit"] == "frames/s" and rec["cores"] in (1, 8)
    assert abs(rec["value"] - 1.0 / rec["seconds_per_frame"]) <= 0.06 * rec["value"] and "1200 rays" in rec["sample"]


def test_launch_shape_helpers_are_host_functions():
    """The per-layer launch-shape entry points run on the host (no GPU needed): tile heights of the bench shapes
    (profiles/round2_tile_sweep_*.md), which kernels read a tile order, which emit BatchNorm partials."""
    lib = native.load_library()
    pick = lib.pcs_conv_pick_tile_rows_dt
    assert pick(1158864, 5112372, 27, 96, 96, 0) == 384 and pick(1158864, 5112372, 27, 96, 96, 1) == 192
    assert pick(329421, 2752033, 27, 128, 128, 0) == 288 and pick(329421, 2752033, 27, 128, 128, 1) == 144
    # 256 -> 256 under autocast: the small stride-16 level takes the weight-stationary kernel's 4-wave tile [r6], the big stride-8
    # level stays on the tall 8-wave tile of conv_os5h
    assert pick(36068, 331722, 27, 256, 256, 0) == 288 and pick(36068, 331722, 27, 256, 256, 2) == 144
    assert pick(113008, 1001308, 27, 256, 256, 1) in (224, 288) and pick(113008, 1001308, 27, 384, 256, 1) == 144
    assert pick(36068, 331722, 27, 16, 32, 0) == 128 and pick(0, 0, 27, 96, 96, 0) == 128
    assert lib.pcs_conv_pick_tile_rows(113008, 1001308, 27, 256, 256) == pick(113008, 1001308, 27, 256, 256, 0)
    for t in (pick(n, p, 27, ci, co, d) for n, p in ((1158864, 5112372), (113008, 1001308), (3000, 9000))
              for ci, co in ((32, 32), (64, 64), (96, 96), (128, 96), (256, 256), (384, 256)) for d in (0, 1)):
        assert 16 <= t <= 512 and t % 16 == 0
    assert lib.pcs_conv_uses_tile_order(96, 96, 27, 0) == 1 and lib.pcs_conv_uses_tile_order(32, 32, 27, 0) == 1
    assert lib.pcs_conv_uses_tile_order(16, 32, 27, 0) == 0 and lib.pcs_conv_uses_tile_order(4, 32, 27, 1) == 0
    assert lib.pcs_conv_emits_bn_partials(128, 128, 27, 288, 0) == 1 and lib.pcs_conv_emits_bn_partials(96, 96, 27, 384, 0) == 1
    assert lib.pcs_conv_emits_bn_partials(5, 33, 27, 128, 0) == 0
    # BASELINE config 5 (RPVNet cr 1.75) widths are served by the wave kernels in fp32 AND in half (round 3: TAIL instances)
    for ci, co in ((56, 56), (56, 112), (112, 112), (224, 168), (168, 168), (336, 224), (224, 448), (672, 448), (448, 448)):
        assert lib.pcs_conv_uses_tile_order(ci, co, 27, 0) == 1 and lib.pcs_conv_uses_tile_order(ci, co, 27, 1) == 1, (ci, co)
        assert lib.pcs_conv_h_applies(ci, co, 27) == 1 and lib.pcs_conv_h_applies(co, ci, 8) == 1
        assert lib.pcs_conv_prepared_weights_bytes(27, ci, co) > 0
    assert lib.pcs_conv_h_applies(100, 64, 27) == 0 and lib.pcs_conv_uses_tile_order(100, 64, 27, 0) == 1  # cin % 4: fp32 only
    assert lib.pcs_conv_h_applies(51, 51, 27) == 0 and lib.pcs_conv_uses_tile_order(51, 51, 27, 0) == 0   # cr 1.6: generic kernel



def test_comm_overlap_summary_on_synthetic_trace():
    """bench.py's `comm` record: RCCL kernel time per step, the part that ran beside compute kernels, and whether the first
    all-reduce kernel started before the last backward convolution finished -- on a hand-made device trace."""
    import types
    sys.path.insert(0, ROOT)
    import bench

    def ev(name, t0, t1):
        return types.SimpleNamespace(name=name, device_type="DeviceType.CUDA", time_range=types.SimpleNamespace(start=t0, end=t1))
    events = [ev("conv_os5_kernel<4>", 0, 1000), ev("wgrad2_kernel", 1000, 1800), ev("ncclDevKernel_AllReduce_Sum_f32", 900, 1500),
              ev("conv_os5_kernel<6>", 1800, 2600), ev("ncclDevKernel_AllReduce_Sum_f32", 2500, 3100), ev("multi_tensor_apply", 3100, 3200),
              types.SimpleNamespace(name="cpu_op", device_type="DeviceType.CPU", time_range=types.SimpleNamespace(start=0, end=5000))]
    rec = bench.comm_overlap_summary(events)
    assert rec["rccl_kernels"] == 2 and abs(rec["rccl_ms_per_step"] - 1.2) < 1e-9
    assert abs(rec["overlapped_with_compute_ms"] - 0.7) < 1e-9 and abs(rec["exposed_ms"] - 0.5) < 1e-9   # 600 + 100 us beside compute
    assert rec["first_rccl_kernel_before_last_conv_ends"] is True and abs(rec["first_rccl_to_last_conv_end_ms"] - 1.7) < 1e-9
    assert bench.comm_overlap_summary([events[0]])["rccl_kernels"] == 0


def test_bench_line_fits_the_drivers_tail():
    """bench.py's compact line must stay under the 2 000 characters the driver keeps (it keeps the TAIL: a longer line loses metric /
    value). The committed line fits untouched; an over-long one is trimmed text first, secondary records next, headline keys never."""
    import copy
    import json
    sys.path.insert(0, ROOT)
    import bench
    log = os.path.join(ROOT, "profiles", "round5_bench.log")
    if not os.path.exists(log):
        pytest.skip("no committed bench line")
    raw = [l for l in open(log).read().splitlines() if l.startswith("{")][-1]
    res = json.loads(raw)
    keep = copy.deepcopy(res)
    line = bench.fit_line(res)
    assert json.loads(line) == keep and "trimmed" not in res and len(line) <= bench.LINE_LIMIT    # untouched
    big = copy.deepcopy(keep)
    big["cpu_baseline"]["sample"] = "worker failed: " + "x" * 400
    big["models"].update({"model%d" % i: [1.0, 2.0, 3.0, 4.0] for i in range(20)})
    line = bench.fit_line(big)
    out = json.loads(line)
    assert len(line) <= bench.LINE_LIMIT and out["trimmed"] is True
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "roofline"):
        assert out[k] == keep[k]
    assert out["cpu_baseline"]["value"] == keep["cpu_baseline"]["value"] and out["cpu_baseline"]["kind"] == "reference"
    assert out["amp_bf16"]["value"] == keep["amp_bf16"]["value"]          # numbers survive; labels and the long lists went first


def test_arithmetic_policies_are_opt_in():
    """The fp32 library path computes in fp32 MFMA arithmetic unless a caller selects a split policy explicitly."""
    from openpcseg_amd import functional as F
    assert F.get_conv_policy() == "fp32" and F.get_wgrad_policy() == "fp32"
    for setter in (F.set_conv_policy, F.set_wgrad_policy):
        with pytest.raises(ValueError):
            setter("tf32")
    F.set_conv_policy("bf16x3")
    F.set_wgrad_policy("bf16x3")
    try:
        assert F.get_conv_policy() == "bf16x3" and F._wgrad_split(96, 96) and not F._wgrad_split(64, 96)
    finally:
        F.set_conv_policy("fp32")
        F.set_wgrad_policy("fp32")
    lib = native.load_library()
    assert lib.pcs_conv_x3_applies(96, 96, 27) == 1 and lib.pcs_conv_x3_applies(56, 448, 27) == 1
    assert lib.pcs_conv_x3_applies(4, 32, 27) == 0 and lib.pcs_conv_x3_applies(96, 16, 27) == 0 and lib.pcs_conv_x3_applies(100, 64, 27) == 0
    assert lib.pcs_conv_x3_column_tiles(96) == 6 and lib.pcs_conv_x3_column_tiles(256) == 4 and lib.pcs_conv_x3_column_tiles(32) == 2
    assert lib.pcs_conv_prepared_weights_x3_bytes(27, 96, 96) == 3 * 27 * 6 * 3 * 1024


def test_weights_multi_plan_is_a_host_function():
    """pcs_weights_multi_plan fills the launch geometry of a job table without a device: work-block prefix sums for transposes
    (one 32 x 32 tile per block) and half re-packs (256 fragment words per block), and refuses shapes the half kernels do not serve."""
    import ctypes
    from openpcseg_amd import native
    lib = native.load_library()
    arr = (native._WeightJob * 3)()
    for j, (k, a, b, kind, tr) in zip(arr, ((27, 96, 96, 0, 0), (8, 128, 96, 1, 1), (27, 56, 112, 2, 0))):
        j.src, j.dst, j.K, j.A, j.B, j.kind, j.transpose = 4096, 8192, k, a, b, kind, tr
    blocks = lib.pcs_weights_multi_plan(ctypes.byref(arr), 3)
    t0 = 27 * 3 * 3
    assert arr[0].first_block == 0 and arr[1].first_block == t0
    # job 1: dgrad of 128 -> 96: contraction over B = 96 (3 steps), columns A = 128
    assert arr[1].ns == 3 and arr[1].nt16 * 16 >= 128 and arr[1].nctt in (2, 4, 6, 8)
    w1 = (8 * arr[1].nt16 * arr[1].ns * 64 + 255) // 256
    assert arr[2].first_block == t0 + w1 and arr[2].ns == 2   # 56 channels: two 32-channel steps, the second zero-padded
    assert blocks == arr[2].first_block + (27 * arr[2].nt16 * arr[2].ns * 64 + 255) // 256
    arr[1].A = 30   # contraction / columns the half kernels do not serve
    assert lib.pcs_weights_multi_plan(ctypes.byref(arr), 3) == -1 and b"job 1" in lib.pcs_last_error()


def test_weight_prep_cache_refreshes_all_layers_once(monkeypatch):
    """functional._WeightPrep: the prepared copies belong to one PASS over the model. The first request of a new pass (= a copy
    that was already handed out is asked for again) refreshes every registered layer's copies in ONE backend call, whatever
    happened to the weights in between -- including writes the version counter does not see (`w.data.copy_()`); within a
    pass a version bump or a new storage also refreshes; a dead parameter's copies are dropped."""
    import torch
    from openpcseg_amd import functional as F

    class FakeBackend:
        def __init__(self):
            self.calls = []

        def prepared_weights_buffer(self, weight, kind, transpose):
            return torch.zeros(1)

        def weights_multi(self, jobs):
            self.calls.append([(w.data_ptr(), kind, bool(tr)) for w, dst, kind, tr in jobs])

    monkeypatch.setattr(F._WeightPrep, "usable", staticmethod(lambda be, w: True))
    prep, be = F._WeightPrep(), FakeBackend()
    ws = [torch.nn.Parameter(torch.randn(27, 8, 8)) for _ in range(3)]
    for w in ws:                      # first pass: every layer is new -> one call each (nothing else is stale yet)
        prep.get(be, w, ("t",))
    assert [len(c) for c in be.calls] == [1, 1, 1]
    be.calls.clear()
    for w in ws:                      # second pass, weights untouched: ONE call for all three, at the first request
        prep.get(be, w, ("t",))
    assert [len(c) for c in be.calls] == [3]
    be.calls.clear()
    ws[1].data.mul_(2.0)              # behind autograd's back: same version counter, same storage
    prep.get(be, ws[2], ("t",))       # third pass starts at another layer ...
    assert len(be.calls) == 1 and len(be.calls[0]) == 3   # ... and refreshes all three, the silently rewritten one included
    prep.get(be, ws[1], ("t",))
    assert len(be.calls) == 1         # same pass: a hit
    with torch.no_grad():
        ws[0].add_(1.0)               # a versioned write in the middle of a pass (ws[0] not handed out yet in this pass)
    prep.get(be, ws[0], ("t",))
    assert len(be.calls) == 2 and be.calls[1] == [(ws[0].data_ptr(), "t", False)]
    prep.get(be, ws[1], (torch.bfloat16, True))           # a new kind for one layer: only that copy
    assert len(be.calls) == 3 and be.calls[2] == [(ws[1].data_ptr(), torch.bfloat16, True)]
    ws[2].data = torch.randn(27, 8, 8)                    # new storage for a parameter of this pass ...
    prep.invalidate()                                     # ... and the explicit switch: everything is stale
    be.calls.clear()
    prep.get(be, ws[0], ("t",))
    assert len(be.calls) == 1 and len(be.calls[0]) == 4   # three transposes + the bf16 copy
    assert (ws[2].data_ptr(), "t", False) in be.calls[0]
    del ws[0]
    import gc
    gc.collect()
    fresh = torch.nn.Parameter(torch.randn(8, 4, 4))
    prep.get(be, fresh, ("t",))       # registering a new parameter drops the dead one's copies
    assert sum(1 for v in prep.entries.values() if v[0]() is not None) == len(prep.entries) == 3


def test_step_budget_tools(tmp_path):
    """tools/stats_diff.py + tools/step_budget.py: the difference of two kernel-statistics files grouped by owner."""
    import subprocess
    import sys as _sys
    a, b, d = tmp_path / "a.csv", tmp_path / "b.csv", tmp_path / "d.csv"
    head = '"Name","Calls","TotalDurationNs","AverageNs"\n'
    a.write_text(head + '"void (anonymous namespace)::conv_os5_kernel<4>(pcs::ConvArgs)",30,30000000,1000000\n"__amd_rocclr_copyBuffer",600,2400000,4000\n')
    b.write_text(head + '"void (anonymous namespace)::conv_os5_kernel<4>(pcs::ConvArgs)",70,70000000,1000000\n"__amd_rocclr_copyBuffer",680,2720000,4000\n'
                        '"void (anonymous namespace)::bn_apply_kernel<4, F32>(void const*)",252,12600000,50000\n')
    tools = os.path.join(ROOT, "tools")
    subprocess.run([_sys.executable, os.path.join(tools, "stats_diff.py"), str(a), str(b), str(d)], check=True)
    out = subprocess.run([_sys.executable, os.path.join(tools, "step_budget.py"), str(d), "4", "t"], check=True, capture_output=True, text=True).stdout
    assert "| conv fwd / dgrad (fused gather-GEMM-scatter) | 10 | 10.00 |" in out
    assert "| copies / fills (runtime) | 20 | 0.08 |" in out and "| BatchNorm" in out and "| **total** | **93** |" in out


class _TorchRunKernels:
    """HipBackend's own sorted-run pass (sort, scan, host read, allocations, memo) with only its two kernel calls -- run heads and
    emit, csrc/quantize.hip -- restated in torch. No quantize_frame_keys: hostdata then builds the key in torch as well."""
    _sorted_runs, _voxel_emit = native.HipBackend._sorted_runs, native.HipBackend._voxel_emit
    quantize_sorted_keys, unique_inverse_csr = native.HipBackend.quantize_sorted_keys, native.HipBackend.unique_inverse_csr

    def _run_heads(self, skeys):
        flags = torch.ones(skeys.numel(), dtype=torch.int32)
        flags[1:] = (skeys[1:] != skeys[:-1]).int()
        return flags

    def _run_emit(self, entry, flags, rank, perm, src, *outs):
        assert entry in ("pcs_quantize_emit", "pcs_unique_emit") and len(outs) == 3
        if flags.numel() == 0:      # the entries return before they launch
            return
        head = flags.bool()
        if entry == "pcs_quantize_emit":
            vox, index, inverse = outs
            vox.copy_(src[perm[head]])
            if index is not None:
                index.copy_(perm[head])
        else:
            uniq, inverse, rowptr = outs
            uniq.copy_(src[head])
            rowptr[:-1] = head.nonzero()[:, 0]
            rowptr[-1] = flags.numel()
        if inverse is not None:
            inverse[perm] = rank - 1


def test_sparse_quantize_frames_host_logic(monkeypatch):
    """hostdata.sparse_quantize_frames / workloads.synthetic.device_collate: the key construction -- one
    lexicographic key with the frame on top orders every frame like its own ravel hash -- against the per-frame NumPy path
    (make_batch), through the backend's own sort / flag / scan / emit pass with its two kernel calls in torch (the HIP pass itself:
    -m gpu, test_device_input_pipeline_matches_the_host_dataloader). Equal-length, ragged and single-frame batches."""
    from openpcseg_amd.workloads import synthetic as syn

    monkeypatch.setattr(native, "_BACKEND", _TorchRunKernels())
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # the entry point refuses host tensors: no CPU path
    for seeds, npts in (([3, 4, 5], 6000), ([7], 3000)):
        d = syn.device_collate(syn.make_raw_batch(seeds, n_points=npts))
        b = syn.make_batch(seeds, n_points=npts)
        assert torch.equal(d["lidar"].C, b["lidar"].C) and torch.equal(d["lidar"].F, b["lidar"].F)
        assert torch.equal(d["targets"].F, b["targets"].F)
    raw = syn.make_raw_batch([3, 4], n_points=4000)           # ragged: the second frame keeps 2 500 of its rows
    keep = torch.cat([torch.arange(0, 4000), torch.arange(4000, 6500)])
    rag = {"points": raw["points"][keep], "frames": raw["frames"][keep], "labels": raw["labels"][keep], "num_frames": 2,
           "offsets": [0, 4000, 6500]}
    d = syn.device_collate(rag)
    from openpcseg_amd.hostdata import sparse_collate_fn
    frames = [syn.voxelize_scan(rag["points"][a:b].numpy(), seed=0) for a, b in ((0, 4000), (4000, 6500))]
    ref = sparse_collate_fn(frames)
    assert torch.equal(d["lidar"].C, ref["lidar"].C) and torch.equal(d["lidar"].F, ref["lidar"].F)


# ---- grouping rows by key ("Grouping rows by key") -------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("n", [0, 1, 2, 257])
def test_csr_torch_half_contract_on_host_tensors(n, m):
    """native._sorted_csr, the torch half of HipBackend._csr: entries sorted by row, equal rows in ascending position, keys outside
    [0, m) outside [rowptr[0], rowptr[m]), m + 1 row pointers -- against NumPy's stable argsort and bincount; int32 keys = int64 keys."""
    rng = np.random.default_rng(100 * n + m)
    keys = rng.integers(-1, m + 2, size=n)     # heavy ties; -1, m and m + 1 have no row
    valid = (keys >= 0) & (keys < m)
    got = {}
    for dtype in (torch.int32, torch.int64):
        order, rowptr = native._sorted_csr(torch.from_numpy(keys).to(dtype), m)
        assert order.dtype == torch.int64 and order.shape == (n,) and rowptr.shape == (m + 1,)
        got[dtype] = order, rowptr = order.numpy(), rowptr.numpy()
        ref = np.argsort(keys, kind="stable")
        assert np.array_equal(order[rowptr[0]:rowptr[m]], ref[valid[ref]])
        assert np.array_equal(np.diff(rowptr), np.bincount(keys[valid], minlength=m))
        assert rowptr[0] == (keys < 0).sum()
    assert all(np.array_equal(a, b) for a, b in zip(got[torch.int32], got[torch.int64]))
    be = object.__new__(native.HipBackend)      # host tensors never reach the library half
    assert all(torch.equal(a, torch.from_numpy(b)) for a, b in zip(be._csr(torch.from_numpy(keys), m), got[torch.int64]))


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_unique_inverse_csr_run_pass_and_seeded_memo(monkeypatch, n):
    """HipBackend.unique_inverse_csr with only its two kernel calls in torch == torch.unique(return_inverse, return_counts); the memo
    it leaves on `inverse` carries the epoch field and is found through the one function voxelize_fwd looks its order up with."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))   # the entry refuses host tensors
    keys = torch.from_numpy(np.random.default_rng(n).integers(-40, 40, size=n))
    uniq, inverse, counts = _TorchRunKernels().unique_inverse_csr(keys)
    ru, rinv, rc = torch.unique(keys, return_inverse=True, return_counts=True)
    assert torch.equal(uniq, ru) and torch.equal(inverse, rinv) and torch.equal(counts, rc.int())
    assert (uniq.dtype, inverse.dtype, counts.dtype) == (torch.int64, torch.int64, torch.int32)
    if n == 0:
        assert not hasattr(inverse, "_pcs_vox_csr")
        return
    m = uniq.numel()
    holder, slot, extra = native._vox_csr_memo(inverse, m, n)
    key, (perm, rowptr), epoch = getattr(holder, slot)
    assert holder is inverse and slot == "_pcs_vox_csr" and key == native._cache_key(inverse) + extra and key[-2:] == (m, n)
    assert epoch == native.CACHE_STATS["epoch"]
    order, ptr = native._sorted_csr(inverse, m)
    assert torch.equal(perm, order) and torch.equal(rowptr, ptr)
    before = dict(native.CACHE_STATS)
    native.CACHE_STATS["epoch"] += 1                       # a later step: the hit counts as one across steps
    try:
        hit = native._cached(*native._vox_csr_memo(inverse, m, n), lambda: pytest.fail("the seeded memo was not found"))
        assert hit[0] is perm and hit[1] is rowptr
        assert [native.CACHE_STATS[k] - before[k] for k in ("hit", "miss", "cross")] == [1, 0, 1]
    finally:
        native.CACHE_STATS["epoch"] = before["epoch"]


# ---- convolution routing ("Convolution routing") --------------------------------------------------------------------------------
class _RouteStub:
    """A backend of which only the routing surface exists: settable answers to the shape queries, and the three conv entries
    recording what they are handed."""

    def __init__(self, served_h=False, served_x3=False, extras=False):
        self.served_h, self.served_x3, self.extras, self.asked, self.calls = served_h, served_x3, extras, [], []

    def conv_h_applies(self, cin, cout, k):
        self.asked.append("h")
        return self.served_h

    def conv_x3_applies(self, cin, cout, k):
        self.asked.append("x3")
        return self.served_x3

    def conv_supports_addend(self, cin, cout, k, dtype=0):
        return self.extras

    def prepare_weights_h(self, w, dtype, transpose):
        return w

    def prepare_weights_x3(self, w, transpose):
        return w

    def conv_gather_gemm(self, src, weight, kmap, **kw):
        self.calls.append(("fp32", kw))
        return torch.zeros((kmap.n_dst, weight.shape[2]), dtype=src.dtype)

    def conv_gather_gemm_h(self, src, wp, k, cout, kmap, **kw):
        self.calls.append(("half", kw))
        return torch.zeros((kmap.n_dst, cout), dtype=src.dtype)

    def conv_gather_gemm_x3(self, src, wp, k, cout, kmap, bias=None, tile_rows=None, bn_sums=None, ordered=True, bn_raw=False):
        self.calls.append(("x3", {}))   # the signature of the real entry: no write-back extras
        return torch.zeros((kmap.n_dst, cout), dtype=src.dtype)


def _route_combinations():
    import itertools
    return list(itertools.product((None, torch.bfloat16), (True, False), ("fp32", "bf16x3"), (True, False), (True, False)))


def _expected_family(hd, on_device, policy, served, x3_allowed):
    if hd is not None and on_device and served:
        return "half"
    if hd is None and on_device and x3_allowed and policy == "bf16x3" and served:
        return "x3"
    return "fp32"


def test_conv_family_route_table():
    """functional._conv_family over {no half dtype, bf16} x {device, host} x {policy fp32, bf16x3} x {served, unserved} x {x3 allowed,
    not}: the rules of DESIGN.md in their order; a host operand is fp32 and asks the backend nothing, so a backend without the two
    shape queries serves it."""

    class Bare:
        pass

    seen = set()
    try:
        for hd, on_device, policy, served, x3 in _route_combinations():
            F.set_conv_policy(policy)
            be = _RouteStub(served_h=served, served_x3=served)
            fam = F._conv_family(be, hd, on_device, 8, 8, 27, x3=x3)
            assert fam == _expected_family(hd, on_device, policy, served, x3), (hd, on_device, policy, served, x3, fam)
            assert fam != "half" or on_device
            assert fam != "x3" or hd is None
            if not on_device:
                assert be.asked == [] and F._conv_family(Bare(), hd, False, 8, 8, 27, x3=x3) == "fp32"
            elif hd is not None:
                assert be.asked == ["h"]   # a half dtype in play never asks for the split kernel
            seen.add(fam)
    finally:
        F.set_conv_policy("fp32")
    assert seen == {"half", "x3", "fp32"}   # not vacuous: every family is the answer somewhere


def test_conv_act_fusable_agrees_with_the_route(monkeypatch):
    """conv_act_fusable is the route's answer: over the combinations of the route table (x3 is always allowed in conv3d; the write-back
    query answers both ways instead), it is true exactly when the routed forward hands act_slope to an entry that takes it -- the half
    entry, or the fp32 entry of a shape with write-back extras. The bf16x3 entry is never handed one: the runner refuses. Host
    operands never fuse (callers ask first). Host tensors stand in for device ones as in test_sparse_quantize_frames_host_logic."""
    from types import SimpleNamespace
    n, k, c = 12, 27, 8
    kmap = SimpleNamespace(n_dst=n, n_src=n, K=k)
    entry = SimpleNamespace(fwd=kmap, rev=kmap)
    w = torch.nn.Parameter(torch.randn(k, c, c))
    seen = set()
    try:
        for hd, on_device, policy, served, extras in _route_combinations():
            F.set_conv_policy(policy)
            be = _RouteStub(served_h=served, served_x3=served, extras=extras)
            with monkeypatch.context() as mp:
                mp.setattr(native, "_BACKEND", be)
                if on_device:
                    mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
                x = torch.randn(n, c).to(hd or torch.float32)
                fusable = F.conv_act_fusable(x, w)
                fam = _expected_family(hd, on_device, policy, served, True)
                try:
                    F._SparseConv.apply(x, w, entry, False, False, False, 0.1)
                    (name, kw), = be.calls   # one entry call per convolution
                    assert name == fam and kw.get("act_slope") == 0.1
                    taken = name == "half" or (name == "fp32" and extras)
                except AssertionError as e:
                    assert "act_slope" in str(e) and fam == "x3" and be.calls == []
                    taken = False
            assert all(name != "x3" or "act_slope" not in kw for name, kw in be.calls)
            assert fusable == (taken and on_device), (hd, on_device, policy, served, extras, fusable, taken)
            seen.add((fam, fusable))
    finally:
        F.set_conv_policy("fp32")
    assert {("half", True), ("fp32", True), ("fp32", False), ("x3", False)} <= seen


@pytest.mark.parametrize("backend", ["oracle", "torch_cpu"])
def test_conv3d_half_host_features_forward_and_backward(monkeypatch, backend):
    """conv3d on 16-bit HOST features runs forward and backward on a backend that has none of the device shape queries (the oracle
    adapter): the route sends a host operand to the fp32 entry in both directions. The values are those of the same run on the fp32
    copy of the features, rounded to bf16 where the 16-bit run rounds (output, input gradient); the weight gradient is exact."""
    from openpcseg_amd import cpu_fallback
    from oracle.adapter import OracleBackend
    be = OracleBackend() if backend == "oracle" else cpu_fallback.TorchCpuBackend()
    assert backend != "oracle" or not hasattr(be, "conv_h_applies")
    monkeypatch.setattr(native, "_BACKEND", be)
    g = torch.Generator().manual_seed(5)
    box = torch.stack(torch.meshgrid(*[torch.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)
    keep = torch.randperm(box.shape[0], generator=g)[:130].sort().values
    coords = torch.cat([box[keep], torch.zeros(130, 1, dtype=torch.long)], 1).int()
    feats = torch.randn(130, 8, generator=g).bfloat16()
    w0 = torch.randn(27, 8, 8, generator=g) * 0.2
    res = {}
    for dtype in (torch.bfloat16, torch.float32):
        x = feats.to(dtype).clone().requires_grad_(True)
        w = w0.clone().requires_grad_(True)
        y = F.conv3d(SparseTensor(x, coords), w, 3)
        y.F.float().sum().backward()
        assert y.F.dtype == dtype and x.grad.dtype == dtype and w.grad.dtype == torch.float32
        res[dtype] = (y.F.detach(), x.grad, w.grad)
    (yh, gxh, gwh), (y32, gx32, gw32) = res[torch.bfloat16], res[torch.float32]
    assert torch.equal(yh, y32.bfloat16()) and torch.equal(gxh, gx32.bfloat16()) and torch.equal(gwh, gw32)
    assert float(y32.abs().max()) > 0 and float(gx32.abs().max()) > 0 and float(gw32.abs().max()) > 0


# ---- one BatchNorm entry for every fused caller (fused.bn_rows) ----------------------------------------------------------------
# the smallest shapes at which the routes differ: c = 32 serves both merge kernels' BatchNorm mode, c = 24 the range merge's add mode
_BN_N, _BN_M = 8, 5


def _bn_case(c, n=_BN_N):
    g = torch.Generator().manual_seed(c + n)
    r = lambda *s: torch.randn(*s, generator=g)
    idx8 = torch.randint(-1, _BN_M, (n, 8), generator=g).int()
    pxpy = torch.cat([torch.zeros(n, 1), torch.rand(n, 2, generator=g) * 2 - 1], 1)
    coords = torch.cat([torch.arange(n).reshape(-1, 1).repeat(1, 3), torch.zeros(n, 1, dtype=torch.long)], 1).int()
    return {"lin": r(n, c), "vox": r(_BN_M, c), "idx8": idx8, "w8": torch.rand(n, 8, generator=g), "img": r(1, c, 4, 8), "pxpy": pxpy,
            "a3": [r(n, c), r(n, c), r(n, c)], "coords": coords}


def _bn_entries():
    """name -> (modules, call, switch variable or None): every way into the fused BatchNorm passes."""
    from openpcseg_amd import block_fusion, fused
    from openpcseg_amd.workloads import cylinder
    sp = lambda k: SparseTensor(k["lin"].clone(), k["coords"])
    own, stock = (lambda c: [fused.FusedBatchNorm(c)]), (lambda c: [torch.nn.BatchNorm1d(c)])
    return {
        "FusedBatchNorm": (own, lambda b, k: b[0](sp(k), relu=True), None),
        "bn_forward": (stock, lambda b, k: block_fusion.bn_forward(b[0], sp(k), relu=True), None),
        "_dense_bn_apply": (stock, lambda b, k: block_fusion._dense_bn_apply(b[0], k["lin"], True), None),
        "cylinder._dense_bn": (own, lambda b, k: cylinder._dense_bn(b[0], k["lin"], relu=True), None),
        "point_merge": (own, lambda b, k: fused.point_merge(b[0], k["lin"], k["vox"], k["idx8"], k["w8"]), "PCS_POINT_MERGE"),
        "range_point_merge": (own, lambda b, k: fused.range_point_merge(b[0], k["lin"], k["vox"], k["idx8"], k["w8"], k["img"], k["pxpy"]),
                              "PCS_RANGE_MERGE"),
        "recon_gate": (lambda c: [fused.FusedBatchNorm(c) for _ in range(3)], lambda b, k: fused.recon_gate(b, k["a3"], k["lin"]),
                       "PCS_RECON_GATE"),
    }


_SWITCHED = [("point_merge", 32), ("range_point_merge", 32), ("range_point_merge", 24), ("recon_gate", 32)]


@pytest.mark.parametrize("entry,c,switch", [(e, 32, None) for e in ("FusedBatchNorm", "bn_forward", "_dense_bn_apply", "cylinder._dense_bn")] +
                         [(e, c, s) for e, c in _SWITCHED for s in ("1", "0")])
def test_every_batchnorm_entry_counts_a_training_step_once(monkeypatch, entry, c, switch):
    """A training call raises num_batches_tracked by exactly one, an eval call by none; a layer somebody else counted -- for good
    (`counted_by_parent`) or for this step (`_pcs_bumped`, cleared by the call) -- is not counted again. The entries that have a
    switch: with the fused kernel (1) and through the literal sequence (0)."""
    from openpcseg_amd import cpu_fallback
    make, call, var = _bn_entries()[entry]
    assert (var is None) == (switch is None)
    if var is not None:
        monkeypatch.setenv(var, switch)
    k = _bn_case(c)
    count = lambda bns: [int(b.num_batches_tracked) for b in bns]
    rows = lambda y: (y.feats if isinstance(y, SparseTensor) else y).shape[0]
    with cpu_fallback.enabled():
        bns = [b.train() for b in make(c)]
        assert rows(call(bns, k)) == _BN_N and count(bns) == [1] * len(bns)
        for b in bns:
            b.eval()
        with torch.no_grad():
            call(bns, k)
        assert count(bns) == [1] * len(bns)
        for b in bns:
            b.train().counted_by_parent = True
        call(bns, k)
        assert count(bns) == [1] * len(bns)
        for b in bns:
            b.counted_by_parent = False
            b.__dict__["_pcs_bumped"] = True
        call(bns, k)
        assert count(bns) == [1] * len(bns) and not any(b.__dict__["_pcs_bumped"] for b in bns)
        call(bns, k)   # the mark was for one step
        assert count(bns) == [2] * len(bns)


def test_point_merge_of_an_empty_shard_counts_one_row_like_every_other_path():
    """n = 0 rows in training mode (a rank without points): point_merge takes the literal sequence, whose statistics read an
    empty shard's count as 1 -- finite running statistics, the ones FusedBatchNorm leaves on the same empty input -- and returns a
    (0, c) tensor whose backward runs."""
    from openpcseg_amd import cpu_fallback, fused
    c = 32
    k = _bn_case(c, n=0)
    with cpu_fallback.enabled():
        ref = fused.FusedBatchNorm(c).train()
        ref(SparseTensor(k["lin"].clone(), k["coords"]), relu=True)
        bn = fused.FusedBatchNorm(c).train()
        lin, vox = k["lin"].clone().requires_grad_(True), k["vox"].clone().requires_grad_(True)
        out = fused.point_merge(bn, lin, vox, k["idx8"], k["w8"])
        assert out.shape == (0, c)
        out.sum().backward()
    assert torch.isfinite(bn.running_mean).all() and torch.isfinite(bn.running_var).all()
    assert torch.equal(bn.running_mean, ref.running_mean) and torch.equal(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == 1
    assert lin.grad.shape == (0, c) and vox.grad.shape == (_BN_M, c) and not vox.grad.any()
    assert bn.weight.grad is not None and torch.isfinite(bn.weight.grad).all() and torch.isfinite(bn.bias.grad).all()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_fused_batchnorm_has_the_dtype_rules_of_bn_forward(training):
    """A residual of another dtype is cast to the features' dtype, a cat_with of another dtype is concatenated by torch: FusedBatchNorm
    and block_fusion.bn_forward on a stock BatchNorm with the same state both give what torch's own BatchNorm1d gives on the fp32
    rows with the bf16 operand widened exactly (+ other.float(), ReLU, or cat). Tolerance: fp32 rounding of a handful of operations
    on values of a few units: 1e-5 absolute; a bf16 detour of the features would miss it by 1e-2."""
    from openpcseg_amd import block_fusion, cpu_fallback, fused
    c = 32
    k = _bn_case(c)
    other = torch.randn(_BN_N, c, generator=torch.Generator().manual_seed(7)).bfloat16()

    def seeded(bn):
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, c))
            bn.bias.copy_(torch.linspace(-0.5, 0.5, c))
            bn.running_mean.copy_(torch.linspace(-1, 1, c))
            bn.running_var.copy_(torch.linspace(0.5, 2, c))
        return bn.train(training)

    with cpu_fallback.enabled():
        for kw in ({"residual": other, "relu": True}, {"cat_with": other}, {"cat_with": SparseTensor(other, k["coords"]), "relu": True}):
            own, stock, ref = seeded(fused.FusedBatchNorm(c)), seeded(torch.nn.BatchNorm1d(c)), seeded(torch.nn.BatchNorm1d(c))
            with torch.no_grad():
                want = ref(k["lin"].clone())
            if "residual" in kw:
                want = want + other.float()
            if kw.get("relu"):
                want = torch.relu(want)
            if "cat_with" in kw:
                want = torch.cat([want, other.float()], 1)
            a = own(SparseTensor(k["lin"].clone(), k["coords"]), **kw)
            b = block_fusion.bn_forward(stock, SparseTensor(k["lin"].clone(), k["coords"]), **kw)
            for got, bn in ((a.feats, own), (b.feats, stock)):
                assert got.dtype == torch.float32 and got.shape == want.shape == (_BN_N, 2 * c if "cat_with" in kw else c)
                assert float((got.detach() - want).abs().max()) <= 1e-5, sorted(kw)
                assert torch.allclose(bn.running_mean, ref.running_mean, atol=1e-6) and torch.allclose(bn.running_var, ref.running_var, atol=1e-6)


# ---- one weight-gradient entry for every layer kind (functional._weight_grad) ---------------------------------------------------
class _WgradStub:
    """A backend of which only the two weight-gradient entries exist; they record (entry, operand dtypes, operand shapes, a_col,
    split) and return zeros."""

    def __init__(self, half_entry=True):
        self.calls = []
        if half_entry:
            self.conv_wgrad_h = lambda fa, fb, kmap, a_col: self._record("conv_wgrad_h", fa, fb, kmap, a_col, None)

    def conv_wgrad(self, fa, fb, kmap, a_col, split=False):
        return self._record("conv_wgrad", fa, fb, kmap, a_col, split)

    def _record(self, name, fa, fb, kmap, a_col, split):
        self.calls.append((name, (fa.dtype, fb.dtype), (tuple(fa.shape), tuple(fb.shape)), a_col, split))
        return torch.zeros((kmap.K, fa.shape[1], fb.shape[1]))


_WG_N = 5


def _wgrad_sites():
    """name -> run(ca, cb, dtype, hd): the backward of each of the five Functions, asked for the weight gradient alone, on
    (_WG_N, ca) rows and a (_WG_N, cb) gradient of `dtype`; hd is the half dtype the forward would have noted. -> weight gradient."""
    from types import SimpleNamespace as NS
    from openpcseg_amd import linear
    rows = lambda c, dtype: torch.ones(_WG_N, c, dtype=dtype)
    ident = lambda: {("_pcs_identity", _WG_N, "cpu"): NS(K=1)}

    def sparse(ca, cb, dtype, hd, transposed=False):
        ctx = NS(for_backwards=(rows(ca, dtype), torch.zeros(2, ca, cb), NS(fwd=NS(K=2)), transposed, hd), with_skip=False,
                 needs_input_grad=(False, True))
        return F._SparseConv.backward(ctx, rows(cb, dtype))[1]

    def pointwise(ca, cb, dtype, hd):
        ctx = NS(saved_tensors=(rows(ca, dtype), torch.zeros(ca, cb)), hd=hd, cache=ident(), needs_input_grad=(False, True, False))
        return F._PointwiseConv.backward(ctx, rows(cb, dtype))[1]

    def skinny(ca, cb, dtype, hd):
        ctx = NS(saved_tensors=(rows(ca, dtype), torch.zeros(cb, ca)), km=NS(K=1), hd=hd, needs_input_grad=(False, True, False))
        return linear._SkinnyLinear.backward(ctx, rows(cb, dtype))[1]

    def parts(ca, cb, dtype, hd):
        ctx = NS(saved_tensors=(torch.zeros(cb, ca), rows(ca, dtype)), km=NS(K=1), hd=hd, has_bias=False,
                 needs_input_grad=(True, False, False, False, False))
        return linear._SkinnyLinearParts.backward(ctx, rows(cb, dtype))[0]

    def point(ca, cb, dtype, hd):
        ctx = NS(saved_tensors=(rows(ca, dtype), torch.zeros(cb, ca)), hd=hd, has_bias=False, in_dtype=dtype,
                 needs_input_grad=(False, True, False))
        linear._POINT_MAPS.update(ident())
        try:
            return linear._PointLinear.backward(ctx, rows(cb, dtype))[1]
        finally:
            linear._POINT_MAPS.clear()

    return {"_SparseConv": sparse, "_PointwiseConv": pointwise, "_SkinnyLinear": skinny, "_SkinnyLinearParts": parts, "_PointLinear": point}


def test_weight_gradient_entry_table(monkeypatch):
    """Which backend entry each of the five weight-gradient callers takes, with which operands: the half entry if and only if the
    layer runs in a half dtype, the backend has it and both widths (after the caller's zero padding) are multiples of 4; otherwise
    both operands in fp32 to the fp32 entry. _PointwiseConv pads both widths on a device tensor of >= 32 padded input channels,
    _PointLinear always pads its input width; the result comes back at the unpadded widths. `split` reaches the backend from
    _SparseConv alone, under the bf16x3 policy from 96 x 96 channels."""
    f32, bf = torch.float32, torch.bfloat16
    sites = _wgrad_sites()
    shapes = lambda ca, cb: ((_WG_N, ca), (_WG_N, cb))

    def one(site, ca, cb, dtype, hd, be=None, **kw):
        be = be or _WgradStub()
        with monkeypatch.context() as mp:
            mp.setattr(native, "_BACKEND", be)
            gw = sites[site](ca, cb, dtype, hd, **kw)
        (call,) = be.calls   # one entry call per weight gradient
        assert gw.dtype == f32 and tuple(gw.shape) in ((ca, cb), (cb, ca), (2, ca, cb)), (site, gw.shape)
        return call

    for site in sites:
        assert one(site, 32, 32, f32, None) == ("conv_wgrad", (f32, f32), shapes(32, 32), 0, False), site
        assert one(site, 32, 32, bf, bf) == ("conv_wgrad_h", (bf, bf), shapes(32, 32), 0, None), site
        # a backend without the half entry: fp32 operands to the fp32 entry
        assert one(site, 32, 32, bf, bf, be=_WgradStub(half_entry=False)) == ("conv_wgrad", (f32, f32), shapes(32, 32), 0, False), site
    for site in ("_SparseConv", "_SkinnyLinear", "_SkinnyLinearParts"):   # a width off the half entry: fp32 entry, operands unpadded
        for ca, cb in ((6, 32), (32, 6)):
            assert one(site, ca, cb, bf, bf) == ("conv_wgrad", (f32, f32), shapes(ca, cb), 0, False), (site, ca, cb)
    assert one("_SparseConv", 32, 32, f32, None, transposed=True)[3] == 1   # a transposed conv's input rows are the map's column 1
    # _PointLinear: the input width is padded (Linear(9, 64): 9 -> 12), the output width is not -- off the half entry it is fp32
    assert one("_PointLinear", 9, 64, f32, None) == ("conv_wgrad", (f32, f32), shapes(12, 64), 0, False)
    assert one("_PointLinear", 9, 64, bf, bf) == ("conv_wgrad_h", (bf, bf), shapes(12, 64), 0, None)
    assert one("_PointLinear", 8, 6, bf, bf) == ("conv_wgrad", (f32, f32), shapes(8, 6), 0, False)
    # _PointwiseConv pads on the device only, and only layers of >= 32 (padded) input channels
    assert one("_PointwiseConv", 153, 32, f32, None) == ("conv_wgrad", (f32, f32), shapes(153, 32), 0, False)   # host rows
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        assert one("_PointwiseConv", 153, 32, f32, None) == ("conv_wgrad", (f32, f32), shapes(156, 32), 0, False)
        assert one("_PointwiseConv", 153, 32, f32, bf) == ("conv_wgrad_h", (bf, bf), shapes(156, 32), 0, None)
        assert one("_PointwiseConv", 32, 153, f32, bf) == ("conv_wgrad_h", (bf, bf), shapes(32, 156), 0, None)
        assert one("_PointwiseConv", 9, 32, f32, bf) == ("conv_wgrad", (f32, f32), shapes(9, 32), 0, False)
    F.set_wgrad_policy("bf16x3")
    try:
        assert one("_SparseConv", 96, 96, f32, None)[4] is True and one("_SparseConv", 64, 96, f32, None)[4] is False
        assert one("_SparseConv", 96, 96, bf, bf)[0] == "conv_wgrad_h"
        for site in sites:
            if site != "_SparseConv":
                assert one(site, 96, 96, f32, None)[4] is False, site
    finally:
        F.set_wgrad_policy("fp32")


# ---- Linear over tall rows: one eligibility rule, one dtype rule for every site (openpcseg_amd/linear.py) ------------------------------
_TL_ROWS = (4095, 4096, 0)
_TL_WIDTHS = ((9, 64), (32, 256), (256, 20), (8, 6), (100, 36))
_TL_PARTS = (((256, 128, 96), 20), ((256, 128, 94), 20))
_TL_KINDS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp64": torch.float64, "3d": torch.float32}
_TL_AMP = {"off": None, "bf16": torch.bfloat16}
_TL_HD = {None: "", torch.bfloat16: "b", torch.float16: "h", torch.float64: "d"}
_TL_WORKLOAD_SITES = ("cylinder._linear", "spvcnn._merge", "rpvnet._merge")


def _tl_home():
    """Where the family lives, and the one site that is a call rather than a function of its own."""
    from types import SimpleNamespace as NS
    from openpcseg_amd import linear

    def spvcnn_parts(lin, parts):   # block_fusion._spvcnn_forward's classifier line
        out = linear.parts_linear(lin.weight, lin.bias, parts)
        return lin(torch.cat(parts, dim=1)) if out is linear.NOT_SERVED else out
    return NS(point=linear._PointLinear, skinny=linear._SkinnyLinear, parts=linear._SkinnyLinearParts, FusedLinear=linear.FusedLinear,
              devoxelized_linear=linear.devoxelized_linear, spvcnn_parts=spvcnn_parts)


def _tall_linear_routes(mp, home):
    """{site: {(kind, autocast): "codes of the widths at 4095 rows / at 4096 / at 0"}}: which Function each site of DESIGN.md's table
    takes and the half dtype it is handed. P = _PointLinear, S = _SkinnyLinear, Q = _SkinnyLinearParts, R = the forward-only
    gather-GEMM of the frozen classifier, each followed by b / h for bf16 / fp16; - = the stock path; !Name = raises."""
    from types import SimpleNamespace as NS
    from openpcseg_amd import block_fusion, fused, inference
    from openpcseg_amd.workloads import cylinder, rpvnet, spvcnn
    log, marker = [], torch.zeros(1)

    def recorder(code, hd_of):
        return staticmethod(lambda *a: (log.append(code + _TL_HD[hd_of(a)]), marker)[1])

    mp.setattr(home.point, "apply", recorder("P", lambda a: F._amp_dtype(a[0])))
    mp.setattr(home.skinny, "apply", recorder("S", lambda a: a[4]))
    mp.setattr(home.parts, "apply", recorder("Q", lambda a: a[3]))
    mp.setattr(F, "_run_conv", lambda be, fam, x, w3, km, hd, *a, **kw: (log.append("R" + _TL_HD[hd]), (marker, x, False))[1])
    mp.setattr(F, "_conv_family", lambda *a, **kw: "fp32")
    mp.setattr(F, "_identity_map", lambda *a, **kw: "km")
    mp.setattr(F, "spdevoxelize", lambda v, idx, wts: v)
    mp.setattr(torch.nn.Linear, "forward", lambda self, x: (log.append("-"), marker)[1])
    mp.setattr(torch.nn.functional, "linear", lambda x, w, b=None: (log.append("-"), marker)[1])
    mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    mp.setattr(torch.Tensor, "float", lambda self: self)   # the stock path's casts: nothing is computed here
    cat = torch.cat   # the parts' fallback: torch's own shape and dtype rules on one row, the row count of the first part
    mp.setattr(torch, "cat", lambda ps, dim=0: cat([p[:1] for p in ps], dim=dim).expand(ps[0].shape[0], *[-1] * (ps[0].dim() - 1)))
    mp.setattr(native, "_BACKEND", NS(bn_apply=None, name="stub"))
    mp.setattr(block_fusion, "_dense_bn_apply", lambda bn, h, relu: h)
    for m in (spvcnn, rpvnet):
        mp.setattr(m, "point_maps", lambda x, z: (None, None))
    mp.setattr(fused, "point_merge", lambda bn, h, *a: h)
    mp.setattr(fused, "range_point_merge", lambda bn, h, *a: h)
    amp = {"dtype": None}
    mp.setattr(torch, "is_autocast_enabled", lambda *a: amp["dtype"] is not None)
    mp.setattr(torch, "get_autocast_dtype", lambda *a: amp["dtype"] or torch.float32)

    mods = {}

    def lin_of(cls, cin, cout):
        if (cls, cin, cout) not in mods:
            m = mods[(cls, cin, cout)] = cls(cin, cout)
            m.__dict__["_pcs_orig_class"] = torch.nn.Linear   # what fuse() leaves on a re-classed stock module
        return mods[(cls, cin, cout)]

    def z_of(x):
        return NS(F=x, C=None, idx_query=None, weights=None, additional_features=None)

    stock, own = torch.nn.Linear, home.FusedLinear
    single = {
        "FusedLinear.forward": lambda x, ci, co: lin_of(own, ci, co).forward(x),
        "devoxelized_linear": lambda x, ci, co: home.devoxelized_linear(lin_of(stock, ci, co).weight, 0, x, None, None, {}),
        "FoldedLinear.devoxelized_part": lambda x, ci, co: inference.FoldedLinear(lin_of(own, ci, co)).devoxelized_part(0, x, None, None, cache={}),
        "FoldedLinear.devoxelized_part, no cache": lambda x, ci, co: inference.FoldedLinear(lin_of(own, ci, co)).devoxelized_part(0, x, None, None),
        "block_fusion._dense_step": lambda x, ci, co: block_fusion._dense_step(lin_of(stock, ci, co), torch.nn.Identity(), None, x),
        "block_fusion._dense_linear_forward": lambda x, ci, co: block_fusion._dense_linear_forward(lin_of(stock, ci, co), x),
        "cylinder._linear": lambda x, ci, co: cylinder._linear(lin_of(stock, ci, co), x),
        "spvcnn._merge": lambda x, ci, co: spvcnn.SPVCNN._merge(NS(point_transforms=[[lin_of(stock, ci, co), None]]), 0, NS(F=None), z_of(x)),
        "rpvnet._merge": lambda x, ci, co: rpvnet.RPVNet._merge(NS(point_transforms=[[lin_of(stock, ci, co), None]], grid_sample_mode="bilinear"),
                                                                0, NS(F=None), z_of(x), None, None),
    }
    multi = {
        "FusedLinear.forward_parts": lambda ps, ci, co: lin_of(own, ci, co).forward_parts(ps),
        "block_fusion._spvcnn_forward": lambda ps, ci, co: home.spvcnn_parts(lin_of(stock, ci, co), ps),
    }
    made = {}

    def rows(kind, n, c, dtype=None):
        key = (kind, n, c, dtype)
        if key not in made:
            made[key] = torch.zeros(1, dtype=dtype or _TL_KINDS[kind]).expand((n, 2, c) if kind == "3d" else (n, c))   # no memory behind it
        return made[key]

    def one(run, *a):
        del log[:]
        try:
            run(*a)
        except Exception as e:
            return "!" + type(e).__name__
        return "+".join(log)

    table = {}
    for name, amp_dtype in _TL_AMP.items():
        amp["dtype"] = amp_dtype
        for kind in _TL_KINDS:
            for site, run in single.items():
                table.setdefault(site, {})[(kind, name)] = " / ".join(
                    " ".join(one(run, rows(kind, n, ci), ci, co) for ci, co in _TL_WIDTHS) for n in _TL_ROWS)
        # parts: as above, and "mixed" = an fp32 part in front of bf16 ones (the first dtype that is not fp32 names the call's)
        for kind in tuple(_TL_KINDS) + ("mixed",):
            for site, run in multi.items():
                def parts(n, widths):
                    if kind == "mixed":
                        return [rows("fp32", n, c, torch.bfloat16 if i else None) for i, c in enumerate(widths)]
                    return [rows(kind, n, c) for c in widths]
                table.setdefault(site, {})[(kind, name)] = " / ".join(
                    " ".join(one(run, parts(n, ws), sum(ws), co) for ws, co in _TL_PARTS) for n in _TL_ROWS)
    return table


def _tl_table(fp32_off, fp32_amp, bf16, fp64_off=None, fp64_amp=None, d3_off=None, d3_amp=None, every_row=False):
    """The codes at 4096 rows by (kind, autocast) -> the full table of one site: the same codes at 4095 and 0 rows (every_row: a site
    without a row floor), else the stock path there. Unnamed kinds: the stock path at every width."""
    none = " ".join("-" * len(fp32_off.split()))
    at = {("fp32", "off"): fp32_off, ("fp32", "bf16"): fp32_amp, ("bf16", "off"): bf16, ("bf16", "bf16"): bf16,
          ("fp64", "off"): fp64_off or none, ("fp64", "bf16"): fp64_amp or none, ("3d", "off"): d3_off or none, ("3d", "bf16"): d3_amp or none}
    return {k: " / ".join((v if every_row else none, v, v if every_row else none)) for k, v in at.items()}


# What the PARENT of linear.py answered (the probe above, run against that tree with the Functions at their old addresses and
# _spvcnn_forward's pasted block executed from its source), widths in _TL_WIDTHS order / parts in _TL_PARTS order.
_TL_POINT = ("P P P - P", "Pb Pb Pb - Pb", "Pb Pb Pb - Pb")
_TL_PARTS_ROUTES = {**_tl_table("Q -", "Qb -", "Qb -"), **{("mixed", a): "- - / Qb - / - -" for a in _TL_AMP},
                    **{("3d", a): " / ".join(["!RuntimeError !RuntimeError"] * 3) for a in _TL_AMP}}   # torch.cat of the fallback
_TL_PARENT = {
    "FusedLinear.forward": _tl_table("- S S - S", "- Sb Sb - Sb", "- Sb Sb - Sb"),
    "devoxelized_linear": _tl_table("- S S - S", "- S S - S", "- Sb Sb - Sb"),                        # ignores autocast
    "FoldedLinear.devoxelized_part": _tl_table("- R R - R", "- R R - R", "- Rb Rb - Rb"),             # likewise
    "FoldedLinear.devoxelized_part, no cache": _tl_table("- S S - S", "- S S - S", "- Sb Sb - Sb"),
    "block_fusion._dense_step": _tl_table(*_TL_POINT),
    "block_fusion._dense_linear_forward": _tl_table(*_TL_POINT),
    # the three workload sites tested neither dtype nor rank: fp64 rows were computed in fp32, a 3-D tensor failed in backward
    "cylinder._linear": _tl_table(*_TL_POINT, *_TL_POINT[:2], *_TL_POINT[:2]),
    "spvcnn._merge": _tl_table(*_TL_POINT, *_TL_POINT[:2], *_TL_POINT[:2], every_row=True),
    "rpvnet._merge": _tl_table(*_TL_POINT, *_TL_POINT[:2], *_TL_POINT[:2], every_row=True),
    "FusedLinear.forward_parts": _TL_PARTS_ROUTES,
    "block_fusion._spvcnn_forward": _TL_PARTS_ROUTES,
}


def test_tall_linear_route_table(monkeypatch):
    """Every site that runs a Linear over tall rows takes the Function, and hands it the half dtype, that it took on the parent of
    linear.py: rows 4095 / 4096 / 0, widths on and off the 16-byte pieces, fp32 / bf16 / fp64 rows, a 3-D tensor, autocast off / bf16,
    parts that sum to the weight's width in whole pieces and not. The ONLY answers allowed to differ from the parent's: fp64 rows
    and 3-D tensors at the three workload sites, which the shared rule now sends to the stock Linear."""
    with monkeypatch.context() as mp:
        got = _tall_linear_routes(mp, _tl_home())
    assert set(got) == set(_TL_PARENT)
    stock = _tl_table("- - - - -", "- - - - -", "- - - - -")
    for site, want in _TL_PARENT.items():
        assert set(got[site]) == set(want), site
        for key, codes in want.items():
            if site in _TL_WORKLOAD_SITES and key[0] in ("fp64", "3d"):
                assert codes != stock[key], (site, key)   # the parent did serve them
                codes = stock[key]
            assert got[site][key] == codes, (site, key, got[site][key], codes)


# ---- the convolution plan (csrc/conv_plan.h): what the entries launch from and the shape queries answer from ----------------------------
PLAN_FAMILY = ("none", "block", "wave4", "wave5", "wave5h", "wave6h", "wave5x")   # ConvFamily
PLAN_KIND = {"fp32": (0, 0), "bf16": (1, 1), "fp16": (1, 2), "x3": (2, 0)}           # entry -> (ConvKind, dtype code)
PLAN_STATS, PLAN_ORDER, PLAN_EXTRAS, PLAN_POST_AFFINE, PLAN_UNALIGNED = 1, 2, 4, 8, 16   # what the call carries


def conv_plan(lib, entry, cin, cout, k, tile_rows, flags=0):
    """pcs_debug_conv_plan as a dict: the fields of the ConvPlan a call of `entry` with these sizes and flags is launched from."""
    import ctypes
    out = (ctypes.c_int32 * 12)()
    kind, dtype = PLAN_KIND[entry]
    lib.pcs_debug_conv_plan(kind, dtype, cin, cout, k, tile_rows, flags, out)
    keys = ("family", "nctt", "ncoltiles", "threads", "tail", "R", "rs", "kc", "nt16", "ns", "lds", "answers")
    p = dict(zip(keys, out))
    p["family"] = PLAN_FAMILY[p["family"]]
    p["waves"] = p["threads"] // 64
    p["emits_stats"], p["reads_order"], p["takes_extras"] = bool(p["answers"] & 1), bool(p["answers"] & 2), bool(p["answers"] & 4)
    return p


def test_conv_plan_and_queries_agree():
    """Every shape query is the plan's own field: over dtype 0 / 1 / 2 and the x3 entry, channel widths of the configs (and some no
    wave kernel serves), K on both sides of 8 and 32, every tile height 16 .. 512 plus 0, 8 and 520, and degenerate sizes, the plan of
    pcs_debug_conv_plan and the query give the same answer. The prepared-weights sizes are K x nt16 x ns KB of the plan (x 3 planes for
    bf16x3), its column tiles cover cout, and the tile-order / extras answers do not depend on the tile height."""
    lib = native.load_library()
    widths = (4, 5, 16, 32, 48, 56, 64, 96, 100, 128, 168, 192, 256, 384, 672)
    tiles = (0, 8) + tuple(range(16, 513, 16)) + (520,)
    shapes = [(ci, co, k) for ci in widths for co in widths for k in (1, 8, 9, 27, 32, 33)] + [(0, 32, 27), (32, 0, 27), (32, 32, 0), (-4, 32, 27)]
    served = set()
    for cin, cout, k in shapes:
        for entry in ("fp32", "bf16", "fp16", "x3"):
            x3, dtype = entry == "x3", PLAN_KIND[entry][1]
            order = None if x3 else bool(lib.pcs_conv_uses_tile_order(cin, cout, k, dtype))
            extras = None if x3 else bool(lib.pcs_conv_supports_epilogue(cin, cout, k, dtype))
            for t in tiles:
                p = conv_plan(lib, entry, cin, cout, k, t, PLAN_STATS)
                emits = lib.pcs_conv_x3_emits_bn_partials(cin, cout, k, t) if x3 else lib.pcs_conv_emits_bn_partials(cin, cout, k, t, dtype)
                assert p["emits_stats"] == bool(emits), (entry, cin, cout, k, t, p)
                if x3:
                    assert p["reads_order"] == (p["family"] == "wave5x") and not p["takes_extras"]
                else:
                    assert (p["reads_order"], p["takes_extras"]) == (order, extras), (entry, cin, cout, k, t, p)
                if p["family"] == "none":
                    assert p["answers"] == 0 and (min(cin, cout, k) <= 0 or entry != "fp32")
                    continue
                served.add(p["family"])
                assert p["ncoltiles"] * 16 * p["nctt"] >= cout > (p["ncoltiles"] - 1) * 16 * p["nctt"] and p["threads"] in (128, 256, 384, 512)
                if entry == "fp32":
                    continue
                applies = lib.pcs_conv_x3_applies(cin, cout, k) if x3 else lib.pcs_conv_h_applies(cin, cout, k)
                nbytes = lib.pcs_conv_prepared_weights_x3_bytes(k, cin, cout) if x3 else lib.pcs_conv_prepared_weights_bytes(k, cin, cout)
                assert applies == 1 and nbytes == k * p["nt16"] * p["ns"] * 1024 * (3 if x3 else 1), (entry, cin, cout, k, p)
                assert p["nt16"] == p["ncoltiles"] * p["nctt"] and p["ns"] == (cin + 31) // 32
                if x3:
                    assert p["nctt"] == lib.pcs_conv_x3_column_tiles(cout)
    assert served == set(PLAN_FAMILY[1:])
    # what the call carries: statistics off 16 bytes go nowhere, and the generic kernel is what an unaligned tensor runs on
    p = conv_plan(lib, "fp32", 64, 64, 27, 128, PLAN_STATS | PLAN_UNALIGNED)
    assert (p["family"], p["emits_stats"], p["takes_extras"], p["reads_order"]) == ("block", False, False, False)


# (entry, cin, cout, K, (n_dst, n_pairs) of the 12-frame bench map the shape runs on, the picker's height there,
#  family, nctt, waves, TAIL, R, rs, kc). MinkUNet / SPVCNN / RPVNet / Cylinder3D widths; x3 serves 384 -> 256 as 64-column tiles
# (pcs_conv_x3_applies says 1: convx_nctt(256) = 4), so it is pinned with the others.
PLAN_TABLE = [
    ("fp32", 32, 32, 27, (688382, 3790760), 288, "wave5", 2, 4, 0, 2, 0, 0),
    ("bf16", 32, 32, 27, (688382, 3790760), 144, "wave5h", 2, 4, 0, 2, 0, 0),
    ("x3", 32, 32, 27, (688382, 3790760), 288, "wave5x", 2, 4, 0, 2, 0, 0),
    ("fp32", 64, 64, 27, (329421, 2752033), 224, "wave5", 4, 4, 0, 2, 0, 0),
    ("bf16", 64, 64, 27, (329421, 2752033), 144, "wave6h", 4, 4, 0, 1, 2, 1),
    ("x3", 64, 64, 27, (329421, 2752033), 224, "wave5x", 4, 4, 0, 4, 0, 0),
    ("fp32", 96, 96, 27, (1158864, 5112372), 384, "wave5", 6, 8, 0, 2, 0, 0),
    ("bf16", 96, 96, 27, (1158864, 5112372), 192, "wave6h", 6, 4, 0, 1, 2, 1),
    ("x3", 96, 96, 27, (1158864, 5112372), 384, "wave5x", 6, 8, 0, 3, 0, 0),
    ("fp32", 128, 96, 27, (1158864, 5112372), 384, "wave5", 6, 8, 0, 2, 0, 0),
    ("bf16", 128, 96, 27, (1158864, 5112372), 192, "wave6h", 6, 4, 0, 1, 1, 1),
    ("x3", 128, 96, 27, (1158864, 5112372), 384, "wave5x", 6, 8, 0, 3, 0, 0),
    ("fp32", 128, 128, 27, (113008, 1001308), 224, "wave5", 4, 4, 0, 2, 0, 0),
    ("bf16", 128, 128, 27, (113008, 1001308), 112, "wave6h", 8, 4, 0, 1, 1, 1),
    ("x3", 128, 128, 27, (113008, 1001308), 224, "wave5x", 4, 4, 0, 4, 0, 0),
    ("fp32", 256, 256, 27, (36068, 331722), 288, "wave5", 4, 4, 0, 2, 0, 0),
    ("bf16", 256, 256, 27, (36068, 331722), 144, "wave6h", 8, 4, 0, 1, 1, 2),
    ("x3", 256, 256, 27, (36068, 331722), 288, "wave5x", 4, 4, 0, 4, 0, 0),
    ("fp32", 384, 256, 27, (113008, 1001308), 256, "wave5", 4, 4, 0, 2, 0, 0),
    ("bf16", 384, 256, 27, (113008, 1001308), 144, "wave6h", 8, 4, 0, 1, 1, 3),
    ("x3", 384, 256, 27, (113008, 1001308), 256, "wave5x", 4, 4, 0, 4, 0, 0),
    ("fp32", 16, 32, 27, (688382, 3790760), 128, "wave4", 2, 4, 1, 1, 0, 0),
    ("fp32", 5, 33, 27, (688382, 3790760), 128, "block", 4, 4, 1, 1, 0, 0),
    ("fp32", 96, 96, 8, (329421, 688382), 192, "wave5", 6, 4, 0, 2, 0, 0),
    ("bf16", 96, 96, 8, (329421, 688382), 192, "wave6h", 6, 4, 0, 1, 2, 1),
    ("x3", 96, 96, 8, (329421, 688382), 192, "wave5x", 6, 4, 0, 3, 0, 0),
    ("fp32", 64, 64, 8, (113008, 329421), 224, "wave5", 4, 4, 0, 2, 0, 0),
    ("bf16", 64, 64, 8, (113008, 329421), 112, "wave5h", 4, 4, 0, 2, 0, 0),
    ("x3", 64, 64, 8, (113008, 329421), 224, "wave5x", 4, 4, 0, 4, 0, 0),
]


def test_conv_plan_of_the_workload_shapes_is_pinned():
    """The plan of the shapes the five workloads run, at the tile height the picker gives on the bench maps (a 256-CU device, which
    is also what the picker assumes without one): kernel family, 16-column tiles per column tile, waves, TAIL instance, row blocks
    per group, and the weight-stationary kernel's row blocks per sub-group and contraction chunks. Values written down from the
    launchers of the parent of the plan (profiles/conv_plan_refactor.md has the kernel names of a traced run next to them)."""
    lib = native.load_library()
    for entry, cin, cout, k, (n_dst, n_pairs), tile, family, nctt, waves, tail, r, rs, kc in PLAN_TABLE:
        assert lib.pcs_conv_pick_tile_rows_dt(n_dst, n_pairs, k, cin, cout, PLAN_KIND[entry][1]) == tile, (entry, cin, cout, k)
        p = conv_plan(lib, entry, cin, cout, k, tile)
        assert (p["family"], p["nctt"], p["waves"], p["tail"], p["R"], p["rs"], p["kc"]) == (family, nctt, waves, tail, r, rs, kc), \
            (entry, cin, cout, k, tile, p)
