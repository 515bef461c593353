"""What the scan-mixing tests share (test_scanmix_host.py, test_scanmix.py) with tests/golden/make_mix_golden.py: the fixture's
input frames, the host composition of a mixed frame (`xyzret` with the ring column) and of the recorded training batch, and the
comparison with tests/golden/mix_golden.npz."""
import hashlib
import os

import numpy as np
import torch

from openpcseg_amd import scanmix

HERE = os.path.dirname(os.path.abspath(__file__))
BATCH_KEYS = ("lidar_C", "targets_F", "targets_C", "targets_mapped_F", "targets_mapped_C", "inverse_map_F", "inverse_map_C", "num_points", "offset")


def load_gold():
    return np.load(os.path.join(HERE, "golden", "mix_golden.npz"))


def scalar(a):
    return np.asarray(a).reshape(-1)[0].item()


def digest(rng=None):
    """(sha256 of the 624 Mersenne-Twister words, index into them) of the global generator or of a RandomState."""
    st = (rng or np.random).get_state()
    return hashlib.sha256(np.ascontiguousarray(st[1], dtype=np.uint32).tobytes()).digest(), int(st[2])


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def frames_and_labels(gold):
    """The fixture's input: the two frames of tests/golden/transform_golden.npz and the recorded learned labels."""
    t = np.load(os.path.join(HERE, "golden", "transform_golden.npz"))
    return [t["frame%d" % f].astype(np.float32) for f in (0, 1)], [gold["labels_f%d" % f].astype(np.int64) for f in (0, 1)]


def omega_of(gold):
    return tuple(float(v) for v in gold["omega"])


def host_xyzret(frames, labels, index, plan_row, omega, atan, lasermix="reference"):
    """__getitem__(index) on the host: frame `index` mixed with the other one, the ring column appended -> ((m, 5) float32, labels)."""
    pts, lab = scanmix.mix_scan_host(frames[index], labels[index], frames[1 - index], labels[1 - index], plan_row, omega, atan=atan,
                                     lasermix=lasermix)
    return np.concatenate([pts, scanmix.ring_ids_host(pts, atan=atan)[:, None]], axis=1), lab


def host_train_batch(frames, labels, plan, params, omega, voxel, atan):
    """collate_batch over get_single_sample of both frames, each the other's partner, on the host -> the fixture's batch keys."""
    from transform_cases import host_batch
    mixed = [scanmix.mix_scan_host(frames[f], labels[f], frames[1 - f], labels[1 - f], plan[f], omega, atan=atan) for f in (0, 1)]
    sizes = [m[0].shape[0] for m in mixed]
    raw = {"points": torch.from_numpy(np.concatenate([m[0] for m in mixed])), "labels": torch.from_numpy(np.concatenate([m[1] for m in mixed])),
           "offsets": [0] + np.cumsum(sizes).tolist(), "num_frames": 2}
    return batch_arrays(host_batch(raw, params, 1, voxel))


def batch_arrays(out):
    """A collated batch (host_batch's, or transform.device_batch(eval_maps=True)'s) -> the fixture's keys as host arrays."""
    got = {"lidar_F": out["lidar"].F.cpu().numpy(), "num_points": np.asarray(out["num_points"]).reshape(-1)}
    for k in ("lidar", "targets", "targets_mapped", "inverse_map"):
        got[k + "_C"] = out[k].C.cpu().numpy()
        if k != "lidar":
            got[k + "_F"] = out[k].F.cpu().numpy().reshape(-1)
    scene = got["lidar_C"][:, 3]
    got["offset"] = np.cumsum(np.bincount(scene, minlength=int(scene.max()) + 1))
    return got


def assert_equals_batch(gold, batch):
    """Integers equal, the feature rows bit for bit."""
    for k in BATCH_KEYS:
        ref = gold["batch_" + k]
        ref = ref.T if k.endswith("_C") else ref
        assert batch[k].shape == ref.shape, (k, batch[k].shape, ref.shape)
        assert np.array_equal(np.asarray(batch[k]).astype(np.int64), ref.astype(np.int64)), k
    assert same_bits(batch["lidar_F"], np.ascontiguousarray(gold["batch_lidar_F"].T)), "lidar_F"


def cases(gold):
    """The recorded frames -> [(name, seed, index, xyzret (m, 5) float32, labels (m,) int64, (sha, pos) after)]."""
    out = []
    for name in ("laser", "swap", "noswap"):
        out.append((name, scalar(gold[name + "_seed"]), scalar(gold[name + "_index"]), np.ascontiguousarray(gold[name + "_xyzret"].T),
                    gold[name + "_labels"].astype(np.int64), (gold[name + "_state_after"].tobytes(), scalar(gold[name + "_pos_after"]))))
    return out
