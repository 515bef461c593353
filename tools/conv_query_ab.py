#!/usr/bin/env python3
"""Host-side A/B of the convolution shape queries of two library builds (no GPU needed).

  python tools/conv_query_ab.py dump <libpcseg_hip.so> <out.npz>     one process per library (and per environment setting)
  python tools/conv_query_ab.py compare <a.npz> <b.npz>              exit status 1 when any answer differs

Every query that says which kernel a shape runs on, over dtype 0 / 1 / 2, the channel widths of the model configs (plus a few no
kernel serves), K in {1, 2, 8, 27, 32, 33, 125}, every tile height 16 .. 512 plus 0, 8 and 520, degenerate sizes, the prepared-
weights sizes, pcs_weights_multi_plan, and the tile-height picker on the (n_dst, n_pairs) of the bench maps.
The library is opened with ctypes alone, so a build that lacks newer symbols can be asked too."""
import ctypes
import itertools
import sys

import numpy as np

WIDTHS = [4, 5, 8, 16, 20, 24, 32, 33, 36, 48, 56, 64, 96, 100, 112, 128, 160, 168, 192, 224, 256, 288, 336, 384, 448, 512, 672, 1000]
KS = [1, 2, 8, 27, 32, 33, 125]
TILES = [0, 8] + list(range(16, 513, 16)) + [520]
DEGENERATE = [(0, 32, 27), (32, 0, 27), (32, 32, 0), (-4, 32, 27), (32, -4, 27), (32, 32, -1)]
# (n_dst, n_pairs): the k3 levels of MinkUNet-34 on the 12-frame bench maps (profiles/round3_layer_table.txt), their k2 stride-2
# maps, and three small ones
MAPS = [(1158864, 5112372), (688382, 3790760), (329421, 2752033), (113008, 1001308), (36068, 331722), (688382, 1158864),
        (329421, 688382), (113008, 329421), (36068, 113008), (1500, 9000), (5000, 40000), (100, 300)]


class Job(ctypes.Structure):   # pcs_weight_job of include/pcseg_hip.h
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("K", ctypes.c_int32), ("A", ctypes.c_int32), ("B", ctypes.c_int32),
                ("kind", ctypes.c_int32), ("transpose", ctypes.c_int32), ("nctt", ctypes.c_int32), ("nt16", ctypes.c_int32),
                ("ns", ctypes.c_int32), ("first_block", ctypes.c_int64)]


def dump(path, out):
    lib = ctypes.CDLL(path)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    for name, res, args in (("pcs_conv_emits_bn_partials", i32, [i32] * 5), ("pcs_conv_x3_emits_bn_partials", i32, [i32] * 4),
                            ("pcs_conv_uses_tile_order", i32, [i32] * 4), ("pcs_conv_supports_epilogue", i32, [i32] * 4),
                            ("pcs_conv_h_applies", i32, [i32] * 3), ("pcs_conv_x3_applies", i32, [i32] * 3),
                            ("pcs_conv_x3_column_tiles", i32, [i32]), ("pcs_conv_prepared_weights_bytes", ctypes.c_size_t, [i32] * 3),
                            ("pcs_conv_prepared_weights_x3_bytes", ctypes.c_size_t, [i32] * 3),
                            ("pcs_conv_pick_tile_rows_dt", i32, [i64, i64, i32, i32, i32, i32]),
                            ("pcs_weights_multi_plan", i64, [ctypes.c_void_p, i32])):
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    shapes = list(itertools.product(WIDTHS, WIDTHS, KS)) + DEGENERATE
    res = {}
    res["emits"] = np.array([lib.pcs_conv_emits_bn_partials(ci, co, k, t, d) for ci, co, k in shapes for t in TILES for d in (0, 1, 2)])
    res["x3_emits"] = np.array([lib.pcs_conv_x3_emits_bn_partials(ci, co, k, t) for ci, co, k in shapes for t in TILES])
    for key, f in (("order", lib.pcs_conv_uses_tile_order), ("epilogue", lib.pcs_conv_supports_epilogue)):
        res[key] = np.array([f(ci, co, k, d) for ci, co, k in shapes for d in (0, 1, 2)])
    for key, f in (("h_applies", lib.pcs_conv_h_applies), ("x3_applies", lib.pcs_conv_x3_applies)):
        res[key] = np.array([f(ci, co, k) for ci, co, k in shapes])
    for key, f in (("bytes", lib.pcs_conv_prepared_weights_bytes), ("x3_bytes", lib.pcs_conv_prepared_weights_x3_bytes)):
        res[key] = np.array([f(k, ci, co) for ci, co, k in shapes], dtype=np.uint64)
    res["x3_tiles"] = np.array([lib.pcs_conv_x3_column_tiles(co) for co in [-1, 0] + WIDTHS])
    res["pick"] = np.array([lib.pcs_conv_pick_tile_rows_dt(nd, npair, k, ci, co, d) for ci, co, k in shapes for nd, npair in MAPS
                            for d in (0, 1, 2)])
    plan = []
    for ci, co, k in shapes:
        for kind, tr in ((0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
            j = Job(1, 1, k, ci, co, kind, tr, -1, -1, -1, -1)   # pointers are only checked for null
            blocks = lib.pcs_weights_multi_plan(ctypes.byref(j), 1)
            plan.append((blocks, j.nctt, j.nt16, j.ns, j.first_block))
    res["multi_plan"] = np.array(plan, dtype=np.int64)
    np.savez(out, **res)
    print("%s: %d answers" % (path, sum(v.size for v in res.values())))


def compare(a, b):
    x, y = np.load(a), np.load(b)
    bad = 0
    for key in x.files:
        n = int((x[key] != y[key]).sum())
        print("%-12s %8d inputs, %d differ" % (key, x[key].shape[0], n))
        bad += n
    print("FAILED: %d answers differ" % bad if bad else "all %d inputs answer alike" % sum(x[k].shape[0] for k in x.files))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2], sys.argv[3]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
