#!/usr/bin/env python3
"""Every fused-convolution entry over the dense-map shapes of tests/test_dense_parity.py (FWD_CASES + TAIL_CASES), with and without a
tile order, BatchNorm partials and an addend: one line per launch with the SHA-256 of the output and of the raw partial sums.

  python tools/conv_entry_sha.py > new.txt                    (PCS_LIB_PATH / PCS_CONVH_WS select library and policy)
  rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python tools/conv_entry_sha.py > new.txt

Two builds that launch the same kernels on the same data print the same file; under `rocprofv3 --kernel-trace` the trace lists
the kernel names, grids, workgroup and LDS sizes of the same launches in the same order (tools/conv_entry_sha.py --trace-diff
a_kernel_trace.csv b_kernel_trace.csv compares two of them)."""
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# stride, cin, cout, forced tile height (None = the picker's): tests/test_dense_parity.py
CASES = [(4, 128, 128, None), (4, 128, 128, 112), (4, 128, 128, 256), (4, 128, 128, 288), (4, 192, 128, None), (4, 192, 128, 128),
         (4, 256, 128, 224), (8, 256, 256, None), (8, 256, 256, 128), (8, 256, 256, 224), (8, 256, 256, 288), (8, 384, 256, None),
         (8, 384, 256, 256), (2, 64, 64, None), (2, 128, 64, 256), (2, 64, 64, 192), (4, 64, 32, 224), (4, 128, 128, 176),
         (8, 128, 256, 192), (1, 96, 96, 384), (1, 128, 96, None), (1, 96, 96, 128), (1, 96, 128, None),
         (1, 56, 56, None), (2, 56, 112, None), (2, 112, 112, None), (1, 168, 168, None), (1, 224, 168, 256), (4, 336, 224, None),
         (8, 224, 448, None), (8, 672, 448, None), (8, 448, 448, 224), (2, 48, 48, None), (4, 100, 64, None), (4, 36, 24, 128),
         (8, 44, 200, None)]


def sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def trace_diff(a, b):
    cols = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z",
            "LDS_Block_Size", "Scratch_Size")
    rows = []
    for p in (a, b):
        with open(p) as f:
            r = sorted(csv.DictReader(f), key=lambda x: int(x.get("Dispatch_Id") or x["Start_Timestamp"]))
        rows.append([tuple(x.get(c, "") for c in cols) for x in r])
    n = sum(1 for x, y in zip(*rows) if x != y) + abs(len(rows[0]) - len(rows[1]))
    conv = sum(1 for x in rows[0] if "conv_os" in x[0])
    print("%d / %d launches (%d of conv kernels), %d differ in name, grid, workgroup, LDS or scratch size" % (len(rows[0]), len(rows[1]), conv, n))
    return 1 if n else 0


def main():
    import torch
    from openpcseg_amd import functional as F
    from openpcseg_amd import native
    from openpcseg_amd.workloads.synthetic import make_batch
    be = native.backend()
    dev = torch.device("cuda:0")
    levels = {1: make_batch([0, 1])["lidar"].C.to(dev)}
    for s in (1, 2, 4):
        levels[2 * s] = F.spdownsample(levels[s], 2, 2, s)
    maps = {s: F.build_kernel_map(c, c, (3, 3, 3), (s,) * 3, (1, 1, 1)).fwd for s, c in levels.items()}
    for stride, cin, cout, tile in CASES:
        kmap = maps[stride]
        g = torch.Generator(device="cpu").manual_seed(stride * 100000 + cin * 100 + cout)
        x = torch.randn(kmap.n_src, cin, generator=g).to(dev)
        w = (torch.randn(27, cin, cout, generator=g) / (cin * 27) ** 0.5).to(dev)
        add = torch.randn(kmap.n_dst, cout, generator=g).to(dev)
        entries = [("fp32", lambda **kw: be.conv_gather_gemm(x, w, kmap, **kw), add, True)]
        for dt, name in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            if be.conv_h_applies(cin, cout, 27):
                xh, wp = x.to(dt), be.prepare_weights_h(w, dt, transpose=False)
                entries.append((name, lambda xh=xh, wp=wp, **kw: be.conv_gather_gemm_h(xh, wp, 27, cout, kmap, **kw), add.to(dt), True))
        if be.conv_x3_applies(cin, cout, 27):
            wp3 = be.prepare_weights_x3(w, transpose=False)
            entries.append(("x3", lambda wp3=wp3, **kw: be.conv_gather_gemm_x3(x, wp3, 27, cout, kmap, **kw), None, False))
        for name, run, addend, extras in entries:
            for ordered in (False, "force"):
                got = []
                y = run(tile_rows=tile, ordered=ordered, bn_sums=got, bn_raw=True)
                line = ["s%d %dx%d tile %s %s %s" % (stride, cin, cout, tile, name, "ordered" if ordered else "rows"), sha(y),
                        sha(got[0]) if got else "-", sha(run(tile_rows=tile, ordered=ordered))]
                if extras:
                    line.append(sha(run(tile_rows=tile, ordered=ordered, addend=addend)))
                print(" ".join(line))
    torch.cuda.synchronize()


if __name__ == "__main__":
    sys.exit(trace_diff(sys.argv[2], sys.argv[3]) if len(sys.argv) > 1 and sys.argv[1] == "--trace-diff" else main())
