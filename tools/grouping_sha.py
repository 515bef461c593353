#!/usr/bin/env python3
"""Every operator that groups rows by an integer key ("Grouping rows by key"), on seeded inputs with many ties: one line per
output with its SHA-256. Two trees that compute the same bits print the same file.

  python tools/grouping_sha.py > new.txt          (PCS_INDEX_CSR=0 selects the torch half of the CSR builder for int32 indices too)

Sizes: 5000 rows (a few rows per key everywhere) and 400 000 rows (one frame batch of the bench workload)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def main():
    import torch
    from openpcseg_amd import hostdata, native
    be = native.backend()
    dev = torch.device("cuda:0")

    def show(name, n, *outs):
        print("%-28s n=%-7d %s" % (name, n, " ".join("-" if o is None else sha(o) for o in outs)))

    for n in (5000, 400000):
        g = torch.Generator().manual_seed(n)
        m = n // 8

        def ri(lo, hi, *shape, dtype=torch.int64):
            return torch.randint(lo, hi, shape, generator=g).to(dtype).to(dev)

        def rn(*shape):
            return torch.randn(*shape, generator=g).to(dev)

        show("quantize float", n, *be.quantize(rn(n, 3) * 4, (0.5, 0.5, 0.5), True, True))
        show("quantize int", n, *be.quantize(ri(0, 24, n, 3, dtype=torch.int32), (1.0, 1.0, 1.0), True, True))
        frames = torch.sort(ri(0, 4, n)).values
        show("sparse_quantize_frames", n, *hostdata.sparse_quantize_frames(ri(-10, 14, n, 3, dtype=torch.int32), frames, 4))
        uniq, inverse, counts = be.unique_inverse_csr(ri(0, m, n))
        show("unique_inverse_csr", n, uniq, inverse, counts)
        feats = rn(n, 16)
        show("voxelize_fwd seeded order", n, be.voxelize_fwd(feats, inverse.int(), counts, cache_on=inverse))
        idx = ri(-1, m, n, dtype=torch.int32)
        show("voxelize_fwd", n, be.voxelize_fwd(feats, idx, be.count(idx, m)))
        show("devoxelize_bwd", n, be.devoxelize_bwd(feats, ri(-1, m, n, 8, dtype=torch.int32), torch.rand(n, 8, generator=g).to(dev), m))
        # few distinct values: a row's maximum is reached by several points, the argmax is the first of them in CSR order
        show("scatter_max_fwd", n, *be.scatter_max_fwd(ri(0, 4, n, 8).float(), ri(0, m, n), m))
        b, h, w = (2, 16, 64) if n == 5000 else (4, 64, 512)
        pxpy = torch.stack([ri(0, b, n), ri(-2, w + 2, n), ri(-2, h + 2, n)], dim=1).int().contiguous()   # some points off the image
        cmap = be.map_count(pxpy, b, h, w)
        show("denselize_fwd", n, be.denselize_fwd(rn(n, 8), cmap, pxpy))
        show("denselize_bwd", n, be.denselize_bwd(rn(b, 8, h, w), cmap, pxpy))
        fxy = torch.cat([torch.sort(ri(0, b, n)).values.float()[:, None], torch.rand(n, 2, generator=g).to(dev) * 2.2 - 1.1], dim=1).contiguous()
        show("range_sample_bwd", n, be.range_sample_bwd(rn(n, 8), fxy, b, h, w))
    torch.cuda.synchronize()
    print("memo", {k: v for k, v in native.CACHE_STATS.items() if k != "epoch"})


if __name__ == "__main__":
    main()
