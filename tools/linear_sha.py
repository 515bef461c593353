#!/usr/bin/env python3
"""Every site that runs a Linear over tall rows ("Linear over tall rows"), on seeded inputs: one line per site, width and
autocast setting with the SHA-256 of the output and of every gradient. Two trees that compute the same bits print the same file.

  python tools/linear_sha.py > new.txt

4101 rows (the row floor plus a ragged tail); widths on and off the 16-byte pieces; autocast off and bf16. Also runs on a tree from
before linear.py, where the same Functions live in fused.py and block_fusion.py."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = 4101
WIDTHS = ((9, 64), (32, 256), (256, 20), (8, 6), (100, 36))
PARTS = (((256, 128, 96), 20), ((256, 128, 94), 20))


def sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def main():
    import torch
    from torch import nn
    import openpcseg_amd
    from openpcseg_amd import functional as F
    from openpcseg_amd import inference
    from openpcseg_amd import modules as spnn
    from openpcseg_amd.sparse import SparseTensor
    try:
        from openpcseg_amd import linear as home
        row_linear = home.row_linear
    except ImportError:   # before linear.py: what cylinder._linear / block_fusion._dense_step did
        from openpcseg_amd import block_fusion
        from openpcseg_amd import fused as home
        row_linear = lambda x, w, b: block_fusion._PointLinear.apply(x, w, b) if w.shape[0] % 4 == 0 else None
    dev = torch.device("cuda:0")

    def rn(g, *shape):
        return (torch.randn(*shape, generator=g) * 2 + 0.5).to(dev)

    def show(site, widths, amp, y, leaves):
        """y's hash, then -- after backward of a seeded weighted sum -- the gradient of every leaf."""
        g = torch.Generator().manual_seed(7)
        hashes = [sha(y)]
        if leaves:
            (y.float() * torch.randn(y.shape, generator=g).to(dev)).sum().backward()
            hashes += ["-" if t.grad is None else sha(t.grad) for t in leaves]
        print("%-32s %-18s amp=%-5s %s" % (site, widths, amp, " ".join(hashes)))

    for amp in (None, torch.bfloat16):
        name = "off" if amp is None else "bf16"
        ctx = lambda: torch.autocast("cuda", dtype=amp, enabled=amp is not None)
        for cin, cout in WIDTHS:
            g = torch.Generator().manual_seed(cin * 1000 + cout)
            torch.manual_seed(cin * 1000 + cout)   # the modules' initial weights
            lin, own = nn.Linear(cin, cout).to(dev), home.FusedLinear(cin, cout).to(dev)
            own.load_state_dict(lin.state_dict())
            x0 = rn(g, N, cin)
            idx = torch.randint(-1, N, (5000, 8), generator=g).int().to(dev)
            wts = torch.rand(5000, 8, generator=g).to(dev)
            coords = torch.stack([torch.arange(N) % 64, torch.arange(N) // 64, torch.zeros(N), torch.zeros(N)], 1).int().to(dev)

            x = x0.clone().requires_grad_(True)
            with ctx():
                y = row_linear(x, lin.weight, lin.bias)
                y = lin(x) if y is None else y
            show("row-wise", (cin, cout), name, y, [x, lin.weight, lin.bias])
            lin.zero_grad()

            x = x0.clone().requires_grad_(True)
            with ctx():
                y = own.forward(x)
            show("FusedLinear.forward", (cin, cout), name, y, [x, own.weight, own.bias])
            own.zero_grad()

            for xin in (x0, x0.bfloat16()):   # the voxel features arrive in either dtype; autocast plays no part
                x = xin.clone().requires_grad_(True)
                with ctx():
                    y = home.devoxelized_linear(lin.weight, 0, x, idx, wts, {})
                show("devoxelized_linear %s" % str(xin.dtype)[6:], (cin, cout), name, y, [x, lin.weight])
                lin.zero_grad()
                with torch.no_grad(), ctx():
                    y = inference.FoldedLinear(own).devoxelized_part(0, xin, idx, wts, cache={})
                show("FoldedLinear.devoxelized_part %s" % str(xin.dtype)[6:], (cin, cout), name, y, [])

            for ci, co in ((cin, cout),) + (((153, 32),) if cin == 100 else ()):   # 153: the width its weight gradient zero-pads
                x = rn(g, N, ci).requires_grad_(True)
                w = (rn(g, ci, co) * 0.05).requires_grad_(True)
                with ctx():
                    y = F.conv3d(SparseTensor(x, coords), w, kernel_size=1).feats
                show("conv3d 1x1x1", (ci, co), name, y, [x, w])

        for widths, cout in PARTS:
            g = torch.Generator().manual_seed(sum(widths))
            torch.manual_seed(sum(widths))
            own = home.FusedLinear(sum(widths), cout).to(dev)
            for mixed in (False, True):   # mixed: an fp32 part in front of bf16 ones
                parts = [(rn(g, N, c).bfloat16() if mixed and i else rn(g, N, c)).requires_grad_(True) for i, c in enumerate(widths)]
                with ctx():
                    y = own.forward_parts(parts)
                show("forward_parts%s" % (" mixed" if mixed else ""), widths + (cout,), name, y, parts + [own.weight, own.bias])
                own.zero_grad()

        class Net(nn.Module):   # fuse() touches the dense layers of models that have sparse convolutions
            def __init__(self):
                super().__init__()
                self.stem = nn.Sequential(spnn.Conv3d(4, 8, 3), spnn.BatchNorm(8), spnn.ReLU(True))
                self.mlp = nn.Sequential(nn.Linear(9, 64), nn.BatchNorm1d(64), nn.ReLU(True), nn.Linear(64, 36), nn.BatchNorm1d(36), nn.ReLU(True))
                self.head = nn.Linear(36, 20)

            def forward(self, x):
                return self.head(self.mlp(x))

        torch.manual_seed(5)
        net = Net().to(dev).train()
        openpcseg_amd.fuse(net)
        x = rn(torch.Generator().manual_seed(3), N, 9).requires_grad_(True)
        with ctx():
            y = net(x)
        show("fuse(): Linear-BN-ReLU x2 + head", "9-64-36-20", name, y, [x] + [p for _, p in sorted(net.named_parameters()) if p.requires_grad])
        print("%-32s %-18s amp=%-5s %s" % ("  its running statistics", "", name, " ".join(sha(b) for _, b in sorted(net.named_buffers()))))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
