#!/usr/bin/env python3
"""Point-cloud classification with nn.PointNet2 (Qi et al., "PointNet++"): every set-abstraction level picks its centroids by farthest
point sampling (dgll_amd.points.fps, one HIP launch per batch), groups the points within a radius of each (points.radius, first K by
index) and reduces each group with nn.PointNetConv -- all on the device, on clouds of UNEQUAL size, with no padding and no [B, M, N]
distance array.

    python examples/pointnet2/train.py --synthetic [--clouds 240 --points 256 --hidden 32,64,128 --radii 0.3,0.6 --neighbors 32
                                                    --epochs 30 --batch 24 --bf16]

--synthetic: the sampled surfaces of examples/dgcnn/train.py (six classes, clouds of points / 2 to points points, rotated at random).
The script prints the loss per epoch and at the end the accuracy on held-out clouds.  Adam; --bf16 stores the positions in bf16: the
searches and the first level run in bf16, the global_nn stages and what follows them in fp32 (mixed precision, fp32 parameters).
"""
import argparse
import importlib.util
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from dgll_amd.nn.Convolution import PointNet2  # noqa: E402

_spec = importlib.util.spec_from_file_location("dgcnn_train", os.path.join(HERE, "..", "dgcnn", "train.py"))
_dgcnn = importlib.util.module_from_spec(_spec)         # the sampled surfaces of the DGCNN example, loaded by path: both files are train.py
_spec.loader.exec_module(_dgcnn)
SURFACES, batches, make_clouds = _dgcnn.SURFACES, _dgcnn.batches, _dgcnn.make_clouds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--clouds", type=int, default=240)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--hidden", default="32,64,128")
    ap.add_argument("--radii", default="0.3,0.6")
    ap.add_argument("--neighbors", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the sampled surfaces are the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if args.bf16 else torch.float32
    clouds, labels = make_clouds(args.clouds, args.points, 0)
    held = max(len(SURFACES), args.clouds // 5)
    train_ids, test_ids = torch.arange(held, args.clouds), torch.arange(held)
    torch.manual_seed(0)
    model = PointNet2(0, len(SURFACES), hidden=tuple(int(h) for h in args.hidden.split(",")),
                      radii=tuple(float(r) for r in args.radii.split(",")), max_num_neighbors=args.neighbors, dropout=0.3).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    print("pointnet++ on %d clouds of %d to %d points, %d classes: two levels of fps (ratios 0.5, 0.25) and a ball query of %d neighbours"
          % (args.clouds, args.points // 2, args.points, len(SURFACES), args.neighbors))
    gen = torch.Generator().manual_seed(1)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0, total, seen = time.time(), 0.0, 0
        for pos, segs, y in batches(clouds, labels, args.batch, train_ids[torch.randperm(len(train_ids), generator=gen)], dev, dtype):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model((None, pos, segs)).float(), y)
            loss.backward()
            opt.step()
            total, seen = total + loss.item() * len(segs), seen + len(segs)
        torch.cuda.synchronize()
        print("epoch %3d  loss %.4f  %.1f ms" % (epoch, total / seen, (time.time() - t0) * 1e3))
    model.eval()
    hit = 0
    with torch.no_grad():
        for pos, segs, y in batches(clouds, labels, args.batch, test_ids, dev, dtype):
            hit += int((model((None, pos, segs)).argmax(1) == y).sum())
    print("held-out accuracy %.3f on %d clouds (chance %.3f)" % (hit / len(test_ids), len(test_ids), 1.0 / len(SURFACES)))


if __name__ == "__main__":
    main()
