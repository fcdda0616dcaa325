#!/usr/bin/env python3
"""Point-cloud classification with nn.DGCNN (Wang et al., "Dynamic Graph CNN for Learning on Point Clouds"): the graph of every
EdgeConv layer is the k-nearest-neighbour graph of the layer's OWN input features, rebuilt on the device in every layer of every step
(dgll_amd.knn.knn_graph, one HIP launch per graph, nothing stored per pair of points).

    python examples/dgcnn/train.py --synthetic [--clouds 240 --points 256 --k 16 --hidden 32,32,64 --emb 128 --epochs 30 --batch 24
                                                --bf16]

--synthetic: every cloud is one of six surfaces -- sphere, cube, torus, cylinder, cone, two crossed discs -- sampled with noise, scaled
anisotropically a little, rotated at random and given its own number of points (between half of --points and --points), so a batch
is a list of clouds of UNEQUAL size: the search runs segmented, and no padding exists.  No dataset is needed.  The script prints the
loss per epoch and at the end the accuracy on held-out clouds.  Adam; --bf16 keeps the layers' activations in bf16 (fp32 parameters).
"""
import argparse
import math
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from dgll_amd.nn.Convolution import DGCNN  # noqa: E402

SURFACES = ("sphere", "cube", "torus", "cylinder", "cone", "discs")


def sample_surface(kind, n, gen):
    """n points of the surface `kind`, roughly inside the unit ball"""
    u, v = torch.rand(n, generator=gen), torch.rand(n, generator=gen)
    a = 2 * math.pi * u
    if kind == "sphere":
        z = 2 * v - 1
        r = (1 - z * z).sqrt()
        p = torch.stack([r * a.cos(), r * a.sin(), z], 1)
    elif kind == "cube":
        p = torch.rand(n, 3, generator=gen) * 2 - 1
        face = torch.randint(0, 3, (n,), generator=gen)
        sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
        p[torch.arange(n), face] = sign
        p = p * 0.7
    elif kind == "torus":
        b = 2 * math.pi * v
        p = torch.stack([(0.7 + 0.3 * b.cos()) * a.cos(), (0.7 + 0.3 * b.cos()) * a.sin(), 0.3 * b.sin()], 1)
    elif kind == "cylinder":
        p = torch.stack([0.6 * a.cos(), 0.6 * a.sin(), 2 * v - 1], 1)
    elif kind == "cone":
        h = v.sqrt()
        p = torch.stack([0.8 * h * a.cos(), 0.8 * h * a.sin(), 1 - 2 * h], 1)
    else:
        r = v.sqrt()
        flat = torch.stack([r * a.cos(), r * a.sin(), torch.zeros(n)], 1)
        swap = torch.rand(n, generator=gen) < 0.5
        p = torch.where(swap[:, None], flat[:, [2, 0, 1]], flat)
    return p


def random_rotation(gen):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=gen))
    return q * torch.sign(torch.diagonal(r))


def make_clouds(count, points, seed):
    """(list of [n_i, 3] clouds with points / 2 <= n_i <= points, labels [count])"""
    gen = torch.Generator().manual_seed(seed)
    clouds, labels = [], []
    for c in range(count):
        label = c % len(SURFACES)
        n = int(torch.randint(points // 2, points + 1, (1,), generator=gen))
        p = sample_surface(SURFACES[label], n, gen) * (0.85 + 0.3 * torch.rand(3, generator=gen))
        p = p @ random_rotation(gen).t() + 0.02 * torch.randn(n, 3, generator=gen)
        clouds.append(p)
        labels.append(label)
    return clouds, torch.tensor(labels)


def batches(clouds, labels, size, order, dev, dtype):
    for at in range(0, len(order), size):
        ids = order[at:at + size].tolist()
        yield torch.cat([clouds[i] for i in ids]).to(dev, dtype), [clouds[i].shape[0] for i in ids], labels[ids].to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--clouds", type=int, default=240)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--hidden", default="32,32,64")
    ap.add_argument("--emb", type=int, default=128)
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
    model = DGCNN(3, hidden=tuple(int(h) for h in args.hidden.split(",")), k=args.k, emb=args.emb, n_classes=len(SURFACES), dropout=0.3).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    n_pts = sum(c.shape[0] for c in clouds)
    print("dgcnn on %d clouds of %d to %d points (%d in all), %d classes, k = %d: %d searches per step, none stores a distance matrix"
          % (args.clouds, args.points // 2, args.points, n_pts, len(SURFACES), args.k, len(model.convs)))
    gen = torch.Generator().manual_seed(1)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0, total, seen = time.time(), 0.0, 0
        for x, segs, y in batches(clouds, labels, args.batch, train_ids[torch.randperm(len(train_ids), generator=gen)], dev, dtype):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(x, segs).float(), y)
            loss.backward()
            opt.step()
            total, seen = total + loss.item() * len(segs), seen + len(segs)
        torch.cuda.synchronize()
        print("epoch %3d  loss %.4f  %.1f ms" % (epoch, total / seen, (time.time() - t0) * 1e3))
    model.eval()
    hit = 0
    with torch.no_grad():
        for x, segs, y in batches(clouds, labels, args.batch, test_ids, dev, dtype):
            hit += int((model(x, segs).argmax(1) == y).sum())
    print("held-out accuracy %.3f on %d clouds (chance %.3f)" % (hit / len(test_ids), len(test_ids), 1.0 / len(SURFACES)))


if __name__ == "__main__":
    main()
