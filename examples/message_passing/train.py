#!/usr/bin/env python3
"""Layers written with the per-edge operators of dgll_amd.ops_mp (the general path under the fused attention layers):

    python examples/message_passing/train.py --synthetic [--nodes 20000 --communities 8 --bf16 --layer agnn|gat]

--layer gat (the default) is a two-layer multi-head GAT written HERE with the operators alone -- copy `MPGATConv` to start a layer
of your own:

    e = leaky_relu(u_add_v(a_src . z_j, a_dst . z_i))      alpha = edge_softmax(e)      out_i = u_mul_e_sum(z, alpha)

--layer agnn is nn.AGNN (DGL's AGNNConv: cosine attention with a learnable scale), which is built on the same operators.
--synthetic: the planted-community graph of examples/transformer/train.py with noisy one-hot-ish features; every node trains.  Adam;
--bf16 keeps the activations in bf16 (fp32 parameters; per-edge tensors are fp32 either way).

What this path costs next to nn.gatConv (fused, nothing per edge): e, alpha and their gradients are real [nnz, heads] fp32 tensors.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from dgll_amd import dense, ops_mp, synth  # noqa: E402
from dgll_amd.nn.Convolution import AGNN  # noqa: E402


def planted(n, k, avg_in, avg_out, seed, device):
    """Symmetric planted-community graph with self-loops and (labels, features): node v belongs to community v % k."""
    gen = torch.Generator().manual_seed(seed)
    labels = torch.arange(n) % k
    m_in, m_out = n * avg_in // 2, n * avg_out // 2
    src_in = torch.randint(0, n, (m_in,), generator=gen)
    dst_in = (torch.randint(0, n // k, (m_in,), generator=gen) * k + src_in % k).clamp(max=n - 1)       # same community
    src_out, dst_out = torch.randint(0, n, (m_out,), generator=gen), torch.randint(0, n, (m_out,), generator=gen)
    graph = synth.build_graph(torch.cat([src_in, src_out]), torch.cat([dst_in, dst_out]), n, symmetric=True, self_loops=True, weighted=False)
    width = max(16, k)
    x = torch.nn.functional.one_hot(labels, width).float() + torch.randn(n, width, generator=gen)
    return graph.to(device), labels.to(device), x.to(device)


class MPGATConv(torch.nn.Module):
    """GAT (Velickovic et al.) from the per-edge operators.  out_feats per head must be a whole number of 16-byte vectors (4 fp32 / 8
    bf16 columns).  forward(graph, x, get_attention=False) -> [n, heads * out_feats] (and alpha [nnz, heads])."""

    def __init__(self, in_feats, out_feats, heads, negative_slope=0.2):
        super().__init__()
        self.heads, self.out_feats, self.negative_slope = heads, out_feats, negative_slope
        self.fc = torch.nn.Linear(in_feats, heads * out_feats, bias=False)
        self.attn_src = torch.nn.Parameter(torch.randn(heads, out_feats) * out_feats ** -0.5)
        self.attn_dst = torch.nn.Parameter(torch.randn(heads, out_feats) * out_feats ** -0.5)

    def forward(self, graph, x, get_attention=False):
        z = dense.linear(x, self.fc.weight.t())                                         # [n, heads * out_feats]
        zh = z.view(-1, self.heads, self.out_feats).float()
        s_src, s_dst = (zh * self.attn_src).sum(-1), (zh * self.attn_dst).sum(-1)       # [n, heads] fp32
        e = torch.nn.functional.leaky_relu(ops_mp.u_add_v(graph, s_src, s_dst), self.negative_slope)
        alpha = ops_mp.edge_softmax(graph, e)                                           # [nnz, heads]
        out = ops_mp.u_mul_e_sum(graph, z, alpha, self.heads)
        return (out, alpha) if get_attention else out


class MPGAT(torch.nn.Module):
    def __init__(self, nfeat, nhid, nclass, heads):
        super().__init__()
        self.layer1 = MPGATConv(nfeat, nhid, heads)
        self.layer2 = MPGATConv(nhid * heads, -(-nclass // 8) * 8, 1)       # one head, padded to whole vectors of either dtype
        self.nclass = nclass

    def forward(self, graph, x):
        h = torch.nn.functional.elu(self.layer1(graph, x))
        return self.layer2(graph, h)[:, :self.nclass]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--layer", choices=("gat", "agnn"), default="gat")
    ap.add_argument("--nodes", type=int, default=20_000)
    ap.add_argument("--communities", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=8, help="per head (gat); the embedding width is hidden * heads (agnn)")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    if not args.synthetic:
        raise SystemExit("pass --synthetic (the planted-community graph is the only data source of this example)")
    if not torch.cuda.is_available():
        raise SystemExit("this example runs the HIP kernels: a GPU is required")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    graph, labels, x = planted(args.nodes, args.communities, 12, 3, 0, dev)
    if args.bf16:
        x = x.to(torch.bfloat16)
    nclass = int(labels.max()) + 1
    if args.layer == "gat":
        model = MPGAT(x.shape[1], args.hidden, nclass, args.heads).to(dev)
    else:
        model = AGNN(x.shape[1], args.hidden * args.heads, nclass).to(dev)
    print("%s on %d nodes, %d entries: a per-edge tensor of %d heads is %.1f MB" %
          (args.layer, graph.n_rows, graph.nnz, args.heads if args.layer == "gat" else 1,
           4e-6 * graph.nnz * (args.heads if args.layer == "gat" else 1)))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0 = time.time()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(graph, x).float(), labels)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if epoch % 10 == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                pred = model(graph, x).argmax(1)
            print("epoch %3d  loss %.4f  acc %.3f  %.1f ms" % (epoch, loss.item(), (pred == labels).float().mean().item(), dt * 1e3))


if __name__ == "__main__":
    main()
