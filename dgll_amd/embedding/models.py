"""The reference's classes -- SkipGramModel, RandomWalkEmbedding, DeepWalk, Node2vec -- on the device kernels."""
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn

from ..graph import CSRGraph
from .sgns import NoiseTable, sgns_step
from .struc2vec import StrucContext, struc_walks
from .walks import AliasTable, as_walk_graph, random_walks, walk_info


class SkipGramModel(nn.Module):
    """skipgram.py:3-26: W1 [N, D] and W2 [D, N], both torch.rand.  The output table is stored [N, D] (rows are what the kernels
    gather and add to); W2 is its transposed view, so `forward` computes what the reference's does."""

    def __init__(self, totalNodes, embedDim, device=None):
        super().__init__()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.W1 = nn.Parameter(torch.rand((totalNodes, embedDim)).to(device), requires_grad=False)
        w2 = torch.rand((embedDim, totalNodes))
        self.W_out = nn.Parameter(w2.t().contiguous().to(device), requires_grad=False)

    @property
    def W2(self):
        return self.W_out.t()

    def forward(self, features):
        return torch.matmul(torch.matmul(features.to(self.W1.device), self.W1), self.W2)


def _encode_graph(graph, device, weighted=False):
    """(CSRGraph on the device, sorted node labels or None).  networkx graphs: labels are encoded by their sorted order; with
    `weighted` the edges carry their `weight` attribute, 1 where it is missing (node2vec.py:43-47)."""
    from ..data.dgraph import DGraph

    if isinstance(graph, (CSRGraph, DGraph)):
        return as_walk_graph(graph, device), None
    if not (hasattr(graph, "nodes") and hasattr(graph, "adjacency")):
        raise TypeError("graph must be a networkx graph, a CSRGraph or a DGraph, got %r" % type(graph))
    labels = sorted(graph.nodes())
    code = {v: i for i, v in enumerate(labels)}
    src, dst, val = [], [], []
    for v, nbrs in graph.adjacency():
        cv = code[v]
        for u, attr in nbrs.items():
            src.append(cv)
            dst.append(code[u])
            if weighted:
                val.append(attr.get("weight", 1))
    n = len(labels)
    g = CSRGraph.from_coo(torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64),
                          torch.tensor(val, dtype=torch.float32) if weighted else None, (n, n))
    return g.to(device), labels


class RandomWalkEmbedding:
    """randomWalkEmbedding.py:9-66 with the training loop both subclasses share.
    Keyword-only extras: negatives (K per pair), batch_walks (walks per launch and per synchronous step), seed (None: drawn from
    numpy's global generator), device, weighted (walk in proportion to the edge weights: networkx's `weight` attribute or the
    CSR's values; the table is built here, once)."""
    p = q = 1.0

    def __init__(self, graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, negatives=5, batch_walks=1024, seed=None,
                 device=None, weighted=False):
        self.graph = graph
        if walkLength == 0:
            self.walkLength = 3
            warnings.warn("Set Walk to default: {}".format(self.walkLength))
        else:
            self.walkLength = walkLength
        if embedDim == 0:
            self.embedDim = 2
            warnings.warn("Set Embedding Dimention to default: {}".format(self.embedDim))
        else:
            self.embedDim = embedDim
        if numbOfWalksPerVertex == 0:           # difference (d)
            self.numbOfWalksPerVertex = 3
            warnings.warn("Set Walks per Vertex to default: {}".format(self.numbOfWalksPerVertex))
        else:
            self.numbOfWalksPerVertex = numbOfWalksPerVertex
        if windowSize == 0:
            self.windowSize = 3
            warnings.warn("Set Context Window to default: {}".format(self.windowSize))
        else:
            self.windowSize = windowSize
        if lr == 0:
            self.lr = 0.25
            warnings.warn("Set Learning Rate to default: {}".format(self.lr))
        else:
            self.lr = lr
        if device is None:
            device = graph.device if isinstance(graph, CSRGraph) and graph.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.csr, self.labels = _encode_graph(graph, self.device, bool(weighted))
        self.alias = AliasTable.from_graph(self.csr) if weighted else None
        self._code = None if self.labels is None else {v: i for i, v in enumerate(self.labels)}
        self.totalNodes = self.csr.n_rows
        self.negatives, self.batch_walks = int(negatives), int(batch_walks)
        if self.batch_walks < 1:
            raise ValueError("batch_walks must be >= 1")
        self.seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if seed is None else int(seed)
        self.noise = NoiseTable.from_graph(self.csr).to(self.device)
        self.model = None
        self.losses = []                  # loss sum of every epoch (learnNodeEmbedding call), for inspection
        self._walks_drawn = 0             # global walk index: no two walks of this object share a Philox counter
        self._epoch = 0
        self.adj_list = None

    # ---- the reference's accessors ---------------------------------------------------------------------------------------
    def encode(self, node):
        if self._code is None:
            return int(node)
        return self._code[node]

    def getAdjacencyList(self):
        if self.adj_list is None:
            rp, col = self.csr.rowptr.cpu().tolist(), self.csr.col.cpu().tolist()
            self.adj_list = [col[rp[i]:rp[i + 1]] for i in range(self.totalNodes)]
        return self.adj_list

    def getGraph(self):
        return self.graph

    # ---- walks -------------------------------------------------------------------------------------------------------------
    def _walk_batch(self, starts, length, info=None):
        walks = random_walks(self.csr, starts, length, p=self.p, q=self.q, seed=self.seed, first_walk_index=self._walks_drawn, info=info,
                             alias=self.alias)
        first = self._walks_drawn
        self._walks_drawn += int(starts.numel())
        return walks, first

    def RandomWalk(self, node, t):
        """Encoded ids of one walk of at most t nodes from `node` (it ends early at a node without out-edges)."""
        starts = torch.tensor([self.encode(node)], dtype=torch.int64, device=self.device)
        walks, _ = self._walk_batch(starts, int(t))
        return [v for v in walks[0].cpu().tolist() if v >= 0]

    # ---- training ----------------------------------------------------------------------------------------------------------
    def _train(self, model, shuffle):
        if model.W1.shape != (self.totalNodes, self.embedDim) or not model.W1.is_cuda:
            raise ValueError("the model must hold [%d, %d] tables on the GPU" % (self.totalNodes, self.embedDim))
        self.model = model
        w_in, w_out = model.W1.data, model.W_out.data
        info = torch.zeros(2, dtype=torch.int64, device=self.device)
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        gen = torch.Generator()
        for r in range(self.numbOfWalksPerVertex):
            gen.manual_seed((self.seed + 0x9E3779B97F4A7C15 * (self._epoch * self.numbOfWalksPerVertex + r + 1)) % (2 ** 63))
            order = torch.randperm(self.totalNodes, generator=gen) if shuffle else torch.arange(self.totalNodes)
            order = order.to(self.device)
            for b in range(0, self.totalNodes, self.batch_walks):
                walks, first = self._walk_batch(order[b:b + self.batch_walks], self.walkLength, info)
                total += sgns_step(w_in, w_out, walks, self.windowSize, self.negatives, self.noise, self.lr, self.seed, first)
        self._epoch += 1
        self.last_capped = walk_info(info)       # the one blocking read of the epoch (raises on a bad graph)
        self.losses.append(float(total))
        return self.model

    def learnNodeEmbedding(self, model):
        """One epoch: numbOfWalksPerVertex rounds over a seeded shuffle of all nodes, in batches of batch_walks starts."""
        return self._train(model, shuffle=True)

    def learnEdgeEmbedding(self, model):
        """As learnNodeEmbedding, over the nodes in order (deepWalk.py:72-80)."""
        return self._train(model, shuffle=False)

    def getNodeEmbedding(self, node):
        return self.model.W1[self.encode(node)].data

    def getEdgeEmbedding(self, srcNode, dstNode):
        return self.getNodeEmbedding(srcNode) * self.getNodeEmbedding(dstNode)       # utils.py operator_hadamard


class DeepWalk(RandomWalkEmbedding):
    """deepWalk.py:13-85: uniform walks; weighted=True: first-order walks in proportion to the edge weights."""

    def __init__(self, graph=None, walkLength=0, embedDim=0, numbOfWalksPerVertex=0, windowSize=0, lr=0, **kw):
        if graph is None:
            warnings.warn("Provide a graph: {}".format(graph))
            sys.exit()
        super().__init__(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, **kw)


class Struc2Vec(RandomWalkEmbedding):
    """struc2vec.py:22-61: walks over the multilayer context graph of structural similarity (StrucContext, built here, once, on the
    device); stay_prob == 0 selects 0.3.  temp_path and reuse are accepted and ignored: nothing is pickled to disk.  The noise
    table of the negative draws stays in-degree^0.75 of the input graph."""

    def __init__(self, graph=None, walkLength=0, embedDim=0, numbOfWalksPerVertex=0, windowSize=0, lr=0, verbose=0, stay_prob=0,
                 opt1_reduce_len=True, opt2_reduce_sim_calc=True, opt3_num_layers=None, temp_path=None, reuse=False, **kw):
        if graph is None:
            warnings.warn("Provide a graph: {}".format(graph))
            sys.exit()
        super().__init__(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, **kw)
        if stay_prob == 0:
            self.stay_prob = 0.3
            warnings.warn("Set stay prob. to default: {}".format(self.stay_prob))
        else:
            self.stay_prob = stay_prob
        self.verbose = verbose
        self.opt1_reduce_len, self.opt2_reduce_sim_calc, self.opt3_num_layers = opt1_reduce_len, opt2_reduce_sim_calc, opt3_num_layers
        self.context = StrucContext.from_graph(self.csr, opt1_reduce_len, opt2_reduce_sim_calc, opt3_num_layers)

    def _walk_batch(self, starts, length, info=None):
        walks = struc_walks(self.context, starts, length, self.stay_prob, self.seed, self._walks_drawn, info=info)
        first = self._walks_drawn
        self._walks_drawn += int(starts.numel())
        return walks, first


class Node2vec(RandomWalkEmbedding):
    """node2vec.py:13-118: second-order walks with return parameter p and in-out parameter q (0 selects 0.5 and 0.8); weighted=True
    multiplies every transition by the edge's weight, as the reference's computeProbabilities does."""

    def __init__(self, graph=None, walkLength=0, embedDim=0, numbOfWalksPerVertex=0, windowSize=0, lr=0, p=0, q=0, **kw):
        if graph is None:
            warnings.warn("Provide a graph: {}".format(graph))
            sys.exit()
        super().__init__(graph, walkLength, embedDim, numbOfWalksPerVertex, windowSize, lr, **kw)
        if p == 0:
            self.p = 0.5
            warnings.warn("Set p to default: {}".format(self.p))
        else:
            self.p = p
        if q == 0:
            self.q = 0.8
            warnings.warn("Set q to default: {}".format(self.q))
        else:
            self.q = q
