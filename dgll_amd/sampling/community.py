"""CommunityBatchLoader: CoG / Cluster-GCN style batches -- one group of whole communities at a time, as the induced subgraph of its
nodes (dgll_amd/community.py finds the communities and forms the groups)."""
import torch

from ..community import CommunityBook, cog_order
from ..graph import CSRGraph


def induced_range(graph, start, end, normalize="row"):
    """CSRGraph of the subgraph induced by the contiguous node range [start, end) with local ids: the range's rows, the columns
    filtered to the range and shifted.  normalize="row": every entry of a row is 1 / (entries kept in that row); None: the parent's
    values (or none)."""
    if normalize not in ("row", None):
        raise ValueError("normalize must be 'row' or None")
    e0, e1 = int(graph.rowptr[start]), int(graph.rowptr[end])
    col = graph.col[e0:e1]
    keep = (col >= start) & (col < end)
    kept = torch.zeros(e1 - e0 + 1, dtype=torch.int64, device=graph.device)
    torch.cumsum(keep, 0, out=kept[1:])
    rowptr = kept[graph.rowptr[start:end + 1] - e0].contiguous()
    new_col = (col[keep] - start).contiguous()
    if normalize == "row":
        deg = rowptr[1:] - rowptr[:-1]
        val = torch.repeat_interleave(1.0 / deg.clamp(min=1).to(torch.float32), deg)
    else:
        val = None if graph.val is None else graph.val[e0:e1][keep]
    return CSRGraph(rowptr, new_col, val, end - start, end - start, check=False)


class CommunityBatchLoader:
    """Iterates the groups of a CommunityBook: yields (node_range, graph, features, labels) with node_range = (start, end) in the
    book's id space, graph the induced CSRGraph of those nodes with local ids, and the range's rows of the features and labels.

    graph_or_book: a square CSRGraph -- `cog_order(graph, batch_size, **cog_kw)` is run on it (GPU) and the graph relabelled -- or a
    CommunityBook whose `relabel(graph)` result is passed as `graph=`.  features / labels come in the caller's node order and are
    permuted once (`x[book.perm]`); `book.perm[start:end]` names a batch's nodes in the caller's ids.  shuffle: a seeded
    permutation of the groups per epoch.  The induced graphs are built on first use and kept."""

    def __init__(self, graph_or_book, features, labels, batch_size, shuffle=False, seed=0, normalize="row", graph=None, **cog_kw):
        if normalize not in ("row", None):
            raise ValueError("normalize must be 'row' or None")
        if isinstance(graph_or_book, CommunityBook):
            if graph is None or graph.perm is None or not torch.equal(graph.perm, graph_or_book.perm.to(graph.device)):
                raise ValueError("with a CommunityBook, pass graph=book.relabel(the graph)")
            self.book, self.graph = graph_or_book, graph
        else:
            self.book = cog_order(graph_or_book, batch_size, seed=seed, **cog_kw)
            self.graph = self.book.relabel(graph_or_book)
        perm = self.book.perm
        self.features = None if features is None else features[perm.to(features.device)]
        self.labels = None if labels is None else labels[perm.to(labels.device)]
        self.batch_size, self.shuffle, self.seed, self.normalize = int(batch_size), bool(shuffle), int(seed), normalize
        self.ranges = [tuple(r) for r in self.book.group_ranges.tolist()]
        self.epoch = 0
        self._graphs = {}

    def __len__(self):
        return len(self.ranges)

    def batch(self, i):
        start, end = self.ranges[i]
        g = self._graphs.get(i)
        if g is None:
            g = self._graphs[i] = induced_range(self.graph, start, end, self.normalize)
        return ((start, end), g, None if self.features is None else self.features[start:end],
                None if self.labels is None else self.labels[start:end])

    def __iter__(self):
        order = list(range(len(self.ranges)))
        if self.shuffle:
            gen = torch.Generator()
            gen.manual_seed(self.seed + 7919 * self.epoch)
            order = torch.randperm(len(order), generator=gen).tolist()
        self.epoch += 1
        for i in order:
            yield self.batch(i)
