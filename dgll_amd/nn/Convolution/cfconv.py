"""Continuous-filter convolution (DGL's CFConv, SchNet's interaction layer: argument names and module names, hence state-dict keys)
on the gfx950 aggregation engine.

    CFConv(node_in_feats, edge_in_feats, hidden_feats, out_feats)
    ShiftedSoftplus(beta=1, shift=2, threshold=20)          softplus(x) - log(shift)

Over the entries j of row i of the graph (a CSRGraph [n_dst x n_src], anything as_csr_graph takes; rectangular blocks allowed; edge
values are ignored), with a_ij the attributes of that entry (SchNet: the radial basis expansion of the distance) in the graph's
entry order:

    w_ij = project_edge(a_ij)        project_edge = Linear, ShiftedSoftplus, Linear, ShiftedSoftplus     [nnz, hidden_feats]
    out_i = project_out(sum_j project_node(h_j) * w_ij)      project_node = Linear; project_out = Linear, ShiftedSoftplus

The state-dict keys are DGL's: project_edge.0.*, project_edge.2.*, project_node.*, project_out.0.*.  The aggregation is ONE pass of
ops_ef (u_op_e_sum with op="mul"): the product h_j * w_ij does not exist per edge, and the backward reads h and w again.  A
hidden width that is not a whole number of 16-byte vectors is padded with zero columns (0 * 0 = 0) and unpadded after the
aggregation.  A row without entries aggregates 0.  On the GPU the Linear layers run through dense.linear (bf16 activations with
fp32 parameters included).  Host tensors take gineconv's `_host_aggregate`; a GPU tensor never reaches it.
"""
import math

from ... import backend as F
from ...graph import as_csr_graph
from .agnnconv import _linear
from .dotgatconv import _split_feat
from .gineconv import _aggregate


class ShiftedSoftplus(F.nn.Module):
    """softplus(x) - log(shift), DGL's: 0 at x = 0 with the default shift of 2."""

    def __init__(self, beta=1, shift=2, threshold=20):
        super().__init__()
        self.shift = shift
        self.softplus = F.nn.Softplus(beta=beta, threshold=threshold)

    def forward(self, inputs):
        if inputs.dtype == F.float32 or inputs.dtype == F.float64:
            return self.softplus(inputs) - math.log(float(self.shift))
        # bf16: the difference is formed in fp32 and rounded once (softplus(x) rounded first would cancel against log(shift) near x = 0)
        return (self.softplus(inputs.float()) - math.log(float(self.shift))).to(inputs.dtype)


def _run(seq, h):
    """a Sequential of Linear and element-wise modules, the Linear ones through the dense transform path on the GPU"""
    for m in seq:
        h = _linear(m, h) if isinstance(m, F.nn.Linear) else m(h)
    return h


class CFConv(F.nn.Module):
    """DGL's CFConv.  forward(graph, node_feats, edge_feats) -> [n_dst, out_feats]; node_feats: a tensor [n_src, node_in_feats], or
    (feat_src, feat_dst) for blocks (only the sources enter); edge_feats [nnz, edge_in_feats] in the graph's entry order."""

    def __init__(self, node_in_feats, edge_in_feats, hidden_feats, out_feats):
        super().__init__()
        self.project_edge = F.nn.Sequential(F.nn.Linear(edge_in_feats, hidden_feats), ShiftedSoftplus(),
                                            F.nn.Linear(hidden_feats, hidden_feats), ShiftedSoftplus())
        self.project_node = F.nn.Linear(node_in_feats, hidden_feats)
        self.project_out = F.nn.Sequential(F.nn.Linear(hidden_feats, out_feats), ShiftedSoftplus())

    def forward(self, graph, node_feats, edge_feats):
        graph = as_csr_graph(graph)
        h_src, _ = _split_feat(graph, node_feats)
        if edge_feats.dim() != 2 or edge_feats.shape[0] != graph.nnz:
            raise ValueError("CFConv: edge features must be [nnz, edge_in_feats] with nnz = %d in the graph's entry order, got %s"
                             % (graph.nnz, tuple(edge_feats.shape)))
        hv = _linear(self.project_node, h_src)
        he = _run(self.project_edge, edge_feats).to(hv.dtype)
        return _run(self.project_out, _aggregate(graph, hv, he, "mul"))
