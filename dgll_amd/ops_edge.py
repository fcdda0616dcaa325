"""Per-edge operators of the GAT / SpecialSpmm path (C ABI: dgll_hip_sddmm_csr, dgll_hip_gat_pass,
dgll_hip_segment_max).  GPU only; no fallback."""
import ctypes as C
import os

import torch

from . import _lib
from .graph import CSRGraph
from .ops import _dtype_code, epv, _require_cuda, alloc_features, as_rows16


def _ready(x):
    """x on 16-byte rows for kernels that load whole vectors and use the columns behind the last one: a copy has zeros there."""
    return as_rows16(x, zero_pad=True)


def _empty_padded(n, width, dtype, device):
    return alloc_features(n, width, dtype, device, pad_to=epv(dtype))


def _ws(plan, heads, fo, dev, other_plan=None):
    """(workspace or None, its size in bytes) of a GAT pass over `plan` (the larger of the two for a pass pair)."""
    n = int(_lib.lib.dgll_hip_gat_workspace_bytes(plan, heads, fo))
    if other_plan is not None:
        n = max(n, int(_lib.lib.dgll_hip_gat_workspace_bytes(other_plan, heads, fo)))
    return (torch.empty(n, dtype=torch.uint8, device=dev) if n else None), n


# ------------------------------------------------------------------------------------------------ SDDMM
def sddmm_raw(graph, g, b):
    """edge_out[k] = <g[row(k)], b[col[k]]> -- SpecialSpmmFunction.backward's grad_values (gatconv.py:76-78)."""
    _require_cuda(g, b, graph.rowptr)
    if g.dtype != b.dtype:
        b = b.to(g.dtype)
    feat = g.shape[1]
    tile = 64 * epv(g.dtype)
    out = torch.empty(graph.nnz, dtype=torch.float32, device=g.device)
    total = None
    for c0 in range(0, feat, tile):  # > 64 vectors per row: column blocks, summed
        gs, bs = _ready(g[:, c0:c0 + tile]), _ready(b[:, c0:c0 + tile])
        _lib.launch("dgll_hip_sddmm_csr", g.device, graph.rowptr.data_ptr(), graph.col.data_ptr(), gs.data_ptr(), gs.stride(0),
                    bs.data_ptr(), bs.stride(0), _dtype_code(gs), out.data_ptr(), graph.n_rows, gs.shape[1])
        if feat > tile:
            total = out.clone() if total is None else total + out
    return out if total is None else total


# ------------------------------------------------------------------------------------------------ segment max
class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph):
        _require_cuda(x, graph.rowptr)
        if x.shape[0] != graph.n_cols:      # the backward walks the transposed structure: one row pointer per source row
            raise ValueError("X has %d rows but the adjacency gathers from %d" % (x.shape[0], graph.n_cols))
        xs = _ready(x)
        feat = x.shape[1]
        y = _empty_padded(graph.n_rows, feat, x.dtype, x.device)
        arg = torch.empty((graph.n_rows, y.stride(0)), dtype=torch.int32, device=x.device)
        _lib.launch("dgll_hip_segment_max", x.device, graph.rowptr.data_ptr(), graph.col.data_ptr(), xs.data_ptr(), xs.stride(0),
                    y.data_ptr(), arg.data_ptr(), y.stride(0), _dtype_code(xs), graph.n_rows, feat)
        ctx.save_for_backward(arg)
        ctx.n_src, ctx.graph, ctx.feat = x.shape[0], graph, feat
        return y

    @staticmethod
    def backward(ctx, g):
        """The gradient goes to the arg-max row only: a gather over the transposed structure (dgll_hip_segment_max_bwd),
        one wavefront per source row, no atomics.  Sampled blocks (col == arange: every source row has exactly one
        in-edge) need no sort: their transposed structure is rowptr = arange, col = the row of each edge."""
        (arg,) = ctx.saved_tensors
        graph, feat = ctx.graph, ctx.feat
        if graph.identity_cols and graph.n_cols == graph.nnz:
            t_rowptr = torch.arange(ctx.n_src + 1, dtype=torch.int64, device=g.device)
            t_col = graph.row_index().to(torch.int32)
        else:
            gt, _ = graph.transpose()
            t_rowptr, t_col = gt.rowptr, gt.col
        gs = _ready(g.to(arg.device))
        grad = _empty_padded(ctx.n_src, feat, g.dtype, g.device)
        _lib.launch("dgll_hip_segment_max_bwd", g.device, t_rowptr.data_ptr(), t_col.data_ptr(), gs.data_ptr(), gs.stride(0),
                    arg.data_ptr(), arg.stride(0), grad.data_ptr(), grad.stride(0), _dtype_code(gs), ctx.n_src, feat)
        return grad, None


def segment_max(graph, x):
    """max over each row's neighbours -- NeighborAggregator 'max' (sageconv.py:37-38); empty rows give 0."""
    return _SegmentMax.apply(x, graph)


# ------------------------------------------------------------------------------------------------ fused GAT
def head_width_padded(fo, dtype, pow2=True):
    """Per-head column count the kernels need: a whole number of 16-byte vectors -- a power of two of them for the
    first-generation kernels (max-subtracted softmax, attention dropout given as an edge_scale array), any number for
    sparseGatConv's form, with or without dropout drawn in the kernels."""
    vec = epv(dtype)
    vecs = -(-fo // vec)
    if not pow2:
        return vecs * vec
    p = 1
    while p < vecs:
        p <<= 1
    return p * vec


def _row_slot(x, byte_off, n_floats):
    """fp32 [rows, n_floats] alias of the bytes [byte_off, byte_off + 4 n_floats) of every row of `x`'s storage -- a slot in
    the padding between a row's last column and the next row (the caller owns that padding)."""
    esz = x.element_size()
    base, stride = x.storage_offset() * esz + byte_off, x.stride(0) * esz
    if base % 4 or stride % 4 or byte_off + 4 * n_floats > stride:
        raise ValueError("no room for a %d-float slot at byte %d of %d-byte rows" % (n_floats, byte_off, stride))
    return torch.empty(0, dtype=torch.float32, device=x.device).set_(x.untyped_storage(), base // 4, (x.shape[0], n_floats),
                                                                    (stride // 4, 1))


def _empty_like_rows(n, like):
    """[n, like.shape[1]] with `like`'s row stride (the same padding behind every row)."""
    return alloc_features(n, like.shape[1], like.dtype, like.device, pad_to=like.stride(0))


ROW_SCORES = os.environ.get("DGLL_GAT_ROW_SCORES", "1") != "0"     # 0: the forward always gathers T (A/B, tests)
ROW_SCORES_BWD = os.environ.get("DGLL_GAT_ROW_SCORES_BWD", "1") != "0"   # the rows pass of the backward in the same form (6.07 -> 5.68 ms)


def dropout_seed(device):
    """Two 32-bit seed words on `device` from torch's generator there (follows torch.manual_seed; safe under graph capture: a replay
    draws new words, and the kernels read them from this tensor)."""
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (2,), dtype=torch.int32, device=device)


def _check_dropout(p, seed, device):
    """(p, seed) of an active in-kernel dropout, or None."""
    p = float(p)
    if p == 0.0:
        return None
    if not 0.0 < p < 1.0:
        raise ValueError("dropout_p must lie in [0, 1), got %r" % p)
    if seed is None:
        seed = dropout_seed(device)
    if seed.dtype != torch.int32 or seed.numel() != 2 or seed.device != device or not seed.is_contiguous():
        raise ValueError("dropout_seed must be a contiguous 2-element int32 tensor on the layer's device")
    return p, seed


def gat_dropout_mask(graph, heads, p, seed):
    """fp32 [nnz, heads] multipliers the kernels draw for (p, seed) -- dgll_hip_gat_dropout_mask for a graph on the GPU (seed: 2-element
    int32 tensor there), dgll_host_gat_dropout_mask for host tensors.  For tests and for the explicit edge_scale= path; training with
    dropout_p never materialises it."""
    dev = graph.rowptr.device
    seed = seed.to(torch.int32).contiguous()
    out = torch.empty((graph.nnz, heads), dtype=torch.float32, device=dev)
    col = graph.col.contiguous()
    if dev.type == "cuda":
        _lib.launch("dgll_hip_gat_dropout_mask", dev, graph.rowptr.data_ptr(), col.data_ptr(), graph.n_rows, heads, seed.data_ptr(),
                    float(p), out.data_ptr())
    else:
        code = _lib.lib.dgll_host_gat_dropout_mask(graph.rowptr.data_ptr(), col.data_ptr(), graph.n_rows, heads, seed.data_ptr(), float(p),
                                                   out.data_ptr())
        _lib.check(code, "dgll_host_gat_dropout_mask")
    return out


def _rowscore_addressable(h):
    """The row-score kernels address the gathered rows by 32-bit byte offsets formed with a 24-bit multiply: at most 2^24 rows of
    less than 2^24 bytes, 4 GB in all.  Mirrors rowscore_addressable() of csrc/edge.hip (the passes refuse what this would let through)."""
    row_bytes = h.stride(0) * h.element_size()
    return h.shape[0] <= (1 << 24) and row_bytes < (1 << 24) and h.shape[0] * row_bytes <= 0xFFFFFFFF


def _gat_pass(kind, graph, heads, fo, alpha, h, apply_elu=0, mode=0, ws=None, perm=None, n_cols=None, tag=None, **fields):
    """One dgll_hip_gat_pass launch over `graph` (A; A^T for the transposed pass).  `fields`: further members of dgll_gat_desc by name,
    as the values the struct takes (addresses, pitches in elements; None is NULL).  ws: (workspace, bytes) shared with another pass,
    None = this pass's own.  n_cols: None = the graph's."""
    dev = h.device
    plan = graph.plan()
    ws, ws_bytes = _ws(plan, heads, fo, dev) if ws is None else ws
    # the leading members of the struct in its order (pass .. workspace_bytes), the rest by name: one call fills the descriptor
    d = _lib.GatDesc(kind, _dtype_code(h), mode, apply_elu, plan, graph.rowptr.data_ptr(), graph.col.data_ptr(), _lib.ptr(perm), graph.n_rows,
                     graph.n_cols if n_cols is None else n_cols, heads, fo, alpha, _lib.ptr(ws), ws_bytes, h=h.data_ptr(), ld_h=h.stride(0),
                     **fields)
    _lib.launch("dgll_hip_gat_pass", dev, C.byref(d), tag=tag)


def _drop_fields(dropout):
    """dgll_gat_desc's drop_p / drop_seed of an active (p, seed); nothing without dropout."""
    return {} if dropout is None else {"drop_p": dropout[0], "drop_seed": dropout[1].data_ptr()}


def _gat_strided_forward(h, s, t, graph, heads, fo, alpha, apply_elu, pack_scores, attn2=None, dropout=None):
    """Forward gather pass with strided scores.  Returns (h with aligned rows, s, t, out, rowsum, packed).
    attn2: fp32 [heads * fo], a2 of every head laid out like a row of h (t = h . a2 per head): when the scores cannot ride in the rows'
    padding the pass forms t_j from the row it gathers anyway instead of fetching T[j] (the row-score form: attn2 with a NULL
    col_score; the reference builds its logit from the gathered rows too, gatconv.py:122-125).
    dropout: (p, seed) -- attention dropout drawn in the kernel (either score form; the scores do not ride in the rows' padding then:
    the in-row form has no dropout instantiation)."""
    _require_cuda(h, s, t, graph.rowptr)
    dev = h.device
    h = _ready(h)
    esz, width = h.element_size(), heads * fo
    s = s.to(torch.float32).contiguous()
    t = t.to(torch.float32).contiguous()
    packed = bool(pack_scores) and dropout is None and (h.stride(0) - width) * esz >= 4 * heads
    if packed:
        t_gather = _row_slot(h, width * esz, heads)
        t_gather.copy_(t)
    else:
        t_gather = t
    out = _empty_like_rows(graph.n_rows, h)
    rowsum = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev)
    row_scores = attn2 is not None and not packed and ROW_SCORES and _rowscore_addressable(h)
    form = "packed" if packed else ("rowscore" if row_scores else "")
    if dropout is not None:
        form = (form + " dropout").strip()
    # how the t_j reach the pass: formed from the gathered rows (attn2, which n_cols = the rows of h bounds), or gathered
    if row_scores:
        a2 = attn2.detach().to(torch.float32).contiguous()
        scores = {"attn2": a2.data_ptr()}
    else:
        scores = {"col_score": t_gather.data_ptr(), "col_score_stride": t_gather.stride(0)}
    _gat_pass(_lib.GAT_FORWARD, graph, heads, fo, float(alpha), h, apply_elu=int(apply_elu), n_cols=int(h.shape[0]), row_score=s.data_ptr(),
              out=out.data_ptr(), ld_out=out.stride(0), rowsum=rowsum.data_ptr(), **scores, **_drop_fields(dropout),
              tag=lambda: ("gat", "fwd", heads, fo, str(h.dtype), graph.nnz, form))
    return h, s, t, out, rowsum, packed


def _gat_strided_backward(g, h, s, t, out, rowsum, graph, heads, fo, alpha, apply_elu, packed, attn=None, rows_first=False,
                          dropout=None):
    """Both backward gather passes (rows of A, then rows of A^T) with strided scores.  attn = (a1, a2) fp32 [heads * fo]: the
    scores are S = H.a1, T = H.a2 per head and their contribution to grad_h is added by the second pass's epilogue.
    dropout: the forward's (p, seed): both passes draw the same mask again.
    Returns (grad_h, grad_s, grad_t)."""
    dev, esz, width = h.device, h.element_size(), heads * fo
    g = _ready(g.to(h.dtype))
    gt, _ = graph.transpose()
    dn = _empty_like_rows(graph.n_rows, h)
    t_gather = _row_slot(h, width * esz, heads) if packed else t       # written by the forward; h's padding is ours
    if packed and (dn.stride(0) - width) * esz >= 8 * heads:
        sd = _row_slot(dn, width * esz, 2 * heads)
    else:
        sd = torch.empty((graph.n_rows, 2 * heads), dtype=torch.float32, device=dev)
    grad_h = _empty_like_rows(graph.n_cols, h)
    grad_s = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev)
    grad_t = torch.empty((graph.n_cols, heads), dtype=torch.float32, device=dev)
    ws = _ws(graph.plan(), heads, fo, dev, gt.plan())      # one workspace: the transposed pass is stream-ordered after the rows pass
    kind = (heads, fo, str(h.dtype), graph.nnz, "packed" if packed else ("dropout" if dropout is not None else ""))
    a1 = a2 = None
    gs_cols = grad_s
    if attn is not None:
        if graph.n_rows != graph.n_cols:
            # a rectangular adjacency whose rows ARE its first n_rows columns (a rank's merged adjacency, dist.py: own rows, then halo
            # rows): the transposed pass owns n_cols rows, grad_S exists for the first n_rows of them -- nobody uses a halo node's s here
            if not rows_first or graph.n_rows > graph.n_cols:
                raise ValueError("the score-gradient epilogue needs a square adjacency (grad_S of the rows the transposed pass owns)")
            gs_cols = torch.zeros((graph.n_cols, heads), dtype=torch.float32, device=dev)
        a1, a2 = (v.detach().to(torch.float32).contiguous() for v in attn)
    rows_rowscore = a2 is not None and not packed and ROW_SCORES_BWD and _rowscore_addressable(h)
    if rows_rowscore:      # t_j from the gathered rows, as in the forward
        scores = {"attn2": a2.data_ptr()}
    else:
        scores = {"col_score": t_gather.data_ptr(), "col_score_stride": t_gather.stride(0)}
    drop = _drop_fields(dropout)
    # the strided form is always the only launch over its rows: the exact dd_i
    _gat_pass(_lib.GAT_ROWS, graph, heads, fo, alpha, h, apply_elu=apply_elu, ws=ws, phase=_lib.GAT_ROWS_EXACT_ONLY, n_cols=int(h.shape[0]),
              row_score=s.data_ptr(), out=out.data_ptr(), ld_out=out.stride(0), grad_out=g.data_ptr(), ld_grad_out=g.stride(0),
              rowsum=rowsum.data_ptr(), dn=dn.data_ptr(), ld_dn=dn.stride(0), sd=sd.data_ptr(), sd_stride=sd.stride(0),
              grad_score=grad_s.data_ptr(), **scores, **drop,
              tag=lambda: ("gat", "bwd_rows") + (kind[:4] + (("rowscore " + kind[4]).strip(),) if rows_rowscore else kind))
    if gs_cols is not grad_s:
        gs_cols[:graph.n_rows].copy_(grad_s)
    # the rows pass left {s_i, dd_i} side by side in sd: the columns' scores and, `heads` floats behind them, their dd
    _gat_pass(_lib.GAT_TRANSPOSED, gt, heads, fo, alpha, h, ws=ws, dn=dn.data_ptr(), ld_dn=dn.stride(0), row_score=t.data_ptr(),
              col_score=sd.data_ptr(), col_dd=sd.data_ptr() + 4 * heads, col_score_stride=sd.stride(0), grad_h=grad_h.data_ptr(),
              ld_grad_h=grad_h.stride(0), grad_score=grad_t.data_ptr(), attn1=_lib.ptr(a1), attn2=_lib.ptr(a2),
              grad_s_rows=_lib.ptr(gs_cols if a1 is not None else None), **drop, tag=lambda: ("gat", "bwd_cols") + kind)
    return grad_h, grad_s, grad_t


class _GatAggregateStrided(torch.autograd.Function):
    """sparseGatConv's form (exp(-leakyrelu); attention dropout drawn in the kernels from (dropout_p, dropout_seed) when given) on
    the second-generation kernels.  These passes are bound by cache-line fills per edge, so per-node scalars
    that are gathered per edge live next to what is gathered anyway: with `pack_scores` (the caller owns the padding behind
    h's rows) T sits in the padding of the feature rows -- a 47-class output row is 96 of 128 bytes -- and the backward keeps
    {s_i, dd_i} in the padding of its DN rows; without room they are compact / side-by-side arrays."""

    @staticmethod
    def forward(ctx, h, s, t, graph, heads, fo, alpha, apply_elu, pack_scores, dropout_p=0.0, dropout_seed=None):
        drop = _check_dropout(dropout_p, dropout_seed, h.device)
        h, s, t, out, rowsum, packed = _gat_strided_forward(h, s, t, graph, heads, fo, alpha, apply_elu, pack_scores, dropout=drop)
        ctx.graph, ctx.cfg, ctx.packed = graph, (heads, fo, float(alpha), int(apply_elu)), packed
        ctx.drop_p = drop[0] if drop else 0.0
        ctx.save_for_backward(h, s, t, out, rowsum, drop[1] if drop else None)
        return out

    @staticmethod
    def backward(ctx, g):
        h, s, t, out, rowsum, seed = ctx.saved_tensors
        heads, fo, alpha, apply_elu = ctx.cfg
        grad_h, grad_s, grad_t = _gat_strided_backward(g, h, s, t, out, rowsum, ctx.graph, heads, fo, alpha, apply_elu, ctx.packed,
                                                       dropout=(ctx.drop_p, seed) if seed is not None else None)
        return grad_h, grad_s, grad_t, None, None, None, None, None, None, None, None


class _GatLayerStrided(torch.autograd.Function):
    """The whole attention layer after the transform: scores S = H.a1, T = H.a2 per head (one skinny product
    H . blockdiag(a1 | a2), gatconv.py:122-125 without the [2 fo, E] edge matrix), then the aggregation above.  As ONE autograd
    node the backward needs no [n, 2 heads] x [2 heads, heads * fo] product and no add over [n, heads * fo] for the scores'
    contribution to grad_H: the transposed gather pass adds grad_S * a1 + grad_T * a2 in its epilogue."""

    @staticmethod
    def forward(ctx, h, A, graph, heads, fo, alpha, apply_elu, pack_scores, dropout_p=0.0, dropout_seed=None):
        """h: one row per COLUMN of `graph`; a rectangular graph's rows are its first n_rows columns (dist.py's merged adjacency)."""
        from . import dense

        drop = _check_dropout(dropout_p, dropout_seed, h.device)
        h = _ready(h)
        if h.shape[0] != graph.n_cols or graph.n_rows > graph.n_cols:
            raise ValueError("gat_layer: h needs one row per column of the adjacency, whose rows are its first columns")
        Ad = A.detach().to(h.dtype)
        st = (dense.transform_bf16(h, Ad.t(), out_dtype=torch.float32) if (dense._mfma_ok(h) and Ad.shape[1] <= 256)
              else dense.mm_nt(h, Ad.t()).float())
        # a2 of every head laid out like a row of h (A is block-diagonal: column heads + k holds a2 of head k in rows k fo .. (k + 1) fo)
        h, s, t, out, rowsum, packed = _gat_strided_forward(h, st[:graph.n_rows, :heads], st[:, heads:], graph, heads, fo, alpha, apply_elu,
                                                            pack_scores, attn2=Ad[:, heads:].float().sum(1), dropout=drop)
        ctx.graph, ctx.cfg, ctx.packed = graph, (heads, fo, float(alpha), int(apply_elu)), packed
        ctx.drop_p = drop[0] if drop else 0.0
        ctx.save_for_backward(h, Ad, s, t, out, rowsum, drop[1] if drop else None)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import dense

        h, Ad, s, t, out, rowsum, seed = ctx.saved_tensors
        heads, fo, alpha, apply_elu = ctx.cfg
        # block-diagonal A: column k holds a1 of head k in rows k fo .. (k + 1) fo, column heads + k holds a2
        a1 = Ad[:, :heads].float().sum(1)
        a2 = Ad[:, heads:].float().sum(1)
        grad_h, grad_s, grad_t = _gat_strided_backward(g, h, s, t, out, rowsum, ctx.graph, heads, fo, alpha, apply_elu, ctx.packed,
                                                       attn=(a1, a2) if ctx.needs_input_grad[0] else None, rows_first=True,
                                                       dropout=(ctx.drop_p, seed) if seed is not None else None)
        grad_A = None
        if ctx.needs_input_grad[1]:      # dA = H^T . [grad_S | grad_T], columns padded to a 16-byte row for the split-K kernel
            n = 2 * heads
            pad = -n % 8
            gst = torch.zeros((h.shape[0], n + pad), dtype=h.dtype, device=h.device)
            gst[:grad_s.shape[0], :heads] = grad_s
            gst[:, heads:n] = grad_t
            grad_A = dense.grad_weight(h, gst)[:, :n]
        return (grad_h if ctx.needs_input_grad[0] else None), grad_A, None, None, None, None, None, None, None, None


class _GatAggregate(torch.autograd.Function):
    """out = act( sum_j w_ij scale_ij h_j / sum_j w_ij ) for all heads at once; see include/dgll_hip.h."""

    @staticmethod
    def forward(ctx, h, s, t, edge_scale, graph, heads, fo, alpha, apply_elu, mode):
        _require_cuda(h, s, t, graph.rowptr)
        dev = h.device
        h = _ready(h)
        s = s.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        out = _empty_padded(graph.n_rows, heads * fo, h.dtype, dev)
        rowsum = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev)
        rowmax = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev) if mode == 1 else None
        if edge_scale is not None:
            edge_scale = edge_scale.to(torch.float32).contiguous()
        _gat_pass(_lib.GAT_FORWARD, graph, heads, fo, float(alpha), h, apply_elu=int(apply_elu), mode=int(mode), row_score=s.data_ptr(),
                  col_score=t.data_ptr(), edge_scale=_lib.ptr(edge_scale), out=out.data_ptr(), ld_out=out.stride(0), rowsum=rowsum.data_ptr(),
                  rowmax=_lib.ptr(rowmax))
        ctx.graph, ctx.cfg = graph, (heads, fo, float(alpha), int(apply_elu), int(mode))
        ctx.save_for_backward(h, s, t, edge_scale, out, rowsum, rowmax)
        return out

    @staticmethod
    def backward(ctx, g):
        h, s, t, edge_scale, out, rowsum, rowmax = ctx.saved_tensors
        graph = ctx.graph
        heads, fo, alpha, apply_elu, mode = ctx.cfg
        dev = h.device
        g = _ready(g.to(h.dtype))
        gt, perm = graph.transpose()
        dn = _empty_padded(graph.n_rows, heads * fo, h.dtype, dev)
        dd = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev)
        grad_h = _empty_padded(graph.n_cols, heads * fo, h.dtype, dev)
        grad_s = torch.empty((graph.n_rows, heads), dtype=torch.float32, device=dev)
        grad_t = torch.empty((graph.n_cols, heads), dtype=torch.float32, device=dev)
        ws = _ws(graph.plan(), heads, fo, dev, gt.plan())      # one workspace: the transposed pass is stream-ordered after the rows pass
        _gat_pass(_lib.GAT_ROWS, graph, heads, fo, alpha, h, apply_elu=apply_elu, mode=mode, ws=ws, phase=_lib.GAT_ROWS_EXACT_ONLY,
                  row_score=s.data_ptr(), col_score=t.data_ptr(), edge_scale=_lib.ptr(edge_scale), out=out.data_ptr(), ld_out=out.stride(0),
                  grad_out=g.data_ptr(), ld_grad_out=g.stride(0), rowsum=rowsum.data_ptr(), rowmax=_lib.ptr(rowmax), dn=dn.data_ptr(),
                  ld_dn=dn.stride(0), dd=dd.data_ptr(), grad_score=grad_s.data_ptr())
        _gat_pass(_lib.GAT_TRANSPOSED, gt, heads, fo, alpha, h, mode=mode, ws=ws, perm=perm, dn=dn.data_ptr(), ld_dn=dn.stride(0),
                  row_score=t.data_ptr(), col_score=s.data_ptr(), col_dd=dd.data_ptr(), rowmax=_lib.ptr(rowmax), edge_scale=_lib.ptr(edge_scale),
                  grad_h=grad_h.data_ptr(), ld_grad_h=grad_h.stride(0), grad_score=grad_t.data_ptr())
        return grad_h, grad_s, grad_t, None, None, None, None, None, None, None


def gat_aggregate(graph, h, s, t, heads, alpha, apply_elu=True, mode=0, edge_scale=None, pack_scores=False, dropout_p=0.0,
                  dropout_seed=None):
    """Fused multi-head edge-softmax + aggregation.  h: [N, heads*fo] with fo already padded per `head_width_padded`
    (pow2=False suffices for mode 0 without edge_scale); s, t: [N, heads].  pack_scores: the caller owns the padding behind
    h's rows (h.stride(0) > h.shape[1]) and lets the kernels keep per-node scores there.
    dropout_p in (0, 1) (mode 0 without edge_scale): attention dropout drawn inside the kernels, nothing stored per edge;
    dropout_seed: 2-element int32 tensor on h's device (None: drawn from torch's generator there), kept for the backward.  The mask
    is a function of (seed, row, column, head): duplicate (row, column) entries of an uncoalesced adjacency share a draw."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("gat_aggregate expects a CSRGraph")
    fo = h.shape[1] // heads
    strided = mode == 0 and edge_scale is None
    if fo * heads != h.shape[1] or head_width_padded(fo, h.dtype, pow2=not strided) != fo:
        raise ValueError("per-head width %d is not padded for the kernels (need %d)"
                         % (fo, head_width_padded(fo, h.dtype, pow2=not strided)))
    if strided:
        return _GatAggregateStrided.apply(h, s, t, graph, heads, fo, alpha, apply_elu, pack_scores, dropout_p, dropout_seed)
    if float(dropout_p) != 0.0:
        raise ValueError("dropout_p needs mode 0 without edge_scale (in-kernel dropout is sparseGatConv's form)")
    return _GatAggregate.apply(h, s, t, edge_scale, graph, heads, fo, alpha, apply_elu, mode)


def gat_layer(graph, h, A, heads, alpha, apply_elu=True, pack_scores=False, dropout_p=0.0, dropout_seed=None):
    """sparseGatConv after its transform as one autograd node: h [N, heads*fo] (per-head width a whole number of 16-byte
    vectors), A [heads*fo, 2*heads] = blockdiag(a1_k | a2_k).  GPU, mode 0.  dropout_p / dropout_seed: attention dropout drawn
    inside the kernels, as gat_aggregate's."""
    if not isinstance(graph, CSRGraph):
        raise TypeError("gat_layer expects a CSRGraph")
    fo = h.shape[1] // heads
    if fo * heads != h.shape[1] or head_width_padded(fo, h.dtype, pow2=False) != fo:
        raise ValueError("per-head width %d is not a whole number of 16-byte vectors" % fo)
    return _GatLayerStrided.apply(h, A, graph, heads, fo, alpha, apply_elu, pack_scores, dropout_p, dropout_seed)


# ------------------------------------------------------------------------------------------------ split launches
# Building blocks of the partitioned GAT (dgll_amd/dist.py): the same kernels on the two column-halves of an adjacency.
def gat_fwd_part(graph, h, s_rows, t_cols, out, rowsum, heads, fo, alpha, apply_elu, raw, accumulate):
    """One half of a split forward: rows of `graph` gather from `h` / `t_cols`; numerator into `out`, denominator into
    `rowsum` (raw), optionally on top of what a previous launch left there (accumulate)."""
    _gat_pass(_lib.GAT_FORWARD, graph, heads, fo, float(alpha), h, apply_elu=int(apply_elu), row_score=s_rows.data_ptr(),
              col_score=t_cols.data_ptr(), out=out.data_ptr(), ld_out=out.stride(0), rowsum=rowsum.data_ptr(), raw=int(raw),
              accumulate=int(accumulate))


def gat_bwd_rows_part(graph, h_cols, s_rows, t_cols, out, g, rowsum, dn, dd, grad_s, heads, fo, alpha, apply_elu, accumulate,
                      partial=None):
    """Rows pass over one column half of A.  accumulate: False / 0 = first (or only) launch (writes DN, dd, grad_s; dd_i from the
    stored output row), True / 1 = a further half (grad_s +=), 3 = DECLARED the only launch over these rows: exact dd_i;
    4 / 5 / 6 with `partial` (fp32 [n_rows, 3 * heads], the same buffer every time) = first / middle / last launch of a SPLIT
    exact pass (DGLL_GAT_ROWS_EXACT_FIRST / _MIDDLE / _LAST).  The values are the descriptor's `phase`."""
    split = int(accumulate) >= _lib.GAT_ROWS_EXACT_FIRST
    if split and (partial is None or partial.dtype != torch.float32 or partial.numel() < graph.n_rows * 3 * heads
                  or not partial.is_contiguous()):
        raise ValueError("a split exact rows pass needs a contiguous fp32 [n_rows, 3 * heads] `partial` buffer")
    _gat_pass(_lib.GAT_ROWS, graph, heads, fo, float(alpha), h_cols, apply_elu=int(apply_elu), phase=int(accumulate),
              row_score=s_rows.data_ptr(), col_score=t_cols.data_ptr(), out=out.data_ptr(), ld_out=out.stride(0), grad_out=g.data_ptr(),
              ld_grad_out=g.stride(0), rowsum=rowsum.data_ptr(), dn=dn.data_ptr(), ld_dn=dn.stride(0), dd=dd.data_ptr(),
              grad_score=grad_s.data_ptr(), partial3=partial.data_ptr() if split else None)


def gat_bwd_cols_part(graph_t, dn, h_rows, t_rows, s_cols, dd_cols, grad_h, grad_t, heads, fo, alpha):
    """Pass 2 over a transposed structure `graph_t` (rows = source nodes with features h_rows / scores t_rows, columns =
    destination rows with dn / s_cols / dd_cols)."""
    _gat_pass(_lib.GAT_TRANSPOSED, graph_t, heads, fo, float(alpha), h_rows, dn=dn.data_ptr(), ld_dn=dn.stride(0), row_score=t_rows.data_ptr(),
              col_score=s_cols.data_ptr(), col_dd=dd_cols.data_ptr(), grad_h=grad_h.data_ptr(), ld_grad_h=grad_h.stride(0),
              grad_score=grad_t.data_ptr())
