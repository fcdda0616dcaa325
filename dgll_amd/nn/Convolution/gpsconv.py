"""General, powerful, scalable graph-transformer layer (PyG's GPSConv, Rampasek et al.'s "Recipe for a General, Powerful, Scalable
Graph Transformer": argument names, parameter names and shapes) on the gfx950 engine.

    GPSConv(channels, conv, heads=1, dropout=0.0, act="relu", norm="batch_norm", attn_type="multihead", attn_kwargs=None)

forward(graph, x, segs=None, batch=None, **conv_kwargs) -> [N, channels]: a local message-passing layer and global attention inside
every graph of the batch, side by side, then a feed-forward block:

    h1  = norm1(dropout(conv(graph, x, **conv_kwargs)) + x)                                (skipped when conv is None)
    h2  = norm2(dropout(out_proj(attention(in_proj(x) split in q, k, v))) + x)
    out = h1 + h2;   out = norm3(out + mlp(out));   mlp = Linear(C, 2C), act, Dropout, Linear(2C, C), Dropout

`conv` is any layer of this package called as conv(graph, x, **conv_kwargs); of a layer that returns a tuple (GatedGCNConv returns
node and edge features) the first element is used.  The batch is cut into graphs by `segs` (sizes: no read-back) or `batch` (sorted
graph ids, PyG's batch vector), as in ops_pool; with neither, all rows are one graph.

The attention parameters are those of torch.nn.MultiheadAttention -- attn.in_proj_weight [3C, C], attn.in_proj_bias [3C],
attn.out_proj.weight, attn.out_proj.bias -- and the feed-forward ones mlp.0.* and mlp.3.*, so a PyG state dict loads.  The norms are
torch.nn.BatchNorm1d ("batch_norm"), torch.nn.LayerNorm ("layer_norm") or None, used directly: their keys are norm1.weight, ...
where PyG, which wraps them, has norm1.module.weight; rename those keys when loading a PyG state dict.

On the GPU the projections and the feed-forward products run on the dense transform path (dense.linear) and the attention is ONE
autograd node over three MFMA passes (ops_dense_attn.segment_attention): q, k and v are column slices of the one in_proj output, no
padded [B, max_n, C] batch and no [n, n] array exist.  Heads whose width is not a whole number of 16-byte vectors are padded with
zero rows in the WEIGHTS and unpadded after the attention; the scale stays that of the true head width.  Host tensors take
`_host_attention`, a per-graph torch loop, so that the layer's own logic can be exercised without a GPU; a GPU tensor never reaches
it.

Not built: dropout of the attention probabilities (attn_kwargs={"dropout": p} with p != 0 raises) and attn_type other than
"multihead" (raises).
"""
from ... import backend as F
from ... import ops, ops_dense_attn
from ...ops_pool import segment_sizes
from .gatconv import _unpad_heads
from .gatv2conv import _pad_head_rows
from .pnaconv import _linear

_ACTS = {"relu": F.nn.ReLU, "gelu": F.nn.GELU, "elu": F.nn.ELU, "silu": F.nn.SiLU, "tanh": F.nn.Tanh, "leaky_relu": F.nn.LeakyReLU}
_NORMS = {"batch_norm": F.nn.BatchNorm1d, "layer_norm": F.nn.LayerNorm}


def _host_attention(q, k, v, heads, sizes, scale):
    """[N, heads * D]: softmax(scale q k^T) v inside every segment, graph by graph (host tensors only)"""
    out, at = [], 0
    for n in sizes:
        qs, ks, vs = (t[at:at + n].reshape(n, heads, t.shape[1] // heads).transpose(0, 1) for t in (q, k, v))
        out.append((F.softmax(qs @ ks.transpose(1, 2) * scale, dim=-1) @ vs).transpose(0, 1).reshape(n, q.shape[1]))
        at += n
    return F.cat(out) if out else q[:0]


class _Attention(F.nn.Module):
    """the parameters of torch.nn.MultiheadAttention(channels, heads), under its names and with its initialisation"""

    def __init__(self, channels):
        super().__init__()
        self.in_proj_weight = F.nn.Parameter(F.empty(3 * channels, channels))
        self.in_proj_bias = F.nn.Parameter(F.zeros(3 * channels))
        self.out_proj = F.nn.Linear(channels, channels)
        self.reset_parameters()

    def reset_parameters(self):
        F.nn.init.xavier_uniform_(self.in_proj_weight)
        F.nn.init.zeros_(self.in_proj_bias)
        self.out_proj.reset_parameters()
        F.nn.init.zeros_(self.out_proj.bias)


class GPSConv(F.nn.Module):
    """PyG's GPSConv.  forward(graph, x, segs=None, batch=None, **conv_kwargs) -> [N, channels]."""

    def __init__(self, channels, conv, heads=1, dropout=0.0, act="relu", norm="batch_norm", attn_type="multihead", attn_kwargs=None):
        super().__init__()
        if attn_type != "multihead":
            raise ValueError("GPSConv: attn_type=%r is not built (only 'multihead': dense attention inside every graph)" % (attn_type,))
        attn_kwargs = dict(attn_kwargs or {})
        if float(attn_kwargs.pop("dropout", 0.0)) != 0.0:
            raise ValueError("GPSConv: dropout of the attention probabilities is not built (attn_kwargs['dropout'] must be 0.0)")
        if attn_kwargs:
            raise ValueError("GPSConv: attn_kwargs %s are not built" % sorted(attn_kwargs))
        if int(heads) < 1 or channels % int(heads):
            raise ValueError("GPSConv: heads = %r does not divide the %d channels" % (heads, channels))
        if act not in _ACTS or not (norm is None or norm in _NORMS):
            raise ValueError("GPSConv: act must be one of %s and norm one of %s or None" % (sorted(_ACTS), sorted(_NORMS)))
        self.channels, self.conv, self.heads, self.dropout, self.attn_type = channels, conv, int(heads), float(dropout), attn_type
        self.attn = _Attention(channels)
        self.mlp = F.nn.Sequential(F.nn.Linear(channels, 2 * channels), _ACTS[act](), F.nn.Dropout(dropout),
                                   F.nn.Linear(2 * channels, channels), F.nn.Dropout(dropout))
        self.norm1, self.norm2, self.norm3 = (None if norm is None else _NORMS[norm](channels) for _ in range(3))

    def reset_parameters(self):
        if self.conv is not None and hasattr(self.conv, "reset_parameters"):
            self.conv.reset_parameters()
        self.attn.reset_parameters()
        for m in (self.mlp[0], self.mlp[3], self.norm1, self.norm2, self.norm3):
            if m is not None:
                m.reset_parameters()

    def _attention(self, x, sizes):
        heads, fo = self.heads, self.channels // self.heads
        fo_pad = ops.head_width_padded(fo, x.dtype, pow2=False) if x.is_cuda else fo
        scale = float(fo) ** -0.5                   # of the true head width: the padding columns are zeros and add nothing to <q, k>
        a = self.attn
        qkv = _linear(x, _pad_head_rows(a.in_proj_weight, 3 * heads, fo, fo_pad), _pad_head_rows(a.in_proj_bias, 3 * heads, fo, fo_pad))
        q, k, v = qkv.split(heads * fo_pad, dim=1)
        if x.is_cuda:
            out = _unpad_heads(ops_dense_attn.segment_attention(q, k, v, heads, segs=sizes, scale=scale), heads, fo, fo_pad)
        else:
            out = _host_attention(q, k, v, heads, sizes, scale)
        return _linear(out, a.out_proj.weight, a.out_proj.bias)

    def forward(self, graph, x, segs=None, batch=None, **conv_kwargs):
        sizes = segment_sizes("GPSConv", x.shape[0], segs, batch)
        drop = lambda t: F.dropout(t, p=self.dropout, training=self.training)      # noqa: E731
        norm = lambda m, t: t if m is None else m(t)                                # noqa: E731
        hs = []
        if self.conv is not None:
            h = self.conv(graph, x, **conv_kwargs)
            h = h[0] if isinstance(h, (tuple, list)) else h
            hs.append(norm(self.norm1, drop(h) + x))
        hs.append(norm(self.norm2, drop(self._attention(x, sizes)) + x))
        out = sum(hs)
        h = out
        for m in self.mlp:
            h = _linear(h, m.weight, m.bias) if isinstance(m, F.nn.Linear) else m(h)
        return norm(self.norm3, out + h)

    def extra_repr(self):
        return "%d, heads=%d, attn_type=%s" % (self.channels, self.heads, self.attn_type)
