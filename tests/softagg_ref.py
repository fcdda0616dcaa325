"""The oracle of the soft-aggregation tests: dgll_amd.ops_softagg restated in float64, row by row and entry by entry, with the
formulas of the issue written out (no autograd): both modes, with and without e.

    reference(rowptr, col, x, e, theta, go, mode, eps=1e-7, semi_grad=False) -> dict
        out [n_dst, F], grad_x [n_src, F], grad_e [nnz, F] (None without e), grad_theta (a float; None with semi_grad) and
        scale = sum |g_ic * d out_ic / d theta|, the size the error of grad_theta is judged on (the gradient itself is ONE sum over the
        whole graph and may cancel)

    m_k = relu(x[j] + e[k]) + eps        gate_k = (x[j] + e[k] > 0)
    softmax:     a_k = softmax_k(t m_k)   out = sum a m        dout/dm = a (1 + t (m - out))  (semi_grad: a)   dout/dt = sum a m^2 - out^2
    power-mean:  mc = min(m, 100)   S = sum mc^p   out = (S / deg)^(1/p)   dout/dm = out^(1-p) mc^(p-1) / deg  (0 where m > 100)
                 dout/dp = (out / p) (sum mc^p ln mc / S - ln out)

composition(...) is the same forward written with torch's index ops for autograd (test_soft_agg_host.py holds one against the other).
No element is excluded anywhere: the gate is a comparison of the exact sum of two stored values, and the fp32 sum of two fp32 values
has the sign of the exact sum.
"""
import torch

MODES = ("softmax", "power")


def reference(rowptr, col, x, e, theta, go, mode, eps=1e-7, semi_grad=False):
    assert mode in MODES
    x, go = x.double(), go.double()
    e = None if e is None else e.double()
    th = float(theta)
    n_dst, F = go.shape
    rp, col = rowptr.tolist(), col.long()
    out = torch.zeros(n_dst, F, dtype=torch.float64)
    gx = torch.zeros_like(x)
    ge = None if e is None else torch.zeros_like(e)
    gth, scale = 0.0, 0.0
    for i in range(n_dst):
        b, en = rp[i], rp[i + 1]
        if en == b:
            continue
        idx = col[b:en]
        s = x[idx] if e is None else x[idx] + e[b:en]
        gate = (s > 0).double()
        m = torch.relu(s) + eps
        g = go[i]
        if mode == "softmax":
            a = torch.softmax(th * m, 0)
            o = (a * m).sum(0)
            dm = a if semi_grad else a * (1 + th * (m - o))
            dth = (a * (m - o) ** 2).sum(0)         # = sum a m^2 - out^2 (sum a = 1), without the cancellation
        else:
            deg = en - b
            mc = m.clamp(max=100.0)
            S = (mc ** th).sum(0)
            o = (S / deg) ** (1.0 / th)
            dm = o ** (1 - th) * mc ** (th - 1) / deg * (m <= 100.0).double()
            dth = (o / th) * ((mc ** th * mc.log()).sum(0) / S - o.log())
        out[i] = o
        t = g * dm * gate
        gx.index_add_(0, idx, t)
        if ge is not None:
            ge[b:en] = t
        gth += float((g * dth).sum())
        scale += float((g * dth).abs().sum())
    none = mode == "softmax" and semi_grad
    return {"out": out, "grad_x": gx, "grad_e": ge, "grad_theta": None if none else gth, "scale": scale}


def composition(rowptr, col, x, e, theta, mode, eps=1e-7, semi_grad=False):
    """out [n_dst, F] from per-edge tensors and scatter ops, differentiable in x, e and theta (a tensor)."""
    n_dst = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n_dst), deg)
    s = x[col.long()] if e is None else x[col.long()] + e
    m = torch.relu(s) + eps
    F = m.shape[1]
    index = row.unsqueeze(1).expand(-1, F)
    zeros = torch.zeros(n_dst, F, dtype=m.dtype)
    if mode == "softmax":
        z = theta * m
        if semi_grad:
            z = z.detach()
        top = torch.full((n_dst, F), -float("inf"), dtype=m.dtype).scatter_reduce(0, index, z.detach(), "amax", include_self=True)
        w = torch.exp(z - top[row])
        a = w / zeros.index_add(0, row, w)[row]
        return zeros.index_add(0, row, a * m)
    mc = m.clamp(max=100.0)
    mean = zeros.index_add(0, row, mc ** theta) / deg.clamp(min=1).to(m.dtype).unsqueeze(1)
    live = (deg > 0).unsqueeze(1)
    return torch.where(live, torch.where(live, mean, torch.ones_like(mean)) ** (1.0 / theta), zeros)
