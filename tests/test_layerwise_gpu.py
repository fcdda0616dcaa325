"""Layer-wise samplers (LADIES / FastGCN) on the MI355X: stage parity with the reference's fixtures, the selection's distribution,
determinism, edge cases, training numerics on the blocks, convergence and the mini-batch pipeline."""
import glob
import itertools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import layerwise_ref as ref
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

FIXTURES = sorted(os.path.basename(p)[len("layerwise_"):-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "layerwise_*.npz")))


def load(name):
    d = np.load(os.path.join(GOLDEN_DIR, "layerwise_%s.npz" % name), allow_pickle=False)
    return {k: d[k] for k in d.files if k != "meta"}, json.loads(str(d["meta"]))


def make_sampler(meta, fanouts, g):
    from dgll_amd.sampling import layerwise as lw

    return getattr(lw, meta["class"])(list(fanouts), g, **meta["kwargs"])


def csr_graph(indptr, indices, n, device):
    from dgll_amd.graph import CSRGraph

    return CSRGraph(torch.as_tensor(np.asarray(indptr, np.int64)), torch.as_tensor(np.asarray(indices, np.int32)), None, n, n).to(device)


def lap_numpy(s):
    L = s.lap
    return sp.csr_matrix((L.val.double().cpu().numpy(), L.col.cpu().numpy(), L.rowptr.cpu().numpy()), shape=(L.n_rows, L.n_cols))


def random_graph(n, deg, seed, device, isolated=()):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n * deg)
    dst = np.minimum((src + rng.zipf(1.6, n * deg)) % n, n - 1)
    keep = (src != dst) & ~np.isin(src, isolated) & ~np.isin(dst, isolated)
    A = sp.csr_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), shape=(n, n))
    A.data[:] = 1.0
    A.sort_indices()
    return A, csr_graph(A.indptr, A.indices, n, device)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---- stage parity with the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_stages_match_the_reference(name, cuda_device):
    from dgll_amd.sampling import layerwise as lw

    fx, meta = load(name)
    n = int(fx["n"])
    s = make_sampler(meta, fx["fanouts"], csr_graph(fx["a_indptr"], fx["a_indices"], n, cuda_device))
    flat = bool(meta["kwargs"].get("flat", False))
    fastgcn = meta["class"].startswith("FastGCN")
    wrs = not fastgcn or bool(meta["kwargs"].get("wrs", False))
    dev = lambda a: torch.as_tensor(np.asarray(a, np.int64)).to(cuda_device)      # noqa: E731
    for l in range(meta["layers"]):
        k = lambda t: fx["l%d_%s" % (l, t)]      # noqa: E731
        rows = dev(k("rows"))
        if fastgcn:
            mass = s.global_mass
            p = s.p_global().cpu().numpy()
        else:
            mass = lw.column_mass(s.lap, rows, flat=flat, ws=s.ws)
            p = mass.p_dense().cpu().numpy()
        np.testing.assert_allclose(p, k("p"), rtol=1e-5, atol=0)
        cols = k("cols")
        if wrs:
            w = lw.wrs_weights(mass.p_of(dev(k("draw"))), n)
        else:
            w = lw.inverse_weights(mass.p_of(dev(cols)), int(k("s")))
        np.testing.assert_allclose(w.cpu().numpy(), k("w"), rtol=1e-5)
        blk, m, _ = lw.extract_block(s.lap, rows, dev(cols), torch.as_tensor(k("w")).to(cuda_device), ws=s.ws, sorted_cols=meta["union"])
        torch.cuda.synchronize()
        assert blk.n_rows == len(k("rows")) and blk.n_cols == m == len(cols)
        assert np.array_equal(blk.rowptr.cpu().numpy(), k("indptr"))
        ri, rv = ref.sorted_within_rows(k("indptr"), k("indices"), k("values"))
        assert np.array_equal(blk.col.cpu().numpy(), ri)
        np.testing.assert_allclose(blk.val.cpu().numpy(), rv, rtol=1e-5)
    if fastgcn:   # fix (b): our layer-2 rows are the global ids of the sampled set (the reference used local ids)
        torch.manual_seed(0)
        batch = fx["batch"]
        _, _, blocks = s.sample_seeded(None, batch, 5)
        nodes0 = s.last_nodes[0].cpu().numpy()
        assert blocks[0].n_rows == len(nodes0) and blocks[-1].n_rows == len(batch)
        if meta["union"]:
            assert set(batch.tolist()) <= set(nodes0.tolist()) and np.all(np.diff(nodes0) > 0)
        assert not np.array_equal(nodes0, np.arange(len(nodes0)))
        check_blocks(s, batch, blocks)


def check_blocks(s, batch, blocks, input_nodes=None):
    """Every block equals the float64 restatement of L[R][:, C] * w for the sampler's own node sets (p, weights recomputed)."""
    L = lap_numpy(s)
    n = L.shape[0]
    rows = np.asarray(batch, np.int64)
    if s.per_batch:
        p_global = None
    else:
        p_global = ref.column_p(L, None, s.flat)
    assert len(blocks) == s.layers and blocks[-1].n_rows == len(rows)
    for l, cols_t in enumerate(s.last_nodes):
        cols = cols_t.cpu().numpy()
        blk = blocks[s.layers - 1 - l]
        p = p_global if p_global is not None else ref.column_p(L, rows, s.flat)
        s_num = int(min(np.sum(p > 0), s.fanouts[l]))
        if s.union:
            assert len(cols) >= s_num
        else:
            assert len(cols) == s_num and len(set(cols.tolist())) == s_num and np.all(p[cols] > 0)
        w = ref.wrs_weights(p[cols], n) if s.weights == "wrs" else ref.inverse_weights(p[cols], s_num)
        indptr, indices, values = ref.block(L, rows, cols, w)
        assert blk.n_rows == len(rows) and blk.n_cols == len(cols)
        assert np.array_equal(blk.rowptr.cpu().numpy(), indptr)
        assert np.array_equal(blk.col.cpu().numpy(), indices)
        np.testing.assert_allclose(blk.val.cpu().numpy(), values, rtol=1e-5)
        rows = cols
    if input_nodes is not None:
        assert np.array_equal(input_nodes.cpu().numpy(), rows)


# ---- selection ---------------------------------------------------------------------------------------------------------------
def test_selection_follows_plackett_luce(cuda_device):
    from scipy import stats

    from dgll_amd.sampling import layerwise as lw

    p = np.array([0.38, 0.24, 0.16, 0.11, 0.07, 0.04])
    mass = lw.mass_from_p(torch.tensor(p, device=cuda_device))
    trials = 20000
    draws = torch.stack([lw.select(mass, 3, seed)[0] for seed in range(trials)]).cpu().numpy()
    counts = {}
    for t in map(tuple, draws):
        counts[t] = counts.get(t, 0) + 1
    exp, obs = [], []
    for t in itertools.permutations(range(6), 3):
        q = p[t[0]] * p[t[1]] / (1 - p[t[0]]) * p[t[2]] / (1 - p[t[0]] - p[t[1]])
        exp.append(q * trials)
        obs.append(counts.get(t, 0))
    assert sum(obs) == trials                    # every draw is an ordered triple of distinct candidates
    exp, obs = np.array(exp), np.array(obs)
    big = exp >= 5
    e, o = exp[big], obs[big]
    if (~big).any():                             # rare triples pooled into one bin
        e, o = np.append(e, exp[~big].sum()), np.append(o, obs[~big].sum())
    chi2 = float(((o - e) ** 2 / e).sum())
    assert chi2 < stats.chi2.ppf(0.9999, len(e) - 1), chi2
    incl = np.zeros(6)
    for t in itertools.permutations(range(6), 3):
        q = p[t[0]] * p[t[1]] / (1 - p[t[0]]) * p[t[2]] / (1 - p[t[0]] - p[t[1]])
        incl[list(t)] += q
    got = np.bincount(draws.reshape(-1), minlength=6)
    chi2_i = float((((got - incl * trials) ** 2) / (incl * trials * (1 - incl))).sum())
    assert chi2_i < stats.chi2.ppf(0.9999, 6), chi2_i
    # s = number of candidates: every candidate, once; a fan-out above it is capped
    for f in (6, 9):
        ids, info = lw.select(mass, f, 123)
        assert int(info[1]) == 6 and sorted(ids[:6].cpu().tolist()) == list(range(6))


# ---- determinism ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def medium(cuda_device):
    A, g = random_graph(6000, 8, 3, cuda_device, isolated=(17,))
    return A, g


def same(a, b):
    inp_a, _, blk_a = a
    inp_b, _, blk_b = b
    return torch.equal(inp_a, inp_b) and all(torch.equal(x.rowptr, y.rowptr) and torch.equal(x.col, y.col) and
                                             torch.equal(x.val, y.val) for x, y in zip(blk_a, blk_b))


@pytest.mark.parametrize("cls", ["Ladies", "FastGCNSampler", "FastGCNSamplerFlat"])
def test_same_seed_same_sample(cls, medium, cuda_device):
    from dgll_amd.sampling import layerwise as lw

    A, g = medium
    batch = np.arange(100, 1123)
    s1, s2 = getattr(lw, cls)([512, 1024], g), getattr(lw, cls)([512, 1024], g)
    a = s1.sample_seeded(None, batch, 77)
    check_blocks(s1, batch, a[2], a[0])
    assert same(a, s1.sample_seeded(None, batch, 77)) and same(a, s2.sample_seeded(None, batch, 77))
    assert not torch.equal(a[0], s1.sample_seeded(None, batch, 78)[0])
    np.random.seed(4)
    seq = [s1.sample(None, batch) for _ in range(3)]
    np.random.seed(4)
    assert all(same(x, s2.sample(None, batch)) for x in seq)
    assert not same(seq[0], seq[1])


# ---- edge cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Ladies", "LadiesFlatWrs", "FastGCNSampler", "FastGCNSamplerFlat"])
@pytest.mark.parametrize("batch", [[17], [5999], [0], [17, 5999, 1, 2, 3]], ids=["isolated", "last", "one", "mixed"])
def test_edge_cases(cls, batch, medium, cuda_device):
    from dgll_amd.sampling import layerwise as lw

    A, g = medium
    kw = {"flat": True} if cls == "LadiesFlatWrs" else {}
    s = getattr(lw, cls)([4096, 7], g, **kw)              # a fan-out above the candidates, then a small one
    inp, out, blocks = s.sample_seeded(None, np.array(batch), 9)
    check_blocks(s, batch, blocks, inp)
    if cls.startswith("Ladies"):
        L = lap_numpy(s)
        assert blocks[-1].n_cols == len(np.unique(L[np.array(batch)].indices))      # every candidate drawn


def test_empty_rows_give_bias_only(medium, cuda_device):
    from dgll_amd.nn import gcnConv
    from dgll_amd.sampling import FastGCNSamplerFlat, layerwise

    A, g = medium
    s = FastGCNSamplerFlat([3, 3], g)                   # no union with the batch: most batch rows keep nothing
    batch = np.arange(200, 264)
    inp, _, blocks = s.sample_seeded(None, batch, 1)
    layerwise.record_stream(blocks, inp, torch.cuda.current_stream(cuda_device))
    check_blocks(s, batch, blocks, inp)
    deg = (blocks[-1].rowptr[1:] - blocks[-1].rowptr[:-1]).cpu()
    assert (deg == 0).any()
    conv = gcnConv(5, 4).to(cuda_device)
    y = conv(torch.randn(blocks[-1].n_cols, 5, device=cuda_device), blocks[-1])
    empty = torch.nonzero(deg == 0).flatten()
    assert torch.equal(y[empty.to(cuda_device)], conv.bias.detach().expand(len(empty), 4))


# ---- training on blocks ------------------------------------------------------------------------------------------------------
class Model(torch.nn.Module):
    """The reference's Model (MQLadies.py:48-60): two GCN layers, hidden 128, ReLU between them."""

    def __init__(self, fin, hid, ncls):
        super().__init__()
        from dgll_amd.nn import gcnConv

        self.conv1, self.conv2 = gcnConv(fin, hid), gcnConv(hid, ncls)

    def forward(self, blocks, x):
        return self.conv2(torch.relu(self.conv1(x, blocks[0])), blocks[1])


@pytest.mark.parametrize("cls", ["Ladies", "FastGCNSampler"])
def test_one_batch_matches_float64_autograd(cls, medium, cuda_device):
    from dgll_amd import ops
    from dgll_amd.sampling import layerwise as lw

    A, g = medium
    torch.manual_seed(0)
    s = getattr(lw, cls)([512, 1024], g)
    inp, _, blocks = s.sample_seeded(None, np.arange(0, 1023), 21)
    lw.record_stream(blocks, inp, torch.cuda.current_stream(cuda_device))
    x_all = torch.randn(6000, 50)
    labels = torch.randint(0, 7, (1023,))
    model = Model(50, 128, 7).to(cuda_device)
    logits = model(blocks, x_all[inp.cpu()].to(cuda_device))
    loss = ops.cross_entropy(logits, labels.to(cuda_device))
    loss.backward()
    # float64 on the CPU, same blocks and parameters
    dense = lambda b: torch.sparse_csr_tensor(b.rowptr.cpu(), b.col.long().cpu(), b.val.double().cpu(), (b.n_rows, b.n_cols)).to_dense()   # noqa: E731
    B0, B1 = dense(blocks[0]), dense(blocks[1])
    P = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    x = x_all[inp.cpu()].double()
    h = torch.relu(B0 @ (x @ P["conv1.weight"]) + P["conv1.bias"])
    z = B1 @ (h @ P["conv2.weight"]) + P["conv2.bias"]
    torch.nn.functional.cross_entropy(z, labels).backward()
    assert rel(logits.detach().cpu(), z.detach()) < 1e-4
    for k, prm in model.named_parameters():
        assert rel(prm.grad.cpu(), P[k].grad) < 1e-4, k


def planted_partition(n, classes, seed, device):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % classes
    src, dst = [], []
    for v in range(n):
        same_cls = np.nonzero(y == y[v])[0]
        src += [v] * 10
        dst += rng.choice(same_cls, 8).tolist() + rng.integers(0, n, 2).tolist()
    src, dst = np.array(src), np.array(dst)
    keep = src != dst
    A = sp.csr_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), shape=(n, n))
    A = ((A + A.T) > 0).astype(np.float64).tocsr()
    A.sort_indices()
    centers = rng.normal(size=(classes, 16))
    x = centers[y] + 2.5 * rng.normal(size=(n, 16))
    return A, csr_graph(A.indptr, A.indices, n, device), torch.tensor(x, dtype=torch.float32), torch.tensor(y)


@pytest.mark.parametrize("cls", ["Ladies", "FastGCNSampler"])
def test_training_converges(cls, cuda_device):
    from dgll_amd import ops
    from dgll_amd.sampling import layerwise as lw

    n = 2000
    A, g, x, y = planted_partition(n, 4, 0, cuda_device)
    torch.manual_seed(1)
    np.random.seed(1)
    s = getattr(lw, cls)([256, 512], g)
    model = Model(16, 128, 4).to(cuda_device)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    xd, yd = x.to(cuda_device), y.to(cuda_device)
    for step in range(60):
        batch = np.random.choice(n, 256, replace=False)
        inp, _, blocks = s.sample(None, batch)
        lw.record_stream(blocks, inp, torch.cuda.current_stream(cuda_device))     # consumed on this stream
        loss = ops.cross_entropy(model(blocks, xd[inp]), yd[torch.as_tensor(batch, device=cuda_device)])
        opt.zero_grad()
        loss.backward()
        opt.step()
    correct = 0
    with torch.no_grad():
        for i in range(0, n, 500):
            batch = np.arange(i, min(i + 500, n))
            inp, _, blocks = s.sample(None, batch)
            lw.record_stream(blocks, inp, torch.cuda.current_stream(cuda_device))
            correct += int((model(blocks, xd[inp]).argmax(1).cpu() == y[batch]).sum())
    assert correct / n >= 0.8, correct / n


# ---- pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Ladies", "FastGCNSampler"])
def test_pipeline_equals_serial_sampling(cls, cuda_device):
    from dgll_amd import ops
    from dgll_amd.cache import GraphCacheServer
    from dgll_amd.data import DGraph
    from dgll_amd.dataloader import DataLoader
    from dgll_amd.pipeline import MiniBatchPipeline
    from dgll_amd.sampling import layerwise as lw

    n = 2000
    A, g, x, y = planted_partition(n, 4, 2, cuda_device)
    dg = DGraph.from_csr(A.indptr.astype(np.int64), A.indices.astype(np.int64), labels=y, features=x)
    s = getattr(lw, cls)([128, 256], dg)
    srv = GraphCacheServer(x, gpuid=0)
    srv.auto_cache(torch.as_tensor(np.diff(A.indptr)), capacity=700)
    train = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:900]
    torch.manual_seed(3)
    model = Model(16, 32, 4).to(cuda_device)
    for epoch in range(2):
        np.random.seed(10 + epoch)
        serial = [s.sample(dg, train[i:i + 300]) for i in range(0, len(train), 300)]
        np.random.seed(10 + epoch)
        loader = DataLoader(dg, train, s, batch_size=300)
        pipe = MiniBatchPipeline(loader, cache=srv, labels=y, queue_size=2, device=cuda_device)
        got = 0
        cur = torch.cuda.current_stream(cuda_device)
        for b, ref_item in zip(pipe, serial):
            lw.record_stream(b.subgraphs, b.input_nodes, cur)
            assert same((b.input_nodes, None, b.subgraphs), ref_item)
            feats = b.features[0]
            assert torch.equal(feats.cpu(), x[b.input_nodes.cpu()])
            with torch.no_grad():
                l_pipe = ops.cross_entropy(model(b.subgraphs, feats.contiguous()), b.labels)
                l_ser = ops.cross_entropy(model(ref_item[2], x[ref_item[0].cpu()].to(cuda_device)), y[ref_item[1]].to(cuda_device))
            assert torch.equal(l_pipe, l_ser)
            got += 1
        assert got == len(serial) == 3
