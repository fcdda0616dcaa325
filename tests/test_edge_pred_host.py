"""Edge-prediction sampler, host side: the numpy restatement (tests/edge_pred_ref.py) maps entries to pairs, draws uniform negatives,
filters existing edges and excludes seed edges as documented; the C ABI and the Python front end refuse bad arguments without a GPU."""
import numpy as np
import pytest
import torch

import edge_pred_ref as ref

STAT_SEED = 20240607


def gap_graph():
    """9 nodes; rows 0-1 empty, row 2 = [5, 7], rows 3-5 empty, row 6 = [0, 2, 8], rows 7-8 empty."""
    rowptr = np.asarray([0, 0, 0, 2, 2, 2, 2, 5, 5, 5], np.int64)
    return rowptr, np.asarray([5, 7, 0, 2, 8], np.int32), 9


def test_exact_cases():
    rowptr, col, n = gap_graph()
    nnz = len(col)
    assert [ref.row_of(rowptr, e) for e in range(nnz)] == [2, 2, 6, 6, 6]        # empty runs in front, between and behind
    g, capped = ref.pairs_and_negatives(rowptr, col, n, [0, nnz - 1, 2], 0, 5)   # K = 0; entry 0 and entry nnz - 1
    assert g.tolist() == [[5, 2], [8, 6], [0, 6]] and not capped.any()
    out, pairs = ref.compact(g)
    assert out.tolist() == [0, 2, 5, 6, 8] and pairs.tolist() == [[2, 1], [4, 3], [0, 3]] and pairs.dtype == np.int32
    g1, _ = ref.pairs_and_negatives(rowptr, col, n, [3], 4, 5)                   # B = 1
    assert g1.shape == (5, 2) and g1[0].tolist() == [2, 6] and (g1[1:, 0] == 2).all() and (0 <= g1[1:, 1]).all() and (g1[1:, 1] < n).all()
    g2, _ = ref.pairs_and_negatives(rowptr, col, n, [3, 1, 3], 4, 5)             # the same edge twice: identical negatives,
    assert np.array_equal(g2[3:7], g2[11:15]) and np.array_equal(g2[3:7], g1[1:])  # and the same as alone (batch independence)
    # a changed seed or k changes the draw (N large enough that equal candidates are no accident)
    big = 1 << 30
    draws = {(s, k): ref.negative(rowptr, col, big, 4, k, s)[0] for s in (5, 6) for k in (0, 1)}
    assert len(set(draws.values())) == 4
    assert ref.negative(rowptr, col, big, 4, 1, 5) == ref.negative(rowptr, col, big, 4, 1, 5)
    # the counter domain: word 2 of the negatives' counter is neither a layer nor layer | 2^31
    assert ref.NEG_DOMAIN & 0x80000000 == 0 and ref.NEG_DOMAIN > 64
    with pytest.raises(AssertionError):
        ref.pairs_and_negatives(rowptr, col, n, [nnz], 1, 5)


def test_unfiltered_negatives_are_uniform():
    """N = 12, 4096 positives with K = 1: candidate counts against 4096 / 12, Pearson statistic below the chi-square 0.999 quantile at
    11 degrees of freedom (31.26), the bar of test_neighbor_host.py."""
    n = 12
    rowptr = np.arange(n + 1, dtype=np.int64) * 342
    rowptr[-1] = 4096                                                           # 11 rows of 342 and one of 334
    col = (np.arange(4096) % n).astype(np.int32)
    g, capped = ref.pairs_and_negatives(rowptr, col, n, np.arange(4096), 1, STAT_SEED)
    assert not capped.any() and np.array_equal(g[4096:, 0], col)
    counts = np.bincount(g[4096:, 1], minlength=n)
    exp = 4096 / n
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print("pearson", chi2, "counts", counts)
    assert chi2 < 31.26, chi2


def test_filter_existing_rejects_and_caps():
    """Node N - 1 is a source of 13 rows in 16, so a negative of an edge N - 1 -> v is rejected with probability ~13/16 per attempt:
    (13/16)^16 ~ 3.6 % of the draws run out of 16 attempts; none runs out of 1024."""
    rowptr, col, n = ref.build_graph(1003, hub=500, hub_degree=1000, seed=5)
    eids = np.nonzero(col == n - 1)[0][:300]
    assert len(eids) == 300
    g, capped = ref.pairs_and_negatives(rowptr, col, n, eids, 1, 11, filter_existing=True, max_attempts=16)
    print("capped", int(capped.sum()), "of 300")
    assert 1 <= capped.sum() <= 40 and not capped[:300].any()
    for (u, c), cap in zip(g[300:], capped[300:]):
        assert u == n - 1 and ref.has_edge(rowptr, col, u, c) == bool(cap)
    g2, capped2 = ref.pairs_and_negatives(rowptr, col, n, eids, 1, 11, filter_existing=True, max_attempts=1024)
    assert not capped2.any() and not any(ref.has_edge(rowptr, col, int(u), int(c)) for u, c in g2[300:])
    keep = ~capped[300:]
    assert np.array_equal(g[300:][keep], g2[300:][keep])                        # more attempts change only the capped draws
    g0, capped0 = ref.pairs_and_negatives(rowptr, col, n, eids, 1, 11, filter_existing=False)
    assert not capped0.any() and any(ref.has_edge(rowptr, col, int(u), int(c)) for u, c in g0[300:])
    out, pairs = ref.compact(g)
    ref.check_invariants(rowptr, col, n, out, pairs, 300, [], filter_existing=True, capped_flags=capped)


def hand_block():
    """6 nodes; destinations 10, 11, 12, sources 10, 11, 12, 20, 21, 22.  Row 10 <- {11, 20, 20 (parallel), 21}, row 11 <- {10},
    row 12 <- {10, 22}."""
    src = np.asarray([10, 11, 12, 20, 21, 22], np.int64)
    col = np.asarray([1, 3, 3, 4, 0, 0, 5], np.int32)
    val = np.asarray([0.25] * 4 + [1.0] + [0.5] * 2, np.float32)
    return {"rowptr": np.asarray([0, 4, 5, 7], np.int64), "col": col, "val": val, "n_rows": 3, "n_cols": 6, "src": src, "dst": src[:3]}


def test_exclusion_on_a_hand_written_block():
    blk = hand_block()
    positives = [(20, 10), (11, 10), (12, 22)]          # 20 -> 10 (parallel entries), 11 -> 10 (its reverse 10 -> 11 is row 11), 12 -> 22
    assert ref.exclude(blk, positives, None) is blk
    s = ref.exclude(blk, positives, "self")
    assert s["rowptr"].tolist() == [0, 1, 2, 4] and s["col"].tolist() == [4, 0, 0, 5]
    assert s["val"].view(np.uint32).tolist() == np.asarray([1.0, 1.0, 0.5, 0.5], np.float32).view(np.uint32).tolist()   # a val recomputed
    r = ref.exclude(blk, positives, "reverse")
    assert r["rowptr"].tolist() == [0, 1, 1, 2] and r["col"].tolist() == [4, 0]                 # row 11 emptied, 22 -> 12 gone too
    assert r["val"].tolist() == [1.0, 1.0]
    for out in (s, r):
        assert (out["n_rows"], out["n_cols"]) == (3, 6) and out["src"] is blk["src"]            # shapes and sources unchanged
    third = ref.exclude(blk, [(21, 10)], "self")
    assert third["val"][:3].view(np.uint32).tolist() == [int((np.float32(1) / np.float32(3)).view(np.uint32))] * 3
    assert ref.exclude(blk, positives, "self", norm=None)["val"] is None
    rp, pair, other = ref.incidence(np.asarray([[0, 1], [2, 2], [1, 0]], np.int32), 4)          # (i, i) twice; node 3 in no pair
    assert rp.tolist() == [0, 2, 4, 6, 6] and pair.tolist() == [0, 2, 0, 2, 1, 1] and other.tolist() == [1, 1, 0, 0, 2, 2]


def test_c_abi_argument_validation_needs_no_gpu():
    from dgll_amd import _lib

    lib = _lib.lib
    p = 16                     # any non-NULL, 16-byte aligned address: the checks fail before anything is touched

    def bad(code, text):
        assert code == -1 and text in _lib.last_error(), (code, _lib.last_error())

    # draw(stream, rowptr, col, n_total, nnz, edge_ids, n_edges, negatives, filter, max_attempts, seed, mark, epoch, bitmap, prefix, pairs, cap, info)
    bad(lib.dgll_hip_ep_draw(None, None, p, 10, 20, p, 4, 2, 0, 16, 1, p, 1, p, p, p, 12, p), "non-NULL")
    bad(lib.dgll_hip_ep_draw(None, p, p, 10, 20, p, 4, 2, 0, 16, 1, p, 1, p, p, None, 12, p), "non-NULL")
    bad(lib.dgll_hip_ep_draw(None, p, p, 2 ** 31, 20, p, 4, 2, 0, 16, 1, p, 1, p, p, p, 12, p), "node count")
    bad(lib.dgll_hip_ep_draw(None, p, p, 10, 20, p, 4, -1, 0, 16, 1, p, 1, p, p, p, 12, p), "negatives")
    bad(lib.dgll_hip_ep_draw(None, p, p, 10, 20, p, 4, 2, 1, 0, 1, p, 1, p, p, p, 12, p), "max_attempts")
    bad(lib.dgll_hip_ep_draw(None, p, p, 10, 20, p, 4, 2, 0, 16, 1, p, 0, p, p, p, 12, p), "epoch")
    bad(lib.dgll_hip_ep_draw(None, p, p, 10, 20, p, 4, 2, 0, 16, 1, p, 1, p, p, p, 11, p), "pairs buffer")
    # compact(stream, n_total, bitmap, prefix, n_nodes, pairs, n_pairs, output_nodes, local_pairs)
    bad(lib.dgll_hip_ep_compact(None, 10, p, p, 3, p, 12, None, p), "non-NULL")
    bad(lib.dgll_hip_ep_compact(None, 2 ** 31, p, p, 3, p, 12, p, p), "node count")
    bad(lib.dgll_hip_ep_compact(None, 10, p, p, 11, p, 12, p, p), "unique nodes")
    # exclude_count(stream, rowptr, col, n_rows, nnz, src_nodes, n_cols, n_total, keys, n_keys, out_rowptr, info)
    bad(lib.dgll_hip_ep_exclude_count(None, p, p, 3, 7, None, 6, 10, p, 2, p, p), "non-NULL")
    bad(lib.dgll_hip_ep_exclude_count(None, p, p, 3, 7, p, 6, 2 ** 31, p, 2, p, p), "node count")
    bad(lib.dgll_hip_ep_exclude_count(None, p, p, 7, 7, p, 6, 10, p, 2, p, p), "block rows")
    bad(lib.dgll_hip_ep_exclude_count(None, p, p, 3, 7, p, 6, 10, p, 2, p, None), "info")
    bad(lib.dgll_hip_ep_exclude_fill(None, p, p, 3, 7, p, 6, 10, p, 2, None, 4, p, p), "non-NULL")
    bad(lib.dgll_hip_ep_exclude_fill(None, p, p, 3, 7, p, 6, 10, p, 2, p, 8, p, p), "kept entries")
    bad(lib.dgll_hip_ep_exclude_fill(None, p, p, 3, 7, p, 6, 10, p, 2, p, 4, None, p), "column output")
    # pair_dot(stream, h, ldh, n_nodes, feat, dtype, pairs, n_pairs, score)
    bad(lib.dgll_hip_pair_dot(None, None, 8, 5, 7, 0, p, 3, p), "non-NULL")
    bad(lib.dgll_hip_pair_dot(None, p, 8, 5, 7, 0, None, 3, p), "non-NULL")
    bad(lib.dgll_hip_pair_dot(None, p, 8, 5, 0, 0, p, 3, p), "feat")
    bad(lib.dgll_hip_pair_dot(None, p, 8, 5, 7, 2, p, 3, p), "dtype")
    bad(lib.dgll_hip_pair_dot(None, p, 7, 5, 7, 0, p, 3, p), "pitch")
    bad(lib.dgll_hip_pair_dot(None, 8, 8, 5, 7, 0, p, 3, p), "aligned")
    # pair_dot_bwd(stream, h, ldh, n_nodes, feat, dtype, inc_rowptr, inc_pair, inc_other, n_pairs, g, grad_h, ldg)
    bad(lib.dgll_hip_pair_dot_bwd(None, p, 8, 5, 7, 0, p, p, p, 3, None, p, 8), "non-NULL")
    bad(lib.dgll_hip_pair_dot_bwd(None, p, 8, 5, 0, 0, p, p, p, 3, p, p, 8), "feat")
    bad(lib.dgll_hip_pair_dot_bwd(None, p, 8, 5, 7, 7, p, p, p, 3, p, p, 8), "dtype")
    bad(lib.dgll_hip_pair_dot_bwd(None, p, 8, 5, 7, 0, p, p, p, 3, p, p, 4), "grad_h")


def small_graph():
    rowptr, col, n = ref.build_graph(67, hub=33, hub_degree=40, seed=2)
    from dgll_amd.graph import CSRGraph

    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n, n)


def test_front_end_refuses_what_it_documents(monkeypatch):
    import dgll.sampling.edge as alias
    import dgll_amd.sampling
    from dgll_amd.sampling import EdgePredictionSampler, FastNeighborSampler, NeighborSampler, PairBatch

    assert alias.EdgePredictionSampler is dgll_amd.sampling.EdgePredictionSampler and alias.PairBatch is PairBatch
    with pytest.raises(TypeError, match="NeighborSampler"):
        EdgePredictionSampler(FastNeighborSampler([4, 4]))
    with pytest.raises(TypeError, match="NeighborSampler"):
        EdgePredictionSampler([4, 4])
    bs = NeighborSampler([4, 4])
    for k in (-1, 1.5):
        with pytest.raises(ValueError, match="negatives"):
            EdgePredictionSampler(bs, negatives=k)
    for mode in ("both", "reverse_id", True):
        with pytest.raises(ValueError, match="exclude"):
            EdgePredictionSampler(bs, exclude=mode)
    for a in (0, -3):
        with pytest.raises(ValueError, match="max_attempts"):
            EdgePredictionSampler(bs, max_attempts=a)
    s = EdgePredictionSampler(bs, negatives=0, filter_existing=True, exclude="reverse", max_attempts=1)      # the edge values are fine
    with pytest.raises(ValueError, match="graph"):
        s.sample(None, [0, 1])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        s.sample(small_graph(), [0, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        EdgePredictionSampler(NeighborSampler([4])).sample_seeded(small_graph(), [0], 1)


def test_pair_batch_and_pair_dot_refuse_on_the_host():
    from dgll_amd import ops
    from dgll_amd.sampling import PairBatch

    b = PairBatch(torch.arange(4), torch.tensor([[0, 1], [2, 2], [1, 0]], dtype=torch.int32), 1, 2, capped=1)
    assert len(b) == 3 and b.labels().tolist() == [1.0, 0.0, 0.0] and b.labels().dtype == torch.float32 and b.capped == 1
    rp, pair, other = b.incidence()                         # torch ops only: the same CSR as the restatement's
    want = ref.incidence(b.pairs.numpy(), 4)
    assert b.incidence()[0] is rp and rp.dtype == torch.int64 and pair.dtype == torch.int32 and other.dtype == torch.int32
    assert all(np.array_equal(x.numpy(), w) for x, w in zip((rp, pair, other), want))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pair_dot(torch.ones(4, 8), b)                   # no CPU fallback
