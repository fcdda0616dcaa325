"""Subgraph samplers without a GPU: the numpy restatement on hand-written cases and against sampling.community.induced_range, the
distribution of GraphSAINT's draw rule, and the refusals of the Python and C interfaces.

The restatement and distribution tests validate tests/subgraph_ref.py (what the GPU tests compare the device against), not the
shipped code: only the two refusal tests run the library.  The shipped kernels are held to the restatement in test_subgraph_gpu.py."""
import numpy as np
import pytest
import torch

import subgraph_ref as ref

DIST_DEGREES = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 24, 25]          # 100 entries
DIST_DRAWS, DIST_SEED = 4096, 0xC0FFEE


# 6 nodes: row 0 holds a parallel entry (2 twice) and a self-loop, row 1 is empty, row 4 lists only node 1 (kept by no set without
# 1), rows unsorted.
HAND_ROWPTR = np.array([0, 5, 5, 8, 10, 11, 14], np.int64)
HAND_COL = np.array([2, 0, 5, 2, 3,   4, 0, 2,   5, 1,   1,   3, 0, 4], np.int32)
HAND_VAL = np.arange(1, 15, dtype=np.float32) / 8


def test_restatement_hand_written():
    rp, cl, vl, eid = ref.node_subgraph(HAND_ROWPTR, HAND_COL, HAND_VAL, [5, 0, 2, 4], None)
    # locals: 5 -> 0, 0 -> 1, 2 -> 2, 4 -> 3.  row 5: cols 3 0 4 -> keeps 0 (1), 4 (3); row 0: 2 0 5 2 3 -> 2 1 0 2; row 2: 4 0 2 -> 3 1 2;
    # row 4: col 1 -> nothing
    assert rp.tolist() == [0, 2, 6, 9, 9]
    assert cl.tolist() == [1, 3, 2, 1, 0, 2, 3, 1, 2] and cl.dtype == np.int32
    assert eid.tolist() == [12, 13, 0, 1, 2, 3, 5, 6, 7] and eid.dtype == np.int64
    assert np.array_equal(vl, HAND_VAL[eid]) and vl.dtype == np.float32
    rp2, cl2, vl2, eid2 = ref.node_subgraph(HAND_ROWPTR, HAND_COL, HAND_VAL, [5, 0, 2, 4], "row")
    assert np.array_equal(rp2, rp) and np.array_equal(cl2, cl) and np.array_equal(eid2, eid)
    assert np.array_equal(vl2, np.array([0.5] * 2 + [0.25] * 4 + [np.float32(1.0 / 3)] * 3, np.float32))
    # the empty row alone, and no values without parent values
    rp3, cl3, vl3, eid3 = ref.node_subgraph(HAND_ROWPTR, HAND_COL, None, [1], None)
    assert rp3.tolist() == [0, 0] and len(cl3) == 0 and vl3 is None and len(eid3) == 0
    # nothing listed
    rp4, cl4, vl4, _ = ref.node_subgraph(HAND_ROWPTR, HAND_COL, None, [], "row")
    assert rp4.tolist() == [0] and len(cl4) == 0 and vl4.dtype == np.float32 and len(vl4) == 0
    # every node in order: the parent itself
    rp5, cl5, vl5, eid5 = ref.node_subgraph(HAND_ROWPTR, HAND_COL, HAND_VAL, np.arange(6), None)
    assert np.array_equal(rp5, HAND_ROWPTR) and np.array_equal(cl5, HAND_COL) and np.array_equal(vl5, HAND_VAL)
    assert np.array_equal(eid5, np.arange(14))


@pytest.mark.parametrize("normalize", [None, "row"])
@pytest.mark.parametrize("with_val", [False, True])
def test_restatement_equals_induced_range(normalize, with_val):
    from dgll_amd.graph import CSRGraph
    from dgll_amd.sampling.community import induced_range

    rng = np.random.default_rng(3)
    n = 203
    deg = rng.integers(0, 12, n)
    deg[17] = 150
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)            # unsorted, parallel entries, self-loops
    val = rng.random(len(col)).astype(np.float32) if with_val else None
    g = CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None if val is None else torch.as_tensor(val), n, n)
    for start, end in ((0, n), (0, 1), (10, 75), (17, 18), (100, 203), (50, 50)):
        want = induced_range(g, start, end, normalize)
        rp, cl, vl, _ = ref.node_subgraph(rowptr, col, val, np.arange(start, end), normalize)
        assert np.array_equal(rp, want.rowptr.numpy()) and np.array_equal(cl, want.col.numpy())
        if want.val is None:
            assert vl is None
        else:
            assert np.array_equal(vl.view(np.uint32), want.val.numpy().view(np.uint32))


def dist_graph():
    rowptr = np.concatenate([[0], np.cumsum(DIST_DEGREES)]).astype(np.int64)
    col = (np.arange(100) * 7 % 12).astype(np.int32)
    return rowptr, col


def pearson(obs, exp):
    return float(((np.asarray(obs, np.float64) - exp) ** 2 / exp).sum())


def test_node_draw_follows_the_degrees():
    """Mode 1: Pearson against 4096 * deg / 100 over the 11 nodes of positive degree, below the chi-square 0.999 quantile at 10
    degrees of freedom (29.59); node 0 (degree 0) is never drawn."""
    rowptr, col = dist_graph()
    drawn = ref.saint_draws(rowptr, col, "node", DIST_DRAWS, DIST_SEED)
    counts = np.bincount(drawn, minlength=12)
    assert counts[0] == 0 and counts.sum() == DIST_DRAWS
    stat = pearson(counts[1:], DIST_DRAWS * np.asarray(DIST_DEGREES[1:], np.float64) / 100)
    print("node pearson", stat)
    assert stat < 29.59


def test_walk_roots_are_uniform():
    """Mode 3: Pearson against uniform over the 12 nodes, below the 0.999 quantile at 11 degrees of freedom (31.26)."""
    rowptr, col = dist_graph()
    roots = ref.saint_draws(rowptr, col, "walk", (DIST_DRAWS, 1), DIST_SEED)[:, 0]
    counts = np.bincount(roots, minlength=12)
    stat = pearson(counts, DIST_DRAWS / 12)
    print("root pearson", stat)
    assert len(counts) == 12 and stat < 31.26


def test_edge_draw_is_uniform():
    """Mode 2: Pearson against uniform over the 100 entries, below the 0.999 quantile at 99 degrees of freedom (148.2)."""
    rowptr, col = dist_graph()
    entries = ref.saint_draws(rowptr, col, "edge", DIST_DRAWS, DIST_SEED)
    counts = np.bincount(entries, minlength=100)
    stat = pearson(counts, DIST_DRAWS / 100)
    print("edge pearson", stat)
    assert len(counts) == 100 and stat < 148.2


def test_saint_node_sets_of_the_restatement():
    rowptr, col = dist_graph()
    for mode, budget in (("node", 5), ("edge", 5), ("walk", (3, 4))):
        nodes = ref.saint_nodes(rowptr, col, mode, budget, 9)
        assert nodes.dtype == np.int64 and np.all(np.diff(nodes) > 0) and nodes.min() >= 0 and nodes.max() < 12
    assert 0 not in ref.saint_nodes(rowptr, col, "node", 4096, 9)
    # the same seed serves the roots and the walk: the walk starts at its root
    w = ref.saint_draws(rowptr, col, "walk", (64, 3), 9)
    assert w.shape == (64, 4) and np.array_equal(w[:, 0], ref.saint_draws(rowptr, col, "walk", (64, 1), 9)[:, 0])
    dead = w[:, 0] == 0                                                   # node 0 has no entries: the walk ends at once
    assert dead.any() and np.all(w[dead, 1:] == -1) and np.all(w[~dead, 1] >= 0)


def cpu_graph(n_rows=6, n_cols=6):
    from dgll_amd.graph import CSRGraph

    rowptr = HAND_ROWPTR if n_rows == 6 else np.zeros(n_rows + 1, np.int64)
    col = HAND_COL if n_rows == 6 else np.zeros(0, np.int32)
    return CSRGraph(torch.as_tensor(rowptr), torch.as_tensor(col), None, n_rows, n_cols)


def test_python_refusals_without_a_gpu():
    from dgll_amd import sampling
    from dgll_amd.sampling import SAINTSampler, ShaDowKHopSampler, SubgraphWorkspace, node_subgraph

    from dgll.sampling import SAINTSampler as shim_saint, ShaDowKHopSampler as shim_shadow
    from dgll.sampling.subgraph import node_subgraph as shim_node_subgraph

    assert shim_node_subgraph is node_subgraph and shim_saint is SAINTSampler and shim_shadow is ShaDowKHopSampler
    assert sampling.subgraph.LONG_ROW >= 1
    with pytest.raises(ValueError, match="normalize"):
        node_subgraph(cpu_graph(), [0, 1], normalize="sym")
    with pytest.raises(ValueError, match="square"):
        node_subgraph(cpu_graph(4, 7), [0, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        node_subgraph(cpu_graph(), [0, 1])                                # a CPU graph: no quiet fall-back
    with pytest.raises(ValueError):
        SubgraphWorkspace(0, "cpu")
    with pytest.raises(ValueError, match="normalize"):
        ShaDowKHopSampler([5, 2], normalize="sym")
    with pytest.raises(ValueError):
        ShaDowKHopSampler([])
    for mode, budget in (("node", 0), ("edge", -3), ("walk", (0, 4)), ("walk", (4, 0)), ("walk", 7), ("node", (3, 4)), ("metis", 5)):
        with pytest.raises(ValueError):
            SAINTSampler(mode, budget)
    with pytest.raises(ValueError, match="normalize"):
        SAINTSampler("node", 5, normalize="sym")
    for mode in ("node", "edge"):
        with pytest.raises(ValueError, match="none"):
            SAINTSampler(mode, 5, cpu_graph(4, 4))                        # a graph without entries
    with pytest.raises(ValueError, match="needs a graph"):
        SAINTSampler("node", 5).sample_seeded(None, 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            SAINTSampler("node", 5, cpu_graph())
        with pytest.raises(RuntimeError, match="GPU"):
            ShaDowKHopSampler([5, 2], cpu_graph())


def test_c_abi_refusals_without_a_gpu():
    from dgll_amd import _lib

    lib, p = _lib.lib, 16                                                 # 16: any non-NULL pointer; nothing is dereferenced
    assert lib.dgll_hip_sg_long_row() >= 1
    bad_count = [
        (None, p, 10, 5, p, 3, p, 1, p, p),       # rowptr NULL
        (p, p, 10, 5, None, 3, p, 1, p, p),       # nodes NULL with m > 0
        (p, p, 10, 5, p, 3, None, 1, p, p),       # tags NULL
        (p, p, 10, 5, p, 3, p, 1, None, p),       # out_rowptr NULL
        (p, p, 10, 5, p, 3, p, 1, p, None),       # info NULL
        (p, p, 10, 5, p, -1, p, 1, p, p),         # m < 0
        (p, p, 0, 5, p, 3, p, 1, p, p),           # n_total == 0
        (p, p, 2 ** 31, 5, p, 3, p, 1, p, p),     # n_total == 2^31
        (p, p, 10, 5, p, 3, p, 0, p, p),          # epoch 0
    ]
    for args in bad_count:
        assert lib.dgll_hip_sg_count(None, *args) == -1 and _lib.last_error()
    bad_fill = [
        (None, p, None, 10, 5, p, 3, p, 1, p, 2, p, None, None, p),
        (p, p, None, 10, 5, p, 3, None, 1, p, 2, p, None, None, p),
        (p, p, None, 10, 5, p, 3, p, 1, p, 2, None, None, None, p),     # entries without a column output
        (p, p, None, 10, 5, p, -2, p, 1, p, 2, p, None, None, p),
        (p, p, None, 10, 5, p, 3, p, 1, p, 6, p, None, None, p),         # more kept entries than entries
        (p, p, None, -1, 5, p, 3, p, 1, p, 2, p, None, None, p),
    ]
    for args in bad_fill:
        assert lib.dgll_hip_sg_fill(None, *args) == -1 and _lib.last_error()
    bad_draw = [
        (None, p, 10, 5, 1, 4, 0, p, p, None, p),
        (p, p, 10, 5, 0, 4, 0, p, p, None, p),     # mode 0
        (p, p, 10, 5, 4, 4, 0, p, p, p, p),        # mode 4
        (p, p, 10, 5, 1, 0, 0, p, p, None, p),     # budget 0
        (p, p, 10, 5, 1, -4, 0, p, p, None, p),
        (p, p, 10, 0, 2, 4, 0, p, p, None, p),     # no entries to draw
        (p, p, 10, 5, 1, 4, 0, None, p, None, p),  # bitmap NULL
        (p, p, 10, 5, 3, 4, 0, None, None, None, p),   # roots NULL
        (p, p, 0, 5, 3, 4, 0, None, None, p, p),
        (p, p, 10, 5, 1, 4, 0, p, p, None, None),
    ]
    for args in bad_draw:
        assert lib.dgll_hip_sg_draw(None, *args) == -1 and _lib.last_error()
    assert lib.dgll_hip_sg_walk_nodes(None, None, 4, 10, p, p, p) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_sg_walk_nodes(None, p, 0, 10, p, p, p) == -1
    assert lib.dgll_hip_sg_compact(None, 10, None, p, 3, p) == -1 and "NULL" in _lib.last_error()
    assert lib.dgll_hip_sg_compact(None, 10, p, p, 11, p) == -1
    assert lib.dgll_hip_sg_compact(None, 10, p, p, -1, p) == -1
