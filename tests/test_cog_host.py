"""CoG on the host: the group forming against the reference's recorded behaviour, `modularity` against a dense computation, and the
numpy restatement of the size-capped Louvain (tests/louvain_ref.py, what the device is held to bit for bit in test_cog_gpu.py)
against networkx's modularity on the two fixture graphs.  No GPU."""
import hashlib

import numpy as np
import pytest
import torch

import louvain_ref as lref
from conftest import load_golden
from dgll_amd import community, reorder, synth
from dgll_amd.graph import CSRGraph


@pytest.fixture(scope="module")
def golden():
    return load_golden("cog_groups")


def _communities(golden, i):
    ptr, nodes = golden["comm_ptr_%d" % i], golden["comm_nodes_%d" % i]
    return [nodes[ptr[j]:ptr[j + 1]].tolist() for j in range(len(ptr) - 1)]


def test_merge_and_relabel_reproduce_the_reference(golden):
    for i, batch in enumerate(golden.meta["batch"]):
        nodes, gptr = community.merge_groups(_communities(golden, i), batch)
        keep = golden["group_ptr_%d" % i]
        assert nodes.tolist() == golden["group_nodes_%d" % i].tolist() and gptr.tolist() == keep.tolist(), i
        perm, inv, ranges = community.relabel_groups((nodes, gptr))
        assert inv[nodes].tolist() == golden["new_id_%d" % i].tolist(), i              # the reference's con_id_mapping
        assert ranges.tolist() == golden["ranges_%d" % i].tolist(), i                  # its groups_id_map_list
        assert torch.equal(perm[inv], torch.arange(nodes.numel()))


def test_merge_groups_from_a_label_vector():
    labels = torch.tensor([2, 0, 2, 1, 0, 2, 4])                  # community 3 is empty
    nodes, gptr = community.merge_groups(labels, 3)
    assert nodes.tolist() == [1, 4, 3, 0, 2, 5, 6] and gptr.tolist() == [0, 3, 6, 7]
    with pytest.raises(ValueError):
        community.relabel_groups([[0, 1], [1]])


def _graph(golden, name):
    return golden["rowptr_" + name].astype(np.int64), golden["col_" + name].astype(np.int32)


@pytest.mark.parametrize("resolution", [1.0, 0.7])
def test_modularity_equals_the_dense_computation(golden, resolution):
    rowptr, col = _graph(golden, "A")
    n = len(rowptr) - 1
    g = CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(col), None, n, n)
    labels = torch.from_numpy(golden["planted_A"].astype(np.int64))
    a = np.zeros((n, n))
    a[np.repeat(np.arange(n), np.diff(rowptr)), col] = 1.0
    k = a.sum(1)
    same = labels.numpy()[:, None] == labels.numpy()[None, :]
    dense = ((a - resolution * np.outer(k, k) / a.sum()) * same).sum() / a.sum()
    assert abs(community.modularity(g, labels, resolution) - dense) < 1e-12
    assert abs(lref.modularity(rowptr, col, labels.numpy(), resolution) - dense) < 1e-12


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_louvain_reaches_networkx_modularity(golden, name, seed):
    rowptr, col = _graph(golden, name)
    labels = lref.louvain(rowptr, col, seed=seed)
    q = lref.modularity(rowptr, col, labels)
    floor = float(golden["nx_modularity_" + name].min())
    print("graph", name, "seed", seed, "Q", q, "networkx min", floor, "ratio", q / floor)
    assert sorted(np.unique(labels).tolist()) == list(range(int(labels.max()) + 1))            # dense
    assert q >= 0.98 * floor


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cap", [150, 64])
def test_cap_holds_after_every_sweep(golden, name, cap):
    rowptr, col = _graph(golden, name)
    worst, sweeps = [0], [0]

    def check(level, sweep, comm, size):
        worst[0] = max(worst[0], int(np.bincount(comm, weights=size).max()))
        sweeps[0] += 1

    labels = lref.louvain(rowptr, col, max_comm_size=cap, seed=0, on_sweep=check)
    sizes = np.bincount(labels)
    print("graph", name, "cap", cap, "largest community", sizes.max(), "largest after any sweep", worst[0], "sweeps", sweeps[0])
    assert sweeps[0] >= 3 and worst[0] <= cap and sizes.max() <= cap
    assert sizes.max() > cap / 2


def test_two_runs_give_identical_labels(golden):
    rowptr, col = _graph(golden, "A")
    a, b = lref.louvain(rowptr, col, max_comm_size=64, seed=3), lref.louvain(rowptr, col, max_comm_size=64, seed=3)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, lref.louvain(rowptr, col, max_comm_size=64, seed=4))          # the seed picks the active halves


def test_admission_is_a_prefix_in_target_then_id_order():
    comm = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
    target = np.array([0, 0, 0, 3, 3, 0], dtype=np.int32)
    size = np.array([2, 1, 1, 2, 3, 1], dtype=np.int64)
    movers, t = lref.admit(comm, target, size, size.copy(), cap=4)
    assert movers.tolist() == [1, 2] and t.tolist() == [0, 0]                # node 5 would make 5; node 4 (2 + 3) does not fit 3
    tm, tt = community.admit(torch.from_numpy(comm), torch.from_numpy(target), torch.from_numpy(size), torch.from_numpy(size.copy()), 4)
    assert tm.tolist() == [1, 2] and tt.tolist() == [0, 0]


# sha256 of the int64 bytes of label_propagation's labels and of locality_order(method="lpa")'s permutation on the graph below,
# recorded by running exactly these lines against the parent commit's dgll_amd/reorder.py (that file alone, loaded as a module
# of its own): "lpa" must stay bit-identical.
LPA_LABELS_SHA256 = "f06fa17d54243c32568ee0fce6bfe4acee5f12d5d187320c9e05ee4eb3d999de"
LPA_PERM_SHA256 = "b305814cf8e1bf6dc94cc84fb56ba4c7a5cf086e6d619dcff8ba0a0401bcf753"


def lpa_checksums(module):
    g = synth.products_like_graph("cpu", seed=5, n=3000, n_undirected=20000, locality=0.85, n_blocks=6, exact=True, permute_ids=True)
    labels = module.label_propagation(g.rowptr, g.col, g.n_rows, seed=2)
    perm = module.locality_order(g.rowptr, g.col, g.n_rows, method="lpa", seed=2)
    return tuple(hashlib.sha256(x.numpy().astype(np.int64).tobytes()).hexdigest() for x in (labels, perm))


def test_lpa_is_unchanged():
    assert lpa_checksums(reorder) == (LPA_LABELS_SHA256, LPA_PERM_SHA256)
    g = synth.products_like_graph("cpu", seed=5, n=3000, n_undirected=20000, locality=0.85, n_blocks=6, exact=True, permute_ids=True)
    assert torch.equal(g.reorder(seed=2)[1], reorder.locality_order(g.rowptr, g.col, g.n_rows, seed=2))       # "lpa" is the default
    with pytest.raises(ValueError, match="'lpa', 'louvain', 'degree' or 'random'"):
        reorder.locality_order(g.rowptr, g.col, g.n_rows, method="leiden")


def test_louvain_needs_the_gpu_and_a_valid_cap(golden):
    rowptr, col = _graph(golden, "A")
    n = len(rowptr) - 1
    g = CSRGraph(torch.from_numpy(rowptr), torch.from_numpy(col), None, n, n)
    with pytest.raises(RuntimeError, match="GPU only"):
        community.louvain(g)
    with pytest.raises(RuntimeError, match="GPU only"):
        g.reorder(method="louvain")


def test_abi_rejects_bad_arguments_without_a_gpu():
    from dgll_amd import _lib

    p = 16                                                        # never dereferenced: validation comes first
    args = lambda two_m, cap, wave, block: (None, p, p, None, p, p, p, p, p, p, 4, 4, two_m, 1.0, cap, 0, 0, 0, 0, wave, block, p, 1 << 20,  # noqa: E731
                                            p, p)
    assert _lib.lib.dgll_hip_louvain_move(*args(2 ** 53, 4, -1, -1)) == -1 and "2^53" in _lib.last_error()
    assert _lib.lib.dgll_hip_louvain_move(*args(8, 0, -1, -1)) == -1 and "cap" in _lib.last_error()
    assert _lib.lib.dgll_hip_louvain_move(*args(8, 4, 129, -1)) == -1 and "wave_max_deg" in _lib.last_error()
    assert _lib.lib.dgll_hip_louvain_move(*args(8, 4, 4, 4096)) == -1 and "block_max_deg" in _lib.last_error()
    assert _lib.lib.dgll_hip_louvain_scratch_bytes(10, 0) == 64 + 40 and _lib.lib.dgll_hip_louvain_scratch_bytes(10, 3) == 64 + 24 + 16 + 40
