"""Pure numpy / Python restatement of the neighbour sampler (dgll_amd/csrc/neighbor.hip) -- a helper, not a test.  The only native
call is the host Philox (dgll_host_philox4x32_10); every decision is an integer compare, so the device output is bit-equal."""
import numpy as np


def philox(counter4, key2):
    from dgll_amd import _lib

    c = np.asarray(counter4, dtype=np.uint32)
    k = np.asarray(key2, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    assert _lib.lib.dgll_host_philox4x32_10(c.ctypes.data, k.ctypes.data, out.ctypes.data) == 0
    return [int(x) for x in out]


def positions(d, v, fanout, seed, layer):
    """Kept positions (ascending) of a row of degree d of node v."""
    d, v, fanout, seed = int(d), int(v), int(fanout), int(seed) & (2 ** 64 - 1)
    if fanout < 0 or d <= fanout:
        return list(range(d))
    key = [seed & 0xFFFFFFFF, seed >> 32]
    taken, words = set(), []
    for i in range(fanout):                      # Floyd: j = d - fanout .. d - 1
        if i % 4 == 0:
            words = philox([v & 0xFFFFFFFF, v >> 32, layer, i // 4], key)
        j = d - fanout + i
        t = (words[i % 4] * (j + 1)) >> 32
        taken.add(j if t in taken else t)
    assert len(taken) == fanout
    return sorted(taken)


def draw(rowptr, col, v, fanout, seed, layer):
    """Global ids of the kept in-neighbours of v, in ascending position."""
    b, e = int(rowptr[v]), int(rowptr[v + 1])
    return [int(col[b + p]) for p in positions(e - b, v, fanout, seed, layer)]


def to_block(dst, drawn_rows, norm):
    """(src_nodes, rowptr, col, val): src = [dst | new ids ascending], local columns ascending within a row."""
    dst = [int(v) for v in dst]
    local = {v: i for i, v in enumerate(dst)}
    assert len(local) == len(dst), "duplicate destination"
    new = sorted({c for row in drawn_rows for c in row} - set(local))
    for i, c in enumerate(new):
        local[c] = len(dst) + i
    rowptr, col, val = [0], [], []
    for row in drawn_rows:
        ids = sorted(local[c] for c in row)
        col += ids
        val += [np.float32(1.0 / len(ids))] * len(ids) if ids else []
        rowptr.append(len(col))
    return (np.asarray(dst + new, np.int64), np.asarray(rowptr, np.int64), np.asarray(col, np.int32),
            np.asarray(val, np.float32) if norm == "mean" else None)


def sample_blocks(rowptr, col, seeds, fanouts, seed, norm="mean"):
    """(input_nodes, blocks): blocks outermost first, each a dict {rowptr, col, val, n_rows, n_cols, dst, src}; fanouts in DGL's
    order (the last entry is applied to the seeds first; layer index = position in fanouts)."""
    rows = np.asarray(seeds, np.int64).reshape(-1)
    blocks = []
    for layer in range(len(fanouts) - 1, -1, -1):
        drawn = [draw(rowptr, col, int(v), fanouts[layer], seed, layer) for v in rows]
        src, rp, cl, vl = to_block(rows, drawn, norm)
        blocks.append({"rowptr": rp, "col": cl, "val": vl, "n_rows": len(rows), "n_cols": len(src), "dst": rows, "src": src})
        rows = src
    blocks.reverse()
    return rows, blocks


def check_invariants(rowptr, col, seeds, fanouts, input_nodes, blocks, norm="mean"):
    """The structural contract, for blocks given as dicts of numpy arrays (rowptr, col, val, n_rows, n_cols, src, dst)."""
    assert len(blocks) == len(fanouts)
    assert np.array_equal(blocks[-1]["dst"], np.asarray(seeds, np.int64).reshape(-1))
    assert np.array_equal(input_nodes, blocks[0]["src"])
    for i, (blk, f) in enumerate(zip(blocks, fanouts)):
        dst, src, rp, cl = blk["dst"], blk["src"], blk["rowptr"], blk["col"]
        n_dst = len(dst)
        assert blk["n_rows"] == n_dst and blk["n_cols"] == len(src) and len(rp) == n_dst + 1 and rp[0] == 0 and rp[-1] == len(cl)
        if i + 1 < len(blocks):
            assert blk["n_rows"] == blocks[i + 1]["n_cols"] and np.array_equal(dst, blocks[i + 1]["src"])
        assert len(np.unique(src)) == len(src)                                  # sources are unique
        assert np.array_equal(src[:n_dst], dst)                                 # the destinations first, in order
        assert np.all(np.diff(src[n_dst:]) > 0)                                 # then ascending
        used = np.zeros(len(src), bool)
        used[cl] = True
        assert used[n_dst:].all()                                               # every new node is somebody's neighbour
        deg = rowptr[dst + 1] - rowptr[dst] if n_dst else np.zeros(0, np.int64)
        want = deg if f < 0 else np.minimum(deg, f)
        assert np.array_equal(np.diff(rp), want)                                # min(d, f) per row
        for r in range(n_dst):
            ids = cl[rp[r]:rp[r + 1]]
            assert np.all(np.diff(ids) > 0)                                     # ascending and unique within a row
            nbrs = col[rowptr[dst[r]]:rowptr[dst[r] + 1]]
            assert np.isin(src[ids], nbrs).all()                                # every edge exists in the graph
            if norm == "mean" and len(ids):
                assert abs(float(blk["val"][rp[r]:rp[r + 1]].astype(np.float64).sum()) - 1.0) < 1e-5
        if norm != "mean":
            assert blk["val"] is None
