"""numpy restatement of the reference's layer-wise samplers (GPU Accelerator/MQLadies.py, MQFastGCN*.py, utils.py), pinned to the
fixtures tests/golden/layerwise_*.npz by tests/test_layerwise_host.py and used as the float64 oracle of the GPU tests."""
import numpy as np
import scipy.sparse as sp


def adjacency(indptr, indices, n):
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))


def row_normalized(A):
    """D^-1 (A + I), rows summing to 0 kept at 0 (utils.py:12-20)."""
    M = (A + sp.eye(A.shape[0])).tocsr()
    rowsum = np.asarray(M.sum(1)).flatten()
    inv = np.where(rowsum != 0, 1.0 / np.where(rowsum != 0, rowsum, 1.0), 0.0)
    return sp.diags(inv).dot(M).tocsr()


def sym_normalized_transpose(A):
    """D^-1/2 (A + I)^T D^-1/2 with D the row sums of A + I (+1e-20) (utils.py:215-222)."""
    M = (A + sp.eye(A.shape[0])).tocsr()
    d = np.power(np.asarray(M.sum(1)).flatten() + 1e-20, -0.5)
    d[np.isinf(d)] = 0.0
    D = sp.diags(d)
    return (D.dot(M.transpose()).dot(D)).tocsr()


def column_p(L, rows, flat=False):
    """p over all N columns from the rows R: sum_i L_ij^2 (sqrt with flat), normalised."""
    Q = L[rows, :] if rows is not None else L
    q = np.asarray(Q.multiply(Q).sum(0)).flatten()
    if flat:
        q = np.sqrt(q)
    return q / q.sum()


def wrs_weights(p_sel, n):
    """estWRS_weights (utils.py:199-213) for a GIVEN draw order: p_sel = p of the drawn ids in order, n = len(p) = N."""
    m = len(p_sel)
    w = np.zeros(m)
    p_sum = 0.0
    for i in range(m):
        alpha = n / (i + 1) / (n - i)
        w[i] = (1 - p_sum) / p_sel[i] * alpha
        w[:i] = w[:i] * (1 - alpha) + alpha
        p_sum += p_sel[i]
    return w


def inverse_weights(p_sel, s):
    return 1.0 / p_sel / s


def block(L, rows, cols, w):
    """L[R][:, cols] * w as CSR (indptr, local ids sorted within a row, values)."""
    B = L[rows][:, cols].multiply(w).tocsr()
    B.sort_indices()
    return B.indptr.astype(np.int64), B.indices.astype(np.int64), B.data.astype(np.float64)


def sorted_within_rows(indptr, indices, values=None):
    """(indices, values) with every row's entries ordered by column."""
    idx = np.array(indices, copy=True)
    val = None if values is None else np.array(values, copy=True)
    for r in range(len(indptr) - 1):
        a, b = indptr[r], indptr[r + 1]
        o = np.argsort(idx[a:b], kind="stable")
        idx[a:b] = idx[a:b][o]
        if val is not None:
            val[a:b] = val[a:b][o]
    return idx, val
