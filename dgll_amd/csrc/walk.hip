// walk.hip -- uniform (DeepWalk), second-order (node2vec) and edge-weighted random walks over a device CSR, and the per-row alias
// tables the weighted walks draw from.
//
// One lane per walk.  A step is pointer chasing: rowptr[v], rowptr[v + 1] (one load level), then col[b + r] (a second, dependent
// level); the biased step adds, per attempt, a binary search of the candidate in the previous node's sorted row (log2 deg(t)
// dependent loads).  Nothing overlaps inside a walk, so the kernel is bound by the latency of those dependent loads times the
// walks in flight; a lane whose walk has hit a dead end idles until the longest walk of its wavefront ends.
// Every random word is Philox4x32-10 with key = seed and counter = (walk index lo, walk index hi, step, attempt): walk i is the
// same whichever launch, batch or batch size draws it.  Every decision is an integer compare (mulhi for the candidate, x1 < T for
// the acceptance), so a host restatement is bit-exact.
// Weighted walks draw the out-edge from a per-row alias table (Vose), 8 bytes per edge: {keep threshold T, alias index local to the
// row}.  slot = mulhi(x0, deg); e = x1 < T[b + slot] ? slot : alias[b + slot]: one more dependent load level (rowptr, table entry,
// col) than the uniform step.  The second-order bias is the same rejection step on top, with word 2 as the acceptance word, so
// P(x | t, v) is proportional to w_vx * bias(t, x).  A slot that always keeps itself is its own alias with T = 2^32 - 1 (no 33-bit
// threshold); a row whose weights sum to 0 carries {0, slot} in every slot, which no live row holds, and ends the walk.
#include <math.h>

#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace walk {

enum { kInfoCapped = 0, kInfoErr = 1 };
enum { kErrStart = 1, kErrCol = 2, kErrWeight = 4, kErrAlias = 8 };

// is x an out-neighbour of t?  t's row ascends (the Python layer checks it once per graph)
__device__ __forceinline__ bool has_edge(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int32_t t, int32_t x) {
    int64_t lo = rowptr[t], hi = rowptr[t + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t c = col[mid];
        if (c == x) return true;
        if (c < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(kBlock) void random_walk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             int64_t n_nodes, const int64_t* __restrict__ starts, int64_t n, int length,
                                                             uint64_t first, uint64_t seed, uint64_t t_ret, uint64_t t_common,
                                                             uint64_t t_far, int biased, int max_attempts,
                                                             int32_t* __restrict__ walks, unsigned long long* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t widx = first + (uint64_t)i;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int32_t* out = walks + i * length;
    const int64_t s0 = starts[i];
    int32_t v = (int32_t)s0, t = -1;
    if (s0 < 0 || s0 >= n_nodes) { v = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrStart); }
    out[0] = v;
    unsigned long long capped = 0;
    for (int s = 1; s < length; ++s) {
        int32_t next = -1;
        if (v >= 0) {
            const int64_t b = rowptr[v];
            const uint32_t deg = (uint32_t)(rowptr[v + 1] - b);          // < 2^32: checked on the host
            if (deg != 0u) {
                for (int a = 0; a < max_attempts; ++a) {
                    const uint32_t ctr[4] = {(uint32_t)widx, (uint32_t)(widx >> 32), (uint32_t)s, (uint32_t)a};
                    uint32_t x[4];
                    philox4x32_10(ctr, key, x);
                    next = col[b + (int64_t)__umulhi(x[0], deg)];
                    if (next < 0 || next >= n_nodes) { next = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrCol); break; }
                    if (!biased || s == 1) break;                        // the first step has no previous node
                    const uint64_t T = next == t ? t_ret : (has_edge(rowptr, col, t, next) ? t_common : t_far);
                    if ((uint64_t)x[1] < T) break;
                    if (a == max_attempts - 1) ++capped;                 // the cap: keep the last candidate, and say so
                }
            }
        }
        t = v; v = next;
        out[s] = v;
    }
    if (capped) atomicAdd(info + kInfoCapped, capped);
}

// Vose's alias construction, one lane per row (a once-per-graph pass).  q = w deg / sum(w) in float64, in the row's edge order; the
// two worklists are stacks that grow from the two ends of the row's own stretch of `work`, so the order of every pairing is fixed
// and two builds give the same bits.  A slot l taken from `small` is final: T = round(2^32 q_l) (clamped to 2^32 - 1), alias = the
// slot on top of `large`, which gives up 1 - q_l.  What is left when one list runs dry keeps itself.  A zero weight is always in
// `small` with T = 0, and aliases only come from `large` (q >= 1), so a zero-weight edge is never drawn.
// Returns false when a weight is negative, NaN or infinite; the row is then left a dead end.
__host__ __device__ inline bool alias_build_row(const float* __restrict__ val, int64_t b, int64_t e, double* __restrict__ q,
                                                uint32_t* __restrict__ work, uint2* __restrict__ table) {
    const uint32_t deg = (uint32_t)(e - b);                                  // < 2^32: checked on the host
    double sum = 0.0;
    float w_top = 0.0f;
    uint32_t top = 0;                                                        // the heaviest edge: a positive weight when sum > 0
    bool bad = false;
    for (uint32_t j = 0; j < deg; ++j) {
        const float w = val[b + j];
        if (!(w >= 0.0f) || isinf(w)) { bad = true; continue; }
        sum += (double)w;
        if (w > w_top) { w_top = w; top = j; }
    }
    if (bad || !(sum > 0.0)) {                                               // a dead row: the walk ends here
        for (uint32_t j = 0; j < deg; ++j) table[b + j] = make_uint2(0u, j);
        return !bad;
    }
    const double scale = (double)deg / sum;
    uint32_t ns = 0, nl = 0;                                                 // small: work[b, b + ns), large: work[e - nl, e)
    for (uint32_t j = 0; j < deg; ++j) {
        const double qj = (double)val[b + j] * scale;
        q[b + j] = qj;
        if (qj < 1.0) work[b + ns++] = j; else work[e - ++nl] = j;
    }
    while (ns != 0u && nl != 0u) {
        const uint32_t l = work[b + --ns], g = work[e - nl];
        const double ql = q[b + l];
        table[b + l] = make_uint2((uint32_t)fmin(rint(ql * 4294967296.0), 4294967295.0), g);
        const double qg = (q[b + g] + ql) - 1.0;
        q[b + g] = qg;
        if (qg < 1.0) { --nl; work[b + ns++] = g; }
    }
    for (uint32_t k = 0; k < ns + nl; ++k) {                                 // the rest keeps itself (q = 1 up to float64 drift)
        const uint32_t j = k < ns ? work[b + k] : work[e - nl + (k - ns)];
        table[b + j] = val[b + j] > 0.0f ? make_uint2(0xFFFFFFFFu, j) : make_uint2(0u, top);
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void alias_build_kernel(const int64_t* __restrict__ rowptr, const float* __restrict__ val,
                                                             int64_t n_rows, double* __restrict__ q, uint32_t* __restrict__ work,
                                                             uint2* __restrict__ table, unsigned long long* __restrict__ info) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_rows) return;
    const int64_t b = rowptr[r], e = rowptr[r + 1];
    if (e > b && !alias_build_row(val, b, e, q, work, table)) atomicOr(info + kInfoErr, (unsigned long long)kErrWeight);
}

// random_walk_kernel with the candidate drawn from the alias table; word 2 is the acceptance word
__global__ __launch_bounds__(kBlock) void random_walk_weighted_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                      const uint2* __restrict__ table, int64_t n_nodes,
                                                                      const int64_t* __restrict__ starts, int64_t n, int length,
                                                                      uint64_t first, uint64_t seed, uint64_t t_ret, uint64_t t_common,
                                                                      uint64_t t_far, int biased, int max_attempts,
                                                                      int32_t* __restrict__ walks, unsigned long long* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t widx = first + (uint64_t)i;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int32_t* out = walks + i * length;
    const int64_t s0 = starts[i];
    int32_t v = (int32_t)s0, t = -1;
    if (s0 < 0 || s0 >= n_nodes) { v = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrStart); }
    out[0] = v;
    unsigned long long capped = 0;
    for (int s = 1; s < length; ++s) {
        int32_t next = -1;
        if (v >= 0) {
            const int64_t b = rowptr[v];
            const uint32_t deg = (uint32_t)(rowptr[v + 1] - b);          // < 2^32: checked on the host
            if (deg != 0u) {
                for (int a = 0; a < max_attempts; ++a) {
                    const uint32_t ctr[4] = {(uint32_t)widx, (uint32_t)(widx >> 32), (uint32_t)s, (uint32_t)a};
                    uint32_t x[4];
                    philox4x32_10(ctr, key, x);
                    const uint32_t slot = __umulhi(x[0], deg);
                    const uint2 ta = table[b + (int64_t)slot];
                    if (ta.x == 0u && ta.y == slot) { next = -1; break; }   // the row's weights sum to 0: a dead end
                    const uint32_t e = x[1] < ta.x ? slot : ta.y;
                    if (e >= deg) { next = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrAlias); break; }
                    next = col[b + (int64_t)e];
                    if (next < 0 || next >= n_nodes) { next = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrCol); break; }
                    if (!biased || s == 1) break;                        // the first step has no previous node
                    const uint64_t T = next == t ? t_ret : (has_edge(rowptr, col, t, next) ? t_common : t_far);
                    if ((uint64_t)x[2] < T) break;
                    if (a == max_attempts - 1) ++capped;                 // the cap: keep the last candidate, and say so
                }
            }
        }
        t = v; v = next;
        out[s] = v;
    }
    if (capped) atomicAdd(info + kInfoCapped, capped);
}

// struc2vec's walk over the multilayer context graph: a stacked CSR of n_layers * n_nodes rows (row layer * n_nodes + v holds v's
// neighbours in that layer, plain node ids) with its alias table.  The lane carries (v, layer), layer 0 at the start.  Attempt a of
// step s draws one block: x0 < t_stay stays in the layer and emits a neighbour drawn from the row as random_walk_weighted_kernel
// draws it (x1 the slot, x2 keep or alias); otherwise x3 < t_up[row] moves up when row (layer + 1) * n_nodes + v has entries, and
// down when it is not an up-move and layer > 0 -- no node is emitted and the next attempt follows.  The last allowed attempt stays
// whatever x0 says and is counted.  The same pointer chasing as above with one more level (t_up) on a layer move.
__global__ __launch_bounds__(kBlock) void struc_walk_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const uint2* __restrict__ table, const uint32_t* __restrict__ t_up,
                                                            int64_t n_nodes, int n_layers, const int64_t* __restrict__ starts, int64_t n,
                                                            int length, uint64_t first, uint64_t seed, uint64_t t_stay, int max_attempts,
                                                            int32_t* __restrict__ walks, int32_t* __restrict__ layers_out,
                                                            unsigned long long* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t widx = first + (uint64_t)i;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    int32_t* out = walks + i * length;
    int32_t* lay = layers_out ? layers_out + i * length : nullptr;
    const int64_t s0 = starts[i];
    int32_t v = (int32_t)s0;
    int layer = 0;
    if (s0 < 0 || s0 >= n_nodes) { v = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrStart); }
    out[0] = v;
    if (lay) lay[0] = v >= 0 ? 0 : -1;
    unsigned long long capped = 0;
    for (int s = 1; s < length; ++s) {
        int32_t next = -1;
        if (v >= 0) {
            for (int a = 0; a < max_attempts; ++a) {
                const uint32_t ctr[4] = {(uint32_t)widx, (uint32_t)(widx >> 32), (uint32_t)s, (uint32_t)a};
                uint32_t x[4];
                philox4x32_10(ctr, key, x);
                const int64_t row = (int64_t)layer * n_nodes + v;
                const bool last = a == max_attempts - 1;
                if (last) ++capped;                                          // the cap: this attempt stays, and says so
                if ((uint64_t)x[0] < t_stay || last) {
                    const int64_t b = rowptr[row];
                    const uint32_t deg = (uint32_t)(rowptr[row + 1] - b);    // < 2^32: checked on the host
                    if (deg == 0u) break;                                    // nobody to go to in this layer: the walk ends
                    const uint32_t slot = __umulhi(x[1], deg);
                    const uint2 ta = table[b + (int64_t)slot];
                    if (ta.x == 0u && ta.y == slot) break;                   // the row's weights sum to 0: a dead end
                    const uint32_t e = x[2] < ta.x ? slot : ta.y;
                    if (e >= deg) { atomicOr(info + kInfoErr, (unsigned long long)kErrAlias); break; }
                    next = col[b + (int64_t)e];
                    if (next < 0 || next >= n_nodes) { next = -1; atomicOr(info + kInfoErr, (unsigned long long)kErrCol); }
                    break;
                }
                if (x[3] < t_up[row]) {
                    if (layer + 1 < n_layers) {
                        const int64_t above = row + n_nodes;
                        if (rowptr[above + 1] > rowptr[above]) ++layer;
                    }
                } else if (layer > 0) {
                    --layer;
                }
            }
        }
        v = next;
        out[s] = v;
        if (lay) lay[s] = v >= 0 ? layer : -1;
    }
    if (capped) atomicAdd(info + kInfoCapped, capped);
}

}  // namespace walk
}  // namespace dgll

using namespace dgll;

// acceptance thresholds T = round(2^32 w / M) of the classes w = {1/p (return), 1 (common neighbour), 1/q (far)}, M = max w:
// float64 on the host, integers on the device
static void thresholds(double p, double q, uint64_t out3[3]) {
    const double wr = 1.0 / p, wf = 1.0 / q, m = fmax(fmax(wr, 1.0), wf);
    out3[0] = (uint64_t)rint(4294967296.0 * (wr / m));
    out3[1] = (uint64_t)rint(4294967296.0 * (1.0 / m));
    out3[2] = (uint64_t)rint(4294967296.0 * (wf / m));
}

DGLL_API int dgll_hip_random_walk(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_nodes, const int64_t* starts,
                                  int64_t n, int length, uint64_t first_walk_index, uint64_t seed, double p, double q,
                                  int max_attempts, int32_t* walks, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && (starts || n == 0) && (walks || n == 0) && info, "CSR, starts, walks and info must be non-NULL");
    DGLL_REQUIRE(length >= 1, "walk length must be >= 1");
    DGLL_REQUIRE(p > 0.0 && q > 0.0 && isfinite(p) && isfinite(q), "node2vec p and q must be positive and finite");
    DGLL_REQUIRE(n >= 0 && n_nodes > 0 && n_nodes < (1ll << 31) && n <= (1ll << 31) * kBlock - kBlock, "walk count, node count < 2^31");
    DGLL_REQUIRE(max_attempts >= 1024, "the attempt cap must be at least 1024");
    if (n == 0) return DGLL_OK;
    uint64_t T[3];
    thresholds(p, q, T);
    const int biased = !(p == 1.0 && q == 1.0);
    hipLaunchKernelGGL(walk::random_walk_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       rowptr, col, n_nodes, starts, n, length, first_walk_index, seed, T[0], T[1], T[2], biased, max_attempts, walks,
                       reinterpret_cast<unsigned long long*>(info));
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_alias_build(void* stream, const int64_t* rowptr, const float* val, int64_t n_rows, int64_t nnz, void* scratch,
                                  size_t scratch_bytes, uint32_t* table, int64_t* info) {
    DGLL_REQUIRE(rowptr && info && ((val && scratch && table) || nnz == 0), "CSR, scratch, table and info must be non-NULL");
    DGLL_REQUIRE(n_rows >= 0 && n_rows <= (1ll << 31) * kBlock - kBlock && nnz >= 0, "row and edge counts must be >= 0");
    DGLL_REQUIRE(nnz == 0 || scratch_bytes / 12 >= (size_t)nnz, "scratch must hold 12 bytes per edge");
    DGLL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0 && (reinterpret_cast<uintptr_t>(table) & 7u) == 0,
                 "scratch and table must be 8-byte aligned");
    if (n_rows == 0 || nnz == 0) return DGLL_OK;
    double* q = static_cast<double*>(scratch);
    hipLaunchKernelGGL(walk::alias_build_kernel, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), rowptr, val, n_rows, q, reinterpret_cast<uint32_t*>(q + nnz),
                       reinterpret_cast<uint2*>(table), reinterpret_cast<unsigned long long*>(info));
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_random_walk_weighted(void* stream, const int64_t* rowptr, const int32_t* col, const uint32_t* table, int64_t n_nodes,
                                           const int64_t* starts, int64_t n, int length, uint64_t first_walk_index, uint64_t seed, double p,
                                           double q, int max_attempts, int32_t* walks, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && table && (starts || n == 0) && (walks || n == 0) && info,
                 "CSR, alias table, starts, walks and info must be non-NULL");
    DGLL_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, "the alias table must be 8-byte aligned");
    DGLL_REQUIRE(length >= 1, "walk length must be >= 1");
    DGLL_REQUIRE(p > 0.0 && q > 0.0 && isfinite(p) && isfinite(q), "node2vec p and q must be positive and finite");
    DGLL_REQUIRE(n >= 0 && n_nodes > 0 && n_nodes < (1ll << 31) && n <= (1ll << 31) * kBlock - kBlock, "walk count, node count < 2^31");
    DGLL_REQUIRE(max_attempts >= 1024, "the attempt cap must be at least 1024");
    if (n == 0) return DGLL_OK;
    uint64_t T[3];
    thresholds(p, q, T);
    const int biased = !(p == 1.0 && q == 1.0);
    hipLaunchKernelGGL(walk::random_walk_weighted_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), rowptr, col, reinterpret_cast<const uint2*>(table), n_nodes, starts, n, length,
                       first_walk_index, seed, T[0], T[1], T[2], biased, max_attempts, walks, reinterpret_cast<unsigned long long*>(info));
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_struc_walk(void* stream, const int64_t* rowptr, const int32_t* col, const uint32_t* table, const uint32_t* t_up,
                                 int64_t n_nodes, int n_layers, const int64_t* starts, int64_t n, int length, uint64_t first_walk_index,
                                 uint64_t seed, double stay_prob, int max_attempts, int32_t* walks, int32_t* layers_out, int64_t* info) {
    DGLL_REQUIRE(rowptr && (starts || n == 0) && (walks || n == 0) && info && t_up, "CSR, t_up, starts, walks and info must be non-NULL");
    DGLL_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0, "the alias table must be 8-byte aligned");
    DGLL_REQUIRE(length >= 1, "walk length must be >= 1");
    DGLL_REQUIRE(stay_prob >= 0.0 && stay_prob <= 1.0, "stay_prob must lie in [0, 1]");
    DGLL_REQUIRE(n >= 0 && n_nodes > 0 && n_nodes < (1ll << 31) && n <= (1ll << 31) * kBlock - kBlock, "walk count, node count < 2^31");
    DGLL_REQUIRE(n_layers >= 1 && max_attempts >= 1, "n_layers and the attempt cap must be >= 1");
    if (n == 0) return DGLL_OK;
    const uint64_t t_stay = (uint64_t)rint(4294967296.0 * stay_prob);
    hipLaunchKernelGGL(walk::struc_walk_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), rowptr, col, reinterpret_cast<const uint2*>(table), t_up, n_nodes, n_layers,
                       starts, n, length, first_walk_index, seed, t_stay, max_attempts, walks, layers_out,
                       reinterpret_cast<unsigned long long*>(info));
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_host_node2vec_thresholds(double p, double q, uint64_t* out3) {
    DGLL_REQUIRE(out3, "output must be non-NULL");
    DGLL_REQUIRE(p > 0.0 && q > 0.0 && isfinite(p) && isfinite(q), "node2vec p and q must be positive and finite");
    thresholds(p, q, out3);
    return DGLL_OK;
}
