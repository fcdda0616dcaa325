// walk.hip -- uniform (DeepWalk) and second-order (node2vec) random walks over a device CSR.
//
// One lane per walk.  A step is pointer chasing: rowptr[v], rowptr[v + 1] (one load level), then col[b + r] (a second, dependent
// level); the biased step adds, per attempt, a binary search of the candidate in the previous node's sorted row (log2 deg(t)
// dependent loads).  Nothing overlaps inside a walk, so the kernel is bound by the latency of those dependent loads times the
// walks in flight; a lane whose walk has hit a dead end idles until the longest walk of its wavefront ends.
// Every random word is Philox4x32-10 with key = seed and counter = (walk index lo, walk index hi, step, attempt): walk i is the
// same whichever launch, batch or batch size draws it.  Every decision is an integer compare (mulhi for the candidate, x1 < T for
// the acceptance), so a host restatement is bit-exact.
#include <math.h>

#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace walk {

enum { kInfoCapped = 0, kInfoErr = 1 };
enum { kErrStart = 1, kErrCol = 2 };

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

DGLL_API int dgll_host_node2vec_thresholds(double p, double q, uint64_t* out3) {
    DGLL_REQUIRE(out3, "output must be non-NULL");
    DGLL_REQUIRE(p > 0.0 && q > 0.0 && isfinite(p) && isfinite(q), "node2vec p and q must be positive and finite");
    thresholds(p, q, out3);
    return DGLL_OK;
}
