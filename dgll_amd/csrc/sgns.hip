// sgns.hip -- one batch-synchronous SGD step of skip-gram with negative sampling over a batch of walks.
//
// Pairs are enumerated from the walks inside the kernels (no pair list): centre = position j of walk w, context slot s in [0, 2W)
// = position j + o(s), o = -W..-1, 1..W, inside the walk and not -1.  Each pair has K negatives drawn by inverse CDF over the
// noise table (uint64 fixed point scaled to 2^32, searchsorted side = right on one Philox word, counter = (walk index lo, hi,
// j * 2W + s, k | 2^31)); a negative equal to the pair's context gets coefficient 0.  All gradients are taken at the weights as
// the step found them, so the three passes are:
//   scores   a lane group per centre: gather u_c = W_in[c]; for every target gather v, dot, g = sigma(.) - label; the centre's
//            delta sum_t g_t v_t stays in registers (in LDS beyond 4 dwords per lane); g, the target ids and delta go to scratch
//            with plain stores; the loss is reduced per workgroup in fp64
//   out      a lane group per position p: the positive updates that share the destination walk[p] (up to 2W centres) are summed
//            in registers, then one atomic row add; every negative of centre p is one atomic row add of g u_p
//   in       W_in[c] -= lr delta (atomics: a node is the centre at several positions of a batch)
// Global fp32 atomics run at the memory side: every atomic wave-instruction here is one contiguous row segment (lanes run across
// D), the full-rate shape; one lane per row is an order of magnitude slower.
#include <math.h>

#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace sgns {

constexpr int kE = 4;          // dwords of a row one lane keeps in registers
constexpr int kMaxDim = 4032;  // the deltas of a workgroup's four centres fit 64 KB of LDS

// first index whose cumulative weight exceeds x: searchsorted(cdf, x, side = "right"); cdf[n - 1] = 2^32 > x
__device__ __forceinline__ int32_t noise_draw(const uint64_t* __restrict__ cdf, int64_t n, uint64_t widx, uint32_t pair, uint32_t k,
                                              uint64_t seed) {
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const uint32_t ctr[4] = {(uint32_t)widx, (uint32_t)(widx >> 32), pair, k | 0x80000000u};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] > (uint64_t)x[0]) hi = mid; else lo = mid + 1;
    }
    return (int32_t)lo;
}

// node at position j of walk w, -1 outside the walk, after a dead end or for an id outside the tables
__device__ __forceinline__ int32_t node_at(const int32_t* __restrict__ walks, int64_t w, int j, int L, int64_t n_nodes) {
    if (j < 0 || j >= L) return -1;
    const int32_t v = walks[w * L + j];
    return (v < 0 || v >= n_nodes) ? -1 : v;
}

__device__ __forceinline__ int slot_offset(int s, int W) { return s < W ? s - W : s - W + 1; }
__device__ __forceinline__ int offset_slot(int o, int W) { return o < 0 ? o + W : o + W - 1; }

__global__ __launch_bounds__(kBlock) void negatives_kernel(const int32_t* __restrict__ walks, int64_t n, int L, int W, int K,
                                                           const uint64_t* __restrict__ cdf, int64_t n_nodes, uint64_t first,
                                                           uint64_t seed, int32_t* __restrict__ out) {
    const int64_t total = n * L * 2 * W * K;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int k = (int)(i % K);
        const int64_t pr = i / K;
        const int s = (int)(pr % (2 * W));
        const int64_t c = pr / (2 * W);
        const int j = (int)(c % L);
        const int64_t w = c / L;
        const bool pair = node_at(walks, w, j, L, n_nodes) >= 0 && node_at(walks, w, j + slot_offset(s, W), L, n_nodes) >= 0;
        out[i] = pair ? noise_draw(cdf, n_nodes, first + (uint64_t)w, (uint32_t)(j * 2 * W + s), (uint32_t)k, seed) : -1;
    }
}

__device__ __forceinline__ float softplus(float x) { return x > 0.0f ? x + log1pf(expf(-x)) : log1pf(expf(x)); }

// GW lanes per centre; kLds: the delta lives in LDS (D > GW * kE), u_c is re-read (it stays in L1)
template <int GW, bool kLds>
__global__ __launch_bounds__(kBlock) void scores_kernel(const float* __restrict__ w_in, const float* __restrict__ w_out, int64_t n_nodes,
                                                        int D, const int32_t* __restrict__ walks, int64_t n, int L, int W, int K,
                                                        const uint64_t* __restrict__ cdf, uint64_t first, uint64_t seed,
                                                        float* __restrict__ g_out, int32_t* __restrict__ tgt_out,
                                                        float* __restrict__ delta_out, double* __restrict__ loss_out) {
    extern __shared__ float lds_acc[];
    __shared__ double red[kBlock / GW];
    const int gl = (int)(threadIdx.x % GW), grp = (int)(threadIdx.x / GW);
    const int64_t c = (int64_t)blockIdx.x * (kBlock / GW) + grp;
    const int T1 = 1 + K;
    double loss = 0.0;
    const int64_t w = c / L;
    const int j = (int)(c % L);
    const int32_t ctr = c < n * L ? node_at(walks, w, j, L, n_nodes) : -1;
    if (ctr >= 0) {
        const float* urow = w_in + (int64_t)ctr * D;
        float* accl = lds_acc + (size_t)grp * D;
        float u[kE], acc[kE];
        if (!kLds) {
#pragma unroll
            for (int e = 0; e < kE; ++e) { const int d = gl + e * GW; u[e] = d < D ? urow[d] : 0.0f; acc[e] = 0.0f; }
        } else {
            for (int d = gl; d < D; d += GW) accl[d] = 0.0f;
        }
        // one target: its dot with u_c, g, the loss term, the delta; lane 0 of the group records (g, id)
        auto target = [&](int32_t tgt, float label, float coef, int64_t at) {
            const float* vrow = w_out + (int64_t)tgt * D;
            float v[kE], part = 0.0f;
            if (!kLds) {
#pragma unroll
                for (int e = 0; e < kE; ++e) { const int d = gl + e * GW; v[e] = d < D ? vrow[d] : 0.0f; part = fmaf(u[e], v[e], part); }
            } else {
                for (int d = gl; d < D; d += GW) part = fmaf(urow[d], vrow[d], part);
            }
#pragma unroll
            for (int off = GW / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, GW);
            const float g = coef * (1.0f / (1.0f + expf(-part)) - label);
            if (!kLds) {
#pragma unroll
                for (int e = 0; e < kE; ++e) acc[e] = fmaf(g, v[e], acc[e]);
            } else {
                for (int d = gl; d < D; d += GW) accl[d] = fmaf(g, vrow[d], accl[d]);
            }
            if (gl == 0) {
                g_out[at] = g; tgt_out[at] = tgt;
                loss += (double)(coef * softplus(label != 0.0f ? -part : part));
            }
        };
        for (int s = 0; s < 2 * W; ++s) {
            const int32_t ctx = node_at(walks, w, j + slot_offset(s, W), L, n_nodes);
            if (ctx < 0) continue;
            const int64_t at = (c * 2 * W + s) * T1;
            target(ctx, 1.0f, 1.0f, at);
            for (int k0 = 0; k0 < K; k0 += GW) {          // the group's lanes draw GW negatives at a time
                const int32_t mine = k0 + gl < K ? noise_draw(cdf, n_nodes, first + (uint64_t)w, (uint32_t)(j * 2 * W + s),
                                                              (uint32_t)(k0 + gl), seed) : -1;
                const int lim = K - k0 < GW ? K - k0 : GW;
                for (int kk = 0; kk < lim; ++kk) {
                    const int32_t neg = __shfl(mine, kk, GW);
                    target(neg, 0.0f, neg == ctx ? 0.0f : 1.0f, at + 1 + k0 + kk);
                }
            }
        }
        float* drow = delta_out + c * D;
        if (!kLds) {
#pragma unroll
            for (int e = 0; e < kE; ++e) { const int d = gl + e * GW; if (d < D) drow[d] = acc[e]; }
        } else {
            for (int d = gl; d < D; d += GW) drow[d] = accl[d];
        }
    }
    if (gl == 0) red[grp] = loss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < kBlock / GW; ++i) sum += red[i];
        if (sum != 0.0) atomicAdd(loss_out, sum);
    }
}

// W_out: lanes across D in chunks of GW * kE, so any D runs through the same code
template <int GW>
__global__ __launch_bounds__(kBlock) void update_out_kernel(const float* __restrict__ w_in, float* __restrict__ w_out, int64_t n_nodes, int D,
                                                            const int32_t* __restrict__ walks, int64_t n, int L, int W, int K,
                                                            const float* __restrict__ g_in, const int32_t* __restrict__ tgt_in, float lr) {
    const int gl = (int)(threadIdx.x % GW), grp = (int)(threadIdx.x / GW);
    const int64_t c = (int64_t)blockIdx.x * (kBlock / GW) + grp;
    if (c >= n * L) return;
    const int T1 = 1 + K;
    const int64_t w = c / L;
    const int j = (int)(c % L);
    const int32_t me = node_at(walks, w, j, L, n_nodes);
    if (me < 0) return;
    for (int d0 = 0; d0 < D; d0 += GW * kE) {
        // as a context: sum over the centres whose window holds this position
        float acc[kE] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool any = false;
        for (int o = -W; o <= W; ++o) {
            if (o == 0) continue;
            const int32_t cen = node_at(walks, w, j - o, L, n_nodes);          // centre at j - o sees this position at offset o
            if (cen < 0) continue;
            const float g = g_in[((c - o) * 2 * W + offset_slot(o, W)) * T1];
            const float* urow = w_in + (int64_t)cen * D;
#pragma unroll
            for (int e = 0; e < kE; ++e) { const int d = d0 + gl + e * GW; if (d < D) acc[e] = fmaf(g, urow[d], acc[e]); }
            any = true;
        }
        float* orow = w_out + (int64_t)me * D;
        if (any) {
#pragma unroll
            for (int e = 0; e < kE; ++e) { const int d = d0 + gl + e * GW; if (d < D) atomicAdd(orow + d, -lr * acc[e]); }
        }
        // as a centre: every negative of its pairs
        float u[kE];
        const float* urow = w_in + (int64_t)me * D;
#pragma unroll
        for (int e = 0; e < kE; ++e) { const int d = d0 + gl + e * GW; u[e] = d < D ? urow[d] : 0.0f; }
        for (int s = 0; s < 2 * W; ++s) {
            if (node_at(walks, w, j + slot_offset(s, W), L, n_nodes) < 0) continue;
            const int64_t at = (c * 2 * W + s) * T1;
            for (int k = 1; k < T1; ++k) {
                const float g = g_in[at + k];
                if (g == 0.0f) continue;                     // coefficient 0 (the negative is the context), or sigma underflowed
                float* nrow = w_out + (int64_t)tgt_in[at + k] * D;
#pragma unroll
                for (int e = 0; e < kE; ++e) { const int d = d0 + gl + e * GW; if (d < D) atomicAdd(nrow + d, -lr * g * u[e]); }
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void update_in_kernel(float* __restrict__ w_in, int64_t n_nodes, int D, const int32_t* __restrict__ walks,
                                                           int64_t n, int L, const float* __restrict__ delta, float lr) {
    const int64_t total = n * L * D;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t c = i / D;
        const int32_t v = walks[c];
        if (v < 0 || v >= n_nodes) continue;
        const float x = delta[i];
        if (x != 0.0f) atomicAdd(w_in + (int64_t)v * D + (i - c * D), -lr * x);
    }
}

inline int group_width(int D) { return D <= 4 ? 4 : (D <= 16 ? 16 : 64); }

}  // namespace sgns
}  // namespace dgll

using namespace dgll;

#define SGNS_COMMON_CHECKS                                                                                                        \
    DGLL_REQUIRE(walks && cdf, "walks and the noise table must be non-NULL");                                                    \
    DGLL_REQUIRE(n >= 1 && length >= 1 && window >= 1 && negatives >= 0 && n_nodes > 0 && n_nodes < (1ll << 31),                  \
                 "walk count, walk length, window >= 1, negatives >= 0, node count < 2^31");                                      \
    DGLL_REQUIRE((int64_t)length * 2 * window < (1ll << 32) && n * length * 2 * window * (1 + negatives) < (1ll << 40),           \
                 "pair index fits 32 bits, batch scratch below 2^40 entries")

DGLL_API int dgll_hip_sgns_negatives(void* stream, const int32_t* walks, int64_t n, int length, int window, int negatives,
                                     const uint64_t* cdf, int64_t n_nodes, uint64_t first_walk_index, uint64_t seed, int32_t* out) {
    SGNS_COMMON_CHECKS;
    DGLL_REQUIRE(out && negatives >= 1, "output must be non-NULL, negatives >= 1");
    const int64_t total = n * length * 2 * window * negatives;
    const int64_t grid = (total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(sgns::negatives_kernel, dim3((unsigned)(grid > 65536 ? 65536 : grid)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       walks, n, length, window, negatives, cdf, n_nodes, first_walk_index, seed, out);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

template <int GW>
static int sgns_launch(hipStream_t st, float* w_in, float* w_out, int64_t n_nodes, int D, const int32_t* walks, int64_t n, int L, int W,
                       int K, const uint64_t* cdf, uint64_t first, uint64_t seed, float lr, float* g, int32_t* tgt, float* delta,
                       double* loss) {
    const int groups = kBlock / GW;
    const unsigned grid = (unsigned)((n * L + groups - 1) / groups);
    if (D <= GW * sgns::kE) {
        hipLaunchKernelGGL((sgns::scores_kernel<GW, false>), dim3(grid), dim3(kBlock), 0, st, w_in, w_out, n_nodes, D, walks, n, L, W, K, cdf,
                           first, seed, g, tgt, delta, loss);
    } else {
        hipLaunchKernelGGL((sgns::scores_kernel<GW, true>), dim3(grid), dim3(kBlock), (size_t)groups * D * sizeof(float), st, w_in, w_out,
                           n_nodes, D, walks, n, L, W, K, cdf, first, seed, g, tgt, delta, loss);
    }
    hipLaunchKernelGGL((sgns::update_out_kernel<GW>), dim3(grid), dim3(kBlock), 0, st, w_in, w_out, n_nodes, D, walks, n, L, W, K, g, tgt, lr);
    const int64_t total = n * L * D, blocks = (total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(sgns::update_in_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(kBlock), 0, st, w_in, n_nodes, D, walks, n,
                       L, delta, lr);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_sgns_step(void* stream, float* w_in, float* w_out, int64_t n_nodes, int dim, const int32_t* walks, int64_t n,
                                int length, int window, int negatives, const uint64_t* cdf, uint64_t first_walk_index, uint64_t seed,
                                float lr, float* g_scratch, int32_t* target_scratch, float* delta_scratch, double* loss) {
    SGNS_COMMON_CHECKS;
    DGLL_REQUIRE(w_in && w_out && g_scratch && target_scratch && delta_scratch && loss, "tables, scratch and loss must be non-NULL");
    DGLL_REQUIRE(dim >= 1 && dim <= sgns::kMaxDim, "embedding dimension in [1, 4032]");
    DGLL_REQUIRE(n * length < (1ll << 31) - kBlock, "at most 2^31 centre positions per step");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DGLL_HIP_TRY(hipMemsetAsync(loss, 0, sizeof(double), st));
    switch (sgns::group_width(dim)) {
        case 4: return sgns_launch<4>(st, w_in, w_out, n_nodes, dim, walks, n, length, window, negatives, cdf, first_walk_index, seed, lr,
                                      g_scratch, target_scratch, delta_scratch, loss);
        case 16: return sgns_launch<16>(st, w_in, w_out, n_nodes, dim, walks, n, length, window, negatives, cdf, first_walk_index, seed, lr,
                                        g_scratch, target_scratch, delta_scratch, loss);
        default: return sgns_launch<64>(st, w_in, w_out, n_nodes, dim, walks, n, length, window, negatives, cdf, first_walk_index, seed, lr,
                                        g_scratch, target_scratch, delta_scratch, loss);
    }
}
