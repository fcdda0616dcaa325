// edge_pred.hip -- link prediction on the device (dgll_amd/sampling/edge.py, dgll_amd/ops_pair.py).
//
// The graph is neighbor.hip's: a CSR of in-neighbours, entry e of row v is the edge col[e] -> v, and e IS the edge id.
//   dgll_hip_ep_draw            a lane per pair slot.  Slot p < B is positive p: u = col[e], v = the row of e (upper bound over rowptr,
//                               so runs of empty rows are stepped over).  Slot B + i * K + k is negative k of positive i: (u, c),
//                               c = mulhi32(word 0 of Philox(counter {e lo, e hi, k | 2^30, attempt}, key seed), N); with filtering a
//                               candidate whose row holds u (binary search, columns ascending within a row) is rejected, and after
//                               max_attempts rejections the last one is kept and counted.  Both endpoints set their bit in an N-bit
//                               bitmap (integer atomicOr; an epoch tag per node, never cleared, spares the atomic for a node that
//                               has set it already in this call).  Then one workgroup: popcount prefix per word, M into info.
//   dgll_hip_ep_compact         output_nodes = the set bits in ascending id order; local id of a node = prefix[word] + popcount(bits
//                               below): every global pair becomes a local one.
//   dgll_hip_ep_exclude_count   a lane group per block row: entries whose (dst, src) global key is in the sorted list of excluded
//   dgll_hip_ep_exclude_fill    keys (binary search) are dropped; count, one-workgroup scan, then the fill keeps the survivors in
//                               their order (ballot rank inside the group) and rewrites val = 1 / kept.
//   dgll_hip_pair_dot           a lane group per pair: score = <h[src], h[dst]>, 16-byte lane loads, fp32, xor-shuffle reduction.
//   dgll_hip_pair_dot_bwd       a lane group per node: grad_h[i] = sum over the node's incidence row, in its stored order, of
//                               g[pair] * h[other].  A gather: no float atomics, the same bits every run.
// Nothing depends on which thread wins: the bitmap is an OR, the tag is a filter in front of an idempotent OR (a lost race repeats
// the OR), the capped count and the error bits are integer atomics.
#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace ep {

constexpr int kGrid = 2048;            // grid-stride cap
enum { kInfoNodes = 0, kInfoCapped = 1, kInfoErr = 2, kInfoWords = 8 };
enum { kErrEdge = 1, kErrCol = 2 };
constexpr uint32_t kNegDomain = 0x40000000u;   // counter word 2: the neighbour sampler uses layer and layer | 2^31

inline int grid_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > kGrid ? kGrid : g));
}

__device__ __forceinline__ void flag(int64_t* info, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(info + kInfoErr), bit);
}

// v in [0, n_total)
__device__ __forceinline__ void touch(int64_t v, uint32_t* __restrict__ mark, uint32_t epoch, uint32_t* __restrict__ bitmap) {
    if (mark[v] != epoch) {
        mark[v] = epoch;
        atomicOr(bitmap + (v >> 5), 1u << (v & 31));
    }
}

// the row of entry e in [0, rowptr[n]): upper_bound(rowptr, e) - 1
__device__ __forceinline__ int64_t row_of_entry(const int64_t* __restrict__ rowptr, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;            // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// does row c (columns ascending) hold u?
__device__ __forceinline__ bool row_has(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t c, int32_t u) {
    int64_t lo = rowptr[c], hi = rowptr[c + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t x = col[mid];
        if (x == u) return true;
        if (x < u) lo = mid + 1; else hi = mid;
    }
    return false;
}

__global__ __launch_bounds__(kBlock) void draw_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_total,
                                                      int64_t nnz, const int64_t* __restrict__ edge_ids, int64_t n_edges, int negatives,
                                                      int filter, int max_attempts, uint64_t seed, uint32_t* __restrict__ mark,
                                                      uint32_t epoch, uint32_t* __restrict__ bitmap, int32_t* __restrict__ pairs,
                                                      int64_t* __restrict__ info) {
    const int64_t n_pairs = n_edges * (1 + (int64_t)negatives);
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n_pairs; p += (int64_t)gridDim.x * kBlock) {
        const bool positive = p < n_edges;
        const int64_t i = positive ? p : (p - n_edges) / negatives;
        const uint32_t k = positive ? 0u : (uint32_t)((p - n_edges) % negatives);
        const int64_t e = edge_ids[i];
        int32_t src = 0, dst = 0;
        bool ok = false;
        if (e < 0 || e >= nnz) {
            if (positive) flag(info, kErrEdge);
        } else {
            const int32_t u = col[e];
            if (u < 0 || u >= n_total) {
                if (positive) flag(info, kErrCol);
            } else if (positive) {
                src = u;
                dst = (int32_t)row_of_entry(rowptr, n_total, e);
                ok = true;
            } else {
                uint32_t c = 0;
                bool taken = false;
                for (int a = 0; a < max_attempts && !taken; ++a) {
                    const uint32_t ctr[4] = {(uint32_t)e, (uint32_t)((uint64_t)e >> 32), k | kNegDomain, (uint32_t)a};
                    uint32_t x[4];
                    philox4x32_10(ctr, key, x);
                    c = __umulhi(x[0], (uint32_t)n_total);
                    taken = !filter || !row_has(rowptr, col, c, u);
                }
                if (!taken) atomicAdd(reinterpret_cast<unsigned long long*>(info + kInfoCapped), 1ull);
                src = u;
                dst = (int32_t)c;
                ok = true;
            }
        }
        pairs[2 * p] = src;
        pairs[2 * p + 1] = dst;
        if (ok) {
            if (positive) touch(src, mark, epoch, bitmap);       // a negative's source is its positive's
            touch(dst, mark, epoch, bitmap);
        }
    }
}

// one workgroup: prefix[w] = set bits in words < w, their total into info[kInfoNodes]
__global__ __launch_bounds__(kBlock) void bitmap_scan_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words, int32_t* __restrict__ prefix,
                                                             int64_t* __restrict__ info) {
    __shared__ int64_t part[kBlock];
    const int t = threadIdx.x;
    const int64_t chunk = (n_words + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n_words ? t * chunk : n_words, hi = lo + chunk < n_words ? lo + chunk : n_words;
    int64_t sum = 0;
    for (int64_t w = lo; w < hi; ++w) sum += __popc(bitmap[w]);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        info[kInfoNodes] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t w = lo; w < hi; ++w) { prefix[w] = (int32_t)run; run += __popc(bitmap[w]); }
}

// output_nodes = set bits ascending; every global id of `pairs` to its rank among them
__global__ __launch_bounds__(kBlock) void compact_kernel(const uint32_t* __restrict__ bitmap, const int32_t* __restrict__ prefix,
                                                         int64_t n_words, int64_t n_total, int64_t n_nodes,
                                                         const int32_t* __restrict__ pairs, int64_t n_ids,
                                                         int64_t* __restrict__ output_nodes, int32_t* __restrict__ local_pairs) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t w = first; w < n_words; w += stride) {
        uint32_t bits = bitmap[w];
        int64_t k = prefix[w];
        while (bits && k < n_nodes) {
            output_nodes[k++] = w * 32 + (__ffs(bits) - 1);
            bits &= bits - 1u;
        }
    }
    for (int64_t j = first; j < n_ids; j += stride) {
        const int32_t c = pairs[j];
        int32_t l = 0;
        if (c >= 0 && c < n_total) l = prefix[c >> 5] + __popc(bitmap[c >> 5] & ((1u << (c & 31)) - 1u));
        local_pairs[j] = l;
    }
}

// ---- exclusion ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool excluded(const int64_t* __restrict__ keys, int64_t n_keys, int64_t key) {
    int64_t lo = 0, hi = n_keys;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t x = keys[mid];
        if (x == key) return true;
        if (x < key) lo = mid + 1; else hi = mid;
    }
    return false;
}

// is entry e of row r (global destination d) kept?  a local column outside the source list is kept as it is (never an index here)
__device__ __forceinline__ bool kept_entry(const int32_t* __restrict__ col, const int64_t* __restrict__ src_nodes, int64_t n_cols,
                                           int64_t n_total, const int64_t* __restrict__ keys, int64_t n_keys, int64_t d, int64_t e) {
    const int32_t c = col[e];
    if (c < 0 || c >= n_cols) return true;
    return !excluded(keys, n_keys, d * n_total + src_nodes[c]);
}

// FILL = false: out_rowptr[r + 1] = kept entries of row r.  FILL = true: out_rowptr is scanned; survivors in order, val = 1 / kept.
// A group of G lanes per row walks it G entries at a time; every lane of a wavefront runs every step.
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void exclude_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_rows,
                                                         const int64_t* __restrict__ src_nodes, int64_t n_cols, int64_t n_total,
                                                         const int64_t* __restrict__ keys, int64_t n_keys, int64_t* __restrict__ out_rowptr,
                                                         int64_t out_nnz, int32_t* __restrict__ out_col, float* __restrict__ out_val) {
    constexpr int kRowsPerWave = kWave / G;
    constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t r0 = wave * kRowsPerWave; r0 < n_rows; r0 += waves * kRowsPerWave) {
        const int64_t r = r0 + lane / G;
        const bool valid = r < n_rows;
        const int64_t b = valid ? rowptr[r] : 0, end = valid ? rowptr[r + 1] : 0;
        const int64_t d = valid ? src_nodes[r] : 0;              // the destinations are the first n_rows sources
        int64_t at = 0, total = 0;
        float v = 0.0f;
        if (FILL && valid) {
            at = out_rowptr[r];
            total = out_rowptr[r + 1] - at;
            v = total > 0 ? (float)(1.0 / (double)total) : 0.0f;
        }
        int64_t count = 0;
        for (int64_t base = b; __any(base < end); base += G) {
            const int64_t e = base + gl;
            const bool keep = e < end && kept_entry(col, src_nodes, n_cols, n_total, keys, n_keys, d, e);
            const unsigned long long m = (__ballot(keep) >> gbase) & kGroupMask;
            if (FILL && keep) {
                const int64_t o = at + count + __popcll(m & ((1ull << gl) - 1ull));
                if (o >= 0 && o < out_nnz) {                     // always, when out_rowptr is the count pass's under the same keys
                    out_col[o] = col[e];
                    if (out_val) out_val[o] = v;
                }
            }
            count += __popcll(m);
        }
        if (!FILL && valid && gl == 0) out_rowptr[r + 1] = count;
    }
}

// one workgroup: in-place inclusive scan of out_rowptr[1..n], out_rowptr[0] = 0, the total into info[0]
__global__ __launch_bounds__(kBlock) void scan_kernel(int64_t* __restrict__ out_rowptr, int64_t n_rows, int64_t* __restrict__ info) {
    __shared__ int64_t part[kBlock];
    const int t = threadIdx.x;
    const int64_t chunk = (n_rows + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n_rows ? t * chunk : n_rows, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += out_rowptr[i + 1];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        out_rowptr[0] = 0;
        info[0] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { run += out_rowptr[i + 1]; out_rowptr[i + 1] = run; }
}

// ---- pair scores ----------------------------------------------------------------------------------------------------------------
// Rows are read as 16-byte vectors of EPV elements (pitch and base 16-byte aligned); the columns of the last vector behind `feat` are
// masked, so the padding of a row may hold anything.  group: lanes per work item, a power of two <= 64.
template <typename T, int EPV>
__device__ __forceinline__ void load_masked(const T* __restrict__ row, int vec, int feat, float (&f)[EPV]) {
    VecIO<T, EPV>::unpack(VecIO<T, EPV>::load(row + (int64_t)vec * EPV), f);
    const int left = feat - vec * EPV;
    if (left < EPV) {
#pragma unroll
        for (int j = 0; j < EPV; ++j) f[j] = j < left ? f[j] : 0.0f;
    }
}

template <typename T, int EPV>
__global__ __launch_bounds__(kBlock) void pair_dot_kernel(const T* __restrict__ h, int64_t ldh, int64_t n_nodes, int feat,
                                                          const int32_t* __restrict__ pairs, int64_t n_pairs, int group,
                                                          float* __restrict__ score) {
    const int lane = lane_id(), gl = lane & (group - 1), per_wave = kWave / group, n_vec = (feat + EPV - 1) / EPV;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t p0 = wave * per_wave; p0 < n_pairs; p0 += waves * per_wave) {
        const int64_t p = p0 + lane / group;
        const int64_t a = p < n_pairs ? pairs[2 * p] : -1, b = p < n_pairs ? pairs[2 * p + 1] : -1;
        const bool ok = a >= 0 && a < n_nodes && b >= 0 && b < n_nodes;
        float acc = 0.0f;
        if (ok) {
            const T* ra = h + a * ldh;
            const T* rb = h + b * ldh;
            for (int v = gl; v < n_vec; v += group) {
                float x[EPV], y[EPV];
                load_masked<T, EPV>(ra, v, feat, x);
                load_masked<T, EPV>(rb, v, feat, y);
#pragma unroll
                for (int j = 0; j < EPV; ++j) acc = fmaf(x[j], y[j], acc);
            }
        }
        for (int o = group >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (p < n_pairs && gl == 0) score[p] = ok ? acc : __uint_as_float(0x7fc00000u);     // an id outside [0, M): NaN, nothing read
    }
}

template <typename T, int EPV>
__global__ __launch_bounds__(kBlock) void pair_dot_bwd_kernel(const T* __restrict__ h, int64_t ldh, int64_t n_nodes, int feat,
                                                              const int64_t* __restrict__ inc_rowptr, const int32_t* __restrict__ inc_pair,
                                                              const int32_t* __restrict__ inc_other, int64_t n_pairs,
                                                              const float* __restrict__ g, int group, T* __restrict__ grad,
                                                              int64_t ldg) {
    const int lane = lane_id(), gl = lane & (group - 1), per_wave = kWave / group, n_vec = (feat + EPV - 1) / EPV;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t i0 = wave * per_wave; i0 < n_nodes; i0 += waves * per_wave) {
        const int64_t i = i0 + lane / group;
        if (i >= n_nodes) continue;
        const int64_t b = inc_rowptr[i], end = inc_rowptr[i + 1];
        for (int v = gl; v < n_vec; v += group) {
            float acc[EPV];
#pragma unroll
            for (int j = 0; j < EPV; ++j) acc[j] = 0.0f;
            for (int64_t e = b; e < end; ++e) {                  // the stored order: ascending (pair, slot)
                const int64_t p = inc_pair[e], o = inc_other[e];
                if (p < 0 || p >= n_pairs || o < 0 || o >= n_nodes) continue;
                const float w = g[p];
                float x[EPV];
                load_masked<T, EPV>(h + o * ldh, v, feat, x);
#pragma unroll
                for (int j = 0; j < EPV; ++j) acc[j] = fmaf(w, x[j], acc[j]);
            }
            VecIO<T, EPV>::store(grad + i * ldg + (int64_t)v * EPV, acc);    // whole vectors: the padding of grad's rows is its own
        }
    }
}

inline int group_for(int n_vec) {
    int g = 1;
    while (g < n_vec && g < kWave) g <<= 1;
    return g;
}

}  // namespace ep
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_ep_draw(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, const int64_t* edge_ids,
                              int64_t n_edges, int negatives, int filter_existing, int max_attempts, uint64_t seed, uint32_t* mark,
                              uint32_t epoch, uint32_t* bitmap, int32_t* prefix, int32_t* pairs, int64_t pairs_cap, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && edge_ids && mark && bitmap && prefix && pairs && info,
                 "CSR, edge ids, mark / bitmap / prefix workspaces, pair output and info must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && nnz >= 0 && n_edges > 0 && n_edges < (1ll << 31) && epoch != 0,
                 "node count and edge-batch size in [1, 2^31), nnz >= 0, non-zero epoch");
    DGLL_REQUIRE(negatives >= 0 && max_attempts >= 1, "negatives >= 0 and max_attempts >= 1");
    const int64_t n_pairs = n_edges * (1 + (int64_t)negatives);
    DGLL_REQUIRE(n_pairs < (1ll << 31) && pairs_cap >= n_pairs, "the pairs buffer holds n_edges * (1 + negatives) < 2^31 pairs");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, ep::kInfoWords * sizeof(int64_t), st));
    DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st));
    hipLaunchKernelGGL(ep::draw_kernel, dim3(ep::grid_for(n_pairs, kBlock)), dim3(kBlock), 0, st, rowptr, col, n_total, nnz, edge_ids, n_edges,
                       negatives, filter_existing, max_attempts, seed, mark, epoch, bitmap, pairs, info);
    hipLaunchKernelGGL(ep::bitmap_scan_kernel, dim3(1), dim3(kBlock), 0, st, bitmap, n_words, prefix, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_ep_compact(void* stream, int64_t n_total, const uint32_t* bitmap, const int32_t* prefix, int64_t n_nodes,
                                 const int32_t* pairs, int64_t n_pairs, int64_t* output_nodes, int32_t* local_pairs) {
    DGLL_REQUIRE(bitmap && prefix && pairs && output_nodes && local_pairs,
                 "the bitmap and prefix of dgll_hip_ep_draw, its pairs, the node output and the local-pair output must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_nodes > 0 && n_nodes <= n_total && n_pairs > 0 && n_pairs < (1ll << 31),
                 "node count in [1, 2^31), 1 <= unique nodes <= node count, pair count in [1, 2^31)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32, work = n_words > 2 * n_pairs ? n_words : 2 * n_pairs;
    hipLaunchKernelGGL(ep::compact_kernel, dim3(ep::grid_for(work, kBlock)), dim3(kBlock), 0, st, bitmap, prefix, n_words, n_total, n_nodes,
                       pairs, 2 * n_pairs, output_nodes, local_pairs);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

static int exclude_check(const int64_t* rowptr, const int32_t* col, int64_t n_rows, const int64_t* src_nodes, int64_t n_cols, int64_t n_total,
                         const int64_t* keys, int64_t n_keys, const int64_t* out_rowptr) {
    DGLL_REQUIRE(rowptr && src_nodes && keys && out_rowptr, "block row pointers, source nodes, sorted keys and output row pointers must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_rows > 0 && n_rows <= n_cols && n_cols < (1ll << 31) && n_keys > 0,
                 "node count in [1, 2^31), 1 <= block rows <= block sources < 2^31, at least one key");
    (void)col;
    return DGLL_OK;
}

template <bool FILL>
static void exclude_launch(hipStream_t st, int64_t nnz_hint, const int64_t* rowptr, const int32_t* col, int64_t n_rows, const int64_t* src_nodes,
                           int64_t n_cols, int64_t n_total, const int64_t* keys, int64_t n_keys, int64_t* out_rowptr, int64_t out_nnz,
                           int32_t* out_col, float* out_val) {
    if (nnz_hint > 16 * n_rows)         // long rows on average (a copied fan-out -1 layer): a wavefront per row
        hipLaunchKernelGGL((ep::exclude_kernel<64, FILL>), dim3(ep::grid_for(n_rows, kBlock / 64)), dim3(kBlock), 0, st, rowptr, col, n_rows,
                           src_nodes, n_cols, n_total, keys, n_keys, out_rowptr, out_nnz, out_col, out_val);
    else
        hipLaunchKernelGGL((ep::exclude_kernel<16, FILL>), dim3(ep::grid_for(n_rows, kBlock / 16)), dim3(kBlock), 0, st, rowptr, col, n_rows,
                           src_nodes, n_cols, n_total, keys, n_keys, out_rowptr, out_nnz, out_col, out_val);
}

DGLL_API int dgll_hip_ep_exclude_count(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t nnz,
                                       const int64_t* src_nodes, int64_t n_cols, int64_t n_total, const int64_t* keys, int64_t n_keys,
                                       int64_t* out_rowptr, int64_t* info) {
    if (int rc = exclude_check(rowptr, col, n_rows, src_nodes, n_cols, n_total, keys, n_keys, out_rowptr)) return rc;
    DGLL_REQUIRE(info && nnz >= 0 && (nnz == 0 || col), "info must be non-NULL, nnz >= 0, columns non-NULL when there are entries");
    hipStream_t st = static_cast<hipStream_t>(stream);
    exclude_launch<false>(st, nnz, rowptr, col, n_rows, src_nodes, n_cols, n_total, keys, n_keys, out_rowptr, 0, nullptr, nullptr);
    hipLaunchKernelGGL(ep::scan_kernel, dim3(1), dim3(kBlock), 0, st, out_rowptr, n_rows, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_ep_exclude_fill(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int64_t nnz,
                                      const int64_t* src_nodes, int64_t n_cols, int64_t n_total, const int64_t* keys, int64_t n_keys,
                                      const int64_t* out_rowptr, int64_t out_nnz, int32_t* out_col, float* out_val) {
    if (int rc = exclude_check(rowptr, col, n_rows, src_nodes, n_cols, n_total, keys, n_keys, out_rowptr)) return rc;
    DGLL_REQUIRE(nnz >= 0 && out_nnz >= 0 && out_nnz <= nnz && (nnz == 0 || col) && (out_nnz == 0 || out_col),
                 "0 <= kept entries <= entries, columns and the column output non-NULL when there are entries");
    if (out_nnz == 0) return DGLL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    exclude_launch<true>(st, nnz, rowptr, col, n_rows, src_nodes, n_cols, n_total, keys, n_keys, const_cast<int64_t*>(out_rowptr), out_nnz,
                         out_col, out_val);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

static int pair_dot_check(const void* h, int64_t ldh, int64_t n_nodes, int feat, int dtype, int64_t n_pairs) {
    DGLL_REQUIRE(h != nullptr, "h must be non-NULL");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(feat >= 1 && n_nodes > 0 && n_nodes < (1ll << 31) && n_pairs > 0 && n_pairs < (1ll << 31),
                 "feat >= 1, node and pair counts in [1, 2^31)");
    const int epv = dtype == DGLL_F32 ? 4 : 8;
    DGLL_REQUIRE(aligned16(h) && ldh % epv == 0 && ldh >= feat, "rows of h: 16-byte aligned base, a pitch of whole 16-byte vectors >= feat");
    return DGLL_OK;
}

DGLL_API int dgll_hip_pair_dot(void* stream, const void* h, int64_t ldh, int64_t n_nodes, int feat, int dtype, const int32_t* pairs,
                               int64_t n_pairs, float* score) {
    DGLL_REQUIRE(pairs && score, "pairs and score must be non-NULL");
    if (int rc = pair_dot_check(h, ldh, n_nodes, feat, dtype, n_pairs)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int epv = dtype == DGLL_F32 ? 4 : 8, group = ep::group_for((feat + epv - 1) / epv);
    const int grid = ep::grid_for(n_pairs, kBlock / group);
    if (dtype == DGLL_F32)
        hipLaunchKernelGGL((ep::pair_dot_kernel<float, 4>), dim3(grid), dim3(kBlock), 0, st, static_cast<const float*>(h), ldh, n_nodes, feat,
                           pairs, n_pairs, group, score);
    else
        hipLaunchKernelGGL((ep::pair_dot_kernel<bf16_t, 8>), dim3(grid), dim3(kBlock), 0, st, static_cast<const bf16_t*>(h), ldh, n_nodes, feat,
                           pairs, n_pairs, group, score);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_pair_dot_bwd(void* stream, const void* h, int64_t ldh, int64_t n_nodes, int feat, int dtype, const int64_t* inc_rowptr,
                                   const int32_t* inc_pair, const int32_t* inc_other, int64_t n_pairs, const float* g, void* grad_h,
                                   int64_t ldg) {
    DGLL_REQUIRE(inc_rowptr && inc_pair && inc_other && g && grad_h, "incidence CSR, score gradient and grad_h must be non-NULL");
    if (int rc = pair_dot_check(h, ldh, n_nodes, feat, dtype, n_pairs)) return rc;
    const int epv = dtype == DGLL_F32 ? 4 : 8;
    DGLL_REQUIRE(aligned16(grad_h) && ldg % epv == 0 && ldg >= (feat + epv - 1) / epv * epv,
                 "rows of grad_h: 16-byte aligned base, a pitch of whole 16-byte vectors that covers feat rounded up to one");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int group = ep::group_for((feat + epv - 1) / epv);
    const int grid = ep::grid_for(n_nodes, kBlock / group);
    if (dtype == DGLL_F32)
        hipLaunchKernelGGL((ep::pair_dot_bwd_kernel<float, 4>), dim3(grid), dim3(kBlock), 0, st, static_cast<const float*>(h), ldh, n_nodes, feat,
                           inc_rowptr, inc_pair, inc_other, n_pairs, g, group, static_cast<float*>(grad_h), ldg);
    else
        hipLaunchKernelGGL((ep::pair_dot_bwd_kernel<bf16_t, 8>), dim3(grid), dim3(kBlock), 0, st, static_cast<const bf16_t*>(h), ldh, n_nodes,
                           feat, inc_rowptr, inc_pair, inc_other, n_pairs, g, group, static_cast<bf16_t*>(grad_h), ldg);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
