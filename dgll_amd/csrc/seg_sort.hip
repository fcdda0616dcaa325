// seg_sort.hip -- dgll_hip_segment_sort, dgll_hip_pool_select, dgll_hip_pool_select_bwd: ordering the rows of every segment of a batch
// by a score, and the scaled gather (with its backward) that TopKPooling, SAGPooling and SortPooling put behind it.  The contract is in
// include/dgll_hip.h; DESIGN.md 4.4n says why the geometry is what it is.
//
// The order is built from ONE 64-bit key per row, smaller is better: the high word is a monotone DESCENDING image of the fp32 score
// (-0 counted as +0, every NaN as the largest word, behind -inf), the low word the row's offset inside its segment.  Keys are unique,
// so the bitonic network -- which is not stable -- still yields "score descending, ties to the smaller index".  Slots that hold no row
// carry the all-ones sentinel, larger than any key (an offset is < 2^31).
//
// Where the keys live.  A lane owns KPL consecutive slots of the network, slot i = t * KPL + u, in REGISTERS for the whole sort.  A
// compare-exchange at stride j therefore pairs
//     j < KPL                two registers of the same lane: no traffic at all;
//     KPL <= j < 64 KPL      the same register of lane t ^ (j / KPL) of the same wavefront: one cross-lane move, no LDS, no barrier;
//     j >= 64 KPL            the same register of a lane of another wavefront: the only stages that go through LDS (written
//                            transposed, s[u * 256 + t], so that neither side has bank conflicts) with two barriers each.
// With 4096 keys in a workgroup (KPL = 16) that is 3 LDS stages out of 78.  A segment of at most 64 rows is the case KPL = 1 of one
// wavefront: it never reaches the third tier, so the wave kernel has no LDS and no barrier, and four segments share a workgroup.
// A workgroup sorts only the power of two that covers its segment (fewer stages for a short segment in a wide instance).
//
// Segments longer than the tile: the tile kernel sorts runs of DGLL_SEGSORT_TILE keys into a scratch array, then ceil(log2(runs))
// merge launches go back and forth between two scratch arrays; a workgroup writes one tile of the output, every lane finding the
// start of its 16 outputs by a merge-path binary search over the two runs in memory.  Correct, not tuned.
// No atomics, no waiting on another workgroup: two runs give the same bits.
#include "common.hpp"

namespace dgll {
namespace segsort {

typedef unsigned long long key_t;
constexpr key_t kSentinel = ~0ull;
constexpr int kTile = DGLL_SEGSORT_TILE;
constexpr int kMaxKpl = kTile / kBlock;        // slots per lane of the widest instance
static_assert(kMaxKpl == 16, "the register tier below is written out for at most 16 slots per lane");

__device__ __forceinline__ float score_at(const void* score, int sdt, int64_t i) {
    return sdt == DGLL_BF16 ? bf16_to_f32(static_cast<const bf16_t*>(score)[i]) : static_cast<const float*>(score)[i];
}

__device__ __forceinline__ key_t make_key(float s, uint32_t local) {
    uint32_t bits = __float_as_uint(s), d = 0xffffffffu;                   // NaN: behind -inf (0xff800000)
    if (s == s) {
        if (bits == 0x80000000u) bits = 0u;                                // -0 is +0
        d = (bits & 0x80000000u) ? bits : bits ^ 0x7fffffffu;              // larger score, smaller word
    }
    return ((key_t)d << 32) | (key_t)local;
}

__device__ __forceinline__ void keep(key_t& mine, key_t other, bool keep_min) {
    const bool take = keep_min ? other < mine : other > mine;
    mine = take ? other : mine;
}

// stride J inside the lane's own registers
template <int KPL, int J>
__device__ __forceinline__ void reg_stage(key_t (&key)[KPL], int i0, int k) {
    if constexpr (J < KPL) {
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
            if ((u & J) == 0) {
                const bool asc = ((i0 + u) & k) == 0;
                const key_t a = key[u], b = key[u | J];
                const bool sw = (a > b) == asc;
                key[u] = sw ? b : a;
                key[u | J] = sw ? a : b;
            }
        }
    }
}

// stride pj * KPL: lane t ^ pj of the same wavefront (pj < 64)
template <int KPL>
__device__ __forceinline__ void shfl_stage(key_t (&key)[KPL], int t, int pj, int k) {
    const bool lower = (t & pj) == 0;
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const key_t other = __shfl_xor(key[u], pj);
        keep(key[u], other, lower == (((t * KPL + u) & k) == 0));
    }
}

// stride pj * KPL: lane t ^ pj of another wavefront of the workgroup
template <int KPL>
__device__ __forceinline__ void lds_stage(key_t (&key)[KPL], key_t* s, int t, int pj, int k) {
    const bool lower = (t & pj) == 0;
#pragma unroll
    for (int u = 0; u < KPL; ++u) s[u * kBlock + t] = key[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < KPL; ++u) keep(key[u], s[u * kBlock + (t ^ pj)], lower == (((t * KPL + u) & k) == 0));
    __syncthreads();                                    // the next stage writes the same slots
}

// ascending bitonic sort of the slots [0, npow2); slot t * KPL + u is key[u] of lane t.  npow2 is the same in every lane that runs
// the sort together (a workgroup with LDS, a wavefront without).
template <int KPL, bool LDS>
__device__ __forceinline__ void sort_slots(key_t (&key)[KPL], key_t* s, int t, int npow2) {
    const int i0 = t * KPL;
    for (int k = 2; k <= npow2; k <<= 1) {
        for (int j = k >> 1; j >= KPL; j >>= 1) {
            if (LDS && j >= KPL * kWave) lds_stage<KPL>(key, s, t, j / KPL, k);
            else shfl_stage<KPL>(key, t, j / KPL, k);
        }
        if (k > 8) reg_stage<KPL, 8>(key, i0, k);
        if (k > 4) reg_stage<KPL, 4>(key, i0, k);
        if (k > 2) reg_stage<KPL, 2>(key, i0, k);
        reg_stage<KPL, 1>(key, i0, k);
    }
}

struct Seg {
    int64_t b, size, o0, m;         // first row, rows, first output slot, outputs asked for (not yet cut to size)
};

__device__ __forceinline__ Seg segment_of(const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ out_ptr, int64_t s, int64_t n) {
    int64_t b = seg_ptr[s], e = seg_ptr[s + 1];
    if (b < 0) b = 0;
    if (b > n) b = n;
    if (e > n) e = n;
    Seg g;
    g.b = b;
    g.size = e > b ? e - b : 0;
    g.o0 = out_ptr[s];
    g.m = out_ptr[s + 1] - g.o0;
    return g;
}

// what the owner of segment s writes besides its order: -1 into the output slots behind the segment's size, and into the inverse
// entries of rows that no segment covers (in front of the first segment, behind the last)
__device__ __forceinline__ void write_extras(const Seg& g, int64_t s, int64_t n_segs, int64_t n, int64_t* __restrict__ out_idx,
                                             int32_t* __restrict__ out_inv, int64_t n_out, int t, int step) {
    int64_t lo = g.o0 + g.size, hi = g.o0 + g.m;
    if (lo < 0) lo = 0;
    if (hi > n_out) hi = n_out;
    for (int64_t q = lo + t; q < hi; q += step) out_idx[q] = -1;
    if (out_inv == nullptr) return;
    if (s == 0) for (int64_t r = t; r < g.b; r += step) out_inv[r] = -1;
    if (s == n_segs - 1) for (int64_t r = g.b + g.size + t; r < n; r += step) out_inv[r] = -1;
}

// the row that holds rank r of its segment
__device__ __forceinline__ void emit(const Seg& g, int64_t r, key_t key, int64_t* __restrict__ out_idx, int32_t* __restrict__ out_inv,
                                     int64_t n_out) {
    const int64_t row = g.b + (int64_t)(uint32_t)key, slot = g.o0 + r;
    if (row >= g.b + g.size) return;                    // never for a key this file made: a row of the segment or nothing
    const bool kept = r < g.m && slot >= 0 && slot < n_out;
    if (kept) out_idx[slot] = row;
    if (out_inv != nullptr) out_inv[row] = kept ? (int32_t)slot : -1;
}

// ---- segments of at most 64 rows: a wavefront each, registers and cross-lane moves only ------------------------------------------
__global__ __launch_bounds__(kBlock) void wave_sort_kernel(const void* __restrict__ score, int sdt, int64_t n,
                                                           const int64_t* __restrict__ seg_ptr, int64_t n_segs,
                                                           const int64_t* __restrict__ out_ptr, int64_t* __restrict__ out_idx,
                                                           int32_t* __restrict__ out_inv, int64_t n_out) {
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (s >= n_segs) return;                            // the whole wavefront leaves
    Seg g = segment_of(seg_ptr, out_ptr, s, n);
    write_extras(g, s, n_segs, n, out_idx, out_inv, n_out, lane, kWave);
    if (g.size > kWave) g.size = kWave;                 // the host chose this kernel from max_seg; stay in bounds
    const int size = (int)g.size;
    key_t key[1] = {lane < size ? make_key(score_at(score, sdt, g.b + lane), (uint32_t)lane) : kSentinel};
    int npow2 = 1;
    while (npow2 < size) npow2 <<= 1;
    sort_slots<1, false>(key, nullptr, lane, npow2);
    if (lane < size) emit(g, lane, key[0], out_idx, out_inv, n_out);
}

// ---- a workgroup per segment (LONG: per run of kTile rows of a segment; runs of a segment longer than the tile go to `runs`) ----------
template <int KPL, bool LONG>
__global__ __launch_bounds__(kBlock) void tile_sort_kernel(const void* __restrict__ score, int sdt, int64_t n,
                                                           const int64_t* __restrict__ seg_ptr, int64_t n_segs,
                                                           const int64_t* __restrict__ out_ptr, int64_t* __restrict__ out_idx,
                                                           int32_t* __restrict__ out_inv, int64_t n_out, key_t* __restrict__ runs) {
    __shared__ key_t s_key[KPL * kBlock];
    constexpr int kCap = KPL * kBlock;
    const int t = (int)threadIdx.x;
    const int64_t s = blockIdx.x, r0 = LONG ? (int64_t)blockIdx.y * kCap : 0;
    Seg g = segment_of(seg_ptr, out_ptr, s, n);
    if (r0 == 0) write_extras(g, s, n_segs, n, out_idx, out_inv, n_out, t, kBlock);
    if (!LONG && g.size > kCap) g.size = kCap;          // the host chose KPL from max_seg; stay in bounds
    if (r0 >= g.size) return;                           // the whole workgroup leaves
    const int cnt = (int)(g.size - r0 < kCap ? g.size - r0 : kCap);
    int npow2 = 1;
    while (npow2 < cnt) npow2 <<= 1;
    // coalesced load: the lanes that hold slots below npow2 read consecutive rows; which slot a row starts in does not matter
    const int active = npow2 > KPL ? npow2 / KPL : 1;
    key_t key[KPL];
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const int el = u * active + t;
        key[u] = (t < active && el < cnt) ? make_key(score_at(score, sdt, g.b + r0 + el), (uint32_t)(r0 + el)) : kSentinel;
    }
    sort_slots<KPL, true>(key, s_key, t, npow2);
    const bool to_runs = LONG && g.size > kCap;
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const int i = t * KPL + u;
        if (i < cnt) {
            if (to_runs) runs[g.b + r0 + i] = key[u];
            else emit(g, i, key[u], out_idx, out_inv, n_out);
        }
    }
}

// ---- one merge pass over the segments longer than the tile: runs of L keys of src, pairwise, into dst (LAST: into the outputs) ------
template <bool LAST>
__global__ __launch_bounds__(kBlock) void merge_kernel(const key_t* __restrict__ src, key_t* __restrict__ dst, int64_t n,
                                                       const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ out_ptr,
                                                       int64_t* __restrict__ out_idx, int32_t* __restrict__ out_inv, int64_t n_out,
                                                       int64_t L) {
    const int t = (int)threadIdx.x;
    const Seg g = segment_of(seg_ptr, out_ptr, blockIdx.x, n);
    const int64_t t0 = (int64_t)blockIdx.y * kTile;
    if (g.size <= kTile || t0 >= g.size) return;        // a one-run segment was finished by the tile kernel
    const int64_t base = t0 / (2 * L) * (2 * L);
    const int64_t a1 = base + L < g.size ? base + L : g.size, b1 = base + 2 * L < g.size ? base + 2 * L : g.size;
    const int64_t lenA = a1 - base, lenB = b1 - a1;     // lenB == 0: an odd run at the end, copied through
    const key_t* __restrict__ A = src + g.b + base;
    const key_t* __restrict__ B = src + g.b + a1;
    const int64_t d = t0 - base + (int64_t)t * kMaxKpl;  // this lane's first output of the pair
    if (d >= lenA + lenB) return;
    const int cnt = (int)(lenA + lenB - d < kMaxKpl ? lenA + lenB - d : kMaxKpl);
    int64_t lo = d > lenB ? d - lenB : 0, hi = d < lenA ? d : lenA;
    while (lo < hi) {                                   // merge path: how many of the first d outputs come from A
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] < B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    int64_t ai = lo, bi = d - lo;
    key_t ka = ai < lenA ? A[ai] : kSentinel, kb = bi < lenB ? B[bi] : kSentinel;
    for (int c = 0; c < cnt; ++c) {
        const bool from_a = ka < kb;                    // keys are unique and smaller than the sentinel
        const key_t key = from_a ? ka : kb;
        if (from_a) { ++ai; ka = ai < lenA ? A[ai] : kSentinel; }
        else { ++bi; kb = bi < lenB ? B[bi] : kSentinel; }
        if (LAST) emit(g, base + d + c, key, out_idx, out_inv, n_out);
        else dst[g.b + base + d + c] = key;
    }
}

// ---- the scaled gather and its backward --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float act_of(int act, float s) {
    if (act == DGLL_POOL_ACT_TANH) return tanhf(s);
    if (act == DGLL_POOL_ACT_SIGMOID) return 1.0f / (1.0f + expf(-s));
    return act == DGLL_POOL_ACT_IDENTITY ? s : 1.0f;
}
// d act / d s from a = act(s)
__device__ __forceinline__ float dact_of(int act, float a) {
    if (act == DGLL_POOL_ACT_TANH) return 1.0f - a * a;
    if (act == DGLL_POOL_ACT_SIGMOID) return a * (1.0f - a);
    return act == DGLL_POOL_ACT_IDENTITY ? 1.0f : 0.0f;
}

// vector `vec` of a row as fp32, zeros from column feat on (EPV == 1: one column, nothing behind it is touched)
template <typename T, int EPV>
__device__ __forceinline__ void load_masked(const T* __restrict__ row, int vec, int feat, float (&f)[EPV]) {
    VecIO<T, EPV>::unpack(VecIO<T, EPV>::load(row + (int64_t)vec * EPV), f);
    const int left = feat - vec * EPV;
    if (left < EPV) {
#pragma unroll
        for (int j = 0; j < EPV; ++j) f[j] = j < left ? f[j] : 0.0f;
    }
}

// `group` lanes (a power of two <= 64) per output row j: out[j, :] = x[idx[j], :] * act(score[idx[j]]); idx[j] outside [0, n): zeros
template <typename T, int EPV>
__global__ __launch_bounds__(kBlock) void select_fwd_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int feat,
                                                            const void* __restrict__ score, int sdt, int act,
                                                            const int64_t* __restrict__ idx, int64_t n_out, int group,
                                                            T* __restrict__ out, int64_t ldo) {
    const int lane = lane_id(), gl = lane & (group - 1), per_wave = kWave / group, n_vec = (feat + EPV - 1) / EPV;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t j0 = wave * per_wave; j0 < n_out; j0 += waves * per_wave) {
        const int64_t j = j0 + lane / group;
        if (j >= n_out) continue;
        const int64_t i = idx[j];
        const bool ok = i >= 0 && i < n;
        const float mult = (ok && act != DGLL_POOL_ACT_NONE) ? act_of(act, score_at(score, sdt, i)) : 1.0f;
        for (int v = gl; v < n_vec; v += group) {
            float f[EPV];
            if (ok) {
                load_masked<T, EPV>(x + i * ldx, v, feat, f);
#pragma unroll
                for (int c = 0; c < EPV; ++c) f[c] *= mult;
            } else {
#pragma unroll
                for (int c = 0; c < EPV; ++c) f[c] = 0.0f;
            }
            VecIO<T, EPV>::store(out + j * ldo + (int64_t)v * EPV, f);        // whole vectors: the padding of out's rows is its own
        }
    }
}

// `group` lanes per row i of x, rows in order: j = inv[i] >= 0: grad_x[i] = g[j] * act(s_i), grad_score[i] = act'(s_i) <g[j], x[i]>;
// every other row: zeros
template <typename T, int EPV>
__global__ __launch_bounds__(kBlock) void select_bwd_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int feat,
                                                            const void* __restrict__ score, int sdt, int act,
                                                            const int32_t* __restrict__ inv, const T* __restrict__ g, int64_t ldg,
                                                            int64_t n_out, int group, T* __restrict__ gx, int64_t ldgx,
                                                            float* __restrict__ gs) {
    const int lane = lane_id(), gl = lane & (group - 1), per_wave = kWave / group, n_vec = (feat + EPV - 1) / EPV;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t i0 = wave * per_wave; i0 < n; i0 += waves * per_wave) {      // i0 is the same in the whole wavefront
        const int64_t i = i0 + lane / group;
        const bool live = i < n;
        const int64_t j = live ? (int64_t)inv[i] : -1;
        const bool kept = j >= 0 && j < n_out;
        const float a = (kept && act != DGLL_POOL_ACT_NONE) ? act_of(act, score_at(score, sdt, i)) : 1.0f;
        float dot = 0.0f;
        if (live) {
            for (int v = gl; v < n_vec; v += group) {
                float gv[EPV];
#pragma unroll
                for (int c = 0; c < EPV; ++c) gv[c] = 0.0f;
                if (kept) {
                    load_masked<T, EPV>(g + j * ldg, v, feat, gv);
                    if (gs != nullptr) {
                        float xv[EPV];
                        load_masked<T, EPV>(x + i * ldx, v, feat, xv);
#pragma unroll
                        for (int c = 0; c < EPV; ++c) dot = fmaf(gv[c], xv[c], dot);
                    }
#pragma unroll
                    for (int c = 0; c < EPV; ++c) gv[c] *= a;
                }
                if (gx != nullptr) VecIO<T, EPV>::store(gx + i * ldgx + (int64_t)v * EPV, gv);
            }
        }
        for (int o = group >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);   // every lane of the wavefront is here
        if (live && gl == 0 && gs != nullptr) gs[i] = kept ? dact_of(act, a) * dot : 0.0f;
    }
}

inline int group_for(int n_vec) {
    int g = 1;
    while (g < n_vec && g < kWave) g <<= 1;
    return g;
}

inline unsigned row_grid(int64_t rows, int group) {
    const int64_t per_block = (int64_t)kWavesPerBlock * (kWave / group);
    const int64_t blocks = (rows + per_block - 1) / per_block;
    return (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
}

template <typename T>
static inline bool rows_vec16(const T* p, int64_t ld) { return p == nullptr || (aligned16(p) && ((size_t)ld * sizeof(T)) % 16 == 0); }

template <typename T, int EPV>
void launch_select(hipStream_t st, const void* x, int64_t ldx, int64_t n, int feat, const void* score, int sdt, int act, const int64_t* idx,
                   int64_t n_out, void* out, int64_t ldo) {
    const int group = group_for((feat + EPV - 1) / EPV);
    hipLaunchKernelGGL((select_fwd_kernel<T, EPV>), dim3(row_grid(n_out, group)), dim3(kBlock), 0, st, static_cast<const T*>(x), ldx, n, feat,
                       score, sdt, act, idx, n_out, group, static_cast<T*>(out), ldo);
}

template <typename T, int EPV>
void launch_select_bwd(hipStream_t st, const void* x, int64_t ldx, int64_t n, int feat, const void* score, int sdt, int act,
                       const int32_t* inv, const void* g, int64_t ldg, int64_t n_out, void* gx, int64_t ldgx, float* gs) {
    const int group = group_for((feat + EPV - 1) / EPV);
    hipLaunchKernelGGL((select_bwd_kernel<T, EPV>), dim3(row_grid(n, group)), dim3(kBlock), 0, st, static_cast<const T*>(x), ldx, n, feat,
                       score, sdt, act, inv, static_cast<const T*>(g), ldg, n_out, group, static_cast<T*>(gx), ldgx, gs);
}

template <int KPL>
void launch_tile(hipStream_t st, int64_t n_segs, const void* score, int sdt, int64_t n, const int64_t* seg_ptr, const int64_t* out_ptr,
                 int64_t* out_idx, int32_t* out_inv, int64_t n_out) {
    hipLaunchKernelGGL((tile_sort_kernel<KPL, false>), dim3((unsigned)n_segs), dim3(kBlock), 0, st, score, sdt, n, seg_ptr, n_segs, out_ptr,
                       out_idx, out_inv, n_out, (key_t*)nullptr);
}

}  // namespace segsort
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_segment_sort(void* stream, const void* score, int score_dtype, int64_t n, const int64_t* seg_ptr, int64_t n_segs,
                                   int64_t max_seg, const int64_t* out_ptr, int64_t* out_idx, int32_t* out_inv, int64_t n_out,
                                   void* scratch) {
    using namespace segsort;
    DGLL_REQUIRE(score_dtype == DGLL_F32 || score_dtype == DGLL_BF16, "dgll_hip_segment_sort: score_dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "dgll_hip_segment_sort: n must be in [0, 2^31)");
    DGLL_REQUIRE(n_segs >= 0 && n_segs < (int64_t(1) << 31) && n_out >= 0 && n_out < (int64_t(1) << 31) && max_seg >= 0,
                 "dgll_hip_segment_sort: n_segs and n_out must be in [0, 2^31), max_seg >= 0");
    if (n == 0 || n_segs == 0 || n_out == 0) return DGLL_OK;
    DGLL_REQUIRE(score != nullptr && seg_ptr != nullptr && out_ptr != nullptr && out_idx != nullptr,
                 "dgll_hip_segment_sort: score, seg_ptr, out_ptr and out_idx must be non-NULL");
    const int64_t n_runs = (max_seg + kTile - 1) / kTile;
    DGLL_REQUIRE(n_runs <= 1 || scratch != nullptr,
                 "dgll_hip_segment_sort: a segment of more than 4096 rows (DGLL_SEGSORT_TILE) needs the scratch array of 16 n bytes");
    DGLL_REQUIRE(n_runs <= 65535, "dgll_hip_segment_sort: max_seg must be at most 65535 * DGLL_SEGSORT_TILE");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (max_seg <= kWave) {
        const unsigned grid = (unsigned)((n_segs + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(wave_sort_kernel, dim3(grid), dim3(kBlock), 0, st, score, score_dtype, n, seg_ptr, n_segs, out_ptr, out_idx, out_inv,
                           n_out);
    } else if (n_runs <= 1) {
        if (max_seg <= 1 * kBlock) launch_tile<1>(st, n_segs, score, score_dtype, n, seg_ptr, out_ptr, out_idx, out_inv, n_out);
        else if (max_seg <= 2 * kBlock) launch_tile<2>(st, n_segs, score, score_dtype, n, seg_ptr, out_ptr, out_idx, out_inv, n_out);
        else if (max_seg <= 4 * kBlock) launch_tile<4>(st, n_segs, score, score_dtype, n, seg_ptr, out_ptr, out_idx, out_inv, n_out);
        else if (max_seg <= 8 * kBlock) launch_tile<8>(st, n_segs, score, score_dtype, n, seg_ptr, out_ptr, out_idx, out_inv, n_out);
        else launch_tile<16>(st, n_segs, score, score_dtype, n, seg_ptr, out_ptr, out_idx, out_inv, n_out);
    } else {
        segsort::key_t* buf[2] = {static_cast<segsort::key_t*>(scratch), static_cast<segsort::key_t*>(scratch) + n};
        const dim3 grid((unsigned)n_segs, (unsigned)n_runs);
        hipLaunchKernelGGL((tile_sort_kernel<kMaxKpl, true>), grid, dim3(kBlock), 0, st, score, score_dtype, n, seg_ptr, n_segs, out_ptr,
                           out_idx, out_inv, n_out, buf[0]);
        int pass = 0;
        for (int64_t L = kTile; L < max_seg; L *= 2, ++pass) {
            if (L * 2 >= max_seg) hipLaunchKernelGGL((merge_kernel<true>), grid, dim3(kBlock), 0, st, buf[pass & 1], buf[(pass + 1) & 1], n,
                                                     seg_ptr, out_ptr, out_idx, out_inv, n_out, L);
            else hipLaunchKernelGGL((merge_kernel<false>), grid, dim3(kBlock), 0, st, buf[pass & 1], buf[(pass + 1) & 1], n, seg_ptr, out_ptr,
                                    out_idx, out_inv, n_out, L);
        }
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

static int pool_select_check(const char* who, int dtype, int score_dtype, int act, int64_t n, int64_t F, int64_t n_out) {
    const std::string w(who);
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, w + ": dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(score_dtype == DGLL_F32 || score_dtype == DGLL_BF16, w + ": score_dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(act >= DGLL_POOL_ACT_NONE && act <= DGLL_POOL_ACT_SIGMOID, w + ": act must be one of DGLL_POOL_ACT_*");
    DGLL_REQUIRE(n >= 0 && n < (int64_t(1) << 31) && n_out >= 0 && n_out < (int64_t(1) << 31), w + ": n and n_out must be in [0, 2^31)");
    DGLL_REQUIRE(F >= 1 && F <= DGLL_POOL_MAX_F, w + ": F must be in [1, 65536] (DGLL_POOL_MAX_F)");
    return DGLL_OK;
}

DGLL_API int dgll_hip_pool_select(void* stream, const void* x, int64_t ld_x, int dtype, int64_t n, int64_t F, const void* score,
                                  int score_dtype, int act, const int64_t* idx, int64_t n_out, void* out, int64_t ld_out) {
    using namespace segsort;
    if (int rc = pool_select_check("dgll_hip_pool_select", dtype, score_dtype, act, n, F, n_out)) return rc;
    DGLL_REQUIRE(ld_x >= F && ld_out >= F, "dgll_hip_pool_select: the row pitches ld_x and ld_out must be >= F");
    if (n_out == 0) return DGLL_OK;
    DGLL_REQUIRE(idx != nullptr && out != nullptr && (n == 0 || x != nullptr) && (act == DGLL_POOL_ACT_NONE || n == 0 || score != nullptr),
                 "dgll_hip_pool_select: x, idx and out (and score unless act is DGLL_POOL_ACT_NONE) must be non-NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DGLL_F32) {
        if (rows_vec16((const float*)x, ld_x) && rows_vec16((const float*)out, ld_out))
            launch_select<float, 4>(st, x, ld_x, n, (int)F, score, score_dtype, act, idx, n_out, out, ld_out);
        else launch_select<float, 1>(st, x, ld_x, n, (int)F, score, score_dtype, act, idx, n_out, out, ld_out);
    } else {
        if (rows_vec16((const bf16_t*)x, ld_x) && rows_vec16((const bf16_t*)out, ld_out))
            launch_select<bf16_t, 8>(st, x, ld_x, n, (int)F, score, score_dtype, act, idx, n_out, out, ld_out);
        else launch_select<bf16_t, 1>(st, x, ld_x, n, (int)F, score, score_dtype, act, idx, n_out, out, ld_out);
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_pool_select_bwd(void* stream, const void* x, int64_t ld_x, int dtype, int64_t n, int64_t F, const void* score,
                                      int score_dtype, int act, const int32_t* inv, const void* g, int64_t ld_g, int64_t n_out,
                                      void* grad_x, int64_t ld_grad_x, float* grad_score) {
    using namespace segsort;
    if (int rc = pool_select_check("dgll_hip_pool_select_bwd", dtype, score_dtype, act, n, F, n_out)) return rc;
    DGLL_REQUIRE(ld_x >= F && ld_g >= F && (grad_x == nullptr || ld_grad_x >= F),
                 "dgll_hip_pool_select_bwd: the row pitches ld_x, ld_g and ld_grad_x must be >= F");
    if (n == 0 || (grad_x == nullptr && grad_score == nullptr)) return DGLL_OK;
    DGLL_REQUIRE(inv != nullptr && x != nullptr && (n_out == 0 || g != nullptr) && (act == DGLL_POOL_ACT_NONE || score != nullptr),
                 "dgll_hip_pool_select_bwd: x, inv and g (and score unless act is DGLL_POOL_ACT_NONE) must be non-NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == DGLL_F32) {
        if (rows_vec16((const float*)x, ld_x) && rows_vec16((const float*)g, ld_g) && rows_vec16((const float*)grad_x, ld_grad_x))
            launch_select_bwd<float, 4>(st, x, ld_x, n, (int)F, score, score_dtype, act, inv, g, ld_g, n_out, grad_x, ld_grad_x, grad_score);
        else launch_select_bwd<float, 1>(st, x, ld_x, n, (int)F, score, score_dtype, act, inv, g, ld_g, n_out, grad_x, ld_grad_x, grad_score);
    } else {
        if (rows_vec16((const bf16_t*)x, ld_x) && rows_vec16((const bf16_t*)g, ld_g) && rows_vec16((const bf16_t*)grad_x, ld_grad_x))
            launch_select_bwd<bf16_t, 8>(st, x, ld_x, n, (int)F, score, score_dtype, act, inv, g, ld_g, n_out, grad_x, ld_grad_x, grad_score);
        else launch_select_bwd<bf16_t, 1>(st, x, ld_x, n, (int)F, score, score_dtype, act, inv, g, ld_g, n_out, grad_x, ld_grad_x, grad_score);
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
