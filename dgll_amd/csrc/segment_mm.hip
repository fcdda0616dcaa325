// segment_mm.hip -- grouped dense products: y_i = x_i . W[type_i] over a set of rows (DGL's segment_mm / gather_mm / TypedLinear).
//
//   forward / input gradient   C[rows of segment r, N] = A[rows of segment r, K] . W_r[K, N]        dgll_hip_segment_mm
//   weight gradient            dW_r[K, N] = A_r^T . G_r, fp32, exactly zero for an empty segment    dgll_hip_segment_mm_gradw
//   weight pack                all R matrices, any strides (W_r or W_r^T), in one launch            dgll_hip_segment_mm_pack
//
// The kernels of dense.hip keep ONE weight resident in LDS for a persistent workgroup; here the weight changes every few rows, and
// how often is only known on the device.  What this file does instead:
//   * Tile list without the host.  A work item is (segment, 32-row tile of it).  Their number is at most ceil(M / 32) + R + 1, which
//     the host knows without reading the segment lengths; the grid is sized by that bound.  A one-workgroup plan kernel turns the
//     lengths into clamped offsets segoff[R + 2] and the tile prefix tileptr[R + 2]; every wave finds its segment by binary search in
//     tileptr and leaves when it is past the total.  Offsets are clamped to [0, M], so a wrong device seglen can address nothing
//     outside the operands; the rows no segment covers form a pseudo segment R whose tiles store zeros.
//   * A WAVE owns a tile: 32 rows x all N <= 256 columns in accumulators (weight = MFMA "A", activations = "B", as in
//     gemm_bf16_nt_kernel: a lane loads 16 bytes of its own row and ends up with 4-column pieces of that row).  The four waves of a
//     workgroup take four consecutive tiles of the list: inside a long segment that is 128 consecutive rows reading the same weight
//     addresses at the same time (one fetch from L2, the rest L1 hits); a 3-row segment costs one wave, not four.  No barrier.
//   * The weights are packed in MFMA FRAGMENT order instead of being staged through LDS: for (segment, k group, column tile) the 64
//     lanes' 16-byte fragments lie in lane order, so a weight fetch is one contiguous 1 KiB per wave instruction, no LDS, no bank
//     conflicts, nothing to restage when the segment changes.  The packed set is R K N elements; it is read from L2.
//   * A row-index operand `rows`: tile row t loads a[rows[t]] and stores c[rows[t]] -- gather_mm runs on the unsorted rows through the
//     sort permutation, with no permuted copy of a and no un-permute pass over c.
//   * bf16 on v_mfma_f32_32x32x16_bf16, fp32 on v_mfma_f32_32x32x2_f32 (exact fp32 FMA arithmetic), one template.
//   * Weight gradient: work item (segment, row slab); a workgroup stages 16 rows of a (128 columns) and g (all N) TRANSPOSED in LDS
//     (coalesced 16-byte row loads in, one 16-byte fragment read out), wave w owns k-tile w.  A segment of one slab writes dW_r
//     itself; longer ones write one fp32 partial per slab, summed in slab order by the finish kernel, which also zeroes the empty
//     segments.  No atomics: two runs give the same bits.
// Compiled without the packed fp32 instructions, from inside the file (as fps.hip): the common build flags stay as they are.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include <algorithm>

#include "common.hpp"

namespace dgll {
namespace segmm {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int kTileRows = 32;        // rows of a forward work item (one wave)
constexpr int kGwRows = 16;          // rows per LDS stage of the weight gradient
constexpr int kGwKBlock = 128;       // columns of a per workgroup of the weight gradient (32 per wave)
constexpr int kGwMinSlab = 512;      // rows per slab at the least
constexpr int kGwSlabsTarget = 128;  // slabs aimed at over all rows

template <typename T> struct Elem;
template <> struct Elem<bf16_t> { static constexpr int kPerLane = 8, kGroup = 16; };   // k per 16-byte fragment / per MFMA group
template <> struct Elem<float> { static constexpr int kPerLane = 4, kGroup = 8; };

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ int64_t load_index(const void* p, int bytes, int64_t i) {
    return bytes == 8 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
}

// ---- plan: lengths -> clamped offsets, tile prefix, partial-slot prefix (one workgroup) -------------------------------------------
// Element r < R is segment r; element R is the pseudo segment of the rows behind the last segment.  partptr counts the tiles of the
// segments that have more than one (the weight gradient's slab partials).
__global__ __launch_bounds__(kBlock) void segmm_plan_kernel(const void* __restrict__ seglen, int len_bytes, int64_t R, int64_t M, int unit,
                                                            int64_t* __restrict__ segoff, int32_t* __restrict__ tileptr,
                                                            int32_t* __restrict__ partptr) {
    __shared__ int64_t s_len[kBlock];
    __shared__ int64_t s_tiles[kBlock], s_parts[kBlock];
    const int tid = threadIdx.x;
    const int64_t per = (R + 1 + kBlock - 1) / kBlock;
    const int64_t r0 = min64(tid * per, R + 1), r1 = min64(r0 + per, R + 1);
    auto length = [&](int64_t r) {
        int64_t v = r < R ? load_index(seglen, len_bytes, r) : M;       // the pseudo segment takes whatever is left
        return v < 0 ? 0 : (v > M ? M : v);
    };
    int64_t sum = 0;
    for (int64_t r = r0; r < r1; ++r) sum += length(r);
    s_len[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < kBlock; ++i) { const int64_t v = s_len[i]; s_len[i] = run; run += v; }
    }
    __syncthreads();
    int64_t raw = s_len[tid], tiles = 0, parts = 0;
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t b = min64(raw, M);
        raw += length(r);
        const int64_t e = min64(raw, M);
        segoff[r] = b;
        if (r == R) segoff[R + 1] = M;
        const int64_t t = (e - b + unit - 1) / unit;
        tiles += t;
        parts += t > 1 ? t : 0;
    }
    s_tiles[tid] = tiles;
    s_parts[tid] = parts;
    __syncthreads();
    if (tid == 0) {
        int64_t run_t = 0, run_p = 0;
        for (int i = 0; i < kBlock; ++i) {
            const int64_t t = s_tiles[i], p = s_parts[i];
            s_tiles[i] = run_t; s_parts[i] = run_p;
            run_t += t; run_p += p;
        }
        tileptr[R + 1] = (int32_t)run_t;
        partptr[R + 1] = (int32_t)run_p;
    }
    __syncthreads();
    raw = s_len[tid];
    int64_t run_t = s_tiles[tid], run_p = s_parts[tid];
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t b = min64(raw, M);
        raw += length(r);
        const int64_t e = min64(raw, M);
        tileptr[r] = (int32_t)run_t;
        partptr[r] = (int32_t)run_p;
        const int64_t t = (e - b + unit - 1) / unit;
        run_t += t;
        run_p += t > 1 ? t : 0;
    }
}

// the segment of work item `item`: the s in [0, R] with tileptr[s] <= item < tileptr[s + 1] (item < tileptr[R + 1])
__device__ __forceinline__ int find_segment(const int32_t* __restrict__ tileptr, int R, int item) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tileptr[mid + 1] <= item) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- weight pack --------------------------------------------------------------------------------------------------------------
// packed[r][k group][column tile][lane] = 16 bytes: element e of lane (l32, half) is W_r[k = group * kGroup + half * kPerLane + e]
// [n = 32 tile + l32], zero past K or N.  src element (r, k, n) at r * sr + k * sk + n * sn: the strides choose W_r or W_r^T.
template <typename S, typename T>
__global__ __launch_bounds__(kBlock) void segmm_pack_kernel(const S* __restrict__ src, int64_t sr, int64_t sk, int64_t sn, int64_t total,
                                                            int K, int N, int groups, int nt, T* __restrict__ dst) {
    constexpr int KPL = Elem<T>::kPerLane, KG = Elem<T>::kGroup;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;       // fragment index
    if (i >= total) return;
    const int lane = (int)(i & 63);
    int64_t q = i >> 6;
    const int t = (int)(q % nt); q /= nt;
    const int gi = (int)(q % groups);
    const int64_t r = q / groups;
    const int n = t * 32 + (lane & 31), k0 = gi * KG + (lane >> 5) * KPL;
    float v[KPL];
#pragma unroll
    for (int e = 0; e < KPL; ++e) {
        v[e] = 0.0f;
        if (n < N && k0 + e < K) {
            const S x = src[r * sr + (int64_t)(k0 + e) * sk + (int64_t)n * sn];
            if constexpr (sizeof(S) == 2) v[e] = bf16_to_f32(x); else v[e] = x;
        }
    }
    if constexpr (sizeof(T) == 2)
        *reinterpret_cast<uint4*>(dst + i * 8) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                                            pack_bf16x2(v[6], v[7]));
    else
        *reinterpret_cast<float4*>(dst + i * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    const void* a;
    int64_t lda;
    const void* packed;
    const int64_t* segoff;
    const int32_t* tileptr;
    const void* rows;
    int rows_bytes;
    void* c;
    int64_t ldc;
    int64_t M;
    int R, K, N, groups, nt;
    int seg_begin, seg_end;      // the segments this launch computes; `packed` starts at seg_begin
};

template <typename T> __device__ __forceinline__ uint4 keep_first(uint4 v, int valid);      // the first `valid` elements, zeros behind
template <> __device__ __forceinline__ uint4 keep_first<bf16_t>(uint4 v, int valid) {
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] &= (2 * d < valid ? 0x0000ffffu : 0u) | (2 * d + 1 < valid ? 0xffff0000u : 0u);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <> __device__ __forceinline__ uint4 keep_first<float>(uint4 v, int valid) {
    return make_uint4(0 < valid ? v.x : 0u, 1 < valid ? v.y : 0u, 2 < valid ? v.z : 0u, 3 < valid ? v.w : 0u);
}

template <typename T> __device__ __forceinline__ f32x16_t mfma_group(uint4 w, uint4 x, f32x16_t acc);
template <> __device__ __forceinline__ f32x16_t mfma_group<bf16_t>(uint4 w, uint4 x, f32x16_t acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, x), acc, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16_t mfma_group<float>(uint4 w, uint4 x, f32x16_t acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.x), __uint_as_float(x.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.y), __uint_as_float(x.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.z), __uint_as_float(x.z), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.w), __uint_as_float(x.w), acc, 0, 0, 0);
}

template <typename T, int NT>
__global__ __launch_bounds__(kBlock) void segmm_fwd_kernel(const FwdArgs p) {
    constexpr int KPL = Elem<T>::kPerLane, KG = Elem<T>::kGroup;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t item64 = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (item64 >= p.tileptr[p.R + 1]) return;                       // (no barrier in this kernel: waves leave on their own)
    const int item = (int)item64;
    const int s = find_segment(p.tileptr, p.R, item);
    if (s == p.R ? p.seg_begin != 0 : (s < p.seg_begin || s >= p.seg_end)) return;      // another launch's segment (wave-uniform)
    const int64_t row0 = p.segoff[s] + (int64_t)(item - p.tileptr[s]) * kTileRows;
    const int64_t rend = p.segoff[s + 1];
    const int64_t trow = row0 + l32;
    const bool valid_row = trow < rend;
    const int64_t tld = valid_row ? trow : rend - 1;                // clamp loads, mask stores (row0 < rend: the tile exists)
    int64_t grow = p.rows ? load_index(p.rows, p.rows_bytes, tld) : tld;
    const bool ok = valid_row && grow >= 0 && grow < p.M;           // a row index outside the operands is neither read nor written
    grow = (grow >= 0 && grow < p.M) ? grow : 0;
    T* crow = static_cast<T*>(p.c) + grow * p.ldc;
    const bool cvec = (p.ldc * sizeof(T)) % (4 * sizeof(T)) == 0 && (reinterpret_cast<uintptr_t>(p.c) % (4 * sizeof(T))) == 0;

    if (s == p.R) {                                                 // rows no segment covers: zeros.  Deliberately the slow path (a lane per row,
                                                                    // scalar stores): it only runs for a device seglen whose sum is not M
        if (ok)
            for (int n = half; n < p.N; n += 2) crow[n] = (T)0;
        return;
    }
    const T* arow = static_cast<const T*>(p.a) + grow * p.lda;
    const uint4* wfrag = static_cast<const uint4*>(p.packed) + ((int64_t)(s - p.seg_begin) * p.groups * p.nt) * 64 + lane;

    f32x16_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    auto fetch = [&](int gi, uint4& x, uint4 (&w)[NT]) {
        const int k = gi * KG + half * KPL;
        x = make_uint4(0, 0, 0, 0);
        if (k < p.K) {
            x = *reinterpret_cast<const uint4*>(arow + k);
            if (k + KPL > p.K) x = keep_first<T>(x, p.K - k);      // what lies behind column K is never multiplied
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < p.nt) w[t] = wfrag[((int64_t)gi * p.nt + t) * 64];
    };
    uint4 x_cur, w_cur[NT], x_nxt, w_nxt[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) w_cur[t] = w_nxt[t] = make_uint4(0, 0, 0, 0);
    x_nxt = make_uint4(0, 0, 0, 0);
    x_cur = make_uint4(0, 0, 0, 0);
    if (p.groups > 0) fetch(0, x_cur, w_cur);
    for (int gi = 0; gi < p.groups; ++gi) {
        if (gi + 1 < p.groups) fetch(gi + 1, x_nxt, w_nxt);         // in flight during the MFMAs
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < p.nt) acc[t] = mfma_group<T>(w_cur[t], x_cur, acc[t]);
        x_cur = x_nxt;
#pragma unroll
        for (int t = 0; t < NT; ++t) w_cur[t] = w_nxt[t];
    }
    if (!ok) return;
    // D[i][j]: j = lane % 32 = this lane's row, i = (r & 3) + 8 (r >> 2) + 4 half = the column inside the tile
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = t * 32 + g * 8 + half * 4;
            if (n >= p.N) continue;
            const float v[4] = {acc[t][g * 4], acc[t][g * 4 + 1], acc[t][g * 4 + 2], acc[t][g * 4 + 3]};
            if (n + 4 <= p.N && cvec) {
                if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(crow + n) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
                else *reinterpret_cast<float4*>(crow + n) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int i = 0; i < 4; ++i)
                    if (n + i < p.N) store_one<T>(crow + n + i, v[i]);
            }
        }
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
struct GwArgs {
    const void* a;
    int64_t lda;
    const void* g;
    int64_t ldg;
    const int64_t* segoff;
    const int32_t* tileptr;
    const int32_t* partptr;
    const void* rows;
    int rows_bytes;
    float* gw;            // dW_r at gw + r * gw_sr, rows on pitch gw_ld
    int64_t gw_sr, gw_ld;
    float* partial;       // [slots][K][N]
    int64_t slots;
    int64_t M;
    int R, K, N, slab;
};

template <typename T, int NT>
__global__ __launch_bounds__(kBlock) void segmm_gradw_kernel(const GwArgs p) {
    constexpr int EPV = Elem<T>::kPerLane;                          // elements per 16-byte vector
    constexpr int PITCH = kGwRows * (int)sizeof(T) + (sizeof(T) == 4 ? 16 : 0);      // bytes per staged COLUMN (16 rows of it)
    constexpr int XV = kGwKBlock / EPV, GV = NT * 32 / EPV, RV = XV + GV;             // vectors per row: a's block, g
    constexpr int IT = (kGwRows * RV + kBlock - 1) / kBlock;
    __shared__ __attribute__((aligned(16))) char lds[(kGwKBlock + NT * 32) * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int item = blockIdx.x;
    if (item >= p.tileptr[p.R]) return;                             // uniform per workgroup; the pseudo segment's slabs are not work
    const int s = find_segment(p.tileptr, p.R, item);
    const int ns = p.tileptr[s + 1] - p.tileptr[s], j = item - p.tileptr[s];
    const int64_t rbeg = p.segoff[s] + (int64_t)j * p.slab;
    const int64_t rend = min64(rbeg + p.slab, p.segoff[s + 1]);
    const int kb = blockIdx.y * kGwKBlock;
    float* dst;
    int64_t dld;
    if (ns == 1) { dst = p.gw + (int64_t)s * p.gw_sr; dld = p.gw_ld; }
    else {
        const int64_t slot = (int64_t)p.partptr[s] + j;
        if (slot >= p.slots) return;                                // cannot happen (the bound is proven in DESIGN); never write past the workspace
        dst = p.partial + slot * (int64_t)p.K * p.N; dld = p.N;
    }

    f32x16_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    uint4 reg[IT];
    auto fetch = [&](int64_t m) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = tid + it * kBlock;
            const int r = v / RV, c = v % RV;
            const bool is_x = c < XV;
            const int col = is_x ? kb + c * EPV : (c - XV) * EPV;
            const int64_t row = m + r;
            reg[it] = make_uint4(0, 0, 0, 0);
            if (v < kGwRows * RV && row < rend && col < (is_x ? p.K : p.N)) {
                const int64_t grow = p.rows ? load_index(p.rows, p.rows_bytes, row) : row;
                if (grow >= 0 && grow < p.M)
                    reg[it] = *reinterpret_cast<const uint4*>((is_x ? static_cast<const T*>(p.a) + grow * p.lda
                                                                    : static_cast<const T*>(p.g) + grow * p.ldg) + col);
            }
        }
    };
    auto park = [&]() {                                             // transposed: column-major, 16 rows per column
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int v = tid + it * kBlock;
            if (v >= kGwRows * RV) continue;
            const int r = v / RV, c = v % RV;
            const int cbase = c < XV ? c * EPV : kGwKBlock + (c - XV) * EPV;
            const uint32_t w[4] = {reg[it].x, reg[it].y, reg[it].z, reg[it].w};
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                char* q = lds + (cbase + e) * PITCH + r * (int)sizeof(T);
                if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16_t*>(q) = (bf16_t)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                else *reinterpret_cast<uint32_t*>(q) = w[e];
            }
        }
    };
    const bool works = kb + wave * 32 < p.K;                        // this wave owns a k-tile
    const int nt = (p.N + 31) / 32;
    fetch(rbeg);
    park();
    __syncthreads();
    for (int64_t m = rbeg; m < rend; m += kGwRows) {
        const bool more = m + kGwRows < rend;
        if (more) fetch(m + kGwRows);                               // in flight during the MFMAs
        if (works) {
            constexpr int STEPS = kGwRows * (int)sizeof(T) / 32;    // 16-byte fragments per lane half and column: 1 (bf16), 2 (fp32)
#pragma unroll
            for (int u = 0; u < STEPS; ++u) {
                const int off = (u * 2 + half) * 16;
                const uint4 xa = *reinterpret_cast<const uint4*>(lds + (wave * 32 + l32) * PITCH + off);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < nt) {
                        const uint4 gb = *reinterpret_cast<const uint4*>(lds + (kGwKBlock + t * 32 + l32) * PITCH + off);
                        acc[t] = mfma_group<T>(xa, gb, acc[t]);
                    }
            }
        }
        __syncthreads();                                            // everyone has read the stage
        if (more) park();
        __syncthreads();
    }
    if (!works) return;
    // D[i][j]: i = the column of a (k), j = lane % 32 = the column of g: 32 lanes write 32 consecutive n
    const int k0 = kb + wave * 32;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = t * 32 + l32;
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (k < p.K) dst[(int64_t)k * dld + n] = acc[t][r];
        }
    }
}

// empty segments: zeros; segments of several slabs: the partials in slab order; one slab: already written
__global__ __launch_bounds__(kBlock) void segmm_gradw_finish_kernel(const GwArgs p) {
    const int r = blockIdx.x;
    const int ns = p.tileptr[r + 1] - p.tileptr[r];
    if (ns == 1) return;
    const int64_t count = (int64_t)p.K * p.N;
    const int64_t slot0 = p.partptr[r];
    float* dst = p.gw + (int64_t)r * p.gw_sr;
    for (int64_t i = (int64_t)blockIdx.y * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.y * kBlock) {
        float sum = 0.0f;
        for (int z = 0; z < ns; ++z)
            if (slot0 + z < p.slots) sum += p.partial[(slot0 + z) * count + i];
        dst[(i / p.N) * p.gw_ld + (i % p.N)] = sum;
    }
}

static inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }
static inline int gw_slab(int64_t M) {
    const int64_t per = (M + kGwSlabsTarget - 1) / kGwSlabsTarget;
    return (int)std::min<int64_t>(std::max<int64_t>(kGwMinSlab, (per + kGwRows - 1) / kGwRows * kGwRows), 1 << 30);
}
// a segment of t > 1 slabs has more than (t - 1) slab rows, and t <= 2 (t - 1): all such segments together hold fewer than 2 M / slab slabs
static inline int64_t gw_slots(int64_t M) { return 2 * (M / gw_slab(M)) + 2; }
static inline int64_t plan_bytes(int64_t R) { return round16((R + 2) * 8) + 2 * round16((R + 2) * 4); }

struct Plan { int64_t* segoff; int32_t* tileptr; int32_t* partptr; };
static inline Plan plan_at(void* ws, int64_t R) {
    char* b = static_cast<char*>(ws);
    Plan pl;
    pl.segoff = reinterpret_cast<int64_t*>(b);
    pl.tileptr = reinterpret_cast<int32_t*>(b + round16((R + 2) * 8));
    pl.partptr = reinterpret_cast<int32_t*>(b + round16((R + 2) * 8) + round16((R + 2) * 4));
    return pl;
}

}  // namespace segmm
}  // namespace dgll

using namespace dgll;
using namespace dgll::segmm;

static inline int elem_bytes(int dtype) { return dtype == DGLL_BF16 ? 2 : 4; }
static inline int k_group(int dtype) { return dtype == DGLL_BF16 ? 16 : 8; }

DGLL_API int64_t dgll_hip_segment_mm_packed_bytes(int64_t R, int K, int N, int dtype) {
    if (R <= 0 || K <= 0 || N <= 0) return 0;
    const int64_t groups = (K + k_group(dtype) - 1) / k_group(dtype), nt = (N + 31) / 32;
    return R * groups * nt * 1024;
}

DGLL_API int dgll_hip_segment_mm_pack(void* stream, const void* b, int src_dtype, int64_t stride_r, int64_t stride_k, int64_t stride_n,
                                      int64_t R, int K, int N, int dst_dtype, void* packed) {
    DGLL_REQUIRE(R >= 0 && K >= 0 && N >= 0, "negative size");
    if (R == 0 || K == 0 || N == 0) return DGLL_OK;
    DGLL_REQUIRE(b && packed, "NULL argument");
    DGLL_REQUIRE((src_dtype == DGLL_F32 || src_dtype == DGLL_BF16) && (dst_dtype == DGLL_F32 || dst_dtype == DGLL_BF16), "unknown dtype");
    DGLL_REQUIRE(N <= 256, "dgll_hip_segment_mm_pack packs at most N = 256 columns (split columns on the host)");
    DGLL_REQUIRE(aligned16(packed), "packed must be 16-byte aligned");
    const int groups = (K + k_group(dst_dtype) - 1) / k_group(dst_dtype), nt = (N + 31) / 32;
    const int64_t total = R * groups * nt * 64;
    const int64_t blocks = (total + kBlock - 1) / kBlock;
    DGLL_REQUIRE(blocks <= 0x7fffffff, "too many weights for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)blocks);
#define DGLL_SEGMM_PACK(S, T)                                                                                                    \
    hipLaunchKernelGGL((segmm_pack_kernel<S, T>), grid, dim3(kBlock), 0, s, static_cast<const S*>(b), stride_r, stride_k, stride_n, \
                       total, K, N, groups, nt, static_cast<T*>(packed))
    if (src_dtype == DGLL_F32 && dst_dtype == DGLL_F32) DGLL_SEGMM_PACK(float, float);
    else if (src_dtype == DGLL_F32) DGLL_SEGMM_PACK(float, bf16_t);
    else if (dst_dtype == DGLL_F32) DGLL_SEGMM_PACK(bf16_t, float);
    else DGLL_SEGMM_PACK(bf16_t, bf16_t);
#undef DGLL_SEGMM_PACK
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

static int check_common(const void* a, int64_t lda, int dtype, const void* seglen, int seglen_bytes, int64_t R, const void* rows,
                        int rows_bytes, int64_t M, int K, int N) {
    DGLL_REQUIRE(M >= 0 && R >= 0 && K >= 0 && N >= 0, "negative size");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "unknown dtype");
    DGLL_REQUIRE(N <= 256, "the grouped products keep all N <= 256 output columns of a tile in accumulators (split columns on the host)");
    DGLL_REQUIRE(R < (1 << 30) && M / kTileRows + R + 2 < 0x7fffffff, "too many rows or segments for one launch");
    DGLL_REQUIRE(R == 0 || seglen, "NULL seglen");
    DGLL_REQUIRE(seglen_bytes == 4 || seglen_bytes == 8, "seglen must be int32 or int64");
    DGLL_REQUIRE(!rows || rows_bytes == 4 || rows_bytes == 8, "rows must be int32 or int64");
    if (M == 0 || K == 0) return DGLL_OK;
    DGLL_REQUIRE(a, "NULL matrix");
    const int epv = 16 / elem_bytes(dtype);
    DGLL_REQUIRE(lda >= (K + epv - 1) / epv * epv, "pitch < width rounded up to 16 bytes");
    DGLL_REQUIRE(aligned16(a) && lda % epv == 0, "rows must start on 16-byte boundaries");
    return DGLL_OK;
}

DGLL_API int64_t dgll_hip_segment_mm_workspace(int64_t R) { return R < 0 ? 0 : plan_bytes(R); }

DGLL_API int dgll_hip_segment_mm(void* stream, const void* a, int64_t lda, int dtype, const void* packed, const void* seglen,
                                 int seglen_bytes, int64_t R, const void* rows, int rows_bytes, void* c, int64_t ldc, int64_t M, int K,
                                 int N, int64_t seg_begin, int64_t seg_end, int build_plan, void* workspace, int64_t workspace_bytes) {
    const int rc = check_common(a, lda, dtype, seglen, seglen_bytes, R, rows, rows_bytes, M, K, N);
    if (rc != DGLL_OK) return rc;
    if (M == 0 || N == 0) return DGLL_OK;
    DGLL_REQUIRE(c, "NULL matrix");
    DGLL_REQUIRE(ldc >= N, "pitch < width");
    DGLL_REQUIRE(0 <= seg_begin && seg_begin <= seg_end && seg_end <= R, "segment range outside [0, R]");
    DGLL_REQUIRE(K == 0 || seg_begin == seg_end || packed, "NULL packed weights");
    DGLL_REQUIRE(!packed || aligned16(packed), "packed must be 16-byte aligned");
    DGLL_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= plan_bytes(R), "workspace too small for the tile list");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan pl = plan_at(workspace, R);
    if (build_plan) {      // (0: the workspace holds the list of an earlier call with the same seglen, R and M -- another range or column block)
        hipLaunchKernelGGL(segmm_plan_kernel, dim3(1), dim3(kBlock), 0, s, seglen, seglen_bytes, R, M, kTileRows, pl.segoff, pl.tileptr, pl.partptr);
        DGLL_HIP_TRY(hipGetLastError());
    }
    FwdArgs p{};
    p.a = a; p.lda = lda; p.packed = packed; p.segoff = pl.segoff; p.tileptr = pl.tileptr; p.rows = rows; p.rows_bytes = rows_bytes;
    p.c = c; p.ldc = ldc; p.M = M; p.R = (int)R; p.K = K; p.N = N;
    p.groups = (K + k_group(dtype) - 1) / k_group(dtype);
    p.nt = (N + 31) / 32;
    p.seg_begin = (int)seg_begin; p.seg_end = (int)seg_end;
    const int64_t tiles = (M + kTileRows - 1) / kTileRows + R + 1;         // >= sum over segments (the pseudo one included) of ceil(len / 32)
    const dim3 grid((uint32_t)((tiles + kWavesPerBlock - 1) / kWavesPerBlock));
#define DGLL_SEGMM_FWD(T, NTV) hipLaunchKernelGGL((segmm_fwd_kernel<T, NTV>), grid, dim3(kBlock), 0, s, p)
#define DGLL_SEGMM_FWD_T(T)                          \
    if (p.nt <= 1) DGLL_SEGMM_FWD(T, 1);             \
    else if (p.nt <= 2) DGLL_SEGMM_FWD(T, 2);        \
    else if (p.nt <= 4) DGLL_SEGMM_FWD(T, 4);        \
    else DGLL_SEGMM_FWD(T, 8)
    if (dtype == DGLL_BF16) { DGLL_SEGMM_FWD_T(bf16_t); } else { DGLL_SEGMM_FWD_T(float); }
#undef DGLL_SEGMM_FWD_T
#undef DGLL_SEGMM_FWD
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int64_t dgll_hip_segment_mm_gradw_workspace(int64_t M, int64_t R, int K, int N) {
    if (M < 0 || R < 0 || K < 0 || N < 0) return 0;
    return plan_bytes(R) + gw_slots(M) * (int64_t)K * N * (int64_t)sizeof(float);
}

DGLL_API int dgll_hip_segment_mm_gradw(void* stream, const void* a, int64_t lda, const void* g, int64_t ldg, int dtype, const void* seglen,
                                       int seglen_bytes, int64_t R, const void* rows, int rows_bytes, float* gw, int64_t gw_stride_r,
                                       int64_t gw_ld, int64_t M, int K, int N, void* workspace, int64_t workspace_bytes) {
    int rc = check_common(a, lda, dtype, seglen, seglen_bytes, R, rows, rows_bytes, M, K, N);
    if (rc != DGLL_OK) return rc;
    rc = check_common(g, ldg, dtype, seglen, seglen_bytes, R, rows, rows_bytes, M, N, N);
    if (rc != DGLL_OK) return rc;
    if (R == 0 || K == 0 || N == 0) return DGLL_OK;
    DGLL_REQUIRE(gw, "NULL matrix");
    DGLL_REQUIRE(gw_ld >= N && gw_stride_r >= 0, "pitch < width");
    DGLL_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= dgll_hip_segment_mm_gradw_workspace(M, R, K, N),
                 "workspace too small for the slab partials");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Plan pl = plan_at(workspace, R);
    GwArgs p{};
    p.a = a; p.lda = lda; p.g = g; p.ldg = ldg; p.segoff = pl.segoff; p.tileptr = pl.tileptr; p.partptr = pl.partptr;
    p.rows = rows; p.rows_bytes = rows_bytes; p.gw = gw; p.gw_sr = gw_stride_r; p.gw_ld = gw_ld;
    p.partial = reinterpret_cast<float*>(static_cast<char*>(workspace) + plan_bytes(R));
    p.slots = gw_slots(M); p.M = M; p.R = (int)R; p.K = K; p.N = N; p.slab = gw_slab(M);
    hipLaunchKernelGGL(segmm_plan_kernel, dim3(1), dim3(kBlock), 0, s, seglen, seglen_bytes, R, M, p.slab, pl.segoff, pl.tileptr, pl.partptr);
    DGLL_HIP_TRY(hipGetLastError());
    if (M > 0) {
        const int64_t items = (M + p.slab - 1) / p.slab + R;                 // >= sum over the R segments of ceil(len / slab)
        const dim3 grid((uint32_t)items, (uint32_t)((K + kGwKBlock - 1) / kGwKBlock));
        const int nt = (N + 31) / 32;
#define DGLL_SEGMM_GW(T, NTV) hipLaunchKernelGGL((segmm_gradw_kernel<T, NTV>), grid, dim3(kBlock), 0, s, p)
#define DGLL_SEGMM_GW_T(T)                      \
    if (nt <= 1) DGLL_SEGMM_GW(T, 1);           \
    else if (nt <= 2) DGLL_SEGMM_GW(T, 2);      \
    else if (nt <= 4) DGLL_SEGMM_GW(T, 4);      \
    else DGLL_SEGMM_GW(T, 8)
        if (dtype == DGLL_BF16) { DGLL_SEGMM_GW_T(bf16_t); } else { DGLL_SEGMM_GW_T(float); }
#undef DGLL_SEGMM_GW_T
#undef DGLL_SEGMM_GW
        DGLL_HIP_TRY(hipGetLastError());
    }
    const int64_t count = (int64_t)K * N;
    hipLaunchKernelGGL(segmm_gradw_finish_kernel, dim3((uint32_t)R, (uint32_t)std::min<int64_t>((count + kBlock - 1) / kBlock, 64)),
                       dim3(kBlock), 0, s, p);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
