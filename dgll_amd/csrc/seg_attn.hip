// seg_attn.hip -- dense attention inside every segment of a batch (the global half of a GraphGPS block):
//
//     S = scale . Q_s,h K_s,h^T      P = softmax over the keys of the segment      O_s,h = P V_s,h
//
// for every segment s (rows seg_ptr[s] .. seg_ptr[s + 1] of q, k, v) and every head h of width D <= 128.  Rows never see another
// segment; an empty segment costs nothing.  No [n, n] array exists in any pass, nothing is atomic, cleared or read back.
//
//   DGLL_SEG_ATTN_FORWARD   out, lse                      (online softmax: running max and sum per query, O rescaled)
//   DGLL_SEG_ATTN_ROWS      grad_q, delta_i = <dO_i, O_i> (P recomputed from lse; sweeps the key tiles of the segment)
//   DGLL_SEG_ATTN_COLS      grad_k, grad_v                (32 keys in accumulators; sweeps the query tiles of the segment)
//
// Work split.  A work item is (segment, 32-row tile of it, head): blockIdx.y is the head, and the four waves of a workgroup take
// four consecutive tiles of the list, each on its own (no workgroup barrier anywhere): a 20-node molecule costs one wave per head.
// The wrapper uploads seg_ptr and the tile prefix tile_ptr (tile_ptr[s] = tiles of the segments before s) together; a wave finds
// its segment by binary search in tile_ptr and leaves when its item is past tile_ptr[S].  The grid is sized by the bound
// ceil(N / 32) + S that holds for any cut of N rows.  Segment bounds are clamped to [0, N] on the device: a wrong table can
// address nothing outside the operands.
//
// Data movement (all products on v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x2_f32, one template):
//   * Scores are computed TRANSPOSED, S^T = K Q^T per 32 x 32 tile: the swept rows are MFMA "A", the wave's own rows "B".  A lane
//     loads 16 bytes of ITS OWN row per k-group, so neither operand needs LDS, and the own-row fragments (Q in the forward; Q and
//     dO in ROWS; K and V in COLS) stay in registers for the whole sweep.
//   * The accumulator layout then gives lane (l32, half) 16 scores of ONE own row l32 against the swept rows
//     (r & 3) + 8 (r >> 2) + 4 half: the softmax max and sum are an in-lane reduction plus one exchange with lane ^ 32.
//   * The 16 probabilities (or dS values) are converted in place into the "B" operand of the second product, O^T += V^T P^T; the
//     swept-row order inside a k-group is the accumulator's, and the "A" fragment is read from LDS in that same order.
//     P never leaves registers.
//   * Only the "A" operand of the second product needs a transpose.  The lane already holds the 16-byte pieces of its swept row
//     (they were the first product's "A" fragments, or V's in the forward), writes them element-wise into a WAVE-PRIVATE slab
//     T[d][32 swept rows] and reads back 8-byte (bf16) / 16-byte (fp32) fragments.  One wave's LDS operations execute in order, so
//     a compiler fence (wave_barrier) is all that separates the writes from the reads.
//     Slab: (32 * ceil(D / 32)) rows of 72 bytes (bf16) / 144 bytes (fp32), padded so the 32 lanes of a fragment read hit distinct
//     banks: 9 / 18 KiB per wave at D = 128, 36 / 72 KiB per workgroup, i.e. 4 / 2 workgroups per CU of 160 KiB by LDS (the
//     accumulators, 64 to 128 registers plus the resident fragments, bound the occupancy before LDS does).  COLS reuses the one
//     slab for Q^T and then dO^T, and keeps lse / delta of the 32 swept queries in 256 further bytes.
//   * scale . log2(e) is one multiplier and the exponentials are exp2.  Swept rows past the end of a segment are loaded clamped to
//     its last row and enter the softmax as -inf (their P and dS are exactly 0); own rows past the end are computed and not stored.
//   * D that is not a multiple of 32: fragments past D are zeros on load, stores are masked.
// Compiled without the packed fp32 instructions, from inside the file (as segment_mm.hip): the common build flags stay as they are.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include <algorithm>

#include "common.hpp"

namespace dgll {
namespace segattn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int kTile = DGLL_SEG_ATTN_TILE;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

// elements per 16-byte fragment / per MFMA k-group, bytes per slab row (32 elements and a pad that spreads the banks)
template <typename T> struct Elem;
template <> struct Elem<bf16_t> { static constexpr int kPerLane = 8, kGroup = 16, kPitch = 72; };
template <> struct Elem<float> { static constexpr int kPerLane = 4, kGroup = 8, kPitch = 144; };

struct Args {
    const int64_t* seg_ptr;
    const int64_t* tile_ptr;
    int64_t N;
    int S, heads, D;
    int dtiles;      // 32-column tiles of a head that hold data: ceil(D / 32)
    int sgroups;     // k-groups of a head that hold data: ceil(D / kGroup)
    float scale, scale_log2;
    const void *q, *k, *v, *go, *o;
    int64_t ldq, ldk, ldv, ldgo, ldo;
    void *out, *out2;
    int64_t ldout, ldout2;
    float* lse;
    float* delta;
};

struct Item { int64_t begin, end, row0; };      // the segment's rows [begin, end), the tile's first row

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the work item of this wave: false when there is none (past the list, or a table that does not describe N rows)
__device__ __forceinline__ bool find_item(const Args& p, int wave, Item& w) {
    const int64_t item = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (item >= p.tile_ptr[p.S]) return false;
    int lo = 0, hi = p.S - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p.tile_ptr[mid + 1] <= item) lo = mid + 1; else hi = mid;
    }
    w.begin = clamp64(p.seg_ptr[lo], 0, p.N);
    w.end = clamp64(p.seg_ptr[lo + 1], w.begin, p.N);
    w.row0 = w.begin + (item - p.tile_ptr[lo]) * kTile;
    return w.row0 >= w.begin && w.row0 < w.end;
}

// swept row (inside its tile) of accumulator register r of a lane of half `half`
__device__ __forceinline__ int swept(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

template <typename T> __device__ __forceinline__ f32x16_t mfma_group(uint4 a, uint4 b, f32x16_t acc);
template <> __device__ __forceinline__ f32x16_t mfma_group<bf16_t>(uint4 a, uint4 b, f32x16_t acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x16_t mfma_group<float>(uint4 a, uint4 b, f32x16_t acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// the 16-byte pieces of one row of a head: f[g] = row[g * kGroup + half * kPerLane ..], zeros past D
template <typename T, int G> __device__ __forceinline__ void load_frags(const T* row, int D, int half, uint4 (&f)[G]) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int d = g * Elem<T>::kGroup + half * Elem<T>::kPerLane;
        f[g] = make_uint4(0, 0, 0, 0);
        if (d < D) f[g] = *reinterpret_cast<const uint4*>(row + d);
    }
}

// 32 x 32 tile of products: lane (l32, half) gets <swept row swept(r, half), own row l32> in register r
template <typename T, int G> __device__ __forceinline__ f32x16_t products(const uint4 (&a)[G], const uint4 (&b)[G], int sgroups) {
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (g < sgroups) acc = mfma_group<T>(a[g], b[g], acc);
    return acc;
}

// the lane's swept row into the slab, transposed: slab[d][l32] for every column d of the tiles that hold data
template <typename T, int G> __device__ __forceinline__ void stage(char* slab, const uint4 (&f)[G], int dtiles, int half, int l32) {
    constexpr int EPV = Elem<T>::kPerLane, KG = Elem<T>::kGroup, PITCH = Elem<T>::kPitch;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g * KG >= dtiles * 32) continue;
        const uint32_t w[4] = {f[g].x, f[g].y, f[g].z, f[g].w};
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
            char* q = slab + (g * KG + half * EPV + e) * PITCH + l32 * (int)sizeof(T);
            if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16_t*>(q) = (bf16_t)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
            else *reinterpret_cast<uint32_t*>(q) = w[e];
        }
    }
}

// acc[t][d][own row] += sum over the swept rows of slab[32 t + d][swept row] . x[swept row][own row]; x in the layout of products()
template <typename T, int DT>
__device__ __forceinline__ void accumulate(const char* slab, const float (&x)[16], f32x16_t (&acc)[DT], int dtiles, int half, int l32) {
    constexpr int PITCH = Elem<T>::kPitch;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {       // registers 8 m .. 8 m + 7: swept rows 16 m + 4 half + {0 .. 3} and the same + 8
            const uint4 b = make_uint4(pack_bf16x2(x[8 * m], x[8 * m + 1]), pack_bf16x2(x[8 * m + 2], x[8 * m + 3]),
                                       pack_bf16x2(x[8 * m + 4], x[8 * m + 5]), pack_bf16x2(x[8 * m + 6], x[8 * m + 7]));
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                if (t >= dtiles) continue;
                const char* a = slab + (t * 32 + l32) * PITCH + (16 * m + 4 * half) * 2;
                const uint2 lo = *reinterpret_cast<const uint2*>(a), hi = *reinterpret_cast<const uint2*>(a + 16);
                acc[t] = mfma_group<bf16_t>(make_uint4(lo.x, lo.y, hi.x, hi.y), b, acc[t]);
            }
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {       // registers 4 g .. 4 g + 3: swept rows 8 g + 4 half + {0 .. 3}
            const uint4 b = make_uint4(__float_as_uint(x[4 * g]), __float_as_uint(x[4 * g + 1]), __float_as_uint(x[4 * g + 2]),
                                       __float_as_uint(x[4 * g + 3]));
#pragma unroll
            for (int t = 0; t < DT; ++t) {
                if (t >= dtiles) continue;
                const uint4 a = *reinterpret_cast<const uint4*>(slab + (t * 32 + l32) * PITCH + (8 * g + 4 * half) * 4);
                acc[t] = mfma_group<float>(a, b, acc[t]);
            }
        }
    }
}

template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d) {
    if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
    else *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

// acc[t] holds [32 columns of tile t][own row l32]: register r is column swept(r, half), four consecutive columns per 4 registers
template <typename T, int DT>
__device__ __forceinline__ void store_rows(T* row, const f32x16_t (&acc)[DT], float mul, int D, int half) {
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = t * 32 + 8 * g + 4 * half;
            if (d < D) store4<T>(row + d, acc[t][4 * g] * mul, acc[t][4 * g + 1] * mul, acc[t][4 * g + 2] * mul, acc[t][4 * g + 3] * mul);
        }
}

template <int DT> __device__ __forceinline__ void clear(f32x16_t (&acc)[DT]) {
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}

#define DGLL_SEG_ATTN_PROLOGUE                                                                                              \
    constexpr int KG = Elem<T>::kGroup, PITCH = Elem<T>::kPitch, G = DT * 32 / KG;                                          \
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                             \
    const int half = lane >> 5, l32 = lane & 31;                                                                            \
    Item w;                                                                                                                 \
    if (!find_item(p, wave, w)) return;                /* (no workgroup barrier in these kernels: waves leave on their own) */ \
    const int head = blockIdx.y;                                                                                            \
    const int64_t col0 = (int64_t)head * p.D;                                                                               \
    const int64_t own = w.row0 + l32 < w.end ? w.row0 + l32 : w.end - 1;      /* clamp the loads, mask the stores */         \
    const bool own_ok = w.row0 + l32 < w.end

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(kBlock) void seg_attn_fwd_kernel(const Args p) {
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * DT * 32 * Elem<T>::kPitch];
    DGLL_SEG_ATTN_PROLOGUE;
    char* slab = lds + wave * (DT * 32 * PITCH);
    uint4 qf[G], f[G];
    load_frags<T, G>(static_cast<const T*>(p.q) + own * p.ldq + col0, p.D, half, qf);
    f32x16_t acc[DT];
    clear<DT>(acc);
    float m = -INFINITY, l = 0.0f;
    for (int64_t kt = w.begin; kt < w.end; kt += kTile) {
        const int64_t krow = kt + l32 < w.end ? kt + l32 : w.end - 1;
        const int valid = (int)(w.end - kt < kTile ? w.end - kt : kTile);
        load_frags<T, G>(static_cast<const T*>(p.k) + krow * p.ldk + col0, p.D, half, f);
        const f32x16_t s = products<T, G>(f, qf, p.sgroups);
        load_frags<T, G>(static_cast<const T*>(p.v) + krow * p.ldv + col0, p.D, half, f);
        __builtin_amdgcn_wave_barrier();               // the reads of the last tile are issued before these writes
        stage<T, G>(slab, f, p.dtiles, half, l32);
        float pr[16], mx = m;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pr[r] = swept(r, half) < valid ? s[r] * p.scale_log2 : -INFINITY;
            mx = fmaxf(mx, pr[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));            // key kt is valid: mx is finite from the first tile on
        const float alpha = __builtin_amdgcn_exp2f(m - mx);
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pr[r] = __builtin_amdgcn_exp2f(pr[r] - mx);
            sum += pr[r];
        }
        sum += __shfl_xor(sum, 32);
        l = l * alpha + sum;
        m = mx;
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] *= alpha;
        __builtin_amdgcn_wave_barrier();
        accumulate<T, DT>(slab, pr, acc, p.dtiles, half, l32);
    }
    if (!own_ok) return;
    store_rows<T, DT>(static_cast<T*>(p.out) + own * p.ldout + col0, acc, 1.0f / l, p.D, half);
    if (half == 0) p.lse[own * p.heads + head] = (m + __builtin_amdgcn_logf(l)) * kLn2;
}

// ---- backward over query tiles: grad_q and delta ----------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float dot16(uint4 a, uint4 b) {
    constexpr int EPV = Elem<T>::kPerLane;
    float x[EPV], y[EPV], s = 0.0f;
    VecIO<T, EPV>::unpack(a, x);
    VecIO<T, EPV>::unpack(b, y);
#pragma unroll
    for (int e = 0; e < EPV; ++e) s += x[e] * y[e];
    return s;
}

template <typename T, int DT>
__global__ __launch_bounds__(kBlock) void seg_attn_rows_kernel(const Args p) {
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * DT * 32 * Elem<T>::kPitch];
    DGLL_SEG_ATTN_PROLOGUE;
    char* slab = lds + wave * (DT * 32 * PITCH);
    uint4 qf[G], gf[G], f[G];
    load_frags<T, G>(static_cast<const T*>(p.q) + own * p.ldq + col0, p.D, half, qf);
    load_frags<T, G>(static_cast<const T*>(p.go) + own * p.ldgo + col0, p.D, half, gf);
    load_frags<T, G>(static_cast<const T*>(p.o) + own * p.ldo + col0, p.D, half, f);
    float delta = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g) delta += dot16<T>(gf[g], f[g]);
    delta += __shfl_xor(delta, 32);
    const float lse2 = p.lse[own * p.heads + head] * kLog2e;
    f32x16_t acc[DT];
    clear<DT>(acc);
    for (int64_t kt = w.begin; kt < w.end; kt += kTile) {
        const int64_t krow = kt + l32 < w.end ? kt + l32 : w.end - 1;
        const int valid = (int)(w.end - kt < kTile ? w.end - kt : kTile);
        load_frags<T, G>(static_cast<const T*>(p.k) + krow * p.ldk + col0, p.D, half, f);
        const f32x16_t s = products<T, G>(f, qf, p.sgroups);
        __builtin_amdgcn_wave_barrier();
        stage<T, G>(slab, f, p.dtiles, half, l32);      // K^T: grad_q^T += K^T dS^T
        load_frags<T, G>(static_cast<const T*>(p.v) + krow * p.ldv + col0, p.D, half, f);
        const f32x16_t dp = products<T, G>(f, gf, p.sgroups);
        float ds[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pr = swept(r, half) < valid ? __builtin_amdgcn_exp2f(s[r] * p.scale_log2 - lse2) : 0.0f;
            ds[r] = pr * (dp[r] - delta);
        }
        __builtin_amdgcn_wave_barrier();
        accumulate<T, DT>(slab, ds, acc, p.dtiles, half, l32);
    }
    if (!own_ok) return;
    store_rows<T, DT>(static_cast<T*>(p.out) + own * p.ldout + col0, acc, p.scale, p.D, half);
    if (half == 0) p.delta[own * p.heads + head] = delta;
}

// ---- backward over key tiles: grad_k and grad_v -------------------------------------------------------------------------------------
template <typename T, int DT>
__global__ __launch_bounds__(kBlock) void seg_attn_cols_kernel(const Args p) {
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * (DT * 32 * Elem<T>::kPitch + 256)];
    DGLL_SEG_ATTN_PROLOGUE;
    char* slab = lds + wave * (DT * 32 * PITCH + 256);
    float* stat = reinterpret_cast<float*>(slab + DT * 32 * PITCH);      // lse . log2(e) [32] | delta [32] of the swept queries
    uint4 kf[G], vf[G], f[G];
    load_frags<T, G>(static_cast<const T*>(p.k) + own * p.ldk + col0, p.D, half, kf);
    load_frags<T, G>(static_cast<const T*>(p.v) + own * p.ldv + col0, p.D, half, vf);
    f32x16_t acck[DT], accv[DT];
    clear<DT>(acck);
    clear<DT>(accv);
    for (int64_t qt = w.begin; qt < w.end; qt += kTile) {
        const int64_t qrow = qt + l32 < w.end ? qt + l32 : w.end - 1;
        const int valid = (int)(w.end - qt < kTile ? w.end - qt : kTile);
        const float st = half == 0 ? p.lse[qrow * p.heads + head] * kLog2e : p.delta[qrow * p.heads + head];
        load_frags<T, G>(static_cast<const T*>(p.q) + qrow * p.ldq + col0, p.D, half, f);
        const f32x16_t s = products<T, G>(f, kf, p.sgroups);
        __builtin_amdgcn_wave_barrier();
        stat[lane] = st;
        stage<T, G>(slab, f, p.dtiles, half, l32);      // Q^T: grad_k^T += Q^T dS
        load_frags<T, G>(static_cast<const T*>(p.go) + qrow * p.ldgo + col0, p.D, half, f);
        const f32x16_t dp = products<T, G>(f, vf, p.sgroups);
        __builtin_amdgcn_wave_barrier();
        float pr[16], ds[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 l4 = *reinterpret_cast<const float4*>(stat + 8 * g + 4 * half);
            const float4 d4 = *reinterpret_cast<const float4*>(stat + 32 + 8 * g + 4 * half);
            const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int r = 4 * g + c;
                pr[r] = swept(r, half) < valid ? __builtin_amdgcn_exp2f(s[r] * p.scale_log2 - lq[c]) : 0.0f;
                ds[r] = pr[r] * (dp[r] - dq[c]);
            }
        }
        accumulate<T, DT>(slab, ds, acck, p.dtiles, half, l32);
        __builtin_amdgcn_wave_barrier();
        stage<T, G>(slab, f, p.dtiles, half, l32);      // dO^T: grad_v^T += dO^T P
        __builtin_amdgcn_wave_barrier();
        accumulate<T, DT>(slab, pr, accv, p.dtiles, half, l32);
    }
    if (!own_ok) return;
    store_rows<T, DT>(static_cast<T*>(p.out) + own * p.ldout + col0, acck, p.scale, p.D, half);
    store_rows<T, DT>(static_cast<T*>(p.out2) + own * p.ldout2 + col0, accv, 1.0f, p.D, half);
}

#undef DGLL_SEG_ATTN_PROLOGUE

}  // namespace segattn
}  // namespace dgll

using namespace dgll;
using namespace dgll::segattn;

static int check_matrix(const void* m, int64_t ld, int epv, int64_t width) {
    DGLL_REQUIRE(m, "NULL matrix");
    DGLL_REQUIRE(ld >= width, "pitch < heads * D");
    DGLL_REQUIRE(aligned16(m) && ld % epv == 0, "rows must start on 16-byte boundaries");
    return DGLL_OK;
}

DGLL_API int dgll_hip_segment_attn_pass(void* stream, const dgll_seg_attn_desc* d) {
    DGLL_REQUIRE(d, "NULL descriptor");
    DGLL_REQUIRE(d->pass == DGLL_SEG_ATTN_FORWARD || d->pass == DGLL_SEG_ATTN_ROWS || d->pass == DGLL_SEG_ATTN_COLS, "unknown pass");
    DGLL_REQUIRE(d->dtype == DGLL_F32 || d->dtype == DGLL_BF16, "unknown dtype");
    DGLL_REQUIRE(d->n_rows >= 0 && d->n_segs >= 0, "negative size");
    DGLL_REQUIRE(d->n_rows < ((int64_t)1 << 31) && d->n_segs < ((int64_t)1 << 31), "N and S must be below 2^31 for one launch");
    DGLL_REQUIRE(d->heads >= 1 && d->heads <= 65535, "heads must be in [1, 65535]");
    const int epv = d->dtype == DGLL_BF16 ? 8 : 4;
    DGLL_REQUIRE(d->D >= 1 && d->D % epv == 0, "D must be a whole number of 16-byte vectors (4 fp32 / 8 bf16 columns)");
    DGLL_REQUIRE(d->D <= DGLL_SEG_ATTN_MAX_D, "D is at most DGLL_SEG_ATTN_MAX_D = 128 columns per head");
    if (d->n_rows == 0) return DGLL_OK;
    DGLL_REQUIRE(d->n_segs >= 1 && d->seg_ptr && d->tile_ptr, "NULL seg_ptr or tile_ptr");
    const int64_t width = (int64_t)d->heads * d->D;
    int rc = check_matrix(d->q, d->ld_q, epv, width);
    if (rc == DGLL_OK) rc = check_matrix(d->k, d->ld_k, epv, width);
    if (rc == DGLL_OK) rc = check_matrix(d->v, d->ld_v, epv, width);
    if (rc == DGLL_OK) rc = check_matrix(d->out, d->ld_out, epv, width);
    if (rc == DGLL_OK && d->pass != DGLL_SEG_ATTN_FORWARD) rc = check_matrix(d->grad_out, d->ld_grad_out, epv, width);
    if (rc == DGLL_OK && d->pass == DGLL_SEG_ATTN_ROWS) rc = check_matrix(d->o, d->ld_o, epv, width);
    if (rc == DGLL_OK && d->pass == DGLL_SEG_ATTN_COLS) rc = check_matrix(d->out2, d->ld_out2, epv, width);
    if (rc != DGLL_OK) return rc;
    DGLL_REQUIRE(d->lse, "NULL lse");
    DGLL_REQUIRE(d->pass == DGLL_SEG_ATTN_FORWARD || d->delta, "NULL delta");

    Args p{};
    p.seg_ptr = d->seg_ptr; p.tile_ptr = d->tile_ptr; p.N = d->n_rows; p.S = (int)d->n_segs; p.heads = d->heads; p.D = d->D;
    p.dtiles = (d->D + 31) / 32;
    p.sgroups = (d->D + 2 * epv - 1) / (2 * epv);
    p.scale = d->scale; p.scale_log2 = d->scale * kLog2e;
    p.q = d->q; p.k = d->k; p.v = d->v; p.go = d->grad_out; p.o = d->o;
    p.ldq = d->ld_q; p.ldk = d->ld_k; p.ldv = d->ld_v; p.ldgo = d->ld_grad_out; p.ldo = d->ld_o;
    p.out = d->out; p.out2 = d->out2; p.ldout = d->ld_out; p.ldout2 = d->ld_out2;
    p.lse = d->lse; p.delta = d->delta;
    const int64_t items = (d->n_rows + kTile - 1) / kTile + d->n_segs;      // >= sum over the segments of ceil(size / 32)
    const dim3 grid((uint32_t)((items + kWavesPerBlock - 1) / kWavesPerBlock), (uint32_t)d->heads);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define DGLL_SEG_ATTN_LAUNCH(KERNEL, T)                                                             \
    if (p.dtiles <= 1) hipLaunchKernelGGL((KERNEL<T, 1>), grid, dim3(kBlock), 0, s, p);             \
    else if (p.dtiles <= 2) hipLaunchKernelGGL((KERNEL<T, 2>), grid, dim3(kBlock), 0, s, p);        \
    else hipLaunchKernelGGL((KERNEL<T, 4>), grid, dim3(kBlock), 0, s, p)
#define DGLL_SEG_ATTN_PASS(KERNEL)                                                                  \
    if (d->dtype == DGLL_BF16) { DGLL_SEG_ATTN_LAUNCH(KERNEL, bf16_t); } else { DGLL_SEG_ATTN_LAUNCH(KERNEL, float); }
    if (d->pass == DGLL_SEG_ATTN_FORWARD) { DGLL_SEG_ATTN_PASS(seg_attn_fwd_kernel) }
    else if (d->pass == DGLL_SEG_ATTN_ROWS) { DGLL_SEG_ATTN_PASS(seg_attn_rows_kernel) }
    else { DGLL_SEG_ATTN_PASS(seg_attn_cols_kernel) }
#undef DGLL_SEG_ATTN_PASS
#undef DGLL_SEG_ATTN_LAUNCH
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
