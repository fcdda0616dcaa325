// point_rows.hpp -- reading rows of points and their squared distance, shared by fps.hip and radius.hip (knn.hip carries a copy of the
// loads of its own).  A row is D <= kMaxD columns of fp32 or bf16 on a pitch; it is read eight columns at a time, as 16-byte vectors
// where the caller says the address allows it and column by column otherwise, and comes back as fp32 with zeros from column D on,
// whatever the memory behind the row holds.  The distance is the difference form sum_c (a_c - b_c)^2 in fp32, columns ascending, every
// step one fused multiply-add WRITTEN as one: two places that compute the distance of the same pair get the same bits, whatever the
// compiler would have contracted.
#pragma once
#include "common.hpp"

namespace dgll {
namespace points {

constexpr int kMaxD = 32;           // DGLL_FPS_MAX_D, DGLL_RADIUS_MAX_D
constexpr int kOct = kMaxD / 8;     // groups of eight columns in the widest row

__device__ __forceinline__ float load_one(const float* p) { return *p; }
__device__ __forceinline__ float load_one(const bf16_t* p) { return bf16_lo((uint32_t)*p); }
// eight columns from a 16-byte aligned address; left > 0 of them belong to the row
__device__ __forceinline__ void load_vec8(const float* p, int left, float (&f)[8]) {
    float a[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    VecIO<float, 4>::unpack(VecIO<float, 4>::load(p), a);
    if (left > 4) VecIO<float, 4>::unpack(VecIO<float, 4>::load(p + 4), b);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}
__device__ __forceinline__ void load_vec8(const bf16_t* p, int left, float (&f)[8]) {
    (void)left;
    VecIO<bf16_t, 8>::unpack(VecIO<bf16_t, 8>::load(p), f);
}
// columns col0 .. col0 + 7 of a row as fp32; zero from column D on
template <typename T, bool VEC>
__device__ __forceinline__ void load8(const T* row, int col0, int D, float (&f)[8]) {
    const int left = D - col0;
    if (left <= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.0f;
        return;
    }
    if (VEC) {
        load_vec8(row + col0, left, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e >= left) f[e] = 0.0f;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = e < left ? load_one(row + col0 + e) : 0.0f;
    }
}

// the whole row (D <= kMaxD) into registers
template <typename T, bool VEC>
__device__ __forceinline__ void load_row(const T* row, int D, float (&q)[kMaxD]) {
#pragma unroll
    for (int o = 0; o < kOct; ++o) {
        float f[8];
        load8<T, VEC>(row, o * 8, D, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[o * 8 + e] = f[e];
    }
}

__device__ __forceinline__ float sq_step(float acc, float a, float b) {
    const float df = a - b;
    return fmaf(df, df, acc);
}

// d(row, q) for a row in memory and one in registers (zeros from column D on)
template <typename T, bool VEC>
__device__ __forceinline__ float sq_dist(const T* row, int D, const float (&q)[kMaxD]) {
    float acc = 0.0f;
#pragma unroll
    for (int o = 0; o < kOct; ++o) {
        if (o * 8 < D) {
            float f[8];
            load8<T, VEC>(row, o * 8, D, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = sq_step(acc, f[e], q[o * 8 + e]);
        }
    }
    return acc;
}

template <typename T>
static inline bool rows_vec16(const T* x, int64_t ld) { return aligned16(x) && ((size_t)ld * sizeof(T)) % 16 == 0; }

}  // namespace points
}  // namespace dgll
