// gather.hpp -- the inner gather loop shared by the SpMM kernels (spmm.hip) and the fused aggregate -> transform kernel
// (fused_sage.hip): see spmm.hip's header for the design.
#pragma once
#include "common.hpp"

// spmm.hip: the SpMM behind every dgll_hip_spmm_csr* entry point (only_long: the long rows of the plan only)
int dgll_spmm_csr_impl(void* stream, const dgll_csr_plan* plan, const int64_t* rowptr, const int32_t* col,
                       const float* val, const void* X, int64_t ldx, int x_dtype, void* Y, int64_t ldy,
                       int y_dtype, int64_t n_rows, int64_t n_cols, int feat, int reduce, int epilogue,
                       const float* bias, void* workspace, size_t workspace_bytes, const float* row_scale, int accumulate,
                       const void* gate, int64_t ldg, int only_long);

namespace dgll {

// Accumulate edges [b, e) of one row into acc (this lane's EPV columns starting at xcol).
template <typename XT, int EPV, int LPR, bool HAS_VAL, int U>
__device__ __forceinline__ void gather_edges(const int32_t* __restrict__ col, const float* __restrict__ val,
                                             const XT* __restrict__ xcol, int64_t ldx, int64_t b, int64_t e,
                                             int lane, float (&acc)[EPV], bool preloaded = false, int first_col = 0,
                                             float first_val = 0.0f) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int slot = lane / LPR;

    int my_col = first_col;               // preloaded: the caller requested the row's first index batch a row ago
    float my_val = first_val;
    if (!preloaded) {
        my_col = 0;
        my_val = 0.0f;
        if (b + lane < e) {
            my_col = __builtin_nontemporal_load(col + b + lane);   // indices and weights are streamed once: keep them
            if (HAS_VAL) my_val = __builtin_nontemporal_load(val + b + lane);   // from displacing feature rows in L2
        }
    }
    for (int64_t k0 = b; k0 < e; k0 += kWave) {
        const int64_t left = e - k0;
        const int nb = left < kWave ? (int)left : kWave;
        const int cur_col = my_col;
        const float cur_val = my_val;
        // prefetch the next batch of indices while this one is consumed
        const int64_t kn = k0 + kWave + lane;
        if (kn < e) {
            my_col = __builtin_nontemporal_load(col + kn);
            if (HAS_VAL) my_val = __builtin_nontemporal_load(val + kn);
        }
        // Row offsets are formed with ONE 32x32->64 multiply (v_mad_u64_u32): column ids and the leading dimension both
        // fit 32 bits.  Full rounds need no masking; only the last, partial round clamps and zeroes its idle slots.
        const uint32_t ld32 = (uint32_t)ldx;
        int j = 0;
        for (; j + SLOTS * U <= nb; j += SLOTS * U) {
            int c[U];
            float w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int src = j + u * SLOTS + slot;
                c[u] = __shfl(cur_col, src);
                w[u] = HAS_VAL ? __shfl(cur_val, src) : 1.0f;
            }
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = IO::load(xcol + (uint64_t)(uint32_t)c[u] * ld32);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(v[u], f);
#pragma unroll
                for (int i = 0; i < EPV; ++i) acc[i] = HAS_VAL ? fmaf(w[u], f[i], acc[i]) : acc[i] + f[i];
            }
        }
        if (j < nb) {
            // the U gathers are still issued back to back with no branch in between: an out-of-range slot re-reads the
            // batch's last valid edge (same cache lines as a live request) and is zeroed after the load
            int c[U];
            float w[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = j + u * SLOTS + slot;
                ok[u] = idx < nb;
                const int src = ok[u] ? idx : nb - 1;
                c[u] = __shfl(cur_col, src);
                w[u] = HAS_VAL ? __shfl(cur_val, src) : 1.0f;
            }
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = IO::load(xcol + (uint64_t)(uint32_t)c[u] * ld32);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(ok[u] ? v[u] : IO::zero(), f);
#pragma unroll
                for (int i = 0; i < EPV; ++i) acc[i] = HAS_VAL ? fmaf(w[u], f[i], acc[i]) : acc[i] + f[i];
            }
        }
    }
    // combine the slots: lanes that differ only in the slot bits hold the same columns
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
        for (int i = 0; i < EPV; ++i) acc[i] += __shfl_xor(acc[i], off);
    }
}

// acc[i] + the acc[i] of the lane whose id differs in bit OFF.  Inside a row of 16 lanes that is a DPP rotation (no LDS traffic).
template <int OFF> __device__ __forceinline__ float xor_lane(float v) {
    if constexpr (OFF == 8) return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /* row_ror:8 */, 0xf, 0xf, false));
    else return __shfl_xor(v, OFF);
}

// Unpack a gathered 16-byte register to floats, or to zeros where ok is false (an idle slot's request).  bf16: one v_perm_b32 per
// element whose selector moves the element's two bytes to the top of the word or picks zero bytes -- the mask costs nothing extra.
template <typename XT, int EPV>
__device__ __forceinline__ void unpack_if(const typename VecIO<XT, EPV>::raw_t& r, bool ok, float (&f)[EPV]) {
    if constexpr (sizeof(XT) == 2 && EPV == 8) {
        const uint32_t lo = ok ? 0x01000c0cu : 0x0c0c0c0cu, hi = ok ? 0x03020c0cu : 0x0c0c0c0cu;
        const uint32_t d[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = __uint_as_float(__builtin_amdgcn_perm(0u, d[i], lo));
            f[2 * i + 1] = __uint_as_float(__builtin_amdgcn_perm(0u, d[i], hi));
        }
    } else {
        VecIO<XT, EPV>::unpack(ok ? r : VecIO<XT, EPV>::zero(), f);
    }
}

// Group-local variant (spmm_rowgroup_kernel): the wavefront's SLOTS = 64 / LPR slots are shared by G = SLOTS / SPR rows, each on
// GL = SPR * LPR adjacent lanes.  b / n (first edge, edge count; n = 0: nothing to gather) are uniform inside a lane group and
// differ between the groups; all groups advance together until the longest row is done, finished groups masked and not branched.
// Every group fetches the next GL column ids (and weights) of ITS row with one coalesced load, hands them out inside the group
// and requests the following batch while the current one is consumed.  A round is SPR x U edges per row.
// Order of the sum: the wave-per-row kernel sends edge k of a round to its slot k % SLOTS at level k / SLOTS and adds its slots as
// a tree of adjacent pairs.  Here slot q of a row does the work of G of those slots, q G .. q G + G - 1, at U / G levels each: it
// adds them as that same tree before the round's sum goes into acc, and the slots of a row continue the tree.  So rows of at most
// SPR x U edges come out bit-identical to gather_edges(); longer rows differ in the last bits (fixed order, the same run to run).
template <typename XT, int EPV, int LPR, int SPR, bool HAS_VAL, int U>
__device__ __forceinline__ void gather_edges_grouped(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                     const XT* __restrict__ xcol, uint32_t ld32, int64_t b, int n, int lane,
                                                     float (&acc)[EPV]) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR, G = SLOTS / SPR, GL = SPR * LPR, UL = U / G, R = SPR * U;
    static_assert(SLOTS % SPR == 0 && G >= 1 && U % G == 0 && GL % R == 0, "row-group geometry");
    const int gl = lane % GL, gbase = lane - gl, q = gl / LPR;
    const int64_t off = b + gl;           // this lane's entry of the group's index batch (one offset for ids and weights)

    // the longest row of the wavefront, in a scalar register: every branch below is wave-uniform
    int nmax = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) nmax = max(nmax, __builtin_amdgcn_readlane(n, g * GL));

    int my_col = 0;
    float my_val = 0.0f;
    if (gl < n) {
        my_col = __builtin_nontemporal_load(col + off);
        if (HAS_VAL) my_val = __builtin_nontemporal_load(val + off);
    }
    for (int kb = 0; kb < nmax; kb += GL) {
        const int cur_col = my_col;       // a finished group keeps its last ids: its (masked) gathers re-read lines it has just used
        const float cur_val = my_val;
        if (kb + GL + gl < n) {
            my_col = __builtin_nontemporal_load(col + off + kb + GL);
            if (HAS_VAL) my_val = __builtin_nontemporal_load(val + off + kb + GL);
        }
#pragma unroll 1
        for (int j = 0; j < GL && kb + j < nmax; j += R) {
            int c[U];
            float w[U];
            bool ok[U];
#pragma unroll
            for (int m = 0; m < U; ++m) {
                const int idx = j + (m % UL) * SLOTS + q * G + m / UL;
                ok[m] = kb + idx < n;
                c[m] = __shfl(cur_col, gbase + idx);
                w[m] = HAS_VAL ? __shfl(cur_val, gbase + idx) : 1.0f;
            }
            typename IO::raw_t v[U];
#pragma unroll
            for (int m = 0; m < U; ++m) v[m] = IO::load(xcol + (uint64_t)(uint32_t)c[m] * ld32);
            float t[G][EPV];
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int l = 0; l < UL; ++l) {
                    const int m = g * UL + l;
                    float f[EPV];
                    unpack_if<XT, EPV>(v[m], ok[m], f);
#pragma unroll
                    for (int i = 0; i < EPV; ++i) {
                        if (l == 0) t[g][i] = HAS_VAL ? fmaf(w[m], f[i], 0.0f) : f[i];
                        else t[g][i] = HAS_VAL ? fmaf(w[m], f[i], t[g][i]) : t[g][i] + f[i];
                    }
                }
                if constexpr (G >= 2) {
                    if (g % 2 == 1) {     // the first tree level at once, and the scheduler kept from unpacking all U registers first
#pragma unroll
                        for (int i = 0; i < EPV; ++i) t[g - 1][i] += t[g][i];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
#pragma unroll
            for (int s = 2; s < G; s <<= 1) {
#pragma unroll
                for (int g = 0; g < G; g += 2 * s) {
#pragma unroll
                    for (int i = 0; i < EPV; ++i) t[g][i] += t[g + s][i];
                }
            }
#pragma unroll
            for (int i = 0; i < EPV; ++i) acc[i] += t[0][i];
        }
    }
    // combine the SPR slots of every row
    if constexpr (SPR >= 2) {
#pragma unroll
        for (int i = 0; i < EPV; ++i) acc[i] += xor_lane<LPR>(acc[i]);
    }
    if constexpr (SPR >= 4) {
#pragma unroll
        for (int i = 0; i < EPV; ++i) acc[i] += xor_lane<2 * LPR>(acc[i]);
    }
    static_assert(SPR <= 4, "row-group kernel: 2 or 4 slots per row");
}

}  // namespace dgll
