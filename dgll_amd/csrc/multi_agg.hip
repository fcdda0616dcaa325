// multi_agg.hip -- several neighbourhood reductions from ONE gather (PNA / DGL's PNAConv): the three passes of dgll_amd/ops_agg.py
// behind ONE entry point, dgll_hip_multi_agg_pass (include/dgll_hip.h: dgll_multi_agg_desc).
//
//   forward  rows of A     gathers x_j once per entry into a flat per-lane state -- per column: the sum and the sum of squares about a
//                          shift, the maximum and the minimum with the source rows that attain them -- and the row's epilogue writes
//                          out[i, (s * n_agg + a) * F + f] = scaler_s(i) * agg_a(i)[f], plus the row's mean / variance (stats) and the
//                          arg-max / arg-min source rows (arg) for the backward
//   rows     no gather     folds the scalers into the output gradient and writes, per row, the five coefficient vectors the next pass
//                          reads (coef fp32 [n_rows, 5 F]: c0 | c1 | mean | g_max | g_min) and grad_y
//   cols     rows of A^T   holds x_j; per entry i gathers the coefficients of row i:
//                          grad_x[j] = sum_i c0_i + c1_i (x_j - mean_i) + (argmax_i == j) g_max_i + (argmin_i == j) g_min_i
//                          c0 = g_sum + g_mean / D,  c1 = (2 g_var + g_std / std) / D where var > 0 and EXACTLY 0 elsewhere
//
// Two things are numerical requirements and not style:
//  * the variance is accumulated about a shift, the row's first entry (d = x_j - x_{col[b]}: every lane group of a long row can load
//    it): var = E[d^2] - E[d]^2 has lost the common offset, and a row whose entries are all equal gives d = 0, so var = 0 exactly and
//    std = sqrt(1e-30).  The raw form E[x^2] - E[x]^2 cancels, and with fused multiply-add does not even give 0 for a one-entry row;
//  * the variance term of the gradient is formed per entry as c1_i * (x_j - mean_i), x_j in registers; split into
//    x_j * sum c1_i - sum c1_i mean_i it would cancel at small std.  Where var <= 0 it is exactly 0 (relu'(0) = 0), or 1 / std = 1e15
//    would meet a rounding residue.
// Ties of max / min: among the entries attaining the extreme, the smallest source id -- independent of the sweep order, so that the
// long-row merge needs no positions.  A pair (j, i) stored more than once counts once for max / min (adjacent in the sorted rows of
// A^T: the first is kept), and once per entry for the other aggregators.
//
// Lane layout, tiles, index batches: row_tiles.hpp.  A row's `lpr` lanes are at least its F / EPV vectors; rows wider than 64 lanes are
// cut into column blocks of 64 vectors over blockIdx.y.  The long-row merge moves the state through LDS one pair of quantities at a
// time (2 * EPV floats per lane: 8 KB fp32, 16 KB bf16), in group order.  No atomics.  The column used for addressing is clamped.
#include "row_tiles.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace magg {

constexpr int kLongRow = DGLL_MAGG_LONG_ROW;    // rows longer than this are swept by a whole workgroup
constexpr float kStdEps = 1e-30f;               // std = sqrt(var + kStdEps), as DGL's PNAConv
constexpr int kCoefBlocks = 5;                  // c0 | c1 | mean | g_max | g_min
enum { kNeedLin = 1, kNeedVar = 2, kNeedMax = 4, kNeedMin = 8 };

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    int64_t n_rows, n_cols, tiles;
    const char* x;   int64_t pb_x;          // forward: the gathered matrix; cols: the held matrix (pitches in BYTES)
    const char* y;   int64_t pb_y;          // forward: the per-row addend or NULL
    const char* g;   int64_t pb_g;          // rows: grad_out
    char* out;       int64_t pb_out;        // forward: out; rows: grad_y (or NULL); cols: grad_x
    float* stats;    int64_t ld_stats;      // [*, 2 F]: mean | var
    int32_t* arg;    int64_t ld_arg;        // [*, 2 F]: argmax | argmin
    float* coef;     int64_t ld_coef;       // [*, 5 F]
    int64_t F, fb;                          // columns, and the bytes of F columns of the storage type (one block of out / grad_out)
    uint32_t aggs, scalers;                 // the ordered code lists, four bits a code, the first in the low bits
    int n_agg, n_scaler, need, vpr, lpr;    // need: kNeed* of the aggregators asked; vpr: 16-byte vectors of F columns
    float delta;
};

__device__ __forceinline__ float scaler_of(int code, float logd, float delta) {
    return code == DGLL_MAGG_AMPLIFICATION ? logd / delta : (code == DGLL_MAGG_ATTENUATION ? delta / logd : 1.0f);
}

// EPV fp32 (or int32, as bits) values at a 16-byte aligned address, four at a time
template <int EPV>
__device__ __forceinline__ void load_f32(const float* p, float (&f)[EPV]) {
#pragma unroll
    for (int q = 0; q < EPV; q += 4) {
        float t[4];
        VecIO<float, 4>::unpack(VecIO<float, 4>::load(p + q), t);
#pragma unroll
        for (int d = 0; d < 4; ++d) f[q + d] = t[d];
    }
}
template <int EPV>
__device__ __forceinline__ void store_f32(float* p, const float (&f)[EPV]) {
#pragma unroll
    for (int q = 0; q < EPV; q += 4) {
        const float t[4] = {f[q], f[q + 1], f[q + 2], f[q + 3]};
        VecIO<float, 4>::store(p + q, t);
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void magg_forward_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[2 * EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int tid = lanes.tid, lpr = lanes.lpr;
    const int v = (int)blockIdx.y * lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row of T,
    const int64_t ce = active ? (int64_t)v * EPV : 0;       // and element offset in a block of the fp32 / int32 side arrays

    float sh[EPV], s1[EPV], s2[EPV], mx[EPV], mn[EPV];      // shift; sum and sum of squares about it; maximum, minimum
    int amx[EPV], amn[EPV];                                 // the source rows attaining them

    auto load_row = [&](int64_t, int64_t b, int64_t e, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) {
            s1[d] = s2[d] = 0.0f;
            mx[d] = -INFINITY;
            mn[d] = INFINITY;
            amx[d] = amn[d] = 0x7fffffff;
        }
        typename IO::raw_t r = IO::zero();
        if (on && active && e > b) r = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)rt::clamp_index(a.col[b], (int)a.n_cols) * a.pb_x + cb));
        IO::unpack(r, sh);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t r[U];
            int c[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                c[u] = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                r[u] = IO::zero();
                if (ok[u]) r[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c[u] * a.pb_x + cb));
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float f[EPV];
                IO::unpack(r[u], f);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float dd = f[d] - sh[d];
                    s1[d] += dd;
                    s2[d] = fmaf(dd, dd, s2[d]);
                    if (f[d] > mx[d] || (f[d] == mx[d] && c[u] < amx[d])) { mx[d] = f[d]; amx[d] = c[u]; }
                    if (f[d] < mn[d] || (f[d] == mn[d] && c[u] < amn[d])) { mn[d] = f[d]; amn[d] = c[u]; }
                }
            }
        }
    };

    // the row's outputs from its complete state; no cross-lane traffic (the long-row path calls it from one lane group alone)
    auto finish = [&](int64_t row, int64_t b, int64_t e) {
        if (!active) return;
        const int64_t deg = e - b;
        const int blocks = a.n_agg * a.n_scaler;
        char* orow = a.out + row * a.pb_out + cb;
        float mean[EPV], var[EPV], o[EPV];
        if (deg == 0) {                                     // a row without entries: zeros in every block (y and the scalers do not apply)
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = 0.0f;
            for (int k = 0; k < blocks; ++k) IO::store(reinterpret_cast<T*>(orow + (int64_t)k * a.fb), o);
            if (a.stats) {
                store_f32<EPV>(a.stats + row * a.ld_stats + ce, o);
                store_f32<EPV>(a.stats + row * a.ld_stats + a.F + ce, o);
            }
            if (a.arg) {
#pragma unroll
                for (int d = 0; d < EPV; ++d) o[d] = __uint_as_float(0xffffffffu);      // -1
                store_f32<EPV>(reinterpret_cast<float*>(a.arg + row * a.ld_arg + ce), o);
                store_f32<EPV>(reinterpret_cast<float*>(a.arg + row * a.ld_arg + a.F + ce), o);
            }
            return;
        }
        const float fd = (float)deg, inv = 1.0f / fd, logd = logf(fd + 1.0f);
        float yv[EPV];
        {
            typename IO::raw_t r = IO::zero();
            if (a.y) r = IO::load(reinterpret_cast<const T*>(a.y + row * a.pb_y + cb));
            IO::unpack(r, yv);
        }
#pragma unroll
        for (int d = 0; d < EPV; ++d) {
            const float m1 = s1[d] * inv;
            mean[d] = sh[d] + m1;
            var[d] = fmaxf(fmaf(-m1, m1, s2[d] * inv), 0.0f);
        }
        for (int ai = 0; ai < a.n_agg; ++ai) {
            const int code = (int)((a.aggs >> (4 * ai)) & 15u);
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                float r;
                if (code == DGLL_MAGG_MEAN) r = mean[d] + yv[d];
                else if (code == DGLL_MAGG_SUM) r = fmaf(fd, yv[d], fmaf(fd, sh[d], s1[d]));
                else if (code == DGLL_MAGG_MAX) r = mx[d] + yv[d];
                else if (code == DGLL_MAGG_MIN) r = mn[d] + yv[d];
                else if (code == DGLL_MAGG_VAR) r = var[d];
                else r = sqrtf(var[d] + kStdEps);
                o[d] = r;
            }
            for (int si = 0; si < a.n_scaler; ++si) {
                const float sc = scaler_of((int)((a.scalers >> (4 * si)) & 15u), logd, a.delta);
                float w[EPV];
#pragma unroll
                for (int d = 0; d < EPV; ++d) w[d] = sc * o[d];
                IO::store(reinterpret_cast<T*>(orow + (int64_t)(si * a.n_agg + ai) * a.fb), w);
            }
        }
        if (a.stats) {
            store_f32<EPV>(a.stats + row * a.ld_stats + ce, mean);
            store_f32<EPV>(a.stats + row * a.ld_stats + a.F + ce, var);
        }
        if (a.arg) {
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = __uint_as_float((uint32_t)amx[d]);
            store_f32<EPV>(reinterpret_cast<float*>(a.arg + row * a.ld_arg + ce), o);
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = __uint_as_float((uint32_t)amn[d]);
            store_f32<EPV>(reinterpret_cast<float*>(a.arg + row * a.ld_arg + a.F + ce), o);
        }
    };

    // one pair of quantities of every lane group through LDS; the first lane group (sub == tid) takes the others' in group order
    auto exchange = [&](const float (&p)[EPV], const float (&q)[EPV]) {
        __syncthreads();                                    // the previous exchange has been read
#pragma unroll
        for (int d = 0; d < EPV; ++d) {
            lds[d * kBlock + tid] = p[d];
            lds[(EPV + d) * kBlock + tid] = q[d];
        }
        __syncthreads();
    };

    // rt::sweep_rows written out: through the header the fp32 kernel's registers are numbered differently (a refactor does
    // not change instruction text).  A long row: the first lane group takes the others' sums, then maxima, then minima, and writes it.
    auto short_row = [&](int64_t row, bool mine, int64_t b, int64_t e) {
        load_row(row, b, e, mine);
        rt::for_each_batch(b, e, 0, 1, lanes, batch);
        if (mine) finish(row, b, e);
    };
    auto long_row = [&](int64_t row, int64_t b, int64_t e) {
        load_row(row, b, e, true);
        rt::for_each_batch(b, e, lanes.gid, lanes.groups, lanes, batch);
        float bits[EPV];
        exchange(s1, s2);
        if (tid < lpr) {
            for (int p = 1; p < lanes.groups; ++p) {
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    s1[d] += lds[d * kBlock + p * lpr + tid];
                    s2[d] += lds[(EPV + d) * kBlock + p * lpr + tid];
                }
            }
        }
#pragma unroll
        for (int d = 0; d < EPV; ++d) bits[d] = __uint_as_float((uint32_t)amx[d]);
        exchange(mx, bits);
        if (tid < lpr) {
            for (int p = 1; p < lanes.groups; ++p) {
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float o = lds[d * kBlock + p * lpr + tid];
                    const int oa = (int)__float_as_uint(lds[(EPV + d) * kBlock + p * lpr + tid]);
                    if (o > mx[d] || (o == mx[d] && oa < amx[d])) { mx[d] = o; amx[d] = oa; }
                }
            }
        }
#pragma unroll
        for (int d = 0; d < EPV; ++d) bits[d] = __uint_as_float((uint32_t)amn[d]);
        exchange(mn, bits);
        if (tid < lpr) {
            for (int p = 1; p < lanes.groups; ++p) {
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float o = lds[d * kBlock + p * lpr + tid];
                    const int oa = (int)__float_as_uint(lds[(EPV + d) * kBlock + p * lpr + tid]);
                    if (o < mn[d] || (o == mn[d] && oa < amn[d])) { mn[d] = o; amn[d] = oa; }
                }
            }
            finish(row, b, e);
        }
    };
    rt::for_each_tile(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, short_row, long_row);
}

// ---- rows: element-wise per row, no gather ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void magg_rows_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T);
    using IO = VecIO<T, EPV>;
    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    if (v >= a.vpr) return;                                 // (no collectives in this kernel)
    const int64_t cb = (int64_t)v * 16, ce = (int64_t)v * EPV;

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row = tile * lanes.groups + lanes.gid;
        if (row >= a.n_rows) continue;
        const int64_t deg = a.rowptr[row + 1] - a.rowptr[row];
        float c0[EPV], c1[EPV], gmx[EPV], gmn[EPV], gy[EPV], mean[EPV], var[EPV];
#pragma unroll
        for (int d = 0; d < EPV; ++d) c0[d] = c1[d] = gmx[d] = gmn[d] = gy[d] = mean[d] = var[d] = 0.0f;
        if (deg > 0) {                                      // (a row without entries: zeros, its blocks of out did not depend on anything)
            const float fd = (float)deg, inv = 1.0f / fd, logd = logf(fd + 1.0f);
            if (a.stats) {
                load_f32<EPV>(a.stats + row * a.ld_stats + ce, mean);
                load_f32<EPV>(a.stats + row * a.ld_stats + a.F + ce, var);
            }
            const char* grow = a.g + row * a.pb_g + cb;
            for (int ai = 0; ai < a.n_agg; ++ai) {
                const int code = (int)((a.aggs >> (4 * ai)) & 15u);
                float ga[EPV];                              // the aggregator's gradient, the scalers folded
#pragma unroll
                for (int d = 0; d < EPV; ++d) ga[d] = 0.0f;
                for (int si = 0; si < a.n_scaler; ++si) {
                    const float sc = scaler_of((int)((a.scalers >> (4 * si)) & 15u), logd, a.delta);
                    float f[EPV];
                    IO::unpack(IO::load(reinterpret_cast<const T*>(grow + (int64_t)(si * a.n_agg + ai) * a.fb)), f);
#pragma unroll
                    for (int d = 0; d < EPV; ++d) ga[d] = fmaf(sc, f[d], ga[d]);
                }
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    if (code == DGLL_MAGG_MEAN) { c0[d] = fmaf(ga[d], inv, c0[d]); gy[d] += ga[d]; }
                    else if (code == DGLL_MAGG_SUM) { c0[d] += ga[d]; gy[d] = fmaf(fd, ga[d], gy[d]); }
                    else if (code == DGLL_MAGG_MAX) { gmx[d] = ga[d]; gy[d] += ga[d]; }
                    else if (code == DGLL_MAGG_MIN) { gmn[d] = ga[d]; gy[d] += ga[d]; }
                    else if (code == DGLL_MAGG_VAR) { if (var[d] > 0.0f) c1[d] = fmaf(2.0f * ga[d], inv, c1[d]); }
                    else { if (var[d] > 0.0f) c1[d] = fmaf(ga[d] / sqrtf(var[d] + kStdEps), inv, c1[d]); }
                }
            }
        }
        if (a.coef) {
            float* crow = a.coef + row * a.ld_coef + ce;
            store_f32<EPV>(crow, c0);
            store_f32<EPV>(crow + a.F, c1);
            store_f32<EPV>(crow + 2 * a.F, mean);
            store_f32<EPV>(crow + 3 * a.F, gmx);
            store_f32<EPV>(crow + 4 * a.F, gmn);
        }
        if (a.out) IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), gy);
    }
}

// ---- cols: rows of A^T ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void magg_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T);
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0, ce = active ? (int64_t)v * EPV : 0;
    const bool lin = a.need & kNeedLin, sq = a.need & kNeedVar, hi = a.need & kNeedMax, lo = a.need & kNeedMin;

    float acc[EPV], xj[EPV];
    int64_t row_b = 0;                                      // the current row and its first entry
    int cur = 0;

    auto load_row = [&](int64_t row, int64_t b, int64_t, bool on) {
        row_b = b;
        cur = (int)row;
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = 0.0f;
        typename IO::raw_t r = IO::zero();
        if (on && active) r = IO::load(reinterpret_cast<const T*>(a.x + row * a.pb_x + cb));
        IO::unpack(r, xj);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        int my_keep = 0;                                    // the first of a run of equal entries (the rows of A^T are sorted)
        if (lanes.sub < nb) {
            const int64_t k = k0 + lanes.sub;
            my_keep = k == row_b || a.col[k - 1] != a.col[k] ? 1 : 0;
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; ++t) {
            const int64_t i = rt::hand_round(my_col, t, lanes);
            const int keep = rt::hand_round(my_keep, t, lanes);
            if (!(t < nb && active)) continue;
            const float* crow = a.coef + i * a.ld_coef + ce;
            float c[EPV], m[EPV];
            if (lin) {
                load_f32<EPV>(crow, c);
#pragma unroll
                for (int d = 0; d < EPV; ++d) acc[d] += c[d];
            }
            if (sq) {                                       // per entry, never x_j * sum c1 - sum c1 mean
                load_f32<EPV>(crow + a.F, c);
                load_f32<EPV>(crow + 2 * a.F, m);
#pragma unroll
                for (int d = 0; d < EPV; ++d) acc[d] = fmaf(c[d], xj[d] - m[d], acc[d]);
            }
            if (hi && keep) {
                load_f32<EPV>(crow + 3 * a.F, c);
                load_f32<EPV>(reinterpret_cast<const float*>(a.arg + i * a.ld_arg + ce), m);
#pragma unroll
                for (int d = 0; d < EPV; ++d)
                    if ((int)__float_as_uint(m[d]) == cur) acc[d] += c[d];
            }
            if (lo && keep) {
                load_f32<EPV>(crow + 4 * a.F, c);
                load_f32<EPV>(reinterpret_cast<const float*>(a.arg + i * a.ld_arg + a.F + ce), m);
#pragma unroll
                for (int d = 0; d < EPV; ++d)
                    if ((int)__float_as_uint(m[d]) == cur) acc[d] += c[d];
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), acc);     // a source no row references: zeros
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, load_row, batch, finish);
}

template <typename T>
void launch(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_MAGG_FORWARD) hipLaunchKernelGGL((magg_forward_kernel<T>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_MAGG_ROWS) hipLaunchKernelGGL((magg_rows_kernel<T>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((magg_cols_kernel<T>), grid, dim3(kBlock), 0, s, a);
}

// an fp32 / int32 side array of `blocks` blocks of F columns: 16-byte aligned, a pitch of whole 16-byte vectors >= blocks * F
inline bool side_array(const void* p, int64_t ld, int64_t blocks, int64_t F) { return p && aligned16(p) && ld % 4 == 0 && ld >= blocks * F; }

}  // namespace magg
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_multi_agg_pass(void* stream, const dgll_multi_agg_desc* d) {
    static const char* const kPass = "dgll_hip_multi_agg_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_multi_agg_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_MAGG_FORWARD || d->pass == DGLL_MAGG_ROWS || d->pass == DGLL_MAGG_COLS,
                 "dgll_hip_multi_agg_pass: pass must be DGLL_MAGG_FORWARD, DGLL_MAGG_ROWS or DGLL_MAGG_COLS");
    const bool fwd = d->pass == DGLL_MAGG_FORWARD, rows = d->pass == DGLL_MAGG_ROWS;
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, 0, d->rowptr, d->col, !rows)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    DGLL_REQUIRE(d->n_agg >= 1 && d->n_agg <= 6, "dgll_hip_multi_agg_pass: n_agg in [1, 6]");
    DGLL_REQUIRE(d->n_scaler >= 1 && d->n_scaler <= 3, "dgll_hip_multi_agg_pass: n_scaler in [1, 3]");
    uint32_t aggs = 0, scalers = 0;
    int seen = 0, need = 0;
    for (int i = 0; i < d->n_agg; ++i) {
        const int c = d->agg[i];
        DGLL_REQUIRE(c >= DGLL_MAGG_MEAN && c <= DGLL_MAGG_STD, "dgll_hip_multi_agg_pass: agg: unknown aggregator code (DGLL_MAGG_MEAN .. DGLL_MAGG_STD)");
        DGLL_REQUIRE(!(seen >> c & 1), "dgll_hip_multi_agg_pass: agg: an aggregator code is repeated");
        seen |= 1 << c;
        aggs |= (uint32_t)c << (4 * i);
        need |= c == DGLL_MAGG_MEAN || c == DGLL_MAGG_SUM ? magg::kNeedLin
                : (c == DGLL_MAGG_MAX ? magg::kNeedMax : (c == DGLL_MAGG_MIN ? magg::kNeedMin : magg::kNeedVar));
    }
    seen = 0;
    for (int i = 0; i < d->n_scaler; ++i) {
        const int c = d->scaler[i];
        DGLL_REQUIRE(c >= DGLL_MAGG_IDENTITY && c <= DGLL_MAGG_ATTENUATION,
                     "dgll_hip_multi_agg_pass: scaler: unknown scaler code (DGLL_MAGG_IDENTITY .. DGLL_MAGG_ATTENUATION)");
        DGLL_REQUIRE(!(seen >> c & 1), "dgll_hip_multi_agg_pass: scaler: a scaler code is repeated");
        seen |= 1 << c;
        scalers |= (uint32_t)c << (4 * i);
    }
    DGLL_REQUIRE(d->delta > 0.0f && d->delta < INFINITY, "dgll_hip_multi_agg_pass: delta must be a positive finite number");
    const bool need_var = need & magg::kNeedVar, need_arg = need & (magg::kNeedMax | magg::kNeedMin);

    magg::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.F = d->F;
    a.fb = d->F * esz;
    a.aggs = aggs;
    a.scalers = scalers;
    a.n_agg = d->n_agg;
    a.n_scaler = d->n_scaler;
    a.need = need;
    a.delta = d->delta;
    if (fwd) {
        DGLL_REQUIRE_OPERAND(kPass, x, d->F);
        if (d->y) DGLL_REQUIRE_OPERAND(kPass, y, d->F);
        DGLL_REQUIRE_OPERAND(kPass, out, d->n_scaler * d->n_agg * d->F);
        DGLL_REQUIRE(!d->stats || magg::side_array(d->stats, d->ld_stats, 2, d->F),
                     "dgll_hip_multi_agg_pass: forward: stats, where given, 16-byte aligned fp32 on a pitch of whole vectors >= 2 F");
        DGLL_REQUIRE(!d->arg || magg::side_array(d->arg, d->ld_arg, 2, d->F),
                     "dgll_hip_multi_agg_pass: forward: arg, where given, 16-byte aligned int32 on a pitch of whole vectors >= 2 F");
        a.x = static_cast<const char*>(d->x);       a.pb_x = d->ld_x * esz;
        a.y = static_cast<const char*>(d->y);       a.pb_y = d->ld_y * esz;
        a.out = static_cast<char*>(d->out);         a.pb_out = d->ld_out * esz;
        a.stats = d->stats;                         a.ld_stats = d->ld_stats;
        a.arg = d->arg;                             a.ld_arg = d->ld_arg;
    } else if (rows) {
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->n_scaler * d->n_agg * d->F);
        DGLL_REQUIRE(d->coef || d->grad_y, "dgll_hip_multi_agg_pass: rows: one of coef and grad_y must be given");
        DGLL_REQUIRE(!d->coef || magg::side_array(d->coef, d->ld_coef, magg::kCoefBlocks, d->F),
                     "dgll_hip_multi_agg_pass: rows: coef, where given, 16-byte aligned fp32 on a pitch of whole vectors >= 5 F");
        DGLL_REQUIRE(!(d->coef && need_var) || d->stats, "dgll_hip_multi_agg_pass: rows: stats must be non-NULL when VAR or STD is asked");
        DGLL_REQUIRE(!d->stats || magg::side_array(d->stats, d->ld_stats, 2, d->F),
                     "dgll_hip_multi_agg_pass: rows: stats 16-byte aligned fp32 on a pitch of whole vectors >= 2 F");
        if (d->grad_y) DGLL_REQUIRE_OPERAND(kPass, grad_y, d->F);
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.stats = d->stats;                             a.ld_stats = d->ld_stats;
        a.coef = d->coef;                               a.ld_coef = d->ld_coef;
        a.out = static_cast<char*>(d->grad_y);          a.pb_out = d->ld_grad_y * esz;
    } else {
        DGLL_REQUIRE_OPERAND(kPass, x, d->F);
        DGLL_REQUIRE(magg::side_array(d->coef, d->ld_coef, magg::kCoefBlocks, d->F),
                     "dgll_hip_multi_agg_pass: cols: coef non-NULL, 16-byte aligned fp32 on a pitch of whole vectors >= 5 F");
        DGLL_REQUIRE(!need_arg || magg::side_array(d->arg, d->ld_arg, 2, d->F),
                     "dgll_hip_multi_agg_pass: cols: arg non-NULL (MAX or MIN is asked), 16-byte aligned int32 on a pitch of whole vectors >= 2 F");
        DGLL_REQUIRE_OPERAND(kPass, grad_x, d->F);
        a.x = static_cast<const char*>(d->x);           a.pb_x = d->ld_x * esz;
        a.coef = d->coef;                               a.ld_coef = d->ld_coef;
        a.arg = d->arg;                                 a.ld_arg = d->ld_arg;
        a.out = static_cast<char*>(d->grad_x);          a.pb_out = d->ld_grad_x * esz;
    }
    a.vpr = (int)(d->F / epv);
    const rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) magg::launch<float>(d->pass, grid, st, a);
    else magg::launch<bf16_t>(d->pass, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
