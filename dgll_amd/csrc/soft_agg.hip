// soft_agg.hip -- the learnable per-column soft reductions of DeeperGCN (PyG's GENConv: SoftmaxAggregation, PowerMeanAggregation) and their
// exact backward.  The three passes of dgll_amd/ops_softagg.py behind ONE entry point, dgll_hip_soft_agg_pass (include/dgll_hip.h:
// dgll_soft_agg_desc).  Entry k of row i of A is the edge j = col[k] -> i, e[k] its row (optional).  For every column, with theta = t or p
// (ONE fp32 in device memory, read by the kernels: the host never sees its value) and g = grad_out:
//
//   m_k = relu(x_j + e_k) + eps      gate_k = (x_j + e_k > 0)
//   softmax:     a_k = exp(t m_k - lse_i)      out_i = sum_k a_k m_k        dout/dm_k = a_k (1 + t (m_k - out_i))   (semi_grad: a_k)
//                                                                          dout/dt   = sum_k a_k (m_k - out_i)^2   (= sum a m^2 - out^2)
//   power-mean:  mc_k = min(m_k, 100)  S_i = sum_k mc_k^p   out_i = (S_i / deg_i)^(1/p)
//                                                                          dout/dm_k = (out_i / S_i) mc_k^(p-1)     (0 where m_k > 100)
//                                                                          dout/dp   = (out_i / p) sum_k (mc_k^p / S_i) (ln mc_k - ln out_i)
//   (both scalar derivatives are written as ONE sum over the row's entries -- sum_k a_k = 1 and sum_k mc_k^p / S_i = 1 take the row's own
//   term inside -- so the rows pass needs no reduction per row and a long row only shares its entries among the lane groups)
//
//   forward  rows of A     x_j gathered, e_k streamed; softmax: an online softmax PER COLUMN in exp2 form, state {max, l, acc} x EPV per
//                          lane; power-mean: S.  One store of out_i and of the fp32 row statistics (softmax {lse | out}, power {out | S})
//                          at the row's end, nothing per edge
//   rows     rows of A     g_i and the row's statistics held, x_j gathered, e_k read: grad_e[k] = g_i dout/dm_k gate_k (one store per entry),
//                          and the scalar gradient: every lane sums its entries' terms over the tiles of its workgroup, the workgroup
//                          reduces its lanes in a fixed order into ONE fp32 partial, soft_agg_sum_kernel adds the partials in workgroup
//                          order.  No float atomics: two runs give the same bits
//   cols     rows of A^T   x_j held, g_i and the statistics of row i gathered (i = colT[k']), e at slot perm[k']: grad_x[j]
//
// message() forms m and the gate in every pass: the same fp32 sum of the same two STORED values (an add alone: nothing to contract), so the
// forward's relu and the backward's gates agree bit for bit.  Without e the sum is x_j + 0.
//
// Lane layout, tiles, index batches: row_tiles.hpp (rt::make_flat_geometry).  A row's `lpr` lanes are at least its F / EPV vectors; rows
// wider than 64 lanes are cut into column blocks of 64 vectors over blockIdx.y.  Two entries in flight per lane.  The long-row merge of
// the forward is merge_columns below -- rt::merge_partials<true> assumes ONE maximum at st[0]; here every column has its own, so the
// rescale is per column -- in group order; that of cols is rt::merge_partials<false>.  col and perm values used for addressing are clamped.
#include "row_tiles.hpp"

namespace dgll {
namespace soft_agg {

constexpr int kLongRow = DGLL_SOFT_AGG_LONG_ROW;    // rows longer than this are swept by a whole workgroup
constexpr float kClamp = 100.0f;                    // power-mean: messages are clamped to [eps, 100] (PyG's PowerMeanAggregation)

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;                    // cols: A^T's entry -> A's entry (the slot of e)
    const float* theta;                     // t or p
    int64_t n_rows, n_cols, nnz, tiles;
    float eps;
    int semi;                               // softmax: dout/dm is a_k alone
    const char* x;   int64_t pb_x;          // pitches in BYTES
    const char* e;   int64_t pb_e;
    const char* g;   int64_t pb_g;
    const float* st; int64_t ld_st;         // the row statistics, pitch in floats
    char* out;       int64_t pb_out;        // forward: out; cols: grad_x; rows: grad_e (or NULL)
    float* st_out;                          // forward: the statistics
    float* partials;                        // rows: one fp32 per workgroup (or NULL: no scalar gradient)
    int vpr, lpr;                           // 16-byte vectors of F columns; lanes of a row
};

// m and the gate of one element, in every pass
__device__ __forceinline__ float message(float x, float e, float eps, bool& gate) {
    const float s = x + e;
    gate = s > 0.0f;
    return (gate ? s : 0.0f) + eps;
}

template <int EPV>
__device__ __forceinline__ void load_f32(const float* p, float (&f)[EPV]) {
#pragma unroll
    for (int q = 0; q < EPV / 4; ++q) {
        float part[4];
        VecIO<float, 4>::unpack(VecIO<float, 4>::load(p + 4 * q), part);
#pragma unroll
        for (int d = 0; d < 4; ++d) f[4 * q + d] = part[d];
    }
}

template <int EPV>
__device__ __forceinline__ void store_f32(float* p, const float (&f)[EPV]) {
#pragma unroll
    for (int q = 0; q < EPV / 4; ++q) {
        const float part[4] = {f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
        VecIO<float, 4>::store(p + 4 * q, part);
    }
}

// What the backward needs of a row, from its statistics and theta; weight(m, dm, dth): dm = dout/dm_k and dth = the entry's term of
// dout/dtheta, both for one element.
//   softmax  c0 = lse (log2 units), c1 = out;  power  c0 = out / S (0 for an empty or degenerate row), c1 = log2 out
template <int MODE>
__device__ __forceinline__ void row_terms(float s0, float s1, float& c0, float& c1) {
    if constexpr (MODE == DGLL_SOFT_AGG_SOFTMAX) {
        c0 = s0 * rt::kLog2e;
        c1 = s1;
    } else {
        const bool ok = s0 > 0.0f && s1 > 0.0f;
        c0 = ok ? s0 / s1 : 0.0f;
        c1 = ok ? __builtin_amdgcn_logf(s0) : 0.0f;
    }
}

template <int MODE>
__device__ __forceinline__ void weight(float m, float th, float c0, float c1, bool semi, float& dm, float& dth) {
    if constexpr (MODE == DGLL_SOFT_AGG_SOFTMAX) {
        const float a = __builtin_amdgcn_exp2f(fmaf(th * rt::kLog2e, m, -c0));
        dm = semi ? a : a * fmaf(th, m - c1, 1.0f);
        dth = a * (m - c1) * (m - c1);               // sum_k a_k (m_k - out)^2 = sum_k a_k m_k^2 - out^2, without the cancellation
    } else {
        const float mc = fminf(m, kClamp), l2 = __builtin_amdgcn_logf(mc);
        const float w = c0 * __builtin_amdgcn_exp2f(th * l2);        // (out / S) mc^p
        dm = m > kClamp ? 0.0f : w / mc;
        dth = w * (l2 - c1) * rt::kLn2 / th;
    }
}

// The forward's long-row merge: every lane group's state goes through lds (NS * kBlock floats), one column of the lane's EPV at a time, and
// the first lane group adds the others to its own in group order; softmax: as online-softmax states {max (log2 units), l, acc} of that
// column, rescaled to the larger maximum (rt::merge_partials has one maximum for the whole state).  Then done().
template <int MODE, int EPV, int NS, typename Done>
__device__ __forceinline__ void merge_columns(float (&st)[NS * EPV], float* lds, const rt::Lanes& L, Done&& done) {
#pragma unroll
    for (int d = 0; d < EPV; ++d) {
        __syncthreads();                            // the previous merge has read its partials
#pragma unroll
        for (int s = 0; s < NS; ++s) lds[s * kBlock + L.tid] = st[s * EPV + d];
        __syncthreads();
        if (L.tid < L.lpr) {
            for (int p = 1; p < L.groups; ++p) {
                float o[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) o[s] = lds[s * kBlock + p * L.lpr + L.tid];
                if constexpr (MODE == DGLL_SOFT_AGG_SOFTMAX) {
                    const float mn = fmaxf(st[d], o[0]);
                    const float s0 = st[d] == mn ? 1.0f : __builtin_amdgcn_exp2f(st[d] - mn);
                    const float s1 = o[0] == mn ? 1.0f : __builtin_amdgcn_exp2f(o[0] - mn);
                    st[d] = mn;
#pragma unroll
                    for (int s = 1; s < NS; ++s) st[s * EPV + d] = fmaf(st[s * EPV + d], s0, o[s] * s1);
                } else {
#pragma unroll
                    for (int s = 0; s < NS; ++s) st[s * EPV + d] += o[s];
                }
            }
        }
    }
    if (L.tid < L.lpr) done();
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE, bool HAS_E>
__global__ __launch_bounds__(kBlock) void soft_agg_forward_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    constexpr bool kSoftmax = MODE == DGLL_SOFT_AGG_SOFTMAX;
    constexpr int NS = kSoftmax ? 3 : 1;                    // softmax: [0, EPV) max, [EPV, 2 EPV) l, [2 EPV, 3 EPV) acc; power: S
    using IO = VecIO<T, EPV>;
    __shared__ float lds[NS * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row of T
    const float th = *a.theta, ts = th * rt::kLog2e, eps = a.eps;

    float st[NS * EPV];

    auto load_row = [&](int64_t, int64_t, int64_t, bool) {
#pragma unroll
        for (int d = 0; d < NS * EPV; ++d) st[d] = 0.0f;
        if constexpr (kSoftmax) {
#pragma unroll
            for (int d = 0; d < EPV; ++d) st[d] = -INFINITY;
        }
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rx[U], re[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = re[u] = IO::zero();
                if (ok[u]) {
                    rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    if constexpr (HAS_E) re[u] = IO::load(reinterpret_cast<const T*>(a.e + (k0 + t + u) * a.pb_e + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fx[EPV], fe[EPV];
                IO::unpack(rx[u], fx);
                IO::unpack(re[u], fe);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    bool gate;
                    const float m = message(fx[d], fe[d], eps, gate);
                    if constexpr (kSoftmax) {
                        const float z = ts * m, mn = fmaxf(st[d], z);
                        const float s0 = __builtin_amdgcn_exp2f(st[d] - mn), w = __builtin_amdgcn_exp2f(z - mn);
                        st[d] = mn;
                        st[EPV + d] = fmaf(st[EPV + d], s0, w);
                        st[2 * EPV + d] = fmaf(st[2 * EPV + d], s0, w * m);
                    } else {
                        st[d] += __builtin_amdgcn_exp2f(th * __builtin_amdgcn_logf(fminf(m, kClamp)));
                    }
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t b, int64_t e) {
        if (!active) return;
        float o[EPV], s[EPV];                               // a row without entries: zeros in out and in the statistics
#pragma unroll
        for (int d = 0; d < EPV; ++d) {
            o[d] = s[d] = 0.0f;
            if (e > b) {
                if constexpr (kSoftmax) {
                    o[d] = st[2 * EPV + d] / st[EPV + d];
                    s[d] = (st[d] + __builtin_amdgcn_logf(st[EPV + d])) * rt::kLn2;
                } else {
                    s[d] = st[d];
                    o[d] = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(st[d] / (float)(e - b)) / th);
                }
            }
        }
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);
        float* sp = a.st_out + row * a.ld_st + (int64_t)v * EPV;
        const int64_t half = (int64_t)a.vpr * EPV;          // F
        store_f32<EPV>(sp, kSoftmax ? s : o);               // softmax {lse | out}, power {out | S}
        store_f32<EPV>(sp + half, kSoftmax ? o : s);
    };

    auto long_done = [&](int64_t row, int64_t b, int64_t e) { merge_columns<MODE, EPV, NS>(st, lds, lanes, [&] { finish(row, b, e); }); };
    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, load_row, batch, finish, long_done);
}

// ---- rows: grad_e per entry and the workgroup's share of the scalar gradient ---------------------------------------------------------------
template <typename T, int MODE, bool HAS_E>
__global__ __launch_bounds__(kBlock) void soft_agg_rows_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[kWavesPerBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const float th = *a.theta, eps = a.eps;
    const bool semi = a.semi != 0, need_e = a.out != nullptr;       // uniform: kernel arguments

    float gi[EPV], c0[EPV], c1[EPV];
    float sum = 0.0f;                                       // this lane's share of the scalar gradient

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        typename IO::raw_t r = IO::zero();
        float s0[EPV], s1[EPV];
#pragma unroll
        for (int d = 0; d < EPV; ++d) s0[d] = s1[d] = 0.0f;
        if (on && active) {
            r = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
            const float* sp = a.st + row * a.ld_st + (int64_t)v * EPV;
            load_f32<EPV>(sp, s0);
            load_f32<EPV>(sp + (int64_t)a.vpr * EPV, s1);
        }
        IO::unpack(r, gi);
#pragma unroll
        for (int d = 0; d < EPV; ++d) row_terms<MODE>(s0[d], s1[d], c0[d], c1[d]);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rx[U], re[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = re[u] = IO::zero();
                if (ok[u]) {
                    rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    if constexpr (HAS_E) re[u] = IO::load(reinterpret_cast<const T*>(a.e + (k0 + t + u) * a.pb_e + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fx[EPV], fe[EPV], o[EPV];
                IO::unpack(rx[u], fx);
                IO::unpack(re[u], fe);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    bool gate;
                    const float m = message(fx[d], fe[d], eps, gate);
                    float dm, dth;
                    weight<MODE>(m, th, c0[d], c1[d], semi, dm, dth);
                    o[d] = gate ? gi[d] * dm : 0.0f;
                    sum = fmaf(gi[d], dth, sum);
                }
                if constexpr (HAS_E) {
                    if (need_e) IO::store(reinterpret_cast<T*>(a.out + (k0 + t + u) * a.pb_out + cb), o);
                }
            }
        }
    };

    // (a long row: every lane group holds g_i and the statistics and takes its share of the entries)
    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, load_row, batch);

    if (a.partials == nullptr) return;                      // uniform
    // the workgroup's lanes in a fixed order: a butterfly inside each wavefront, then the four wavefronts in turn
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lanes.lane == 0) lds[lanes.wave] = sum;
    __syncthreads();
    if (lanes.tid == 0) {
        float total = lds[0];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) total += lds[w];
        a.partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
    }
}

// n partials in workgroup order -> out[0]: thread t adds partials t, t + 256, ... in that order, then the 256 sums are added as a
// fixed tree.  One workgroup.
__global__ __launch_bounds__(kBlock) void soft_agg_sum_kernel(const float* partials, int64_t n, float* out) {
    __shared__ float lds[kBlock];
    const int tid = (int)threadIdx.x;
    float s = 0.0f;
    for (int64_t i = tid; i < n; i += kBlock) s += partials[i];
    lds[tid] = s;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if (tid < half) lds[tid] += lds[tid + half];
        __syncthreads();
    }
    if (tid == 0) out[0] = lds[0];
}

// ---- cols: rows of A^T ---------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE, bool HAS_E>
__global__ __launch_bounds__(kBlock) void soft_agg_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const float th = *a.theta, eps = a.eps;
    const bool semi = a.semi != 0;

    float acc[EPV], xj[EPV];

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = 0.0f;
        typename IO::raw_t r = IO::zero();
        if (on && active) r = IO::load(reinterpret_cast<const T*>(a.x + row * a.pb_x + cb));
        IO::unpack(r, xj);
    };

    // one batch of the row's entries, two in flight; the slot of e travels with the index
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        int my_slot = 0;
        if constexpr (HAS_E) {
            if (lanes.sub < nb) {
                const int64_t s = a.perm[k0 + lanes.sub];
                my_slot = (int)max((int64_t)0, min(s, a.nnz - 1));
            }
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rg[U], re[U];
            float s0[U][EPV], s1[U][EPV];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = rt::hand_round(my_col, t + u, lanes);
                int slot = 0;
                if constexpr (HAS_E) slot = rt::hand_round(my_slot, t + u, lanes);
                ok[u] = t + u < nb && active;
                rg[u] = re[u] = IO::zero();
#pragma unroll
                for (int d = 0; d < EPV; ++d) s0[u][d] = s1[u][d] = 0.0f;
                if (ok[u]) {
                    rg[u] = IO::load(reinterpret_cast<const T*>(a.g + (int64_t)i * a.pb_g + cb));
                    const float* sp = a.st + (int64_t)i * a.ld_st + (int64_t)v * EPV;
                    load_f32<EPV>(sp, s0[u]);
                    load_f32<EPV>(sp + (int64_t)a.vpr * EPV, s1[u]);
                    if constexpr (HAS_E) re[u] = IO::load(reinterpret_cast<const T*>(a.e + (int64_t)slot * a.pb_e + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fg[EPV], fe[EPV];
                IO::unpack(rg[u], fg);
                IO::unpack(re[u], fe);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    bool gate;
                    const float m = message(xj[d], fe[d], eps, gate);
                    float c0, c1, dm, dth;
                    row_terms<MODE>(s0[u][d], s1[u][d], c0, c1);
                    weight<MODE>(m, th, c0, c1, semi, dm, dth);
                    acc[d] += gate ? fg[d] * dm : 0.0f;
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), acc);     // a source no row references: zeros
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, load_row, batch, finish);
}

template <typename T, int MODE, bool HAS_E>
void launch_e(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_SOFT_AGG_FORWARD) hipLaunchKernelGGL((soft_agg_forward_kernel<T, MODE, HAS_E>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_SOFT_AGG_ROWS) hipLaunchKernelGGL((soft_agg_rows_kernel<T, MODE, HAS_E>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((soft_agg_cols_kernel<T, MODE, HAS_E>), grid, dim3(kBlock), 0, s, a);
}

template <typename T>
void launch(int pass, int mode, bool has_e, dim3 grid, hipStream_t s, const Args& a) {
    if (mode == DGLL_SOFT_AGG_SOFTMAX) {
        if (has_e) launch_e<T, DGLL_SOFT_AGG_SOFTMAX, true>(pass, grid, s, a);
        else launch_e<T, DGLL_SOFT_AGG_SOFTMAX, false>(pass, grid, s, a);
    } else {
        if (has_e) launch_e<T, DGLL_SOFT_AGG_POWER, true>(pass, grid, s, a);
        else launch_e<T, DGLL_SOFT_AGG_POWER, false>(pass, grid, s, a);
    }
}

}  // namespace soft_agg
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_soft_agg_pass(void* stream, const dgll_soft_agg_desc* d) {
    static const char* const kPass = "dgll_hip_soft_agg_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_soft_agg_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_SOFT_AGG_FORWARD || d->pass == DGLL_SOFT_AGG_ROWS || d->pass == DGLL_SOFT_AGG_COLS,
                 "dgll_hip_soft_agg_pass: pass must be DGLL_SOFT_AGG_FORWARD, DGLL_SOFT_AGG_ROWS or DGLL_SOFT_AGG_COLS");
    DGLL_REQUIRE(d->mode == DGLL_SOFT_AGG_SOFTMAX || d->mode == DGLL_SOFT_AGG_POWER,
                 "dgll_hip_soft_agg_pass: mode must be DGLL_SOFT_AGG_SOFTMAX or DGLL_SOFT_AGG_POWER");
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, d->nnz, d->rowptr, d->col, true)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    DGLL_REQUIRE(d->theta != nullptr, "dgll_hip_soft_agg_pass: theta (t or p: one fp32 value in device memory) must be non-NULL");
    DGLL_REQUIRE(d->eps >= 0.0f, "dgll_hip_soft_agg_pass: eps must be >= 0");
    DGLL_REQUIRE(d->stats != nullptr, "dgll_hip_soft_agg_pass: stats (the fp32 row statistics [n_dst, 2 F]) must be non-NULL");
    DGLL_REQUIRE(aligned16(d->stats), "dgll_hip_soft_agg_pass: stats must be 16-byte aligned");
    DGLL_REQUIRE(d->ld_stats % 4 == 0 && d->ld_stats >= 2 * d->F, "dgll_hip_soft_agg_pass: ld_stats is no pitch of whole 16-byte vectors >= 2 F");
    const bool has_e = d->e != nullptr;

    soft_agg::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.theta = d->theta;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.nnz = d->nnz;
    a.eps = d->eps;
    a.semi = d->mode == DGLL_SOFT_AGG_SOFTMAX && d->semi_grad != 0;
    a.st = d->stats;
    a.st_out = d->stats;
    a.ld_st = d->ld_stats;
    DGLL_REQUIRE_OPERAND(kPass, x, d->F);                   // every pass forms the message from x (and e)
    a.x = static_cast<const char*>(d->x);               a.pb_x = d->ld_x * esz;
    if (has_e) {
        DGLL_REQUIRE_OPERAND(kPass, e, d->F);
        a.e = static_cast<const char*>(d->e);           a.pb_e = d->ld_e * esz;
    }
    a.vpr = (int)(d->F / epv);
    rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t n_written = 0;                                  // rows: the partials its launch writes
    if (d->pass == DGLL_SOFT_AGG_FORWARD) {
        DGLL_REQUIRE_OPERAND(kPass, out, d->F);
        a.out = static_cast<char*>(d->out);             a.pb_out = d->ld_out * esz;
    } else if (d->pass == DGLL_SOFT_AGG_ROWS) {
        DGLL_REQUIRE(d->grad_e != nullptr || d->grad_theta != nullptr, "dgll_hip_soft_agg_pass: rows: nothing to write (grad_e and grad_theta are both NULL)");
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        if (d->grad_e != nullptr) {
            DGLL_REQUIRE(has_e, "dgll_hip_soft_agg_pass: rows: grad_e without e (e must be non-NULL for this pass)");
            DGLL_REQUIRE_OPERAND(kPass, grad_e, d->F);
            a.out = static_cast<char*>(d->grad_e);      a.pb_out = d->ld_grad_e * esz;
        }
        if (d->grad_theta != nullptr) {
            DGLL_REQUIRE(!a.semi, "dgll_hip_soft_agg_pass: rows: semi_grad has no scalar gradient (grad_theta must be NULL)");
            DGLL_REQUIRE(d->n_partials >= 1 && d->n_partials <= DGLL_SOFT_AGG_MAX_PARTIALS,
                         "dgll_hip_soft_agg_pass: rows: n_partials (the workgroups per column block at the most) must be in [1, DGLL_SOFT_AGG_MAX_PARTIALS = 1024]");
            DGLL_REQUIRE(d->partials != nullptr, "dgll_hip_soft_agg_pass: rows: partials [n_partials * column blocks] fp32 must be non-NULL");
            a.partials = d->partials;
            if (geo.grid > d->n_partials) geo.grid = d->n_partials;     // a bounded grid: the tiles are taken grid-stride
            n_written = geo.grid * geo.col_blocks;
        }
    } else {
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_x, d->F);
        DGLL_REQUIRE(!has_e || d->perm != nullptr, "dgll_hip_soft_agg_pass: cols: perm must be non-NULL when e is given");
        a.perm = d->perm;
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.out = static_cast<char*>(d->grad_x);          a.pb_out = d->ld_grad_x * esz;
    }
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    if (d->dtype == DGLL_F32) soft_agg::launch<float>(d->pass, d->mode, has_e, grid, st, a);
    else soft_agg::launch<bf16_t>(d->pass, d->mode, has_e, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    if (d->pass == DGLL_SOFT_AGG_ROWS && d->grad_theta != nullptr) {
        hipLaunchKernelGGL(soft_agg::soft_agg_sum_kernel, dim3(1), dim3(kBlock), 0, st, (const float*)d->partials, n_written, d->grad_theta);
        DGLL_HIP_TRY(hipGetLastError());
    }
    return DGLL_OK;
}
