// edge_proj.hip -- edge-feature aggregation with the edge projection FUSED in (PyG's GINEConv(edge_dim=)): the message combines the
// gathered source row with e_k = b + a_k W, formed per entry in registers from the raw edge attributes a [nnz, De] (De <= 16), so that
// no [nnz, F] array exists in any pass.  The passes of dgll_amd/ops_efp.py behind ONE entry point, dgll_hip_edge_proj_pass
// (include/dgll_hip.h: dgll_edge_proj_desc).  Entry k of row i of A is the edge j = col[k] -> i, a[k] its attribute row.
//
//   forward  rows of A     out[i] = s_i sum_k m(x[col_k], e_k): x gathered, a[k] read by every lane of the row (one address: a broadcast)
//   cols     rows of A^T   grad_x[j] = sum_k' s_i dm/dx g[i], i = colT[k']: x_j held (ADD_RELU), g[i] gathered, a at slot perm[k'] -- a
//                          scattered read of De values.  ADD_RELU and MUL only: ADD's grad_x reads neither x nor e (edge_feat.hip's cols)
//   param    rows of A     t_k = s_i dm/de g[i] (never stored); grad_W[d] = sum_k a[k, d] t_k, grad_b = sum_k t_k: every lane keeps its
//                          (DS + 1) x EPV sums over ALL the tiles of its workgroup (`partials` workgroups, tiles grid-stride), the lane
//                          groups are merged through LDS in group order and the workgroup writes one fp32 slab [De + 1, F]; the slabs
//                          are summed in slab order by the caller.  No float atomics.
//   dots     rows of A     grad_a[k, d] = sum over the columns of W[d, :] t_k: De dot products over the row's lanes per entry (a
//                          butterfly; every lane ends with the same bits).  Past one column block the per-block partial dots go to
//                          dots_part [col_blocks, nnz, De] fp32 and the caller sums them in block order.
//
// e is formed by ONE device function (form_e) in every pass: it starts from b, takes d ascending, one fmaf per term, so the forward's
// relu and both backward gates see the same bits.  A lane's slice W[:, its columns] and b are loaded once per kernel.  The kernels
// are templates over the storage type, op and the De bucket DB (4, 8, 16: W's slice is DB x EPV registers); the attribute columns
// past De are replaced by zeros after the load (and W's rows past De are zeros), so the bytes behind De in a's pitch reach nothing.
// Lane layout, tiles, index batches: row_tiles.hpp, as edge_feat.hip.  col and perm values used for addressing are clamped.
#include "row_tiles.hpp"

namespace dgll {
namespace efp {

constexpr int kLongRow = DGLL_EFP_LONG_ROW;     // rows longer than this are swept by a whole workgroup

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;                    // cols: A^T's entry -> A's entry (the slot of a)
    const float* scale;                     // per destination row, or NULL (1)
    int64_t n_rows, n_cols, nnz, tiles;
    const char* x;   int64_t pb_x;          // pitches in BYTES
    const char* a;   int64_t pb_a;
    const char* g;   int64_t pb_g;
    char* out;       int64_t pb_out;        // forward: out; cols: grad_x; dots: grad_a
    const float* w;                         // [De, F] fp32, contiguous
    const float* bias;                      // [F] fp32, or NULL (0)
    float* slabs;                           // param: [gridDim.x, De + 1, F] fp32
    float* part;                            // dots: [col_blocks, nnz, De] fp32, or NULL (grad_a written directly)
    int64_t F;
    int vpr, lpr, De;                       // 16-byte vectors of F columns; lanes of a row
};

template <int OP>
__device__ __forceinline__ float message(float x, float e) {
    if constexpr (OP == DGLL_EF_MUL) return x * e;
    const float s = x + e;
    if constexpr (OP == DGLL_EF_ADD_RELU) return s > 0.0f ? s : 0.0f;
    return s;
}

// t = dm/de * gi (gi = s_i g[i])
template <int OP>
__device__ __forceinline__ float edge_term(float x, float e, float gi) {
    if constexpr (OP == DGLL_EF_MUL) return x * gi;
    if constexpr (OP == DGLL_EF_ADD_RELU) return x + e > 0.0f ? gi : 0.0f;
    return gi;
}

// THE projection: e = b + sum_d a[d] W[d, :] for the lane's columns, d ascending, one fmaf per term
template <int DB, int EPV>
__device__ __forceinline__ void form_e(const float (&w)[DB][EPV], const float (&b)[EPV], const float (&av)[DB], float (&e)[EPV]) {
#pragma unroll
    for (int c = 0; c < EPV; ++c) e[c] = b[c];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int c = 0; c < EPV; ++c) e[c] = fmaf(av[d], w[d][c], e[c]);
}

// the lane's slice of W and b, once per kernel (rows past De and an idle lane: zeros)
template <int DB, int EPV>
__device__ __forceinline__ void load_weight(const Args& a, bool active, int v, bool want_bias, float (&w)[DB][EPV], float (&b)[EPV]) {
    using W4 = VecIO<float, 4>;
#pragma unroll
    for (int c = 0; c < EPV; ++c) b[c] = 0.0f;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
#pragma unroll
        for (int q = 0; q < EPV / 4; ++q) {
            typename W4::raw_t r = W4::zero();
            if (active && d < a.De) r = W4::load(a.w + (int64_t)d * a.F + (int64_t)v * EPV + q * 4);
            float f[4];
            W4::unpack(r, f);
#pragma unroll
            for (int c = 0; c < 4; ++c) w[d][q * 4 + c] = f[c];
        }
    }
    if (want_bias && active && a.bias) {
#pragma unroll
        for (int q = 0; q < EPV / 4; ++q) {
            float f[4];
            W4::unpack(W4::load(a.bias + (int64_t)v * EPV + q * 4), f);
#pragma unroll
            for (int c = 0; c < 4; ++c) b[q * 4 + c] = f[c];
        }
    }
}

// one attribute row: the 16-byte vectors that hold columns [0, De) (the pitch is whole vectors, so they are inside the row), then the
// columns past De replaced by zeros
template <typename T, int DB>
struct ARow {
    static constexpr int EPV = 16 / (int)sizeof(T), NV = (DB + EPV - 1) / EPV;
    using IO = VecIO<T, EPV>;
    typename IO::raw_t r[NV];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < NV; ++q) r[q] = IO::zero();
    }
    __device__ __forceinline__ void load(const char* p, int De) {
#pragma unroll
        for (int q = 0; q < NV; ++q)
            if (q * EPV < De) r[q] = IO::load(reinterpret_cast<const T*>(p + q * 16));
    }
    __device__ __forceinline__ void unpack(int De, float (&av)[DB]) const {
        float f[NV][EPV];
#pragma unroll
        for (int q = 0; q < NV; ++q) IO::unpack(r[q], f[q]);
#pragma unroll
        for (int d = 0; d < DB; ++d) av[d] = d < De ? f[d / EPV][d % EPV] : 0.0f;
    }
};

__device__ __forceinline__ void store_elem(float* p, float v) { *p = v; }
__device__ __forceinline__ void store_elem(bf16_t* p, float v) { *p = (bf16_t)(pack_bf16x2(v, 0.0f) & 0xffffu); }

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <typename T, int OP, int DB>
__global__ __launch_bounds__(kBlock) void efp_forward_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row of T

    float w[DB][EPV], b[EPV], acc[EPV];
    load_weight<DB, EPV>(a, active, v, true, w, b);

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rx[U];
            ARow<T, DB> ra[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = IO::zero();
                ra[u].clear();
                if (ok[u]) {
                    rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    ra[u].load(a.a + (k0 + t + u) * a.pb_a, a.De);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fx[EPV], av[DB], e[EPV];
                IO::unpack(rx[u], fx);
                ra[u].unpack(a.De, av);
                form_e<DB, EPV>(w, b, av, e);
#pragma unroll
                for (int d = 0; d < EPV; ++d) acc[d] += message<OP>(fx[d], e[d]);
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        const float s = a.scale ? a.scale[row] : 1.0f;
        float o[EPV];
#pragma unroll
        for (int d = 0; d < EPV; ++d) o[d] = s * acc[d];
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);       // a row without entries: zeros
    };

    auto load_row = [&](int64_t, int64_t, int64_t, bool) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = 0.0f;
    };
    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, load_row, batch, finish);
}

// ---- cols: rows of A^T (ADD_RELU, MUL) -------------------------------------------------------------------------------------------------
template <typename T, int OP, int DB>
__global__ __launch_bounds__(kBlock) void efp_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;

    float w[DB][EPV], b[EPV], acc[EPV], xj[EPV];
    load_weight<DB, EPV>(a, active, v, true, w, b);

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = xj[d] = 0.0f;
        if constexpr (OP == DGLL_EF_ADD_RELU) {
            typename IO::raw_t r = IO::zero();
            if (on && active) r = IO::load(reinterpret_cast<const T*>(a.x + row * a.pb_x + cb));
            IO::unpack(r, xj);
        }
    };

    // one batch of the row's entries, two in flight; the scale of the gathered row and the slot of a travel with the index
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        float my_s = 1.0f;
        if (a.scale && lanes.sub < nb) my_s = a.scale[my_col];
        int my_slot = 0;
        if (lanes.sub < nb) {
            const int64_t s = a.perm[k0 + lanes.sub];
            my_slot = (int)max((int64_t)0, min(s, a.nnz - 1));
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rg[U];
            ARow<T, DB> ra[U];
            float s[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = rt::hand_round(my_col, t + u, lanes);
                s[u] = rt::hand_round(my_s, t + u, lanes);
                const int slot = rt::hand_round(my_slot, t + u, lanes);
                ok[u] = t + u < nb && active;
                rg[u] = IO::zero();
                ra[u].clear();
                if (ok[u]) {
                    rg[u] = IO::load(reinterpret_cast<const T*>(a.g + (int64_t)i * a.pb_g + cb));
                    ra[u].load(a.a + (int64_t)slot * a.pb_a, a.De);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fg[EPV], av[DB], e[EPV];
                IO::unpack(rg[u], fg);
                ra[u].unpack(a.De, av);
                form_e<DB, EPV>(w, b, av, e);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    if constexpr (OP == DGLL_EF_MUL) acc[d] = fmaf(s[u] * e[d], fg[d], acc[d]);
                    else acc[d] += xj[d] + e[d] > 0.0f ? s[u] * fg[d] : 0.0f;
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

// ---- param: grad_W and grad_b as one slab per workgroup ------------------------------------------------------------------------------
// DS: the rows of grad_W a workgroup sums (DB, or DB / 2 with the two halves over blockIdx.z); the gate of ADD_RELU needs all of W in
// either case.  Block z = 0 also sums grad_b.
template <typename T, int OP, int DB, int DS>
__global__ __launch_bounds__(kBlock) void efp_param_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    constexpr bool kReadX = OP != DGLL_EF_ADD, kGate = OP == DGLL_EF_ADD_RELU;
    constexpr int WD = kGate ? DB : 1;                      // W is held for the gate alone
    static_assert(DS == DB || 2 * DS == DB, "one or two slices of d");
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const bool upper = DS < DB && blockIdx.z != 0;           // this workgroup sums rows [DS, DB)

    float w[WD][EPV], b[EPV], gi[EPV];                      // gi: s_i g[i]
    float sw[DS][EPV], sb[EPV];
    if constexpr (kGate) load_weight<DB, EPV>(a, active, v, true, w, b);
#pragma unroll
    for (int c = 0; c < EPV; ++c) {
        sb[c] = 0.0f;
#pragma unroll
        for (int d = 0; d < DS; ++d) sw[d][c] = 0.0f;
    }

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        typename IO::raw_t r = IO::zero();
        float s = 1.0f;
        if (on && active) {
            r = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
            if (a.scale) s = a.scale[row];
        }
        IO::unpack(r, gi);
#pragma unroll
        for (int d = 0; d < EPV; ++d) gi[d] *= s;
    };

    auto batch = [&](int64_t k0, int nb) {
        int my_col = 0;
        if constexpr (kReadX) my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rx[U];
            ARow<T, DB> ra[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int c = 0;
                if constexpr (kReadX) c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = IO::zero();
                ra[u].clear();
                if (ok[u]) {
                    if constexpr (kReadX) rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    ra[u].load(a.a + (k0 + t + u) * a.pb_a, a.De);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fx[EPV], av[DB], e[EPV], as[DS];
                IO::unpack(rx[u], fx);
                ra[u].unpack(a.De, av);
                if constexpr (kGate) form_e<DB, EPV>(w, b, av, e);
#pragma unroll
                for (int d = 0; d < DS; ++d) {
                    as[d] = av[d];
                    if constexpr (DS < DB) as[d] = upper ? av[DS + d] : av[d];
                }
#pragma unroll
                for (int c = 0; c < EPV; ++c) {
                    const float tk = edge_term<OP>(fx[c], kGate ? e[c] : 0.0f, gi[c]);
                    sb[c] += tk;
#pragma unroll
                    for (int d = 0; d < DS; ++d) sw[d][c] = fmaf(as[d], tk, sw[d][c]);
                }
            }
        }
    };

    // every lane group keeps its sums over the rows and the shares of long rows it took; nothing is done at the end of a row
    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, load_row, batch);

    // the workgroup's slab: row by row, the lane groups merged in group order
    float* slab = a.slabs + (int64_t)blockIdx.x * (a.De + 1) * a.F;
    const int d0 = upper ? DS : 0;
    auto put = [&](int row, const float (&st)[EPV]) {
        if (!active) return;
        float* p = slab + (int64_t)row * a.F + (int64_t)v * EPV;
#pragma unroll
        for (int q = 0; q < EPV / 4; ++q) {
            const float f[4] = {st[q * 4], st[q * 4 + 1], st[q * 4 + 2], st[q * 4 + 3]};
            VecIO<float, 4>::store(p + q * 4, f);
        }
    };
#pragma unroll
    for (int d = 0; d < DS; ++d) rt::merge_partials<false>(sw[d], lds, lanes, [&] { if (d0 + d < a.De) put(d0 + d, sw[d]); });
    rt::merge_partials<false>(sb, lds, lanes, [&] { if (!upper) put(a.De, sb); });
}

// ---- dots: grad_a, De dot products over the row's lanes per entry ---------------------------------------------------------------------
template <typename T, int OP, int DB>
__global__ __launch_bounds__(kBlock) void efp_dots_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    constexpr bool kReadX = OP != DGLL_EF_ADD, kGate = OP == DGLL_EF_ADD_RELU;
    using IO = VecIO<T, EPV>;

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;

    float w[DB][EPV], b[EPV], gi[EPV];
    load_weight<DB, EPV>(a, active, v, kGate, w, b);

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        typename IO::raw_t r = IO::zero();
        float s = 1.0f;
        if (on && active) {
            r = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
            if (a.scale) s = a.scale[row];
        }
        IO::unpack(r, gi);
#pragma unroll
        for (int d = 0; d < EPV; ++d) gi[d] *= s;
    };

    auto batch = [&](int64_t k0, int nb) {
        int my_col = 0;
        if constexpr (kReadX) my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rx[U];
            ARow<T, DB> ra[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int c = 0;
                if constexpr (kReadX) c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = IO::zero();
                ra[u].clear();
                if (ok[u]) {
                    if constexpr (kReadX) rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    if constexpr (kGate) ra[u].load(a.a + (k0 + t + u) * a.pb_a, a.De);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {               // every lane of the wavefront takes part in the butterfly
                float fx[EPV], e[EPV], tk[EPV], p[DB];
                IO::unpack(rx[u], fx);
                if constexpr (kGate) {
                    float av[DB];
                    ra[u].unpack(a.De, av);
                    form_e<DB, EPV>(w, b, av, e);
                }
#pragma unroll
                for (int c = 0; c < EPV; ++c) tk[c] = ok[u] ? edge_term<OP>(fx[c], kGate ? e[c] : 0.0f, gi[c]) : 0.0f;
#pragma unroll
                for (int d = 0; d < DB; ++d) {
                    p[d] = 0.0f;
#pragma unroll
                    for (int c = 0; c < EPV; ++c) p[d] = fmaf(w[d][c], tk[c], p[d]);
                    for (int off = 1; off < lanes.lpr; off <<= 1) p[d] += __shfl_xor(p[d], off);
                }
                if (t + u >= nb) continue;
                const int64_t k = k0 + t + u;
#pragma unroll
                for (int d = 0; d < DB; ++d) {          // lane d of the group (modulo its size) stores column d
                    if (d >= a.De || (d & (lanes.lpr - 1)) != lanes.sub) continue;
                    if (a.part) a.part[((int64_t)blockIdx.y * a.nnz + k) * a.De + d] = p[d];
                    else store_elem(reinterpret_cast<T*>(a.out + k * a.pb_out) + d, p[d]);
                }
            }
        }
    };

    // (a long row: every lane group holds g[i] and takes its share of the entries)
    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, load_row, batch);
}

template <typename T, int OP, int DB>
void launch_bucket(int pass, dim3 grid, hipStream_t s, const Args& a) {
    constexpr int DS = sizeof(T) == 2 && DB == 16 ? 8 : DB;     // bf16 at De > 8: the sums in two halves over blockIdx.z
    if (pass == DGLL_EFP_FORWARD) hipLaunchKernelGGL((efp_forward_kernel<T, OP, DB>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_EFP_PARAM) {
        grid.z = DB / DS;
        hipLaunchKernelGGL((efp_param_kernel<T, OP, DB, DS>), grid, dim3(kBlock), 0, s, a);
    } else if (pass == DGLL_EFP_DOTS) hipLaunchKernelGGL((efp_dots_kernel<T, OP, DB>), grid, dim3(kBlock), 0, s, a);
    else if constexpr (OP != DGLL_EF_ADD) hipLaunchKernelGGL((efp_cols_kernel<T, OP, DB>), grid, dim3(kBlock), 0, s, a);
}

template <typename T, int OP>
void launch_op(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (a.De <= 4) launch_bucket<T, OP, 4>(pass, grid, s, a);
    else if (a.De <= 8) launch_bucket<T, OP, 8>(pass, grid, s, a);
    else launch_bucket<T, OP, 16>(pass, grid, s, a);
}

template <typename T>
void launch(int pass, int op, dim3 grid, hipStream_t s, const Args& a) {
    if (op == DGLL_EF_ADD) launch_op<T, DGLL_EF_ADD>(pass, grid, s, a);
    else if (op == DGLL_EF_ADD_RELU) launch_op<T, DGLL_EF_ADD_RELU>(pass, grid, s, a);
    else launch_op<T, DGLL_EF_MUL>(pass, grid, s, a);
}

}  // namespace efp
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_edge_proj_pass(void* stream, const dgll_edge_proj_desc* d) {
    static const char* const kPass = "dgll_hip_edge_proj_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_edge_proj_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_EFP_FORWARD || d->pass == DGLL_EFP_COLS || d->pass == DGLL_EFP_PARAM || d->pass == DGLL_EFP_DOTS,
                 "dgll_hip_edge_proj_pass: pass must be DGLL_EFP_FORWARD, DGLL_EFP_COLS, DGLL_EFP_PARAM or DGLL_EFP_DOTS");
    DGLL_REQUIRE(d->op == DGLL_EF_ADD || d->op == DGLL_EF_ADD_RELU || d->op == DGLL_EF_MUL,
                 "dgll_hip_edge_proj_pass: op must be DGLL_EF_ADD, DGLL_EF_ADD_RELU or DGLL_EF_MUL");
    DGLL_REQUIRE(d->pass != DGLL_EFP_COLS || d->op != DGLL_EF_ADD,
                 "dgll_hip_edge_proj_pass: cols: op DGLL_EF_ADD reads neither x nor e: it is dgll_hip_edge_feat_pass's DGLL_EF_COLS");
    DGLL_REQUIRE(d->De >= 1 && d->De <= DGLL_EFP_MAX_DE, "dgll_hip_edge_proj_pass: De (the edge attribute width) must be in [1, DGLL_EFP_MAX_DE = 16]");
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, d->nnz, d->rowptr, d->col, true)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    const bool relu = d->op == DGLL_EF_ADD_RELU, mul = d->op == DGLL_EF_MUL;

    efp::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.scale = d->scale;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.nnz = d->nnz;
    a.F = d->F;
    a.De = d->De;
    a.vpr = (int)(d->F / epv);
    rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    bool read_x, read_a = true, read_w = true;
    if (d->pass == DGLL_EFP_FORWARD) {
        read_x = true;
        DGLL_REQUIRE_OPERAND(kPass, out, d->F);
        a.out = static_cast<char*>(d->out);             a.pb_out = d->ld_out * esz;
    } else if (d->pass == DGLL_EFP_COLS) {
        read_x = relu;
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_x, d->F);
        DGLL_REQUIRE(d->perm != nullptr, "dgll_hip_edge_proj_pass: cols: perm must be non-NULL (a is read at slot perm[k'])");
        a.perm = d->perm;
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.out = static_cast<char*>(d->grad_x);          a.pb_out = d->ld_grad_x * esz;
    } else if (d->pass == DGLL_EFP_PARAM) {
        read_x = relu || mul;
        read_w = relu;
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE(d->partials >= 1 && d->partials <= DGLL_EFP_MAX_PARTIALS,
                     "dgll_hip_edge_proj_pass: param: partials (the workgroups, and slabs) must be in [1, DGLL_EFP_MAX_PARTIALS = 512]");
        DGLL_REQUIRE(d->slabs != nullptr && aligned16(d->slabs), "dgll_hip_edge_proj_pass: param: slabs [partials, De + 1, F] fp32 must be non-NULL and 16-byte aligned");
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.slabs = d->slabs;
        geo.grid = d->partials;
    } else {
        read_x = relu || mul;
        read_a = relu;
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE(geo.col_blocks == 1 || d->dots_part != nullptr,
                     "dgll_hip_edge_proj_pass: dots: dots_part [col_blocks, nnz, De] fp32 must be non-NULL past one column block (64 lane vectors)");
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        if (geo.col_blocks > 1) a.part = d->dots_part;
        else {
            DGLL_REQUIRE_OPERAND(kPass, grad_a, d->De);
            a.out = static_cast<char*>(d->grad_a);      a.pb_out = d->ld_grad_a * esz;
        }
    }
    if (read_x) {
        DGLL_REQUIRE_OPERAND(kPass, x, d->F);
        a.x = static_cast<const char*>(d->x);           a.pb_x = d->ld_x * esz;
    }
    if (read_a) {
        DGLL_REQUIRE_OPERAND(kPass, a, d->De);
        a.a = static_cast<const char*>(d->a);           a.pb_a = d->ld_a * esz;
    }
    if (read_w) {
        DGLL_REQUIRE(d->weight != nullptr && aligned16(d->weight), "dgll_hip_edge_proj_pass: weight [De, F] fp32 must be non-NULL and 16-byte aligned");
        DGLL_REQUIRE(d->bias == nullptr || aligned16(d->bias), "dgll_hip_edge_proj_pass: bias [F] fp32 must be NULL or 16-byte aligned");
        a.w = d->weight;
        a.bias = d->bias;
    }
    rt::set_geometry(a, geo);
    if (geo.grid == 0 || d->n_rows == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) efp::launch<float>(d->pass, d->op, grid, st, a);
    else efp::launch<bf16_t>(d->pass, d->op, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
