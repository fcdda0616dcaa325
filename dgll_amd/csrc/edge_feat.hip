// edge_feat.hip -- edge-feature aggregation (DGL's GINEConv, CFConv): a gather-reduce whose message combines the gathered source row
// with a per-edge row of the same width, and its exact backward.  The three passes of dgll_amd/ops_ef.py behind ONE entry point,
// dgll_hip_edge_feat_pass (include/dgll_hip.h: dgll_edge_feat_desc).  Entry k of row i of A is the edge j = col[k] -> i, e[k] its row.
//
//   forward  rows of A     out[i] = s_i sum_k m(x[col_k], e[k]): x gathered, e streamed at slot k
//   cols     rows of A^T   grad_x[j] = sum_k' s_i dm/dx g[i], i = colT[k']: x_j held (ADD_RELU only), g[i] gathered, s by the gathered
//                          row, e at slot perm[k'] -- a scattered read per entry (ADD reads neither x nor e)
//   edge     rows of A     grad_e[k] = s_i dm/de g[i]: g[i] held with s_i folded in, x[col_k] gathered (ADD_RELU, MUL), e[k] read
//                          (ADD_RELU); one store per entry and no reduction, so a long row only shares its entries among the groups
//
//   op         m              dm/dx   dm/de
//   ADD        x + e          1       1
//   ADD_RELU   relu(x + e)    gate    gate       gate = (x + e > 0)
//   MUL        x * e          e       x
//
// The gate is never stored: every pass forms the same fp32 sum of the same two stored values (an add alone: nothing to contract), so
// the forward's relu and the backward's gates agree bit for bit.  Each pass is a template over the storage type and over op: the
// operands an op does not read are not loaded, and may be NULL.
//
// Lane layout, tiles, index batches: row_tiles.hpp.  A row's `lpr` lanes are at least its F / EPV vectors; rows wider than 64 lanes are
// cut into column blocks of 64 vectors over blockIdx.y.  Two entries in flight per lane (two or four 16-byte loads).  The long-row
// merge of forward and cols is rt::merge_partials, in group order.  No atomics.  col and perm values used for addressing are clamped.
#include "row_tiles.hpp"

namespace dgll {
namespace ef {

constexpr int kLongRow = DGLL_EF_LONG_ROW;      // rows longer than this are swept by a whole workgroup

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;                    // cols: A^T's entry -> A's entry (the slot of e)
    const float* scale;                     // per destination row, or NULL (1)
    int64_t n_rows, n_cols, nnz, tiles;
    const char* x;   int64_t pb_x;          // pitches in BYTES
    const char* e;   int64_t pb_e;
    const char* g;   int64_t pb_g;
    char* out;       int64_t pb_out;        // forward: out; cols: grad_x; edge: grad_e
    int vpr, lpr;                           // 16-byte vectors of F columns; lanes of a row
};

template <int OP>
__device__ __forceinline__ float message(float x, float e) {
    if constexpr (OP == DGLL_EF_MUL) return x * e;
    const float s = x + e;
    if constexpr (OP == DGLL_EF_ADD_RELU) return s > 0.0f ? s : 0.0f;
    return s;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void ef_forward_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row of T

    float acc[EPV];

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
                    re[u] = IO::load(reinterpret_cast<const T*>(a.e + (k0 + t + u) * a.pb_e + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fx[EPV], fe[EPV];
                IO::unpack(rx[u], fx);
                IO::unpack(re[u], fe);
#pragma unroll
                for (int d = 0; d < EPV; ++d) acc[d] += message<OP>(fx[d], fe[d]);
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

// ---- cols: rows of A^T ---------------------------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void ef_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    constexpr bool kReadE = OP != DGLL_EF_ADD;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;

    float acc[EPV], xj[EPV];

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = xj[d] = 0.0f;
        if constexpr (OP == DGLL_EF_ADD_RELU) {
            typename IO::raw_t r = IO::zero();
            if (on && active) r = IO::load(reinterpret_cast<const T*>(a.x + row * a.pb_x + cb));
            IO::unpack(r, xj);
        }
    };

    // one batch of the row's entries, two in flight; the scale of the gathered row and the slot of e travel with the index
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        float my_s = 1.0f;
        if (a.scale && lanes.sub < nb) my_s = a.scale[my_col];
        int my_slot = 0;
        if constexpr (kReadE) {
            if (lanes.sub < nb) {
                const int64_t s = a.perm[k0 + lanes.sub];
                my_slot = (int)max((int64_t)0, min(s, a.nnz - 1));
            }
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rg[U], re[U];
            float s[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = rt::hand_round(my_col, t + u, lanes);
                s[u] = rt::hand_round(my_s, t + u, lanes);
                int slot = 0;
                if constexpr (kReadE) slot = rt::hand_round(my_slot, t + u, lanes);
                ok[u] = t + u < nb && active;
                rg[u] = re[u] = IO::zero();
                if (ok[u]) {
                    rg[u] = IO::load(reinterpret_cast<const T*>(a.g + (int64_t)i * a.pb_g + cb));
                    if constexpr (kReadE) re[u] = IO::load(reinterpret_cast<const T*>(a.e + (int64_t)slot * a.pb_e + cb));
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
                    if constexpr (OP == DGLL_EF_MUL) acc[d] = fmaf(s[u] * fe[d], fg[d], acc[d]);
                    else if constexpr (OP == DGLL_EF_ADD_RELU) acc[d] += xj[d] + fe[d] > 0.0f ? s[u] * fg[d] : 0.0f;
                    else acc[d] = fmaf(s[u], fg[d], acc[d]);
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

// ---- edge: one row of grad_e per entry, no reduction ------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void ef_edge_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    constexpr bool kReadX = OP != DGLL_EF_ADD, kReadE = OP == DGLL_EF_ADD_RELU;
    using IO = VecIO<T, EPV>;

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;

    float gi[EPV];                                          // s_i g[i]

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
            typename IO::raw_t rx[U], re[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int c = 0;
                if constexpr (kReadX) c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rx[u] = re[u] = IO::zero();
                if (ok[u]) {
                    if constexpr (kReadX) rx[u] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
                    if constexpr (kReadE) re[u] = IO::load(reinterpret_cast<const T*>(a.e + (k0 + t + u) * a.pb_e + cb));
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
                    if constexpr (OP == DGLL_EF_MUL) o[d] = fx[d] * gi[d];
                    else if constexpr (OP == DGLL_EF_ADD_RELU) o[d] = fx[d] + fe[d] > 0.0f ? gi[d] : 0.0f;
                    else o[d] = gi[d];
                }
                IO::store(reinterpret_cast<T*>(a.out + (k0 + t + u) * a.pb_out + cb), o);
            }
        }
    };

    // (a long row: every lane group holds g[i] and takes its share of the entries)
    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, load_row, batch);
}

template <typename T, int OP>
void launch_op(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_EF_FORWARD) hipLaunchKernelGGL((ef_forward_kernel<T, OP>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_EF_COLS) hipLaunchKernelGGL((ef_cols_kernel<T, OP>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((ef_edge_kernel<T, OP>), grid, dim3(kBlock), 0, s, a);
}

template <typename T>
void launch(int pass, int op, dim3 grid, hipStream_t s, const Args& a) {
    if (op == DGLL_EF_ADD) launch_op<T, DGLL_EF_ADD>(pass, grid, s, a);
    else if (op == DGLL_EF_ADD_RELU) launch_op<T, DGLL_EF_ADD_RELU>(pass, grid, s, a);
    else launch_op<T, DGLL_EF_MUL>(pass, grid, s, a);
}

}  // namespace ef
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_edge_feat_pass(void* stream, const dgll_edge_feat_desc* d) {
    static const char* const kPass = "dgll_hip_edge_feat_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_edge_feat_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_EF_FORWARD || d->pass == DGLL_EF_COLS || d->pass == DGLL_EF_EDGE,
                 "dgll_hip_edge_feat_pass: pass must be DGLL_EF_FORWARD, DGLL_EF_COLS or DGLL_EF_EDGE");
    DGLL_REQUIRE(d->op == DGLL_EF_ADD || d->op == DGLL_EF_ADD_RELU || d->op == DGLL_EF_MUL,
                 "dgll_hip_edge_feat_pass: op must be DGLL_EF_ADD, DGLL_EF_ADD_RELU or DGLL_EF_MUL");
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, d->nnz, d->rowptr, d->col, true)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    const bool relu = d->op == DGLL_EF_ADD_RELU, mul = d->op == DGLL_EF_MUL;

    ef::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.scale = d->scale;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.nnz = d->nnz;
    bool read_x, read_e;
    if (d->pass == DGLL_EF_FORWARD) {
        read_x = read_e = true;
        DGLL_REQUIRE_OPERAND(kPass, out, d->F);
        a.out = static_cast<char*>(d->out);             a.pb_out = d->ld_out * esz;
    } else if (d->pass == DGLL_EF_COLS) {
        read_x = relu;
        read_e = relu || mul;
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_x, d->F);
        DGLL_REQUIRE(!read_e || d->perm != nullptr, "dgll_hip_edge_feat_pass: cols: perm must be non-NULL when e is read (ADD_RELU, MUL)");
        a.perm = d->perm;
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.out = static_cast<char*>(d->grad_x);          a.pb_out = d->ld_grad_x * esz;
    } else {
        read_x = relu || mul;
        read_e = relu;
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_e, d->F);
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.out = static_cast<char*>(d->grad_e);          a.pb_out = d->ld_grad_e * esz;
    }
    if (read_x) {
        DGLL_REQUIRE_OPERAND(kPass, x, d->F);
        a.x = static_cast<const char*>(d->x);           a.pb_x = d->ld_x * esz;
    }
    if (read_e) {
        DGLL_REQUIRE_OPERAND(kPass, e, d->F);
        a.e = static_cast<const char*>(d->e);           a.pb_e = d->ld_e * esz;
    }
    a.vpr = (int)(d->F / epv);
    const rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) ef::launch<float>(d->pass, d->op, grid, st, a);
    else ef::launch<bf16_t>(d->pass, d->op, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
