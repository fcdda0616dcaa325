// res_gated.hip -- gated aggregation with nothing stored per edge (Bresson & Laurent's residual gated graph convnet in the form of PyG's
// ResGatedGraphConv: no edge features), and its exact backward.  The three passes of dgll_amd/ops_res_gated.py behind ONE entry point,
// dgll_hip_res_gated_pass (include/dgll_hip.h: dgll_res_gated_desc).  Entry e of row i of A is the edge j = col[e] -> i.  For every
// column, with k [n_dst, F], q and v [n_src, F] and g = grad_out:
//
//   s = sigmoid(k_i + q_j)        out_i = sum_e s v_j        (`mean`: divided by the row's entry count)
//
//   forward  rows of A     k_i held, q_j and v_j gathered; one store of out_i at the row's end
//   rows     rows of A     grad_k_i = g_i * sum_e s (1 - s) v_j: k_i and g_i held, q_j and v_j gathered
//   cols     rows of A^T   S1_j = sum_e' g_i s (1 - s), S2_j = sum_e' g_i s: q_j held, k_i and g_i gathered (i = colT[e']);
//                          grad_q_j = v_j S1_j (v_j loaded at the row's end), grad_v_j = S2_j; either output may be left out, and what
//                          only it needs is then neither loaded nor summed
//
// The gate is never stored: every pass computes the same fp32 function of the same STORED k and q (the sum k_i + q_j is one fp32
// addition, whichever operand is held), so forward and backward see one gate, and no [nnz, F] array exists in either.  cols is an
// ordinary gather over the transposed structure: it needs no permutation.
// sigmoid(x) = 1 / (1 + exp2(-x log2 e)): exp2 overflows to +inf and the reciprocal of +inf is 0, exp2 underflows to 0 and the
// reciprocal of 1 is 1 -- a saturated gate is exactly 0 or 1, never NaN, and s (1 - s) is then exactly 0.
//
// Lane layout, tiles, index batches: row_tiles.hpp, as gated.hip.  A row's `lpr` lanes are at least its F / EPV vectors; rows wider
// than 64 lanes are cut into column blocks of 64 vectors over blockIdx.y.  Two entries in flight per lane (four 16-byte loads).
// The long-row merge is rt::merge_partials, in group order.  No atomics.  col values used for addressing are clamped.
#include "row_tiles.hpp"

namespace dgll {
namespace res_gated {

constexpr int kLongRow = DGLL_RES_GATED_LONG_ROW;   // rows longer than this are swept by a whole workgroup

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    int64_t n_rows, n_cols, tiles;
    int mean;                               // forward: the row is divided by its entry count
    const char* k;    int64_t pb_k;         // pitches in BYTES
    const char* q;    int64_t pb_q;
    const char* v;    int64_t pb_v;
    const char* g;    int64_t pb_g;
    char* out;        int64_t pb_out;
    char* gk;         int64_t pb_gk;
    char* gq;         int64_t pb_gq;
    char* gv;         int64_t pb_gv;
    int vpr, lpr;                           // 16-byte vectors of F columns; lanes of a row
};

__device__ __forceinline__ float sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-rt::kLog2e * x));
}

// ---- forward (ROWS == false): out_i = sum s v_j;  rows (ROWS == true): grad_k_i = g_i sum s (1 - s) v_j -------------------------------
// One kernel text for the two sweeps over A: they gather the same two rows per entry and differ in the weight of v_j and in the end.
template <typename T, bool ROWS>
__global__ __launch_bounds__(kBlock) void res_gated_rows_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row

    float acc[EPV], ki[EPV], gi[EPV];

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = 0.0f;
        typename IO::raw_t rk = IO::zero(), rg = IO::zero();
        if (on && active) {
            rk = IO::load(reinterpret_cast<const T*>(a.k + row * a.pb_k + cb));
            if constexpr (ROWS) rg = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
        }
        IO::unpack(rk, ki);
        IO::unpack(rg, gi);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rq[U], rv[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rq[u] = rv[u] = IO::zero();
                if (ok[u]) {
                    rq[u] = IO::load(reinterpret_cast<const T*>(a.q + (int64_t)c * a.pb_q + cb));
                    rv[u] = IO::load(reinterpret_cast<const T*>(a.v + (int64_t)c * a.pb_v + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fq[EPV], fv[EPV];
                IO::unpack(rq[u], fq);
                IO::unpack(rv[u], fv);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float s = sigmoid(ki[d] + fq[d]);
                    acc[d] = fmaf(ROWS ? s * (1.0f - s) : s, fv[d], acc[d]);
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t b, int64_t e) {
        if (!active) return;
        float o[EPV];                                       // a row without entries: zeros
        if constexpr (ROWS) {
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = gi[d] * acc[d];
            IO::store(reinterpret_cast<T*>(a.gk + row * a.pb_gk + cb), o);
        } else {
            const float scale = a.mean && e > b ? 1.0f / (float)(e - b) : 1.0f;
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = acc[d] * scale;
            IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);
        }
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, load_row, batch, finish);
}

// ---- cols: rows of A^T, two outputs; a.k is gathered (n_cols = n_dst rows), a.q and a.v are the pass's own rows ------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void res_gated_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[2 * EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const bool need_q = a.gq != nullptr, need_v = a.gv != nullptr;     // uniform: kernel arguments

    float st[2 * EPV], qj[EPV];                             // [0, EPV) S1 (grad_q), [EPV, 2 EPV) S2 (grad_v)

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < 2 * EPV; ++d) st[d] = 0.0f;
        typename IO::raw_t r = IO::zero();
        if (on && active) r = IO::load(reinterpret_cast<const T*>(a.q + row * a.pb_q + cb));
        IO::unpack(r, qj);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rk[U], rg[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rk[u] = rg[u] = IO::zero();
                if (ok[u]) {
                    rk[u] = IO::load(reinterpret_cast<const T*>(a.k + (int64_t)i * a.pb_k + cb));
                    rg[u] = IO::load(reinterpret_cast<const T*>(a.g + (int64_t)i * a.pb_g + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fk[EPV], fg[EPV];
                IO::unpack(rk[u], fk);
                IO::unpack(rg[u], fg);
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float s = sigmoid(fk[d] + qj[d]);
                    if (need_q) st[d] = fmaf(fg[d], s * (1.0f - s), st[d]);
                    if (need_v) st[EPV + d] = fmaf(fg[d], s, st[EPV + d]);
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        float o[EPV];                                       // a source no row references: zeros
        if (need_q) {
            float fv[EPV];
            IO::unpack(IO::load(reinterpret_cast<const T*>(a.v + row * a.pb_v + cb)), fv);
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = fv[d] * st[d];
            IO::store(reinterpret_cast<T*>(a.gq + row * a.pb_gq + cb), o);
        }
        if (need_v) {
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = st[EPV + d];
            IO::store(reinterpret_cast<T*>(a.gv + row * a.pb_gv + cb), o);
        }
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, st, lds, load_row, batch, finish);
}

template <typename T>
void launch(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_RES_GATED_FORWARD) hipLaunchKernelGGL((res_gated_rows_kernel<T, false>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_RES_GATED_ROWS) hipLaunchKernelGGL((res_gated_rows_kernel<T, true>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((res_gated_cols_kernel<T>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace res_gated
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_res_gated_pass(void* stream, const dgll_res_gated_desc* d) {
    static const char* const kPass = "dgll_hip_res_gated_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_res_gated_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_RES_GATED_FORWARD || d->pass == DGLL_RES_GATED_ROWS || d->pass == DGLL_RES_GATED_COLS,
                 "dgll_hip_res_gated_pass: pass must be DGLL_RES_GATED_FORWARD, DGLL_RES_GATED_ROWS or DGLL_RES_GATED_COLS");
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, 0, d->rowptr, d->col, true)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);

    res_gated::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.mean = d->mean != 0;
    DGLL_REQUIRE_OPERAND(kPass, k, d->F);                   // every pass forms the gate from k and q
    DGLL_REQUIRE_OPERAND(kPass, q, d->F);
    a.k = static_cast<const char*>(d->k);               a.pb_k = d->ld_k * esz;
    a.q = static_cast<const char*>(d->q);               a.pb_q = d->ld_q * esz;
    if (d->pass == DGLL_RES_GATED_FORWARD) {
        DGLL_REQUIRE_OPERAND(kPass, v, d->F);
        DGLL_REQUIRE_OPERAND(kPass, out, d->F);
        a.v = static_cast<const char*>(d->v);           a.pb_v = d->ld_v * esz;
        a.out = static_cast<char*>(d->out);             a.pb_out = d->ld_out * esz;
    } else if (d->pass == DGLL_RES_GATED_ROWS) {
        DGLL_REQUIRE_OPERAND(kPass, v, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, grad_k, d->F);
        a.v = static_cast<const char*>(d->v);           a.pb_v = d->ld_v * esz;
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.gk = static_cast<char*>(d->grad_k);           a.pb_gk = d->ld_grad_k * esz;
    } else {
        DGLL_REQUIRE(d->grad_q != nullptr || d->grad_v != nullptr, "dgll_hip_res_gated_pass: cols: nothing to write (grad_q and grad_v are both NULL)");
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        if (d->grad_q != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, v, d->F);
            DGLL_REQUIRE_OPERAND(kPass, grad_q, d->F);
            a.v = static_cast<const char*>(d->v);       a.pb_v = d->ld_v * esz;
            a.gq = static_cast<char*>(d->grad_q);       a.pb_gq = d->ld_grad_q * esz;
        }
        if (d->grad_v != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, grad_v, d->F);
            a.gv = static_cast<char*>(d->grad_v);       a.pb_gv = d->ld_grad_v * esz;
        }
    }
    a.vpr = (int)(d->F / epv);
    const rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) res_gated::launch<float>(d->pass, grid, st, a);
    else res_gated::launch<bf16_t>(d->pass, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
