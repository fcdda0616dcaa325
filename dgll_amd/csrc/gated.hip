// gated.hip -- edge-gated aggregation with edge outputs (Bresson & Laurent's residual gated graph convnet, DGL's GatedGCNConv): a
// gather-reduce whose per-column gate is the sigmoid of an edge row that the pass itself forms and returns, and its exact backward.
// The three passes of dgll_amd/ops_gated.py behind ONE entry point, dgll_hip_gated_pass (include/dgll_hip.h: dgll_gated_desc).
// Entry k of row i of A is the edge j = col[k] -> i.  For every column:
//
//   ehat[k] = c[k] + a[i] + b[j]      sig[k] = sigmoid(ehat[k])      S_i = sum_k sig[k] + eps      out[i] = (sum_k sig[k] v[j]) / S_i
//
//   forward  rows of A     a_i held, b_j and v_j gathered, c[k] streamed; stores ehat[k] (rounded to the storage type) and, at the row's
//                          end, out_i and the fp32 row state 1 / S_i and the unrounded out_i
//   rows     rows of A     t[k] = ge[k] + g_i (v_j - out_i) / S_i sig[k] (1 - sig[k]): g_i, out_i, 1 / S_i held, v_j gathered, ehat[k] and
//                          ge[k] (optional) read; stores t[k] (grad_c), sums it into grad_a[i], leaves w_i = g_i / S_i for cols
//   cols     rows of A^T   grad_b[j] = sum_k' t[perm k'], grad_v[j] = sum_k' sig[perm k'] w_i, i = colT[k']: t and ehat at slot perm[k'] --
//                          scattered reads -- and w_i gathered; two outputs, either may be left out
//
// The gate is never stored: every pass computes the same fp32 function of the same STORED ehat, so forward and backward see one gate.
// sigmoid(x) = 1 / (1 + exp2(-x log2 e)): exp2 overflows to +inf and the reciprocal of +inf is 0, exp2 underflows to 0 and the
// reciprocal of 1 is 1 -- a saturated gate is exactly 0 or 1, never NaN.
//
// Lane layout, tiles, index batches: row_tiles.hpp, as edge_feat.hip.  A row's `lpr` lanes are at least its F / EPV vectors; rows wider
// than 64 lanes are cut into column blocks of 64 vectors over blockIdx.y.  Two entries in flight per lane (four to six 16-byte loads).
// The long-row merge is rt::merge_partials, in group order.  No atomics.  col and perm values used for addressing are clamped.
#include "row_tiles.hpp"

namespace dgll {
namespace gated {

constexpr int kLongRow = DGLL_GATED_LONG_ROW;   // rows longer than this are swept by a whole workgroup

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;                    // cols: A^T's entry -> A's entry (the slot of t and ehat)
    int64_t n_rows, n_cols, nnz, tiles;
    float eps;
    const char* a;    int64_t pb_a;         // pitches in BYTES
    const char* b;    int64_t pb_b;
    const char* c;    int64_t pb_c;
    const char* v;    int64_t pb_v;
    const char* g;    int64_t pb_g;
    const char* ge;   int64_t pb_ge;        // rows: the gradient through ehat, or NULL (zeros)
    char* out;        int64_t pb_out;
    char* ehat;       int64_t pb_ehat;      // forward writes it, rows and cols read it
    char* inv;        int64_t pb_inv;       // fp32 row state: 1 / S_i ...
    char* o32;        int64_t pb_o32;       // ... and the unrounded out_i
    char* t;          int64_t pb_t;         // rows writes it (grad_c), cols reads it
    char* ga;         int64_t pb_ga;
    char* w;          int64_t pb_w;         // rows writes w_i = g_i / S_i, cols gathers it
    char* gb;         int64_t pb_gb;
    char* gv;         int64_t pb_gv;
    int vpr, lpr;                           // 16-byte vectors of F columns; lanes of a row
};

__device__ __forceinline__ float sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-rt::kLog2e * x));
}

// f as the storage type keeps it: what a later pass reads back
template <typename T, int EPV>
__device__ __forceinline__ void round_to_storage(float (&f)[EPV]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int d = 0; d < EPV; d += 2) {
            const uint32_t p = pack_bf16x2(f[d], f[d + 1]);
            f[d] = bf16_lo(p);
            f[d + 1] = bf16_hi(p);
        }
    }
}

// EPV fp32 values of the row state (one or two 16-byte vectors)
template <int EPV>
__device__ __forceinline__ void load_state(const char* p, float (&f)[EPV]) {
    using S = VecIO<float, 4>;
#pragma unroll
    for (int q = 0; q < EPV / 4; ++q) {
        float part[4];
        S::unpack(S::load(reinterpret_cast<const float*>(p) + 4 * q), part);
#pragma unroll
        for (int d = 0; d < 4; ++d) f[4 * q + d] = part[d];
    }
}
template <int EPV>
__device__ __forceinline__ void store_state(char* p, const float (&f)[EPV]) {
    using S = VecIO<float, 4>;
#pragma unroll
    for (int q = 0; q < EPV / 4; ++q) {
        float part[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) part[d] = f[4 * q + d];
        S::store(reinterpret_cast<float*>(p) + 4 * q, part);
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void gated_forward_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[2 * EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset in a row of T ...
    const int64_t sb = cb * (4 / (int)sizeof(T));           // ... and in a row of the fp32 state

    float st[2 * EPV], ai[EPV];                             // [0, EPV) the numerator, [EPV, 2 EPV) the denominator

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < 2 * EPV; ++d) st[d] = 0.0f;
        typename IO::raw_t r = IO::zero();
        if (on && active) r = IO::load(reinterpret_cast<const T*>(a.a + row * a.pb_a + cb));
        IO::unpack(r, ai);
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rb[U], rv[U], rc[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rb[u] = rv[u] = rc[u] = IO::zero();
                if (ok[u]) {
                    rb[u] = IO::load(reinterpret_cast<const T*>(a.b + (int64_t)c * a.pb_b + cb));
                    rv[u] = IO::load(reinterpret_cast<const T*>(a.v + (int64_t)c * a.pb_v + cb));
                    rc[u] = IO::load(reinterpret_cast<const T*>(a.c + (k0 + t + u) * a.pb_c + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fb[EPV], fv[EPV], e[EPV];
                IO::unpack(rb[u], fb);
                IO::unpack(rv[u], fv);
                IO::unpack(rc[u], e);
#pragma unroll
                for (int d = 0; d < EPV; ++d) e[d] = e[d] + ai[d] + fb[d];
                IO::store(reinterpret_cast<T*>(a.ehat + (k0 + t + u) * a.pb_ehat + cb), e);
                round_to_storage<T>(e);                     // the gate of the stored value: the one the backward recomputes
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float s = sigmoid(e[d]);
                    st[d] = fmaf(s, fv[d], st[d]);
                    st[EPV + d] += s;
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        float inv[EPV], o[EPV];
#pragma unroll
        for (int d = 0; d < EPV; ++d) {
            inv[d] = 1.0f / (st[EPV + d] + a.eps);
            o[d] = st[d] * inv[d];                          // a row without entries: 0 / eps
        }
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);
        store_state(a.inv + row * a.pb_inv + sb, inv);
        store_state(a.o32 + row * a.pb_o32 + sb, o);
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, st, lds, load_row, batch, finish);
}

// ---- rows: t[k] per entry, its row sum, and w_i ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void gated_rows_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const int64_t sb = cb * (4 / (int)sizeof(T));
    const bool sweep = a.t != nullptr;                      // without grad_c the pass only leaves w (uniform: a kernel argument)
    const bool has_ge = a.ge != nullptr;

    float acc[EPV], gs[EPV], oi[EPV];                       // sum of t; g_i / S_i; out_i

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = gs[d] = oi[d] = 0.0f;
        if (on && active) {
            float inv[EPV];
            IO::unpack(IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb)), gs);
            load_state(a.inv + row * a.pb_inv + sb, inv);
            load_state(a.o32 + row * a.pb_o32 + sb, oi);
#pragma unroll
            for (int d = 0; d < EPV; ++d) gs[d] *= inv[d];
        }
    };

    auto batch = [&](int64_t k0, int nb) {
        if (!sweep) return;
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rv[U], re[U], rg[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb && active;
                rv[u] = re[u] = rg[u] = IO::zero();
                if (ok[u]) {
                    rv[u] = IO::load(reinterpret_cast<const T*>(a.v + (int64_t)c * a.pb_v + cb));
                    re[u] = IO::load(reinterpret_cast<const T*>(a.ehat + (k0 + t + u) * a.pb_ehat + cb));
                    if (has_ge) rg[u] = IO::load(reinterpret_cast<const T*>(a.ge + (k0 + t + u) * a.pb_ge + cb));
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float fv[EPV], fe[EPV], o[EPV];
                IO::unpack(rv[u], fv);
                IO::unpack(re[u], fe);
                IO::unpack(rg[u], o);                       // ge[k], zeros without one
#pragma unroll
                for (int d = 0; d < EPV; ++d) {
                    const float s = sigmoid(fe[d]);
                    o[d] = fmaf(gs[d] * (fv[d] - oi[d]), s * (1.0f - s), o[d]);
                    acc[d] += o[d];
                }
                IO::store(reinterpret_cast<T*>(a.t + (k0 + t + u) * a.pb_t + cb), o);
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        if (a.ga) IO::store(reinterpret_cast<T*>(a.ga + row * a.pb_ga + cb), acc);     // a row without entries: zeros
        if (a.w) IO::store(reinterpret_cast<T*>(a.w + row * a.pb_w + cb), gs);
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, load_row, batch, finish);
}

// ---- cols: rows of A^T, two outputs ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void gated_cols_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[2 * EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;
    const bool need_b = a.gb != nullptr, need_v = a.gv != nullptr;     // uniform: kernel arguments

    float st[2 * EPV];                                      // [0, EPV) grad_b, [EPV, 2 EPV) grad_v

    auto load_row = [&](int64_t, int64_t, int64_t, bool) {
#pragma unroll
        for (int d = 0; d < 2 * EPV; ++d) st[d] = 0.0f;
    };

    // one batch of the row's entries, two in flight; the slot of t and ehat travels with the index
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        int my_slot = 0;
        if (lanes.sub < nb) {
            const int64_t s = a.perm[k0 + lanes.sub];
            my_slot = (int)max((int64_t)0, min(s, a.nnz - 1));
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t rt_[U], re[U], rw[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = rt::hand_round(my_col, t + u, lanes);
                const int slot = rt::hand_round(my_slot, t + u, lanes);
                ok[u] = t + u < nb && active;
                rt_[u] = re[u] = rw[u] = IO::zero();
                if (ok[u]) {
                    if (need_b) rt_[u] = IO::load(reinterpret_cast<const T*>(a.t + (int64_t)slot * a.pb_t + cb));
                    if (need_v) {
                        re[u] = IO::load(reinterpret_cast<const T*>(a.ehat + (int64_t)slot * a.pb_ehat + cb));
                        rw[u] = IO::load(reinterpret_cast<const T*>(a.w + (int64_t)i * a.pb_w + cb));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!ok[u]) continue;
                float ft[EPV], fe[EPV], fw[EPV];
                IO::unpack(rt_[u], ft);
                IO::unpack(re[u], fe);
                IO::unpack(rw[u], fw);
#pragma unroll
                for (int d = 0; d < EPV; ++d) st[d] += ft[d];
                if (need_v) {
#pragma unroll
                    for (int d = 0; d < EPV; ++d) st[EPV + d] = fmaf(sigmoid(fe[d]), fw[d], st[EPV + d]);
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        float o[EPV];                                       // a source no row references: zeros
        if (need_b) {
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = st[d];
            IO::store(reinterpret_cast<T*>(a.gb + row * a.pb_gb + cb), o);
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
    if (pass == DGLL_GATED_FORWARD) hipLaunchKernelGGL((gated_forward_kernel<T>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_GATED_ROWS) hipLaunchKernelGGL((gated_rows_kernel<T>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((gated_cols_kernel<T>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace gated
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_gated_pass(void* stream, const dgll_gated_desc* d) {
    static const char* const kPass = "dgll_hip_gated_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_gated_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_GATED_FORWARD || d->pass == DGLL_GATED_ROWS || d->pass == DGLL_GATED_COLS,
                 "dgll_hip_gated_pass: pass must be DGLL_GATED_FORWARD, DGLL_GATED_ROWS or DGLL_GATED_COLS");
    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, d->nnz, d->rowptr, d->col, true)) return rc;
    DGLL_REQUIRE(d->eps > 0.0f, "dgll_hip_gated_pass: eps must be positive (it is the denominator of a row without entries)");
    const auto [epv, esz] = rt::storage_of(d->dtype);

    gated::Args a{};
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.nnz = d->nnz;
    a.eps = d->eps;
    if (d->pass == DGLL_GATED_FORWARD) {
        DGLL_REQUIRE_OPERAND(kPass, a, d->F);
        DGLL_REQUIRE_OPERAND(kPass, b, d->F);
        DGLL_REQUIRE_OPERAND(kPass, c, d->F);
        DGLL_REQUIRE_OPERAND(kPass, v, d->F);
        DGLL_REQUIRE_OPERAND(kPass, out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, ehat, d->F);
        DGLL_REQUIRE_OPERAND(kPass, inv_s, d->F);
        DGLL_REQUIRE_OPERAND(kPass, out32, d->F);
        a.a = static_cast<const char*>(d->a);           a.pb_a = d->ld_a * esz;
        a.b = static_cast<const char*>(d->b);           a.pb_b = d->ld_b * esz;
        a.c = static_cast<const char*>(d->c);           a.pb_c = d->ld_c * esz;
        a.v = static_cast<const char*>(d->v);           a.pb_v = d->ld_v * esz;
        a.out = static_cast<char*>(d->out);             a.pb_out = d->ld_out * esz;
        a.ehat = static_cast<char*>(d->ehat);           a.pb_ehat = d->ld_ehat * esz;
        a.inv = reinterpret_cast<char*>(d->inv_s);      a.pb_inv = d->ld_inv_s * 4;
        a.o32 = reinterpret_cast<char*>(d->out32);      a.pb_o32 = d->ld_out32 * 4;
    } else if (d->pass == DGLL_GATED_ROWS) {
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->F);
        DGLL_REQUIRE_OPERAND(kPass, inv_s, d->F);
        DGLL_REQUIRE_OPERAND(kPass, out32, d->F);
        a.g = static_cast<const char*>(d->grad_out);    a.pb_g = d->ld_grad_out * esz;
        a.inv = reinterpret_cast<char*>(d->inv_s);      a.pb_inv = d->ld_inv_s * 4;
        a.o32 = reinterpret_cast<char*>(d->out32);      a.pb_o32 = d->ld_out32 * 4;
        DGLL_REQUIRE((d->grad_c != nullptr) == (d->grad_a != nullptr),
                     "dgll_hip_gated_pass: rows: grad_c and grad_a go together (both NULL: the pass only leaves w)");
        DGLL_REQUIRE(d->grad_c != nullptr || d->w != nullptr, "dgll_hip_gated_pass: rows: nothing to write (grad_c, grad_a and w are all NULL)");
        if (d->grad_c != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, v, d->F);
            DGLL_REQUIRE_OPERAND(kPass, ehat, d->F);
            DGLL_REQUIRE_OPERAND(kPass, grad_c, d->F);
            DGLL_REQUIRE_OPERAND(kPass, grad_a, d->F);
            a.v = static_cast<const char*>(d->v);       a.pb_v = d->ld_v * esz;
            a.ehat = static_cast<char*>(d->ehat);       a.pb_ehat = d->ld_ehat * esz;
            a.t = static_cast<char*>(d->grad_c);        a.pb_t = d->ld_grad_c * esz;
            a.ga = static_cast<char*>(d->grad_a);       a.pb_ga = d->ld_grad_a * esz;
            if (d->grad_ehat != nullptr) {
                DGLL_REQUIRE_OPERAND(kPass, grad_ehat, d->F);
                a.ge = static_cast<const char*>(d->grad_ehat);  a.pb_ge = d->ld_grad_ehat * esz;
            }
        }
        if (d->w != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, w, d->F);
            a.w = static_cast<char*>(d->w);             a.pb_w = d->ld_w * esz;
        }
    } else {
        DGLL_REQUIRE(d->perm != nullptr, "dgll_hip_gated_pass: cols: perm must be non-NULL (t and ehat are read at slot perm[k'])");
        DGLL_REQUIRE(d->grad_b != nullptr || d->grad_v != nullptr, "dgll_hip_gated_pass: cols: nothing to write (grad_b and grad_v are both NULL)");
        a.perm = d->perm;
        if (d->grad_b != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, grad_c, d->F);
            DGLL_REQUIRE_OPERAND(kPass, grad_b, d->F);
            a.t = static_cast<char*>(d->grad_c);        a.pb_t = d->ld_grad_c * esz;
            a.gb = static_cast<char*>(d->grad_b);       a.pb_gb = d->ld_grad_b * esz;
        }
        if (d->grad_v != nullptr) {
            DGLL_REQUIRE_OPERAND(kPass, ehat, d->F);
            DGLL_REQUIRE_OPERAND(kPass, w, d->F);
            DGLL_REQUIRE_OPERAND(kPass, grad_v, d->F);
            a.ehat = static_cast<char*>(d->ehat);       a.pb_ehat = d->ld_ehat * esz;
            a.w = static_cast<char*>(d->w);             a.pb_w = d->ld_w * esz;
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
    if (d->dtype == DGLL_F32) gated::launch<float>(d->pass, grid, st, a);
    else gated::launch<bf16_t>(d->pass, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
