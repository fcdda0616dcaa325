// sparse_attn.hip -- scaled dot-product attention over the edges of a graph (DGL's DotGatConv, PyG's TransformerConv, graph
// transformers): the three gather passes of dgll_amd/ops_attn.py behind ONE entry point, dgll_hip_sparse_attn_pass
// (include/dgll_hip.h: dgll_attn_desc).
//
//   s_ij = scale <q_i, k_j>     alpha = softmax over row i     out_i = sum_j alpha_ij v_j     lse_i = log sum_j exp s_ij       (per head)
//
// The score is a dot product of two DIFFERENT rows and the value a third: every edge gathers k_j and v_j while the row holds q_i
// (kv_shared: k and v are one buffer, each source row is loaded once and serves score and value -- one gather per edge, as GATv2).
// Nothing is stored per edge: the forward keeps an online softmax (running max, denominator and accumulator in fp32, exp2 form) and
// leaves lse_i per (row, head); the two backward passes recompute alpha_ij = exp(s_ij - lse_i) from it.  With g = d out:
//
//   forward  rows of A     holds q_i; gathers k_j, v_j                                  -> out, lse
//   rows     rows of A     holds q_i, g_i, lse_i; gathers k_j, v_j                      -> dq, {lse_i, delta_i}
//            d_ij = <g_i, v_j>,  delta_i = sum alpha d,  A = sum alpha d k_j,  B = sum alpha k_j:  dq_i = scale (A - delta_i B).  Bilinear
//            in sums over the row: one sweep, and delta_i comes from the pass's own fp32 dot products, not from a rounded stored output.
//   cols     rows of A^T   holds k_j, v_j; gathers q_i, g_i, {lse_i, delta_i}           -> dv_j = sum_i alpha g_i,
//                                                                                          dk_j = scale sum_i alpha (d_ij - delta_i) q_i
//
// Lane layout, tiles, index batches and the long-row merge: row_tiles.hpp; heads, lanes of a head and column blocks as in gatv2.hip.
#include "row_tiles.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace sat {

constexpr int kLongRow = DGLL_ATTN_LONG_ROW;   // rows longer than this are swept by a whole workgroup
using rt::head_sum2;
using rt::kLn2;
using rt::kLog2e;

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    int64_t n_rows, n_cols, tiles;
    const char* q; int64_t pb_q;            // pitches in BYTES
    const char* k; int64_t pb_k;
    const char* v; int64_t pb_v;
    const char* g; int64_t pb_g;
    char* out;     int64_t pb_out;          // forward: out; rows: dq; cols: dk
    char* out2;    int64_t pb_out2;         // cols: dv
    float* lse;                             // [n_dst, heads]      forward: written; rows: read
    float* ld2;                             // [n_dst, 2 heads]    rows: written; cols: read
    int heads, D, vph, lph, hpb, lpr, kv_shared;
    float scale;
};

template <int KIND, int EPV> struct Parts { static constexpr int N = KIND == 0 ? EPV + 2 : (KIND == 1 ? 2 * EPV + 1 : 2 * EPV); };

// State of one lane (its EPV columns of one head of one row), flat so that the long-row merge can move it through LDS:
//   KIND 0: [0] m (log2 units)  [1] l  [2 ..] acc        KIND 1: [0] delta  then A | B, EPV each        KIND 2: dv | dk (unscaled), EPV each
template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void sparse_attn_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), NP = Parts<KIND, EPV>::N, U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[NP * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int hl = lanes.sub / a.lph, v = lanes.sub - hl * a.lph;
    const int head = (int)blockIdx.y * a.hpb + hl;
    const bool active = hl < a.hpb && head < a.heads && v < a.vph;
    const int hx = active ? head : 0;
    const int64_t cb = active ? ((int64_t)head * a.D + (int64_t)v * EPV) * (int64_t)sizeof(T) : 0;   // byte offset of the lane's columns
    const bool shared = a.kv_shared != 0;
    const float scale = a.scale, sl2 = a.scale * kLog2e;     // s * sl2: the score in log2 units

    // per row: own = q_i (forward, rows) or k_j (cols); held = g_i (rows) or v_j (cols); nl = -lse_i in log2 units (rows)
    float own[EPV], held[EPV], lse_i = 0.0f, nl = 0.0f;
    float st[NP];

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        const bool ld = on && active;
        typename IO::raw_t r = IO::zero();
        if (ld) r = IO::load(reinterpret_cast<const T*>((KIND == 2 ? a.k : a.q) + row * (KIND == 2 ? a.pb_k : a.pb_q) + cb));
        IO::unpack(r, own);
        if constexpr (KIND == 1) {
            typename IO::raw_t rg = IO::zero();
            if (ld) rg = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
            IO::unpack(rg, held);
            lse_i = ld ? a.lse[row * a.heads + hx] : 0.0f;
            nl = -lse_i * kLog2e;
        } else if constexpr (KIND == 2) {
            typename IO::raw_t rv = r;
            if (ld && !shared) rv = IO::load(reinterpret_cast<const T*>(a.v + row * a.pb_v + cb));
            IO::unpack(rv, held);
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) st[k] = 0.0f;
        if constexpr (KIND == 0) st[0] = -INFINITY;
    };

    // one entry of the row: column c of the pass's CSR (a source row in the forward and rows passes: r0 = k_c, r1 = v_c; a destination
    // row in the cols pass: r0 = q_c, r1 = g_c); !ok: a masked slot of the last batch -- its loads were skipped (zeros), it adds nothing
    auto entry = [&](bool ok, const typename IO::raw_t& r0, const typename IO::raw_t& r1, float lse_c, float delta_c) {
        float f0[EPV], f1[EPV];
        IO::unpack(r0, f0);
        IO::unpack(r1, f1);
        if constexpr (KIND == 0) {
            float p = 0.0f;
#pragma unroll
            for (int d = 0; d < EPV; ++d) p = fmaf(own[d], f0[d], p);
            float e2 = head_sum(p, a.lph) * sl2;
            e2 = ok ? e2 : -INFINITY;
            const float m = st[0], mn = fmaxf(m, e2);
            const float sc = mn == m ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
            const float w = ok ? __builtin_amdgcn_exp2f(e2 - mn) : 0.0f;
            st[0] = mn;
            st[1] = fmaf(st[1], sc, w);
#pragma unroll
            for (int d = 0; d < EPV; ++d) st[2 + d] = fmaf(st[2 + d], sc, w * f1[d]);
        } else if constexpr (KIND == 1) {
            float p = 0.0f, q = 0.0f;
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                p = fmaf(own[d], f0[d], p);
                q = fmaf(held[d], f1[d], q);
            }
            head_sum2(p, q, a.lph);
            const float alpha = ok ? __builtin_amdgcn_exp2f(fmaf(p, sl2, nl)) : 0.0f;
            const float ad = alpha * q;
            st[0] += ad;
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                st[1 + d] = fmaf(ad, f0[d], st[1 + d]);
                st[1 + EPV + d] = fmaf(alpha, f0[d], st[1 + EPV + d]);
            }
        } else {
            float p = 0.0f, q = 0.0f;                       // f0 = q_i, f1 = g_i, own = k_j, held = v_j
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                p = fmaf(f0[d], own[d], p);
                q = fmaf(f1[d], held[d], q);
            }
            head_sum2(p, q, a.lph);
            const float alpha = ok ? __builtin_amdgcn_exp2f(fmaf(p, sl2, -lse_c * kLog2e)) : 0.0f;
            const float de = alpha * (q - delta_c);
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                st[d] = fmaf(alpha, f1[d], st[d]);
                st[EPV + d] = fmaf(de, f0[d], st[EPV + d]);
            }
        }
    };

    // one batch of the row's entries, two entries in flight
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t r0[U], r1[U];
            float lse_c[U], delta_c[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t c = rt::hand_round(my_col, t + u, lanes);
                ok[u] = t + u < nb;
                r0[u] = IO::zero();
                r1[u] = IO::zero();
                lse_c[u] = delta_c[u] = 0.0f;
                if (ok[u] && active) {
                    if constexpr (KIND == 2) {
                        r0[u] = IO::load(reinterpret_cast<const T*>(a.q + c * a.pb_q + cb));
                        r1[u] = IO::load(reinterpret_cast<const T*>(a.g + c * a.pb_g + cb));
                        lse_c[u] = a.ld2[c * 2 * a.heads + hx];
                        delta_c[u] = a.ld2[c * 2 * a.heads + a.heads + hx];
                    } else {
                        r0[u] = IO::load(reinterpret_cast<const T*>(a.k + c * a.pb_k + cb));
                        if (!shared) r1[u] = IO::load(reinterpret_cast<const T*>(a.v + c * a.pb_v + cb));
                    }
                }
                if constexpr (KIND != 2) {
                    if (shared) r1[u] = r0[u];          // one load of the source row serves score and value
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) entry(ok[u], r0[u], r1[u], lse_c[u], delta_c[u]);
        }
    };

    // the row's outputs from its complete state; no cross-lane traffic (the long-row path calls it from one lane group alone)
    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        float o[EPV];
        if constexpr (KIND == 0) {
            const float l = st[1], inv = l > 0.0f ? 1.0f / l : 0.0f;           // an empty row: 0, never NaN
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = st[2 + d] * inv;
            if (v == 0) a.lse[row * a.heads + head] = l > 0.0f ? (st[0] + __builtin_amdgcn_logf(l)) * kLn2 : 0.0f;
        } else if constexpr (KIND == 1) {
            const float delta = st[0];
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = scale * (st[1 + d] - delta * st[1 + EPV + d]);
            if (v == 0) {
                a.ld2[row * 2 * a.heads + head] = lse_i;
                a.ld2[row * 2 * a.heads + a.heads + head] = delta;
            }
        } else {
            float o2[EPV];
#pragma unroll
            for (int d = 0; d < EPV; ++d) {                                    // a row nobody references: zeros
                o2[d] = st[d];
                o[d] = scale * st[EPV + d];
            }
            IO::store(reinterpret_cast<T*>(a.out2 + row * a.pb_out2 + cb), o2);
        }
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);
    };

    rt::reduce_rows<KIND == 0>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, st, lds, load_row, batch, finish);
}

template <typename T>
void launch(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_ATTN_FORWARD) hipLaunchKernelGGL((sparse_attn_kernel<T, 0>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_ATTN_ROWS) hipLaunchKernelGGL((sparse_attn_kernel<T, 1>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((sparse_attn_kernel<T, 2>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace sat
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_sparse_attn_pass(void* stream, const dgll_attn_desc* d) {
    static const char* const kPass = "dgll_hip_sparse_attn_pass";
    DGLL_REQUIRE(d != nullptr, "the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_ATTN_FORWARD || d->pass == DGLL_ATTN_ROWS || d->pass == DGLL_ATTN_COLS,
                 "pass must be DGLL_ATTN_FORWARD, DGLL_ATTN_ROWS or DGLL_ATTN_COLS");
    if (const int rc = rt::require_head_pass(d->dtype, d->heads, d->D, d->n_rows, d->n_cols, d->rowptr, d->col)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    DGLL_REQUIRE_OPERAND(kPass, q, d->heads * d->D);
    DGLL_REQUIRE_OPERAND(kPass, k, d->heads * d->D);
    DGLL_REQUIRE_OPERAND(kPass, v, d->heads * d->D);
    DGLL_REQUIRE_OPERAND(kPass, out, d->heads * d->D);
    DGLL_REQUIRE(!d->kv_shared || (d->k == d->v && d->ld_k == d->ld_v), "kv_shared: k and v must be the same buffer with the same pitch");
    if (d->pass == DGLL_ATTN_FORWARD) {
        DGLL_REQUIRE(d->lse != nullptr, "forward: lse must be non-NULL");
    } else {
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->heads * d->D);
        DGLL_REQUIRE(d->lse_delta != nullptr, "backward: lse_delta must be non-NULL");
        if (d->pass == DGLL_ATTN_ROWS) {
            DGLL_REQUIRE(d->lse != nullptr, "rows pass: lse must be non-NULL");
        } else {
            DGLL_REQUIRE_OPERAND(kPass, out2, d->heads * d->D);          // dv
        }
    }

    sat::Args a;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.q = static_cast<const char*>(d->q);         a.pb_q = d->ld_q * esz;
    a.k = static_cast<const char*>(d->k);         a.pb_k = d->ld_k * esz;
    a.v = static_cast<const char*>(d->v);         a.pb_v = d->ld_v * esz;
    a.g = static_cast<const char*>(d->grad_out);  a.pb_g = d->ld_grad_out * esz;
    a.out = static_cast<char*>(d->out);           a.pb_out = d->ld_out * esz;
    a.out2 = static_cast<char*>(d->out2);         a.pb_out2 = d->ld_out2 * esz;
    a.lse = d->lse;
    a.ld2 = d->lse_delta;
    a.heads = d->heads;
    a.D = d->D;
    a.scale = d->scale;
    a.kv_shared = d->kv_shared ? 1 : 0;
    const rt::HeadGeometry geo = rt::make_head_geometry(d->heads, d->D, epv, d->n_rows);
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) sat::launch<float>(d->pass, grid, st, a);
    else sat::launch<bf16_t>(d->pass, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
