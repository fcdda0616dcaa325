// gatv2.hip -- GATv2 ("How Attentive are Graph Attention Networks?"): the three gather passes of dgll_amd/ops_gatv2.py behind ONE entry
// point, dgll_hip_gatv2_pass (include/dgll_hip.h: dgll_gatv2_desc).
//
//   z_ij = xl_j + xr_i     e_ij = attn . lrelu(z_ij)     alpha = softmax over row i     out_i = sum_j alpha_ij xl_j       (per head)
//
// The nonlinearity sits inside the dot product, so the logit does not split into two per-node scalars as GAT's does (gat_kernel.hpp):
// every edge needs the whole feature row of both ends.  Nothing is stored per edge: the forward keeps an online softmax (running max,
// denominator and accumulator in fp32, exp2 form) over ONE gather of xl_j that serves score and value, and leaves lse_i = m + log l per
// (row, head); the two backward passes recompute alpha_ij = exp(e_ij - lse_i) from it.
//
//   forward     rows of A      gathers xl_j; holds xr_i, attn                     -> out, lse
//   rows        rows of A      gathers xl_j; holds g_i, xr_i, attn, lse_i         -> dxr, {lse_i, delta_i}, one dattn partial per workgroup
//               d_ij = <g_i, xl_j>, s = lrelu'(z), L = lrelu(z):  delta = sum alpha d,  P = sum alpha d s,  Q = sum alpha s,  PL, QL the same
//               with L for s;  dxr_i = attn (P - delta Q),  dattn += PL - delta QL.  Bilinear in sums over the row: one sweep, and delta_i
//               comes from the pass's own fp32 dot products, not from a rounded stored output.
//   transposed  rows of A^T    holds xl_j, attn; gathers g_i, xr_i, {lse_i, delta_i} -> dxl_j = sum_i alpha g_i + alpha (d - delta_i) attn s
//
// Lane layout, tiles, index batches and the long-row merge: row_tiles.hpp.  Here a head owns `lph` adjacent lanes (a power of two >=
// its D / EPV 16-byte vectors; the lanes past them idle) and a row `lpr` lanes holding `hpb` whole heads; rows wider than 64 lanes
// are cut into column blocks of whole heads over blockIdx.y.  The partials of a long row are (m, l, acc), the five sums, the
// accumulator.  No atomics: the dattn partials [blocks, heads * D] are summed afterwards in a fixed order.
#include "row_tiles.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace gv2 {

constexpr int kLongRow = DGLL_GATV2_LONG_ROW;  // rows longer than this are swept by a whole workgroup
using rt::head_sum2;
using rt::kLn2;
using rt::kLog2e;

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    int64_t n_rows, n_cols, tiles;
    const char* xl; int64_t pb_xl;          // pitches in BYTES
    const char* xr; int64_t pb_xr;
    const char* g;  int64_t pb_g;
    char* out;      int64_t pb_out;
    const float* attn;
    float* lse;                             // [n_rows, heads]      forward: written; rows: read
    float* ld2;                             // [n_dst, 2 heads]     rows: written; transposed: read
    float* dpart;                           // [gridDim.x, heads * D]  rows: written
    int heads, D, vph, lph, hpb, lpr;
    float slope;
};

template <int KIND, int EPV> struct Parts { static constexpr int N = KIND == 0 ? EPV + 2 : (KIND == 1 ? 4 * EPV + 1 : EPV); };

// State of one lane (its EPV columns of one head of one row), flat so that the long-row merge can move it through LDS:
//   KIND 0: [0] m (log2 units)  [1] l  [2 ..] acc        KIND 1: [0] delta  then P | Q | PL | QL, EPV each        KIND 2: acc
template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void gatv2_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), NP = Parts<KIND, EPV>::N, U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[NP * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int hl = lanes.sub / a.lph, v = lanes.sub - hl * a.lph;
    const int head = (int)blockIdx.y * a.hpb + hl;
    const bool active = hl < a.hpb && head < a.heads && v < a.vph;
    const int hx = active ? head : 0;
    const int64_t cb = active ? ((int64_t)head * a.D + (int64_t)v * EPV) * (int64_t)sizeof(T) : 0;   // byte offset of the lane's columns
    const float slope = a.slope;

    float at[EPV];
#pragma unroll
    for (int d = 0; d < EPV; ++d) at[d] = active ? a.attn[(int64_t)hx * a.D + v * EPV + d] : 0.0f;

    float own[EPV], gi[EPV], lse_i = 0.0f;      // per row: xr_i (forward, rows) or xl_j (transposed); g_i and lse_i (rows)
    float st[NP];
    float dacc[KIND == 1 ? EPV : 1];            // rows: this lane's share of dattn over the rows it finalised
#pragma unroll
    for (int d = 0; d < (KIND == 1 ? EPV : 1); ++d) dacc[d] = 0.0f;

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        const bool ld = on && active;
        typename IO::raw_t r = IO::zero();
        if (ld) r = IO::load(reinterpret_cast<const T*>((KIND == 2 ? a.xl : a.xr) + row * (KIND == 2 ? a.pb_xl : a.pb_xr) + cb));
        IO::unpack(r, own);
        if constexpr (KIND == 1) {
            typename IO::raw_t rg = IO::zero();
            if (ld) rg = IO::load(reinterpret_cast<const T*>(a.g + row * a.pb_g + cb));
            IO::unpack(rg, gi);
            lse_i = ld ? a.lse[row * a.heads + hx] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) st[k] = 0.0f;
        if constexpr (KIND == 0) st[0] = -INFINITY;
    };

    // one entry of the row: column c of the pass's CSR (a source row in the forward and rows passes, a destination row in the
    // transposed pass); !ok: a masked slot of the last batch -- its loads were skipped (zeros) and it adds nothing
    auto entry = [&](bool ok, const typename IO::raw_t& r0, const typename IO::raw_t& r1, float lse_c, float delta_c) {
        float f[EPV];
        IO::unpack(r0, f);
        if constexpr (KIND == 0) {
            float p = 0.0f;
#pragma unroll
            for (int d = 0; d < EPV; ++d) p = fmaf(at[d], lrelu(f[d] + own[d], slope), p);
            float e2 = head_sum(p, a.lph) * kLog2e;
            e2 = ok ? e2 : -INFINITY;
            const float m = st[0], mn = fmaxf(m, e2);
            const float sc = mn == m ? 1.0f : __builtin_amdgcn_exp2f(m - mn);
            const float w = ok ? __builtin_amdgcn_exp2f(e2 - mn) : 0.0f;
            st[0] = mn;
            st[1] = fmaf(st[1], sc, w);
#pragma unroll
            for (int d = 0; d < EPV; ++d) st[2 + d] = fmaf(st[2 + d], sc, w * f[d]);
        } else if constexpr (KIND == 1) {
            float s[EPV], L[EPV], p = 0.0f, q = 0.0f;
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                const float z = f[d] + own[d];
                s[d] = z > 0.0f ? 1.0f : slope;
                L[d] = z * s[d];
                p = fmaf(at[d], L[d], p);
                q = fmaf(gi[d], f[d], q);
            }
            head_sum2(p, q, a.lph);
            const float alpha = ok ? __builtin_amdgcn_exp2f((p - lse_i) * kLog2e) : 0.0f;
            const float ad = alpha * q;
            st[0] += ad;
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                st[1 + d] = fmaf(ad, s[d], st[1 + d]);
                st[1 + EPV + d] = fmaf(alpha, s[d], st[1 + EPV + d]);
                st[1 + 2 * EPV + d] = fmaf(ad, L[d], st[1 + 2 * EPV + d]);
                st[1 + 3 * EPV + d] = fmaf(alpha, L[d], st[1 + 3 * EPV + d]);
            }
        } else {
            float gv[EPV], s[EPV], p = 0.0f, q = 0.0f;     // f = xr_i, gv = g_i, own = xl_j
            IO::unpack(r1, gv);
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                const float z = own[d] + f[d];
                s[d] = z > 0.0f ? 1.0f : slope;
                p = fmaf(at[d], z * s[d], p);
                q = fmaf(gv[d], own[d], q);
            }
            head_sum2(p, q, a.lph);
            const float alpha = ok ? __builtin_amdgcn_exp2f((p - lse_c) * kLog2e) : 0.0f;
            const float de = alpha * (q - delta_c);
#pragma unroll
            for (int d = 0; d < EPV; ++d) st[d] = fmaf(alpha, gv[d], fmaf(de * at[d], s[d], st[d]));
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
                        r0[u] = IO::load(reinterpret_cast<const T*>(a.xr + c * a.pb_xr + cb));
                        r1[u] = IO::load(reinterpret_cast<const T*>(a.g + c * a.pb_g + cb));
                        lse_c[u] = a.ld2[c * 2 * a.heads + hx];
                        delta_c[u] = a.ld2[c * 2 * a.heads + a.heads + hx];
                    } else {
                        r0[u] = IO::load(reinterpret_cast<const T*>(a.xl + c * a.pb_xl + cb));
                    }
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
            for (int d = 0; d < EPV; ++d) {
                o[d] = at[d] * (st[1 + d] - delta * st[1 + EPV + d]);
                dacc[d] += st[1 + 2 * EPV + d] - delta * st[1 + 3 * EPV + d];
            }
            if (v == 0) {
                a.ld2[row * 2 * a.heads + head] = lse_i;
                a.ld2[row * 2 * a.heads + a.heads + head] = delta;
            }
        } else {
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = st[d];                        // a row nobody references: zeros
        }
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);
    };

    rt::reduce_rows<KIND == 0>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, st, lds, load_row, batch, finish);

    if constexpr (KIND == 1) {                  // this workgroup's dattn partial: its lane groups' shares in group order
        const int tid = lanes.tid;
        __syncthreads();
#pragma unroll
        for (int d = 0; d < EPV; ++d) lds[d * kBlock + tid] = dacc[d];
        __syncthreads();
        if (tid < lanes.lpr && active) {
            float* dst = a.dpart + (int64_t)blockIdx.x * a.heads * a.D + (int64_t)head * a.D + v * EPV;
#pragma unroll
            for (int d = 0; d < EPV; ++d) {
                float sum = 0.0f;
                for (int p = 0; p < lanes.groups; ++p) sum += lds[d * kBlock + p * lanes.lpr + tid];
                dst[d] = sum;
            }
        }
    }
}

// grad_attn[c] = sum over the workgroups' partials, in workgroup order: a lane per column
__global__ __launch_bounds__(kBlock) void dattn_sum_kernel(const float* __restrict__ part, int64_t blocks, int feat, float* __restrict__ dattn) {
    const int c = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (c >= feat) return;
    float sum = 0.0f;
    for (int64_t b = 0; b < blocks; ++b) sum += part[b * feat + c];
    dattn[c] = sum;
}

template <typename T>
void launch(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_GATV2_FORWARD) hipLaunchKernelGGL((gatv2_kernel<T, 0>), grid, dim3(kBlock), 0, s, a);
    else if (pass == DGLL_GATV2_ROWS) hipLaunchKernelGGL((gatv2_kernel<T, 1>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((gatv2_kernel<T, 2>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace gv2
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_gatv2_pass(void* stream, const dgll_gatv2_desc* d) {
    static const char* const kPass = "dgll_hip_gatv2_pass";
    DGLL_REQUIRE(d != nullptr, "the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_GATV2_FORWARD || d->pass == DGLL_GATV2_ROWS || d->pass == DGLL_GATV2_TRANSPOSED,
                 "pass must be DGLL_GATV2_FORWARD, DGLL_GATV2_ROWS or DGLL_GATV2_TRANSPOSED");
    if (const int rc = rt::require_head_pass(d->dtype, d->heads, d->D, d->n_rows, d->n_cols, d->rowptr, d->col)) return rc;
    const auto [epv, esz] = rt::storage_of(d->dtype);
    const int64_t feat = (int64_t)d->heads * d->D;
    DGLL_REQUIRE_OPERAND(kPass, xl, d->heads * d->D);
    DGLL_REQUIRE_OPERAND(kPass, xr, d->heads * d->D);
    DGLL_REQUIRE_OPERAND(kPass, out, d->heads * d->D);
    DGLL_REQUIRE(d->attn != nullptr, "attn must be non-NULL");
    if (d->pass == DGLL_GATV2_FORWARD) {
        DGLL_REQUIRE(d->lse != nullptr, "forward: lse must be non-NULL");
    } else {
        DGLL_REQUIRE_OPERAND(kPass, grad_out, d->heads * d->D);
        DGLL_REQUIRE(d->lse_delta != nullptr, "backward: lse_delta must be non-NULL");
        if (d->pass == DGLL_GATV2_ROWS)
            DGLL_REQUIRE(d->lse && d->dattn_part && d->dattn_blocks >= 1 && d->dattn_blocks <= rt::kMaxGridX,
                         "rows pass: lse and the dattn partials non-NULL, 1 <= dattn_blocks <= 2^22");
    }

    gv2::Args a;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.xl =static_cast<const char*>(d->xl);       a.pb_xl = d->ld_xl * esz;
    a.xr = static_cast<const char*>(d->xr);       a.pb_xr = d->ld_xr * esz;
    a.g = static_cast<const char*>(d->grad_out);  a.pb_g = d->ld_grad_out * esz;
    a.out = static_cast<char*>(d->out);           a.pb_out = d->ld_out * esz;
    a.attn = d->attn;
    a.lse = d->lse;
    a.ld2 = d->lse_delta;
    a.dpart = d->dattn_part;
    a.heads = d->heads;
    a.D = d->D;
    a.slope = d->slope;
    const rt::HeadGeometry geo = rt::make_head_geometry(d->heads, d->D, epv, d->n_rows);
    rt::set_geometry(a, geo);
    const int64_t gx = d->pass == DGLL_GATV2_ROWS ? d->dattn_blocks : geo.grid;    // every partial row is written, by a workgroup without tiles as zeros
    if (gx == 0) return DGLL_OK;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, gx, geo.col_blocks, 1, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) gv2::launch<float>(d->pass, grid, st, a);
    else gv2::launch<bf16_t>(d->pass, grid, st, a);
    if (d->pass == DGLL_GATV2_ROWS && d->dattn)
        hipLaunchKernelGGL(gv2::dattn_sum_kernel, dim3((unsigned)((feat + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, d->dattn_part,
                           d->dattn_blocks, (int)feat, d->dattn);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
