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
// Lane layout, tiles, index batches and the long-row merge are those of gatv2.hip (the skeleton is duplicated on purpose: DESIGN 10):
// a head owns `lph` adjacent lanes (a power of two >= its D / EPV 16-byte vectors; the lanes past them idle), a row `lpr` lanes (a
// power of two >= 8 holding `hpb` whole heads), a wavefront 64 / lpr rows at a time.  Rows wider than 64 lanes are cut into column
// blocks of whole heads over blockIdx.y.  A workgroup takes tiles of 4 * 64 / lpr consecutive rows: every lane group sweeps its own
// row (indices read lpr at a time, coalesced, and handed round the group), then the rows of the tile longer than kLongRow are taken
// by the whole workgroup one after another -- lane group k of the 4 * 64 / lpr takes index batches k, k + groups, ... and the partials
// are merged through LDS in group order by the first group.  No atomics anywhere: two runs give the same bits.
#include "common.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace sat {

constexpr int kLongRow = DGLL_ATTN_LONG_ROW;   // rows longer than this are swept by a whole workgroup
constexpr int kMinGroup = 8;                   // lanes per row at least (index batches of at least 8)
constexpr int64_t kMaxGridX = 1 << 22;         // tiles are taken grid-stride past this
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

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

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ void head_sum2(float& p, float& q, int lph) {
    for (int off = 1; off < lph; off <<= 1) {
        p += __shfl_xor(p, off);
        q += __shfl_xor(q, off);
    }
}

template <int KIND, int EPV> struct Parts { static constexpr int N = KIND == 0 ? EPV + 2 : (KIND == 1 ? 2 * EPV + 1 : 2 * EPV); };

// State of one lane (its EPV columns of one head of one row), flat so that the long-row merge can move it through LDS:
//   KIND 0: [0] m (log2 units)  [1] l  [2 ..] acc        KIND 1: [0] delta  then A | B, EPV each        KIND 2: dv | dk (unscaled), EPV each
template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void sparse_attn_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), NP = Parts<KIND, EPV>::N, U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[NP * kBlock];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int lpr = a.lpr, slots = kWave / lpr, groups = kWavesPerBlock * slots;
    const int sub = lane & (lpr - 1), gbase = lane - sub, gid = wave * slots + lane / lpr;
    const int hl = sub / a.lph, v = sub - hl * a.lph;
    const int head = (int)blockIdx.y * a.hpb + hl;
    const bool active = hl < a.hpb && head < a.heads && v < a.vph;
    const int hx = active ? head : 0;
    const int64_t cb = active ? ((int64_t)head * a.D + (int64_t)v * EPV) * (int64_t)sizeof(T) : 0;   // byte offset of the lane's columns
    const bool shared = a.kv_shared != 0;
    const float scale = a.scale, sl2 = a.scale * kLog2e;     // s * sl2: the score in log2 units

    // per row: own = q_i (forward, rows) or k_j (cols); held = g_i (rows) or v_j (cols); nl = -lse_i in log2 units (rows)
    float own[EPV], held[EPV], lse_i = 0.0f, nl = 0.0f;
    float st[NP];

    auto load_row = [&](int64_t row, bool on) {
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

    // entries [b, e) in batches of lpr; this lane group takes batches first, first + stride, ...  Every lane of the wavefront runs
    // every iteration (the trip counts are the wavefront's maxima), so the hand-round shuffles never meet an idle lane.
    auto sweep = [&](int64_t b, int64_t e, int first, int stride) {
        const int total = (int)((e - b + lpr - 1) / lpr);
        const int mine = first < total ? (total - first + stride - 1) / stride : 0;
        const int max_batches = wave_max(mine);
        for (int it = 0; it < max_batches; ++it) {
            const int64_t k0 = b + ((int64_t)first + (int64_t)it * stride) * lpr;
            int nb = 0;
            if (it < mine) nb = e - k0 < lpr ? (int)(e - k0) : lpr;
            int my_col = 0;
            if (sub < nb) my_col = a.col[k0 + sub];
            my_col = min(max(my_col, 0), (int)a.n_cols - 1);      // a corrupt index reads a wrong row, never outside the matrix
            const int max_nb = wave_max(nb);
            for (int t = 0; t < max_nb; t += U) {
                typename IO::raw_t r0[U], r1[U];
                float lse_c[U], delta_c[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t c = __shfl(my_col, gbase + ((t + u) & (lpr - 1)));
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
        }
    };

    // the row's outputs from its complete state; no cross-lane traffic (the long-row path calls it from one lane group alone)
    auto finish = [&](int64_t row) {
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

    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * groups;
        {   // rows of at most kLongRow entries: one per lane group
            const int64_t row = row0 + gid;
            int64_t b = 0, e = 0;
            if (row < a.n_rows) { b = a.rowptr[row]; e = a.rowptr[row + 1]; }
            const bool mine = row < a.n_rows && e - b <= kLongRow;
            if (!mine) e = b;
            load_row(mine ? row : 0, mine);
            sweep(b, e, 0, 1);
            if (mine) finish(row);
        }
        for (int r = 0; r < groups; ++r) {      // longer rows: the whole workgroup, one row after another (all conditions block-uniform)
            const int64_t row = row0 + r;
            if (row >= a.n_rows) break;
            const int64_t b = uniform64(a.rowptr[row]), e = uniform64(a.rowptr[row + 1]);
            if (e - b <= kLongRow) continue;
            load_row(row, true);
            sweep(b, e, gid, groups);
            __syncthreads();                    // the previous merge has read its partials
#pragma unroll
            for (int k = 0; k < NP; ++k) lds[k * kBlock + tid] = st[k];
            __syncthreads();
            if (tid < lpr) {                    // the first lane group (sub == tid) merges the others in group order
                for (int p = 1; p < groups; ++p) {
                    float o[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) o[k] = lds[k * kBlock + p * lpr + tid];
                    if constexpr (KIND == 0) {
                        const float mn = fmaxf(st[0], o[0]);
                        const float s0 = st[0] == mn ? 1.0f : __builtin_amdgcn_exp2f(st[0] - mn);
                        const float s1 = o[0] == mn ? 1.0f : __builtin_amdgcn_exp2f(o[0] - mn);
                        st[0] = mn;
#pragma unroll
                        for (int k = 1; k < NP; ++k) st[k] = fmaf(st[k], s0, o[k] * s1);
                    } else {
#pragma unroll
                        for (int k = 0; k < NP; ++k) st[k] += o[k];
                    }
                }
                finish(row);
            }
        }
    }
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
    DGLL_REQUIRE(d != nullptr, "the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_ATTN_FORWARD || d->pass == DGLL_ATTN_ROWS || d->pass == DGLL_ATTN_COLS,
                 "pass must be DGLL_ATTN_FORWARD, DGLL_ATTN_ROWS or DGLL_ATTN_COLS");
    DGLL_REQUIRE(d->dtype == DGLL_F32 || d->dtype == DGLL_BF16, "dtype must be DGLL_F32 or DGLL_BF16");
    const int epv = d->dtype == DGLL_F32 ? 4 : 8;
    DGLL_REQUIRE(d->heads >= 1 && d->D >= epv && d->D % epv == 0,
                 "heads >= 1 and D a positive multiple of the 16-byte vector width (4 fp32, 8 bf16 columns)");
    DGLL_REQUIRE(d->D / epv <= kWave, "a head may span at most 64 vectors (D <= 256 fp32, 512 bf16)");
    DGLL_REQUIRE((int64_t)d->heads * d->D < (1 << 20), "heads * D < 2^20");
    DGLL_REQUIRE(d->n_rows >= 0 && d->n_rows < (1ll << 31) && d->n_cols > 0 && d->n_cols < (1ll << 31),
                 "row count in [0, 2^31), gathered row count in [1, 2^31)");
    DGLL_REQUIRE(d->rowptr && d->col, "the CSR arrays must be non-NULL");
    DGLL_REQUIRE(d->q && d->k && d->v && d->out, "q, k, v and the pass's output matrix must be non-NULL");
    const int64_t feat = (int64_t)d->heads * d->D;
    DGLL_REQUIRE(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->out) && d->ld_q % epv == 0 && d->ld_k % epv == 0 &&
                     d->ld_v % epv == 0 && d->ld_out % epv == 0 && d->ld_q >= feat && d->ld_k >= feat && d->ld_v >= feat && d->ld_out >= feat,
                 "q, k, v and the output: 16-byte aligned base, a pitch of whole 16-byte vectors >= heads * D");
    DGLL_REQUIRE(!d->kv_shared || (d->k == d->v && d->ld_k == d->ld_v), "kv_shared: k and v must be the same buffer with the same pitch");
    if (d->pass == DGLL_ATTN_FORWARD) {
        DGLL_REQUIRE(d->lse != nullptr, "forward: lse must be non-NULL");
    } else {
        DGLL_REQUIRE(d->grad_out && aligned16(d->grad_out) && d->ld_grad_out % epv == 0 && d->ld_grad_out >= feat,
                     "backward: grad_out non-NULL, 16-byte aligned, a pitch of whole 16-byte vectors >= heads * D");
        DGLL_REQUIRE(d->lse_delta != nullptr, "backward: lse_delta must be non-NULL");
        if (d->pass == DGLL_ATTN_ROWS) {
            DGLL_REQUIRE(d->lse != nullptr, "rows pass: lse must be non-NULL");
        } else {
            DGLL_REQUIRE(d->out2 && aligned16(d->out2) && d->ld_out2 % epv == 0 && d->ld_out2 >= feat,
                         "cols pass: out2 (dv) non-NULL, 16-byte aligned, a pitch of whole 16-byte vectors >= heads * D");
        }
    }

    sat::Args a;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    const int64_t esz = d->dtype == DGLL_F32 ? 4 : 2;
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
    a.vph = d->D / epv;
    a.lph = 1;
    while (a.lph < a.vph) a.lph <<= 1;
    a.hpb = kWave / a.lph < d->heads ? kWave / a.lph : d->heads;       // whole heads per column block
    a.lpr = sat::kMinGroup;
    while (a.lpr < a.hpb * a.lph) a.lpr <<= 1;
    const int groups = kWavesPerBlock * (kWave / a.lpr);
    a.tiles = (d->n_rows + groups - 1) / groups;
    const int64_t gx = a.tiles < sat::kMaxGridX ? a.tiles : sat::kMaxGridX;
    if (gx == 0) return DGLL_OK;
    DGLL_REQUIRE((d->heads + a.hpb - 1) / a.hpb <= 65535, "at most 65535 column blocks of whole heads");
    const dim3 grid((unsigned)gx, (unsigned)((d->heads + a.hpb - 1) / a.hpb));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == DGLL_F32) sat::launch<float>(d->pass, grid, st, a);
    else sat::launch<bf16_t>(d->pass, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
