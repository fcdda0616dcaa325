// mp_ops.hip -- the per-edge message-passing family (DGL's edge_softmax and its generalized SpMM / SDDMM operators): the six passes of
// dgll_amd/ops_mp.py behind ONE entry point, dgll_hip_mp_pass (include/dgll_hip.h: dgll_mp_desc).
//
//   EDGE_SOFTMAX      e_out[s, h] = exp(e[s, h] - m_ih) / l_ih over the entries of row i        (per-edge in, per-edge out)
//   EDGE_SOFTMAX_BWD  e_out[s, h] = alpha (g - sum_row alpha g)          e = alpha, e2 = g      (per-edge in, per-edge out)
//   E_SUM             out[i, h] = sum_k e[s(k), h]                                              (per-edge in, per-row out)
//   U_ADD_V           e_out[s, h] = x[col_k, h] + y[i, h]                                       (per-row in, per-edge out)
//   U_MUL_E_SUM       out[i, h, :] = sum_k e[s(k), h] x[col_k, h, :]                            (node matrix gathered, weighted per entry)
//   U_DOT_V           e_out[s, h] = <x[col_k, h, :], y[i, h, :]>                                (two node matrices, per-edge out)
//
// Entry k of the pass's CSR addresses the per-edge arrays at slot s(k) = perm ? perm[k] : k: with perm a pass runs over A^T while the
// per-edge data stays in A's entry order.  The family is closed under differentiation (ops_mp.py has the table): every backward is
// another of these six over A or over A^T.  No atomics, nothing allocated or read back, fp32 accumulation.  The slot and the column
// used for addressing are clamped: a corrupt index reads or writes a wrong entry, never outside the arrays.
//
// Two lane layouts:
//  * node-matrix passes (U_MUL_E_SUM, U_DOT_V): the row-tile kernels of row_tiles.hpp exactly as sparse_attn.hip uses it -- a lane owns
//    one 16-byte vector of one head, hpb whole heads of lph lanes share a row's lanes, column blocks of whole heads over blockIdx.y;
//    the slot is read and handed round with the index batch and the (entry, head) weight is loaded next to the gathered row, so both
//    are in flight together.  U_DOT_V is the per-head form of typed_spmm.hip's edge-dots pass: lane 0 of a head stores the dot.
//  * per-edge passes: the same tiles with kEdgeLanes lanes per row and a lane per ENTRY -- lane t of a batch owns entry k0 + t and
//    sweeps its heads in register blocks of HB (any heads >= 1: the last block is masked), by 16-byte vectors of four heads where
//    heads % 4 == 0 and the arrays are aligned so, by scalars otherwise.  Without perm the group's loads cover one contiguous span of
//    kEdgeLanes * heads floats.  A row is swept twice per block of heads (reduce, then write): the second sweep
//    re-reads what the first left in cache instead of holding a row of any length in registers.  Rows longer than DGLL_MP_LONG_ROW
//    are taken by the whole workgroup, the lane groups' partial maxima and sums combined through LDS in group order by every thread.
//    kEdgeLanes = 16 follows from reading the hardware notes, not from a measurement: with 8 heads a batch is 512 contiguous bytes
//    (four 128-byte requests) and a wavefront keeps four rows in flight, which suits mean degrees of tens (products ~50).  The
//    choice itself is UNMEASURED: tools/mp_bench.py has timed this one width, 8, 32 and 64 have not been tried.
#include "row_tiles.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace mp {

constexpr int kLongRow = DGLL_MP_LONG_ROW;  // rows longer than this are swept by a whole workgroup
constexpr int kEdgeLanes = 16;              // lanes of a row in the per-edge passes (see above: not compared with other widths)
constexpr int kEdgeGroups = kBlock / kEdgeLanes;
constexpr int kHeadBlock = 8;               // heads a lane holds in registers at the most
using rt::kLog2e;

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;
    int64_t n_rows, n_cols, nnz, tiles;
    const float* e;   int64_t ld_e;
    const float* e2;  int64_t ld_e2;
    float* e_out;     int64_t ld_eo;
    const char* x;    int64_t pb_x;         // node matrices: pitches in BYTES (the per-edge passes: fp32, so 4 * ld)
    const char* y;    int64_t pb_y;
    char* out;        int64_t pb_out;
    int heads, D, vph, lph, hpb, lpr;
};

// slot of entry k in the per-edge arrays, clamped to [0, nnz)
__device__ __forceinline__ int64_t slot_of(const Args& a, int64_t k) {
    if (!a.perm) return k;
    const int64_t s = a.perm[k];
    return s < 0 ? 0 : (s >= a.nnz ? a.nnz - 1 : s);
}

// ---- per-edge passes: KIND is the pass (DGLL_MP_EDGE_SOFTMAX .. DGLL_MP_U_ADD_V), HB the heads of a register block ----------------
// VEC: heads % 4 == 0 and every per-edge and per-row array 16-byte aligned on a pitch of whole vectors -- a lane moves its heads four
// at a time (a group of four heads exists whole or not at all).  The arithmetic per element is the same: the two forms give the same bits.
template <int KIND, int HB, bool VEC>
__global__ __launch_bounds__(kBlock) void mp_edge_kernel(const Args a) {
    static_assert(!VEC || HB % 4 == 0, "vector form: register blocks of whole 16-byte vectors");
    using V4 = VecIO<float, 4>;
    constexpr bool SOFTMAX = KIND == DGLL_MP_EDGE_SOFTMAX, REDUCES = KIND != DGLL_MP_U_ADD_V, WRITES = KIND != DGLL_MP_E_SUM;
    __shared__ float lds[2 * HB * kEdgeGroups];
    const rt::Lanes lanes(kEdgeLanes);
    const int heads = a.heads, sub = lanes.sub;
    const float* xf = reinterpret_cast<const float*>(a.x);
    const float* yf = reinterpret_cast<const float*>(a.y);
    float* of = reinterpret_cast<float*>(a.out);
    const int64_t ld_x = a.pb_x / 4, ld_y = a.pb_y / 4, ld_out = a.pb_out / 4;

    int h0 = 0;                             // first head of the current block
    int64_t cur_row = 0;
    float s0[HB], s1[HB];                   // per head: softmax {row max, row sum}; backward and E_SUM {row sum, -}

    // the block's heads of row r of an array [*, ld]; heads past the last read as 0 and are not stored
    auto load_heads = [&](const float* p, int64_t ld, int64_t r, float (&v)[HB]) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < HB; j += 4) {
                typename V4::raw_t raw = V4::zero();
                if (h0 + j < heads) raw = V4::load(p + r * ld + h0 + j);
                float f[4];
                V4::unpack(raw, f);
#pragma unroll
                for (int t = 0; t < 4; ++t) v[j + t] = f[t];
            }
        } else {
#pragma unroll
            for (int j = 0; j < HB; ++j) v[j] = h0 + j < heads ? p[r * ld + h0 + j] : 0.0f;
        }
    };
    auto store_heads = [&](float* p, int64_t ld, int64_t r, const float (&v)[HB]) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < HB; j += 4) {
                const float f[4] = {v[j], v[j + 1], v[j + 2], v[j + 3]};
                if (h0 + j < heads) V4::store(p + r * ld + h0 + j, f);
            }
        } else {
#pragma unroll
            for (int j = 0; j < HB; ++j)
                if (h0 + j < heads) p[r * ld + h0 + j] = v[j];
        }
    };

    auto reset = [&] {
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            s0[j] = SOFTMAX ? -INFINITY : 0.0f;
            s1[j] = 0.0f;
        }
    };
    // first sweep: this lane's entry of the batch into the lane's partial state
    auto accumulate = [&](int64_t k0, int nb) {
        if (sub >= nb) return;
        const int64_t s = slot_of(a, k0 + sub);
        float v[HB], g[HB];
        load_heads(a.e, a.ld_e, s, v);
        if constexpr (KIND == DGLL_MP_EDGE_SOFTMAX_BWD) load_heads(a.e2, a.ld_e2, s, g);
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            if constexpr (SOFTMAX) {        // online: an entry of -inf adds nothing; a state still at -inf rescales a sum of 0
                const float m = s0[j], mn = fmaxf(m, v[j]);
                const float sc = m == mn ? 1.0f : __builtin_amdgcn_exp2f((m - mn) * kLog2e);
                const float w = v[j] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f((v[j] - mn) * kLog2e);
                s0[j] = mn;
                s1[j] = fmaf(s1[j], sc, w);
            } else if constexpr (KIND == DGLL_MP_EDGE_SOFTMAX_BWD) {
                s0[j] = fmaf(v[j], g[j], s0[j]);
            } else {
                s0[j] += v[j];
            }
        }
    };
    // the lane group's partials into every lane of the group: the max is exact and the sums are butterflies of commutative adds,
    // so all lanes end with the same bits
    auto group_reduce = [&] {
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            if constexpr (SOFTMAX) {
                float m = s0[j];
                for (int off = 1; off < kEdgeLanes; off <<= 1) m = fmaxf(m, __shfl_xor(m, off));
                float l = s0[j] == m ? s1[j] : s1[j] * __builtin_amdgcn_exp2f((s0[j] - m) * kLog2e);
                for (int off = 1; off < kEdgeLanes; off <<= 1) l += __shfl_xor(l, off);
                s0[j] = m;
                s1[j] = l;
            } else {
                float t = s0[j];
                for (int off = 1; off < kEdgeLanes; off <<= 1) t += __shfl_xor(t, off);
                s0[j] = t;
            }
        }
    };
    // a long row: the groups' partials through LDS, combined in group order by every thread (all end with the same bits)
    auto block_reduce = [&] {
        __syncthreads();                    // the previous row has read its partials
        if (sub == 0) {
#pragma unroll
            for (int j = 0; j < HB; ++j) {
                lds[(lanes.gid * HB + j) * 2] = s0[j];
                lds[(lanes.gid * HB + j) * 2 + 1] = s1[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            if constexpr (SOFTMAX) {
                float m = -INFINITY, l = 0.0f;
#pragma unroll 1
                for (int p = 0; p < kEdgeGroups; ++p) m = fmaxf(m, lds[(p * HB + j) * 2]);
#pragma unroll 1
                for (int p = 0; p < kEdgeGroups; ++p) {
                    const float mp = lds[(p * HB + j) * 2], lp = lds[(p * HB + j) * 2 + 1];
                    l += mp == m ? lp : lp * __builtin_amdgcn_exp2f((mp - m) * kLog2e);
                }
                s0[j] = m;
                s1[j] = l;
            } else {
                float t = 0.0f;
#pragma unroll 1
                for (int p = 0; p < kEdgeGroups; ++p) t += lds[(p * HB + j) * 2];
                s0[j] = t;
            }
        }
    };
    // second sweep: this lane's entry of the batch from the row's complete state
    auto emit = [&](int64_t k0, int nb) {
        if (sub >= nb) return;
        const int64_t s = slot_of(a, k0 + sub);
        int64_t c = 0;
        if constexpr (KIND == DGLL_MP_U_ADD_V) {
            if (xf) c = rt::clamp_index(a.col[k0 + sub], (int)a.n_cols);
        }
        float v[HB], g[HB], r[HB];
        if constexpr (KIND == DGLL_MP_U_ADD_V) {
#pragma unroll
            for (int j = 0; j < HB; ++j) v[j] = g[j] = 0.0f;
            if (xf) load_heads(xf, ld_x, c, v);
            if (yf) load_heads(yf, ld_y, cur_row, g);
        } else {
            load_heads(a.e, a.ld_e, s, v);
            if constexpr (KIND == DGLL_MP_EDGE_SOFTMAX_BWD) load_heads(a.e2, a.ld_e2, s, g);
        }
#pragma unroll
        for (int j = 0; j < HB; ++j) {
            if constexpr (SOFTMAX) {        // a row of -inf alone (sum 0), like an entry of -inf: 0, never NaN
                const float inv = s1[j] > 0.0f ? 1.0f / s1[j] : 0.0f;
                r[j] = v[j] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f((v[j] - s0[j]) * kLog2e) * inv;
            } else if constexpr (KIND == DGLL_MP_EDGE_SOFTMAX_BWD) {
                r[j] = v[j] * (g[j] - s0[j]);
            } else {
                r[j] = v[j] + g[j];
            }
        }
        store_heads(a.e_out, a.ld_eo, s, r);
    };
    // E_SUM: lane j of the group stores head h0 + j
    auto store_sums = [&](int64_t row) {
#pragma unroll
        for (int j = 0; j < HB; ++j)
            if (sub == j && h0 + j < heads) of[row * ld_out + h0 + j] = s0[j];
    };

    auto short_row = [&](int64_t row, bool mine, int64_t b, int64_t e) {
        cur_row = row;
        for (h0 = 0; h0 < heads; h0 += HB) {
            if constexpr (REDUCES) {
                reset();
                rt::for_each_batch(b, e, 0, 1, lanes, accumulate);
                group_reduce();
            }
            if constexpr (WRITES) rt::for_each_batch(b, e, 0, 1, lanes, emit);
            else if (mine) store_sums(row);                 // an empty row: zeros
        }
    };
    auto long_row = [&](int64_t row, int64_t b, int64_t e) {
        cur_row = row;
        for (h0 = 0; h0 < heads; h0 += HB) {
            if constexpr (REDUCES) {
                reset();
                rt::for_each_batch(b, e, lanes.gid, lanes.groups, lanes, accumulate);
                group_reduce();
                block_reduce();
            }
            if constexpr (WRITES) rt::for_each_batch(b, e, lanes.gid, lanes.groups, lanes, emit);
            else if (lanes.gid == 0) store_sums(row);
        }
    };
    rt::for_each_tile(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, short_row, long_row);
}

// ---- node-matrix passes: KIND 0 U_MUL_E_SUM, 1 U_DOT_V ---------------------------------------------------------------------------
// State of one lane (its EPV columns of one head of one row): KIND 0 the accumulator, KIND 1 the held row y_i.
template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void mp_node_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float lds[KIND == 0 ? EPV * kBlock : 1];

    const rt::Lanes lanes(a.lpr);
    const int hl = lanes.sub / a.lph, v = lanes.sub - hl * a.lph;
    const int head = (int)blockIdx.y * a.hpb + hl;
    const bool active = hl < a.hpb && head < a.heads && v < a.vph;
    const int hx = active ? head : 0;
    const int64_t cb = active ? ((int64_t)head * a.D + (int64_t)v * EPV) * (int64_t)sizeof(T) : 0;   // byte offset of the lane's columns

    float st[EPV];

    auto load_row = [&](int64_t row, int64_t, int64_t, bool on) {
        typename IO::raw_t r = IO::zero();
        if constexpr (KIND == 1) {
            if (on && active) r = IO::load(reinterpret_cast<const T*>(a.y + row * a.pb_y + cb));
        }
        IO::unpack(r, st);
    };

    // one batch of the row's entries, two entries in flight; the slot travels with the column
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        int my_slot = 0;
        if (lanes.sub < nb) my_slot = (int)slot_of(a, k0 + lanes.sub);
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t r[U];
            float w[U];
            int64_t s[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t c = rt::hand_round(my_col, t + u, lanes);
                s[u] = rt::hand_round(my_slot, t + u, lanes);
                ok[u] = t + u < nb;
                r[u] = IO::zero();
                w[u] = 0.0f;
                if (ok[u] && active) {
                    r[u] = IO::load(reinterpret_cast<const T*>(a.x + c * a.pb_x + cb));
                    if constexpr (KIND == 0) w[u] = a.e[s[u] * a.ld_e + hx];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(r[u], f);
                if constexpr (KIND == 0) {          // a masked slot loaded zeros with weight 0: it adds nothing
#pragma unroll
                    for (int d = 0; d < EPV; ++d) st[d] = fmaf(w[u], f[d], st[d]);
                } else {
                    float p = 0.0f;
#pragma unroll
                    for (int d = 0; d < EPV; ++d) p = fmaf(st[d], f[d], p);
                    p = head_sum(p, a.lph);
                    if (ok[u] && active && v == 0) a.e_out[s[u] * a.ld_eo + head] = p;
                }
            }
        }
    };

    // the row's output from its complete state; no cross-lane traffic (the long-row path calls it from one lane group alone)
    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), st);      // an empty row: zeros
    };

    if constexpr (KIND == 0) {
        rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, st, lds, load_row, batch, finish);
    } else {
        // dots: every entry is already stored.  rt::sweep_rows written out: through the header one instruction of this kernel moves
        // (a refactor does not change instruction text).
        auto short_row = [&](int64_t row, bool mine, int64_t b, int64_t e) {
            load_row(row, b, e, mine);
            rt::for_each_batch(b, e, 0, 1, lanes, batch);
        };
        auto long_row = [&](int64_t row, int64_t b, int64_t e) {
            load_row(row, b, e, true);
            rt::for_each_batch(b, e, lanes.gid, lanes.groups, lanes, batch);
        };
        rt::for_each_tile(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, short_row, long_row);
    }
}

template <int KIND>
void launch_edge(int hb, bool vec, dim3 grid, hipStream_t s, const Args& a) {
    if (hb == 1) hipLaunchKernelGGL((mp_edge_kernel<KIND, 1, false>), grid, dim3(kBlock), 0, s, a);
    else if (hb == 2) hipLaunchKernelGGL((mp_edge_kernel<KIND, 2, false>), grid, dim3(kBlock), 0, s, a);
    else if (hb == 4 && vec) hipLaunchKernelGGL((mp_edge_kernel<KIND, 4, true>), grid, dim3(kBlock), 0, s, a);
    else if (hb == 4) hipLaunchKernelGGL((mp_edge_kernel<KIND, 4, false>), grid, dim3(kBlock), 0, s, a);
    else if (vec) hipLaunchKernelGGL((mp_edge_kernel<KIND, kHeadBlock, true>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((mp_edge_kernel<KIND, kHeadBlock, false>), grid, dim3(kBlock), 0, s, a);
}

template <typename T>
void launch_node(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_MP_U_MUL_E_SUM) hipLaunchKernelGGL((mp_node_kernel<T, 0>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((mp_node_kernel<T, 1>), grid, dim3(kBlock), 0, s, a);
}

}  // namespace mp
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_mp_pass(void* stream, const dgll_mp_desc* d) {
    static const char* const kPass = "dgll_hip_mp_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_mp_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass >= DGLL_MP_EDGE_SOFTMAX && d->pass <= DGLL_MP_U_DOT_V,
                 "dgll_hip_mp_pass: pass must be one of DGLL_MP_EDGE_SOFTMAX .. DGLL_MP_U_DOT_V");
    const bool node = d->pass == DGLL_MP_U_MUL_E_SUM || d->pass == DGLL_MP_U_DOT_V;
    DGLL_REQUIRE(d->nnz >= 0 && d->nnz < (1ll << 31), "dgll_hip_mp_pass: nnz in [0, 2^31)");
    const auto edge_array = [&](const float* p, int64_t ld) { return p != nullptr && ld >= d->heads; };

    mp::Args a;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.perm = d->perm;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.nnz = d->nnz;
    a.e = d->e;          a.ld_e = d->ld_e;
    a.e2 = d->e2;        a.ld_e2 = d->ld_e2;
    a.e_out = d->e_out;  a.ld_eo = d->ld_e_out;
    a.heads = d->heads;
    a.D = d->D;
    hipStream_t st = static_cast<hipStream_t>(stream);

    if (node) {
        if (const int rc = rt::require_head_pass(d->dtype, d->heads, d->D, d->n_rows, d->n_cols, d->rowptr, d->col)) return rc;
        const auto [epv, esz] = rt::storage_of(d->dtype);
        DGLL_REQUIRE_OPERAND(kPass, x, d->heads * d->D);
        if (d->pass == DGLL_MP_U_MUL_E_SUM) {
            DGLL_REQUIRE(edge_array(d->e, d->ld_e), "dgll_hip_mp_pass: u_mul_e_sum: e non-NULL with a pitch >= heads");
            DGLL_REQUIRE_OPERAND(kPass, out, d->heads * d->D);
        } else {
            DGLL_REQUIRE_OPERAND(kPass, y, d->heads * d->D);
            DGLL_REQUIRE(edge_array(d->e_out, d->ld_e_out), "dgll_hip_mp_pass: u_dot_v: e_out non-NULL with a pitch >= heads");
        }
        a.x = static_cast<const char*>(d->x);      a.pb_x = d->ld_x * esz;
        a.y = static_cast<const char*>(d->y);      a.pb_y = d->ld_y * esz;
        a.out = static_cast<char*>(d->out);        a.pb_out = d->ld_out * esz;
        const rt::HeadGeometry geo = rt::make_head_geometry(d->heads, d->D, epv, d->n_rows);
        rt::set_geometry(a, geo);
        if (geo.grid == 0 || (d->nnz == 0 && d->pass == DGLL_MP_U_DOT_V)) return DGLL_OK;
        dim3 grid;
        if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, 1, grid)) return rc;
        if (d->dtype == DGLL_F32) mp::launch_node<float>(d->pass, grid, st, a);
        else mp::launch_node<bf16_t>(d->pass, grid, st, a);
        DGLL_HIP_TRY(hipGetLastError());
        return DGLL_OK;
    }

    DGLL_REQUIRE(d->dtype == DGLL_F32 || d->dtype == DGLL_BF16, "dgll_hip_mp_pass: dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(d->heads >= 1 && d->heads < (1 << 20), "dgll_hip_mp_pass: 1 <= heads < 2^20");
    DGLL_REQUIRE(d->n_rows >= 0 && d->n_rows < (1ll << 31) && d->n_cols > 0 && d->n_cols < (1ll << 31),
                 "dgll_hip_mp_pass: row count in [0, 2^31), gathered row count in [1, 2^31)");
    DGLL_REQUIRE(d->rowptr != nullptr, "dgll_hip_mp_pass: rowptr must be non-NULL");
    a.x = a.y = nullptr;
    a.out = nullptr;
    a.pb_x = a.pb_y = a.pb_out = 0;
    if (d->pass == DGLL_MP_E_SUM || d->pass == DGLL_MP_U_ADD_V)
        DGLL_REQUIRE(d->dtype == DGLL_F32, "dgll_hip_mp_pass: e_sum and u_add_v take fp32 per-row arrays: dtype must be DGLL_F32");
    if (d->pass == DGLL_MP_U_ADD_V) {
        DGLL_REQUIRE(edge_array(d->e_out, d->ld_e_out), "dgll_hip_mp_pass: u_add_v: e_out non-NULL with a pitch >= heads");
        DGLL_REQUIRE((!d->x || (d->col && d->ld_x >= d->heads)) && (!d->y || d->ld_y >= d->heads),
                     "dgll_hip_mp_pass: u_add_v: x (with col) and y, where given, on a pitch >= heads");
        a.x = static_cast<const char*>(d->x);      a.pb_x = d->ld_x * 4;
        a.y = static_cast<const char*>(d->y);      a.pb_y = d->ld_y * 4;
    } else {
        DGLL_REQUIRE(edge_array(d->e, d->ld_e), "dgll_hip_mp_pass: e non-NULL with a pitch >= heads");
        if (d->pass == DGLL_MP_EDGE_SOFTMAX_BWD)
            DGLL_REQUIRE(edge_array(d->e2, d->ld_e2), "dgll_hip_mp_pass: edge_softmax_bwd: e2 (the gradient) non-NULL with a pitch >= heads");
        if (d->pass == DGLL_MP_E_SUM) {
            DGLL_REQUIRE(d->out != nullptr && d->ld_out >= d->heads, "dgll_hip_mp_pass: e_sum: out non-NULL with a pitch >= heads");
            a.out = static_cast<char*>(d->out);    a.pb_out = d->ld_out * 4;
        } else {
            DGLL_REQUIRE(edge_array(d->e_out, d->ld_e_out), "dgll_hip_mp_pass: edge_softmax: e_out non-NULL with a pitch >= heads");
        }
    }
    const rt::HeadGeometry geo = rt::make_row_geometry(mp::kEdgeLanes, d->n_rows);      // (no heads in the lanes: vph = lph = hpb = 0)
    rt::set_geometry(a, geo);
    if (geo.grid == 0 || (d->nnz == 0 && d->pass != DGLL_MP_E_SUM)) return DGLL_OK;
    int hb = 1;
    while (hb < mp::kHeadBlock && hb < d->heads) hb <<= 1;
    // the vector form: every array the pass touches four heads at a time on 16-byte boundaries (E_SUM's per-row output is stored by scalars)
    const auto vec_ok = [](const void* p, int64_t ld) { return p == nullptr || (aligned16(p) && ld % 4 == 0); };
    const bool vec = d->heads % 4 == 0 && vec_ok(a.e, a.ld_e) && vec_ok(a.e2, a.ld_e2) && vec_ok(a.e_out, a.ld_eo) &&
                     vec_ok(a.x, d->ld_x) && vec_ok(a.y, d->ld_y);
    const dim3 grid((unsigned)geo.grid);
    if (d->pass == DGLL_MP_EDGE_SOFTMAX) mp::launch_edge<DGLL_MP_EDGE_SOFTMAX>(hb, vec, grid, st, a);
    else if (d->pass == DGLL_MP_EDGE_SOFTMAX_BWD) mp::launch_edge<DGLL_MP_EDGE_SOFTMAX_BWD>(hb, vec, grid, st, a);
    else if (d->pass == DGLL_MP_E_SUM) mp::launch_edge<DGLL_MP_E_SUM>(hb, vec, grid, st, a);
    else mp::launch_edge<DGLL_MP_U_ADD_V>(hb, vec, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
