// edge.hip -- per-edge kernels of the GAT / SpecialSpmm path for gfx950: SDDMM, fused edge-softmax + SpMM
// (forward), its two backward gather passes, and the max-reduce of the SAGE aggregator.
//
// Reference semantics (all under /root/reference/dgll/nn/Convolution/):
//   sparseGatConv.forward  gatconv.py:111-148   e_ij = exp(-leakyrelu(a1.h_i + a2.h_j)); out_i = sum_j e_ij h_j / sum_j e_ij; elu
//   gatConv.forward        gatconv.py:30-54     att = softmax_j(+leakyrelu(.)) over the adjacency's nonzeros; out = att.Wh; elu
//   SpecialSpmmFunction    gatconv.py:60-81     backward: grad_values[e] = <g[row_e,:], b[col_e,:]>  (SDDMM), grad_b = A^T.g
//   SpGAT / GAT            gatconv.py:154-199   `nheads` independent heads, concatenated (one python call per head)
// Here all heads of a layer run in ONE launch: H is [N, heads*fo] (fo = per-head width, padded by the host to a
// power-of-two number of 16-byte vectors), S[i,k] = a1_k.h_i^k and T[j,k] = a2_k.h_j^k are [N, heads] fp32.
//
// Same skeleton as spmm.hip: one wavefront per row, LPR lanes x 16 bytes per gathered feature row, 64/LPR
// neighbour slots, U gathers in flight per lane, a coalesced 64-edge index batch handed out with ds_bpermute,
// fp32 accumulation, no atomics (fixed reduction order, bit-reproducible).  Nothing per-edge is ever stored:
// the backward passes recompute e_ij from S and T.
#include <algorithm>

#include "common.hpp"
#include "edge_args.hpp"
#include "gat_choice.hpp"

namespace dgll {

// ------------------------------------------------------------------------------------------------ SDDMM
// edge_out[k] = sum_f G[row(k), f] * H[col[k], f]            (gatconv.py:76-78)
template <typename XT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void sddmm_kernel(const EdgeArgs a) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = sub * EPV;
    const bool col_ok = c0 < a.feat;
    const int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (row >= a.n_rows) return;
    const int64_t b = uniform64(a.rowptr[row]), e = uniform64(a.rowptr[row + 1]);
    float g[EPV];
    {
        typename IO::raw_t r = col_ok ? IO::load(static_cast<const XT*>(a.G) + row * a.ldg + c0) : IO::zero();
        IO::unpack(r, g);
    }
    const XT* hcol = static_cast<const XT*>(a.H) + (col_ok ? c0 : 0);
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t k0) {
        for (int j = 0; j < nb; j += SLOTS * U) {
            int idx[U];
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = j + u * SLOTS + slot;
                const int c = __shfl(cur_col, idx[u] < nb ? idx[u] : nb - 1);
                v[u] = IO::load(hcol + (uint64_t)(uint32_t)c * (uint32_t)a.ldh);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(v[u], f);
                float d = 0.0f;
#pragma unroll
                for (int i = 0; i < EPV; ++i) d = fmaf(g[i], f[i], d);
                d = head_sum(d, LPR);
                if (sub == 0 && idx[u] < nb) a.edge_out[k0 + idx[u]] = d;
            }
        }
    });
}

// ------------------------------------------------------------------------------------------------ GAT forward
// out[i, head cols] = act( sum_j w_ij * scale_ij * H[j, cols] / sum_j w_ij ),  w_ij = exp(sign*lrelu(S[i]+T[j]) - M[i])
template <typename XT, typename YT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(const EdgeArgs a, int lph) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = ((int)blockIdx.y * LPR + sub) * EPV;
    const bool col_ok = c0 < a.feat;
    const int head = col_ok ? c0 / a.fo : 0;
  for (int r = 0; r < a.rows_per_wave; ++r) {   // several consecutive rows per wavefront (amortises wave start-up)
    const WorkItem it = resolve_item(a, wave, r);
    if (it.done) return;
    if (!it.valid) continue;
    const int64_t row = it.row, b = it.b, e = it.e;
    const float s_i = a.S[row * a.heads + head];
    const XT* hcol = static_cast<const XT*>(a.H) + (col_ok ? c0 : 0);

    float m_i = 0.0f;
    if (a.use_max) {  // gatConv semantics: subtract the row maximum of the scores (softmax), gatconv.py:36
        float mx = -INFINITY;
        for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t) {
            for (int j = 0; j < nb; j += SLOTS) {  // uniform trip count: every lane takes part in the shuffle
                const int idx = j + slot;
                const int c = __shfl(cur_col, idx < nb ? idx : nb - 1);
                mx = fmaxf(mx, a.sign * lrelu(s_i + a.T[(int64_t)c * a.heads + head], a.alpha));
            }
        });
        m_i = slot_max<LPR>(mx);
    }

    float acc[EPV];
#pragma unroll
    for (int i = 0; i < EPV; ++i) acc[i] = 0.0f;
    float den = 0.0f;
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t k0) {
        for (int j = 0; j < nb; j += SLOTS * U) {
            bool ok[U];
            int idx[U];
            float t[U], sc[U];
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = j + u * SLOTS + slot;
                ok[u] = idx[u] < nb;
                if (!ok[u]) idx[u] = nb - 1;
                const int c = __shfl(cur_col, idx[u]);
                t[u] = a.T[(int64_t)c * a.heads + head];
                sc[u] = a.edge_scale ? a.edge_scale[(k0 + idx[u]) * a.heads + head] : 1.0f;
                v[u] = IO::load(hcol + (uint64_t)(uint32_t)c * (uint32_t)a.ldh);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float w = __expf(a.sign * lrelu(s_i + t[u], a.alpha) - m_i);
                w = ok[u] ? w : 0.0f;
                den += w;
                const float wn = w * sc[u];
                float f[EPV];
                IO::unpack(ok[u] ? v[u] : IO::zero(), f);
#pragma unroll
                for (int i = 0; i < EPV; ++i) acc[i] = fmaf(wn, f[i], acc[i]);
            }
        }
    });
#pragma unroll
    for (int i = 0; i < EPV; ++i) acc[i] = slot_sum<LPR>(acc[i]);
    den = slot_sum<LPR>(den);
    if (it.chunk >= 0) {  // partial of a long row: (acc, den, local max) -> workspace, combined by gat_long_finalize_kernel
        if (slot == 0 && col_ok) {
            float* w = a.ws + it.chunk * a.ws_ld;
#pragma unroll
            for (int i = 0; i < EPV; ++i) w[c0 + i] = acc[i];
            if ((sub % lph) == 0) {
                w[a.ws_vec + head] = den;
                w[a.ws_vec + a.heads + head] = m_i;
            }
        }
        return;
    }
    if (slot == 0 && col_ok) {
        YT* yrow = static_cast<YT*>(a.Y) + row * a.ldy + c0;
        if (a.accumulate) {   // second half of a split adjacency: the first launch left (num, den) of the other columns here
            den += a.out_a[row * a.heads + head];
#pragma unroll
            for (int i = 0; i < EPV; ++i) acc[i] += load_scalar<YT>(yrow + i);
        }
        if (!a.raw) {
            const float inv = 1.0f / den;  // 0/0 -> NaN for edgeless rows, as gatconv.py:139
#pragma unroll
            for (int i = 0; i < EPV; ++i) {
                float v = acc[i] * inv;
                if (a.apply_elu) v = v > 0.0f ? v : expm1f(v);
                acc[i] = v;
            }
        }
        VecIO<YT, EPV>::store(yrow, acc);
    }
    // the per-(row, head) scalars are written after every lane has read the previous launch's denominator
    __builtin_amdgcn_wave_barrier();
    if (slot == 0 && col_ok && (sub % lph) == 0) {
        a.out_a[row * a.heads + head] = den;
        if (a.out_b) a.out_b[row * a.heads + head] = m_i;
    }
  }
}

// ------------------------------------------------------------------------------------------------ GAT backward, pass 1 (rows of A)
// Per row i:  dhp = g * elu'(hp);  DN[i,:] = dhp / den_i;  DD[i,k] = -sum_{f in k} dhp*hp / den_i;
//             ds[i,k] = sum_j dz_ij,   dz_ij = (scale_ij * <DN_i, h_j>_k + DD[i,k]) * w_ij * sign * lrelu'(S_i+T_j)
template <typename XT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void gat_bwd_rows_kernel(const EdgeArgs a, int lph) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = ((int)blockIdx.y * LPR + sub) * EPV;
    const bool col_ok = c0 < a.feat;
    const int head = col_ok ? c0 / a.fo : 0;
  for (int r = 0; r < a.rows_per_wave; ++r) {   // several consecutive rows per wavefront (amortises wave start-up)
    const WorkItem it = resolve_item(a, wave, r);
    if (it.done) return;
    if (!it.valid) continue;
    const int64_t row = it.row, b = it.b, e = it.e;
    const float s_i = a.S[row * a.heads + head];
    const float m_i = a.M ? a.M[row * a.heads + head] : 0.0f;
    const float inv_den = 1.0f / a.DEN[row * a.heads + head];

    float dn[EPV];
    float dd;
    {
        float g[EPV], o[EPV];
        IO::unpack(col_ok ? IO::load(static_cast<const XT*>(a.G) + row * a.ldg + c0) : IO::zero(), g);
        IO::unpack(col_ok ? IO::load(static_cast<const XT*>(a.O) + row * a.ldo + c0) : IO::zero(), o);
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < EPV; ++i) {
            float dhp = g[i], hp = o[i];
            if (a.apply_elu && o[i] <= 0.0f) {  // out = expm1(hp): elu'(hp) = out + 1, hp = log1p(out)
                const float op1 = o[i] + 1.0f;    // saturated ELU (out == -1): gradient 0, and 0 * log(0) must stay 0
                dhp = g[i] * op1;
                hp = op1 > 0.0f ? log1pf(o[i]) : 0.0f;
            }
            dn[i] = dhp * inv_den;
            // bf16: dd_i = -DN_i . hp_i from the ROUNDED DN_i the dot products (and the transposed pass) use -- see gat_kernel.hpp
            if (sizeof(XT) == 2) dn[i] = bf16_to_f32(f32_to_bf16(dn[i]));
            part = fmaf(dn[i], hp, part);
        }
        dd = -head_sum(part, lph);
        if (slot == 0 && col_ok && it.first && !a.accumulate) {   // per-row outputs: written once (row itself / first chunk, first launch)
            VecIO<XT, EPV>::store(static_cast<XT*>(a.Y) + row * a.ldy + c0, dn);
            if ((sub % lph) == 0) a.out_b[row * a.heads + head] = dd;
        }
    }
    uint32_t dnp[4] = {0u, 0u, 0u, 0u};   // DN_i as packed bf16 pairs for the dot2 path (exact: dn was rounded above)
    if constexpr (sizeof(XT) == 2) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dnp[q] = pack_bf16x2(dn[2 * q], dn[2 * q + 1]);
    }

    const XT* hcol = static_cast<const XT*>(a.H) + (col_ok ? c0 : 0);
    float ds = 0.0f;
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t k0) {
        for (int j = 0; j < nb; j += SLOTS * U) {
            bool ok[U];
            int idx[U];
            float t[U], sc[U];
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = j + u * SLOTS + slot;
                ok[u] = idx[u] < nb;
                if (!ok[u]) idx[u] = nb - 1;
                const int c = __shfl(cur_col, idx[u]);
                t[u] = a.T[(int64_t)c * a.heads + head];
                sc[u] = a.edge_scale ? a.edge_scale[(k0 + idx[u]) * a.heads + head] : 1.0f;
                v[u] = IO::load(hcol + (uint64_t)(uint32_t)c * (uint32_t)a.ldh);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float dot = 0.0f;
                if constexpr (sizeof(XT) == 2) {   // bf16: <DN_i, h_j> straight on the packed pairs (v_dot2c_f32_bf16, fp32 accumulate):
                    const uint32_t hv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};   // 4 instructions instead of 8 unpacks + 8 FMAs
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        dot = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, dnp[q]), __builtin_bit_cast(bf16x2_t, hv[q]), dot, false);
                } else {
                    float f[EPV];
                    IO::unpack(v[u], f);
#pragma unroll
                    for (int i = 0; i < EPV; ++i) dot = fmaf(dn[i], f[i], dot);
                }
                dot = head_sum(dot, lph);
                const float z = s_i + t[u];
                const float w = __expf(a.sign * lrelu(z, a.alpha) - m_i);
                const float dz = (sc[u] * dot + dd) * w * a.sign * (z > 0.0f ? 1.0f : a.alpha);
                ds += ok[u] ? dz : 0.0f;
            }
        }
    });
    ds = slot_sum<LPR>(ds);
    if (slot == 0 && col_ok && (sub % lph) == 0) {
        if (it.chunk >= 0) a.ws[it.chunk * a.ws_ld + a.ws_vec + head] = ds;
        else a.out_a[row * a.heads + head] = (a.accumulate ? a.out_a[row * a.heads + head] : 0.0f) + ds;
    }
  }
}

// ------------------------------------------------------------------------------------------------ GAT backward, pass 2 (rows of A^T)
// Per source node j:  dH[j,:] = sum_i w_ij * scale_ij * DN[i,:];   dt[j,k] = sum_i dz_ij   (dz recomputed, see pass 1)
// Here rowptr/col describe A^T (rows = j, columns = i); H is DN (gathered by i); G is the node's own h_j row;
// S holds the per-node score of the ROW side of this pass (T of the forward), T the gathered side (S of the forward).
template <typename XT, typename YT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void gat_bwd_cols_kernel(const EdgeArgs a, int lph) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = ((int)blockIdx.y * LPR + sub) * EPV;
    const bool col_ok = c0 < a.feat;
    const int head = col_ok ? c0 / a.fo : 0;
  for (int r = 0; r < a.rows_per_wave; ++r) {   // several consecutive rows per wavefront (amortises wave start-up)
    const WorkItem it = resolve_item(a, wave, r);
    if (it.done) return;
    if (!it.valid) continue;
    const int64_t row = it.row, b = it.b, e = it.e;
    const float t_j = a.S[row * a.heads + head];
    float hj[EPV];
    IO::unpack(col_ok ? IO::load(static_cast<const XT*>(a.G) + row * a.ldg + c0) : IO::zero(), hj);
    const XT* dncol = static_cast<const XT*>(a.H) + (col_ok ? c0 : 0);

    float acc[EPV];
#pragma unroll
    for (int i = 0; i < EPV; ++i) acc[i] = 0.0f;
    float dt = 0.0f;
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t k0) {
        for (int j = 0; j < nb; j += SLOTS * U) {
            bool ok[U];
            int idx[U];
            float s[U], m[U], dd[U], sc[U];
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = j + u * SLOTS + slot;
                ok[u] = idx[u] < nb;
                if (!ok[u]) idx[u] = nb - 1;
                const int64_t c = __shfl(cur_col, idx[u]);
                s[u] = a.T[c * a.heads + head];
                m[u] = a.M ? a.M[c * a.heads + head] : 0.0f;
                dd[u] = a.DD[c * a.heads + head];
                sc[u] = a.edge_scale ? a.edge_scale[a.perm[k0 + idx[u]] * a.heads + head] : 1.0f;
                v[u] = IO::load(dncol + (uint64_t)(uint32_t)c * (uint32_t)a.ldh);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(ok[u] ? v[u] : IO::zero(), f);
                float dot = 0.0f;
#pragma unroll
                for (int i = 0; i < EPV; ++i) dot = fmaf(f[i], hj[i], dot);
                dot = head_sum(dot, lph);
                const float z = s[u] + t_j;
                float w = __expf(a.sign * lrelu(z, a.alpha) - m[u]);
                w = ok[u] ? w : 0.0f;
                dt += (sc[u] * dot + dd[u]) * w * a.sign * (z > 0.0f ? 1.0f : a.alpha);
                const float wn = w * sc[u];
#pragma unroll
                for (int i = 0; i < EPV; ++i) acc[i] = fmaf(wn, f[i], acc[i]);
            }
        }
    });
#pragma unroll
    for (int i = 0; i < EPV; ++i) acc[i] = slot_sum<LPR>(acc[i]);
    dt = slot_sum<LPR>(dt);
    if (slot == 0 && col_ok) {
        if (it.chunk >= 0) {
            float* w = a.ws + it.chunk * a.ws_ld;
#pragma unroll
            for (int i = 0; i < EPV; ++i) w[c0 + i] = acc[i];
            if ((sub % lph) == 0) w[a.ws_vec + head] = dt;
        } else {
            VecIO<YT, EPV>::store(static_cast<YT*>(a.Y) + row * a.ldy + c0, acc);
            if ((sub % lph) == 0) a.out_a[row * a.heads + head] = dt;
        }
    }
  }
}

// Second pass for long rows of the three GAT kernels: combine the chunk partials in chunk order.
//   kind 0 (forward): softmax-merge (local max m_c, denominator d_c, vector v_c): M = max m_c, den = sum d_c e^{m_c-M},
//                     out = act(sum v_c e^{m_c-M} / den); writes out, rowsum, rowmax
//   kind 1 (backward rows): out_a[row, head] = sum of scalar partials
//   kind 2 (backward cols): Y[row, :] = sum of vector partials, out_a[row, head] = sum of scalar partials
template <typename YT>
__global__ __launch_bounds__(kBlock) void gat_long_finalize_kernel(const EdgeArgs a, const int64_t* __restrict__ long_row,
                                                                   const int32_t* __restrict__ long_chunk0, int kind) {
    const int64_t li = blockIdx.x;
    const int64_t row = long_row[li];
    const int cb = long_chunk0[li], ce = long_chunk0[li + 1];
    // per-(row, head) scalars are written after the whole block has read the previous launch's denominators
    int my_head = -1;
    float my_den = 0.0f, my_max = 0.0f;
    for (int f = (int)threadIdx.x; f < a.feat + a.heads; f += kBlock) {
        const bool vec = f < a.feat;
        const int head = vec ? f / a.fo : f - a.feat;
        const int off = vec ? f : a.ws_vec + head;
        if (kind == 0) {
            float M = -INFINITY;
            for (int c = cb; c < ce; ++c) M = fmaxf(M, a.ws[(int64_t)c * a.ws_ld + a.ws_vec + a.heads + head]);
            float den = 0.0f, v = 0.0f;
            for (int c = cb; c < ce; ++c) {
                const float* w = a.ws + (int64_t)c * a.ws_ld;
                const float sc = __expf(w[a.ws_vec + a.heads + head] - M);
                den += w[a.ws_vec + head] * sc;
                if (vec) v += w[f] * sc;
            }
            if (a.accumulate) den += a.out_a[row * a.heads + head];
            if (vec) {
                YT* y = static_cast<YT*>(a.Y) + row * a.ldy + f;
                if (a.accumulate) v += load_scalar<YT>(y);
                float o = a.raw ? v : v / den;
                if (!a.raw && a.apply_elu) o = o > 0.0f ? o : expm1f(o);
                store_one<YT>(y, o);
            } else {
                my_head = head; my_den = den; my_max = M;
            }
        } else if (kind == 1 && a.exact_dd) {
            // rows pass, exact dd: the chunks carry (sa, sb, sw); ds_i = sa + dd_i * sb with dd_i = -sw / den_i (gat_kernel.hpp)
            if (!vec) {
                float sa = 0.0f, sb = 0.0f, sw = 0.0f;
                for (int c = cb; c < ce; ++c) {
                    const float* w = a.ws + (int64_t)c * a.ws_ld + a.ws_vec;
                    sa += w[head]; sb += w[a.heads + head]; sw += w[2 * a.heads + head];
                }
                gat_finish_scores(a, row, head, sa, sb, sw);      // finalises, or parks / adds the sums in part3 (split launches)
            }
        } else {
            float sacc = 0.0f;
            for (int c = cb; c < ce; ++c) sacc += a.ws[(int64_t)c * a.ws_ld + off];
            if (vec) {
                if (kind == 2) {
                    if (a.attn1) {      // the scores' own contribution to grad_H (see edge_args.hpp): the head's dt first
                        float dt = 0.0f;
                        for (int c = cb; c < ce; ++c) dt += a.ws[(int64_t)c * a.ws_ld + a.ws_vec + head];
                        sacc += a.gs_rows[row * a.heads + head] * a.attn1[f] + dt * a.attn2[f];
                    }
                    store_one<YT>(static_cast<YT*>(a.Y) + row * a.ldy + f, sacc);
                }
            } else {
                my_head = head;
                my_den = ((kind == 1 && a.accumulate == 1) ? a.out_a[row * a.heads + head] : 0.0f) + sacc;
            }
        }
    }
    __syncthreads();
    if (my_head >= 0 && !(kind == 1 && a.exact_dd)) {       // (the exact rows pass wrote its scalars above)
        a.out_a[row * a.heads + my_head] = my_den;
        if (kind == 0 && a.out_b) a.out_b[row * a.heads + my_head] = my_max;
    }
}

// The same second pass with ONE WAVEFRONT per long row (heads <= 64): lane k < heads merges the per-head scalars and
// broadcasts them by shuffle; every lane then combines four columns at a time with float4 reads of the chunk partials.
// Most long rows have two or three chunks, so a whole workgroup per row (above) is mostly launch overhead: 0.83 -> ~0.2 ms
// for the 8 x 32 forward on the products-shaped graph.
template <typename YT>
__global__ __launch_bounds__(kBlock) void gat_long_finalize_wave_kernel(const EdgeArgs a, const int64_t* __restrict__ long_row,
                                                                        const int32_t* __restrict__ long_chunk0, int64_t n_long,
                                                                        int kind) {
    const int lane = lane_id();
    const int64_t li = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (li >= n_long) return;
    const int64_t row = long_row[li];
    const int cb = long_chunk0[li], ce = long_chunk0[li + 1];
    // ---- per-head scalars (lane = head)
    float h_max = 0.0f, h_den = 0.0f;
    if (lane < a.heads) {
        // Chunk partials are read EIGHT AT A TIME and combined in chunk order (the sums are the sequential ones, bit for bit): a hub of
        // ten thousand edges has dozens of chunks, and one dependent load per chunk made a launch's run time the latency chain of
        // its longest row (the SpMM's finalize kernel: 45 -> 12 us per launch with the same change).
        if (kind == 0) {
            float M = -INFINITY;
            float den = 0.0f;
            for (int c = cb; c < ce; c += 8) {
                float m8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) m8[u] = a.ws[(int64_t)(c + u < ce ? c + u : ce - 1) * a.ws_ld + a.ws_vec + a.heads + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) M = fmaxf(M, m8[u]);                 // (a repeated last chunk changes no maximum)
            }
            for (int c = cb; c < ce; c += 8) {
                float d8[8], m8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float* w = a.ws + (int64_t)(c + u < ce ? c + u : ce - 1) * a.ws_ld + a.ws_vec;
                    d8[u] = w[lane]; m8[u] = w[a.heads + lane];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c + u < ce) den += d8[u] * __expf(m8[u] - M);
            }
            if (a.accumulate) den += a.out_a[row * a.heads + lane];
            h_max = M; h_den = den;
        } else if (kind == 1 && a.exact_dd) {
            float sa = 0.0f, sb = 0.0f, sw = 0.0f;
            for (int c = cb; c < ce; c += 8) {
                float a8[8], b8[8], w8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float* w = a.ws + (int64_t)(c + u < ce ? c + u : ce - 1) * a.ws_ld + a.ws_vec;
                    a8[u] = w[lane]; b8[u] = w[a.heads + lane]; w8[u] = w[2 * a.heads + lane];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c + u < ce) { sa += a8[u]; sb += b8[u]; sw += w8[u]; }
            }
            gat_finish_scores(a, row, lane, sa, sb, sw);                       // finalises, or parks / adds the sums in part3
        } else {
            float sacc = 0.0f;
            for (int c = cb; c < ce; c += 8) {
                float s8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) s8[u] = a.ws[(int64_t)(c + u < ce ? c + u : ce - 1) * a.ws_ld + a.ws_vec + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (c + u < ce) sacc += s8[u];
            }
            h_den = ((kind == 1 && a.accumulate == 1) ? a.out_a[row * a.heads + lane] : 0.0f) + sacc;
        }
    }
    // ---- vector part: four columns per lane (fo is a multiple of 4, so they share a head)
    if (kind != 1) {
        const int trips = (a.feat + kWave * 4 - 1) / (kWave * 4);
        for (int it = 0; it < trips; ++it) {
            const int f = it * kWave * 4 + lane * 4;
            const bool live = f < a.feat;
            const int head = live ? f / a.fo : 0;
            const float M = __shfl(h_max, head), den = __shfl(h_den, head);      // every lane takes part
            if (!live) continue;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int c = cb; c < ce; c += 8) {
                float4 p8[8];
                float m8[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float* w = a.ws + (int64_t)(c + u < ce ? c + u : ce - 1) * a.ws_ld;
                    p8[u] = *reinterpret_cast<const float4*>(w + f);
                    m8[u] = kind == 0 ? w[a.ws_vec + a.heads + head] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (c + u >= ce) continue;
                    const float sc = kind == 0 ? __expf(m8[u] - M) : 1.0f;
                    const float4 p = p8[u];
                    v.x = fmaf(p.x, sc, v.x); v.y = fmaf(p.y, sc, v.y); v.z = fmaf(p.z, sc, v.z); v.w = fmaf(p.w, sc, v.w);
                }
            }
            float o[4] = {v.x, v.y, v.z, v.w};
            YT* y = static_cast<YT*>(a.Y) + row * a.ldy + f;
            if (kind == 2 && a.attn1) {      // the scores' own contribution to grad_H (edge_args.hpp); `den` is the head's dt here
                const float gs = a.gs_rows[row * a.heads + head];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] += gs * a.attn1[f + i] + den * a.attn2[f + i];
            }
            if (kind == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (a.accumulate) o[i] += load_scalar<YT>(y + i);
                    if (!a.raw) {
                        o[i] = o[i] / den;
                        if (a.apply_elu) o[i] = o[i] > 0.0f ? o[i] : expm1f(o[i]);
                    }
                }
            }
            VecIO<YT, 4>::store(y, o);
        }
    }
    // per-(row, head) scalars: written after every lane has read the previous launch's denominators
    __builtin_amdgcn_wave_barrier();
    if (lane < a.heads && !(kind == 1 && a.exact_dd)) {       // (the exact rows pass wrote its scalars above)
        a.out_a[row * a.heads + lane] = h_den;
        if (kind == 0 && a.out_b) a.out_b[row * a.heads + lane] = h_max;
    }
}

// ------------------------------------------------------------------------------------------------ segment max
// Y[i,f] = max_k X[col[k], f], arg[i,f] = col of the (first) maximum; empty rows give 0 / -1.   (sageconv.py:37-38)
template <typename XT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void segment_max_kernel(const EdgeArgs a) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = ((int)blockIdx.y * LPR + sub) * EPV;
    const bool col_ok = c0 < a.feat;
    const int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (row >= a.n_rows) return;
    const int64_t b = uniform64(a.rowptr[row]), e = uniform64(a.rowptr[row + 1]);
    const XT* hcol = static_cast<const XT*>(a.H) + (col_ok ? c0 : 0);
    float best[EPV];
    int arg[EPV];
#pragma unroll
    for (int i = 0; i < EPV; ++i) { best[i] = -INFINITY; arg[i] = -1; }
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t) {
        for (int j = 0; j < nb; j += SLOTS * U) {
            bool ok[U];
            int c[U];
            typename IO::raw_t v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = j + u * SLOTS + slot;
                ok[u] = idx < nb;
                c[u] = __shfl(cur_col, ok[u] ? idx : nb - 1);
                v[u] = IO::load(hcol + (uint64_t)(uint32_t)c[u] * (uint32_t)a.ldh);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float f[EPV];
                IO::unpack(v[u], f);
#pragma unroll
                for (int i = 0; i < EPV; ++i)
                    if (ok[u] && (f[i] > best[i] || (f[i] == best[i] && c[u] < arg[i]) || arg[i] < 0)) { best[i] = f[i]; arg[i] = c[u]; }
            }
        }
    });
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
        for (int i = 0; i < EPV; ++i) {
            const float ob = __shfl_xor(best[i], off);
            const int oa = __shfl_xor(arg[i], off);
            if (oa >= 0 && (arg[i] < 0 || ob > best[i] || (ob == best[i] && oa < arg[i]))) { best[i] = ob; arg[i] = oa; }
        }
    }
    if (slot == 0 && col_ok) {
#pragma unroll
        for (int i = 0; i < EPV; ++i)
            if (arg[i] < 0) best[i] = 0.0f;
        VecIO<XT, EPV>::store(static_cast<XT*>(a.Y) + row * a.ldy + c0, best);
#pragma unroll
        for (int i = 0; i < EPV; ++i) a.arg_out[row * a.ldy + c0 + i] = arg[i];
    }
}

// ------------------------------------------------------------------------------------------------ segment max, backward
// grad[j, f] = sum over the destination rows i that list j (once per distinct i) of  (arg[i, f] == j) ? g[i, f] : 0
// -- the gradient of a max goes to the arg-max source row only (torch.max, sageconv.py:37-38).  Driven by the TRANSPOSED
// structure (row j of `rowptr/col` lists the destinations i, ascending), so every output row is produced by one
// wavefront in a fixed order: no atomics, bit-reproducible.  A pair (i, j) stored twice is counted once.
template <typename XT, int EPV, int LPR, int U>
__global__ __launch_bounds__(kBlock) void segment_max_bwd_kernel(const EdgeArgs a, const int32_t* __restrict__ arg, int64_t ldarg) {
    typedef VecIO<XT, EPV> IO;
    constexpr int SLOTS = kWave / LPR;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sub = lane % LPR, slot = lane / LPR;
    const int c0 = ((int)blockIdx.y * LPR + sub) * EPV;
    const bool col_ok = c0 < a.feat;
    const int64_t j = (int64_t)blockIdx.x * kWavesPerBlock + wave;      // source row whose gradient this wavefront writes
    if (j >= a.n_rows) return;
    const int64_t b = uniform64(a.rowptr[j]), e = uniform64(a.rowptr[j + 1]);
    const XT* gcol = static_cast<const XT*>(a.G) + (col_ok ? c0 : 0);
    const int32_t* acol = arg + (col_ok ? c0 : 0);
    float acc[EPV];
#pragma unroll
    for (int i = 0; i < EPV; ++i) acc[i] = 0.0f;
    for_each_batch(a.col, b, e, lane, [&](int nb, int cur_col, int64_t k0) {
        // a repeated (i, j) pair sits in adjacent slots of the sorted transposed row: keep the first
        int prev = __shfl_up(cur_col, 1);
        if (lane == 0) prev = k0 > b ? a.col[k0 - 1] : -1;
        const int keep = (lane < nb && cur_col != prev) ? 1 : 0;
        for (int jj = 0; jj < nb; jj += SLOTS * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = jj + u * SLOTS + slot;
                const int src = idx < nb ? idx : nb - 1;
                const int i = __shfl(cur_col, src);
                const int k = __shfl(keep, src);
                if (idx < nb && k) {
                    float f[EPV];
                    IO::unpack(IO::load(gcol + (uint64_t)(uint32_t)i * (uint32_t)a.ldg), f);
                    const int32_t* ap = acol + (int64_t)i * ldarg;
#pragma unroll
                    for (int q = 0; q < EPV; ++q)
                        if (ap[q] == (int32_t)j) acc[q] += f[q];
                }
            }
        }
    });
#pragma unroll
    for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
        for (int i = 0; i < EPV; ++i) acc[i] += __shfl_xor(acc[i], off);
    }
    if (slot == 0 && col_ok) VecIO<XT, EPV>::store(static_cast<XT*>(a.Y) + j * a.ldy + c0, acc);
}

// ---- host-side dispatch helpers --------------------------------------------------------------------------
static int pick_lpr(int vecs) {
    int lpr = 4;
    while (lpr < 64 && lpr < vecs) lpr <<= 1;
    return lpr;
}

static bool vec_ok(const void* p, int64_t ld, int esz) { return aligned16(p) && (ld * esz) % 16 == 0; }

#define DGLL_LPR_SWITCH(lpr, CALL)   \
    switch (lpr) {                   \
        case 4: { CALL(4); } break;  \
        case 8: { CALL(8); } break;  \
        case 16: { CALL(16); } break;\
        case 32: { CALL(32); } break;\
        default: { CALL(64); } break;\
    }

}  // namespace dgll

dgll::GatTune dgll::g_gat_tune;

using namespace dgll;

DGLL_API int dgll_hip_sddmm_csr(void* stream, const int64_t* rowptr, const int32_t* col, const void* G, int64_t ldg,
                                const void* B, int64_t ldb, int dtype, float* edge_out, int64_t n_rows, int feat) {
    if (n_rows <= 0) return DGLL_OK;
    DGLL_REQUIRE(rowptr && col && G && B && edge_out, "NULL argument");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype");
    const int esz = dtype == DGLL_BF16 ? 2 : 4, epv = 16 / esz;
    DGLL_REQUIRE(feat > 0 && feat <= 64 * epv, "sddmm handles up to 64 vectors per row in one launch (split columns on the host)");
    DGLL_REQUIRE(vec_ok(G, ldg, esz) && vec_ok(B, ldb, esz) && ldg >= ((feat + epv - 1) / epv) * epv && ldb >= ((feat + epv - 1) / epv) * epv,
                 "sddmm operands must be 16-byte aligned with padded leading dimensions");
    EdgeArgs a{};
    a.rowptr = rowptr; a.col = col; a.G = G; a.ldg = ldg; a.H = B; a.ldh = ldb; a.edge_out = edge_out;
    a.n_rows = n_rows; a.feat = feat;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lpr = pick_lpr((feat + epv - 1) / epv);
    dim3 grid((uint32_t)((n_rows + kWavesPerBlock - 1) / kWavesPerBlock));
#define CALL(L)                                                                                                       \
    if (dtype == DGLL_F32) hipLaunchKernelGGL((sddmm_kernel<float, 4, L, 4>), grid, dim3(kBlock), 0, s, a);           \
    else hipLaunchKernelGGL((sddmm_kernel<bf16_t, 8, L, 4>), grid, dim3(kBlock), 0, s, a);
    DGLL_LPR_SWITCH(lpr, CALL)
#undef CALL
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

static int gat_ws_vec(int heads, int fo) { return (heads * fo + 7) & ~7; }
static int gat_ws_ld(int heads, int fo) { return (gat_ws_vec(heads, fo) + 3 * heads + 7) & ~7; }   // three scalars per head (exact rows pass)

DGLL_API size_t dgll_hip_gat_workspace_bytes(const dgll_csr_plan* plan, int heads, int fo) {
    if (!plan || plan->n_chunks == 0 || heads <= 0 || fo <= 0) return 0;
    return (size_t)plan->n_chunks * (size_t)gat_ws_ld(heads, fo) * sizeof(float);
}

// Attach the long-row schedule of `plan` (may be NULL) and its workspace to the launch arguments.
static int gat_attach_plan(EdgeArgs& a, const dgll_csr_plan* plan, void* workspace, size_t workspace_bytes) {
    a.threshold = 0; a.n_chunks = 0; a.ws = nullptr;
    a.ws_vec = gat_ws_vec(a.heads, a.fo); a.ws_ld = gat_ws_ld(a.heads, a.fo);
    if (!plan) return DGLL_OK;
    DGLL_REQUIRE(plan->n_rows == a.n_rows, "plan was built for a different CSR");
    a.threshold = plan->threshold;
    a.n_chunks = plan->n_chunks;
    a.chunk_begin = plan->d_chunk_begin; a.chunk_end = plan->d_chunk_end; a.chunk_row = plan->d_chunk_row;
    if (plan->n_chunks > 0) {
        const size_t need = dgll_hip_gat_workspace_bytes(plan, a.heads, a.fo);
        if (!workspace || workspace_bytes < need) {
            set_error("workspace too small for the plan's long-row partials");
            return DGLL_ERR_WORKSPACE;
        }
        a.ws = static_cast<float*>(workspace);
    }
    return DGLL_OK;
}

static int gat_common(EdgeArgs& a, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads, int fo, int dtype,
                      float alpha, int mode, int apply_elu) {
    DGLL_REQUIRE(rowptr && col, "NULL CSR");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype");
    DGLL_REQUIRE(mode == 0 || mode == 1, "mode");
    const int epv = dtype == DGLL_BF16 ? 8 : 4;
    DGLL_REQUIRE(heads > 0 && fo > 0, "heads/fo must be positive");
    DGLL_REQUIRE(fo % epv == 0, "per-head width must be a multiple of the 16-byte vector (pad on the host)");
    a.rowptr = rowptr; a.col = col; a.n_rows = n_rows; a.heads = heads; a.fo = fo; a.feat = heads * fo;
    a.alpha = alpha; a.sign = mode == 0 ? -1.0f : 1.0f; a.use_max = mode; a.apply_elu = apply_elu;
    a.vph = fo / epv; a.tstride = heads; a.sd_out = nullptr; a.sd_stride = 0;
    return DGLL_OK;
}

// In-kernel attention dropout (a descriptor with drop_seed): p in [0, 1) and the device pointer to the two seed words.
static int gat_drop_args(EdgeArgs& a, double p, const uint32_t* seed) {
    if (!(p >= 0.0 && p < 1.0)) {
        set_error("attention dropout: p must lie in [0, 1)");
        return DGLL_ERR_INVALID;
    }
    DGLL_REQUIRE(seed, "attention dropout needs the device pointer to its two 32-bit seed words");
    DGLL_REQUIRE(a.n_rows < ((int64_t)1 << 31), "attention dropout keys on 32-bit node ids");
    a.drop_p = (float)p; a.drop = gat_dropout_params(p); a.drop_seed = seed;
    return DGLL_OK;
}

// What gat_choose() looks at, read off the filled launch arguments (and the pointers in them).
static GatLaunchDesc gat_describe(GatPass pass, const EdgeArgs& a, int dtype, GatRowsPhase phase, const dgll_csr_plan* plan) {
    const int esz = dtype == DGLL_BF16 ? 2 : 4;
    GatLaunchDesc d{};
    d.pass = pass; d.dtype = dtype; d.heads = a.heads; d.fo = a.fo; d.mode = a.use_max;
    d.edge_scale = a.edge_scale != nullptr;
    d.rowscore = pass != kGatTransposed && a.attn2 != nullptr;
    d.drop = a.drop_seed != nullptr;
    d.phase = phase;
    d.t_stride = a.tstride;
    d.t_aligned16 = !a.T || aligned16(a.T); d.dd_aligned16 = !a.DD || aligned16(a.DD);
    d.sd_out = a.sd_out != nullptr;
    d.score_epilogue = pass == kGatTransposed && a.attn1 != nullptr;
    d.score_behind_row = reinterpret_cast<const char*>(a.T) == static_cast<const char*>(a.H) + (size_t)a.feat * esz;
    d.score_pitch_equal = (int64_t)a.tstride * 4 == a.ldh * esz;
    d.second_follows = !a.DD || a.DD == a.T + 1;
    d.pad_bytes = (a.ldh - a.feat) * esz;
    d.has_plan = plan != nullptr;
    d.n_rows = a.n_rows;
    if (plan) { d.nnz = plan->nnz; d.n_chunks = plan->n_chunks; d.n_long = plan->n_long; }
    d.y_aligned = a.ldy % 4 == 0 && reinterpret_cast<uintptr_t>(a.Y) % (4 * esz) == 0;      // the wavefront finalize kernel stores four columns at once
    return d;
}

// [KIND][TROW][DROP] -> the launch function of that instantiation (gat_*.hip); NULL where kGat2Exists says none exists: gat_choose()
// has refused those.
typedef bool (*Gat2Launch)(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
static const Gat2Launch kGat2Launch[4][2][2] = {
    {{gat2_launch<0, false, false>, gat2_launch<0, false, true>}, {gat2_launch<0, true, false>, gat2_launch<0, true, true>}},
    {{gat2_launch<1, false, false>, nullptr}, {nullptr, nullptr}},
    {{gat2_launch<2, false, false>, gat2_launch<2, false, true>}, {nullptr, nullptr}},
    {{gat2_launch<3, false, false>, gat2_launch<3, false, true>}, {gat2_launch<3, true, false>, gat2_launch<3, true, true>}},
};

// The first-generation kernels: `lph` lanes per head, unroll 4 forward, 2 backward.
template <int L>
static void gat1_launch_lpr(GatPass pass, bool f32, dim3 grid, hipStream_t s, const EdgeArgs& a, int lph) {
    if (pass == kGatForward) {
        if (f32) hipLaunchKernelGGL((gat_fwd_kernel<float, float, 4, L, 4>), grid, dim3(kBlock), 0, s, a, lph);
        else hipLaunchKernelGGL((gat_fwd_kernel<bf16_t, bf16_t, 8, L, 4>), grid, dim3(kBlock), 0, s, a, lph);
    } else if (pass == kGatRows) {
        if (f32) hipLaunchKernelGGL((gat_bwd_rows_kernel<float, 4, L, 2>), grid, dim3(kBlock), 0, s, a, lph);
        else hipLaunchKernelGGL((gat_bwd_rows_kernel<bf16_t, 8, L, 2>), grid, dim3(kBlock), 0, s, a, lph);
    } else {
        if (f32) hipLaunchKernelGGL((gat_bwd_cols_kernel<float, float, 4, L, 2>), grid, dim3(kBlock), 0, s, a, lph);
        else hipLaunchKernelGGL((gat_bwd_cols_kernel<bf16_t, bf16_t, 8, L, 2>), grid, dim3(kBlock), 0, s, a, lph);
    }
}

template <typename YT>
static void gat_finalize(const GatChoice& c, const EdgeArgs& a, const dgll_csr_plan* plan, int pass, hipStream_t s) {
    if (c.finalize == kGatFinalizeWave)
        hipLaunchKernelGGL(gat_long_finalize_wave_kernel<YT>, dim3((uint32_t)((plan->n_long + kWavesPerBlock - 1) / kWavesPerBlock)),
                           dim3(kBlock), 0, s, a, plan->d_long_row, plan->d_long_chunk0, plan->n_long, pass);
    else
        hipLaunchKernelGGL(gat_long_finalize_kernel<YT>, dim3((uint32_t)plan->n_long), dim3(kBlock), 0, s, a, plan->d_long_row,
                           plan->d_long_chunk0, pass);
}

// The common tail of the three passes, `a` filled: the plan's schedule, the choice, the launch it names, the long rows' second launch.
static int gat_run(void* stream, GatPass pass, EdgeArgs& a, int dtype, const dgll_csr_plan* plan, void* workspace, size_t workspace_bytes,
                   GatRowsPhase phase = kGatRowsStoredFirst, float* part3 = nullptr) {
    int rc = gat_attach_plan(a, plan, workspace, workspace_bytes);
    if (rc != DGLL_OK) return rc;
    const GatChoice c = gat_choose(gat_describe(pass, a, dtype, phase, plan), g_gat_tune);
    if (c.error != DGLL_OK) {
        set_error(c.message);
        return c.error;
    }
    a.chunk_blocks = (uint32_t)c.chunk_blocks; a.rows_per_wave = c.rows_per_wave;
    if (pass == kGatRows) {
        gat_rows_phase_args(a, phase, c.generation);
        DGLL_REQUIRE(a.exact_dd < 2 || part3, "a split exact rows pass needs the [n_rows, 3 * heads] partial-sum buffer");
        a.part3 = c.generation == 2 ? part3 : nullptr;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)(c.chunk_blocks + c.row_blocks), (uint32_t)c.grid_y, 1);
    if (c.generation == 2) {
        if (!kGat2Launch[c.kind][c.trow][c.drop](dtype, c.lpr, c.nh, grid, s, a, c.inrow != 0)) {
            set_error("no second-generation GAT kernel for this head layout");
            return DGLL_ERR_UNSUPPORTED;
        }
    } else {
#define CALL(L) gat1_launch_lpr<L>(pass, dtype == DGLL_F32, grid, s, a, c.lph);
        DGLL_LPR_SWITCH(c.lpr, CALL)
#undef CALL
    }
    DGLL_HIP_TRY(hipGetLastError());
    if (c.finalize == kGatFinalizeNone) return DGLL_OK;
    if (pass == kGatRows || dtype == DGLL_F32) gat_finalize<float>(c, a, plan, pass, s);
    else gat_finalize<bf16_t>(c, a, plan, pass, s);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

// the row-score kernels address the gathered rows by 32-bit byte offsets formed with a 24-bit multiply
static bool rowscore_addressable(int64_t n_cols, int64_t ldh, int dtype) {
    const int64_t row_bytes = ldh * (dtype == DGLL_BF16 ? 2 : 4);
    return n_cols > 0 && n_cols <= (1 << 24) && row_bytes < (1 << 24) && n_cols * row_bytes <= (int64_t)0xffffffffll;
}

// Forward and rows pass: how the t_j reach the kernel -- col_score every col_score_stride floats, or attn2 with a NULL col_score (the
// row-score form: formed from the gathered rows) -- checked, then written to `a` with the other gathered-side inputs.
static int gat_gathered_side(EdgeArgs& a, const dgll_gat_desc& d) {
    const bool rowscore = d.attn2 && !d.col_score;
    if (d.drop_seed) {
        DGLL_REQUIRE((d.col_score != nullptr) != (d.attn2 != nullptr), "give col_score (with col_score_stride) or attn2, not both");
        DGLL_REQUIRE(d.n_cols > 0 && d.n_cols < ((int64_t)1 << 31), "attention dropout keys on 32-bit node ids");
    }
    DGLL_REQUIRE(rowscore || d.col_score_stride == 0 || d.col_score_stride >= d.heads, "col_score_stride must be at least heads");
    if (rowscore && !rowscore_addressable(d.n_cols, d.ld_h, d.dtype)) {
        set_error("the row-score form needs h of at most 2^24 rows and 4 GB (fill col_score instead of attn2)");
        return DGLL_ERR_UNSUPPORTED;
    }
    a.H = d.h; a.ldh = d.ld_h; a.S = d.row_score; a.T = d.col_score; a.attn2 = d.attn2; a.edge_scale = d.edge_scale;
    a.tstride = !rowscore && d.col_score_stride > 0 ? d.col_score_stride : d.heads;
    return DGLL_OK;
}

static int gat_fwd_impl(void* stream, const dgll_gat_desc& d) {
    if (d.n_rows <= 0) return DGLL_OK;
    EdgeArgs a{};
    int rc = gat_common(a, d.rowptr, d.col, d.n_rows, d.heads, d.fo, d.dtype, d.alpha, d.mode, d.apply_elu);
    if (rc != DGLL_OK) return rc;
    rc = gat_gathered_side(a, d);
    if (rc != DGLL_OK) return rc;
    DGLL_REQUIRE(d.h && d.row_score && (d.col_score || d.attn2) && d.out && d.rowsum, "NULL argument");
    DGLL_REQUIRE(!d.attn2 || (!d.col_score && d.mode == 0 && !d.edge_scale),
                 "the row-score form takes attn2 INSTEAD of col_score (sparseGatConv's form, no attention dropout array)");
    if (d.drop_seed) {
        DGLL_REQUIRE(d.mode == 0 && !d.edge_scale && !d.raw && !d.accumulate, "in-kernel dropout: sparseGatConv's form, one launch over the rows");
        rc = gat_drop_args(a, d.drop_p, d.drop_seed);
        if (rc != DGLL_OK) return rc;
    }
    DGLL_REQUIRE(d.mode == 0 || d.rowmax, "mode 1 needs a rowmax output");
    const int esz = d.dtype == DGLL_BF16 ? 2 : 4;
    DGLL_REQUIRE(vec_ok(d.h, d.ld_h, esz) && vec_ok(d.out, d.ld_out, esz) && d.ld_h >= a.feat && d.ld_out >= a.feat,
                 "h / out must be 16-byte aligned with padded pitches");
    a.Y = d.out; a.ldy = d.ld_out; a.out_a = d.rowsum; a.out_b = d.mode == 1 ? d.rowmax : nullptr;
    DGLL_REQUIRE(d.mode == 0 || (!d.raw && !d.accumulate), "split (raw / accumulate) launches support mode 0 only");
    a.raw = d.raw; a.accumulate = d.accumulate;
    return gat_run(stream, kGatForward, a, d.dtype, d.plan, d.workspace, d.workspace_bytes);
}

// Pass 1 of the backward (rows of A or of one column-half of A): DN, DD and grad_S.
static int gat_bwd_rows_impl(void* stream, const dgll_gat_desc& d) {
    if (d.n_rows <= 0) return DGLL_OK;
    EdgeArgs a{};
    int rc = gat_common(a, d.rowptr, d.col, d.n_rows, d.heads, d.fo, d.dtype, d.alpha, d.mode, d.apply_elu);
    if (rc != DGLL_OK) return rc;
    rc = gat_gathered_side(a, d);
    if (rc != DGLL_OK) return rc;
    const GatRowsPhase phase = gat_rows_phase(d.phase);
    DGLL_REQUIRE(d.dd || d.sd, "NULL dd: the rows pass writes dd_i into dd, into sd, or both");
    DGLL_REQUIRE(!d.sd || d.sd_stride >= 2 * d.heads, "sd_stride must be at least 2 * heads");
    DGLL_REQUIRE(phase < kGatRowsExactFirst || (d.dd && d.partial3),
                 "a split exact rows pass (phase 4 first / 5 middle / 6 last) needs non-NULL dd and partial3");
    DGLL_REQUIRE(d.h && d.row_score && (d.col_score || d.attn2) && d.out && d.grad_out && d.rowsum && d.dn && d.grad_score, "NULL argument");
    DGLL_REQUIRE(!d.attn2 || (!d.col_score && d.mode == 0 && !d.edge_scale && phase == kGatRowsExactOnly),
                 "the row-score form takes attn2 INSTEAD of col_score: sparseGatConv's form, one launch over the rows (exact dd_i)");
    if (d.drop_seed) {
        DGLL_REQUIRE(d.mode == 0 && !d.edge_scale && phase == kGatRowsExactOnly,
                     "in-kernel dropout: sparseGatConv's form, one launch over the rows (exact dd_i)");
        rc = gat_drop_args(a, d.drop_p, d.drop_seed);
        if (rc != DGLL_OK) return rc;
    }
    DGLL_REQUIRE(d.mode == 0 || d.rowmax, "mode 1 needs the forward's rowmax");
    const int esz = d.dtype == DGLL_BF16 ? 2 : 4;
    DGLL_REQUIRE(vec_ok(d.h, d.ld_h, esz) && vec_ok(d.out, d.ld_out, esz) && vec_ok(d.grad_out, d.ld_grad_out, esz) && vec_ok(d.dn, d.ld_dn, esz),
                 "matrices must be 16-byte aligned with padded pitches");
    a.M = d.mode == 1 ? d.rowmax : nullptr; a.DEN = d.rowsum;
    a.G = d.grad_out; a.ldg = d.ld_grad_out; a.O = d.out; a.ldo = d.ld_out; a.Y = d.dn; a.ldy = d.ld_dn; a.out_a = d.grad_score; a.out_b = d.dd;
    a.sd_out = d.sd; a.sd_stride = d.sd_stride;
    return gat_run(stream, kGatRows, a, d.dtype, d.plan, d.workspace, d.workspace_bytes, phase, d.partial3);
}

// Pass 2 of the backward over a transposed structure (rows = source nodes j, columns = destination rows i):
// grad_H[j] = sum_i w_ij scale_ij DN[i], grad_T[j] = sum_i dz_ij.  h / row_score belong to the rows of this pass, dn / col_score /
// col_dd / rowmax to its columns.
static int gat_bwd_cols_impl(void* stream, const dgll_gat_desc& d) {
    if (d.n_rows <= 0) return DGLL_OK;
    EdgeArgs t{};
    int rc = gat_common(t, d.rowptr, d.col, d.n_rows, d.heads, d.fo, d.dtype, d.alpha, d.mode, 0);
    if (rc != DGLL_OK) return rc;
    DGLL_REQUIRE(d.col_score_stride == 0 || d.col_score_stride >= d.heads, "col_score_stride must be at least heads");
    DGLL_REQUIRE(d.dn && d.h && d.row_score && d.col_score && d.col_dd && d.grad_h && d.grad_score, "NULL argument");
    DGLL_REQUIRE(d.mode == 0 || d.rowmax, "mode 1 needs the forward's rowmax");
    DGLL_REQUIRE(!d.edge_scale || d.perm, "edge_scale needs the transpose permutation");
    const int esz = d.dtype == DGLL_BF16 ? 2 : 4;
    DGLL_REQUIRE(vec_ok(d.dn, d.ld_dn, esz) && vec_ok(d.h, d.ld_h, esz) && vec_ok(d.grad_h, d.ld_grad_h, esz),
                 "matrices must be 16-byte aligned with padded pitches");
    t.perm = d.perm; t.H = d.dn; t.ldh = d.ld_dn; t.G = d.h; t.ldg = d.ld_h; t.S = d.row_score; t.T = d.col_score; t.DD = d.col_dd;
    t.tstride = d.col_score_stride > 0 ? d.col_score_stride : d.heads;
    DGLL_REQUIRE(!d.attn1 || (d.attn2 && d.grad_s_rows), "the score-gradient epilogue needs attn1, attn2 and the rows' grad_S");
    t.attn1 = d.attn1; t.attn2 = d.attn2; t.gs_rows = d.grad_s_rows;
    if (d.drop_seed) {
        DGLL_REQUIRE(d.mode == 0 && !d.edge_scale, "in-kernel dropout: sparseGatConv's form");
        rc = gat_drop_args(t, d.drop_p, d.drop_seed);
        if (rc != DGLL_OK) return rc;
    }
    t.M = d.mode == 1 ? d.rowmax : nullptr; t.edge_scale = d.edge_scale; t.Y = d.grad_h; t.ldy = d.ld_grad_h; t.out_a = d.grad_score;
    t.out_b = nullptr;
    return gat_run(stream, kGatTransposed, t, d.dtype, d.plan, d.workspace, d.workspace_bytes);
}

static_assert(DGLL_GAT_FORWARD == kGatForward && DGLL_GAT_ROWS == kGatRows && DGLL_GAT_TRANSPOSED == kGatTransposed &&
              DGLL_GAT_ROWS_STORED_FIRST == kGatRowsStoredFirst && DGLL_GAT_ROWS_STORED_FURTHER == kGatRowsStoredFurther &&
              DGLL_GAT_ROWS_EXACT_ONLY == kGatRowsExactOnly && DGLL_GAT_ROWS_EXACT_FIRST == kGatRowsExactFirst &&
              DGLL_GAT_ROWS_EXACT_MIDDLE == kGatRowsExactMiddle && DGLL_GAT_ROWS_EXACT_LAST == kGatRowsExactLast,
              "the header's pass and phase values are GatPass and GatRowsPhase");

DGLL_API int dgll_hip_gat_pass(void* stream, const dgll_gat_desc* d) {
    DGLL_REQUIRE(d != nullptr, "NULL descriptor");
    switch (d->pass) {
        case DGLL_GAT_FORWARD: return gat_fwd_impl(stream, *d);
        case DGLL_GAT_ROWS: return gat_bwd_rows_impl(stream, *d);
        case DGLL_GAT_TRANSPOSED: return gat_bwd_cols_impl(stream, *d);
    }
    set_error("pass must be DGLL_GAT_FORWARD, DGLL_GAT_ROWS or DGLL_GAT_TRANSPOSED");
    return DGLL_ERR_INVALID;
}

DGLL_API int dgll_hip_debug_gat_choice(int pass, int dtype, int heads, int fo, int mode, int edge_scale, int rowscore, int drop, int phase,
                                       int t_stride, int t_aligned16, int dd_aligned16, int sd_out, int score_epilogue,
                                       int score_behind_row, int score_pitch_equal, int second_follows, int64_t pad_bytes, int has_plan,
                                       int64_t n_rows, int64_t nnz, int64_t n_chunks, int64_t n_long, int y_aligned, dgll_gat_choice* out) {
    DGLL_REQUIRE(out != nullptr, "out is NULL");
    DGLL_REQUIRE(pass >= kGatForward && pass <= kGatTransposed && (dtype == DGLL_F32 || dtype == DGLL_BF16) && (mode == 0 || mode == 1),
                 "pass / dtype / mode");
    DGLL_REQUIRE(heads > 0 && fo > 0 && fo % (dtype == DGLL_BF16 ? 8 : 4) == 0 && t_stride >= 0 && pad_bytes >= 0 && n_rows > 0 && nnz >= 0 &&
                 n_chunks >= 0 && n_long >= 0, "bad launch description");
    const bool plan = has_plan != 0;
    *out = gat_choose(GatLaunchDesc{(GatPass)pass, dtype, heads, fo, mode, edge_scale != 0, rowscore != 0, drop != 0, gat_rows_phase(phase),
                                    t_stride > 0 ? t_stride : heads, t_aligned16 != 0, dd_aligned16 != 0, sd_out != 0, score_epilogue != 0,
                                    score_behind_row != 0, score_pitch_equal != 0, second_follows != 0, pad_bytes, plan, n_rows,
                                    plan ? nnz : 0, plan ? n_chunks : 0, plan ? n_long : 0, y_aligned != 0}, g_gat_tune);
    if (out->error != DGLL_OK) set_error(out->message);
    return out->error;
}

// The [nnz, heads] multipliers of a CSR as a tensor, from the one function the passes evaluate (tests; callers that want the mask).
__global__ __launch_bounds__(kBlock) void gat_dropout_mask_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                  int64_t n_rows, int heads, const uint32_t* __restrict__ seed,
                                                                  GatDropout d, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const uint32_t s0 = seed[0], s1 = seed[1];
    const uint32_t rk = gat_dropout_row_key(s0, s1, (uint32_t)row);
    const int64_t b = rowptr[row], e = rowptr[row + 1];
    for (int64_t k = b + lane_id(); k < e; k += kWave) {
        const uint32_t ck = gat_dropout_col_key(s0, s1, (uint32_t)col[k]);
        for (int h = 0; h < heads; ++h) out[k * heads + h] = gat_dropout_keep(gat_dropout_draw(rk, ck, (uint32_t)h), d);
    }
}

static int gat_mask_args(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads, const uint32_t* seed, double p, float* out) {
    DGLL_REQUIRE(rowptr && col && seed && out, "NULL argument");
    DGLL_REQUIRE(heads > 0 && n_rows < ((int64_t)1 << 31), "heads must be positive, node ids 32-bit");
    if (!(p >= 0.0 && p < 1.0)) {
        set_error("attention dropout: p must lie in [0, 1)");
        return DGLL_ERR_INVALID;
    }
    return DGLL_OK;
}

DGLL_API int dgll_hip_gat_dropout_mask(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads,
                                       const uint32_t* seed, double p, float* out) {
    if (n_rows <= 0) return DGLL_OK;
    const int rc = gat_mask_args(rowptr, col, n_rows, heads, seed, p, out);
    if (rc != DGLL_OK) return rc;
    hipLaunchKernelGGL(gat_dropout_mask_kernel, dim3((uint32_t)((n_rows + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), rowptr, col, n_rows, heads, seed, gat_dropout_params(p), out);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

// the same on the host (all pointers host memory): a plain loop over the same function, no GPU needed
DGLL_API int dgll_host_gat_dropout_mask(const int64_t* rowptr, const int32_t* col, int64_t n_rows, int heads, const uint32_t* seed,
                                        double p, float* out) {
    if (n_rows <= 0) return DGLL_OK;
    const int rc = gat_mask_args(rowptr, col, n_rows, heads, seed, p, out);
    if (rc != DGLL_OK) return rc;
    const GatDropout d = gat_dropout_params(p);
    for (int64_t i = 0; i < n_rows; ++i)
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            for (int h = 0; h < heads; ++h)
                out[k * heads + h] = gat_dropout_multiplier(seed[0], seed[1], (uint32_t)i, (uint32_t)col[k], (uint32_t)h, d);
    return DGLL_OK;
}

DGLL_API int dgll_hip_segment_max(void* stream, const int64_t* rowptr, const int32_t* col, const void* X, int64_t ldx,
                                  void* Y, int32_t* arg, int64_t ldy, int dtype, int64_t n_rows, int feat) {
    if (n_rows <= 0 || feat <= 0) return DGLL_OK;
    DGLL_REQUIRE(rowptr && col && X && Y && arg, "NULL argument");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype");
    const int esz = dtype == DGLL_BF16 ? 2 : 4, epv = 16 / esz;
    const int vecs = (feat + epv - 1) / epv;
    DGLL_REQUIRE(vec_ok(X, ldx, esz) && vec_ok(Y, ldy, esz) && ldx >= vecs * epv && ldy >= vecs * epv,
                 "segment_max operands must be 16-byte aligned with padded leading dimensions");
    EdgeArgs a{};
    a.rowptr = rowptr; a.col = col; a.H = X; a.ldh = ldx; a.Y = Y; a.ldy = ldy; a.arg_out = arg; a.n_rows = n_rows;
    a.feat = vecs * epv;  // padded columns are computed too (they live inside the padded leading dimension)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lpr = pick_lpr(vecs);
    dim3 grid((uint32_t)((n_rows + kWavesPerBlock - 1) / kWavesPerBlock), (uint32_t)((vecs + lpr - 1) / lpr));
#define CALL(L)                                                                                                          \
    if (dtype == DGLL_F32) hipLaunchKernelGGL((segment_max_kernel<float, 4, L, 4>), grid, dim3(kBlock), 0, s, a);        \
    else hipLaunchKernelGGL((segment_max_kernel<bf16_t, 8, L, 4>), grid, dim3(kBlock), 0, s, a);
    DGLL_LPR_SWITCH(lpr, CALL)
#undef CALL
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_segment_max_bwd(void* stream, const int64_t* t_rowptr, const int32_t* t_col, const void* G, int64_t ldg,
                                      const int32_t* arg, int64_t ldarg, void* grad, int64_t ldgrad, int dtype,
                                      int64_t n_src, int feat) {
    if (n_src <= 0 || feat <= 0) return DGLL_OK;
    DGLL_REQUIRE(t_rowptr && t_col && G && arg && grad, "NULL argument");
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype");
    const int esz = dtype == DGLL_BF16 ? 2 : 4, epv = 16 / esz;
    const int vecs = (feat + epv - 1) / epv;
    DGLL_REQUIRE(vec_ok(G, ldg, esz) && vec_ok(grad, ldgrad, esz) && ldg >= vecs * epv && ldgrad >= vecs * epv && ldarg >= vecs * epv,
                 "segment_max_bwd operands must be 16-byte aligned with padded leading dimensions");
    EdgeArgs a{};
    a.rowptr = t_rowptr; a.col = t_col; a.G = G; a.ldg = ldg; a.Y = grad; a.ldy = ldgrad; a.n_rows = n_src;
    a.feat = vecs * epv;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int lpr = pick_lpr(vecs);
    dim3 grid((uint32_t)((n_src + kWavesPerBlock - 1) / kWavesPerBlock), (uint32_t)((vecs + lpr - 1) / lpr));
#define CALL(L)                                                                                                                  \
    if (dtype == DGLL_F32) hipLaunchKernelGGL((segment_max_bwd_kernel<float, 4, L, 4>), grid, dim3(kBlock), 0, s, a, arg, ldarg);  \
    else hipLaunchKernelGGL((segment_max_bwd_kernel<bf16_t, 8, L, 4>), grid, dim3(kBlock), 0, s, a, arg, ldarg);
    DGLL_LPR_SWITCH(lpr, CALL)
#undef CALL
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
