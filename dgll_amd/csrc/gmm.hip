// gmm.hip -- gather passes over a graph whose edges carry continuous PSEUDO-COORDINATES (MoNet / DGL's GMMConv): the three passes of
// dgll_amd/ops_gmm.py behind ONE entry point, dgll_hip_gmm_pass (include/dgll_hip.h: dgll_gmm_desc).
//
//   h_i = s_i sum_{e = (j -> i)} sum_k w_k(e) x_j W_k      =>      h_i = sum_k Z[i, k, :] W_k,   Z[i, k, :] = s_i sum_e w_k(e) x_j
//   w_k(e) = exp(-0.5 sum_d ((pseudo[e, d] - mu[k, d]) inv_sigma[k, d])^2)
//
// The product with the stacked W_k is a dense transform (dense.py); what is sparse is Z [n_rows, K * F] (kernel-major blocks of width
// F), and it is typed_spmm.hip's gather with the coefficient COMPUTED per entry from pseudo[e, :] instead of read from a table:
//
//   expand    rows of A     gathers x_j once per entry into up to kKernelBlock kernels' accumulators                -> Z
//   contract  rows of A^T   gathers dZ[i, 0 : K F]; pseudo read at slot perm[e']                                    -> dX[j, :] = sum_e sum_k w_k(e) dZ[i_e, k, :]
//   param     entries       streamed, no gather: reads P[e, k] = <x_j, dZ[i, k, :]> (typed_spmm.hip's dots) and pseudo
//                                                                          -> grad_pseudo [nnz, dim]; one slab [2, K, dim] per workgroup
//
// w_k(e) comes from ONE device function (weight): fp32, d ascending, squares of (u - mu) * s, one exponential through
// __builtin_amdgcn_exp2f with log2(e) folded into the factor, so the three passes see the same bits; u == mu gives exp2(-0) = 1 and
// an exponent below -149 gives 0.  In the gather passes the weights of an entry are computed by the lane that read its index in the
// batch and handed round the row's lanes with the index (rt::hand_round): K exponentials per lane and batch, not per lane and entry.
// mu and inv_sigma are staged in LDS once per workgroup.  Lane layout, tiles, index batches and the long-row merge: row_tiles.hpp; the
// expand state (up to 64 floats a lane) crosses LDS kMergeSlice floats at a time.  Rows wider than 64 lanes are cut into column blocks
// over blockIdx.y, kernels past kKernelBlock into further blocks over blockIdx.z (expand; each gathers x_j again) or swept block after
// block by the same lanes (contract).  col and perm values used for addressing are clamped.  No float atomics anywhere.
#include "row_tiles.hpp"

namespace dgll {
namespace gmm {

constexpr int kLongRow = DGLL_GMM_LONG_ROW;         // rows longer than this are swept by a whole workgroup
constexpr int kMaxDim = DGLL_GMM_MAX_DIM;
constexpr int kMaxKernels = DGLL_GMM_MAX_KERNELS;
constexpr int kKernelBlock = DGLL_GMM_KERNEL_BLOCK; // kernels a lane accumulates (expand) or gathers (contract) at a time
constexpr int kParamBlock = 4;                      // kernels per round of the param pass: one 16-byte vector of P
constexpr int kMergeSlice = 16;                     // floats of a lane's state that cross LDS at a time in the long-row merge (16 KB)
constexpr int kTable = 2 * kMaxKernels * kMaxDim;   // mu then inv_sigma, [K, dim] each

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int64_t* perm;                    // contract: A^T's entry -> A's entry (the slot of pseudo)
    const float* scale;                     // expand: per row, or NULL (1)
    const float* pseudo; int64_t ld_pseudo; // [nnz, dim] fp32, pitch in elements
    const float* mu;                        // [K, dim]
    const float* inv_sigma;                 // [K, dim]
    int64_t n_rows, n_cols, nnz, tiles;
    const char* x;   int64_t pb_x;          // the gathered matrix: X (expand), dZ (contract); pitches in BYTES
    char* out;       int64_t pb_out;        // expand: Z; contract: dX
    const float* p;  int64_t ld_p;          // param: P [nnz, ld_p]
    float* gp;       int64_t ld_gp;         // param: grad_pseudo [nnz, ld_gp], or NULL
    float* slabs;                           // param: [gridDim.x, 2, K, dim]
    int64_t fb;                             // bytes of one kernel block of a row of Z / dZ: F * sizeof(T)
    int K, dim, vpr, lpr;                   // vpr: 16-byte vectors of F columns; lpr: lanes of a row
};

// mu and inv_sigma into the workgroup's table (ends with a barrier)
__device__ __forceinline__ void stage_tables(const Args& a, float* tab) {
    const int n = a.K * a.dim;
    for (int i = (int)threadIdx.x; i < n; i += kBlock) {
        tab[i] = a.mu[i];
        tab[n + i] = a.inv_sigma[i];
    }
    __syncthreads();
}

// one row of pseudo into registers (columns past dim, and a lane without an entry: zeros)
__device__ __forceinline__ void load_pseudo(const Args& a, int64_t slot, bool on, float (&u)[kMaxDim]) {
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) {
        u[d] = 0.0f;
        if (on && d < a.dim) u[d] = a.pseudo[slot * a.ld_pseudo + d];
    }
}

// THE weight: w = exp(-0.5 sum_d ((u_d - mu_d) s_d)^2), d ascending, one exp2 with log2(e) folded into the factor
__device__ __forceinline__ float weight(const float (&u)[kMaxDim], const float* mu, const float* s, int dim) {
    float q = 0.0f;
#pragma unroll
    for (int d = 0; d < kMaxDim; ++d) {
        if (d < dim) {
            const float t = (u[d] - mu[d]) * s[d];
            q = fmaf(t, t, q);
        }
    }
    return __builtin_amdgcn_exp2f(q * (-0.5f * rt::kLog2e));
}

// ---- expand: rows of A ----------------------------------------------------------------------------------------------------------------
// BB: kernels of this block.  State of one lane, in slices of MS floats so that the long-row merge can move it through LDS: flat
// index k * EPV + d holds Z[row, b0 + k, lane's column d].
template <typename T, int BB>
__global__ __launch_bounds__(kBlock) void gmm_expand_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), NP = BB * EPV, MS = NP < kMergeSlice ? NP : kMergeSlice, NS = NP / MS, U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float tab[kTable];
    __shared__ float lds[MS * kBlock];

    const rt::Lanes lanes(a.lpr);
    stage_tables(a, tab);
    const int dim = a.dim;
    const float* mu = tab;
    const float* sg = tab + a.K * dim;
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;        // the lane's columns: byte offset inside a kernel block
    const int b0 = (int)blockIdx.z * BB;
    const int nbk = a.K - b0 < BB ? a.K - b0 : BB;          // kernels of this block that exist

    float st[NS][MS];

    auto begin = [&](int64_t, int64_t, int64_t, bool) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < MS; ++k) st[s][k] = 0.0f;
    };

    // one batch of the row's entries, two in flight; the weights of an entry travel with its index
    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const bool has = lanes.sub < nb;
        float my_w[BB];
        {
            float u[kMaxDim];
            load_pseudo(a, k0 + lanes.sub, has, u);
#pragma unroll
            for (int k = 0; k < BB; ++k) my_w[k] = has && k < nbk ? weight(u, mu + (b0 + k) * dim, sg + (b0 + k) * dim, dim) : 0.0f;
        }
        const int max_nb = rt::wave_max(nb);
        for (int t = 0; t < max_nb; t += U) {
            typename IO::raw_t r[U];
            float w[U][BB];
            bool ok[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int c = rt::hand_round(my_col, t + q, lanes);
#pragma unroll
                for (int k = 0; k < BB; ++k) w[q][k] = rt::hand_round(my_w[k], t + q, lanes);
                ok[q] = t + q < nb && active;
                r[q] = IO::zero();
                if (ok[q]) r[q] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + cb));
            }
#pragma unroll
            for (int q = 0; q < U; ++q) {
                float f[EPV];
                IO::unpack(r[q], f);
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    const float cf = ok[q] ? w[q][k] : 0.0f;
#pragma unroll
                    for (int d = 0; d < EPV; ++d) {
                        float& acc = st[(k * EPV + d) / MS][(k * EPV + d) % MS];
                        acc = fmaf(cf, f[d], acc);
                    }
                }
            }
        }
    };

    // the row's outputs from its complete state (the long-row path calls it from the first lane group alone)
    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        const float s = a.scale ? a.scale[row] : 1.0f;
#pragma unroll
        for (int k = 0; k < BB; ++k) {
            if (k < nbk) {
                float o[EPV];
#pragma unroll
                for (int d = 0; d < EPV; ++d) o[d] = s * st[(k * EPV + d) / MS][(k * EPV + d) % MS];
                IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + (int64_t)(b0 + k) * a.fb + cb), o);    // an empty row: zeros
            }
        }
    };

    auto long_done = [&](int64_t row, int64_t b, int64_t e) {
#pragma unroll
        for (int s = 0; s < NS; ++s) rt::merge_partials<false>(st[s], lds, lanes, [&] { if (s == NS - 1) finish(row, b, e); });
    };

    rt::sweep_rows(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, begin, batch, finish, long_done);
}

// ---- contract: rows of A^T ----------------------------------------------------------------------------------------------------------------
// BB: kernels gathered at a time (the blocks of dZ's row are swept one after another by the same lanes)
template <typename T, int BB>
__global__ __launch_bounds__(kBlock) void gmm_contract_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T);
    using IO = VecIO<T, EPV>;
    __shared__ float tab[kTable];
    __shared__ float lds[EPV * kBlock];

    const rt::Lanes lanes(a.lpr);
    stage_tables(a, tab);
    const int dim = a.dim, K = a.K;
    const float* mu = tab;
    const float* sg = tab + K * dim;
    const int v = (int)blockIdx.y * lanes.lpr + lanes.sub;
    const bool active = v < a.vpr;
    const int64_t cb = active ? (int64_t)v * 16 : 0;

    float acc[EPV];

    auto begin = [&](int64_t, int64_t, int64_t, bool) {
#pragma unroll
        for (int d = 0; d < EPV; ++d) acc[d] = 0.0f;
    };

    auto batch = [&](int64_t k0, int nb) {
        const int my_col = rt::batch_index(a.col, k0, nb, (int)a.n_cols, lanes);
        const bool has = lanes.sub < nb;
        int64_t my_slot = 0;
        if (has) my_slot = max((int64_t)0, min(a.perm[k0 + lanes.sub], a.nnz - 1));
        float u[kMaxDim];
        load_pseudo(a, my_slot, has, u);
        const int max_nb = rt::wave_max(nb);
        for (int kb = 0; kb < K; kb += BB) {                // (uniform: every lane of the workgroup has the same K)
            const int nbk = K - kb < BB ? K - kb : BB;
            float my_w[BB];
#pragma unroll
            for (int k = 0; k < BB; ++k) my_w[k] = has && k < nbk ? weight(u, mu + (kb + k) * dim, sg + (kb + k) * dim, dim) : 0.0f;
            for (int t = 0; t < max_nb; ++t) {
                const int c = rt::hand_round(my_col, t, lanes);
                const bool ok = t < nb && active;
                typename IO::raw_t r[BB];
                float w[BB];
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    w[k] = rt::hand_round(my_w[k], t, lanes);
                    r[k] = IO::zero();
                    if (ok && k < nbk) r[k] = IO::load(reinterpret_cast<const T*>(a.x + (int64_t)c * a.pb_x + (int64_t)(kb + k) * a.fb + cb));
                }
#pragma unroll
                for (int k = 0; k < BB; ++k) {
                    const float cf = ok ? w[k] : 0.0f;
                    float f[EPV];
                    IO::unpack(r[k], f);
#pragma unroll
                    for (int d = 0; d < EPV; ++d) acc[d] = fmaf(cf, f[d], acc[d]);
                }
            }
        }
    };

    auto finish = [&](int64_t row, int64_t, int64_t) {
        if (!active) return;
        IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), acc);     // a source no row references: zeros
    };

    rt::reduce_rows<false>(a.tiles, a.n_rows, a.rowptr, kLongRow, lanes, acc, lds, begin, batch, finish);
}

// ---- param: the entries streamed, one slab per workgroup ------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// A thread takes entries blockIdx.x * kBlock + tid, + gridDim.x * kBlock, ...; kParamBlock kernels per round, the same entries in
// every round, so the thread that wrote grad_pseudo[e] in round 0 adds to it in the later ones.  Per round: the thread's sums over its
// entries, a butterfly over the wavefront, the four wavefronts added in order through LDS.
__global__ __launch_bounds__(kBlock) void gmm_param_kernel(const Args a) {
    constexpr int KB = kParamBlock, NV = 2 * KB * kMaxDim;
    using P4 = VecIO<float, 4>;
    static_assert(KB == 4 && NV <= kBlock, "one vector of P per round; one thread per reduced value");
    __shared__ float tab[kTable];
    __shared__ float red[kWavesPerBlock * NV];

    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    stage_tables(a, tab);
    const int dim = a.dim, K = a.K;
    const float* mu = tab;
    const float* sg = tab + K * dim;
    float* slab = a.slabs + (int64_t)blockIdx.x * 2 * K * dim;
    const int64_t first = (int64_t)blockIdx.x * kBlock + tid, step = (int64_t)gridDim.x * kBlock;

    for (int kb = 0; kb < K; kb += KB) {
        float gm[KB][kMaxDim], gs[KB][kMaxDim];
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
            for (int d = 0; d < kMaxDim; ++d) gm[k][d] = gs[k][d] = 0.0f;

        for (int64_t e = first; e < a.nnz; e += step) {
            float u[kMaxDim], pk[KB], gp[kMaxDim];
            load_pseudo(a, e, true, u);
            P4::unpack(P4::load(a.p + e * a.ld_p + kb), pk);        // (ld_p is K rounded up to 4: the vector is inside the row)
#pragma unroll
            for (int d = 0; d < kMaxDim; ++d) gp[d] = 0.0f;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (kb + k < K) {
                    const float* mk = mu + (kb + k) * dim;
                    const float* sk = sg + (kb + k) * dim;
                    const float pw = pk[k] * weight(u, mk, sk, dim);
#pragma unroll
                    for (int d = 0; d < kMaxDim; ++d) {
                        if (d < dim) {
                            const float diff = u[d] - mk[d], s = sk[d];
                            const float q = pw * diff * s;
                            gm[k][d] = fmaf(q, s, gm[k][d]);
                            gs[k][d] = fmaf(-q, diff, gs[k][d]);
                            gp[d] = fmaf(-q, s, gp[d]);
                        }
                    }
                }
            }
            if (a.gp) {
#pragma unroll
                for (int d = 0; d < kMaxDim; ++d) {
                    if (d < dim) {
                        float* dst = a.gp + e * a.ld_gp + d;
                        *dst = kb == 0 ? gp[d] : *dst + gp[d];
                    }
                }
            }
        }

#pragma unroll
        for (int k = 0; k < KB; ++k) {
#pragma unroll
            for (int d = 0; d < kMaxDim; ++d) {
                if (d < dim) {                                      // (uniform)
                    const float m = wave_sum(gm[k][d]), s = wave_sum(gs[k][d]);
                    if (lane == 0) {
                        red[wave * NV + k * kMaxDim + d] = m;
                        red[wave * NV + (KB + k) * kMaxDim + d] = s;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < NV) {
            const int which = tid / (KB * kMaxDim), k = tid / kMaxDim % KB, d = tid % kMaxDim;
            if (kb + k < K && d < dim) {
                float sum = red[tid];
#pragma unroll
                for (int w = 1; w < kWavesPerBlock; ++w) sum += red[w * NV + tid];
                slab[((int64_t)which * K + kb + k) * dim + d] = sum;
            }
        }
        __syncthreads();                                            // the next round writes red again
    }
}

template <typename T, int BB>
void launch_block(int pass, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_GMM_EXPAND) hipLaunchKernelGGL((gmm_expand_kernel<T, BB>), grid, dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((gmm_contract_kernel<T, BB>), grid, dim3(kBlock), 0, s, a);
}

template <typename T>
void launch(int pass, int bb, dim3 grid, hipStream_t s, const Args& a) {
    if (bb == 1) launch_block<T, 1>(pass, grid, s, a);
    else if (bb == 2) launch_block<T, 2>(pass, grid, s, a);
    else if (bb == 4) launch_block<T, 4>(pass, grid, s, a);
    else launch_block<T, 8>(pass, grid, s, a);
}

}  // namespace gmm
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_gmm_pass(void* stream, const dgll_gmm_desc* d) {
    static const char* const kPass = "dgll_hip_gmm_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_gmm_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_GMM_EXPAND || d->pass == DGLL_GMM_CONTRACT || d->pass == DGLL_GMM_PARAM,
                 "dgll_hip_gmm_pass: pass must be DGLL_GMM_EXPAND, DGLL_GMM_CONTRACT or DGLL_GMM_PARAM");
    DGLL_REQUIRE(d->dtype == DGLL_F32 || d->dtype == DGLL_BF16, "dgll_hip_gmm_pass: dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(d->K >= 1 && d->K <= DGLL_GMM_MAX_KERNELS, "dgll_hip_gmm_pass: K (the Gaussian kernels) must be in [1, DGLL_GMM_MAX_KERNELS = 64]");
    DGLL_REQUIRE(d->dim >= 1 && d->dim <= DGLL_GMM_MAX_DIM, "dgll_hip_gmm_pass: dim (the pseudo-coordinates of an entry) must be in [1, DGLL_GMM_MAX_DIM = 8]");
    DGLL_REQUIRE(d->nnz >= 0 && d->nnz < (1ll << 31), "dgll_hip_gmm_pass: nnz (the rows of pseudo) in [0, 2^31)");
    DGLL_REQUIRE(d->pseudo != nullptr && d->ld_pseudo >= d->dim, "dgll_hip_gmm_pass: pseudo fp32 [nnz, dim] must be non-NULL with pitch ld_pseudo >= dim");
    DGLL_REQUIRE(d->mu != nullptr && d->inv_sigma != nullptr, "dgll_hip_gmm_pass: mu and inv_sigma fp32 [K, dim] must be non-NULL");
    const auto [epv, esz] = rt::storage_of(d->dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);

    gmm::Args a{};
    a.pseudo = d->pseudo;
    a.ld_pseudo = d->ld_pseudo;
    a.mu = d->mu;
    a.inv_sigma = d->inv_sigma;
    a.nnz = d->nnz;
    a.K = d->K;
    a.dim = d->dim;

    if (d->pass == DGLL_GMM_PARAM) {
        DGLL_REQUIRE(d->p != nullptr && aligned16(d->p) && d->ld_p == ((int64_t)d->K + 3) / 4 * 4,
                     "dgll_hip_gmm_pass: param: p fp32 [nnz, ld_p] non-NULL, 16-byte aligned, with pitch ld_p = K rounded up to 4");
        DGLL_REQUIRE(d->partials >= 1 && d->partials <= DGLL_GMM_MAX_PARTIALS,
                     "dgll_hip_gmm_pass: param: partials (the workgroups, and slabs) must be in [1, DGLL_GMM_MAX_PARTIALS = 2048]");
        DGLL_REQUIRE(d->slabs != nullptr, "dgll_hip_gmm_pass: param: slabs [partials, 2, K, dim] fp32 must be non-NULL");
        DGLL_REQUIRE(d->grad_pseudo == nullptr || d->ld_grad_pseudo >= d->dim,
                     "dgll_hip_gmm_pass: param: grad_pseudo fp32 [nnz, dim] must be NULL or have a pitch ld_grad_pseudo >= dim");
        a.p = d->p;
        a.ld_p = d->ld_p;
        a.gp = d->grad_pseudo;
        a.ld_gp = d->ld_grad_pseudo;
        a.slabs = d->slabs;
        hipLaunchKernelGGL(gmm::gmm_param_kernel, dim3((unsigned)d->partials), dim3(kBlock), 0, st, a);
        DGLL_HIP_TRY(hipGetLastError());
        return DGLL_OK;
    }

    if (const int rc = rt::require_flat_pass(kPass, d->dtype, d->F, d->n_rows, d->n_cols, d->nnz, d->rowptr, d->col, true)) return rc;
    DGLL_REQUIRE((int64_t)d->K * d->F < (1ll << 31), "dgll_hip_gmm_pass: K * F < 2^31");
    const bool contract = d->pass == DGLL_GMM_CONTRACT;
    DGLL_REQUIRE_OPERAND(kPass, out, contract ? d->F : d->K * d->F);
    if (contract) {
        DGLL_REQUIRE_OPERAND(kPass, dz, d->K * d->F);
        DGLL_REQUIRE(d->perm != nullptr, "dgll_hip_gmm_pass: contract: perm must be non-NULL (pseudo is read at slot perm[e'])");
        a.perm = d->perm;
    } else {
        DGLL_REQUIRE_OPERAND(kPass, x, d->F);
        a.scale = d->scale;
    }
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.x = static_cast<const char*>(contract ? d->dz : d->x);
    a.pb_x = (contract ? d->ld_dz : d->ld_x) * esz;
    a.out = static_cast<char*>(d->out);
    a.pb_out = d->ld_out * esz;
    a.fb = d->F * esz;
    a.vpr = (int)(d->F / epv);
    const rt::HeadGeometry geo = rt::make_flat_geometry(a.vpr, d->n_rows);
    rt::set_geometry(a, geo);
    if (geo.grid == 0) return DGLL_OK;
    // kernels per block: the smallest compiled size that holds K, kKernelBlock for more
    int bb = 1;
    while (bb < gmm::kKernelBlock && bb < d->K) bb <<= 1;
    const int64_t gz = contract ? 1 : ((int64_t)d->K + bb - 1) / bb;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, geo.col_blocks, gz, grid)) return rc;
    if (d->dtype == DGLL_F32) gmm::launch<float>(d->pass, bb, grid, st, a);
    else gmm::launch<bf16_t>(d->pass, bb, grid, st, a);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
