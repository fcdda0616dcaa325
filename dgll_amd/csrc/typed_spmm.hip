// typed_spmm.hip -- gather passes over a graph whose edges carry a TYPE (R-GCN / DGL's RelGraphConv in its basis form): the three
// passes of dgll_amd/ops_typed.py behind ONE entry point, dgll_hip_typed_spmm_pass (include/dgll_hip.h: dgll_typed_desc).
//
//   h_i = sum_{e = (j -> i)} norm_e W_{r_e} x_j,   W_r = sum_b C[r, b] V_b      =>      h_i = sum_b Z[i, b, :] V_b
//   Z[i, b, :] = sum_e norm_e C[r_e, b] x_j                                              (Z: [n_rows, B * F], basis-major blocks of width F)
//
// The product with the stacked bases is a dense transform (dense.py); what is sparse is Z, and it is ONE gather: x_j is loaded once
// per edge and feeds B fp32 accumulators, where B weighted SpMMs would gather it B times from B per-edge value vectors.
//
//   expand    rows of A     gathers x_j; coefficient norm_e C[r_e, b]                        -> Z
//   contract  rows of A^T   gathers dZ[i, 0 : B F] (etype / norm in A^T's entry order)       -> dX[j, :] = sum_e norm_e sum_b C[r_e, b] dZ[i_e, b, :]
//   dots      rows of A     holds dZ[i, :, :]; gathers x_j                                   -> P[e, b] = <x_j, dZ[i, b, :]>  (fp32, norm NOT applied)
//
// Lane layout, tiles, index batches and the long-row merge: row_tiles.hpp.  Here a row's `lpr` lanes are at least its F / EPV vectors,
// and a batch hands round types and norms with the indices.  Rows wider than 64 lanes are cut into column blocks of 64 vectors over
// blockIdx.y (expand, contract) or swept block after block by the same lanes (dots: a dot product spans the blocks, and the lane
// that wrote P[e, b] adds the next block's share to it).  Bases are taken kBasisBlock or fewer at a time (compile-time block sizes
// 1, 2, 4, 8: BB x EPV accumulators per lane, in registers); more bases are further blocks over blockIdx.z, each of which gathers
// x_j again.  The long-row merge moves kMergeSlice floats of the state at a time.  The coefficient table is staged in LDS when its
// R * B entries fit kCoeffLds floats and read from global memory (L2-resident) otherwise.  The type used for addressing is clamped
// to [0, R) and the column to [0, n_cols): a corrupt buffer gives a wrong number, not a fault.
#include "row_tiles.hpp"
#include "edge_args.hpp"

namespace dgll {
namespace typed {

constexpr int kLongRow = DGLL_TYPED_LONG_ROW;       // rows longer than this are swept by a whole workgroup
constexpr int kCoeffLds = DGLL_TYPED_COEFF_LDS;     // the coefficient table goes through LDS when R * B <= this many floats (16 KB)
constexpr int kBasisBlock = DGLL_TYPED_BASIS_BLOCK; // bases per launch block at the most
constexpr int kMergeSlice = 16;                     // floats of a lane's state that cross LDS at a time in the long-row merge (16 KB)

struct Args {
    const int64_t* rowptr;
    const int32_t* col;
    const int32_t* etype;                   // [nnz] in the pass's entry order (expand, contract)
    const float* norm;                      // [nnz] or NULL (expand, contract)
    const float* coeff;                     // [R, B]
    int64_t n_rows, n_cols, tiles;
    const char* x;   int64_t pb_x;          // the gathered matrix: X (expand, dots), dZ (contract); pitches in BYTES
    const char* h;   int64_t pb_h;          // dots: the held matrix dZ
    char* out;       int64_t pb_out;        // expand: Z; contract: dX
    float* p;        int64_t ld_p;          // dots: P [nnz, ld_p]
    int64_t fb;                             // bytes of one basis block of a row of Z / dZ: F * sizeof(T)
    int R, B, vpr, lpr, chunks, staged;     // vpr: 16-byte vectors of F columns; chunks: column blocks of lpr vectors (dots)
};

// KIND 0 expand, 1 contract, 2 dots.  BB: bases of this block (contract: unused, 1).  State of one lane, flat so that the long-row
// merge can move it through LDS: expand st[k * EPV + d] = Z[row, b0 + k, lane's column d]; contract st[d] = dX[row, lane's column d].
template <typename T, int KIND, int BB>
__global__ __launch_bounds__(kBlock) void typed_spmm_kernel(const Args a) {
    constexpr int EPV = 16 / (int)sizeof(T), NP = (KIND == 1 ? 1 : BB) * EPV, MS = NP < kMergeSlice ? NP : kMergeSlice, U = 2;
    using IO = VecIO<T, EPV>;
    __shared__ float tab[KIND == 2 ? 1 : kCoeffLds];
    __shared__ float lds[KIND == 2 ? 1 : MS * kBlock];

    const rt::Lanes lanes(a.lpr);
    const int tid = lanes.tid, lpr = lanes.lpr, groups = lanes.groups, sub = lanes.sub, gid = lanes.gid;
    const int B = a.B, b0 = KIND == 1 ? 0 : (int)blockIdx.z * BB;
    const int nbk = B - b0 < BB ? B - b0 : BB;              // bases of this block that exist
    const bool staged = a.staged != 0;

    if constexpr (KIND != 2) {
        if (staged) {
            for (int i = tid; i < a.R * B; i += kBlock) tab[i] = a.coeff[i];
            __syncthreads();
        }
    }
    auto coeff_at = [&](int i) { return staged ? tab[i] : a.coeff[i]; };

    // the lane's 16-byte vector of the current column block
    bool active = false;
    int64_t cb = 0;                                         // byte offset of the lane's columns inside a basis block
    auto set_chunk = [&](int ch) {
        const int v = ch * lpr + sub;                       // (more than one column block: lpr == 64)
        active = v < a.vpr;
        cb = active ? (int64_t)v * 16 : 0;
    };

    float st[NP];
    float held[KIND == 2 ? NP : 1];                         // dots: dZ[row, b0 + k, lane's columns]

    auto load_row = [&](int64_t row, bool on) {
#pragma unroll
        for (int k = 0; k < NP; ++k) st[k] = 0.0f;
        if constexpr (KIND == 2) {
#pragma unroll
            for (int k = 0; k < BB; ++k) {
                typename IO::raw_t r = IO::zero();
                if (on && active && k < nbk) r = IO::load(reinterpret_cast<const T*>(a.h + row * a.pb_h + (int64_t)(b0 + k) * a.fb + cb));
                float f[EPV];
                IO::unpack(r, f);
#pragma unroll
                for (int d = 0; d < EPV; ++d) held[k * EPV + d] = f[d];
            }
        }
    };

    // the row's entries [b, e), the batches first, first + stride, ... of them, two entries in flight.  rt::for_each_batch written out:
    // through the header the loop's branches come out inverted, and CONTRACT measured 2.7 % slower at one shape.
    auto sweep = [&](int64_t b, int64_t e, int first, int stride, bool first_chunk) {
        const int total = (int)((e - b + lpr - 1) / lpr);
        const int mine = first < total ? (total - first + stride - 1) / stride : 0;
        const int max_batches = rt::wave_max(mine);
        for (int it = 0; it < max_batches; ++it) {
            const int64_t k0 = b + ((int64_t)first + (int64_t)it * stride) * lpr;
            int nb = 0;
            if (it < mine) nb = e - k0 < lpr ? (int)(e - k0) : lpr;
            int my_col = 0, my_type = 0;
            float my_w = 0.0f;
            if (sub < nb) {
                my_col = a.col[k0 + sub];
                if constexpr (KIND != 2) {
                    my_type = a.etype[k0 + sub];
                    my_w = a.norm ? a.norm[k0 + sub] : 1.0f;
                }
            }
            my_col = rt::clamp_index(my_col, (int)a.n_cols);
            my_type = rt::clamp_index(my_type, a.R) * B;        // a corrupt type: a wrong row of C, never outside it
            const int max_nb = rt::wave_max(nb);
            for (int t = 0; t < max_nb; t += U) {
                int64_t c[U];
                int ty[U];
                float w[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    c[u] = rt::hand_round(my_col, t + u, lanes);
                    ok[u] = t + u < nb;
                    ty[u] = 0;
                    w[u] = 0.0f;
                    if constexpr (KIND != 2) {
                        ty[u] = rt::hand_round(my_type, t + u, lanes);
                        w[u] = rt::hand_round(my_w, t + u, lanes);
                    }
                }
                if constexpr (KIND == 1) {
                    for (int bb = 0; bb < B; ++bb) {
                        typename IO::raw_t r[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            r[u] = IO::zero();
                            if (ok[u] && active) r[u] = IO::load(reinterpret_cast<const T*>(a.x + c[u] * a.pb_x + (int64_t)bb * a.fb + cb));
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float cf = ok[u] ? w[u] * coeff_at(ty[u] + bb) : 0.0f;
                            float f[EPV];
                            IO::unpack(r[u], f);
#pragma unroll
                            for (int d = 0; d < EPV; ++d) st[d] = fmaf(cf, f[d], st[d]);
                        }
                    }
                } else {
                    typename IO::raw_t r[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        r[u] = IO::zero();
                        if (ok[u] && active) r[u] = IO::load(reinterpret_cast<const T*>(a.x + c[u] * a.pb_x + cb));
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float f[EPV];
                        IO::unpack(r[u], f);
                        if constexpr (KIND == 0) {
#pragma unroll
                            for (int k = 0; k < BB; ++k) {
                                const float cf = ok[u] && k < nbk ? w[u] * coeff_at(ty[u] + b0 + k) : 0.0f;
#pragma unroll
                                for (int d = 0; d < EPV; ++d) st[k * EPV + d] = fmaf(cf, f[d], st[k * EPV + d]);
                            }
                        } else {
                            // a masked slot loaded zeros: its dots are 0 and nothing is written.  The dots of the group's lanes are
                            // summed by a butterfly (every lane ends with the sum); lane k of the group owns P[e, b0 + k].
                            const int64_t e_at = k0 + t + u;
#pragma unroll
                            for (int k = 0; k < BB; ++k) {
                                float dot = 0.0f;
#pragma unroll
                                for (int d = 0; d < EPV; ++d) dot = fmaf(f[d], held[k * EPV + d], dot);
                                for (int off = 1; off < lpr; off <<= 1) dot += __shfl_xor(dot, off);
                                if (ok[u] && sub == k && k < nbk) {
                                    float* dst = a.p + e_at * a.ld_p + b0 + k;
                                    *dst = first_chunk ? dot : *dst + dot;
                                }
                            }
                            // the padding columns of P: zeros, written once by the last basis block
                            if (ok[u] && first_chunk && blockIdx.z + 1 == gridDim.z && sub < (int)a.ld_p - B) a.p[e_at * a.ld_p + B + sub] = 0.0f;
                        }
                    }
                }
            }
        }
    };

    // the row's outputs from its complete state; no cross-lane traffic (the long-row path calls it from one lane group alone)
    auto finish = [&](int64_t row) {
        if constexpr (KIND == 2) return;
        if (!active) return;
        if constexpr (KIND == 0) {
#pragma unroll
            for (int k = 0; k < BB; ++k) {
                if (k < nbk) {
                    float o[EPV];
#pragma unroll
                    for (int d = 0; d < EPV; ++d) o[d] = st[k * EPV + d];
                    IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + (int64_t)(b0 + k) * a.fb + cb), o);   // an empty row: zeros
                }
            }
        } else if constexpr (KIND == 1) {
            float o[EPV];
#pragma unroll
            for (int d = 0; d < EPV; ++d) o[d] = st[d];
            IO::store(reinterpret_cast<T*>(a.out + row * a.pb_out + cb), o);                                       // a row nobody references: zeros
        }
    };

    const int ch0 = KIND == 2 ? 0 : (int)blockIdx.y, ch1 = KIND == 2 ? a.chunks : ch0 + 1;
    // The tile loop and the long-row merge are rt::for_each_tile and rt::merge_partials written out, with the chunk loop between tile
    // and rows and the state crossing LDS in slices: called through the header, these kernels' register counts move.
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row0 = tile * groups;
        for (int ch = ch0; ch < ch1; ++ch) {
            set_chunk(ch);
            {   // rows of at most kLongRow entries: one per lane group
                const int64_t row = row0 + gid;
                int64_t b = 0, e = 0;
                if (row < a.n_rows) { b = a.rowptr[row]; e = a.rowptr[row + 1]; }
                const bool mine = row < a.n_rows && e - b <= kLongRow;
                if (!mine) e = b;
                load_row(mine ? row : 0, mine);
                sweep(b, e, 0, 1, ch == 0);
                if (mine) finish(row);
            }
            for (int r = 0; r < groups; ++r) {      // longer rows: the whole workgroup, one row after another (all conditions block-uniform)
                const int64_t row = row0 + r;
                if (row >= a.n_rows) break;
                const int64_t b = uniform64(a.rowptr[row]), e = uniform64(a.rowptr[row + 1]);
                if (e - b <= kLongRow) continue;
                load_row(row, true);
                sweep(b, e, gid, groups, ch == 0);
                if constexpr (KIND != 2) {          // (dots: every entry's result is already in P)
#pragma unroll
                    for (int s0 = 0; s0 < NP; s0 += MS) {
                        __syncthreads();            // the previous merge has read its partials
#pragma unroll
                        for (int k = 0; k < MS; ++k) lds[k * kBlock + tid] = st[s0 + k];
                        __syncthreads();
                        if (tid < lpr) {            // the first lane group (sub == tid) merges the others in group order
                            for (int p = 1; p < groups; ++p) {
#pragma unroll
                                for (int k = 0; k < MS; ++k) st[s0 + k] += lds[k * kBlock + p * lpr + tid];
                            }
                        }
                    }
                    if (tid < lpr) finish(row);
                }
            }
        }
    }
}

template <typename T, int KIND>
bool launch_kind(int bb, dim3 grid, hipStream_t s, const Args& a) {
    if constexpr (KIND == 1) {
        hipLaunchKernelGGL((typed_spmm_kernel<T, 1, 1>), grid, dim3(kBlock), 0, s, a);
        return true;
    } else {
        if (bb == 1) hipLaunchKernelGGL((typed_spmm_kernel<T, KIND, 1>), grid, dim3(kBlock), 0, s, a);
        else if (bb == 2) hipLaunchKernelGGL((typed_spmm_kernel<T, KIND, 2>), grid, dim3(kBlock), 0, s, a);
        else if (bb == 4) hipLaunchKernelGGL((typed_spmm_kernel<T, KIND, 4>), grid, dim3(kBlock), 0, s, a);
        else if (bb == 8) hipLaunchKernelGGL((typed_spmm_kernel<T, KIND, 8>), grid, dim3(kBlock), 0, s, a);
        else return false;
        return true;
    }
}

template <typename T>
bool launch(int pass, int bb, dim3 grid, hipStream_t s, const Args& a) {
    if (pass == DGLL_TYPED_EXPAND) return launch_kind<T, 0>(bb, grid, s, a);
    if (pass == DGLL_TYPED_CONTRACT) return launch_kind<T, 1>(bb, grid, s, a);
    return launch_kind<T, 2>(bb, grid, s, a);
}

}  // namespace typed
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_typed_spmm_pass(void* stream, const dgll_typed_desc* d) {
    static const char* const kPass = "dgll_hip_typed_spmm_pass";
    DGLL_REQUIRE(d != nullptr, "dgll_hip_typed_spmm_pass: the pass descriptor must be non-NULL");
    DGLL_REQUIRE(d->pass == DGLL_TYPED_EXPAND || d->pass == DGLL_TYPED_CONTRACT || d->pass == DGLL_TYPED_EDGE_DOTS,
                 "dgll_hip_typed_spmm_pass: pass must be DGLL_TYPED_EXPAND, DGLL_TYPED_CONTRACT or DGLL_TYPED_EDGE_DOTS");
    DGLL_REQUIRE(d->dtype == DGLL_F32 || d->dtype == DGLL_BF16, "dgll_hip_typed_spmm_pass: dtype must be DGLL_F32 or DGLL_BF16");
    const auto [epv, esz] = rt::storage_of(d->dtype);
    DGLL_REQUIRE(d->R >= 1 && d->B >= 1 && (int64_t)d->R * d->B < (1ll << 31),
                 "dgll_hip_typed_spmm_pass: R >= 1 edge types, B >= 1 bases, R * B < 2^31");
    DGLL_REQUIRE(d->F >= epv && d->F % epv == 0, "dgll_hip_typed_spmm_pass: F a positive multiple of the 16-byte vector width (4 fp32, 8 bf16 columns)");
    const int64_t vpr = d->F / epv, wide = (int64_t)d->B * d->F;
    DGLL_REQUIRE(vpr <= (int64_t)kWave * 65535 && wide < (1ll << 31),
                 "dgll_hip_typed_spmm_pass: F at most 64 * 65535 vectors and B * F < 2^31");
    DGLL_REQUIRE(d->n_rows >= 0 && d->n_rows < (1ll << 31) && d->n_cols > 0 && d->n_cols < (1ll << 31),
                 "dgll_hip_typed_spmm_pass: row count in [0, 2^31), gathered row count in [1, 2^31)");
    DGLL_REQUIRE(d->rowptr && d->col, "dgll_hip_typed_spmm_pass: the CSR arrays must be non-NULL");
    const bool dots = d->pass == DGLL_TYPED_EDGE_DOTS, contract = d->pass == DGLL_TYPED_CONTRACT;
    if (!dots) {
        DGLL_REQUIRE(d->etype && d->coeff, "dgll_hip_typed_spmm_pass: expand / contract: etype and coeff must be non-NULL");
        DGLL_REQUIRE_OPERAND(kPass, out, contract ? d->F : d->B * d->F);
    }
    if (!contract) DGLL_REQUIRE_OPERAND(kPass, x, d->F);
    if (d->pass != DGLL_TYPED_EXPAND) DGLL_REQUIRE_OPERAND(kPass, dz, d->B * d->F);
    if (dots) {
        DGLL_REQUIRE(d->p && d->ld_p == ((int64_t)d->B + 3) / 4 * 4, "dgll_hip_typed_spmm_pass: p non-NULL with pitch ld_p = B rounded up to 4");
    }

    typed::Args a;
    a.rowptr = d->rowptr;
    a.col = d->col;
    a.etype = d->etype;
    a.norm = d->norm;
    a.coeff = d->coeff;
    a.n_rows = d->n_rows;
    a.n_cols = d->n_cols;
    a.x = static_cast<const char*>(contract ? d->dz : d->x);
    a.pb_x = (contract ? d->ld_dz : d->ld_x) * esz;
    a.h = static_cast<const char*>(d->dz);
    a.pb_h = d->ld_dz * esz;
    a.out = static_cast<char*>(d->out);
    a.pb_out = d->ld_out * esz;
    a.p = d->p;
    a.ld_p = d->ld_p;
    a.fb = d->F * esz;
    a.R = d->R;
    a.B = d->B;
    a.vpr = (int)vpr;
    const rt::HeadGeometry geo = rt::make_flat_geometry(vpr, d->n_rows);
    rt::set_geometry(a, geo);
    a.chunks = geo.col_blocks;
    a.staged = (int64_t)d->R * d->B <= typed::kCoeffLds ? 1 : 0;
    if (geo.grid == 0) return DGLL_OK;
    // bases per block: the smallest compiled size that holds B, kBasisBlock for more (B <= 8 * 65535)
    int bb = 1;
    while (bb < typed::kBasisBlock && bb < d->B) bb <<= 1;
    const int64_t gz = contract ? 1 : ((int64_t)d->B + bb - 1) / bb;
    dim3 grid;
    if (const int rc = rt::launch_grid(kPass, geo.grid, dots ? 1 : geo.col_blocks, gz, grid)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool found = d->dtype == DGLL_F32 ? typed::launch<float>(d->pass, bb, grid, st, a) : typed::launch<bf16_t>(d->pass, bb, grid, st, a);
    DGLL_REQUIRE(found, "dgll_hip_typed_spmm_pass: no kernel for this basis block size");
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
