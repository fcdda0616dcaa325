// transform_choice.hpp -- which kernel, in which geometry, a launch of the bf16 MFMA transform (dense.hip) gets: transform_choose()
// decides, and nothing else does.  Plain values in, plain values out: no pointer is dereferenced and no device touched, so
// dgll_hip_debug_transform_choice() shows the choice without a GPU (tests/test_dense_choice_host.py).  Included by dense.hip (the
// launch path and the export); the knobs are set in spmm.hip (dgll_hip_debug_tune).
#pragma once
#include <algorithm>

#include <stddef.h>
#include <stdint.h>

#include "host_common.hpp"

namespace dgll {

// What a launch is, as far as the choice goes.
struct TransformDesc {
    int N, K1, K2;              // K2 = 0: no second operand pair
    bool mask;                  // an input ReLU mask on the first operand
    bool out_f32, row_scale, addend, out_gate, gate_bits;   // what the epilogue is given
    bool out_aligned;           // the output is 16-byte aligned and ldo % 8 == 0
    bool ldw_equal;             // both weight matrices have one leading dimension (true without a second pair)
    bool dual;                  // dgll_hip_transform_bf16_dual: two products of ONE operand, K2 unused
    int64_t M;
    int n_cu;                   // compute units of the device (<= 0: 256)
};

// Tuning knobs (diagnostics; defaults are the shipped configuration).  Set through dgll_hip_debug_tune(key, value).
struct TransformTune {
    int kperm = 0;              // key 4: 0 = per-shape choice, 1 = 4-wave kernel always, 2 = no chunk rotation
    int per_cu = 0;             // key 11: workgroups per CU of the resident-weights kernel (0 = default)
    int grid_cap = 0;           // key 16: cap on the resident-weights kernel's grid, in workgroups (0 = none)
};

typedef dgll_transform_choice TransformChoice;   // include/dgll_hip.h: dgll_hip_debug_transform_choice() hands it out as it is

constexpr int kTransformChunkK = 64;        // k per LDS stage (both kernels)
constexpr int kTransformWPitch = kTransformChunkK * 2 + 16;   // 4-wave kernel: bytes per weight row in LDS
// shape of the resident-weights kernel's workgroup (probe builds under tools/probes/ override them)
#ifdef DGLL_RES_RG
constexpr int kResRG = DGLL_RES_RG;
#else
constexpr int kResRG = 2;                   // row groups of 32 rows per wave
#endif
#ifdef DGLL_RES_NW
constexpr int kResNW = DGLL_RES_NW;
#else
constexpr int kResNW = 8;                   // waves per workgroup
#endif

// resident-weights kernel for this shape?  nt = 32-column tiles of N, n_chunks = 64-k chunks of K1 + K2
static inline bool res_applies(int nt, int n_chunks) {
    if (n_chunks < 1 || n_chunks > 8) return false;
    if (nt > 4 && n_chunks > 4) return nt <= 8;            // 256 columns x 512 k: two workgroups of 128 columns
    return (size_t)n_chunks * (nt <= 2 ? 2 : nt <= 4 ? 4 : 8) * 32 * 128 <= 128 * 1024;
}

// which epilogue: 1 (plain) loads nothing; 2 = plain + the output gate as bits (fetched a phase ahead); 0 = everything else
static inline int res_epilogue_kind(const TransformDesc& d) {
    const bool simple = !d.out_f32 && !d.row_scale && !d.addend;
    if (simple && !d.out_gate && !d.gate_bits) return 1;
    if (simple && d.gate_bits && d.out_aligned) return 2;
    return 0;
}

// LDS of a resident-weights workgroup: the weights of its columns for the whole reduction, a staging tile per wave, the bias
static inline size_t res_lds_bytes(int ntw, int nc, int cs) {
    const int nwg_t = ntw * cs;
    return (size_t)nc * nwg_t * 32 * 128 + kResNW * 32 * 80 + nwg_t * 32 * 4;
}

// The resident-weights kernel's grid: per_cu workgroups on each of the device's CUs, in whole groups of 16 (8 XCDs x the COLSPLIT
// partners that (bid >> 3) % COLSPLIT pairs up); key 16 caps it for diagnostics -- a workgroup then wraps to its second row block
// after a few thousand rows instead of a few hundred thousand (tests/test_dense_steady_gpu.py).
static inline int res_grid(size_t lds, int n_cu, const TransformTune& t, int* per_cu_out) {
    int n = n_cu > 0 ? n_cu : 256;
    n = n / 16 * 16;                                        // whole groups of 8 XCDs x COLSPLIT partners
    if (n <= 0) n = 16;
    int per_cu = lds > 80 * 1024 ? 1 : 2;
    if (t.per_cu > 0 && (size_t)t.per_cu * lds <= 160 * 1024) per_cu = t.per_cu;   // diagnostics
    int grid = n * per_cu;
    if (t.grid_cap > 0) grid = std::min(grid, std::max(16, t.grid_cap / 16 * 16));
    if (per_cu_out) *per_cu_out = per_cu;
    return grid;
}

// The rule, in the order it is applied (tools/transform_probe.py, M = 2.45 M): the persistent resident-weights kernel wherever the
// weights of the whole reduction fit LDS (K1 + K2 <= 512) -- fused 256+256 -> 256: 0.90 ms against 1.2-1.4 for the 4-wave kernel,
// single 256 -> 256: 0.59 against 0.82, 256 -> 47: 0.37 against 0.40.  The 4-wave kernel keeps the input-mask form, weight
// matrices of two pitches and longer reductions (weights staged per chunk).  The resident kernel's family by output width:
//   N <= 64    NTW 2, CS 1, COLSPLIT 1      one wave per row group, all columns
//   N <= 128   NTW 4, CS 1, COLSPLIT 1
//   N <= 256   NTW 4, CS 2, COLSPLIT 1      K <= 256: two waves per row group (256 rows per block)
//   N <= 256   NTW 4, CS 1, COLSPLIT 2      K <= 512: two workgroups per row block
// The dual form is NTW 4, CS 2, COLSPLIT 2 with the plain epilogue.  A refusal carries the error code and the text the launch path
// reports ("[..]": the condition as the text has always quoted it).
static TransformChoice transform_choose(const TransformDesc& d, const TransformTune& t) {
    TransformChoice c{};
    const auto refuse = [&c](int code, const char* message) { c.error = code; c.message = message; return c; };
    const auto chunks = [](int k) { return (k + kTransformChunkK - 1) / kTransformChunkK; };
    const auto resident = [&](int ntw, int nc, int cs, int colsplit, int epi, bool dual) {
        c.kernel = 1; c.ntw = ntw; c.nc = nc; c.cs = cs; c.colsplit = colsplit; c.epi = epi; c.dual = dual;
        c.rows_per_block = kResNW * 32 * kResRG / cs;
        const size_t lds = res_lds_bytes(ntw, nc, cs);
        c.lds_bytes = (int)lds;
        c.workgroups = res_grid(lds, d.n_cu, t, &c.per_cu);
        c.row_sequences = c.workgroups / colsplit;
        c.n_blocks = (d.M + c.rows_per_block - 1) / c.rows_per_block;
        c.bits_in_epilogue = epi != 0;       // the plain / bit-gated epilogues write the sign bits themselves
    };
    c.nt = d.N <= 64 ? 2 : d.N <= 128 ? 4 : 8;
    if (d.dual) {
        if (!(d.N <= 256 && d.K1 <= 256))
            return refuse(DGLL_ERR_INVALID, "dgll_hip_transform_bf16_dual: N, K <= 256 (both weight matrices stay resident in LDS) "
                                            "[N <= 256 && K <= 256]");
        c.nt = 8;                            // 256 columns per workgroup (two waves per row group), two workgroups per row block
        resident(4, std::min(std::max(chunks(d.K1), 1), 4), 2, 2, 1, true);
        return c;
    }
    if (d.N > 256)
        return refuse(DGLL_ERR_INVALID, "dgll_hip_transform_bf16 keeps all N <= 256 output columns of a row block in accumulators [N <= 256]");
    const int nt = (d.N + 31) / 32;
    const int n_chunks = chunks(d.K1) + (d.K2 > 0 ? chunks(d.K2) : 0);
    const bool res = t.kperm != 1 && !d.mask && res_applies(nt, n_chunks) && (d.K2 <= 0 || d.ldw_equal);
    const int epi = res_epilogue_kind(d);
    // the bits are an ALTERNATIVE reading of the gate: only the resident-weights kernel's bit epilogue takes them; every other path
    // reads out_gate, which must then be there too
    if (d.gate_bits && !d.out_gate && !(res && epi == 2))
        return refuse(DGLL_ERR_INVALID, "gate_bits alone: this shape / operand set runs a kernel that reads the gate as bf16 -- pass out_gate "
                                        "as well [!gate_bits || out_gate || (res && res_epilogue_kind(a) == 2)]");
    if (!res) {                              // one 128-row block per workgroup, the weights staged per chunk (double buffered)
        c.kernel = 0;
        c.rows_per_block = 128;
        c.lds_bytes = 2 * c.nt * 32 * kTransformWPitch;
        c.n_blocks = (d.M + 127) / 128;
        c.workgroups = c.row_sequences = c.n_blocks;
        return c;
    }
    if (nt <= 2) resident(2, n_chunks, 1, 1, epi, false);
    else if (nt <= 4) resident(4, n_chunks, 1, 1, epi, false);
    else if (n_chunks <= 4) resident(4, n_chunks, 2, 1, epi, false);
    else resident(4, n_chunks, 1, 2, epi, false);
    return c;
}

}  // namespace dgll
