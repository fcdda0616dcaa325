// gat_choice.hpp -- which kernel, in which geometry, a launch of the fused GAT passes gets: gat_choose() decides, and nothing else
// does.  Plain values in, plain values out: no pointer is dereferenced and no device touched, so dgll_hip_debug_gat_choice() shows
// the choice without a GPU (tests/test_gat_choice_host.py).  Included by edge.hip (the launch path) and spmm.hip (the knob).
#pragma once
#include <algorithm>

#include "edge_args.hpp"

namespace dgll {

enum GatPass { kGatForward = 0, kGatRows = 1, kGatTransposed = 2 };          // over the rows of A, of A again, of A^T
enum { kGatFinalizeNone = 0, kGatFinalizeWave = 1, kGatFinalizeGroup = 2 };   // GatChoice::finalize

// What a launch is, as far as the choice goes.
struct GatLaunchDesc {
    GatPass pass;
    int dtype, heads, fo, mode;
    bool edge_scale;            // an [nnz, heads] multiplier array is given
    bool rowscore;              // forward / rows pass: t_j formed from the gathered row (attn2 INSTEAD of T)
    bool drop;                  // attention dropout drawn in the kernel
    GatRowsPhase phase;         // rows pass only
    int t_stride;               // floats per node of the gathered-side score arrays (T; transposed pass: S and dd of the columns)
    bool t_aligned16, dd_aligned16;   // those arrays are 16-byte aligned (true for one that is not given)
    bool sd_out;                // rows pass: {s_i, dd_i} are written side by side
    bool score_epilogue;        // transposed pass: a1 / a2 given, the scores' own share of grad_H is added in the epilogue
    // the gathered-side scores and the gathered rows, as the in-row form needs them:
    bool score_behind_row;      // the first score array starts exactly behind the last column of the first gathered row
    bool score_pitch_equal;     // t_stride floats are as many bytes as a gathered row's pitch
    bool second_follows;        // the second array (dd; transposed pass) sits one float after the first (true if there is none)
    int64_t pad_bytes;          // bytes between a gathered row's last column and the next row
    bool has_plan;
    int64_t n_rows, nnz, n_chunks, n_long;   // rows of the launch; nnz / n_chunks / n_long are the plan's (0 without one)
    bool y_aligned;             // the output matrix admits the wavefront finalize kernel's four-column stores
};

// Tuning knobs (diagnostics; defaults are the shipped configuration).  Set through dgll_hip_debug_tune(key, value).
struct GatTune {
    int gen = 0;                // key 9: 1 = first-generation GAT kernels only, 2 = second generation without the in-row form
};
extern GatTune g_gat_tune;      // edge.hip

typedef dgll_gat_choice GatChoice;   // include/dgll_hip.h: dgll_hip_debug_gat_choice() hands it out as it is

// Second-generation instantiations (gat_*.hip), [KIND][TROW][DROP]: the rows pass has the row-score form and dropout in its exact
// form (KIND 3) only, the transposed pass gathers DN rows, whose scores cannot be formed from them.
constexpr bool kGat2Exists[4][2][2] = {{{true, true}, {true, true}}, {{true, false}, {false, false}},
                                       {{true, true}, {false, false}}, {{true, true}, {true, true}}};

// The rule, in the order it is applied:
//   second generation (gat2_kernel)   sparseGatConv's form -- exp(-leakyrelu), no max subtraction (mode 0), no attention-dropout
//                                     multiplier ARRAY (dropout drawn in the kernel is theirs) -- for any per-head width of up to
//                                     64 16-byte vectors: `nh` heads per wavefront on `lpr` = nh * lanes-per-head lanes per row
//   ... its in-row form (INROW)       one head whose gathered-side scores sit right behind the last column of the gathered rows
//                                     (same pitch) and a lane of the row's group idle: the gather itself brings them along
//   first generation (edge.hip)       everything else (mode 1, edge_scale, key 9 = 1): per-head width a power-of-two number of
//                                     vectors, compact scores, no row-score form, no in-kernel dropout, no score-gradient epilogue
// A refusal carries the error code and the text the launch path reports ("[..]": the condition as the text has always quoted it).
static GatChoice gat_choose(const GatLaunchDesc& d, const GatTune& t) {
    GatChoice c{};
    const auto refuse = [&c](int code, const char* message) { c.error = code; c.message = message; return c; };
    const int esz = d.dtype == DGLL_BF16 ? 2 : 4, feat = d.heads * d.fo;
    c.epv = 16 / esz;
    const int vph = d.fo / c.epv;         // 16-byte vectors a head really uses
    c.kind = d.pass == kGatForward ? 0 : d.pass == kGatTransposed ? 2 : d.phase >= kGatRowsExactOnly ? 3 : 1;
    c.trow = d.rowscore;
    c.drop = d.drop;
    int lph = 1;
    while (lph < vph) lph <<= 1;
    if (t.gen != 1 && !d.edge_scale && d.mode == 0 && lph <= kWave) {
        if (!kGat2Exists[c.kind][c.trow][c.drop]) return refuse(DGLL_ERR_UNSUPPORTED, "no second-generation GAT kernel for this head layout");
        c.generation = 2;
        c.unroll = 4;
        // blocks of 4 / 8 heads are read as float4s: whole blocks, 16-byte aligned
        // (row-score form: no score row is read at all)
        const bool vec = d.heads % 4 == 0 && (d.rowscore || (d.t_stride % 4 == 0 && d.t_aligned16)) && d.dd_aligned16;
        int n = 1;
        for (int cand = 8; cand >= 1; cand >>= 1) {
            if (cand * lph > kWave) continue;
            if (cand > 2 && !(vec && d.heads % cand == 0)) continue;
            if (cand > 1 && cand / 2 >= d.heads) continue;      // would leave half the wavefront's heads idle
            n = cand;
            break;
        }
        while (n * lph < 4) lph <<= 1;                           // at least 4 lanes per row slot (idle lanes inside a head)
        c.lpr = n * lph; c.nh = n; c.lph = lph; c.grid_y = (d.heads + n - 1) / n;
        // the in-row form: the group's first idle lane fetches the score slot (transposed pass: s and dd, 8 bytes); it has no
        // row-score and no dropout instantiation, and key 9 = 2 switches it off
        c.inrow = t.gen != 2 && !c.trow && !c.drop && n == 1 && d.heads == 1 && vph < c.lpr && d.score_behind_row &&
                  d.score_pitch_equal && d.second_follows && d.pad_bytes >= (d.pass == kGatTransposed ? 8 : 4);
    } else {
        if (d.pass == kGatRows && (d.rowscore || d.drop))
            return refuse(DGLL_ERR_INVALID, "the row-score form and in-kernel dropout need the second-generation kernels [!attn2 && !drop]");
        if (d.drop) return refuse(DGLL_ERR_UNSUPPORTED, "no second-generation GAT kernel with dropout for this head layout");
        if (d.rowscore) return refuse(DGLL_ERR_UNSUPPORTED, "no row-score GAT kernel for this head layout");
        if ((vph & (vph - 1)) != 0 || vph > 64)
            return refuse(DGLL_ERR_INVALID, "per-head width / vector must be a power of two <= 64 for the max-subtracted / dropout form "
                                            "(pad on the host) [(*lph & (*lph - 1)) == 0 && *lph <= 64]");
        if (d.t_stride != d.heads || d.sd_out)
            return refuse(DGLL_ERR_UNSUPPORTED, "strided score arrays need the second-generation kernels (mode 0, no attention dropout)");
        if (d.score_epilogue) return refuse(DGLL_ERR_INVALID, "the score-gradient epilogue needs the second-generation kernels [!attn1]");
        c.generation = 1;
        c.unroll = d.pass == kGatForward ? 4 : 2;
        const int vecs = feat / c.epv;
        c.lph = vph; c.nh = 0;
        c.lpr = 4;
        while (c.lpr < 64 && c.lpr < vecs) c.lpr <<= 1;
        c.lpr = std::max(c.lpr, c.lph);
        c.grid_y = (vecs + c.lpr - 1) / c.lpr;
    }
    // long-row schedule of the plan: chunk items first in the grid, then the rows, several per wavefront
    c.rows_per_wave = 1;
    if (d.has_plan) {
        c.chunk_blocks = (d.n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
        // as in spmm.hip: ~96 KiB of gathered bytes per wavefront
        const double row_bytes = (double)d.nnz / (double)std::max<int64_t>(d.n_rows, 1) * feat * (double)esz;
        c.rows_per_wave = std::min(std::max(row_bytes > 0 ? (int)(98304.0 / row_bytes) : 8, 1), 8);
    }
    const int64_t waves = (d.n_rows + c.rows_per_wave - 1) / c.rows_per_wave;
    c.row_blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    // long rows are summed up by a second launch: one wavefront per row (four columns per store: the rows pass writes fp32
    // scalars only, elsewhere the output rows must admit it), or a workgroup per row
    if (d.has_plan && d.n_long > 0)
        c.finalize = d.heads <= kWave && (d.pass == kGatRows || d.y_aligned) ? kGatFinalizeWave : kGatFinalizeGroup;
    return c;
}

}  // namespace dgll
