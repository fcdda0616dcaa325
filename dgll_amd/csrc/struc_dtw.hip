// struc_dtw.hip -- struc2vec's structural distances: exact dynamic time warping between the ordered degree sequences of two nodes,
// one distance per (pair, BFS level), in float64.
//
//     D[i][j] = c(i, j) + min(D[i-1][j], D[i][j-1], D[i-1][j-1]),   D[0][0] = 0, the other borders +inf
//     c = ((max(da, db) + 0.5) / (min(da, db) + 0.5) - 1) * max(ca, cb)       (the reference's cost_max; with counts 1 its cost)
//
// One (pair, level) task per wavefront.  The shorter sequence is the rows, the longer one the columns; the columns sit across the
// lanes in strips of 64 and the rows are swept in a skewed order: lane j works on row i at step i + j, so the three cells a cell
// needs are already there -- D[i-1][j] is the lane's own previous value, D[i][j-1] is what the left neighbour computed one step ago
// and D[i-1][j-1] what it computed two steps ago.  Both arrive by one DPP wave shift (wave_shr:1, a VALU move: no LDS round trip)
// per step; the lane keeps last step's shifted value as its diagonal.  The row element a lane needs travels the same way: lane 0
// takes row t at step t through a uniform (scalar) load, issued one step ahead, and hands it on to the right.  Lane 0's left
// neighbour is the last column of the previous strip: that boundary column, one float64 per row, is kept in LDS (lane 63 writes row
// i at step i + 63, lane 0 read it at step i: in place).  A task is a serial chain of steps of one float64 divide each -- (rows +
// strip width - 1) steps per strip -- so the kernel is bound by the divide's latency times the tasks in flight; no atomics, no
// per-lane arrays.
// The LDS boundary column holds kMaxRows rows per wavefront: the SHORTER sequence of a task may have at most kMaxRows = 1024
// entries (the longer one is unbounded).  The Python layer checks this and raises ValueError; a task over the limit is written as
// NaN here and nothing is read or written out of bounds.
// A level is invalid for a pair from the first level at which either node's sequence is empty: -1.
// No fast-math and no contraction in this file: the divide is IEEE and every cell rounds as the host's float64 loop does, and
// since c and min are symmetric d(a, b) and d(b, a) are the same bits.
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)

namespace dgll {
namespace struc {

constexpr int kMaxRows = 1024;

// lane j receives src of lane j - 1; lane 0 keeps `first`
__device__ __forceinline__ int shift_up1(int first, int src) { return __builtin_amdgcn_update_dpp(first, src, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double shift_up1(double first, double src) {
    const int lo = shift_up1(__double2loint(first), __double2loint(src));
    const int hi = shift_up1(__double2hiint(first), __double2hiint(src));
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kBlock) void struc_dtw_kernel(const int64_t* __restrict__ seq_ptr, const int32_t* __restrict__ seq_deg,
                                                           const int32_t* __restrict__ seq_cnt, const int32_t* __restrict__ pairs,
                                                           int64_t n_tasks, int n_levels, double* __restrict__ dist) {
    __shared__ double boundary[kWavesPerBlock][kMaxRows];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t task = uniform64((int64_t)blockIdx.x * kWavesPerBlock + wave);
    if (task >= n_tasks) return;
    const int lane = lane_id();
    const int64_t p = task / n_levels;
    const int level = (int)(task - p * n_levels);
    const int64_t ra = (int64_t)pairs[2 * p] * n_levels, rb = (int64_t)pairs[2 * p + 1] * n_levels;
    bool gap = false;                                                        // an empty level at or below this one, on either side
    for (int l = lane; l <= level; l += kWave) gap |= seq_ptr[ra + l + 1] == seq_ptr[ra + l] || seq_ptr[rb + l + 1] == seq_ptr[rb + l];
    if (__any(gap)) {
        if (lane == 0) dist[task] = -1.0;
        return;
    }
    int64_t ab = seq_ptr[ra + level], bb = seq_ptr[rb + level];
    int64_t m = seq_ptr[ra + level + 1] - ab, n = seq_ptr[rb + level + 1] - bb;
    if (n < m) { int64_t t = ab; ab = bb; bb = t; t = m; m = n; n = t; }   // rows: the shorter sequence
    if (m > kMaxRows) {
        if (lane == 0) dist[task] = nan("");
        return;
    }
    const int32_t* __restrict__ a_deg = seq_deg + ab;
    const int32_t* __restrict__ a_cnt = seq_cnt + ab;
    double* __restrict__ edge = boundary[wave];
    const double inf = __builtin_inf();
    const int rows = (int)m;
    double cur = inf;
    int width = 0;
    for (int64_t j0 = 0; j0 < n; j0 += kWave) {
        width = (int)(n - j0 < kWave ? n - j0 : kWave);
        const bool first_strip = j0 == 0, more = j0 + kWave < n;
        const bool active = lane < width;
        const int db = active ? seq_deg[bb + j0 + lane] : 0, cb = active ? seq_cnt[bb + j0 + lane] : 0;
        cur = inf;                                                           // D[-1][j]
        double diag = (first_strip && lane == 0) ? 0.0 : inf;                // D[-1][j-1]
        int da = 0, ca = 0;
        int next_deg = a_deg[0], next_cnt = a_cnt[0];
        const int steps = rows + width - 1;
        for (int t = 0; t < steps; ++t) {
            const int row_deg = next_deg, row_cnt = next_cnt;                // row t (the last row again once t >= rows: unused)
            const int ahead = t + 1 < rows ? t + 1 : rows - 1;
            next_deg = a_deg[ahead];
            next_cnt = a_cnt[ahead];
            const double in = (!first_strip && t < rows) ? edge[t] : inf;    // D[t][j0 - 1], lane 0's left neighbour
            const double left = shift_up1(in, cur);
            da = shift_up1(row_deg, da);
            ca = shift_up1(row_cnt, ca);
            const int i = t - lane;
            if (active && i >= 0 && i < rows) {
                const double hi = (double)(da > db ? da : db) + 0.5, lo = (double)(da > db ? db : da) + 0.5;
                const double c = (hi / lo - 1.0) * (double)(ca > cb ? ca : cb);
                cur = c + fmin(fmin(cur, left), diag);
                if (more && lane == kWave - 1) edge[i] = cur;
            }
            diag = left;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // lane 63's boundary column, read by every lane next strip
    }
    const double d = __shfl(cur, width - 1);                                 // D[rows-1][n-1]
    if (lane == 0) dist[task] = d;
}

}  // namespace struc
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_struc_dtw(void* stream, const int64_t* seq_ptr, const int32_t* seq_deg, const int32_t* seq_cnt, int64_t n_nodes,
                                int n_levels, const int32_t* pairs, int64_t n_pairs, double* dist) {
    DGLL_REQUIRE(seq_ptr && (pairs || n_pairs == 0) && (dist || n_pairs == 0), "seq_ptr, pairs and dist must be non-NULL");
    DGLL_REQUIRE(n_nodes > 0 && n_nodes < (1ll << 31) && n_levels >= 1 && n_pairs >= 0, "node count in [1, 2^31), n_levels >= 1");
    DGLL_REQUIRE(n_pairs <= ((1ll << 31) - 1) * kWavesPerBlock / n_levels, "too many (pair, level) tasks for one launch");
    if (n_pairs == 0) return DGLL_OK;
    DGLL_REQUIRE(seq_deg && seq_cnt, "seq_deg and seq_cnt must be non-NULL");
    const int64_t n_tasks = n_pairs * n_levels;
    hipLaunchKernelGGL(struc::struc_dtw_kernel, dim3((unsigned)((n_tasks + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), seq_ptr, seq_deg, seq_cnt, pairs, n_tasks, n_levels, dist);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_struc_dtw_max_rows(void) { return struc::kMaxRows; }
