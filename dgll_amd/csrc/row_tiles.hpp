// row_tiles.hpp -- the row-tile skeleton of the gather passes that keep a flat per-lane state: gatv2.hip, sparse_attn.hip, typed_spmm.hip.
// Each of them supplies its own math (load a row, add one entry, finish a row); the rest is here, once -- but for the batch loop, the
// tile loop and the sliced merge of typed_spmm.hip, which that file writes out (it says why).
//
// Lane layout: a lane owns one 16-byte vector of columns, a row `lpr` adjacent lanes (a power of two >= 8; the lanes past the row's
// vectors idle), a wavefront 64 / lpr rows at a time.  A workgroup takes tiles of `groups` = 4 * 64 / lpr consecutive rows, grid-stride:
// every lane group sweeps its own row -- indices read lpr at a time, coalesced, and handed round the group by __shfl -- then the rows
// of the tile longer than `long_row` are taken by the whole workgroup one after another: lane group k takes index batches k,
// k + groups, ... and the partial states are merged through LDS in group order by the first group.  No atomics: two runs give the
// same bits.  The attention passes put `hpb` whole heads of `lph` lanes each into a row's lanes (HeadGeometry).
#pragma once
#include "common.hpp"

namespace dgll {
namespace rt {

constexpr int kMinGroup = 8;                // lanes per row at least (index batches of at least 8)
constexpr int64_t kMaxGridX = 1 << 22;      // tiles are taken grid-stride past this
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

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

struct Lanes {
    int tid, lane, wave, lpr, slots, groups;    // groups: lane groups, and rows of a tile, per workgroup
    int sub, gbase, gid;                        // lane of its group, the group's first lane in the wavefront, group of the workgroup
    __device__ __forceinline__ explicit Lanes(int lanes_per_row)
        : tid((int)threadIdx.x), lane(tid & (kWave - 1)), wave(tid / kWave), lpr(lanes_per_row), slots(kWave / lpr),
          groups(kWavesPerBlock * slots), sub(lane & (lpr - 1)), gbase(lane - sub), gid(wave * slots + lane / lpr) {}
};

// Entries [b, e) in batches of lpr; this lane group takes batches first, first + stride, ...: body(k0, nb) with the batch's first entry
// and its size.  Every lane of the wavefront runs every iteration (the trip count is the wavefront's maximum; nb = 0 for a group that
// has run out), and the caller loops to wave_max(nb) inside, so the hand-round shuffles never meet an idle lane.
template <typename Body>
__device__ __forceinline__ void for_each_batch(int64_t b, int64_t e, int first, int stride, const Lanes& L, Body&& body) {
    const int lpr = L.lpr;
    const int total = (int)((e - b + lpr - 1) / lpr);
    const int mine = first < total ? (total - first + stride - 1) / stride : 0;
    const int max_batches = wave_max(mine);
    for (int it = 0; it < max_batches; ++it) {
        const int64_t k0 = b + ((int64_t)first + (int64_t)it * stride) * lpr;
        int nb = 0;
        if (it < mine) nb = e - k0 < lpr ? (int)(e - k0) : lpr;
        body(k0, nb);
    }
}

// an index that addresses with [0, n): a corrupt one reads a wrong row, never outside the matrix
__device__ __forceinline__ int clamp_index(int v, int n) { return min(max(v, 0), n - 1); }

// this lane's index of the batch, clamped
__device__ __forceinline__ int batch_index(const int32_t* idx, int64_t k0, int nb, int n, const Lanes& L) {
    int v = 0;
    if (L.sub < nb) v = idx[k0 + L.sub];
    return clamp_index(v, n);
}

// what lane t of the group read for the batch (slot t of a batch of nb holds an entry when t < nb)
template <typename V>
__device__ __forceinline__ V hand_round(V mine, int t, const Lanes& L) { return __shfl(mine, L.gbase + (t & (L.lpr - 1))); }

// The grid-stride loop over tiles.  short_row(row, mine, b, e): once per tile and lane group, by every lane; !mine (no such row, or a
// long one): row = 0 and b == e.  long_row(row, b, e): once per row longer than `longer_than`, by the whole workgroup.
template <typename Short, typename Long>
__device__ __forceinline__ void for_each_tile(int64_t tiles, int64_t n_rows, const int64_t* rowptr, int longer_than, const Lanes& L,
                                              Short&& short_row, Long&& long_row) {
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * L.groups;
        {
            const int64_t row = row0 + L.gid;
            int64_t b = 0, e = 0;
            if (row < n_rows) { b = rowptr[row]; e = rowptr[row + 1]; }
            const bool mine = row < n_rows && e - b <= longer_than;
            if (!mine) e = b;
            short_row(mine ? row : 0, mine, b, e);
        }
        for (int r = 0; r < L.groups; ++r) {    // all conditions block-uniform
            const int64_t row = row0 + r;
            if (row >= n_rows) break;
            const int64_t b = uniform64(rowptr[row]), e = uniform64(rowptr[row + 1]);
            if (e - b <= longer_than) continue;
            long_row(row, b, e);
        }
    }
}

// The long-row merge: every lane group's state goes through lds (NP * kBlock floats) and the first lane group (sub == tid) adds the
// others to its own in group order -- SOFTMAX: as online-softmax states [0] m (log2 units), [1] l, [2 ..] acc -- then calls done().
template <bool SOFTMAX, int NP, typename Done>
__device__ __forceinline__ void merge_partials(float (&st)[NP], float* lds, const Lanes& L, Done&& done) {
    __syncthreads();                            // the previous merge has read its partials
#pragma unroll
    for (int k = 0; k < NP; ++k) lds[k * kBlock + L.tid] = st[k];
    __syncthreads();
    if (L.tid < L.lpr) {
        for (int p = 1; p < L.groups; ++p) {
            float o[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) o[k] = lds[k * kBlock + p * L.lpr + L.tid];
            if constexpr (SOFTMAX) {
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
        done();
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct HeadGeometry {
    int vph, lph, hpb, col_blocks;              // vectors and lanes of a head; whole heads per column block, and how many of those
    int lpr;                                    // lanes of a row
    int64_t tiles, grid;                        // tiles of the launch, gridDim.x
};

inline int pow2_at_least(int64_t n, int from) {
    while (from < n) from <<= 1;
    return from;
}

inline HeadGeometry make_row_geometry(int lpr, int64_t n_rows) {
    HeadGeometry g{};
    g.lpr = lpr;
    const int groups = kWavesPerBlock * (kWave / lpr);
    g.tiles = (n_rows + groups - 1) / groups;
    g.grid = g.tiles < kMaxGridX ? g.tiles : kMaxGridX;
    return g;
}

inline HeadGeometry make_head_geometry(int heads, int D, int epv, int64_t n_rows) {
    const int vph = D / epv, lph = pow2_at_least(vph, 1), hpb = kWave / lph < heads ? kWave / lph : heads;
    HeadGeometry g = make_row_geometry(pow2_at_least(hpb * lph, kMinGroup), n_rows);
    g.vph = vph;
    g.lph = lph;
    g.hpb = hpb;
    g.col_blocks = (heads + hpb - 1) / hpb;
    return g;
}

// a matrix of 16-byte lane vectors: non-NULL, 16-byte aligned base, a pitch of whole 16-byte vectors >= width
inline bool require_matrix(const void* p, int64_t ld, int epv, int64_t width) { return p && aligned16(p) && ld % epv == 0 && ld >= width; }

// what every pass over heads requires of its descriptor's dtype, shape and CSR
inline int require_head_pass(int dtype, int heads, int D, int64_t n_rows, int64_t n_cols, const void* rowptr, const void* col) {
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype must be DGLL_F32 or DGLL_BF16");
    const int epv = dtype == DGLL_F32 ? 4 : 8;
    DGLL_REQUIRE(heads >= 1 && D >= epv && D % epv == 0, "heads >= 1 and D a positive multiple of the 16-byte vector width (4 fp32, 8 bf16 columns)");
    DGLL_REQUIRE(D / epv <= kWave, "a head may span at most 64 vectors (D <= 256 fp32, 512 bf16)");
    DGLL_REQUIRE((int64_t)heads * D < (1 << 20), "heads * D < 2^20");
    DGLL_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols > 0 && n_cols < (1ll << 31), "row count in [0, 2^31), gathered row count in [1, 2^31)");
    DGLL_REQUIRE(rowptr && col, "the CSR arrays must be non-NULL");
    return DGLL_OK;
}

}  // namespace rt
}  // namespace dgll
