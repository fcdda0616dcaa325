// row_tiles.hpp -- the row-tile skeleton of the gather passes that keep a flat per-lane state: gatv2.hip, sparse_attn.hip, typed_spmm.hip,
// mp_ops.hip, multi_agg.hip, edge_feat.hip.  Each of them supplies its own math (load a row, add one batch of entries, finish a row);
// the rest is here, once: on the device the lanes, the batch and tile loops, the long-row merge and the row sweep that ties them
// together (sweep_rows / reduce_rows); on the host the prologue of a descriptor entry point (storage_of, require_head_pass /
// require_flat_pass, DGLL_REQUIRE_OPERAND, make_head_geometry / make_flat_geometry, set_geometry, launch_grid).  What a file still
// writes out, because through the header its instruction text changes (each says so at the place):
//   typed_spmm.hip   the batch loop, the tile loop with the chunk loop inside, and the sliced merge
//   mp_ops.hip       mp_edge_kernel: the head-block loop sits outside its two sweeps of a row; mp_node_kernel<*, 1> (dots): the row sweep
//   multi_agg.hip    magg_forward_kernel: the row sweep (its long-row end is three LDS exchanges of its own)
// and, in every kernel, the few lines that decode the lane's columns (hl / v / head / active / cb): as a shared helper they moved
// register counts.
//
// Lane layout: a lane owns one 16-byte vector of columns, a row `lpr` adjacent lanes (a power of two >= 8; the lanes past the row's
// vectors idle), a wavefront 64 / lpr rows at a time.  A workgroup takes tiles of `groups` = 4 * 64 / lpr consecutive rows, grid-stride:
// every lane group sweeps its own row -- indices read lpr at a time, coalesced, and handed round the group by __shfl -- then the rows
// of the tile longer than `long_row` are taken by the whole workgroup one after another: lane group k takes index batches k,
// k + groups, ... and the partial states are merged through LDS in group order by the first group.  No atomics: two runs give the
// same bits.  The attention passes put `hpb` whole heads of `lph` lanes each into a row's lanes (HeadGeometry).
#pragma once
#include <string>
#include <type_traits>

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

// The row sweep a gather kernel ends with.  begin(row, b, e, on) sets up the lane's state for a row (!on: no such row for this lane
// group -- row = 0, b == e -- so it loads nothing); batch(k0, nb) adds one index batch; short_done(row, b, e) ends a row of at most
// `longer_than` entries, in the lane group that swept it; long_done(row, b, e) ends a longer one, in every lane of the workgroup, each
// lane group holding the partial state of its share of the batches.
template <typename Begin, typename Batch, typename ShortDone, typename LongDone>
__device__ __forceinline__ void sweep_rows(int64_t tiles, int64_t n_rows, const int64_t* rowptr, int longer_than, const Lanes& L,
                                           Begin&& begin, Batch&& batch, ShortDone&& short_done, LongDone&& long_done) {
    auto short_row = [&](int64_t row, bool mine, int64_t b, int64_t e) {
        begin(row, b, e, mine);
        for_each_batch(b, e, 0, 1, L, batch);
        if (mine) short_done(row, b, e);
    };
    auto long_row = [&](int64_t row, int64_t b, int64_t e) {
        begin(row, b, e, true);
        for_each_batch(b, e, L.gid, L.groups, L, batch);
        long_done(row, b, e);
    };
    for_each_tile(tiles, n_rows, rowptr, longer_than, L, short_row, long_row);
}

// ... of a pass that leaves nothing to do at the end of a row (every entry's result is stored by its batch)
template <typename Begin, typename Batch>
__device__ __forceinline__ void sweep_rows(int64_t tiles, int64_t n_rows, const int64_t* rowptr, int longer_than, const Lanes& L,
                                           Begin&& begin, Batch&& batch) {
    auto nothing = [](int64_t, int64_t, int64_t) {};
    sweep_rows(tiles, n_rows, rowptr, longer_than, L, begin, batch, nothing, nothing);
}

// ... of a pass that reduces a row into the flat state st: finish(row, b, e) writes the row from its complete state, after
// merge_partials for a long row.
template <bool SOFTMAX, int NP, typename Begin, typename Batch, typename Finish>
__device__ __forceinline__ void reduce_rows(int64_t tiles, int64_t n_rows, const int64_t* rowptr, int longer_than, const Lanes& L,
                                            float (&st)[NP], float* lds, Begin&& begin, Batch&& batch, Finish&& finish) {
    auto long_done = [&](int64_t row, int64_t b, int64_t e) { merge_partials<SOFTMAX>(st, lds, L, [&] { finish(row, b, e); }); };
    sweep_rows(tiles, n_rows, rowptr, longer_than, L, begin, batch, finish, long_done);
}

// ---- host side: the prologue of a descriptor entry point -----------------------------------------------------------------------
struct Storage {
    int epv;                                    // elements of a 16-byte lane vector
    int64_t esz;                                // bytes of an element
};
inline Storage storage_of(int dtype) { return dtype == DGLL_F32 ? Storage{4, 4} : Storage{8, 2}; }

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

// The passes whose rows are F columns without heads (vpr = F / epv vectors): a row's lanes are the smallest power of two that holds
// its vectors, 64 at the most, and wider rows are cut into column blocks of 64 vectors.
inline HeadGeometry make_flat_geometry(int64_t vpr, int64_t n_rows) {
    HeadGeometry g = make_row_geometry(pow2_at_least(vpr < kWave ? vpr : kWave, kMinGroup), n_rows);
    g.col_blocks = (int)((vpr + g.lpr - 1) / g.lpr);
    return g;
}

// the geometry into a kernel's Args: lpr and tiles, and the head fields where the Args have them
template <typename A, typename = void> struct has_heads : std::false_type {};
template <typename A> struct has_heads<A, std::void_t<decltype(A::lph)>> : std::true_type {};
template <typename A>
inline void set_geometry(A& a, const HeadGeometry& g) {
    a.lpr = g.lpr;
    a.tiles = g.tiles;
    if constexpr (has_heads<A>::value) {
        a.vph = g.vph;
        a.lph = g.lph;
        a.hpb = g.hpb;
    }
}

// gridDim of the launch: gx workgroups (the geometry's grid, or the pass's own count) by gy column blocks by gz
inline int launch_grid(const char* pass, int64_t gx, int64_t gy, int64_t gz, dim3& grid) {
    DGLL_REQUIRE(gy <= 65535 && gz <= 65535, std::string(pass) + ": at most 65535 column blocks (of 64 lane vectors or of whole heads) and 65535 basis blocks");
    grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
    return DGLL_OK;
}

// One matrix operand of 16-byte lane vectors, refused under its own name: non-NULL, a 16-byte aligned base, a pitch of whole 16-byte
// vectors >= width (`width_is`: the width in the descriptor's terms).  Use through DGLL_REQUIRE_OPERAND.
inline int require_operand(const char* pass, const char* name, const void* p, int64_t ld, int epv, int64_t width, const char* width_is) {
    const std::string what = std::string(pass) + ": " + name + " non-NULL, 16-byte aligned, pitch ld_" + name + " of whole 16-byte vectors >= " + width_is + ": ";
    DGLL_REQUIRE(p != nullptr, what + name + " must be non-NULL for this pass");
    DGLL_REQUIRE(aligned16(p), what + name + " must be 16-byte aligned");
    DGLL_REQUIRE(ld % epv == 0 && ld >= width, what + "ld_" + name + " is no such pitch");
    return DGLL_OK;
}
// operand `field` of the descriptor d, on the pitch d->ld_<field>; `epv` is the caller's
#define DGLL_REQUIRE_OPERAND(pass, field, width)                                                                        \
    do {                                                                                                                \
        if (const int rc_ = ::dgll::rt::require_operand(pass, #field, d->field, d->ld_##field, epv, width, #width)) return rc_; \
    } while (0)

// what every pass over heads requires of its descriptor's dtype, shape and CSR
inline int require_head_pass(int dtype, int heads, int D, int64_t n_rows, int64_t n_cols, const void* rowptr, const void* col) {
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dtype must be DGLL_F32 or DGLL_BF16");
    const int epv = storage_of(dtype).epv;
    DGLL_REQUIRE(heads >= 1 && D >= epv && D % epv == 0, "heads >= 1 and D a positive multiple of the 16-byte vector width (4 fp32, 8 bf16 columns)");
    DGLL_REQUIRE(D / epv <= kWave, "a head may span at most 64 vectors (D <= 256 fp32, 512 bf16)");
    DGLL_REQUIRE((int64_t)heads * D < (1 << 20), "heads * D < 2^20");
    DGLL_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols > 0 && n_cols < (1ll << 31), "row count in [0, 2^31), gathered row count in [1, 2^31)");
    DGLL_REQUIRE(rowptr && col, "the CSR arrays must be non-NULL");
    return DGLL_OK;
}

// ... and every pass over rows of F columns; nnz: the rows of its per-edge matrices (0 where it has none); col may be NULL in a pass
// that gathers nothing (!gathers)
inline int require_flat_pass(const char* pass, int dtype, int64_t F, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* rowptr,
                             const void* col, bool gathers) {
    const std::string at = std::string(pass) + ": ";
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, at + "dtype must be DGLL_F32 or DGLL_BF16");
    const int epv = storage_of(dtype).epv;
    DGLL_REQUIRE(F >= epv && F % epv == 0 && F < (1ll << 24), at + "F a positive multiple of the 16-byte vector width (4 fp32, 8 bf16 columns), below 2^24");
    DGLL_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && n_cols > 0 && n_cols < (1ll << 31),
                 at + "n_rows in [0, 2^31), n_cols (the gathered rows) in [1, 2^31)");
    DGLL_REQUIRE(nnz >= 0 && nnz < (1ll << 31), at + "nnz (the rows of the per-edge matrices) in [0, 2^31)");
    DGLL_REQUIRE(rowptr != nullptr, at + "the CSR array rowptr must be non-NULL");
    DGLL_REQUIRE(col != nullptr || !gathers, at + "the CSR array col must be non-NULL");
    return DGLL_OK;
}

}  // namespace rt
}  // namespace dgll
