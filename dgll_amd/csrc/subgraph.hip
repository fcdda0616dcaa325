// subgraph.hip -- the subgraph induced by an arbitrary node list, and GraphSAINT's node sets (dgll_amd/sampling/subgraph.py).
//
// The parent is a square CSR over n_total nodes (int64 rowptr, int32 col, optional fp32 val; rows in any order, parallel entries
// allowed); nodes int64[M] in any order names the subgraph's rows: row i of the output is row nodes[i] of the parent with the entries
// whose column is in the list, in the parent's order, the column rewritten to its position in the list.
//   dgll_hip_sg_count   mark    a lane per node: tag[nodes[i]] = epoch << 32 | i by a 64-bit atomic exchange.  ONE 8-byte word per
//                               node holds "selected in this call" and the local id, so an entry of a selected row costs one random
//                               gather; the tags start zeroed, are never cleared, and every call brings a fresh non-zero epoch.  An
//                               old value of the same epoch is a duplicate node.
//                       count   row i: the entries of row nodes[i] whose column's tag carries the epoch.  Rows of at most kLongRow
//                               entries by a LANE GROUP per row (16 lanes, or the wavefront when the parent averages more than 64
//                               entries a row), G entries per round; longer rows by a WORKGROUP per row, 1024 entries per round.
//                       scan    one workgroup (scan.hpp): out_rowptr, nnz into info[0]
//   dgll_hip_sg_fill    the count pass again with the row's offset: a kept entry's place inside its round is the prefix popcount of
//                       the round's ballot (plus, in the workgroup kernel, the kept entries of the lower wavefronts of the round,
//                       through LDS), so the kept entries of a row stay in parent order whatever the scheduling.
//   dgll_hip_sg_draw    GraphSAINT's draws (mode 1 node, 2 edge: bits of an N-bit bitmap; 3: walk roots), then the bitmap's scan
//   dgll_hip_sg_walk_nodes   the bitmap of a walk matrix (entries -1 skipped), then its scan
//   dgll_hip_sg_compact      the set bits in ascending id order
// Nothing depends on which thread wins: the tags are written by one launch and read by later ones, a node listed twice is an error
// and not a result, the bitmap is an OR, the error bits are an OR.  No float arithmetic except the row value 1 / kept.
#include "common.hpp"
#include "philox.hpp"
#include "scan.hpp"

namespace dgll {
namespace sg {

constexpr int kGrid = 2048;            // grid-stride cap
// Rows of more entries than this leave the lane-group kernel for the workgroup kernel.  From reading the code, not measured: a
// group walks its row serially, G entries a round, while the other groups of its wavefront wait for the longest of them -- 512
// entries are 32 rounds of a 16-lane group and 8 of a wavefront; the workgroup kernel pays a barrier a window and one a round of
// 1024 entries.
constexpr int kLongRow = 512;
enum { kInfoCount = 0, kInfoErr = 2, kInfoWords = 8 };
enum { kErrNode = 1, kErrCol = 2, kErrDup = 4 };
enum { kModeNode = 1, kModeEdge = 2, kModeRoots = 3 };

__device__ __forceinline__ void flag(int64_t* info, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(info + kInfoErr), bit);
}

inline int grid_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > kGrid ? kGrid : g));
}

// a lane per listed node
__global__ __launch_bounds__(kBlock) void mark_kernel(const int64_t* __restrict__ nodes, int64_t m, int64_t n_total,
                                                      unsigned long long* __restrict__ tag, uint32_t epoch, int64_t* __restrict__ info) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = nodes[i];
        if (v < 0 || v >= n_total) { flag(info, kErrNode); continue; }
        const unsigned long long old = atomicExch(tag + v, ((unsigned long long)epoch << 32) | (unsigned long long)i);
        if ((uint32_t)(old >> 32) == epoch) flag(info, kErrDup);
    }
}

// Is entry e kept, and under which local id?  A column outside [0, n_total) is never an index: it sets the error bit.
__device__ __forceinline__ bool kept_entry(const int32_t* __restrict__ col, int64_t e, int64_t n_total,
                                           const unsigned long long* __restrict__ tag, uint32_t epoch, int64_t* __restrict__ info,
                                           int32_t& local) {
    const int32_t c = col[e];
    if (c < 0 || c >= n_total) { flag(info, kErrCol); return false; }
    const unsigned long long t = tag[c];
    local = (int32_t)(uint32_t)t;
    return (uint32_t)(t >> 32) == epoch;
}

// one kept entry to its place
__device__ __forceinline__ void put_entry(int64_t o, int64_t out_nnz, int32_t local, int64_t e, float row_val, const float* __restrict__ val,
                                          int32_t* __restrict__ out_col, float* __restrict__ out_val, int64_t* __restrict__ out_eid) {
    if (o < 0 || o >= out_nnz) return;          // never, when out_rowptr is the count pass's under the same tags
    out_col[o] = local;
    if (out_val) out_val[o] = val ? val[e] : row_val;
    if (out_eid) out_eid[o] = e;
}

// 1 / kept, formed as dgll_hip_nb_block forms it
__device__ __forceinline__ float row_value(int64_t kept) { return kept > 0 ? (float)(1.0 / (double)kept) : 0.0f; }

// Rows of at most kLongRow entries: a group of G lanes per row, 64 / G rows per wavefront; every lane of a wavefront runs every
// round.  FILL = false: out_rowptr[r + 1] = kept entries of row r (0 for a longer row: the workgroup kernel writes it afterwards).
// FILL = true: out_rowptr is scanned; val: the parent's values to copy, or NULL for 1 / kept (used only when out_val is given).
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void rows_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const float* __restrict__ val, int64_t n_total, const int64_t* __restrict__ nodes,
                                                      int64_t m, const unsigned long long* __restrict__ tag, uint32_t epoch,
                                                      int64_t* __restrict__ out_rowptr, int64_t out_nnz, int32_t* __restrict__ out_col,
                                                      float* __restrict__ out_val, int64_t* __restrict__ out_eid,
                                                      int64_t* __restrict__ info) {
    constexpr int kRowsPerWave = kWave / G;
    constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t r0 = wave * kRowsPerWave; r0 < m; r0 += waves * kRowsPerWave) {
        const int64_t r = r0 + lane / G;
        const int64_t v = r < m ? nodes[r] : -1;
        const bool valid = v >= 0 && v < n_total;
        const int64_t b = valid ? rowptr[v] : 0;
        const int64_t d = valid ? rowptr[v + 1] - b : 0;
        const bool mine = d > 0 && d <= kLongRow;
        const int64_t end = mine ? b + d : b;
        int64_t at = 0;
        float rv = 0.0f;
        if (FILL && mine) {
            at = out_rowptr[r];
            rv = row_value(out_rowptr[r + 1] - at);
        }
        int64_t count = 0;
        for (int64_t base = b; __any(base < end); base += G) {
            const int64_t e = base + gl;
            int32_t local = 0;
            const bool keep = e < end && kept_entry(col, e, n_total, tag, epoch, info, local);
            const unsigned long long bal = (__ballot(keep) >> gbase) & kGroupMask;
            if (FILL && keep) put_entry(at + count + __popcll(bal & ((1ull << gl) - 1ull)), out_nnz, local, e, rv, val, out_col, out_val, out_eid);
            count += __popcll(bal);
        }
        if (!FILL && r < m && gl == 0) out_rowptr[r + 1] = count;
    }
}

// Rows of more than kLongRow entries: a workgroup per row.  A workgroup takes windows of kWindow rows (a lane of its first wavefront
// reads one row's degree), lists the long ones of the window in LDS in row order (ballot, prefix popcount), and walks each with all
// its lanes, kBlock * kPerLane entries a round: wavefront w takes the span [w * 64 * kPerLane, ...) of the round, kPerLane independent
// coalesced column loads and tag gathers per lane in flight, one barrier a round.  A kept entry's place: the kept entries of the
// lower wavefronts (LDS), of the lane's earlier ballots, and below it in its own ballot.  Every loop bound is the same in every
// thread of the workgroup.  Small windows, so that a batch of a few thousand rows still spreads its hubs over the chip.
constexpr int kWindow = 16;
constexpr int kPerLane = 4;
static_assert(kWindow <= kWave, "one wavefront lists a window");

template <bool FILL>
__global__ __launch_bounds__(kBlock) void long_rows_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, int64_t n_total,
                                                           const int64_t* __restrict__ nodes, int64_t m,
                                                           const unsigned long long* __restrict__ tag, uint32_t epoch,
                                                           int64_t* __restrict__ out_rowptr, int64_t out_nnz,
                                                           int32_t* __restrict__ out_col, float* __restrict__ out_val,
                                                           int64_t* __restrict__ out_eid, int64_t* __restrict__ info) {
    __shared__ int32_t list[kWindow];
    __shared__ int32_t n_list;
    __shared__ int32_t wave_n[2][kWavesPerBlock];       // two buffers: one barrier per round
    const int t = threadIdx.x, lane = lane_id(), w = t / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t first = (int64_t)blockIdx.x * kWindow; first < m; first += (int64_t)gridDim.x * kWindow) {
        if (w == 0) {
            const int64_t r = first + lane;
            const int64_t v = lane < kWindow && r < m ? nodes[r] : -1;
            const bool valid = v >= 0 && v < n_total;
            const bool is_long = valid && rowptr[v + 1] - rowptr[v] > kLongRow;
            const unsigned long long bal = __ballot(is_long);
            if (is_long) list[__popcll(bal & below)] = lane;
            if (lane == 0) n_list = __popcll(bal);
        }
        __syncthreads();
        const int n_long = n_list;
        int buf = 0;
        for (int i = 0; i < n_long; ++i) {
            const int64_t r = first + list[i];
            const int64_t v = nodes[r];                 // valid and long: listed above
            const int64_t b = rowptr[v], d = rowptr[v + 1] - b;
            int64_t at = 0;
            float rv = 0.0f;
            if (FILL) {
                at = out_rowptr[r];
                rv = row_value(out_rowptr[r + 1] - at);
            }
            int64_t count = 0;
            for (int64_t base = 0; base < d; base += kBlock * kPerLane, buf ^= 1) {
                bool keep[kPerLane];
                int32_t local[kPerLane];
                unsigned long long bal[kPerLane];
                int mine = 0;
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    const int64_t p = base + (w * kPerLane + j) * kWave + lane;
                    local[j] = 0;
                    keep[j] = p < d && kept_entry(col, b + p, n_total, tag, epoch, info, local[j]);
                }
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    bal[j] = __ballot(keep[j]);
                    mine += __popcll(bal[j]);
                }
                if (lane == 0) wave_n[buf][w] = mine;
                __syncthreads();
                int before = 0, total = 0;
                for (int j = 0; j < kWavesPerBlock; ++j) {
                    const int x = wave_n[buf][j];
                    before += j < w ? x : 0;
                    total += x;
                }
                if (FILL) {
#pragma unroll
                    for (int j = 0; j < kPerLane; ++j) {
                        const int64_t p = base + (w * kPerLane + j) * kWave + lane;
                        if (keep[j]) put_entry(at + count + before + __popcll(bal[j] & below), out_nnz, local[j], b + p, rv, val, out_col, out_val, out_eid);
                        before += __popcll(bal[j]);
                    }
                }
                count += total;
            }
            if (!FILL && t == 0) out_rowptr[r + 1] = count;
        }
        __syncthreads();                                // list and n_list are read before the next window rewrites them
    }
}

__global__ __launch_bounds__(kBlock) void rowptr_scan_kernel(int64_t* __restrict__ out_rowptr, int64_t m, int64_t* __restrict__ info) {
    scan_counts_to_rowptr(out_rowptr, m, info + kInfoCount);
}

// ---- GraphSAINT's node sets -------------------------------------------------------------------------------------------------------
// the row of entry e in [0, rowptr[n]): the largest v with rowptr[v] <= e (rows without entries are stepped over)
__device__ __forceinline__ int64_t row_of_entry(const int64_t* __restrict__ rowptr, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;             // invariant: rowptr[lo] <= e < rowptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void set_bit(uint32_t* __restrict__ bitmap, int64_t v) { atomicOr(bitmap + (v >> 5), 1u << (v & 31)); }

// a lane per draw: ONE Philox call, counter {i lo, i hi, 0, mode} (word 2 == 0: the walks use their step >= 1 there)
__global__ __launch_bounds__(kBlock) void draw_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t n_total,
                                                      int64_t nnz, int mode, int64_t budget, uint64_t seed, uint32_t* __restrict__ bitmap,
                                                      int64_t* __restrict__ roots, int64_t* __restrict__ info) {
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < budget; i += (int64_t)gridDim.x * kBlock) {
        const uint32_t ctr[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, (uint32_t)mode};
        uint32_t x[4];
        philox4x32_10(ctr, key, x);
        const unsigned long long word = ((unsigned long long)x[0] << 32) | x[1];
        if (mode == kModeRoots) {
            roots[i] = (int64_t)__umul64hi(word, (unsigned long long)n_total);
            continue;
        }
        const int64_t e = (int64_t)__umul64hi(word, (unsigned long long)nnz);       // < nnz
        set_bit(bitmap, row_of_entry(rowptr, n_total, e));
        if (mode == kModeEdge) {
            const int32_t c = col[e];
            if (c < 0 || c >= n_total) flag(info, kErrCol);
            else set_bit(bitmap, c);
        }
    }
}

// a lane per entry of the walk matrix; -1 (behind a dead end) and anything else outside [0, n_total) sets no bit
__global__ __launch_bounds__(kBlock) void walk_bits_kernel(const int32_t* __restrict__ walks, int64_t n_entries, int64_t n_total,
                                                           uint32_t* __restrict__ bitmap) {
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n_entries; j += (int64_t)gridDim.x * kBlock) {
        const int32_t v = walks[j];
        if (v >= 0 && v < n_total) set_bit(bitmap, v);
    }
}

__global__ __launch_bounds__(kBlock) void bitmap_scan_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words, int32_t* __restrict__ prefix,
                                                             int64_t* __restrict__ info) {
    scan_bitmap_words(bitmap, n_words, prefix, info + kInfoCount);
}

// the set bits in ascending id order
__global__ __launch_bounds__(kBlock) void compact_kernel(const uint32_t* __restrict__ bitmap, const int32_t* __restrict__ prefix,
                                                         int64_t n_words, int64_t n_nodes, int64_t* __restrict__ out_nodes) {
    for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * kBlock) {
        uint32_t bits = bitmap[w];
        int64_t k = prefix[w];
        while (bits && k < n_nodes) {
            out_nodes[k++] = w * 32 + (__ffs(bits) - 1);
            bits &= bits - 1u;
        }
    }
}

// both passes over the rows: the lane-group kernel, then the workgroup kernel for the rows it left
template <bool FILL>
static void launch_rows(hipStream_t st, const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_total, int64_t parent_nnz,
                        const int64_t* nodes, int64_t m, const unsigned long long* tag, uint32_t epoch, int64_t* out_rowptr, int64_t out_nnz,
                        int32_t* out_col, float* out_val, int64_t* out_eid, int64_t* info) {
    if (parent_nnz > 64 * n_total)      // long rows on average: a wavefront per row
        hipLaunchKernelGGL((rows_kernel<64, FILL>), dim3(grid_for(m, kBlock / 64)), dim3(kBlock), 0, st, rowptr, col, val, n_total, nodes, m, tag,
                           epoch, out_rowptr, out_nnz, out_col, out_val, out_eid, info);
    else
        hipLaunchKernelGGL((rows_kernel<16, FILL>), dim3(grid_for(m, kBlock / 16)), dim3(kBlock), 0, st, rowptr, col, val, n_total, nodes, m, tag,
                           epoch, out_rowptr, out_nnz, out_col, out_val, out_eid, info);
    hipLaunchKernelGGL((long_rows_kernel<FILL>), dim3(grid_for(m, kWindow)), dim3(kBlock), 0, st, rowptr, col, val,
                       n_total, nodes, m, tag, epoch, out_rowptr, out_nnz, out_col, out_val, out_eid, info);
}

}  // namespace sg
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_sg_long_row(void) { return sg::kLongRow; }

DGLL_API int dgll_hip_sg_count(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, const int64_t* nodes,
                               int64_t m, uint64_t* tag, uint32_t epoch, int64_t* out_rowptr, int64_t* info) {
    DGLL_REQUIRE(rowptr && tag && out_rowptr && info && (nodes || m == 0) && (col || nnz == 0),
                 "row pointers, tags, output row pointers and info must be non-NULL, as the node list and the columns when there are any");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && m >= 0 && m < (1ll << 31) && nnz >= 0 && epoch != 0,
                 "node count in (0, 2^31), 0 <= listed nodes < 2^31, nnz >= 0, non-zero epoch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto* tags = reinterpret_cast<unsigned long long*>(tag);
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, sg::kInfoWords * sizeof(int64_t), st));
    if (m > 0) {
        hipLaunchKernelGGL(sg::mark_kernel, dim3(sg::grid_for(m, kBlock)), dim3(kBlock), 0, st, nodes, m, n_total, tags, epoch, info);
        sg::launch_rows<false>(st, rowptr, col, nullptr, n_total, nnz, nodes, m, tags, epoch, out_rowptr, 0, nullptr, nullptr, nullptr, info);
    }
    hipLaunchKernelGGL(sg::rowptr_scan_kernel, dim3(1), dim3(kBlock), 0, st, out_rowptr, m, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_sg_fill(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_total, int64_t nnz,
                              const int64_t* nodes, int64_t m, const uint64_t* tag, uint32_t epoch, const int64_t* out_rowptr, int64_t out_nnz,
                              int32_t* out_col, float* out_val, int64_t* out_eid, int64_t* info) {
    DGLL_REQUIRE(rowptr && tag && out_rowptr && info && (nodes || m == 0) && (col || nnz == 0),
                 "row pointers, tags, the row pointers of dgll_hip_sg_count and info must be non-NULL, as the node list and the columns when there are any");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && m >= 0 && m < (1ll << 31) && nnz >= 0 && epoch != 0,
                 "node count in (0, 2^31), 0 <= listed nodes < 2^31, nnz >= 0, non-zero epoch");
    DGLL_REQUIRE(out_nnz >= 0 && out_nnz <= nnz && (out_nnz == 0 || out_col), "0 <= kept entries <= entries, column output non-NULL when there are any");
    if (out_nnz == 0 || m == 0) return DGLL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    sg::launch_rows<true>(st, rowptr, col, val, n_total, nnz, nodes, m, reinterpret_cast<const unsigned long long*>(tag), epoch,
                          const_cast<int64_t*>(out_rowptr), out_nnz, out_col, out_val, out_eid, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_sg_draw(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, int64_t nnz, int mode, int64_t budget,
                              uint64_t seed, uint32_t* bitmap, int32_t* prefix, int64_t* roots, int64_t* info) {
    DGLL_REQUIRE(rowptr && info, "row pointers and info must be non-NULL");
    DGLL_REQUIRE(mode == sg::kModeNode || mode == sg::kModeEdge || mode == sg::kModeRoots, "mode must be 1 (node), 2 (edge) or 3 (walk roots)");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && nnz >= 0 && budget >= 1 && budget < (1ll << 31),
                 "node count in (0, 2^31), nnz >= 0, budget in [1, 2^31)");
    if (mode == sg::kModeRoots) DGLL_REQUIRE(roots != nullptr, "mode 3 writes the roots: non-NULL");
    else DGLL_REQUIRE(col && bitmap && prefix && nnz > 0, "modes 1 and 2 draw entries: columns, bitmap and prefix non-NULL, nnz > 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, sg::kInfoWords * sizeof(int64_t), st));
    if (mode != sg::kModeRoots) DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st));
    hipLaunchKernelGGL(sg::draw_kernel, dim3(sg::grid_for(budget, kBlock)), dim3(kBlock), 0, st, rowptr, col, n_total, nnz, mode, budget, seed,
                       bitmap, roots, info);
    if (mode != sg::kModeRoots) hipLaunchKernelGGL(sg::bitmap_scan_kernel, dim3(1), dim3(kBlock), 0, st, bitmap, n_words, prefix, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_sg_walk_nodes(void* stream, const int32_t* walks, int64_t n_entries, int64_t n_total, uint32_t* bitmap, int32_t* prefix,
                                    int64_t* info) {
    DGLL_REQUIRE(walks && bitmap && prefix && info, "walks, bitmap, prefix and info must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_entries >= 1, "node count in (0, 2^31), at least one walk entry");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, sg::kInfoWords * sizeof(int64_t), st));
    DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st));
    hipLaunchKernelGGL(sg::walk_bits_kernel, dim3(sg::grid_for(n_entries, kBlock)), dim3(kBlock), 0, st, walks, n_entries, n_total, bitmap);
    hipLaunchKernelGGL(sg::bitmap_scan_kernel, dim3(1), dim3(kBlock), 0, st, bitmap, n_words, prefix, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_sg_compact(void* stream, int64_t n_total, const uint32_t* bitmap, const int32_t* prefix, int64_t n_nodes,
                                 int64_t* out_nodes) {
    DGLL_REQUIRE(bitmap && prefix && out_nodes, "bitmap, prefix and the node output must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_nodes >= 1 && n_nodes <= n_total, "node count in (0, 2^31), 1 <= set bits <= node count");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    hipLaunchKernelGGL(sg::compact_kernel, dim3(sg::grid_for(n_words, kBlock)), dim3(kBlock), 0, st, bitmap, prefix, n_words, n_total < n_nodes ? n_total : n_nodes,
                       out_nodes);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
