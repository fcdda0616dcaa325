// neighbor.hip -- node-wise fan-out sampling without replacement into message-flow-graph blocks (dgll_amd/sampling/neighbor.py).
//
// One layer is two entry points around the layer's one host read:
//   dgll_hip_nb_sample   count   a lane per destination row: ids validated, the destination marked (epoch tag, never cleared) with its
//                                local id, out count = min(deg, fanout) -- from rowptr alone
//                        scan    one workgroup: out_rowptr, nnz
//                        draw    fanout >= 0: a LANE GROUP per row (16 lanes when fanout <= 16, else the wavefront).  A row with
//                                deg <= fanout is copied (<= 64 entries).  Otherwise Floyd's algorithm: lane i computes word i of the
//                                row's Philox stream and t_i = mulhi(word_i, j_i + 1), j_i = deg - fanout + i, all in parallel; the
//                                only serial part is `fanout` steps of one shuffle and one ballot ("is t_s taken? then j_s").  The
//                                kept positions are ranked inside the group (ascending position) and col[b + pos] is loaded with
//                                independent loads.  A group and not a lane: a lane would keep 64 positions in scratch memory and
//                                run 16 Philox calls serially; a group keeps one position per lane in a register.
//                                fanout < 0: nothing is drawn and nothing is stored -- entry e of the output IS nonzero
//                                rowptr[row] + (e - out_rowptr[r]) of the graph, and every pass over the entries is FLAT (a lane per
//                                output entry, binary search for the row): a hub of 10^5 in-neighbours is never one wavefront's.
//                        mark    every drawn id that is no destination sets its bit in an N-bit bitmap (integer atomicOr)
//                        bitmap scan   one workgroup: exclusive popcount prefix per bitmap word, number of new nodes
//   dgll_hip_nb_block    src_nodes = [destinations in their order | set bits in ascending id order]; local id of a drawn id =
//                        the destination's position, or n_dst + prefix[word] + popcount(bits below); then a flat pass places every
//                        entry at the rank of its local id inside its row (ascending local ids; ties, which only parallel edges of
//                        the graph produce, by entry index).  The rank is a count over the row's entries: <= 64 compares per entry
//                        of a sampled layer, deg per entry of a copied one.
//   dgll_hip_nb_sample_weighted   the same sequence with another draw: the `fanout` smallest exponential race keys -log(u) / w of a row
//                        (weighted sampling without replacement), by a lane group per row of at most kLongRow entries and by a
//                        workgroup per longer row; see "weighted draw" below.  dgll_hip_nb_block finishes the layer unchanged.
// Nothing depends on which thread wins: the marks are set before they are read (separate launches), the bitmap is an OR, the
// order of the new nodes is the bit order.  Errors (row / column id outside [0, N), a destination listed twice) set bits of
// info[2] and the offending id is not used as an index.
#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace nb {

constexpr int kGrid = 2048;            // grid-stride cap
constexpr int kMaxFanout = 64;         // one kept position per lane of a wavefront
enum { kInfoNnz = 0, kInfoNew = 1, kInfoErr = 2, kInfoLong = 3, kInfoWords = 8 };   // kInfoLong: rows listed for wdraw_long_kernel
enum { kErrRow = 1, kErrCol = 2, kErrDup = 4, kErrWeight = 8 };

__device__ __forceinline__ void flag(int64_t* info, unsigned long long bit) {
    atomicOr(reinterpret_cast<unsigned long long*>(info + kInfoErr), bit);
}

inline int grid_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > kGrid ? kGrid : g));
}

// a lane per destination row
__global__ __launch_bounds__(kBlock) void count_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rows, int64_t n_rows,
                                                       int64_t n_total, int fanout, uint32_t* __restrict__ mark, int32_t* __restrict__ local,
                                                       uint32_t epoch, int64_t* __restrict__ out_rowptr, int64_t* __restrict__ info) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kBlock) {
        const int64_t v = rows[r];
        int64_t cnt = 0;
        if (v < 0 || v >= n_total) {
            flag(info, kErrRow);
        } else {
            if (atomicExch(mark + v, epoch) == epoch) flag(info, kErrDup);
            else local[v] = (int32_t)r;
            const int64_t d = rowptr[v + 1] - rowptr[v];
            cnt = (fanout < 0 || d <= fanout) ? (d > 0 ? d : 0) : fanout;
        }
        out_rowptr[r + 1] = cnt;
    }
}

// one workgroup: in-place inclusive scan of out_rowptr[1..n], out_rowptr[0] = 0, nnz into info
__global__ __launch_bounds__(kBlock) void scan_kernel(int64_t* __restrict__ out_rowptr, int64_t n_rows, int64_t* __restrict__ info) {
    __shared__ int64_t part[kBlock];
    const int t = threadIdx.x;
    const int64_t chunk = (n_rows + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n_rows ? t * chunk : n_rows, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += out_rowptr[i + 1];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        out_rowptr[0] = 0;
        info[kInfoNnz] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t i = lo; i < hi; ++i) { run += out_rowptr[i + 1]; out_rowptr[i + 1] = run; }
}

// a drawn id that is in range and no destination becomes a bit
__device__ __forceinline__ void mark_new(int32_t c, int64_t n_total, const uint32_t* __restrict__ mark, uint32_t epoch,
                                         uint32_t* __restrict__ bitmap, int64_t* __restrict__ info) {
    if (c < 0 || c >= n_total) { flag(info, kErrCol); return; }
    if (mark[c] != epoch) atomicOr(bitmap + (c >> 5), 1u << (c & 31));
}

// fanout >= 0: a group of G lanes per row (G >= fanout), 64 / G rows per wavefront; every lane of a wavefront runs every step
template <int G>
__global__ __launch_bounds__(kBlock) void draw_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_total, int fanout,
                                                      uint64_t seed, uint32_t layer, const uint32_t* __restrict__ mark, uint32_t epoch,
                                                      uint32_t* __restrict__ bitmap, const int64_t* __restrict__ out_rowptr,
                                                      int32_t* __restrict__ drawn, int64_t* __restrict__ info) {
    constexpr int kRowsPerWave = kWave / G;
    constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t r0 = wave * kRowsPerWave; r0 < n_rows; r0 += waves * kRowsPerWave) {
        const int64_t r = r0 + lane / G;
        const int64_t v = r < n_rows ? rows[r] : -1;
        const bool valid = v >= 0 && v < n_total;
        const int64_t b = valid ? rowptr[v] : 0;
        const int64_t d = valid ? rowptr[v + 1] - b : 0;
        const bool sampled = d > fanout;
        const int cnt = sampled ? fanout : (int)(d > 0 ? d : 0);
        uint32_t t = 0u, chosen = 0xffffffffu;
        if (sampled && gl < fanout) {           // word gl of the row's stream: call gl / 4, word gl % 4
            const uint32_t ctr[4] = {(uint32_t)v, (uint32_t)((uint64_t)v >> 32), layer, (uint32_t)(gl >> 2)};
            uint32_t x[4];
            philox4x32_10(ctr, key, x);
            const uint32_t word = (gl & 3) == 0 ? x[0] : (gl & 3) == 1 ? x[1] : (gl & 3) == 2 ? x[2] : x[3];
            t = __umulhi(word, (uint32_t)(d - fanout + gl + 1));
        }
        for (int s = 0; s < fanout; ++s) {      // Floyd: step s takes t_s unless an earlier step took it, then j_s = d - fanout + s
            const uint32_t ts = __shfl(t, s, G);
            const unsigned long long hit = (__ballot(sampled && gl < s && chosen == ts) >> gbase) & kGroupMask;
            if (sampled && gl == s) chosen = hit ? (uint32_t)(d - fanout + s) : ts;
        }
        const uint32_t pos = sampled ? chosen : (uint32_t)gl;
        int rank = 0;                           // ascending position
        for (int s = 0; s < fanout; ++s) {
            const uint32_t ps = __shfl(pos, s, G);
            rank += (s < cnt && ps < pos) ? 1 : 0;
        }
        if (gl < cnt) {
            const int32_t c = col[b + pos];
            drawn[out_rowptr[r] + rank] = c;
            mark_new(c, n_total, mark, epoch, bitmap, info);
        }
    }
}

// ---- weighted draw (dgll_hip_nb_sample_weighted) ------------------------------------------------------------------------------
// Position p of node v's row races with key = -log(u) / w (fp64, the arithmetic of lw::keys_kernel), u from ONE Philox call with
// counter (v lo, v hi, layer | 2^31, p): the high bit keeps this stream apart from draw_kernel's (v lo, v hi, layer, word / 4).  The
// kept entries are the `fanout` smallest by (key bits, position): successive draws without replacement in proportion to w.

// Rows longer than this leave the lane-group kernel for the workgroup kernel.  Chosen from reading the code, not measured: a group
// walks a row serially in chunks of G positions, so a short row costs its wavefront at most 1024 / 16 = 64 chunk steps (one Philox
// call and one fp64 log per lane each) while the other groups of that wavefront wait; the workgroup kernel walks a long row four
// chunks of 64 at a time and needs every wavefront's share to hold at least 64 positions (kLongRow >= kBlock).
constexpr int kLongRow = 1024;
constexpr int kLongGrid = 512;                                   // fixed grid of the long-row kernel: it strides over the list
constexpr unsigned long long kNoKey = ~0ull;                     // above every key of a positive finite weight (a finite double >= 0)
constexpr uint32_t kNoPos = 0xffffffffu;
static_assert(kLongRow >= kBlock && kLongRow <= 4096, "every wavefront's share of a long row holds a whole chunk");

__device__ __forceinline__ bool key_lt(unsigned long long ak, uint32_t ap, unsigned long long bk, uint32_t bp) {
    return ak < bk || (ak == bk && ap < bp);
}

// key bits of position p; a weight that is no positive finite number gives kNoKey (never selected) and sets `bad`
__device__ __forceinline__ unsigned long long race_key(int64_t v, uint32_t layer, uint32_t p, const uint32_t key[2], float w, bool& bad) {
    if (!(w > 0.0f && w < __uint_as_float(0x7f800000u))) { bad = true; return kNoKey; }
    const uint32_t ctr[4] = {(uint32_t)v, (uint32_t)((uint64_t)v >> 32), layer | 0x80000000u, p};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    const uint64_t bits = (((uint64_t)x[0] << 32) | x[1]) >> 11;             // 53 random bits
    const double u = ((double)bits + 0.5) * 1.1102230246251565e-16;        // 2^-53
    return (unsigned long long)__double_as_longlong(-log(u) / (double)w);  // positive doubles order like their bits
}

// The group's kept set: lane i < fanout of the group holds the i-th smallest (key, position) seen so far, (kNoKey, kNoPos) while
// fewer than i + 1 were seen.  Every lane offers at most one candidate (has, k, p).  Candidates below the current fanout-th
// smallest are inserted one at a time, lowest lane first: the lanes above the insertion point shift up by one lane and the old
// fanout-th smallest drops out.  The result does not depend on that order (the smallest `fanout` of a set).  Every lane of the
// wavefront runs every step; the loop ends on a wave-wide ballot.
template <int G>
__device__ __forceinline__ void offer(bool has, unsigned long long k, uint32_t p, int fanout, int gl, int gbase, unsigned long long& ck,
                                      uint32_t& cp) {
    constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
    unsigned long long tk = __shfl(ck, fanout - 1, G);
    uint32_t tp = __shfl(cp, fanout - 1, G);
    bool cand = has && key_lt(k, p, tk, tp);
    for (;;) {
        const unsigned long long all = __ballot(cand);
        if (!all) break;
        const unsigned long long m = (all >> gbase) & kGroupMask;
        const int src = m ? __ffsll((long long)m) - 1 : gl;
        const unsigned long long nk = __shfl(k, src, G);
        const uint32_t np = __shfl(p, src, G);
        const unsigned long long pk = __shfl_up(ck, 1, G);
        const uint32_t pp = __shfl_up(cp, 1, G);
        if (m && gl == src) cand = false;
        if (m && gl < fanout && key_lt(nk, np, ck, cp)) {                   // the new pair is below mine: mine moves up a lane
            const bool here = gl == 0 || !key_lt(nk, np, pk, pp);
            ck = here ? nk : pk;
            cp = here ? np : pp;
        }
        tk = __shfl(ck, fanout - 1, G);
        tp = __shfl(cp, fanout - 1, G);
        cand = cand && key_lt(k, p, tk, tp);
    }
}

// rows of at most kLongRow entries: a group of G lanes per row as in draw_kernel; longer rows are appended to long_list
template <int G>
__global__ __launch_bounds__(kBlock) void wdraw_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       const float* __restrict__ weight, const int64_t* __restrict__ rows, int64_t n_rows,
                                                       int64_t n_total, int fanout, uint64_t seed, uint32_t layer,
                                                       const uint32_t* __restrict__ mark, uint32_t epoch, uint32_t* __restrict__ bitmap,
                                                       const int64_t* __restrict__ out_rowptr, int32_t* __restrict__ drawn,
                                                       int32_t* __restrict__ long_list, int64_t* __restrict__ info) {
    constexpr int kRowsPerWave = kWave / G;
    const int lane = lane_id(), gl = lane & (G - 1), gbase = lane & ~(G - 1);
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = ((int64_t)gridDim.x * kBlock) / kWave;
    for (int64_t r0 = wave * kRowsPerWave; r0 < n_rows; r0 += waves * kRowsPerWave) {
        const int64_t r = r0 + lane / G;
        const int64_t v = r < n_rows ? rows[r] : -1;
        const bool valid = v >= 0 && v < n_total;
        const int64_t b = valid ? rowptr[v] : 0;
        const int64_t d = valid ? rowptr[v + 1] - b : 0;
        const bool is_long = d > kLongRow;
        const bool walk = d > fanout && !is_long;
        if (is_long && gl == 0)             // n_rows entries at most: a row slot is appended once
            long_list[atomicAdd(reinterpret_cast<unsigned long long*>(info + kInfoLong), 1ull)] = (int32_t)r;
        unsigned long long ck = kNoKey;
        uint32_t cp = kNoPos;
        bool bad = false;
        for (int64_t base = 0; __any(walk && base < d); base += G) {
            const int64_t p = base + gl;
            const bool act = walk && p < d;
            const unsigned long long k = act ? race_key(v, layer, (uint32_t)p, key, weight[b + p], bad) : kNoKey;
            offer<G>(act && k != kNoKey, k, (uint32_t)p, fanout, gl, gbase, ck, cp);
        }
        const int cnt = walk ? fanout : (is_long || d < 0 ? 0 : (int)d);
        if (!walk && gl < cnt) {            // a copied row: its weights are checked, not used
            const float w = weight[b + gl];
            bad = !(w > 0.0f && w < __uint_as_float(0x7f800000u));
        }
        if (bad) flag(info, kErrWeight);
        const uint32_t pos = walk ? cp : (uint32_t)gl;
        int rank = 0;                           // ascending position
        for (int s = 0; s < fanout; ++s) {
            const uint32_t ps = __shfl(pos, s, G);
            rank += (s < cnt && ps < pos) ? 1 : 0;
        }
        if (gl < cnt && pos != kNoPos) {        // kNoPos: only behind a bad weight, and the error bit is set
            const int32_t c = col[b + pos];
            drawn[out_rowptr[r] + rank] = c;
            mark_new(c, n_total, mark, epoch, bitmap, info);
        }
    }
}

// rows of more than kLongRow entries: one per workgroup.  Wavefront w keeps the `fanout` smallest of the chunks w, w + 4, ... of
// the row; every global winner is among its share's winners, so the fanout smallest of the 4 * fanout pairs in LDS, found by rank
// counting over (key, position), are exact.  Ties (only between the unset pairs behind a bad weight) go by index.
__global__ __launch_bounds__(kBlock) void wdraw_long_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const float* __restrict__ weight, const int64_t* __restrict__ rows,
                                                            int64_t n_total, int fanout, uint64_t seed, uint32_t layer,
                                                            const uint32_t* __restrict__ mark, uint32_t epoch, uint32_t* __restrict__ bitmap,
                                                            const int64_t* __restrict__ out_rowptr, int32_t* __restrict__ drawn,
                                                            const int32_t* __restrict__ long_list, int64_t* __restrict__ info) {
    __shared__ unsigned long long win_key[kWavesPerBlock * kMaxFanout];
    __shared__ uint32_t win_pos[kWavesPerBlock * kMaxFanout];
    __shared__ uint32_t kept[kMaxFanout];
    const int t = threadIdx.x, lane = lane_id(), w = t / kWave, m = kWavesPerBlock * fanout;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int64_t n_long = info[kInfoLong];
    for (int64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int64_t r = long_list[i];
        const int64_t v = rows[r];              // in range: wdraw_kernel lists valid rows only
        const int64_t b = rowptr[v], d = rowptr[v + 1] - b;
        unsigned long long ck = kNoKey;
        uint32_t cp = kNoPos;
        bool bad = false;
        for (int64_t base = (int64_t)w * kWave; base < d; base += kBlock) {
            const int64_t p = base + lane;
            const bool act = p < d;
            const unsigned long long k = act ? race_key(v, layer, (uint32_t)p, key, weight[b + p], bad) : kNoKey;
            offer<kWave>(act && k != kNoKey, k, (uint32_t)p, fanout, lane, 0, ck, cp);
        }
        if (bad) flag(info, kErrWeight);
        if (lane < fanout) { win_key[w * fanout + lane] = ck; win_pos[w * fanout + lane] = cp; }
        __syncthreads();
        if (t < m) {
            const unsigned long long mk = win_key[t];
            const uint32_t mp = win_pos[t];
            int rank = 0;
            for (int j = 0; j < m; ++j) {
                const unsigned long long ok = win_key[j];
                const uint32_t op = win_pos[j];
                rank += (key_lt(ok, op, mk, mp) || (ok == mk && op == mp && j < t)) ? 1 : 0;
            }
            if (rank < fanout) kept[rank] = mp;
        }
        __syncthreads();
        if (t < fanout) {
            const uint32_t mp = kept[t];
            int rank = 0;                       // ascending position
            for (int j = 0; j < fanout; ++j) rank += kept[j] < mp ? 1 : 0;
            if (mp != kNoPos) {
                const int32_t c = col[b + mp];
                drawn[out_rowptr[r] + rank] = c;
                mark_new(c, n_total, mark, epoch, bitmap, info);
            }
        }
        __syncthreads();
    }
}

// row slot of output entry e: the last r with out_rowptr[r] <= e (rows without entries are skipped)
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ out_rowptr, int64_t n_rows, int64_t e) {
    int64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (out_rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// global id of output entry e of row slot r: the stored draw, or (drawn == NULL, every row copied whole) the graph's own nonzero
__device__ __forceinline__ int32_t entry_id(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                            const int64_t* __restrict__ rows, const int64_t* __restrict__ out_rowptr,
                                            const int32_t* __restrict__ drawn, int64_t r, int64_t e) {
    return drawn ? drawn[e] : col[rowptr[rows[r]] + (e - out_rowptr[r])];
}

// fanout < 0: the mark pass, flat over the entries
__global__ __launch_bounds__(kBlock) void mark_flat_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_total,
                                                           const uint32_t* __restrict__ mark, uint32_t epoch, uint32_t* __restrict__ bitmap,
                                                           const int64_t* __restrict__ out_rowptr, int64_t* __restrict__ info) {
    const int64_t E = out_rowptr[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const int64_t r = row_of(out_rowptr, n_rows, e);      // a row with entries has a valid id (count_kernel)
        mark_new(entry_id(rowptr, col, rows, out_rowptr, nullptr, r, e), n_total, mark, epoch, bitmap, info);
    }
}

// one workgroup: prefix[w] = set bits in words < w, their total into info
__global__ __launch_bounds__(kBlock) void bitmap_scan_kernel(const uint32_t* __restrict__ bitmap, int64_t n_words, int32_t* __restrict__ prefix,
                                                             int64_t* __restrict__ info) {
    __shared__ int64_t part[kBlock];
    const int t = threadIdx.x;
    const int64_t chunk = (n_words + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n_words ? t * chunk : n_words, hi = lo + chunk < n_words ? lo + chunk : n_words;
    int64_t sum = 0;
    for (int64_t w = lo; w < hi; ++w) sum += __popc(bitmap[w]);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        info[kInfoNew] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t w = lo; w < hi; ++w) { prefix[w] = (int32_t)run; run += __popc(bitmap[w]); }
}

// src_nodes = [rows | set bits ascending]
__global__ __launch_bounds__(kBlock) void src_nodes_kernel(const int64_t* __restrict__ rows, int64_t n_rows, const uint32_t* __restrict__ bitmap,
                                                           const int32_t* __restrict__ prefix, int64_t n_words, int64_t n_new,
                                                           int64_t* __restrict__ src) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = first; i < n_rows; i += stride) src[i] = rows[i];
    for (int64_t w = first; w < n_words; w += stride) {
        uint32_t bits = bitmap[w];
        int64_t k = prefix[w];
        while (bits && k < n_new) {
            src[n_rows + k++] = w * 32 + (__ffs(bits) - 1);
            bits &= bits - 1u;
        }
    }
}

// local id of every output entry (flat)
__global__ __launch_bounds__(kBlock) void local_ids_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_total,
                                                           const uint32_t* __restrict__ mark, const int32_t* __restrict__ local, uint32_t epoch,
                                                           const uint32_t* __restrict__ bitmap, const int32_t* __restrict__ prefix,
                                                           const int32_t* __restrict__ drawn, const int64_t* __restrict__ out_rowptr,
                                                           int64_t nnz, int32_t* __restrict__ loc) {
    const int64_t E = nnz < out_rowptr[n_rows] ? nnz : out_rowptr[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const int64_t r = drawn ? 0 : row_of(out_rowptr, n_rows, e);
        const int32_t c = entry_id(rowptr, col, rows, out_rowptr, drawn, r, e);
        int32_t l = 0;
        if (c >= 0 && c < n_total)
            l = mark[c] == epoch ? local[c] : (int32_t)(n_rows + prefix[c >> 5] + __popc(bitmap[c >> 5] & ((1u << (c & 31)) - 1u)));
        loc[e] = l;
    }
}

// every entry to the rank of its local id inside its row (flat); values 1 / count
__global__ __launch_bounds__(kBlock) void fill_kernel(const int64_t* __restrict__ out_rowptr, int64_t n_rows, int64_t nnz,
                                                      const int32_t* __restrict__ loc, int32_t* __restrict__ out_col,
                                                      float* __restrict__ out_val) {
    const int64_t E = nnz < out_rowptr[n_rows] ? nnz : out_rowptr[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        const int64_t r = row_of(out_rowptr, n_rows, e);
        const int64_t b = out_rowptr[r], end = out_rowptr[r + 1] < nnz ? out_rowptr[r + 1] : nnz;
        const int32_t mine = loc[e];
        int64_t rank = 0;
        for (int64_t k = b; k < end; ++k) {
            const int32_t other = loc[k];
            rank += (other < mine || (other == mine && k < e)) ? 1 : 0;
        }
        out_col[b + rank] = mine;
        if (out_val) out_val[b + rank] = (float)(1.0 / (double)(end - b));
    }
}

}  // namespace nb
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_nb_max_fanout(void) { return nb::kMaxFanout; }

DGLL_API int dgll_hip_nb_sample(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, const int64_t* rows, int64_t n_rows,
                                int fanout, uint64_t seed, int layer, uint32_t* mark, int32_t* local, uint32_t epoch, uint32_t* bitmap,
                                int32_t* prefix, int32_t* drawn, int64_t drawn_cap, int64_t* out_rowptr, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && rows && mark && local && bitmap && prefix && out_rowptr && info,
                 "CSR, rows, mark / local / bitmap / prefix workspaces, output row pointers and info must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_rows > 0 && n_rows < (1ll << 31) && layer >= 0 && epoch != 0,
                 "node count and row count in [1, 2^31), layer >= 0, non-zero epoch");
    DGLL_REQUIRE(fanout == -1 || (fanout >= 1 && fanout <= nb::kMaxFanout), "fan-out must be -1 (every neighbour) or in [1, 64]");
    DGLL_REQUIRE(fanout < 0 || (drawn && drawn_cap >= n_rows * (int64_t)fanout), "fan-out >= 1 needs a draw buffer of n_rows * fanout entries");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, nb::kInfoWords * sizeof(int64_t), st));
    DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st));
    hipLaunchKernelGGL(nb::count_kernel, dim3(nb::grid_for(n_rows, kBlock)), dim3(kBlock), 0, st, rowptr, rows, n_rows, n_total, fanout, mark,
                       local, epoch, out_rowptr, info);
    hipLaunchKernelGGL(nb::scan_kernel, dim3(1), dim3(kBlock), 0, st, out_rowptr, n_rows, info);
    if (fanout < 0)
        hipLaunchKernelGGL(nb::mark_flat_kernel, dim3(nb::kGrid), dim3(kBlock), 0, st, rowptr, col, rows, n_rows, n_total, mark, epoch, bitmap,
                           out_rowptr, info);
    else if (fanout <= 16)
        hipLaunchKernelGGL(nb::draw_kernel<16>, dim3(nb::grid_for(n_rows, kBlock / 16)), dim3(kBlock), 0, st, rowptr, col, rows, n_rows, n_total,
                           fanout, seed, (uint32_t)layer, mark, epoch, bitmap, out_rowptr, drawn, info);
    else
        hipLaunchKernelGGL(nb::draw_kernel<64>, dim3(nb::grid_for(n_rows, kBlock / 64)), dim3(kBlock), 0, st, rowptr, col, rows, n_rows, n_total,
                           fanout, seed, (uint32_t)layer, mark, epoch, bitmap, out_rowptr, drawn, info);
    hipLaunchKernelGGL(nb::bitmap_scan_kernel, dim3(1), dim3(kBlock), 0, st, bitmap, n_words, prefix, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_nb_long_row(void) { return nb::kLongRow; }

DGLL_API int dgll_hip_nb_sample_weighted(void* stream, const int64_t* rowptr, const int32_t* col, const float* weight, int64_t n_total,
                                         const int64_t* rows, int64_t n_rows, int fanout, uint64_t seed, int layer, uint32_t* mark,
                                         int32_t* local, uint32_t epoch, uint32_t* bitmap, int32_t* prefix, int32_t* drawn, int64_t drawn_cap,
                                         int64_t* out_rowptr, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && weight && rows && mark && local && bitmap && prefix && drawn && out_rowptr && info,
                 "CSR, weights, rows, mark / local / bitmap / prefix workspaces, draw buffer, output row pointers and info must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_rows > 0 && n_rows < (1ll << 31) && layer >= 0 && epoch != 0,
                 "node count and row count in [1, 2^31), layer >= 0, non-zero epoch");
    DGLL_REQUIRE(fanout >= 1 && fanout <= nb::kMaxFanout, "the weighted draw needs a fan-out in [1, 64]");
    DGLL_REQUIRE(drawn_cap >= n_rows * ((int64_t)fanout + 1),
                 "the weighted draw needs a draw buffer of n_rows * (fanout + 1) entries (the last n_rows list the long rows)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    int32_t* long_list = drawn + n_rows * (int64_t)fanout;
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, nb::kInfoWords * sizeof(int64_t), st));
    DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_words * sizeof(uint32_t), st));
    hipLaunchKernelGGL(nb::count_kernel, dim3(nb::grid_for(n_rows, kBlock)), dim3(kBlock), 0, st, rowptr, rows, n_rows, n_total, fanout, mark,
                       local, epoch, out_rowptr, info);
    hipLaunchKernelGGL(nb::scan_kernel, dim3(1), dim3(kBlock), 0, st, out_rowptr, n_rows, info);
    if (fanout <= 16)
        hipLaunchKernelGGL(nb::wdraw_kernel<16>, dim3(nb::grid_for(n_rows, kBlock / 16)), dim3(kBlock), 0, st, rowptr, col, weight, rows, n_rows,
                           n_total, fanout, seed, (uint32_t)layer, mark, epoch, bitmap, out_rowptr, drawn, long_list, info);
    else
        hipLaunchKernelGGL(nb::wdraw_kernel<64>, dim3(nb::grid_for(n_rows, kBlock / 64)), dim3(kBlock), 0, st, rowptr, col, weight, rows, n_rows,
                           n_total, fanout, seed, (uint32_t)layer, mark, epoch, bitmap, out_rowptr, drawn, long_list, info);
    hipLaunchKernelGGL(nb::wdraw_long_kernel, dim3(n_rows < nb::kLongGrid ? (int)n_rows : nb::kLongGrid), dim3(kBlock), 0, st, rowptr, col, weight,
                       rows, n_total, fanout, seed, (uint32_t)layer, mark, epoch, bitmap, out_rowptr, drawn, long_list, info);
    hipLaunchKernelGGL(nb::bitmap_scan_kernel, dim3(1), dim3(kBlock), 0, st, bitmap, n_words, prefix, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_nb_block(void* stream, const int64_t* rowptr, const int32_t* col, int64_t n_total, const int64_t* rows, int64_t n_rows,
                               int fanout, const uint32_t* mark, const int32_t* local, uint32_t epoch, const uint32_t* bitmap,
                               const int32_t* prefix, const int32_t* drawn, const int64_t* out_rowptr, int64_t nnz, int64_t n_new,
                               int32_t* loc, int64_t* src_nodes, int32_t* out_col, float* out_val) {
    DGLL_REQUIRE(rowptr && col && rows && mark && local && bitmap && prefix && out_rowptr && src_nodes,
                 "CSR, rows, the workspaces of dgll_hip_nb_sample, its row pointers and the source-node output must be non-NULL");
    DGLL_REQUIRE(n_total > 0 && n_total < (1ll << 31) && n_rows > 0 && n_rows < (1ll << 31) && nnz >= 0 && n_new >= 0 && n_new <= n_total
                 && n_rows + n_new < (1ll << 31) && epoch != 0, "node, row, entry and new-node counts (local ids are 32-bit), non-zero epoch");
    DGLL_REQUIRE(fanout == -1 || (fanout >= 1 && fanout <= nb::kMaxFanout && (drawn || nnz == 0)),
                 "fan-out -1 or in [1, 64]; fan-out >= 1 needs the draw buffer of dgll_hip_nb_sample");
    DGLL_REQUIRE(nnz == 0 || (loc && out_col), "local-id workspace and column output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n_words = (n_total + 31) / 32;
    const int32_t* dr = fanout < 0 ? nullptr : drawn;
    hipLaunchKernelGGL(nb::src_nodes_kernel, dim3(nb::grid_for(n_words > n_rows ? n_words : n_rows, kBlock)), dim3(kBlock), 0, st, rows, n_rows,
                       bitmap, prefix, n_words, n_new, src_nodes);
    if (nnz > 0) {
        const int grid = nb::grid_for(nnz, kBlock);
        hipLaunchKernelGGL(nb::local_ids_kernel, dim3(grid), dim3(kBlock), 0, st, rowptr, col, rows, n_rows, n_total, mark, local, epoch, bitmap,
                           prefix, dr, out_rowptr, nnz, loc);
        hipLaunchKernelGGL(nb::fill_kernel, dim3(grid), dim3(kBlock), 0, st, out_rowptr, n_rows, nnz, loc, out_col, out_val);
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
