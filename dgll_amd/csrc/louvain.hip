// louvain.hip -- the local-moving sweep of the size-capped Louvain communities (dgll_amd/community.py): for every active node v of
// community a, the neighbouring community it would rather be in.
//
//     W(v, x)  = sum of the weights of v's entries (v, u), u != v, with comm[u] == x          (int64, exact)
//     gain(c)  = (double)W(v, c) - resolution * (double)k_v * (double)tot_c / (double)two_m
//     stay     = (double)W(v, a) - resolution * (double)k_v * (double)(tot_a - k_v) / (double)two_m
//     eligible : csize_c + size_v <= cap,  gain(c) > stay,  not (cnt_a == 1 and cnt_c == 1 and c > a)
//     target   = the eligible c of largest gain, ties to the smallest id; a when there is none
//
// The sweep is synchronous: only start-of-sweep state is read, so a row's decision does not depend on any other row's.  The sums
// W(v, .) are gathered into an open-addressing hash table of {community int32, weight int64} with 2 * next_pow2(deg) slots (load
// <= 1/2, linear probing, the slot claimed by an integer compare-and-swap, the weight added by an integer atomic): exact and
// independent of the order the entries arrive in.  Three tiers by row length, all running the same decide_row():
//   * deg <= wave_max_deg (<= 128): one wavefront per row, the table in the wavefront's own 3 KiB of LDS.  A workgroup of four
//     holds 12 KiB, so the 8 workgroups a CU can hold by wave slots take 96 of its 160 KiB: LDS does not cut the occupancy.
//   * deg <= block_max_deg (<= 2048): one workgroup per row, a 4096-slot table (48 KiB) shared by its four wavefronts; three such
//     workgroups fit a CU.  The rows are taken from a queue the first kernel fills.
//   * longer rows (hubs, coarse levels): one workgroup per row, the table in the caller's scratch, claimed from a bump allocator and
//     cleared here; agent-scope atomics for every access to it (they are served by L2, a plain load could hit a stale L1 line).
// A row is never walked by a single wavefront once it is longer than wave_max_deg.
// Every float64 expression is evaluated left to right without contraction, from integers below 2^53 (checked by the entry point):
// tests/louvain_ref.py restates them in numpy with the same bits.  No float atomics.
//
// The refinement sweep of Leiden (dgll_hip_leiden_refine) runs the same decide_row() through the same three tiers with another
// row policy (RefineRow below: which rows decide, which entries count and under which key, which keys are candidates), after a
// first pass without tables that sums every row's weight into its bound community and into its own sub-community (wC, wS), adds
// wC - wS to its sub-community's `cut` with an integer atomic and fills the queues of the long rows.
#include "common.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace dgll {
namespace louvain {

constexpr int kWaveSlots = 256;                 // wave tier: rows of up to kWaveSlots / 2 entries
constexpr int kBlockSlots = 4096;               // workgroup tier: rows of up to kBlockSlots / 2 entries
constexpr int kEmpty = -1;
constexpr int kGrid = 1024;                     // persistent grids of the two queue kernels
constexpr size_t kHeaderBytes = 64;             // scratch: {mid rows queued, long rows queued, table slots handed out}
enum { kErrCol = 1, kErrScratch = 2, kErrRow = 4, kErrComm = 8, kErrBound = 16 };

struct Args {
    const int64_t* rowptr; const int32_t* col; const int64_t* w; const int64_t* k; const int64_t* size; const int32_t* comm;
    const int64_t* tot; const int64_t* csize; const int32_t* cnt;
    int64_t n, nnz, two_m, cap;
    double resolution;
    uint32_t seed_lo, seed_hi, level, sweep;
    int all_active, wave_max_deg, block_max_deg;
    unsigned long long* ctrl; int32_t* queue;   // queue[n]: workgroup-tier rows from the front, scratch-tier rows from the back
    unsigned long long* g_wts; int32_t* g_keys; int64_t long_slots;
    int32_t* target; unsigned long long* info;
    // refinement only (comm = the sub-communities, tot / csize / cnt theirs)
    const int32_t* bound; const int64_t* totP; unsigned long long* cut; int64_t* wS; int64_t* wC;
};

struct LdsTable {
    int* keys; unsigned long long* wts;
    __device__ __forceinline__ void clear(int64_t i) const { keys[i] = kEmpty; wts[i] = 0ull; }
    __device__ __forceinline__ int claim(int64_t i, int c) const { return atomicCAS(&keys[i], kEmpty, c); }
    __device__ __forceinline__ void add(int64_t i, unsigned long long x) const { atomicAdd(&wts[i], x); }
    __device__ __forceinline__ int key(int64_t i) const { return keys[i]; }
    __device__ __forceinline__ int64_t wt(int64_t i) const { return (int64_t)wts[i]; }
};

struct GlobalTable {
    int* keys; unsigned long long* wts;
    __device__ __forceinline__ void clear(int64_t i) const {
        __hip_atomic_store(&keys[i], kEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&wts[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ int claim(int64_t i, int c) const {
        int expected = kEmpty;
        __hip_atomic_compare_exchange_strong(&keys[i], &expected, c, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;                                                     // the value found: kEmpty when this call claimed the slot
    }
    __device__ __forceinline__ void add(int64_t i, unsigned long long x) const {
        __hip_atomic_fetch_add(&wts[i], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ int key(int64_t i) const { return __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int64_t wt(int64_t i) const {
        return (int64_t)__hip_atomic_load(&wts[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// the threads that share one row: a wavefront (its LDS accesses ordered by a wavefront fence) or the workgroup
template <bool BLOCK> __device__ __forceinline__ void group_sync() {
    if (BLOCK) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ int log2_slots(int64_t deg) {                     // slots = 2 * next_pow2(deg) = 1 << log2_slots, deg >= 1
    return deg <= 1 ? 1 : 65 - __builtin_clzll((unsigned long long)(deg - 1));
}
__device__ __forceinline__ int64_t slot_of(int c, int bits) { return (int64_t)(((uint32_t)c * 0x9E3779B1u) >> (32 - bits)); }

__device__ __forceinline__ bool better(double g, int c, double best_g, int best_c) {
    return c >= 0 && (best_c < 0 || g > best_g || (g == best_g && c < best_c));
}

__device__ __forceinline__ bool node_active(const Args& A, int64_t v) {
    if (A.all_active) return true;
    const uint32_t ctr[4] = {(uint32_t)v, A.level, A.sweep, 0u}, key[2] = {A.seed_lo, A.seed_hi};
    uint32_t x[4];
    philox4x32_10(ctr, key, x);
    return (x[0] & 1u) != 0u;
}

// What a sweep asks of decide_row(), per row: `decides` (does the row choose at all), `key` (does the entry to u != v count, and
// under which table key), `own` (the row's own key was found with weight wa) and `candidate` (may the row move to key c of weight
// wc, and at which gain; the gain must exceed `stay`).  kQueued: the queues were filled by an earlier pass with every long row, so
// the kernels that take them ask `decides` again.
struct MoveRow {                                                             // Louvain local moving: the header of this file
    static constexpr bool kQueued = false;
    int64_t kv, sv; int a, cnt_a; double two_m, stay;
    static __device__ __forceinline__ bool decides(const Args& A, int64_t v, int) { return node_active(A, v); }
    __device__ __forceinline__ MoveRow(const Args& A, int64_t v, int a_)
        : kv(A.k[v]), sv(A.size[v]), a(a_), cnt_a(A.cnt[a_]), two_m((double)A.two_m), stay(0.0) {}
    __device__ __forceinline__ bool key(const Args& A, int u, int& c, int& err) const {
        c = A.comm[u];
        if ((uint64_t)(int64_t)c >= (uint64_t)A.n) { err |= kErrComm; return false; }
        return true;
    }
    __device__ __forceinline__ void own(const Args& A, int64_t wa) {
        stay = (double)wa - A.resolution * (double)kv * (double)(A.tot[a] - kv) / two_m;
    }
    __device__ __forceinline__ bool candidate(const Args& A, int c, int64_t wc, double& gain) const {
        if (A.csize[c] + sv > A.cap) return false;
        if (cnt_a == 1 && c > a && A.cnt[c] == 1) return false;              // two singletons: only the larger id moves (no swaps)
        gain = (double)wc - A.resolution * (double)kv * (double)A.tot[c] / two_m;
        return gain > stay;
    }
};

// Leiden refinement: a singleton v of bound community p that is well connected to p,
//     (double)wC_v >= resolution * (double)k_v * (double)(totP_p - k_v) / (double)two_m,
// joins the sub-community S of p (entries into other bound communities do not count) of largest
//     gain(S) = (double)W(v, S) - resolution * (double)k_v * (double)tot_S / (double)two_m  >  0,      ties to the smallest id,
// among those with csize_S + size_v <= cap, not a singleton of larger id, and well connected themselves:
//     (double)cut_S >= resolution * (double)tot_S * (double)(totP_p - tot_S) / (double)two_m.
struct RefineRow {
    static constexpr bool kQueued = true;
    int64_t kv, sv, tp; int a, p; double two_m, stay;
    static __device__ __forceinline__ bool decides(const Args& A, int64_t v, int s) {
        if (A.cnt[s] != 1) return false;
        const int p = A.bound[v];
        if ((uint64_t)(int64_t)p >= (uint64_t)A.n) return false;             // reported by the sums pass
        const int64_t kv = A.k[v];
        return (double)A.wC[v] >= A.resolution * (double)kv * (double)(A.totP[p] - kv) / (double)A.two_m;
    }
    __device__ __forceinline__ RefineRow(const Args& A, int64_t v, int a_)   // after decides(): bound[v] is in range
        : kv(A.k[v]), sv(A.size[v]), tp(A.totP[A.bound[v]]), a(a_), p(A.bound[v]), two_m((double)A.two_m), stay(0.0) {}
    __device__ __forceinline__ bool key(const Args& A, int u, int& c, int& err) const {
        if (A.bound[u] != p) return false;
        c = A.comm[u];
        if ((uint64_t)(int64_t)c >= (uint64_t)A.n) { err |= kErrComm; return false; }
        return true;
    }
    __device__ __forceinline__ void own(const Args&, int64_t) {}             // a singleton: W(v, own) = 0, and staying gains 0
    __device__ __forceinline__ bool candidate(const Args& A, int c, int64_t wc, double& gain) const {
        if (A.csize[c] + sv > A.cap) return false;
        const int64_t tc = A.tot[c];
        if (c > a && A.cnt[c] == 1) return false;                            // two singletons: only the larger id moves (no swaps)
        if (!((double)(int64_t)A.cut[c] >= A.resolution * (double)tc * (double)(tp - tc) / two_m)) return false;
        gain = (double)wc - A.resolution * (double)kv * (double)tc / two_m;
        return gain > stay;
    }
};

// The decision for row v (own key a, entries [b, b + deg), deg >= 1, table of 1 << bits slots); the same value in every thread of
// the group.  red_gain / red_c: kWavesPerBlock LDS words each (BLOCK only).  err collects error bits.
template <bool BLOCK, typename Row, typename Table>
__device__ int decide_row(const Args& A, int64_t v, int a, int64_t b, int64_t deg, const Table t, int bits, double* red_gain, int* red_c,
                          int& err) {
    const int nt = BLOCK ? kBlock : kWave;
    const int tid = BLOCK ? (int)threadIdx.x : lane_id();
    const int64_t slots = (int64_t)1 << bits, mask = slots - 1;
    Row row(A, v, a);
    for (int64_t i = tid; i < slots; i += nt) t.clear(i);
    group_sync<BLOCK>();
    for (int64_t e = b + tid; e < b + deg; e += nt) {
        const int u = A.col[e];
        if ((uint64_t)(int64_t)u >= (uint64_t)A.n) { err |= kErrCol; continue; }
        if (u == v) continue;                                                // self-loop entries count in k only
        int c;
        if (!row.key(A, u, c, err)) continue;
        const unsigned long long wt = A.w ? (unsigned long long)A.w[e] : 1ull;
        int64_t h = slot_of(c, bits);
        for (;;) {                                                           // at most deg distinct keys in >= 2 deg slots: ends
            const int found = t.claim(h, c);
            if (found == kEmpty || found == c) { t.add(h, wt); break; }
            h = (h + 1) & mask;
        }
    }
    group_sync<BLOCK>();
    int64_t wa = 0;
    for (int64_t h = slot_of(a, bits);; h = (h + 1) & mask) {
        const int found = t.key(h);
        if (found == a) { wa = t.wt(h); break; }
        if (found == kEmpty) break;
    }
    row.own(A, wa);
    double best_g = 0.0;
    int best_c = -1;
    for (int64_t i = tid; i < slots; i += nt) {
        const int c = t.key(i);
        if (c == kEmpty || c == a) continue;
        double gain;
        if (!row.candidate(A, c, t.wt(i), gain)) continue;
        if (better(gain, c, best_g, best_c)) { best_g = gain; best_c = c; }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double og = __shfl_xor(best_g, off);
        const int oc = __shfl_xor(best_c, off);
        if (better(og, oc, best_g, best_c)) { best_g = og; best_c = oc; }
    }
    if (BLOCK) {
        if (lane_id() == 0) { red_gain[threadIdx.x / kWave] = best_g; red_c[threadIdx.x / kWave] = best_c; }
        __syncthreads();
        best_g = red_gain[0];
        best_c = red_c[0];
        for (int wv = 1; wv < kWavesPerBlock; ++wv)
            if (better(red_gain[wv], red_c[wv], best_g, best_c)) { best_g = red_gain[wv]; best_c = red_c[wv]; }
        __syncthreads();                                                     // the table and the reduce words are free again
    } else {
        group_sync<false>();
    }
    return best_c < 0 ? a : best_c;
}

// One wavefront per row.  Decides the rows of the wave tier and those that do not choose, queues the others (unless an earlier
// pass has).
template <typename Row> __global__ __launch_bounds__(kBlock) void louvain_wave_kernel(const Args A) {
    __shared__ int keys[kWavesPerBlock][kWaveSlots];
    __shared__ unsigned long long wts[kWavesPerBlock][kWaveSlots];
    __shared__ int movers;
    if (threadIdx.x == 0) movers = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t v = uniform64((int64_t)blockIdx.x * kWavesPerBlock + wave);
    const int lane = lane_id();
    int err = 0;
    if (v < A.n) {                                                           // no early return: every wavefront meets the barrier below
        const int a = A.comm[v];
        const int64_t b = A.rowptr[v], deg = A.rowptr[v + 1] - b;
        int tgt = a;
        if ((uint64_t)(int64_t)a >= (uint64_t)A.n) {
            err |= kErrComm;
        } else if (b < 0 || deg < 0 || b + deg > A.nnz || deg >= ((int64_t)1 << 30)) {
            err |= kErrRow;
        } else if (deg > 0 && Row::decides(A, v, a)) {
            if (deg <= A.wave_max_deg) {
                const LdsTable t = {keys[wave], wts[wave]};
                tgt = decide_row<false, Row>(A, v, a, b, deg, t, log2_slots(deg), nullptr, nullptr, err);
                if (lane == 0 && tgt != a) atomicAdd(&movers, 1);
            } else if (!Row::kQueued && lane == 0) {                         // its target is written by the kernel that takes it
                if (deg <= A.block_max_deg) {
                    A.queue[atomicAdd(&A.ctrl[0], 1ull)] = (int32_t)v;
                } else {
                    A.queue[A.n - 1 - (int64_t)atomicAdd(&A.ctrl[1], 1ull)] = (int32_t)v;
                }
            }
        }
        if (lane == 0) A.target[v] = tgt;
    }
    if (err) atomicOr(&A.info[1], (unsigned long long)err);
    __syncthreads();
    if (threadIdx.x == 0 && movers) atomicAdd(&A.info[0], (unsigned long long)movers);
}

// One workgroup per queued row; SCRATCH: the rows at the back of the queue, tables in global scratch.
template <typename Row, bool SCRATCH> __global__ __launch_bounds__(kBlock) void louvain_block_kernel(const Args A) {
    __shared__ int keys[SCRATCH ? 1 : kBlockSlots];
    __shared__ unsigned long long wts[SCRATCH ? 1 : kBlockSlots];
    __shared__ double red_gain[kWavesPerBlock];
    __shared__ int red_c[kWavesPerBlock];
    __shared__ long long table_at;
    const int64_t count = (int64_t)A.ctrl[SCRATCH ? 1 : 0];
    int err = 0;
    for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int64_t v = A.queue[SCRATCH ? A.n - 1 - i : i];
        const int a = A.comm[v];                                             // validated by the kernel that queued the row
        const int64_t b = A.rowptr[v], deg = A.rowptr[v + 1] - b;
        const int bits = log2_slots(deg);
        int tgt = a;
        if (Row::kQueued && !Row::decides(A, v, a)) continue;                // the same answer in every thread; target[v] is a already
        if (SCRATCH) {
            const int64_t slots = (int64_t)1 << bits;
            if (threadIdx.x == 0) table_at = (long long)atomicAdd(&A.ctrl[2], (unsigned long long)slots);
            __syncthreads();
            const int64_t at = table_at;
            __syncthreads();
            if (at + slots > A.long_slots) {
                err |= kErrScratch;
            } else {
                const GlobalTable t = {A.g_keys + at, A.g_wts + at};
                tgt = decide_row<true, Row>(A, v, a, b, deg, t, bits, red_gain, red_c, err);
            }
        } else {
            const LdsTable t = {keys, wts};
            tgt = decide_row<true, Row>(A, v, a, b, deg, t, bits, red_gain, red_c, err);
        }
        if (threadIdx.x == 0) {
            A.target[v] = tgt;
            if (tgt != a) atomicAdd(&A.info[0], 1ull);
        }
    }
    if (err) atomicOr(&A.info[1], (unsigned long long)err);
}

// ---- refinement, first pass: no tables ------------------------------------------------------------------------------------------
// The sums of row v (sub-community s, bound community p) over its entries (v, u), u != v, bound[u] == p: wc all of them, ws those with
// sub[u] == s.  Complete in the group's first thread.  red: 2 * kWavesPerBlock LDS words (BLOCK only).
template <bool BLOCK>
__device__ void row_sums(const Args& A, int64_t v, int s, int p, int64_t b, int64_t deg, long long* red, long long& wc, long long& ws,
                         int& err) {
    const int nt = BLOCK ? kBlock : kWave;
    const int tid = BLOCK ? (int)threadIdx.x : lane_id();
    wc = 0;
    ws = 0;
    for (int64_t e = b + tid; e < b + deg; e += nt) {
        const int u = A.col[e];
        if ((uint64_t)(int64_t)u >= (uint64_t)A.n) { err |= kErrCol; continue; }
        if (u == v || A.bound[u] != p) continue;
        const int c = A.comm[u];
        if ((uint64_t)(int64_t)c >= (uint64_t)A.n) { err |= kErrComm; continue; }
        const long long wt = A.w ? (long long)A.w[e] : 1ll;
        wc += wt;
        if (c == s) ws += wt;
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        wc += __shfl_xor(wc, off);
        ws += __shfl_xor(ws, off);
    }
    if (BLOCK) {
        if (lane_id() == 0) { red[threadIdx.x / kWave] = wc; red[kWavesPerBlock + threadIdx.x / kWave] = ws; }
        __syncthreads();
        wc = 0;
        ws = 0;
        for (int wv = 0; wv < kWavesPerBlock; ++wv) { wc += red[wv]; ws += red[kWavesPerBlock + wv]; }
        __syncthreads();                                                     // the reduce words are free again
    }
}

__device__ __forceinline__ void write_sums(const Args& A, int64_t v, int s, long long wc, long long ws) {
    A.wC[v] = wc;
    A.wS[v] = ws;
    if (wc != ws) atomicAdd(&A.cut[s], (unsigned long long)(wc - ws));
}

// One wavefront per row: validates the row, sums the rows of the wave tier, queues the longer ones (every one of them: the decision
// kernels that follow take the same queues).
__global__ __launch_bounds__(kBlock) void refine_sums_wave_kernel(const Args A) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t v = uniform64((int64_t)blockIdx.x * kWavesPerBlock + wave);
    if (v >= A.n) return;                                                    // no workgroup barrier in this kernel
    const int lane = lane_id();
    const int s = A.comm[v], p = A.bound[v];
    const int64_t b = A.rowptr[v], deg = A.rowptr[v + 1] - b;
    int err = 0;
    long long wc = 0, ws = 0;
    bool valid = false;
    if ((uint64_t)(int64_t)s >= (uint64_t)A.n) {
        err |= kErrComm;
    } else if ((uint64_t)(int64_t)p >= (uint64_t)A.n) {
        err |= kErrBound;
    } else if (b < 0 || deg < 0 || b + deg > A.nnz || deg >= ((int64_t)1 << 30)) {
        err |= kErrRow;
    } else if (deg <= A.wave_max_deg) {
        valid = true;
        if (deg > 0) row_sums<false>(A, v, s, p, b, deg, nullptr, wc, ws, err);
    } else {                                                                 // its sums are written by the kernel that takes it
        if (lane == 0) {
            if (deg <= A.block_max_deg) {
                A.queue[atomicAdd(&A.ctrl[0], 1ull)] = (int32_t)v;
            } else {
                A.queue[A.n - 1 - (int64_t)atomicAdd(&A.ctrl[1], 1ull)] = (int32_t)v;
            }
        }
        return;
    }
    if (lane == 0) {
        if (valid) {
            write_sums(A, v, s, wc, ws);
        } else {
            A.wC[v] = 0;
            A.wS[v] = 0;
        }
    }
    if (err) atomicOr(&A.info[1], (unsigned long long)err);
}

// One workgroup per queued row, both queues.
__global__ __launch_bounds__(kBlock) void refine_sums_block_kernel(const Args A) {
    __shared__ long long red[2 * kWavesPerBlock];
    const int64_t mid = (int64_t)A.ctrl[0], count = mid + (int64_t)A.ctrl[1];
    int err = 0;
    for (int64_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int64_t v = A.queue[i < mid ? i : A.n - 1 - (i - mid)];
        const int s = A.comm[v], p = A.bound[v];                             // validated by the kernel that queued the row
        const int64_t b = A.rowptr[v], deg = A.rowptr[v + 1] - b;
        long long wc, ws;
        row_sums<true>(A, v, s, p, b, deg, red, wc, ws, err);
        if (threadIdx.x == 0) write_sums(A, v, s, wc, ws);
    }
    if (err) atomicOr(&A.info[1], (unsigned long long)err);
}

static size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace louvain
}  // namespace dgll

using namespace dgll;

DGLL_API size_t dgll_hip_louvain_scratch_bytes(int64_t n, int64_t long_slots) {
    if (n < 0 || long_slots < 0) return 0;
    return louvain::kHeaderBytes + 8 * (size_t)long_slots + louvain::align8(4 * (size_t)long_slots) + 4 * (size_t)n;
}

// What both entry points check and set up after their own NULL checks: the scalars, the tier limits, the scratch and its layout.
static int prepare(louvain::Args& A, int64_t n, int64_t nnz, int64_t two_m, double resolution, int64_t cap, int wave_max_deg,
                   int block_max_deg, void* scratch, size_t scratch_bytes) {
    DGLL_REQUIRE(n > 0 && n < (1ll << 31) && nnz >= 0, "node count in [1, 2^31), nnz >= 0");
    DGLL_REQUIRE(two_m > 0 && two_m < (1ll << 53), "two_m must lie in [1, 2^53): the gains are exact float64 only below it");
    DGLL_REQUIRE(resolution >= 0.0 && resolution == resolution, "resolution must be a number >= 0");
    DGLL_REQUIRE(cap >= 1, "the community size cap must be >= 1");
    if (wave_max_deg < 0) wave_max_deg = louvain::kWaveSlots / 2;
    if (block_max_deg < 0) block_max_deg = louvain::kBlockSlots / 2;
    DGLL_REQUIRE(wave_max_deg <= louvain::kWaveSlots / 2, "wave_max_deg is at most 128 (a 256-slot table per wavefront)");
    DGLL_REQUIRE(block_max_deg <= louvain::kBlockSlots / 2, "block_max_deg is at most 2048 (a 4096-slot table per workgroup)");
    if (block_max_deg < wave_max_deg) block_max_deg = wave_max_deg;
    DGLL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7u) == 0, "scratch must be 8-byte aligned");
    DGLL_REQUIRE(scratch_bytes >= dgll_hip_louvain_scratch_bytes(n, 0), "scratch is smaller than dgll_hip_louvain_scratch_bytes(n, 0)");
    // the table slots are whatever the scratch holds beyond its header and the queue: 12 bytes each, the int64 halves first
    int64_t long_slots = (int64_t)((scratch_bytes - louvain::kHeaderBytes - 4 * (size_t)n) / 12);
    while (long_slots > 0 && dgll_hip_louvain_scratch_bytes(n, long_slots) > scratch_bytes) --long_slots;
    char* base = static_cast<char*>(scratch);
    A.n = n; A.nnz = nnz; A.two_m = two_m; A.cap = cap; A.resolution = resolution;
    A.seed_lo = 0; A.seed_hi = 0; A.level = 0; A.sweep = 0; A.all_active = 1;
    A.wave_max_deg = wave_max_deg; A.block_max_deg = block_max_deg;
    A.ctrl = reinterpret_cast<unsigned long long*>(base);
    A.g_wts = reinterpret_cast<unsigned long long*>(base + louvain::kHeaderBytes);
    A.g_keys = reinterpret_cast<int32_t*>(base + louvain::kHeaderBytes + 8 * (size_t)long_slots);
    A.queue = reinterpret_cast<int32_t*>(base + louvain::kHeaderBytes + 8 * (size_t)long_slots + louvain::align8(4 * (size_t)long_slots));
    A.long_slots = long_slots;
    A.bound = nullptr; A.totP = nullptr; A.cut = nullptr; A.wS = nullptr; A.wC = nullptr;
    return DGLL_OK;
}

static unsigned rows_grid(int64_t n) { return (unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock); }
static unsigned queue_grid(int64_t n) { return (unsigned)(n < louvain::kGrid ? n : louvain::kGrid); }

// The three tiers of a decision sweep, in stream order.
template <typename Row> static int launch_tiers(const louvain::Args& A, hipStream_t s) {
    hipLaunchKernelGGL(louvain::louvain_wave_kernel<Row>, dim3(rows_grid(A.n)), dim3(kBlock), 0, s, A);
    DGLL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((louvain::louvain_block_kernel<Row, false>), dim3(queue_grid(A.n)), dim3(kBlock), 0, s, A);
    DGLL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((louvain::louvain_block_kernel<Row, true>), dim3(queue_grid(A.n)), dim3(kBlock), 0, s, A);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_louvain_move(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* w, const int64_t* k,
                                   const int64_t* size, const int32_t* comm, const int64_t* tot, const int64_t* csize, const int32_t* cnt,
                                   int64_t n, int64_t nnz, int64_t two_m, double resolution, int64_t cap, uint64_t seed, uint32_t level,
                                   uint32_t sweep, int all_active, int wave_max_deg, int block_max_deg, void* scratch,
                                   size_t scratch_bytes, int32_t* target, int64_t* info) {
    DGLL_REQUIRE(rowptr && k && size && comm && tot && csize && cnt && target && info && scratch, "louvain_move: a NULL array");
    DGLL_REQUIRE(col || nnz == 0, "louvain_move: col must be non-NULL");
    louvain::Args A;
    const int code = prepare(A, n, nnz, two_m, resolution, cap, wave_max_deg, block_max_deg, scratch, scratch_bytes);
    if (code != DGLL_OK) return code;
    A.rowptr = rowptr; A.col = col; A.w = w; A.k = k; A.size = size; A.comm = comm; A.tot = tot; A.csize = csize; A.cnt = cnt;
    A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32); A.level = level; A.sweep = sweep; A.all_active = all_active != 0;
    A.target = target; A.info = reinterpret_cast<unsigned long long*>(info);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DGLL_HIP_TRY(hipMemsetAsync(scratch, 0, louvain::kHeaderBytes, s));
    return launch_tiers<louvain::MoveRow>(A, s);
}

DGLL_API int dgll_hip_leiden_refine(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* w, const int64_t* k,
                                    const int64_t* size, const int32_t* sub, const int32_t* bound, const int64_t* tot,
                                    const int64_t* csize, const int32_t* cnt, const int64_t* totP, int64_t n, int64_t nnz, int64_t two_m,
                                    double resolution, int64_t cap, int wave_max_deg, int block_max_deg, void* scratch,
                                    size_t scratch_bytes, int32_t* target, int64_t* wS, int64_t* wC, int64_t* cut, int64_t* info) {
    DGLL_REQUIRE(rowptr && k && size && sub && bound && tot && csize && cnt && totP && target && wS && wC && cut && info && scratch,
                 "leiden_refine: a NULL array");
    DGLL_REQUIRE(col || nnz == 0, "leiden_refine: col must be non-NULL");
    louvain::Args A;
    const int code = prepare(A, n, nnz, two_m, resolution, cap, wave_max_deg, block_max_deg, scratch, scratch_bytes);
    if (code != DGLL_OK) return code;
    A.rowptr = rowptr; A.col = col; A.w = w; A.k = k; A.size = size; A.comm = sub; A.tot = tot; A.csize = csize; A.cnt = cnt;
    A.bound = bound; A.totP = totP; A.cut = reinterpret_cast<unsigned long long*>(cut); A.wS = wS; A.wC = wC;
    A.target = target; A.info = reinterpret_cast<unsigned long long*>(info);
    hipStream_t s = static_cast<hipStream_t>(stream);
    DGLL_HIP_TRY(hipMemsetAsync(scratch, 0, louvain::kHeaderBytes, s));
    DGLL_HIP_TRY(hipMemsetAsync(cut, 0, 8 * (size_t)n, s));
    // first the sums (they fill the queues and `cut`), then the decisions, which read them
    hipLaunchKernelGGL(louvain::refine_sums_wave_kernel, dim3(rows_grid(n)), dim3(kBlock), 0, s, A);
    DGLL_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(louvain::refine_sums_block_kernel, dim3(queue_grid(n)), dim3(kBlock), 0, s, A);
    DGLL_HIP_TRY(hipGetLastError());
    return launch_tiers<louvain::RefineRow>(A, s);
}
