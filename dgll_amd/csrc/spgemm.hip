// spgemm.hip -- C = A . B with all three matrices in CSR (int64 rowptr, int32 col, optional fp32 val; an absent val is all ones), the
// columns of every row strictly increasing, in the operands and in the result (dgll_hip_spgemm_* in include/dgll_hip.h).  The structure
// of C is unknown before the kernels run, so the product is two passes around ONE 8-byte read-back of nnz(C):
//
//   count + scatter   ub[i] = min(sum of deg_B(k) over row i of A, N) bounds nnz(C_i).  It is parked in c_rowptr[i + 1], the rows are
//                     counted per class (integer atomics, one per wavefront and class) and their ids scattered into three lists.
//   symbolic          every product's column goes into the row's table; the distinct ones are counted into c_rowptr[i + 1]; one
//                     workgroup (scan.hpp) turns the counts into row pointers and the total.
//   numeric           the table is rebuilt, its keys compacted and sorted in LDS (bitonic) and written to c_col; the values are
//                     summed WITHOUT atomics: the entries of A's row are walked in storage order with the lanes spread over row k of
//                     B, which holds no column twice, so no two lanes meet in one step; a lane finds its slot by binary search in the
//                     sorted columns.
//
// Classes by ub (the capacity of a table is at least ub, so a full table still ends every probe):
//   * ub <= 512 (DGLL_SPGEMM_WAVE_MAX): a wavefront per row, four rows per workgroup.  Table of 512 int32 keys per wavefront, in the
//     numeric pass 512 sorted columns beside it and the fp32 sums in the space of the table (dead once compacted): 4 KiB per
//     wavefront, 16 KiB per workgroup; the 8 workgroups a CU holds by wave slots take 128 of its 160 KiB.
//   * ub <= 4096 (DGLL_SPGEMM_LDS_MAX): a workgroup per row.  Symbolic: 16 KiB (8 workgroups per CU).  Numeric: 4096 sorted columns
//     and four arrays of 4096 sums, one per wavefront (the first in the space of the table): 80 KiB, two workgroups (8 wavefronts)
//     per CU.  Each wavefront takes a contiguous quarter of A's row; the four arrays are added in wave order at the end.
//   * longer rows (hubs): a workgroup per row, a dense bitmap of N bits (integer atomicOr) and in the numeric pass a dense fp32
//     array of N sums in the caller's scratch.  The scratch holds a bounded pool of such slots, one per workgroup of the launch;
//     workgroup b works through rows b, b + slots, ... of the list inside the launch.  The bitmap yields the sorted columns
//     directly (scan_bitmap_words); the sums take a barrier per entry of A.
// The keys are hashed with (c * 107) mod slots, linear probing, the key word claimed by an LDS atomicCAS; slots = 2 next_pow2 of
// the bound where that fits the class (load <= 1/2) and the class capacity otherwise.  No floating-point atomic anywhere: the
// order of every sum is fixed by the storage order of A, so two runs give the same bits.
#include "common.hpp"
#include "scan.hpp"

namespace dgll {
namespace spgemm {

constexpr int kWaveCap = DGLL_SPGEMM_WAVE_MAX;
constexpr int kBlockCap = DGLL_SPGEMM_LDS_MAX;
constexpr int kSub = 8;                          // lanes that share one entry of A while keys are inserted (8 entries per wavefront)
constexpr int kEmpty = -1;
constexpr int kIntMax = 0x7fffffff;
constexpr size_t kHeaderBytes = 128;             // 16 control words
enum { kCount = 0, kErr = 3, kCursor = 4 };      // ctl[0..2]: rows per class, ctl[3]: error bits, ctl[4..6]: list cursors
constexpr int kErrRow = 1, kErrCol = 2, kErrTable = 4;
constexpr unsigned kMaxGrid = 8192;

static_assert((kWaveCap & (kWaveCap - 1)) == 0 && (kBlockCap & (kBlockCap - 1)) == 0, "table capacities are powers of two");

struct Args {
    int64_t M, K, N, nnz_a, nnz_b;
    const int64_t* a_ptr; const int32_t* a_col; const float* a_val;
    const int64_t* b_ptr; const int32_t* b_col; const float* b_val;
    int64_t* c_ptr; int32_t* c_col; float* c_val;
    unsigned long long* ctl; int32_t* rows;      // scratch header and the three class lists (wave rows first, long rows last)
    char* pool; int64_t words, slot_bytes;       // long-row slots: {bitmap uint32[words], prefix int32[words], sums float[N]}
};

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
static inline size_t slot_bytes_of(int64_t N) { return align16(8 * (size_t)((N + 31) / 32) + 4 * (size_t)N); }

template <bool BLOCK> __device__ __forceinline__ void group_sync() {
    if (BLOCK) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// phase boundary of the long class: the bitmap is written by L2 atomics and read by plain loads afterwards
__device__ __forceinline__ void long_sync() {
    __threadfence();
    __syncthreads();
    __threadfence();
}

__device__ __forceinline__ int next_pow2(int x) { return x <= 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)(x - 1))); }
__device__ __forceinline__ int table_slots(int64_t bound, int cap) {
    const int want = 2 * next_pow2((int)bound);
    return want < kWave ? kWave : (want < cap ? want : cap);
}
__device__ __forceinline__ int class_of(int64_t ub) { return ub <= 0 ? -1 : ub <= kWaveCap ? 0 : ub <= kBlockCap ? 1 : 2; }

__device__ __forceinline__ int wave_sum(int x) {
    for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// f(e, q) for every product of row i: entry e of A's row, entry q of B's row a_col[e].  SUB consecutive threads share an entry of A.
template <int NT, int SUB, typename F> __device__ __forceinline__ void products(const Args& P, int64_t i, int tid, F f) {
    const int64_t ae = P.a_ptr[i + 1];
    for (int64_t e = P.a_ptr[i] + tid / SUB; e < ae; e += NT / SUB) {
        const int64_t k = P.a_col[e], be = P.b_ptr[k + 1];
        for (int64_t q = P.b_ptr[k] + tid % SUB; q < be; q += SUB) f(e, q);
    }
}

// 1 when this call claimed a slot for c; the probe is bounded by the table
__device__ __forceinline__ int insert(int* t, int mask, int c, int& err) {
    int h = (int)(((uint32_t)c * 107u) & (uint32_t)mask);
    for (int p = 0; p <= mask; ++p) {
        const int found = atomicCAS(&t[h], kEmpty, c);
        if (found == kEmpty) return 1;
        if (found == c) return 0;
        h = (h + 1) & mask;
    }
    err |= kErrTable;
    return 0;
}

// the table of row i in t[0 .. slots); the keys this thread claimed
template <bool BLOCK> __device__ __forceinline__ int build_table(const Args& P, int64_t i, int tid, int* t, int slots, int& err) {
    constexpr int NT = BLOCK ? kBlock : kWave;
    for (int s = tid; s < slots; s += NT) t[s] = kEmpty;
    group_sync<BLOCK>();
    int fresh = 0;
    products<NT, kSub>(P, i, tid, [&](int64_t, int64_t q) {
        const int c = P.b_col[q];
        if ((uint32_t)c >= (uint64_t)P.N) err |= kErrCol;
        else fresh += insert(t, slots - 1, c, err);
    });
    group_sync<BLOCK>();
    return fresh;
}

__global__ void clear_kernel(unsigned long long* ctl) { if (threadIdx.x < 16) ctl[threadIdx.x] = 0ull; }

// kSub lanes per row: ub into c_ptr[i + 1], the rows of every class counted.  A row with a bad pointer or column id counts as empty.
__global__ __launch_bounds__(kBlock) void count_kernel(const Args P) {
    const int lane = lane_id(), sl = lane % kSub;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (int64_t)gridDim.x * kWavesPerBlock;
    constexpr int per = kWave / kSub;
    int err = 0;
    for (int64_t base = wave * per; base < P.M; base += waves * per) {          // the same in the whole wavefront
        const int64_t i = base + lane / kSub;
        int64_t sum = 0;
        int bad = 0;
        if (i < P.M) {
            const int64_t ab = P.a_ptr[i], ae = P.a_ptr[i + 1];
            if (ab < 0 || ae < ab || ae > P.nnz_a) bad = 1;
            else
                for (int64_t e = ab + sl; e < ae; e += kSub) {
                    const int64_t k = P.a_col[e];
                    if ((uint64_t)k >= (uint64_t)P.K) { bad = 1; continue; }
                    const int64_t bb = P.b_ptr[k], be = P.b_ptr[k + 1];
                    if (bb < 0 || be < bb || be > P.nnz_b) bad = 1;
                    else sum += be - bb;
                }
        }
        for (int o = kSub / 2; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); bad |= __shfl_xor(bad, o); }
        if (bad) { err |= kErrRow; sum = 0; }
        const int64_t ub = sum < P.N ? sum : P.N;
        const int cls = (i < P.M && sl == 0) ? class_of(ub) : -1;
        if (i < P.M && sl == 0) P.c_ptr[i + 1] = ub;
        for (int c = 0; c < 3; ++c) {
            const unsigned long long m = __ballot(cls == c);
            if (m != 0ull && lane == 0) atomicAdd(&P.ctl[kCount + c], (unsigned long long)__popcll(m));
        }
    }
    if (err) atomicOr(&P.ctl[kErr], (unsigned long long)err);
}

// a thread per row: its id into the list of its class, the slot taken from the class cursor by one atomic per wavefront
__global__ __launch_bounds__(kBlock) void scatter_kernel(const Args P) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int cls = i < P.M ? class_of(P.c_ptr[i + 1]) : -1;
    const int64_t off[3] = {0, (int64_t)P.ctl[kCount], (int64_t)(P.ctl[kCount] + P.ctl[kCount + 1])};
    for (int c = 0; c < 3; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (m == 0ull) continue;
        const int leader = __ffsll((long long)m) - 1;
        long long at = 0;
        if (lane == leader) at = (long long)atomicAdd(&P.ctl[kCursor + c], (unsigned long long)__popcll(m));
        at = __shfl(at, leader);
        const int64_t pos = off[c] + at + __popcll(m & ((1ull << lane) - 1ull));
        if (cls == c && pos < P.M) P.rows[pos] = (int32_t)i;
    }
}

// BLOCK: a workgroup per row of the workgroup class; otherwise a wavefront per row of the wave class
template <bool BLOCK> __global__ __launch_bounds__(kBlock) void symbolic_kernel(const Args P) {
    constexpr int cap = BLOCK ? kBlockCap : kWaveCap, per = BLOCK ? 1 : kWavesPerBlock;
    __shared__ int tab[per * cap];
    __shared__ int red[kWavesPerBlock];
    const int wave = (int)threadIdx.x / kWave, tid = BLOCK ? (int)threadIdx.x : lane_id();
    const int64_t count = (int64_t)P.ctl[kCount + (BLOCK ? 1 : 0)], off = BLOCK ? (int64_t)P.ctl[kCount] : 0;
    int err = 0;
    for (int64_t base = (int64_t)blockIdx.x * per; base < count; base += (int64_t)gridDim.x * per) {
        const int64_t r = BLOCK ? base : base + wave;
        if (r >= count) continue;                                            // wave class only: no workgroup barrier below
        const int64_t i = P.rows[off + r];
        int fresh = wave_sum(build_table<BLOCK>(P, i, tid, BLOCK ? tab : tab + wave * cap, table_slots(P.c_ptr[i + 1], cap), err));
        if (BLOCK) {
            if (lane_id() == 0) red[wave] = fresh;
            __syncthreads();
            fresh = red[0] + red[1] + red[2] + red[3];
            __syncthreads();                                                 // red and the bound in c_ptr[i + 1] are free again
        } else {
            group_sync<false>();
        }
        if (tid == 0) P.c_ptr[i + 1] = fresh;
    }
    if (err) atomicOr(&P.ctl[kErr], (unsigned long long)err);
}

__device__ __forceinline__ void long_bitmap(const Args& P, int64_t i, uint32_t* bm, int& err) {
    for (int64_t w = threadIdx.x; w < P.words; w += kBlock) bm[w] = 0u;
    long_sync();
    products<kBlock, 32>(P, i, (int)threadIdx.x, [&](int64_t, int64_t q) {
        const int c = P.b_col[q];
        if ((uint32_t)c >= (uint64_t)P.N) err |= kErrCol;
        else atomicOr(&bm[c >> 5], 1u << (c & 31));
    });
    long_sync();
}

__global__ __launch_bounds__(kBlock) void symbolic_long_kernel(const Args P) {
    __shared__ int red[kWavesPerBlock];
    const int64_t count = (int64_t)P.ctl[kCount + 2], off = (int64_t)(P.ctl[kCount] + P.ctl[kCount + 1]);
    uint32_t* bm = reinterpret_cast<uint32_t*>(P.pool + (int64_t)blockIdx.x * P.slot_bytes);
    int err = 0;
    for (int64_t r = blockIdx.x; r < count; r += gridDim.x) {
        const int64_t i = P.rows[off + r];
        long_bitmap(P, i, bm, err);
        int bits = 0;
        for (int64_t w = threadIdx.x; w < P.words; w += kBlock) bits += __popc(bm[w]);
        bits = wave_sum(bits);
        if (lane_id() == 0) red[threadIdx.x / kWave] = bits;
        __syncthreads();
        if (threadIdx.x == 0) P.c_ptr[i + 1] = red[0] + red[1] + red[2] + red[3];
        long_sync();
    }
    if (err) atomicOr(&P.ctl[kErr], (unsigned long long)err);
}

// the counts in c_ptr[1 .. M] to row pointers; the total, or minus the error bits, to *total
__global__ __launch_bounds__(kBlock) void rowptr_kernel(const Args P, int64_t* total) {
    scan_counts_to_rowptr(P.c_ptr, P.M, total);
    __syncthreads();
    if (threadIdx.x == 0 && P.ctl[kErr] != 0ull) *total = -(int64_t)P.ctl[kErr];
}

// first index of cols[0 .. n) that is not below c
__device__ __forceinline__ int lower_bound(const int* cols, int n, int c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// acc[slot of column] += a . b over entries [e0, e1) of A's row in storage order, one wavefront, the lanes over B's row
__device__ __forceinline__ void accumulate(const Args& P, int64_t e0, int64_t e1, const int* cols, int n, float* acc) {
    const int lane = lane_id();
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t k = P.a_col[e], be = P.b_ptr[k + 1];
        const float av = P.a_val ? P.a_val[e] : 1.0f;
        for (int64_t q = P.b_ptr[k] + lane; q < be; q += kWave) {
            const int c = P.b_col[q];
            const int s = lower_bound(cols, n, c);
            if (s < n && cols[s] == c) acc[s] = fmaf(av, P.b_val ? P.b_val[q] : 1.0f, acc[s]);
        }
        group_sync<false>();                                                 // the next entry may meet this one's columns
    }
}

// LDS of a group (int words): BLOCK {tab / sums of wave 0: cap, sums of waves 1..3: 3 cap, cols: cap}, wave {tab / sums: cap, cols: cap}
template <bool BLOCK> __global__ __launch_bounds__(kBlock) void numeric_kernel(const Args P) {
    constexpr int cap = BLOCK ? kBlockCap : kWaveCap, NT = BLOCK ? kBlock : kWave, n_acc = BLOCK ? kWavesPerBlock : 1;
    extern __shared__ __attribute__((aligned(16))) int spgemm_lds[];
    __shared__ int filled[kWavesPerBlock];
    const int wave = (int)threadIdx.x / kWave, tid = BLOCK ? (int)threadIdx.x : lane_id();
    int* tab = BLOCK ? spgemm_lds : spgemm_lds + wave * 2 * cap;
    int* cols = tab + n_acc * cap;
    float* acc = reinterpret_cast<float*>(tab);
    int* fill = &filled[BLOCK ? 0 : wave];
    const int64_t count = (int64_t)P.ctl[kCount + (BLOCK ? 1 : 0)], off = BLOCK ? (int64_t)P.ctl[kCount] : 0;
    for (int64_t base = (int64_t)blockIdx.x * (BLOCK ? 1 : kWavesPerBlock); base < count;
         base += (int64_t)gridDim.x * (BLOCK ? 1 : kWavesPerBlock)) {
        const int64_t r = BLOCK ? base : base + wave;
        if (r >= count) continue;                                            // wave class only: no workgroup barrier below
        const int64_t i = P.rows[off + r], out = P.c_ptr[i];
        const int64_t want = P.c_ptr[i + 1] - out;
        if (want <= 0 || want > cap) continue;                               // not the row pointers of the symbolic pass: write nothing
        const int n = (int)want, slots = table_slots(n, cap), npad = next_pow2(n);
        int err = 0;
        if (tid == 0) *fill = 0;
        build_table<BLOCK>(P, i, tid, tab, slots, err);
        for (int s = tid; s < slots; s += NT) {                              // compact in any order: the sort follows
            const int c = tab[s];
            if (c != kEmpty) { const int at = atomicAdd(fill, 1); if (at < cap) cols[at] = c; }
        }
        for (int s = n + tid; s < npad; s += NT) cols[s] = kIntMax;
        group_sync<BLOCK>();
        const bool ok = *fill == n;
        group_sync<BLOCK>();                                                 // every thread has read the counter
        for (int k = 2; k <= npad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int x = tid; x < npad / 2; x += NT) {
                    const int l = ((x & ~(j - 1)) << 1) | (x & (j - 1)), h = l | j;
                    const int a = cols[l], b = cols[h];
                    if ((a > b) == ((l & k) == 0)) { cols[l] = b; cols[h] = a; }
                }
                group_sync<BLOCK>();
            }
        if (!ok) continue;                                                   // the same answer in the whole group
        for (int s = tid; s < n; s += NT) P.c_col[out + s] = cols[s];
        if (P.c_val == nullptr) { group_sync<BLOCK>(); continue; }
        for (int a = 0; a < n_acc; ++a)
            for (int s = tid; s < n; s += NT) acc[a * cap + s] = 0.0f;
        group_sync<BLOCK>();
        const int64_t ab = P.a_ptr[i], ae = P.a_ptr[i + 1];
        if (BLOCK) {
            const int64_t chunk = (ae - ab + kWavesPerBlock - 1) / kWavesPerBlock;
            const int64_t e0 = ab + wave * chunk < ae ? ab + wave * chunk : ae, e1 = e0 + chunk < ae ? e0 + chunk : ae;
            accumulate(P, e0, e1, cols, n, acc + wave * cap);
            __syncthreads();
            for (int s = tid; s < n; s += NT) P.c_val[out + s] = ((acc[s] + acc[cap + s]) + acc[2 * cap + s]) + acc[3 * cap + s];
        } else {
            accumulate(P, ab, ae, cols, n, acc);
            for (int s = tid; s < n; s += NT) P.c_val[out + s] = acc[s];
        }
        group_sync<BLOCK>();                                                 // the LDS is free again
    }
}

__global__ __launch_bounds__(kBlock) void numeric_long_kernel(const Args P) {
    __shared__ int64_t found;
    const int64_t count = (int64_t)P.ctl[kCount + 2], off = (int64_t)(P.ctl[kCount] + P.ctl[kCount + 1]);
    char* slot = P.pool + (int64_t)blockIdx.x * P.slot_bytes;
    uint32_t* bm = reinterpret_cast<uint32_t*>(slot);
    int32_t* prefix = reinterpret_cast<int32_t*>(slot) + P.words;
    float* sums = reinterpret_cast<float*>(slot) + 2 * P.words;
    for (int64_t r = blockIdx.x; r < count; r += gridDim.x) {
        const int64_t i = P.rows[off + r], out = P.c_ptr[i], want = P.c_ptr[i + 1] - out;
        int err = 0;
        long_bitmap(P, i, bm, err);
        scan_bitmap_words(bm, P.words, prefix, &found);
        long_sync();
        if (found != want) { __syncthreads(); continue; }                    // not the row pointers of the symbolic pass
        for (int64_t w = threadIdx.x; w < P.words; w += kBlock) {            // ascending bits of ascending words: sorted columns
            int64_t at = out + prefix[w];
            for (uint32_t bits = bm[w]; bits != 0u; bits &= bits - 1u, ++at) {
                const int c = (int)(w * 32) + (__ffs((int)bits) - 1);
                P.c_col[at] = c;
                if (P.c_val) sums[c] = 0.0f;
            }
        }
        __syncthreads();
        if (P.c_val == nullptr) continue;
        const int64_t ae = P.a_ptr[i + 1];
        for (int64_t e = P.a_ptr[i]; e < ae; ++e) {                          // storage order; no column twice in a row of B
            const int64_t k = P.a_col[e], be = P.b_ptr[k + 1];
            const float av = P.a_val ? P.a_val[e] : 1.0f;
            for (int64_t q = P.b_ptr[k] + threadIdx.x; q < be; q += kBlock) {
                const int c = P.b_col[q];
                if ((uint32_t)c < (uint64_t)P.N) sums[c] = fmaf(av, P.b_val ? P.b_val[q] : 1.0f, sums[c]);
            }
            __syncthreads();
        }
        for (int64_t w = threadIdx.x; w < P.words; w += kBlock) {
            int64_t at = out + prefix[w];
            for (uint32_t bits = bm[w]; bits != 0u; bits &= bits - 1u, ++at) P.c_val[at] = sums[w * 32 + (__ffs((int)bits) - 1)];
        }
        __syncthreads();
    }
}

// ---- backward of the values: gathers over sorted rows, kSub lanes per pattern entry, a fixed shuffle tree ------------------------
// row of entry e: the last r with ptr[r] <= e
__device__ __forceinline__ int64_t row_of(const int64_t* ptr, int64_t n_rows, int64_t e) {
    int64_t lo = 0, hi = n_rows;                                             // ptr[lo] <= e < ptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

struct BwdArgs {
    int64_t x_rows, nnz_x, y_rows, nnz_y, M, nnz_c;
    const int64_t* x_ptr; const int32_t* x_col;
    const int64_t* y_ptr; const int32_t* y_col; const float* y_val;
    const int64_t* c_ptr; const int32_t* c_col; const float* dc;
    float* grad;
};

// MODE_A: x = A, y = B:    grad[e = (i, k)] = sum over q = (k, j) of row k of B    of B[q]   dC[i, j]
// MODE_B: x = B, y = A^T:  grad[e = (k, j)] = sum over q = (k, i) of row k of A^T  of A^T[q] dC[i, j]
template <int MODE> __global__ __launch_bounds__(kBlock) void bwd_kernel(const BwdArgs P) {
    const int lane = lane_id(), sl = lane % kSub;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (int64_t)gridDim.x * kWavesPerBlock;
    constexpr int per = kWave / kSub;
    for (int64_t base = wave * per; base < P.nnz_x; base += waves * per) {    // the same in the whole wavefront
        const int64_t e = base + lane / kSub;
        float sum = 0.0f;
        if (e < P.nnz_x) {
            const int64_t xr = row_of(P.x_ptr, P.x_rows, e), xc = P.x_col[e];
            const int64_t yr = MODE == DGLL_SPGEMM_BWD_A ? xc : xr;
            if ((uint64_t)yr < (uint64_t)P.y_rows) {
                int64_t qb = P.y_ptr[yr], qe = P.y_ptr[yr + 1];
                if (qb < 0 || qe > P.nnz_y) qe = qb;
                for (int64_t q = qb + sl; q < qe; q += kSub) {
                    const int64_t i = MODE == DGLL_SPGEMM_BWD_A ? xr : (int64_t)P.y_col[q];
                    const int j = MODE == DGLL_SPGEMM_BWD_A ? P.y_col[q] : (int)xc;
                    if ((uint64_t)i >= (uint64_t)P.M) continue;
                    int64_t lo = P.c_ptr[i], hi = P.c_ptr[i + 1];
                    if (lo < 0 || hi > P.nnz_c) continue;
                    const int64_t end = hi;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (P.c_col[mid] < j) lo = mid + 1; else hi = mid;
                    }
                    if (lo < end && P.c_col[lo] == j) sum = fmaf(P.y_val ? P.y_val[q] : 1.0f, P.dc[lo], sum);
                }
            }
        }
        for (int o = kSub / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (e < P.nnz_x && sl == 0) P.grad[e] = sum;
    }
}

inline unsigned capped(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : blocks < (int64_t)kMaxGrid ? blocks : (int64_t)kMaxGrid); }

// the shared host checks and the carving of the scratch; 1: nothing to do
static int prepare(const char* who, int64_t M, int64_t K, int64_t N, const int64_t* a_ptr, const int32_t* a_col, int64_t nnz_a,
                   const int64_t* b_ptr, const int32_t* b_col, int64_t nnz_b, int64_t* c_ptr, void* scratch, int64_t scratch_bytes,
                   Args& P, int64_t& long_slots) {
    const std::string w(who);
    const int64_t lim = int64_t(1) << 31;
    DGLL_REQUIRE(M >= 0 && K >= 0 && N >= 0 && M < lim && K < lim && N < lim, w + ": M, K and N must be in [0, 2^31)");
    DGLL_REQUIRE(nnz_a >= 0 && nnz_b >= 0 && nnz_a < lim && nnz_b < lim, w + ": nnz_a and nnz_b must be in [0, 2^31)");
    if (M == 0 || K == 0 || N == 0 || nnz_a == 0 || nnz_b == 0) return 1;
    DGLL_REQUIRE(a_ptr != nullptr && a_col != nullptr && b_ptr != nullptr && b_col != nullptr && c_ptr != nullptr && scratch != nullptr,
                 w + ": a_rowptr, a_col, b_rowptr, b_col, c_rowptr and scratch must be non-NULL");
    const size_t fixed = kHeaderBytes + align16(4 * (size_t)M), slot = slot_bytes_of(N);
    DGLL_REQUIRE(scratch_bytes >= 0 && (size_t)scratch_bytes >= fixed + slot && aligned16(scratch),
                 w + ": scratch too small: it needs dgll_hip_spgemm_scratch_bytes(M, N, long_slots >= 1) bytes, 16-byte aligned");
    long_slots = (int64_t)(((size_t)scratch_bytes - fixed) / slot);
    if (long_slots > M) long_slots = M;
    if (long_slots > (int64_t)kMaxGrid) long_slots = kMaxGrid;
    P.M = M; P.K = K; P.N = N; P.nnz_a = nnz_a; P.nnz_b = nnz_b;
    P.a_ptr = a_ptr; P.a_col = a_col; P.b_ptr = b_ptr; P.b_col = b_col; P.c_ptr = c_ptr;
    char* base = static_cast<char*>(scratch);
    P.ctl = reinterpret_cast<unsigned long long*>(base);
    P.rows = reinterpret_cast<int32_t*>(base + kHeaderBytes);
    P.pool = base + fixed;
    P.words = (N + 31) / 32;
    P.slot_bytes = (int64_t)slot;
    return 0;
}

}  // namespace spgemm
}  // namespace dgll

using namespace dgll;

DGLL_API size_t dgll_hip_spgemm_scratch_bytes(int64_t M, int64_t N, int64_t long_slots) {
    if (M < 0 || N < 0 || long_slots < 0) return 0;
    return spgemm::kHeaderBytes + spgemm::align16(4 * (size_t)M) + (size_t)long_slots * spgemm::slot_bytes_of(N);
}

DGLL_API int dgll_hip_spgemm_symbolic(void* stream, int64_t M, int64_t K, int64_t N, const int64_t* a_rowptr, const int32_t* a_col,
                                      int64_t nnz_a, const int64_t* b_rowptr, const int32_t* b_col, int64_t nnz_b, int64_t* c_rowptr,
                                      int64_t* total, void* scratch, int64_t scratch_bytes) {
    using namespace spgemm;
    Args P = {};
    int64_t long_slots = 0;
    const int rc = prepare("dgll_hip_spgemm_symbolic", M, K, N, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, c_rowptr, scratch,
                           scratch_bytes, P, long_slots);
    if (rc != 0) return rc < 0 ? rc : DGLL_OK;
    DGLL_REQUIRE(total != nullptr, "dgll_hip_spgemm_symbolic: total must be non-NULL");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(kWave), 0, st, P.ctl);
    hipLaunchKernelGGL(count_kernel, dim3(capped((M + 31) / 32)), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((M + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(symbolic_kernel<false>, dim3(capped((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(symbolic_kernel<true>, dim3(capped(M)), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(symbolic_long_kernel, dim3((unsigned)long_slots), dim3(kBlock), 0, st, P);
    hipLaunchKernelGGL(rowptr_kernel, dim3(1), dim3(kBlock), 0, st, P, total);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_spgemm_numeric(void* stream, int64_t M, int64_t K, int64_t N, const int64_t* a_rowptr, const int32_t* a_col,
                                     const float* a_val, int64_t nnz_a, const int64_t* b_rowptr, const int32_t* b_col, const float* b_val,
                                     int64_t nnz_b, const int64_t* c_rowptr, int32_t* c_col, float* c_val, int64_t nnz_c, void* scratch,
                                     int64_t scratch_bytes) {
    using namespace spgemm;
    if (nnz_c < 0 && nnz_c > -8) {
        const int64_t bits = -nnz_c;
        set_error(std::string("dgll_hip_spgemm_numeric: the symbolic pass could not place every row:") +
                  ((bits & kErrRow) ? " a row pointer of A or B, or a column id of A, is out of range;" : "") +
                  ((bits & kErrCol) ? " a column id of B is outside [0, N);" : "") +
                  ((bits & kErrTable) ? " a table was full (are the columns of every row of B distinct?);" : ""));
        return DGLL_ERR_INVALID;
    }
    DGLL_REQUIRE(nnz_c >= 0 && nnz_c < (int64_t(1) << 31), "dgll_hip_spgemm_numeric: nnz_c must be in [0, 2^31)");
    Args P = {};
    int64_t long_slots = 0;
    const int rc = prepare("dgll_hip_spgemm_numeric", M, K, N, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b,
                           const_cast<int64_t*>(c_rowptr), scratch, scratch_bytes, P, long_slots);
    if (rc != 0) return rc < 0 ? rc : DGLL_OK;
    if (nnz_c == 0) return DGLL_OK;
    DGLL_REQUIRE(c_col != nullptr, "dgll_hip_spgemm_numeric: c_col must be non-NULL");
    P.a_val = a_val; P.b_val = b_val; P.c_col = c_col; P.c_val = c_val;
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int wave_lds = kWavesPerBlock * 2 * kWaveCap * 4, block_lds = (kWavesPerBlock + 1) * kBlockCap * 4;
    static hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(&numeric_kernel<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, block_lds);
    DGLL_HIP_TRY(raised);
    hipLaunchKernelGGL(numeric_kernel<false>, dim3(capped((M + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), wave_lds, st, P);
    hipLaunchKernelGGL(numeric_kernel<true>, dim3(capped(M)), dim3(kBlock), block_lds, st, P);
    hipLaunchKernelGGL(numeric_long_kernel, dim3((unsigned)long_slots), dim3(kBlock), 0, st, P);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_spgemm_bwd(void* stream, int mode, int64_t x_rows, const int64_t* x_rowptr, const int32_t* x_col, int64_t nnz_x,
                                 int64_t y_rows, const int64_t* y_rowptr, const int32_t* y_col, const float* y_val, int64_t nnz_y,
                                 int64_t M, const int64_t* c_rowptr, const int32_t* c_col, const float* grad_c, int64_t nnz_c,
                                 float* grad_x) {
    using namespace spgemm;
    const int64_t lim = int64_t(1) << 31;
    DGLL_REQUIRE(mode == DGLL_SPGEMM_BWD_A || mode == DGLL_SPGEMM_BWD_B, "dgll_hip_spgemm_bwd: mode must be DGLL_SPGEMM_BWD_A or _B");
    DGLL_REQUIRE(x_rows >= 0 && y_rows >= 0 && M >= 0 && x_rows < lim && y_rows < lim && M < lim,
                 "dgll_hip_spgemm_bwd: x_rows, y_rows and M must be in [0, 2^31)");
    DGLL_REQUIRE(nnz_x >= 0 && nnz_y >= 0 && nnz_c >= 0 && nnz_x < lim && nnz_y < lim && nnz_c < lim,
                 "dgll_hip_spgemm_bwd: nnz_x, nnz_y and nnz_c must be in [0, 2^31)");
    if (nnz_x == 0) return DGLL_OK;
    DGLL_REQUIRE(x_rowptr != nullptr && x_col != nullptr && grad_x != nullptr && x_rows > 0,
                 "dgll_hip_spgemm_bwd: x_rowptr, x_col and grad_x must be non-NULL");
    DGLL_REQUIRE(y_rowptr != nullptr && c_rowptr != nullptr && (nnz_y == 0 || y_col != nullptr) && (nnz_c == 0 || (c_col != nullptr && grad_c != nullptr)),
                 "dgll_hip_spgemm_bwd: y_rowptr, y_col, c_rowptr, c_col and grad_c must be non-NULL");
    BwdArgs P = {x_rows, nnz_x, y_rows, nnz_y, M, nnz_c, x_rowptr, x_col, y_rowptr, y_col, y_val, c_rowptr, c_col, grad_c, grad_x};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(capped((nnz_x + 31) / 32));
    if (mode == DGLL_SPGEMM_BWD_A) hipLaunchKernelGGL(bwd_kernel<DGLL_SPGEMM_BWD_A>, grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL(bwd_kernel<DGLL_SPGEMM_BWD_B>, grid, dim3(kBlock), 0, st, P);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
