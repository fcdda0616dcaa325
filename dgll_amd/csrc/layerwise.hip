// layerwise.hip -- layer-wise importance sampling (LADIES / FastGCN) on the device.
//
// One layer of the samplers (dgll_amd/sampling/layerwise.py) is a handful of launches on rows R of a normalised adjacency L:
//   column mass   m_j = sum_{i in R} L_ij^2 in 64-bit fixed point (integer atomics: order-independent, bitwise reproducible), the
//                 distinct touched columns compacted into a candidate list through an epoch-tagged marker (never cleared)
//   select        s = min(#{q > 0}, fanout) nodes without replacement with probability q_j / sum q (q = m or sqrt(m)), in draw
//                 order: exponential race keys k_j = E_j / q_j (E_j = -log U_j, U_j from Philox4x32-10 keyed by (seed, layer),
//                 counter = node id), the s smallest keys by an 8-pass radix select over the key bits, then ranked by (key, id)
//   weights       estWRS_weights (O(m^2) in the reference) as one reverse scan of affine maps in fp64, or 1 / (p_j s)
//   block         L[R, S] scaled by w: count, scan, fill; within a row ascending by local column id
// Passes over the entries of R are flat (entry offsets + binary search), not a wavefront per row: LADIES draws hubs.
// Every integer the host needs to size an output (s, nnz) lands in one small device array, read once per layer.
#include "common.hpp"
#include "philox.hpp"

namespace dgll {
namespace lw {

constexpr int kGrid = 2048;             // grid-stride cap (memory-bound kernels)
constexpr int kMaxLocal = 4096;         // unsorted column maps: local ids < 4096 (128-word bitmap per wavefront)
constexpr int kBitmapWords = kMaxLocal / 32;
constexpr double kQFixed = 1099511627776.0;   // 2^40: fixed-point scale of sqrt(m) (flat variants)

// info[] slots shared with the Python side (one read per layer)
enum { kInfoCand = 0, kInfoS = 1, kInfoM = 2, kInfoNnz = 3, kInfoErr = 4 };
enum { kErrRow = 1, kErrCol = 2, kErrWinners = 4, kErrLocal = 8 };
// ctrl[] of the radix select
enum { kCtrlPrefix = 256, kCtrlK = 257, kCtrlS = 258, kCtrlWin = 259, kCtrlPos = 260, kCtrlWords = 264 };

using ::dgll::philox4x32_10;      // philox.hpp

__device__ __forceinline__ double q_of(unsigned long long m, double inv_scale, int flat) {
    const double d = (double)m * inv_scale;
    return flat ? sqrt(d) : d;
}

// what the totals add up for one column: the fixed-point mass itself, or sqrt(mass) in 2^-40 units
__device__ __forceinline__ unsigned long long total_term(unsigned long long m, double inv_scale, int flat) {
    return flat ? (unsigned long long)rint(sqrt((double)m * inv_scale) * kQFixed) : m;
}

__device__ __forceinline__ double total_of(const unsigned long long* tot, double inv_scale, int flat) {
    const double t = (double)tot[0] * 4294967296.0 + (double)tot[1];
    return flat ? t / kQFixed : t * inv_scale;
}

__device__ __forceinline__ void flag(int64_t* info, unsigned long long bit) {
    if (info) atomicOr(reinterpret_cast<unsigned long long*>(info + kInfoErr), bit);
}

__device__ __forceinline__ int64_t wave_global() { return ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave; }
__device__ __forceinline__ int64_t waves_total() { return ((int64_t)gridDim.x * blockDim.x) / kWave; }

// ---- entry-parallel passes over rows R of L --------------------------------------------------------------------------------
// The rows of a layer are power-law: a hub row holds 10^5 entries.  A wavefront per row would walk it alone, so every pass over the
// entries of R is flat: seg[r] = sum_{q < r} deg(rows[q]) (one workgroup), and entry e belongs to the row found by binary search.
// rows == NULL: all rows, seg = rowptr, entry e is L's nonzero e.
__global__ __launch_bounds__(kBlock) void row_offsets_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rows,
                                                             int64_t n_rows, int64_t n_total, int64_t* __restrict__ seg,
                                                             int64_t* __restrict__ info) {
    __shared__ int64_t part[kBlock];
    const int t = threadIdx.x;
    const int64_t chunk = (n_rows + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < n_rows ? t * chunk : n_rows, hi = lo + chunk < n_rows ? lo + chunk : n_rows;
    int64_t sum = 0;
    for (int64_t r = lo; r < hi; ++r) {
        const int64_t row = rows[r];
        if (row >= 0 && row < n_total) sum += rowptr[row + 1] - rowptr[row];
        else flag(info, kErrRow);
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int j = 0; j < kBlock; ++j) { const int64_t x = part[j]; part[j] = run; run += x; }
        seg[n_rows] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t r = lo; r < hi; ++r) {
        seg[r] = run;
        const int64_t row = rows[r];
        if (row >= 0 && row < n_total) run += rowptr[row + 1] - rowptr[row];
    }
}

// (row slot r, nonzero k of L) of entry e
__device__ __forceinline__ int64_t entry_at(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ rows,
                                            const int64_t* __restrict__ seg, int64_t n_rows, int64_t e, int64_t& r) {
    if (!rows) { r = -1; return e; }
    int64_t lo = 0, hi = n_rows;               // seg[lo] <= e < seg[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg[mid] <= e) lo = mid; else hi = mid;
    }
    r = lo;
    return rowptr[rows[lo]] + (e - seg[lo]);
}

// pass 1: the first thread to touch column c this epoch (atomicExch returns a different tag) appends it and zeroes its mass
__global__ __launch_bounds__(kBlock) void mark_columns_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const int64_t* __restrict__ rows, const int64_t* __restrict__ seg,
                                                              int64_t n_rows, uint32_t* __restrict__ marker, uint32_t epoch,
                                                              unsigned long long* __restrict__ mass, int32_t* __restrict__ cand,
                                                              int64_t* __restrict__ info) {
    const int64_t E = seg[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        int64_t r;
        const int32_t c = col[entry_at(rowptr, rows, seg, n_rows, e, r)];
        if (marker[c] != epoch && atomicExch(marker + c, epoch) != epoch) {
            mass[c] = 0ull;
            const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long*>(info + kInfoCand), 1ull);
            cand[slot] = c;          // slot < distinct columns <= n_total: the candidate array has n_total entries
        }
    }
}

__global__ __launch_bounds__(kBlock) void accumulate_mass_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const float* __restrict__ val, const int64_t* __restrict__ rows,
                                                                 const int64_t* __restrict__ seg, int64_t n_rows, double scale,
                                                                 unsigned long long* __restrict__ mass) {
    const int64_t E = seg[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        int64_t r;
        const int64_t k = entry_at(rowptr, rows, seg, n_rows, e, r);
        const double v = val ? (double)val[k] : 1.0;
        atomicAdd(mass + col[k], (unsigned long long)rint(v * v * scale));
    }
}

// totals as two 64-bit integer sums (high and low 32-bit halves of every term): exact, so order-independent
__global__ __launch_bounds__(kBlock) void totals_kernel(const int32_t* __restrict__ cand, const int64_t* __restrict__ info,
                                                        const unsigned long long* __restrict__ mass, double inv_scale, int flat,
                                                        unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long part[2][kBlock];
    const int64_t n = info[kInfoCand];
    unsigned long long hi = 0, lo = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned long long t = total_term(mass[cand[i]], inv_scale, flat);
        hi += t >> 32; lo += t & 0xffffffffull;
    }
    part[0][threadIdx.x] = hi; part[1][threadIdx.x] = lo;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { part[0][threadIdx.x] += part[0][threadIdx.x + w]; part[1][threadIdx.x] += part[1][threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { atomicAdd(tot, part[0][0]); atomicAdd(tot + 1, part[1][0]); }
}

// p of a list of ids: q_j / sum q
__global__ __launch_bounds__(kBlock) void column_p_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ count, int64_t cap,
                                                          const unsigned long long* __restrict__ mass, double inv_scale, int flat,
                                                          const unsigned long long* __restrict__ tot, double* __restrict__ p) {
    const int64_t n = count ? (*count < cap ? *count : cap) : cap;
    const double total = total_of(tot, inv_scale, flat);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        p[i] = q_of(mass[ids[i]], inv_scale, flat) / total;
}

// ---- weighted selection without replacement ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void keys_kernel(const int32_t* __restrict__ cand, const int64_t* __restrict__ count,
                                                      const unsigned long long* __restrict__ mass, double inv_scale, int flat,
                                                      uint64_t seed, uint32_t layer, unsigned long long* __restrict__ keys,
                                                      unsigned long long* __restrict__ ctrl) {
    const int64_t n = *count;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    unsigned long long pos = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int32_t id = cand[i];
        const double q = q_of(mass[id], inv_scale, flat);
        const uint32_t ctr[4] = {(uint32_t)id, 0u, layer, 0x4c414459u};
        uint32_t x[4];
        philox4x32_10(ctr, key, x);
        const uint64_t bits = (((uint64_t)x[0] << 32) | x[1]) >> 11;             // 53 random bits
        const double u = ((double)bits + 0.5) * 1.1102230246251565e-16;        // (0, 1): 2^-53
        const double k = q > 0.0 ? -log(u) / q : __longlong_as_double(0x7ff0000000000000ll);   // +inf: never drawn
        keys[i] = (unsigned long long)__double_as_longlong(k);                 // positive doubles order like their bits
        pos += q > 0.0 ? 1ull : 0ull;
    }
    if (pos) atomicAdd(ctrl + kCtrlPos, pos);
}

__global__ void select_init_kernel(unsigned long long* __restrict__ ctrl, int64_t fanout) {
    if (threadIdx.x == 0) {
        const unsigned long long pos = ctrl[kCtrlPos];
        const unsigned long long s = pos < (unsigned long long)fanout ? pos : (unsigned long long)fanout;
        ctrl[kCtrlS] = s; ctrl[kCtrlK] = s; ctrl[kCtrlPrefix] = 0ull;
    }
}

// histogram of digit `shift` over the keys that agree with the prefix found so far above it
__global__ __launch_bounds__(kBlock) void radix_hist_kernel(const unsigned long long* __restrict__ keys, const int64_t* __restrict__ count,
                                                            unsigned long long* __restrict__ ctrl, int shift) {
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t n = *count;
    const unsigned long long prefix = ctrl[kCtrlPrefix];
    if (ctrl[kCtrlK] != 0ull) {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
            const unsigned long long k = keys[i];
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (hist[threadIdx.x]) atomicAdd(ctrl + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// one workgroup: the bin holding the k-th smallest key; k becomes the rank inside that bin; the histogram is left zeroed
__global__ __launch_bounds__(kBlock) void radix_pick_kernel(unsigned long long* __restrict__ ctrl, int shift) {
    __shared__ unsigned long long incl[256];
    const unsigned long long h = ctrl[threadIdx.x];
    incl[threadIdx.x] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned long long add = (int)threadIdx.x >= off ? incl[threadIdx.x - off] : 0ull;
        __syncthreads();
        incl[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long k = ctrl[kCtrlK], before = incl[threadIdx.x] - h;
    __syncthreads();
    ctrl[threadIdx.x] = 0ull;
    if (k != 0ull && before < k && k <= incl[threadIdx.x]) {
        ctrl[kCtrlPrefix] |= (unsigned long long)threadIdx.x << shift;
        ctrl[kCtrlK] = k - before;
    }
}

// keys <= T (the s-th smallest): every key < T and all ties of T; the ranking keeps the first s by (key, id)
__global__ __launch_bounds__(kBlock) void gather_winners_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ cand,
                                                                const int64_t* __restrict__ count, int64_t* __restrict__ info, unsigned long long* __restrict__ ctrl,
                                                                unsigned long long* __restrict__ win_key, int32_t* __restrict__ win_id,
                                                                int64_t win_cap) {
    const int64_t n = *count;
    if (ctrl[kCtrlS] == 0ull) return;
    const unsigned long long t = ctrl[kCtrlPrefix];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const unsigned long long k = keys[i];
        if (k > t) continue;
        const unsigned long long slot = atomicAdd(ctrl + kCtrlWin, 1ull);
        if ((int64_t)slot < win_cap) { win_key[slot] = k; win_id[slot] = cand[i]; }
        else flag(info, kErrWinners);
    }
}

// rank of every winner among all winners by (key, id): its draw position; LDS tiles of the winner list
__global__ __launch_bounds__(kBlock) void rank_winners_kernel(const unsigned long long* __restrict__ win_key, const int32_t* __restrict__ win_id,
                                                              const unsigned long long* __restrict__ ctrl, int64_t win_cap,
                                                              int64_t* __restrict__ out_ids, int64_t* __restrict__ info) {
    __shared__ unsigned long long tk[kBlock];
    __shared__ int32_t ti[kBlock];
    const unsigned long long cnt = ctrl[kCtrlWin];
    const int64_t n = (int64_t)cnt < win_cap ? (int64_t)cnt : win_cap;
    const int64_t s = (int64_t)ctrl[kCtrlS];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long mk = i < n ? win_key[i] : 0ull;
    const int32_t mi = i < n ? win_id[i] : 0;
    int64_t rank = 0;
    for (int64_t base = 0; base < n; base += kBlock) {
        __syncthreads();
        if (base + threadIdx.x < n) { tk[threadIdx.x] = win_key[base + threadIdx.x]; ti[threadIdx.x] = win_id[base + threadIdx.x]; }
        __syncthreads();
        const int lim = n - base < kBlock ? (int)(n - base) : kBlock;
        for (int j = 0; j < lim; ++j) rank += (tk[j] < mk || (tk[j] == mk && ti[j] < mi)) ? 1 : 0;
    }
    if (i < n && rank < s) out_ids[rank] = mi;
    if (i == 0) { info[kInfoS] = s; info[kInfoM] = s; }
}

// ---- sorted unique of (S u batch) (FastGCN) ---------------------------------------------------------------------------------
// list element i: a[i] for i < *a_count, b[i - a_cap] for a_cap <= i < a_cap + nb; the first to claim a node keeps it
__global__ __launch_bounds__(kBlock) void union_claim_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ a_count, int64_t a_cap,
                                                             const int64_t* __restrict__ b, int64_t nb, int64_t n_total,
                                                             uint32_t* __restrict__ marker, uint32_t epoch, int64_t* __restrict__ reps,
                                                             unsigned long long* __restrict__ n_reps, int64_t* __restrict__ info) {
    const int64_t na = *a_count < a_cap ? *a_count : a_cap;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a_cap + nb; i += (int64_t)gridDim.x * kBlock) {
        int64_t v;
        if (i < na) v = a[i];
        else if (i >= a_cap) v = b[i - a_cap];
        else continue;
        if (v < 0 || v >= n_total) { flag(info, kErrCol); continue; }
        if (atomicExch(marker + v, epoch) != epoch) reps[atomicAdd(n_reps, 1ull)] = v;
    }
}

__global__ __launch_bounds__(kBlock) void union_rank_kernel(const int64_t* __restrict__ reps, const unsigned long long* __restrict__ n_reps,
                                                            int64_t* __restrict__ out, int64_t* __restrict__ info) {
    __shared__ int64_t tile[kBlock];
    const int64_t n = (int64_t)*n_reps;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t mine = i < n ? reps[i] : 0;
    int64_t rank = 0;
    for (int64_t base = 0; base < n; base += kBlock) {
        __syncthreads();
        if (base + threadIdx.x < n) tile[threadIdx.x] = reps[base + threadIdx.x];
        __syncthreads();
        const int lim = n - base < kBlock ? (int)(n - base) : kBlock;
        for (int j = 0; j < lim; ++j) rank += tile[j] < mine ? 1 : 0;
    }
    if (i < n) out[rank] = mine;
    if (i == 0) info[kInfoM] = n;
}

// ---- weights ------------------------------------------------------------------------------------------------------------------
// mode 0 (estWRS_weights): w_i = F_i((1 - P_i) / p_i * a_i), a_i = n / (i + 1) / (n - i), P_i = sum_{j < i} p_j,
// F_i = f_{m-1} o ... o f_{i+1}, f_j(x) = x (1 - a_j) + a_j.  Chunked over the workgroup: prefix sums and suffix compositions.
// mode 1: w_i = 1 / (p_i * s_num)
__global__ __launch_bounds__(kBlock) void weights_kernel(const double* __restrict__ p, const int64_t* __restrict__ m_dev, int64_t cap,
                                                         const int64_t* __restrict__ snum_dev, int64_t snum_host, int64_t n_total, int mode,
                                                         double* __restrict__ w) {
    __shared__ double sp[kBlock], sa[kBlock], sb[kBlock];
    const int64_t m = m_dev ? (*m_dev < cap ? *m_dev : cap) : cap;
    const int t = threadIdx.x;
    if (mode == 1) {
        const double snum = (double)(snum_dev ? *snum_dev : snum_host);
        for (int64_t i = t; i < m; i += kBlock) w[i] = 1.0 / p[i] / snum;
        return;
    }
    const double n = (double)n_total;
    const int64_t chunk = (m + kBlock - 1) / kBlock;
    const int64_t lo = t * chunk < m ? t * chunk : m, hi = lo + chunk < m ? lo + chunk : m;
    double psum = 0.0, ca = 1.0, cb = 0.0;          // chunk sum of p; chunk map G_t = f_{hi-1} o ... o f_lo as x -> ca x + cb
    for (int64_t i = lo; i < hi; ++i) {
        psum += p[i];
        const double al = n / (double)(i + 1) / (n - (double)i);
        ca *= 1.0 - al; cb = cb * (1.0 - al) + al;
    }
    sp[t] = psum; sa[t] = ca; sb[t] = cb;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;                            // exclusive prefix of the chunk sums
        for (int j = 0; j < kBlock; ++j) { const double x = sp[j]; sp[j] = run; run += x; }
        double ha = 1.0, hb = 0.0;                   // H_j = G_{T-1} o ... o G_{j+1}, from the back
        for (int j = kBlock - 1; j >= 0; --j) {
            const double ga = sa[j], gb = sb[j];
            sa[j] = ha; sb[j] = hb;
            hb = ha * gb + hb; ha = ha * ga;
        }
    }
    __syncthreads();
    double P = sp[t];
    for (int64_t i = lo; i < hi; ++i) {              // initial weights in draw order
        const double al = n / (double)(i + 1) / (n - (double)i);
        w[i] = (1.0 - P) / p[i] * al;
        P += p[i];
    }
    double ia = 1.0, ib = 0.0;                       // maps of this chunk after i
    const double ha = sa[t], hb = sb[t];
    for (int64_t i = hi - 1; i >= lo; --i) {
        const double x = w[i] * ia + ib;
        w[i] = ha * x + hb;
        const double al = n / (double)(i + 1) / (n - (double)i);
        ib = ia * al + ib; ia = ia * (1.0 - al);
    }
}

// ---- block extraction ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void map_columns_kernel(const int64_t* __restrict__ cols, const int64_t* __restrict__ m_dev, int64_t cap,
                                                             int64_t n_total, uint32_t* __restrict__ mark, int32_t* __restrict__ local,
                                                             uint32_t epoch, int64_t* __restrict__ info) {
    const int64_t m = m_dev ? (*m_dev < cap ? *m_dev : cap) : cap;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const int64_t c = cols[i];
        if (c < 0 || c >= n_total) { flag(info, kErrCol); continue; }
        mark[c] = epoch; local[c] = (int32_t)i;
    }
}

// one wavefront per row: kept entries counted into out_rowptr[r + 1]
__global__ __launch_bounds__(kBlock) void block_count_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                             const int64_t* __restrict__ rows, int64_t n_rows, int64_t n_total,
                                                             const uint32_t* __restrict__ mark, uint32_t epoch,
                                                             int64_t* __restrict__ out_rowptr, int64_t* __restrict__ info) {
    const int lane = lane_id();
    for (int64_t r = wave_global(); r < n_rows; r += waves_total()) {
        const int64_t row = rows[r];
        int64_t cnt = 0;
        if (row >= 0 && row < n_total) {
            const int64_t b = rowptr[row], e = rowptr[row + 1];
            for (int64_t k0 = b; k0 < e; k0 += kWave) {
                const bool keep = k0 + lane < e && mark[col[k0 + lane]] == epoch;
                cnt += __popcll(__ballot(keep));
            }
        } else if (lane == 0) {
            flag(info, kErrRow);
        }
        if (lane == 0) out_rowptr[r + 1] = cnt;
    }
}

// one workgroup: in-place inclusive scan of out_rowptr[1..n], out_rowptr[0] = 0, nnz into info
__global__ __launch_bounds__(kBlock) void block_scan_kernel(int64_t* __restrict__ out_rowptr, int64_t n_rows, int64_t* __restrict__ info) {
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

// Unsorted column sets (m <= 4096): every row owns a 128-word bitmap of its kept local ids (set entry-parallel with integer atomicOr),
// a wavefront per row turns it into word prefixes and the row's count, and an entry's position in its row is the number of set
// bits below its own -- ascending local ids whatever order the entries are visited in.
__global__ __launch_bounds__(kBlock) void block_bitmap_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const int64_t* __restrict__ rows, const int64_t* __restrict__ seg,
                                                              int64_t n_rows, const uint32_t* __restrict__ mark,
                                                              const int32_t* __restrict__ local, uint32_t epoch,
                                                              uint32_t* __restrict__ bitmap, int64_t* __restrict__ info) {
    const int64_t E = seg[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        int64_t r;
        const int32_t c = col[entry_at(rowptr, rows, seg, n_rows, e, r)];
        if (mark[c] != epoch) continue;
        const int32_t l = local[c];
        if (l < 0 || l >= kMaxLocal) { flag(info, kErrLocal); continue; }
        atomicOr(bitmap + r * kBitmapWords + (l >> 5), 1u << (l & 31));
    }
}

__global__ __launch_bounds__(kBlock) void block_prefix_kernel(const uint32_t* __restrict__ bitmap, int64_t n_rows, int32_t* __restrict__ below,
                                                              int64_t* __restrict__ out_rowptr) {
    const int lane = lane_id();
    for (int64_t r = wave_global(); r < n_rows; r += waves_total()) {
        const uint32_t* bm = bitmap + r * kBitmapWords;
        const int c0 = __popc(bm[2 * lane]), c1 = __popc(bm[2 * lane + 1]);
        int incl = c0 + c1;
        for (int off = 1; off < kWave; off <<= 1) {
            const int up = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += up;
        }
        below[r * kBitmapWords + 2 * lane] = incl - c0 - c1;
        below[r * kBitmapWords + 2 * lane + 1] = incl - c1;
        if (lane == kWave - 1) out_rowptr[r + 1] = incl;
    }
}

__global__ __launch_bounds__(kBlock) void block_fill_bitmap_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                   const float* __restrict__ val, const int64_t* __restrict__ rows,
                                                                   const int64_t* __restrict__ seg, int64_t n_rows,
                                                                   const uint32_t* __restrict__ mark, const int32_t* __restrict__ local,
                                                                   uint32_t epoch, const double* __restrict__ w,
                                                                   const uint32_t* __restrict__ bitmap, const int32_t* __restrict__ below,
                                                                   const int64_t* __restrict__ out_rowptr, int32_t* __restrict__ out_col,
                                                                   float* __restrict__ out_val) {
    const int64_t E = seg[n_rows];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < E; e += (int64_t)gridDim.x * kBlock) {
        int64_t r;
        const int64_t k = entry_at(rowptr, rows, seg, n_rows, e, r);
        const int32_t c = col[k];
        if (mark[c] != epoch) continue;
        const int32_t l = local[c];
        if (l < 0 || l >= kMaxLocal) continue;
        const int64_t word = r * kBitmapWords + (l >> 5);
        const int64_t pos = out_rowptr[r] + below[word] + __popc(bitmap[word] & ((1u << (l & 31)) - 1u));
        if (pos < out_rowptr[r + 1]) {
            out_col[pos] = l;
            out_val[pos] = (float)((val ? (double)val[k] : 1.0) * w[l]);
        }
    }
}

// Sorted column sets (local ids ascend with the global ids, so CSR order is local order): one wavefront per row, a ballot prefix
// places every kept entry.
__global__ __launch_bounds__(kBlock) void block_fill_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const float* __restrict__ val, const int64_t* __restrict__ rows, int64_t n_rows,
                                                            int64_t n_total, const uint32_t* __restrict__ mark, const int32_t* __restrict__ local,
                                                            uint32_t epoch, const double* __restrict__ w, const int64_t* __restrict__ out_rowptr,
                                                            int32_t* __restrict__ out_col, float* __restrict__ out_val) {
    const int lane = lane_id();
    for (int64_t r = wave_global(); r < n_rows; r += waves_total()) {
        const int64_t row = rows[r];
        if (row < 0 || row >= n_total) continue;
        const int64_t b = rowptr[row], e = rowptr[row + 1];
        const int64_t base = out_rowptr[r], room = out_rowptr[r + 1] - base;
        int64_t done = 0;
        for (int64_t k0 = b; k0 < e; k0 += kWave) {
            const int64_t k = k0 + lane;
            const int32_t c = k < e ? col[k] : 0;
            const bool keep = k < e && mark[c] == epoch;
            const unsigned long long bal = __ballot(keep);
            if (keep) {
                const int64_t pos = done + __popcll(bal & ((1ull << lane) - 1ull));
                const int32_t l = local[c];
                if (pos < room) {
                    out_col[base + pos] = l;
                    out_val[base + pos] = (float)((val ? (double)val[k] : 1.0) * w[l]);
                }
            }
            done += __popcll(bal);
        }
    }
}

inline int grid_for(int64_t work, int per_block) {
    const int64_t g = (work + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > kGrid ? kGrid : g));
}

}  // namespace lw
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_host_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4) {
    DGLL_REQUIRE(counter4 && key2 && out4, "counter, key and output must be non-NULL");
    lw::philox4x32_10(counter4, key2, out4);
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_column_mass(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, const int64_t* rows,
                                     int64_t n_rows, int64_t n_total, uint32_t* marker, uint32_t epoch, unsigned long long* mass,
                                     int shift, int flat, int32_t* cand, int64_t* info, unsigned long long* totals, int64_t* seg) {
    DGLL_REQUIRE(rowptr && col && marker && mass && cand && info && totals && (seg || !rows), "CSR, marker, mass, candidate, info, totals, seg");
    DGLL_REQUIRE(n_rows >= 0 && n_total > 0 && n_total < (1ll << 31) && shift >= 0 && shift <= 62 && epoch != 0,
                 "row count, node count < 2^31, fixed-point shift in [0, 62], non-zero epoch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DGLL_HIP_TRY(hipMemsetAsync(info, 0, 8 * sizeof(int64_t), st));
    DGLL_HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), st));
    if (n_rows > 0) {
        const int64_t* sg = rows ? seg : rowptr;
        if (rows) hipLaunchKernelGGL(lw::row_offsets_kernel, dim3(1), dim3(kBlock), 0, st, rowptr, rows, n_rows, n_total, seg, info);
        hipLaunchKernelGGL(lw::mark_columns_kernel, dim3(lw::kGrid), dim3(kBlock), 0, st, rowptr, col, rows, sg, n_rows, marker, epoch, mass,
                           cand, info);
        hipLaunchKernelGGL(lw::accumulate_mass_kernel, dim3(lw::kGrid), dim3(kBlock), 0, st, rowptr, col, val, rows, sg, n_rows,
                           ldexp(1.0, shift), mass);
        hipLaunchKernelGGL(lw::totals_kernel, dim3(lw::grid_for(n_total, kBlock)), dim3(kBlock), 0, st, cand, info, mass,
                           ldexp(1.0, -shift), flat, totals);
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_column_p(void* stream, const int64_t* ids, const int64_t* count, int64_t cap, const unsigned long long* mass,
                                  int shift, int flat, const unsigned long long* totals, double* p) {
    DGLL_REQUIRE(ids && mass && totals && p && cap >= 0 && shift >= 0 && shift <= 62, "ids, mass, totals, output, capacity, shift");
    if (cap == 0) return DGLL_OK;
    hipLaunchKernelGGL(lw::column_p_kernel, dim3(lw::grid_for(cap, kBlock)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), ids, count,
                       cap, mass, ldexp(1.0, -shift), flat, totals, p);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int64_t dgll_hip_lw_ctrl_words(void) { return lw::kCtrlWords; }

DGLL_API int dgll_hip_lw_select(void* stream, const int32_t* cand, const int64_t* cand_count, int64_t cand_cap, const unsigned long long* mass, int shift, int flat,
                                uint64_t seed, int layer, int64_t fanout, unsigned long long* keys, unsigned long long* ctrl,
                                unsigned long long* win_key, int32_t* win_id, int64_t win_cap, int64_t* out_ids, int64_t* info) {
    DGLL_REQUIRE(cand && cand_count && mass && keys && ctrl && win_key && win_id && out_ids && info, "candidates, mass, workspaces, output and info");
    DGLL_REQUIRE(cand_cap > 0 && fanout >= 1 && win_cap >= fanout && win_cap <= (1ll << 24) && shift >= 0 && shift <= 62 && layer >= 0,
                 "candidate capacity, fan-out >= 1, winner capacity >= fan-out, shift, layer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = lw::grid_for(cand_cap, kBlock);
    const double inv_scale = ldexp(1.0, -shift);
    DGLL_HIP_TRY(hipMemsetAsync(ctrl, 0, lw::kCtrlWords * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(lw::keys_kernel, dim3(grid), dim3(kBlock), 0, st, cand, cand_count, mass, inv_scale, flat, seed, (uint32_t)layer, keys, ctrl);
    hipLaunchKernelGGL(lw::select_init_kernel, dim3(1), dim3(64), 0, st, ctrl, fanout);
    for (int shift_bits = 56; shift_bits >= 0; shift_bits -= 8) {
        hipLaunchKernelGGL(lw::radix_hist_kernel, dim3(grid), dim3(kBlock), 0, st, keys, cand_count, ctrl, shift_bits);
        hipLaunchKernelGGL(lw::radix_pick_kernel, dim3(1), dim3(kBlock), 0, st, ctrl, shift_bits);
    }
    hipLaunchKernelGGL(lw::gather_winners_kernel, dim3(grid), dim3(kBlock), 0, st, keys, cand, cand_count, info, ctrl, win_key, win_id, win_cap);
    hipLaunchKernelGGL(lw::rank_winners_kernel, dim3((win_cap + kBlock - 1) / kBlock), dim3(kBlock), 0, st, win_key, win_id, ctrl, win_cap,
                       out_ids, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_union_sorted(void* stream, const int64_t* a, const int64_t* a_count, int64_t a_cap, const int64_t* b, int64_t nb,
                                      int64_t n_total, uint32_t* marker, uint32_t epoch, int64_t* reps, unsigned long long* n_reps,
                                      int64_t* out, int64_t* info) {
    DGLL_REQUIRE(a && a_count && (b || nb == 0) && marker && reps && n_reps && out && info, "lists, marker, workspaces, output, info");
    DGLL_REQUIRE(a_cap >= 0 && nb >= 0 && a_cap + nb > 0 && a_cap + nb <= (1ll << 24) && epoch != 0, "list sizes, non-zero epoch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DGLL_HIP_TRY(hipMemsetAsync(n_reps, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(lw::union_claim_kernel, dim3(lw::grid_for(a_cap + nb, kBlock)), dim3(kBlock), 0, st, a, a_count, a_cap, b, nb, n_total,
                       marker, epoch, reps, n_reps, info);
    hipLaunchKernelGGL(lw::union_rank_kernel, dim3((a_cap + nb + kBlock - 1) / kBlock), dim3(kBlock), 0, st, reps, n_reps, out, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_weights(void* stream, const double* p, const int64_t* m_dev, int64_t cap, const int64_t* snum_dev, int64_t snum,
                                 int64_t n_total, int mode, double* w) {
    DGLL_REQUIRE(p && w && cap >= 0 && n_total > 0 && (mode == 0 || mode == 1), "p, output, capacity, node count, mode 0 (WRS) or 1 (1/(p s))");
    DGLL_REQUIRE(mode == 0 || snum_dev || snum > 0, "1/(p s) needs s");
    if (cap == 0) return DGLL_OK;
    hipLaunchKernelGGL(lw::weights_kernel, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), p, m_dev, cap, snum_dev, snum, n_total,
                       mode, w);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_block_count(void* stream, const int64_t* rowptr, const int32_t* col, const int64_t* rows, int64_t n_rows,
                                     int64_t n_total, const int64_t* cols, const int64_t* m_dev, int64_t m_cap, uint32_t* mark,
                                     int32_t* local, uint32_t epoch, int sorted, int64_t* seg, uint32_t* bitmap, int32_t* below,
                                     int64_t* out_rowptr, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && (rows || n_rows == 0) && cols && mark && local && out_rowptr && info, "CSR, rows, columns, maps, output, info");
    DGLL_REQUIRE(sorted || (seg && bitmap && below && m_cap <= lw::kMaxLocal), "unsorted columns: at most 4096, seg / bitmap / below workspaces");
    DGLL_REQUIRE(n_rows >= 0 && n_total > 0 && m_cap >= 0 && epoch != 0, "row count, node count, column capacity, non-zero epoch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m_cap > 0)
        hipLaunchKernelGGL(lw::map_columns_kernel, dim3(lw::grid_for(m_cap, kBlock)), dim3(kBlock), 0, st, cols, m_dev, m_cap, n_total, mark,
                           local, epoch, info);
    if (n_rows > 0) {
        if (sorted) {
            hipLaunchKernelGGL(lw::block_count_kernel, dim3(lw::grid_for(n_rows, kWavesPerBlock)), dim3(kBlock), 0, st, rowptr, col, rows,
                               n_rows, n_total, mark, epoch, out_rowptr, info);
        } else {
            DGLL_HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)n_rows * lw::kBitmapWords * sizeof(uint32_t), st));
            hipLaunchKernelGGL(lw::row_offsets_kernel, dim3(1), dim3(kBlock), 0, st, rowptr, rows, n_rows, n_total, seg, info);
            hipLaunchKernelGGL(lw::block_bitmap_kernel, dim3(lw::kGrid), dim3(kBlock), 0, st, rowptr, col, rows, seg, n_rows, mark, local, epoch,
                               bitmap, info);
            hipLaunchKernelGGL(lw::block_prefix_kernel, dim3(lw::grid_for(n_rows, kWavesPerBlock)), dim3(kBlock), 0, st, bitmap, n_rows, below,
                               out_rowptr);
        }
    }
    hipLaunchKernelGGL(lw::block_scan_kernel, dim3(1), dim3(kBlock), 0, st, out_rowptr, n_rows, info);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}

DGLL_API int dgll_hip_lw_block_fill(void* stream, const int64_t* rowptr, const int32_t* col, const float* val, const int64_t* rows,
                                    int64_t n_rows, int64_t n_total, const uint32_t* mark, const int32_t* local, uint32_t epoch,
                                    const double* w, int sorted, int64_t m, const int64_t* seg, const uint32_t* bitmap, const int32_t* below,
                                    const int64_t* out_rowptr, int32_t* out_col, float* out_val, int64_t* info) {
    DGLL_REQUIRE(rowptr && col && (rows || n_rows == 0) && mark && local && w && out_rowptr && info, "CSR, rows, maps, weights, output, info");
    DGLL_REQUIRE(n_rows >= 0 && (sorted || (m <= lw::kMaxLocal && seg && bitmap && below)),
                 "row count; unsorted columns: at most 4096, the seg / bitmap / below of dgll_hip_lw_block_count");
    if (n_rows == 0) return DGLL_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sorted)
        hipLaunchKernelGGL(lw::block_fill_kernel, dim3(lw::grid_for(n_rows, kWavesPerBlock)), dim3(kBlock), 0, st, rowptr, col, val, rows,
                           n_rows, n_total, mark, local, epoch, w, out_rowptr, out_col, out_val);
    else
        hipLaunchKernelGGL(lw::block_fill_bitmap_kernel, dim3(lw::kGrid), dim3(kBlock), 0, st, rowptr, col, val, rows, seg, n_rows, mark,
                           local, epoch, w, bitmap, below, out_rowptr, out_col, out_val);
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
