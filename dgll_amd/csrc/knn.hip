// knn.hip -- dgll_hip_knn: exact k nearest neighbours inside contiguous segments of a point set (DGL's knn_graph / segmented_knn_graph,
// the graph Dynamic Graph CNN rebuilds from the features in every layer).  The contract is in include/dgll_hip.h; DESIGN.md 4.4k says
// why the geometry is what it is.
//
// One launch, nothing per pair in memory.  A workgroup of 256 lanes takes tiles of DGLL_KNN_QUERY_TILE = 256 consecutive rows from a
// bounded grid, lane t owning row r0 + t.  A tile may touch several segments: the workgroup walks them in order (the first by a binary
// search of seg_ptr), and only the lanes whose row lies in the current segment take part in its distances.  The segment's rows stream
// through LDS in tiles of DGLL_KNN_CAND_TILE = 32 rows by kChunk = 32 columns, converted to fp32; every lane reads the same candidate
// vector (a broadcast, no bank conflict) and keeps 32 partial distances in registers.  The query row sits in registers when D <= 32
// and is re-read from global memory (the L2) chunk by chunk above that: 256 query rows of 256 fp32 columns are 256 KiB and fit no LDS.
// Each lane keeps its current top-k as a binary max-heap on the key (d, j) in LDS, entry m of lane t at [m][t] (a lane stays on its
// own bank whatever m it is at), and the root -- its k-th key -- in registers: a candidate is compared with that key first, so once
// the heap has filled an insertion is rare for a lane.  It is not rare for a WAVE (64 lanes, each with its own key), so the lanes first
// mark the candidates of a tile that beat their key in a bit mask and then insert side by side: the wave loops as often as its busiest
// lane has candidates.  A heap because the wave pays for the slowest lane: log2 k steps where a sorted list costs up to k.  The keys
// (d, j) of a lane are distinct, so the result is the same whatever the order of insertion: among equal distances the smaller index
// wins.  A heap sort in place puts the column in ascending order before it is written out.
#include "common.hpp"

namespace dgll {
namespace knn {

constexpr int kQueryTile = DGLL_KNN_QUERY_TILE, kCandTile = DGLL_KNN_CAND_TILE, kChunk = 32;
constexpr int kMaxGrid = 2048;
static_assert(kQueryTile == kBlock, "one lane per query");
static_assert(kCandTile * (kChunk / 8) <= kBlock, "one lane stages eight columns of one candidate row");

__device__ __forceinline__ float load_one(const float* p) { return *p; }
__device__ __forceinline__ float load_one(const bf16_t* p) { return bf16_lo((uint32_t)*p); }
// eight columns from a 16-byte aligned address; left > 0 of them belong to the row
__device__ __forceinline__ void load_vec8(const float* p, int left, float (&f)[8]) {
    float a[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    VecIO<float, 4>::unpack(VecIO<float, 4>::load(p), a);
    if (left > 4) VecIO<float, 4>::unpack(VecIO<float, 4>::load(p + 4), b);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}
__device__ __forceinline__ void load_vec8(const bf16_t* p, int left, float (&f)[8]) {
    (void)left;
    VecIO<bf16_t, 8>::unpack(VecIO<bf16_t, 8>::load(p), f);
}
// columns col0 .. col0 + 7 of a row as fp32; zero from column D on, whatever the memory behind the row holds
template <typename T, bool VEC>
__device__ __forceinline__ void load8(const T* row, int col0, int D, float (&f)[8]) {
    const int left = D - col0;
    if (left <= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.0f;
        return;
    }
    if (VEC) {
        load_vec8(row + col0, left, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e >= left) f[e] = 0.0f;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = e < left ? load_one(row + col0 + e) : 0.0f;
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void load_query_chunk(const T* row, int col0, int D, float (&q)[kChunk]) {
#pragma unroll
    for (int o = 0; o < kChunk / 8; ++o) {
        float f[8];
        load8<T, VEC>(row, col0 + o * 8, D, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[o * 8 + e] = f[e];
    }
}

// ---- a lane's current top-k: a binary max-heap on the key (d, j) in column t of s_d / s_j (entry m at [m][t]) -----------------------
// The keys of one lane are distinct (j is), so the k smallest and their order do not depend on how the heap was built.
__device__ __forceinline__ bool key_above(float d1, int32_t j1, float d2, int32_t j2) { return d1 > d2 || (d1 == d2 && j1 > j2); }

// put (d, j) at the root of the heap of `size` entries and let it sink
template <int KCAP>
__device__ __forceinline__ void sift_down(float (&s_d)[KCAP][kBlock], int32_t (&s_j)[KCAP][kBlock], int t, int size, float d, int32_t j) {
    int m = 0;
    for (;;) {
        int l = 2 * m + 1;
        if (l >= size) break;
        float cd = s_d[l][t];
        int32_t cj = s_j[l][t];
        if (l + 1 < size) {
            const float rd = s_d[l + 1][t];
            const int32_t rj = s_j[l + 1][t];
            if (key_above(rd, rj, cd, cj)) { ++l; cd = rd; cj = rj; }
        }
        if (!key_above(cd, cj, d, j)) break;
        s_d[m][t] = cd;
        s_j[m][t] = cj;
        m = l;
    }
    s_d[m][t] = d;
    s_j[m][t] = j;
}

// append (d, j) to the heap of `size` < k entries and let it rise
template <int KCAP>
__device__ __forceinline__ void sift_up(float (&s_d)[KCAP][kBlock], int32_t (&s_j)[KCAP][kBlock], int t, int size, float d, int32_t j) {
    int m = size;
    while (m > 0) {
        const int p = (m - 1) >> 1;
        const float pd = s_d[p][t];
        const int32_t pj = s_j[p][t];
        if (!key_above(d, j, pd, pj)) break;
        s_d[m][t] = pd;
        s_j[m][t] = pj;
        m = p;
    }
    s_d[m][t] = d;
    s_j[m][t] = j;
}

// VEC: x is 16-byte aligned on a pitch of whole 16-byte vectors.  KCAP >= k: the heap's capacity.
template <typename T, bool VEC, int KCAP>
__global__ __launch_bounds__(kBlock) void knn_kernel(const T* x, int64_t ld, int64_t n, int D, const int64_t* seg_ptr, int64_t S, int k,
                                                     int exclude_self, const int64_t* out_rowptr, int32_t* out_col, float* out_dist,
                                                     int64_t out_nnz, int64_t n_tiles) {
    __shared__ __attribute__((aligned(16))) float s_c[kCandTile][kChunk];
    __shared__ float s_d[KCAP][kBlock];
    __shared__ int32_t s_j[KCAP][kBlock];
    const int t = (int)threadIdx.x;
    const int nch = (D + kChunk - 1) / kChunk;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r0 = tile * kQueryTile, r1 = r0 + kQueryTile < n ? r0 + kQueryTile : n;
        const int64_t i = r0 + t;
        const bool in_range = i < n;
        const T* qrow = x + (in_range ? i : r0) * ld;
        // the first segment that ends behind r0 (S: none)
        int64_t lo = 0, hi = S;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (seg_ptr[mid + 1] > r0) hi = mid; else lo = mid + 1;
        }
        int cnt = 0;                                    // entries of this lane's list, and its k-th key once cnt == k
        float wd = INFINITY;
        int32_t wj = 0x7fffffff;
        float q[kChunk];
        if (nch == 1) {
            if (in_range) load_query_chunk<T, VEC>(qrow, 0, D, q);
            else {
#pragma unroll
                for (int e = 0; e < kChunk; ++e) q[e] = 0.0f;
            }
        }
        for (int64_t s = uniform64(lo); s < S; ++s) {
            int64_t b = uniform64(seg_ptr[s]), e = uniform64(seg_ptr[s + 1]);
            if (b < 0) b = 0;
            if (e > n) e = n;
            if (b >= r1) break;
            const bool active = in_range && i >= b && i < e;
            for (int64_t c0 = b; c0 < e; c0 += kCandTile) {
                const int cn = e - c0 < kCandTile ? (int)(e - c0) : kCandTile;
                float acc[kCandTile];
#pragma unroll
                for (int c = 0; c < kCandTile; ++c) acc[c] = 0.0f;
                for (int ch = 0; ch < nch; ++ch) {
                    __syncthreads();                    // the readers of the previous chunk are done
                    if (t < kCandTile * (kChunk / 8)) {
                        const int r = t / (kChunk / 8), o = t % (kChunk / 8);
                        float f[8];
                        if (r < cn) load8<T, VEC>(x + (c0 + r) * ld, ch * kChunk + o * 8, D, f);
                        else {
#pragma unroll
                            for (int u = 0; u < 8; ++u) f[u] = 0.0f;
                        }
                        const float f0[4] = {f[0], f[1], f[2], f[3]}, f1[4] = {f[4], f[5], f[6], f[7]};
                        VecIO<float, 4>::store(&s_c[r][o * 8], f0);
                        VecIO<float, 4>::store(&s_c[r][o * 8 + 4], f1);
                    }
                    __syncthreads();
                    if (active) {
                        if (nch > 1) load_query_chunk<T, VEC>(qrow, ch * kChunk, D, q);
                        const int dl = D - ch * kChunk;
#pragma unroll
                        for (int v = 0; v < kChunk / 4; ++v) {
                            if (v * 4 < dl) {
#pragma unroll
                                for (int c = 0; c < kCandTile; ++c) {
                                    float cv[4];
                                    VecIO<float, 4>::unpack(VecIO<float, 4>::load(&s_c[c][v * 4]), cv);
#pragma unroll
                                    for (int u = 0; u < 4; ++u) {
                                        const float df = q[v * 4 + u] - cv[u];
                                        acc[c] += df * df;
                                    }
                                }
                            }
                        }
                    }
                }
                if (active) {
                    // The tile's candidates that beat this lane's k-th key as it stands, as a bit mask; the key only falls, so no
                    // other candidate can enter the list.  The lanes then insert their own candidates side by side: the wave loops
                    // as often as its busiest lane has candidates, not once for every candidate that any of its lanes takes.
                    uint32_t take = 0;
#pragma unroll
                    for (int c = 0; c < kCandTile; ++c) {
                        float d = acc[c];
                        if (!(d == d)) d = INFINITY;                        // a NaN distance sorts as +inf
                        acc[c] = d;
                        const int32_t j = (int32_t)(c0 + c);
                        const bool skip = c >= cn || (exclude_self != 0 && c0 + c == i);
                        if (!skip && (cnt < k || d < wd || (d == wd && j < wj))) take |= 1u << c;
                    }
                    while (take != 0) {
                        const int c = __builtin_ctz(take);                  // ascending: equal distances keep the smaller index
                        take &= take - 1;
                        float d = acc[0];
#pragma unroll
                        for (int u = 1; u < kCandTile; ++u) d = u == c ? acc[u] : d;
                        const int32_t j = (int32_t)(c0 + c);
                        if (cnt < k) {
                            sift_up<KCAP>(s_d, s_j, t, cnt, d, j);
                            ++cnt;
                        } else if (key_above(wd, wj, d, j)) {
                            sift_down<KCAP>(s_d, s_j, t, k, d, j);          // replaces the root, the k-th key
                        }
                        if (cnt == k) { wd = s_d[0][t]; wj = s_j[0][t]; }
                    }
                }
            }
        }
        if (in_range && cnt > 0) {
            // heap sort in place: the largest key goes behind the shrinking heap, so the column ends ascending in (d, j)
            for (int m = cnt - 1; m > 0; --m) {
                const float d = s_d[m][t];
                const int32_t j = s_j[m][t];
                s_d[m][t] = s_d[0][t];
                s_j[m][t] = s_j[0][t];
                sift_down<KCAP>(s_d, s_j, t, m, d, j);
            }
            const int64_t pos = out_rowptr[i];
            for (int m = 0; m < cnt; ++m) {
                if (pos + m >= 0 && pos + m < out_nnz) {
                    out_col[pos + m] = s_j[m][t];
                    if (out_dist != nullptr) out_dist[pos + m] = s_d[m][t];
                }
            }
        }
    }
}

template <typename T, bool VEC>
void launch(int k, dim3 grid, hipStream_t st, const T* x, int64_t ld, int64_t n, int D, const int64_t* seg_ptr, int64_t S, int excl,
            const int64_t* out_rowptr, int32_t* out_col, float* out_dist, int64_t out_nnz, int64_t n_tiles) {
    if (k <= 32) hipLaunchKernelGGL((knn_kernel<T, VEC, 32>), grid, dim3(kBlock), 0, st, x, ld, n, D, seg_ptr, S, k, excl, out_rowptr, out_col,
                                    out_dist, out_nnz, n_tiles);
    else hipLaunchKernelGGL((knn_kernel<T, VEC, DGLL_KNN_MAX_K>), grid, dim3(kBlock), 0, st, x, ld, n, D, seg_ptr, S, k, excl, out_rowptr,
                            out_col, out_dist, out_nnz, n_tiles);
}

}  // namespace knn
}  // namespace dgll

using namespace dgll;

DGLL_API int dgll_hip_knn(void* stream, const void* x, int64_t ld_x, int dtype, int64_t n, int64_t D, const int64_t* seg_ptr, int64_t n_segs,
                          int k, int exclude_self, const int64_t* out_rowptr, int32_t* out_col, float* out_dist, int64_t out_nnz) {
    DGLL_REQUIRE(dtype == DGLL_F32 || dtype == DGLL_BF16, "dgll_hip_knn: dtype must be DGLL_F32 or DGLL_BF16");
    DGLL_REQUIRE(k >= 1 && k <= DGLL_KNN_MAX_K, "dgll_hip_knn: k must be in [1, 64] (DGLL_KNN_MAX_K)");
    DGLL_REQUIRE(D >= 1 && D <= DGLL_KNN_MAX_D, "dgll_hip_knn: D must be in [1, 256] (DGLL_KNN_MAX_D)");
    DGLL_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "dgll_hip_knn: n must be in [0, 2^31): the neighbours are int32 row ids");
    DGLL_REQUIRE(n_segs >= 0 && out_nnz >= 0, "dgll_hip_knn: n_segs and out_nnz must be >= 0");
    DGLL_REQUIRE(ld_x >= D, "dgll_hip_knn: the row pitch ld_x must be >= D");
    if (n == 0 || n_segs == 0 || out_nnz == 0) return DGLL_OK;
    DGLL_REQUIRE(x != nullptr && seg_ptr != nullptr && out_rowptr != nullptr && out_col != nullptr,
                 "dgll_hip_knn: x, seg_ptr, out_rowptr and out_col must be non-NULL");
    const size_t esz = dtype == DGLL_F32 ? 4 : 2;
    const bool vec = aligned16(x) && ((size_t)ld_x * esz) % 16 == 0;
    const int64_t n_tiles = (n + knn::kQueryTile - 1) / knn::kQueryTile;
    const dim3 grid((unsigned)(n_tiles < knn::kMaxGrid ? n_tiles : knn::kMaxGrid));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int excl = exclude_self != 0, Di = (int)D;
    if (dtype == DGLL_F32) {
        const float* xp = static_cast<const float*>(x);
        if (vec) knn::launch<float, true>(k, grid, st, xp, ld_x, n, Di, seg_ptr, n_segs, excl, out_rowptr, out_col, out_dist, out_nnz, n_tiles);
        else knn::launch<float, false>(k, grid, st, xp, ld_x, n, Di, seg_ptr, n_segs, excl, out_rowptr, out_col, out_dist, out_nnz, n_tiles);
    } else {
        const bf16_t* xp = static_cast<const bf16_t*>(x);
        if (vec) knn::launch<bf16_t, true>(k, grid, st, xp, ld_x, n, Di, seg_ptr, n_segs, excl, out_rowptr, out_col, out_dist, out_nnz, n_tiles);
        else knn::launch<bf16_t, false>(k, grid, st, xp, ld_x, n, Di, seg_ptr, n_segs, excl, out_rowptr, out_col, out_dist, out_nnz, n_tiles);
    }
    DGLL_HIP_TRY(hipGetLastError());
    return DGLL_OK;
}
