// Runs the entry points of the unmodified segment_mm.hip on arrays read from DIR (dtype: 0 fp32, 1 bf16, as DGLL_F32 / DGLL_BF16):
//   emu fwd   DIR dtype M K N lda ldc R len_bytes rows_bytes bdtype sr sk sn bcount nranges b0 e0 b1 e1 ...
//       per range [b, e): dgll_hip_segment_mm_pack of b + b_i * sr into a buffer of exactly packed_bytes(e - b, K, N), then
//       dgll_hip_segment_mm with seg_begin = b, seg_end = e, build_plan = 1 for the first range and 0 after it.
//       In: a ((M - 1) lda + K rounded up to 16 bytes), b (bcount elements of bdtype), seglen (R), rows (M, when rows_bytes != 0).
//       Out: c (M * ldc elements; ldc == N puts its last element at the guard page), packed (the first range's), the plan arrays.
//   emu gradw DIR dtype M K N lda ldg R len_bytes rows_bytes
//       In: a, g (as a above), seglen, rows.  Out: gw fp32 [R, K, N], the plan arrays.
// Every buffer has exactly the size the API reports or requires and ends at a guard page; outputs and workspaces start as 0xCD bytes.
#include "segment_mm.hip"
#include "emu_runtime.hpp"

static int64_t arg(char** argv, int i) { return atoll(argv[i]); }
static int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); return 1; }
static size_t matrix_bytes(int64_t M, int64_t ld, int K, int dtype) {
    const int eb = dtype == DGLL_BF16 ? 2 : 4, epv = 16 / eb;
    return M > 0 ? (size_t)(((M - 1) * ld + (K + epv - 1) / epv * epv) * eb) : 0;
}
static void save_plan(const std::string& dir, void* ws, int64_t R) {
    const Plan pl = plan_at(ws, R);
    save(dir + "/segoff.bin", pl.segoff, (R + 2) * 8); save(dir + "/tileptr.bin", pl.tileptr, (R + 2) * 4);
    save(dir + "/partptr.bin", pl.partptr, (R + 2) * 4);
}

int main(int argc, char** argv) {
    if (argc < 12) return 1;
    const std::string op = argv[1], dir = argv[2];
    const int dtype = (int)arg(argv, 3), eb = dtype == DGLL_BF16 ? 2 : 4;
    const int64_t M = arg(argv, 4); const int K = (int)arg(argv, 5), N = (int)arg(argv, 6);
    const int64_t lda = arg(argv, 7), ld2 = arg(argv, 8), R = arg(argv, 9);
    const int len_bytes = (int)arg(argv, 10), rows_bytes = (int)arg(argv, 11);
    const void* a = load(dir + "/a.bin", matrix_bytes(M, lda, K, dtype));
    const void* seglen = load(dir + "/seglen.bin", R * len_bytes);
    const void* rows = rows_bytes ? load(dir + "/rows.bin", M * rows_bytes) : nullptr;
    if (op == "fwd") {
        if (argc < 18 || argc != 18 + 2 * arg(argv, 17)) return 1;
        const int bdtype = (int)arg(argv, 12), beb = bdtype == DGLL_BF16 ? 2 : 4;
        const int64_t sr = arg(argv, 13), sk = arg(argv, 14), sn = arg(argv, 15), bcount = arg(argv, 16), nranges = arg(argv, 17);
        const char* b = (const char*)load(dir + "/b.bin", bcount * beb);
        void* c = guarded(M * ld2 * eb);
        const int64_t ws_bytes = dgll_hip_segment_mm_workspace(R);
        void* ws = guarded(ws_bytes);
        for (int64_t i = 0; i < nranges; ++i) {
            const int64_t r0 = arg(argv, 18 + 2 * i), r1 = arg(argv, 19 + 2 * i);
            const int64_t pbytes = dgll_hip_segment_mm_packed_bytes(r1 - r0, K, N, dtype);
            void* packed = pbytes ? guarded(pbytes) : nullptr;
            if (dgll_hip_segment_mm_pack(nullptr, b + r0 * sr * beb, bdtype, sr, sk, sn, r1 - r0, K, N, dtype, packed)) return fail("pack");
            if (i == 0) save(dir + "/packed.bin", packed, pbytes);
            if (dgll_hip_segment_mm(nullptr, a, lda, dtype, packed, seglen, len_bytes, R, rows, rows_bytes ? rows_bytes : 8, c, ld2, M, K, N, r0, r1,
                                    i == 0, ws, ws_bytes)) return fail("segment_mm");
        }
        save(dir + "/c.bin", c, M * ld2 * eb);
        save_plan(dir, ws, R);
    } else if (op == "gradw") {
        const void* g = load(dir + "/g.bin", matrix_bytes(M, ld2, N, dtype));
        float* gw = (float*)guarded(R * K * N * 4);
        const int64_t ws_bytes = dgll_hip_segment_mm_gradw_workspace(M, R, K, N);
        void* ws = guarded((ws_bytes + 15) / 16 * 16);      // (the start must be 16-byte aligned: up to 12 bytes of slack where K N is odd)
        if (dgll_hip_segment_mm_gradw(nullptr, a, lda, g, ld2, dtype, seglen, len_bytes, R, rows, rows_bytes ? rows_bytes : 8, gw, (int64_t)K * N, N, M,
                                      K, N, ws, ws_bytes)) return fail("gradw");
        save(dir + "/gw.bin", gw, R * K * N * 4);
        save_plan(dir, ws, R);
    } else return 1;
    printf("emu ok\n");
    return 0;
}
