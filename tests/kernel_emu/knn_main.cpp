// Runs dgll_hip_knn (the unmodified knn.hip, included below) on arrays read from DIR and writes the results back:
//     emu DIR n D dtype ld n_segs k exclude_self nnz
// Inputs: x [n, ld] in the storage dtype (ld >= D), seg int64 [n_segs + 1], rowptr int64 [n + 1] (the output row pointers).
// Outputs: col int32 [nnz] and dist fp32 [nnz], and col_nodist [nnz] from a second call with out_dist == NULL.  The output buffers
// start as 0xCD bytes and end at a guard page.  Every builtin knn.hip uses has its stand-in in common.hpp.
#include "knn.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 10) return 1;
    std::string dir = argv[1];
    int64_t n = atoll(argv[2]), D = atoll(argv[3]); int dtype = atoi(argv[4]); int64_t ld = atoll(argv[5]), S = atoll(argv[6]);
    int k = atoi(argv[7]), excl = atoi(argv[8]); int64_t nnz = atoll(argv[9]);
    size_t esz = dtype == 0 ? 4 : 2;
    const void* x = load(dir + "/x.bin", n * ld * esz);
    const int64_t* seg = (const int64_t*)load(dir + "/seg.bin", (S + 1) * 8);
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n + 1) * 8);
    int32_t* col = (int32_t*)guarded(nnz * 4); float* dist = (float*)guarded(nnz * 4); int32_t* col2 = (int32_t*)guarded(nnz * 4);
    if (dgll_hip_knn(nullptr, x, ld, dtype, n, D, seg, S, k, excl, rowptr, col, dist, nnz)) { fprintf(stderr, "knn: %s\n", dgll::last_error.c_str()); return 1; }
    if (dgll_hip_knn(nullptr, x, ld, dtype, n, D, seg, S, k, excl, rowptr, col2, nullptr, nnz)) { fprintf(stderr, "knn: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/col.bin", col, nnz * 4); save(dir + "/dist.bin", dist, nnz * 4); save(dir + "/col_nodist.bin", col2, nnz * 4);
    printf("emu ok\n");
    return 0;
}
