// Runs dgll_hip_radius (the unmodified radius.hip with csrc/scan.hpp) on arrays read from DIR:
//     emu DIR m n D dtype ld_y ld_x n_segs r2 K exclude_self square      (square: the queries ARE x)
// Out: rowptr int64 [m + 1], nnz, col int32 and dist fp32 at their capacity m K.
// Outputs start as 0xCD bytes and end at a guard page.
#include "common.hpp"
inline int __popc(uint32_t v) { return __builtin_popcount(v); }     // scan.hpp's bitmap scan, not used here
#include "radius.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    std::string dir = argc == 13 ? argv[1] : (exit(1), "");
    int64_t m = atoll(argv[2]), n = atoll(argv[3]), D = atoll(argv[4]); int dtype = atoi(argv[5]);
    int64_t ld_y = atoll(argv[6]), ld_x = atoll(argv[7]), S = atoll(argv[8]); float r2 = (float)atof(argv[9]);
    int K = atoi(argv[10]), excl = atoi(argv[11]), square = atoi(argv[12]);
    size_t esz = dtype == 0 ? 4 : 2; const void* x = load(dir + "/x.bin", n * ld_x * esz);
    const void* y = square ? x : load(dir + "/y.bin", m * ld_y * esz);
    const int64_t* xseg = (const int64_t*)load(dir + "/xseg.bin", (S + 1) * 8);
    const int64_t* yseg = square ? xseg : (const int64_t*)load(dir + "/yseg.bin", (S + 1) * 8);
    int64_t* rowptr = (int64_t*)guarded((m + 1) * 8); int64_t* nnz = (int64_t*)guarded(8);
    int32_t* col = (int32_t*)guarded(m * K * 4); float* dist = (float*)guarded(m * K * 4);
    int32_t* scratch = (int32_t*)guarded((m * K + m) * 4);
    if (dgll_hip_radius(nullptr, y, ld_y, m, yseg, x, ld_x, n, xseg, S, dtype, D, r2, K, excl, rowptr, col, dist, nnz, scratch)) { fprintf(stderr, "radius: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/rowptr.bin", rowptr, (m + 1) * 8); save(dir + "/nnz.bin", nnz, 8); save(dir + "/col.bin", col, m * K * 4);
    save(dir + "/dist.bin", dist, m * K * 4);
    printf("emu ok\n");
    return 0;
}
