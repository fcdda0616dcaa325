// Runs the three passes of dgll_hip_typed_spmm_pass (the unmodified typed_spmm.hip, included below) on arrays read from DIR and
// writes the results back:  emu DIR n_dst n_src F B R dtype has_norm.  Inputs: rowptr / col / etype / norm (A), trowptr /
// tcol / tetype / tnorm (A^T, its own entry order), coeff fp32 [R, B], x [n_src, F] and dz [n_dst, B * F] in the storage dtype.
// Outputs: z [n_dst, B * F], dx [n_src, F], p fp32 [nnz, B rounded up to 4].
#include "typed_spmm.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 9) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]), F = atoll(argv[4]); int B = atoi(argv[5]), R = atoi(argv[6]), dtype = atoi(argv[7]);
    int has_norm = atoi(argv[8]);
    size_t esz = dtype == 0 ? 4 : 2, ldp = (size_t)(B + 3) / 4 * 4;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int32_t* etype = (const int32_t*)load(dir + "/etype.bin", nnz * 4); const int32_t* tetype = (const int32_t*)load(dir + "/tetype.bin", nnz * 4);
    const float* norm = has_norm ? (const float*)load(dir + "/norm.bin", nnz * 4) : nullptr;
    const float* tnorm = has_norm ? (const float*)load(dir + "/tnorm.bin", nnz * 4) : nullptr;
    const float* coeff = (const float*)load(dir + "/coeff.bin", (size_t)R * B * 4);
    void* x = load(dir + "/x.bin", n_src * F * esz); void* dz = load(dir + "/dz.bin", n_dst * B * F * esz);
    void* z = guarded(n_dst * B * F * esz); void* dx = guarded(n_src * F * esz); float* p = (float*)guarded(nnz * ldp * 4);
    dgll_typed_desc d; memset(&d, 0, sizeof d);
    d.dtype = dtype; d.R = R; d.B = B; d.F = F; d.coeff = coeff; d.x = x; d.ld_x = F; d.dz = dz; d.ld_dz = B * F;
    d.pass = DGLL_TYPED_EXPAND; d.rowptr = rowptr; d.col = col; d.etype = etype; d.norm = norm; d.n_rows = n_dst; d.n_cols = n_src;
    d.out = z; d.ld_out = B * F;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "expand: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_TYPED_EDGE_DOTS; d.out = nullptr; d.ld_out = 0; d.p = p; d.ld_p = ldp; d.etype = nullptr; d.norm = nullptr; d.coeff = nullptr;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "dots: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_TYPED_CONTRACT; d.rowptr = trowptr; d.col = tcol; d.etype = tetype; d.norm = tnorm; d.coeff = coeff; d.n_rows = n_src; d.n_cols = n_dst;
    d.out = dx; d.ld_out = F; d.p = nullptr; d.ld_p = 0; d.x = nullptr; d.ld_x = 0;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "contract: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/z.bin", z, n_dst * B * F * esz); save(dir + "/dx.bin", dx, n_src * F * esz); save(dir + "/p.bin", p, nnz * ldp * 4);
    printf("emu ok\n");
    return 0;
}
