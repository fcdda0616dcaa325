// Runs the three passes of dgll_hip_gmm_pass (the unmodified gmm.hip, included below) on arrays read from DIR and writes the results
// back:  emu DIR n_dst n_src F K dim dtype ld_pseudo has_scale partials.  Inputs: rowptr / col (A), trowptr / tcol / perm (A^T and its
// entry -> A's entry), scale fp32 [n_dst], pseudo fp32 [nnz, ld_pseudo], mu / sigma fp32 [K, dim], x [n_src, F] and dz [n_dst, K * F] in
// the storage dtype, p fp32 [nnz, K rounded up to 4].  Outputs: z [n_dst, K * F], dx [n_src, F], gp fp32 [nnz, dim], slabs fp32
// [partials, 2, K, dim].
#include "gmm.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 11) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]), F = atoll(argv[4]); int K = atoi(argv[5]), dim = atoi(argv[6]), dtype = atoi(argv[7]);
    int64_t ld_pseudo = atoll(argv[8]); int has_scale = atoi(argv[9]); int64_t partials = atoll(argv[10]);
    size_t esz = dtype == 0 ? 4 : 2, ldp = (size_t)(K + 3) / 4 * 4;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    const float* scale = has_scale ? (const float*)load(dir + "/scale.bin", n_dst * 4) : nullptr;
    const float* pseudo = (const float*)load(dir + "/pseudo.bin", nnz * ld_pseudo * 4);
    const float* mu = (const float*)load(dir + "/mu.bin", (size_t)K * dim * 4); const float* sigma = (const float*)load(dir + "/sigma.bin", (size_t)K * dim * 4);
    void* x = load(dir + "/x.bin", n_src * F * esz); void* dz = load(dir + "/dz.bin", n_dst * K * F * esz);
    const float* p = (const float*)load(dir + "/p.bin", nnz * ldp * 4);
    void* z = guarded(n_dst * K * F * esz); void* dx = guarded(n_src * F * esz);
    float* gp = (float*)guarded(nnz * dim * 4); float* slabs = (float*)guarded((size_t)partials * 2 * K * dim * 4);
    dgll_gmm_desc d; memset(&d, 0, sizeof d);
    d.dtype = dtype; d.K = K; d.dim = dim; d.F = F; d.nnz = nnz; d.pseudo = pseudo; d.ld_pseudo = ld_pseudo; d.mu = mu; d.inv_sigma = sigma;
    d.pass = DGLL_GMM_EXPAND; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src; d.scale = scale;
    d.x = x; d.ld_x = F; d.out = z; d.ld_out = K * F;
    if (dgll_hip_gmm_pass(nullptr, &d)) { fprintf(stderr, "expand: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_GMM_CONTRACT; d.rowptr = trowptr; d.col = tcol; d.perm = perm; d.n_rows = n_src; d.n_cols = n_dst; d.scale = nullptr;
    d.x = nullptr; d.ld_x = 0; d.dz = dz; d.ld_dz = K * F; d.out = dx; d.ld_out = F;
    if (dgll_hip_gmm_pass(nullptr, &d)) { fprintf(stderr, "contract: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_GMM_PARAM; d.rowptr = nullptr; d.col = nullptr; d.perm = nullptr; d.dz = nullptr; d.ld_dz = 0; d.out = nullptr; d.ld_out = 0;
    d.p = p; d.ld_p = ldp; d.grad_pseudo = gp; d.ld_grad_pseudo = dim; d.slabs = slabs; d.partials = partials;
    if (dgll_hip_gmm_pass(nullptr, &d)) { fprintf(stderr, "param: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/z.bin", z, n_dst * K * F * esz); save(dir + "/dx.bin", dx, n_src * F * esz);
    save(dir + "/gp.bin", gp, nnz * dim * 4); save(dir + "/slabs.bin", slabs, (size_t)partials * 2 * K * dim * 4);
    printf("emu ok\n");
    return 0;
}
