// Runs the three passes of dgll_hip_gatv2_pass (the unmodified gatv2.hip, included below) on arrays read from DIR and writes the
// results back:  emu DIR n_dst n_src heads D dtype slope dattn_blocks.  Inputs: rowptr / col (A), trowptr / tcol (A^T), xl, xr, g
// in the storage dtype, attn fp32.
#include "gatv2.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 9) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); int heads = atoi(argv[4]), D = atoi(argv[5]), dtype = atoi(argv[6]);
    float slope = atof(argv[7]); int64_t blocks = atoll(argv[8]);
    size_t esz = dtype == 0 ? 4 : 2, F = (size_t)heads * D;
    dgll_gatv2_desc d; memset(&d, 0, sizeof d);
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    void* xl = load(dir + "/xl.bin", n_src * F * esz); void* xr = load(dir + "/xr.bin", n_dst * F * esz);
    void* g = load(dir + "/g.bin", n_dst * F * esz); float* attn = (float*)load(dir + "/attn.bin", F * 4);
    void* out = guarded(n_dst * F * esz); float* lse = (float*)guarded(n_dst * heads * 4);
    void* dxr = guarded(n_dst * F * esz); void* dxl = guarded(n_src * F * esz);
    float* ld2 = (float*)guarded(n_dst * 2 * heads * 4); float* part = (float*)guarded(blocks * F * 4); float* dattn = (float*)guarded(F * 4);
    d.dtype = dtype; d.heads = heads; d.D = D; d.slope = slope;
    d.xl = xl; d.ld_xl = F; d.xr = xr; d.ld_xr = F; d.attn = attn; d.ld_out = F; d.grad_out = g; d.ld_grad_out = F;
    d.pass = DGLL_GATV2_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src; d.out = out; d.lse = lse;
    if (dgll_hip_gatv2_pass(nullptr, &d)) { fprintf(stderr, "fwd: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_GATV2_ROWS; d.out = dxr; d.lse_delta = ld2; d.dattn_part = part; d.dattn_blocks = blocks; d.dattn = dattn;
    if (dgll_hip_gatv2_pass(nullptr, &d)) { fprintf(stderr, "rows: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_GATV2_TRANSPOSED; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst; d.out = dxl; d.lse = nullptr; d.dattn_part = nullptr; d.dattn = nullptr;
    if (dgll_hip_gatv2_pass(nullptr, &d)) { fprintf(stderr, "cols: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/out.bin", out, n_dst * F * esz); save(dir + "/lse.bin", lse, n_dst * heads * 4); save(dir + "/dxr.bin", dxr, n_dst * F * esz);
    save(dir + "/dxl.bin", dxl, n_src * F * esz); save(dir + "/dattn.bin", dattn, F * 4);
    printf("emu ok\n");
    return 0;
}
