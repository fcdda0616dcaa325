// Runs the three passes of dgll_hip_sparse_attn_pass (the unmodified sparse_attn.hip, included below) on arrays read from DIR and
// writes the results back:  emu DIR n_dst n_src heads D dtype scale kv_shared.  Inputs: rowptr / col (A), trowptr / tcol
// (A^T), q, k, v, g in the storage dtype (kv_shared: v is not read, k serves both).
#include "sparse_attn.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    if (argc < 9) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); int heads = atoi(argv[4]), D = atoi(argv[5]), dtype = atoi(argv[6]);
    float scale = atof(argv[7]); int shared = atoi(argv[8]);
    size_t esz = dtype == 0 ? 4 : 2, F = (size_t)heads * D;
    dgll_attn_desc d; memset(&d, 0, sizeof d);
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    void* q = load(dir + "/q.bin", n_dst * F * esz); void* k = load(dir + "/k.bin", n_src * F * esz);
    void* v = shared ? k : load(dir + "/v.bin", n_src * F * esz);
    void* g = load(dir + "/g.bin", n_dst * F * esz);
    void* out = guarded(n_dst * F * esz); float* lse = (float*)guarded(n_dst * heads * 4);
    void* dq = guarded(n_dst * F * esz); void* dk = guarded(n_src * F * esz); void* dv = guarded(n_src * F * esz);
    float* ld2 = (float*)guarded(n_dst * 2 * heads * 4);
    d.dtype = dtype; d.heads = heads; d.D = D; d.scale = scale; d.kv_shared = shared;
    d.q = q; d.ld_q = F; d.k = k; d.ld_k = F; d.v = v; d.ld_v = F; d.ld_out = F; d.ld_out2 = F; d.grad_out = g; d.ld_grad_out = F;
    d.pass = DGLL_ATTN_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src; d.out = out; d.lse = lse;
    if (dgll_hip_sparse_attn_pass(nullptr, &d)) { fprintf(stderr, "fwd: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_ATTN_ROWS; d.out = dq; d.lse_delta = ld2;
    if (dgll_hip_sparse_attn_pass(nullptr, &d)) { fprintf(stderr, "rows: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_ATTN_COLS; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst; d.out = dk; d.out2 = dv; d.lse = nullptr;
    if (dgll_hip_sparse_attn_pass(nullptr, &d)) { fprintf(stderr, "cols: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/out.bin", out, n_dst * F * esz); save(dir + "/lse.bin", lse, n_dst * heads * 4); save(dir + "/dq.bin", dq, n_dst * F * esz);
    save(dir + "/dk.bin", dk, n_src * F * esz); save(dir + "/dv.bin", dv, n_src * F * esz);
    printf("emu ok\n");
    return 0;
}
