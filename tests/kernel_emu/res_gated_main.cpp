// Runs the three passes of dgll_hip_res_gated_pass (the unmodified res_gated.hip, included below) on arrays read from DIR and writes
// the results back:  emu DIR n_dst n_src F dtype ld mean
// Inputs: rowptr / col (A), trowptr / tcol (A^T), k and go [n_dst, F], q and v [n_src, ld] in the storage dtype (ld >= F: q, v and grad_q
// sit on that pitch).  mean != 0: the forward divides every row by its entry count (the other passes do not read the flag).
// Outputs: out, gk [n_dst, F]; gq [n_src, ld] (the columns past F keep the fill), gv [n_src, F]; gq_only [n_src, ld] and gv_only
// [n_src, F] from the cols pass with one output alone (and then without v for gv_only).
inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
#include "res_gated.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_res_gated_desc& d) {
    if (dgll_hip_res_gated_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 8) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]); size_t ld = atoll(argv[6]);
    int mean = atoi(argv[7]);
    size_t esz = dtype == 0 ? 4 : 2;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    void* k = load(dir + "/k.bin", n_dst * F * esz); void* go = load(dir + "/go.bin", n_dst * F * esz);
    void* q = load(dir + "/q.bin", n_src * ld * esz); void* v = load(dir + "/v.bin", n_src * ld * esz);
    void* out = guarded(n_dst * F * esz); void* gk = guarded(n_dst * F * esz);
    void* gq = guarded(n_src * ld * esz); void* gv = guarded(n_src * F * esz); void* gq2 = guarded(n_src * ld * esz); void* gv2 = guarded(n_src * F * esz);
    dgll_res_gated_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.F = F; base.k = k; base.ld_k = F; base.q = q; base.ld_q = ld;

    dgll_res_gated_desc d = base;
    d.pass = DGLL_RES_GATED_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src; d.mean = mean;
    d.v = v; d.ld_v = ld; d.out = out; d.ld_out = F;
    run("forward", d);

    d = base;
    d.pass = DGLL_RES_GATED_ROWS; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
    d.v = v; d.ld_v = ld; d.grad_out = go; d.ld_grad_out = F; d.grad_k = gk; d.ld_grad_k = F;
    run("rows", d);

    dgll_res_gated_desc t = base;
    t.pass = DGLL_RES_GATED_COLS; t.rowptr = trowptr; t.col = tcol; t.n_rows = n_src; t.n_cols = n_dst; t.grad_out = go; t.ld_grad_out = F;
    d = t;
    d.v = v; d.ld_v = ld; d.grad_q = gq; d.ld_grad_q = ld; d.grad_v = gv; d.ld_grad_v = F;
    run("cols", d);
    d = t;
    d.v = v; d.ld_v = ld; d.grad_q = gq2; d.ld_grad_q = ld;
    run("cols (grad_q alone)", d);
    d = t;                                      // grad_v alone: v is not given
    d.grad_v = gv2; d.ld_grad_v = F;
    run("cols (grad_v alone)", d);

    save(dir + "/out.bin", out, n_dst * F * esz); save(dir + "/gk.bin", gk, n_dst * F * esz);
    save(dir + "/gq.bin", gq, n_src * ld * esz); save(dir + "/gv.bin", gv, n_src * F * esz);
    save(dir + "/gq_only.bin", gq2, n_src * ld * esz); save(dir + "/gv_only.bin", gv2, n_src * F * esz);
    printf("emu ok\n");
    return 0;
}
