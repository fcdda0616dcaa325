// Runs the three passes of dgll_hip_gated_pass (the unmodified gated.hip, included below) on arrays read from DIR and writes the
// results back:  emu DIR n_dst n_src F dtype ld_c with_ge
// Inputs: rowptr / col (A), trowptr / tcol / perm (A^T), a [n_dst, F], b and v [n_src, F], go [n_dst, F], ge [nnz, F] and c [nnz, ld_c]
// in the storage dtype (ld_c >= F: c, ehat and grad_c sit on that pitch).  with_ge = 0: grad_ehat is passed as NULL.
// Outputs: out, ga, w [n_dst, F]; inv, o32 fp32 [n_dst, F]; ehat, gc [nnz, ld_c] (the columns past F keep the fill); gb, gv [n_src, F];
// gv_only [n_src, F] from the rows pass that only leaves w and the cols pass with grad_v alone, gb_only with grad_b alone.
inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
#include "gated.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_gated_desc& d) {
    if (dgll_hip_gated_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 8) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]); size_t ld_c = atoll(argv[6]);
    int with_ge = atoi(argv[7]);
    size_t esz = dtype == 0 ? 4 : 2;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    void* a = load(dir + "/a.bin", n_dst * F * esz); void* b = load(dir + "/b.bin", n_src * F * esz); void* v = load(dir + "/v.bin", n_src * F * esz);
    void* c = load(dir + "/c.bin", nnz * ld_c * esz); void* go = load(dir + "/go.bin", n_dst * F * esz); void* ge = load(dir + "/ge.bin", nnz * F * esz);
    void* out = guarded(n_dst * F * esz); void* ehat = guarded(nnz * ld_c * esz);
    float* inv = (float*)guarded(n_dst * F * 4); float* o32 = (float*)guarded(n_dst * F * 4);
    void* gc = guarded(nnz * ld_c * esz); void* ga = guarded(n_dst * F * esz); void* w = guarded(n_dst * F * esz); void* w2 = guarded(n_dst * F * esz);
    void* gb = guarded(n_src * F * esz); void* gv = guarded(n_src * F * esz); void* gb2 = guarded(n_src * F * esz); void* gv2 = guarded(n_src * F * esz);
    dgll_gated_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.F = F; base.nnz = nnz; base.eps = 1e-6f;

    dgll_gated_desc d = base;
    d.pass = DGLL_GATED_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
    d.a = a; d.ld_a = F; d.b = b; d.ld_b = F; d.c = c; d.ld_c = ld_c; d.v = v; d.ld_v = F;
    d.out = out; d.ld_out = F; d.ehat = ehat; d.ld_ehat = ld_c; d.inv_s = inv; d.ld_inv_s = F; d.out32 = o32; d.ld_out32 = F;
    run("forward", d);

    d = base;
    d.pass = DGLL_GATED_ROWS; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
    d.v = v; d.ld_v = F; d.ehat = ehat; d.ld_ehat = ld_c; d.inv_s = inv; d.ld_inv_s = F; d.out32 = o32; d.ld_out32 = F;
    d.grad_out = go; d.ld_grad_out = F; if (with_ge) { d.grad_ehat = ge; d.ld_grad_ehat = F; }
    d.grad_c = gc; d.ld_grad_c = ld_c; d.grad_a = ga; d.ld_grad_a = F; d.w = w; d.ld_w = F;
    run("rows", d);
    d = base;                                   // only w: no per-edge operand is given
    d.pass = DGLL_GATED_ROWS; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
    d.inv_s = inv; d.ld_inv_s = F; d.out32 = o32; d.ld_out32 = F; d.grad_out = go; d.ld_grad_out = F; d.w = w2; d.ld_w = F;
    run("rows (w only)", d);

    dgll_gated_desc t = base;
    t.pass = DGLL_GATED_COLS; t.rowptr = trowptr; t.col = tcol; t.perm = perm; t.n_rows = n_src; t.n_cols = n_dst;
    d = t;
    d.grad_c = gc; d.ld_grad_c = ld_c; d.ehat = ehat; d.ld_ehat = ld_c; d.w = w; d.ld_w = F; d.grad_b = gb; d.ld_grad_b = F; d.grad_v = gv; d.ld_grad_v = F;
    run("cols", d);
    d = t;
    d.grad_c = gc; d.ld_grad_c = ld_c; d.grad_b = gb2; d.ld_grad_b = F;
    run("cols (grad_b alone)", d);
    d = t;
    d.ehat = ehat; d.ld_ehat = ld_c; d.w = w2; d.ld_w = F; d.grad_v = gv2; d.ld_grad_v = F;
    run("cols (grad_v alone)", d);

    save(dir + "/out.bin", out, n_dst * F * esz); save(dir + "/ehat.bin", ehat, nnz * ld_c * esz);
    save(dir + "/inv.bin", inv, n_dst * F * 4); save(dir + "/o32.bin", o32, n_dst * F * 4);
    save(dir + "/gc.bin", gc, nnz * ld_c * esz); save(dir + "/ga.bin", ga, n_dst * F * esz); save(dir + "/w.bin", w, n_dst * F * esz);
    save(dir + "/gb.bin", gb, n_src * F * esz); save(dir + "/gv.bin", gv, n_src * F * esz);
    save(dir + "/gb_only.bin", gb2, n_src * F * esz); save(dir + "/gv_only.bin", gv2, n_src * F * esz);
    printf("emu ok\n");
    return 0;
}
