// Runs the three passes of dgll_hip_soft_agg_pass (the unmodified soft_agg.hip, included below) on arrays read from DIR and writes the
// results back:  emu DIR n_dst n_src F dtype ld mode has_e semi eps
// Inputs: rowptr / col (A), trowptr / tcol / perm (A^T and its entry -> A's entry), theta (one fp32), x [n_src, ld] in the storage dtype
// (ld >= F: x and grad_x sit on that pitch), e [nnz, F] (has_e), go [n_dst, F].
// Outputs: out [n_dst, F], stats fp32 [n_dst, 2 F], gx [n_src, ld] (the columns past F keep the fill), ge [nnz, F] (has_e), gth and gth3
// (one fp32 each: the scalar gradient over DGLL_SOFT_AGG_MAX_PARTIALS and over 3 workgroups per column block; not with semi), and
// ge_only [nnz, F] from a rows pass that writes grad_e alone.  Every builtin soft_agg.hip uses has its stand-in in common.hpp.
#include "soft_agg.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_soft_agg_desc& d) {
    if (dgll_hip_soft_agg_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 11) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]); size_t ld = atoll(argv[6]);
    int mode = atoi(argv[7]), has_e = atoi(argv[8]), semi = atoi(argv[9]); float eps = (float)atof(argv[10]);
    size_t esz = dtype == 0 ? 4 : 2;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    const float* theta = (const float*)load(dir + "/theta.bin", 4);
    void* x = load(dir + "/x.bin", n_src * ld * esz); void* go = load(dir + "/go.bin", n_dst * F * esz);
    void* e = has_e ? load(dir + "/e.bin", nnz * F * esz) : nullptr;
    void* out = guarded(n_dst * F * esz); float* stats = (float*)guarded(n_dst * 2 * F * 4);
    void* gx = guarded(n_src * ld * esz); void* ge = guarded(nnz * F * esz); void* ge2 = guarded(nnz * F * esz);
    size_t blocks = (F * esz / 16 + 63) / 64;
    float* parts = (float*)guarded(DGLL_SOFT_AGG_MAX_PARTIALS * blocks * 4); float* gth = (float*)guarded(16); float* gth3 = (float*)guarded(16);
    dgll_soft_agg_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.mode = mode; base.semi_grad = semi; base.F = F; base.eps = eps; base.theta = theta; base.nnz = nnz;
    base.x = x; base.ld_x = ld; base.e = e; base.ld_e = F; base.stats = stats; base.ld_stats = 2 * F;

    dgll_soft_agg_desc d = base;
    d.pass = DGLL_SOFT_AGG_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src; d.out = out; d.ld_out = F;
    run("forward", d);

    dgll_soft_agg_desc r = base;
    r.pass = DGLL_SOFT_AGG_ROWS; r.rowptr = rowptr; r.col = col; r.n_rows = n_dst; r.n_cols = n_src; r.grad_out = go; r.ld_grad_out = F;
    d = r;
    if (has_e) { d.grad_e = ge; d.ld_grad_e = F; }
    if (!semi) { d.partials = parts; d.n_partials = DGLL_SOFT_AGG_MAX_PARTIALS; d.grad_theta = gth; }
    if (has_e || !semi) run("rows", d);
    if (!semi) {                                // a bounded grid: three workgroups take the tiles grid-stride
        d = r; d.partials = parts; d.n_partials = 3; d.grad_theta = gth3;
        run("rows (three partials)", d);
    }
    if (has_e) {
        d = r; d.grad_e = ge2; d.ld_grad_e = F;
        run("rows (grad_e alone)", d);
    }

    d = base;
    d.pass = DGLL_SOFT_AGG_COLS; d.rowptr = trowptr; d.col = tcol; d.perm = has_e ? perm : nullptr; d.n_rows = n_src; d.n_cols = n_dst;
    d.grad_out = go; d.ld_grad_out = F; d.grad_x = gx; d.ld_grad_x = ld;
    run("cols", d);

    save(dir + "/out.bin", out, n_dst * F * esz); save(dir + "/stats.bin", stats, n_dst * 2 * F * 4);
    save(dir + "/gx.bin", gx, n_src * ld * esz);
    if (has_e) { save(dir + "/ge.bin", ge, nnz * F * esz); save(dir + "/ge_only.bin", ge2, nnz * F * esz); }
    if (!semi) { save(dir + "/gth.bin", gth, 4); save(dir + "/gth3.bin", gth3, 4); }
    printf("emu ok\n");
    return 0;
}
