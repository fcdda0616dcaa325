// Runs the three passes of dgll_hip_multi_agg_pass (the unmodified multi_agg.hip, included below) on arrays read from DIR and writes the
// results back:  emu DIR n_dst n_src F dtype with_y aggs scalers delta  -- aggs / scalers: the ordered code lists as digit strings
// ("012345", "012").  Inputs: rowptr / col (A), trowptr / tcol (A^T), x [n_src, F], y [n_dst, F] and go [n_dst, S * A * F] in the
// storage dtype.  Outputs: out, stats, arg (forward); coef, gy (rows); gx (cols over A^T); then rows and cols once more per block k of
// go with every other block zeroed: gy_k, gx_k (a gradient bar per block needs them: the backward is linear in go).
#include "multi_agg.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_multi_agg_desc& d) {
    if (dgll_hip_multi_agg_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 10) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]), with_y = atoi(argv[6]);
    std::string aggs = argv[7], scalers = argv[8];
    size_t esz = dtype == 0 ? 4 : 2, wide = aggs.size() * scalers.size() * F;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    void* x = load(dir + "/x.bin", n_src * F * esz); void* y = load(dir + "/y.bin", n_dst * F * esz); void* go = load(dir + "/go.bin", n_dst * wide * esz);
    dgll_multi_agg_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.F = F; base.delta = (float)atof(argv[9]);
    base.n_agg = (int)aggs.size(); base.n_scaler = (int)scalers.size();
    for (size_t i = 0; i < aggs.size() && i < 6; ++i) base.agg[i] = aggs[i] - '0';
    for (size_t i = 0; i < scalers.size() && i < 3; ++i) base.scaler[i] = scalers[i] - '0';

    void* out = guarded(n_dst * wide * esz); float* stats = (float*)guarded(n_dst * 2 * F * 4); int32_t* arg = (int32_t*)guarded(n_dst * 2 * F * 4);
    float* coef = (float*)guarded(n_dst * 5 * F * 4); void* gy = guarded(n_dst * F * esz); void* gx = guarded(n_src * F * esz);
    dgll_multi_agg_desc d = base;
    d.pass = DGLL_MAGG_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
    d.x = x; d.ld_x = F; if (with_y) { d.y = y; d.ld_y = F; } d.out = out; d.ld_out = wide; d.stats = stats; d.ld_stats = 2 * F; d.arg = arg; d.ld_arg = 2 * F;
    run("forward", d);
    d = base;
    d.pass = DGLL_MAGG_ROWS; d.rowptr = rowptr; d.n_rows = n_dst; d.n_cols = n_src;
    d.grad_out = go; d.ld_grad_out = wide; d.stats = stats; d.ld_stats = 2 * F; d.coef = coef; d.ld_coef = 5 * F; d.grad_y = gy; d.ld_grad_y = F;
    run("rows", d);
    d = base;
    d.pass = DGLL_MAGG_COLS; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst;
    d.x = x; d.ld_x = F; d.coef = coef; d.ld_coef = 5 * F; d.arg = arg; d.ld_arg = 2 * F; d.grad_x = gx; d.ld_grad_x = F;
    run("cols", d);
    save(dir + "/out.bin", out, n_dst * wide * esz); save(dir + "/stats.bin", stats, n_dst * 2 * F * 4); save(dir + "/arg.bin", arg, n_dst * 2 * F * 4);
    save(dir + "/coef.bin", coef, n_dst * 5 * F * 4); save(dir + "/gy.bin", gy, n_dst * F * esz); save(dir + "/gx.bin", gx, n_src * F * esz);
    char* masked = (char*)guarded(n_dst * wide * esz);
    for (size_t k = 0; k < aggs.size() * scalers.size(); ++k) {
        memset(masked, 0, n_dst * wide * esz);
        for (int64_t i = 0; i < n_dst; ++i) memcpy(masked + (i * wide + k * F) * esz, (const char*)go + (i * wide + k * F) * esz, F * esz);
        d = base;
        d.pass = DGLL_MAGG_ROWS; d.rowptr = rowptr; d.n_rows = n_dst; d.n_cols = n_src;
        d.grad_out = masked; d.ld_grad_out = wide; d.stats = stats; d.ld_stats = 2 * F; d.coef = coef; d.ld_coef = 5 * F; d.grad_y = gy; d.ld_grad_y = F;
        run("rows", d);
        d = base;
        d.pass = DGLL_MAGG_COLS; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst;
        d.x = x; d.ld_x = F; d.coef = coef; d.ld_coef = 5 * F; d.arg = arg; d.ld_arg = 2 * F; d.grad_x = gx; d.ld_grad_x = F;
        run("cols", d);
        save(dir + "/gy_" + std::to_string(k) + ".bin", gy, n_dst * F * esz); save(dir + "/gx_" + std::to_string(k) + ".bin", gx, n_src * F * esz);
    }
    printf("emu ok\n");
    return 0;
}
