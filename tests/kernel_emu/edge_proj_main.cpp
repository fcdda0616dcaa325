// Runs the passes of dgll_hip_edge_proj_pass (the unmodified edge_proj.hip, included below) on arrays read from DIR, for the three ops
// with and without the per-row scale, and writes the results back:  emu DIR n_dst n_src F dtype De ld_x ld_a nulls bias partials
// Inputs: rowptr / col (A), trowptr / tcol / perm (A^T), scale fp32 [n_dst], x [n_src, ld_x], a [nnz, ld_a] and go [n_dst, F] in the
// storage dtype (ld_x >= F: x, out and grad_x sit on that pitch; ld_a >= De: a and grad_a on that one), w fp32 [De, F], b fp32 [F]
// (passed when bias = 1).  nulls = 1: the operands a (pass, op) does not read are passed as NULL; 0: all are.
// Outputs per op o and scale flag m: out_o_m [n_dst, ld_x], gx_o_m [n_src, ld_x] (not for op 0: that pass is edge_feat.hip's),
// slabs_o_m fp32 [partials, De + 1, F], and ga_o_m [nnz, ld_a] -- past one column block gap_o_m fp32 [col_blocks, nnz, De] instead.
// The columns of a pitch past the width keep the fill.
#include "edge_proj.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_edge_proj_desc& d) {
    if (dgll_hip_edge_proj_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 12) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]); int De = atoi(argv[6]);
    size_t ld_x = atoll(argv[7]), ld_a = atoll(argv[8]); int nulls = atoi(argv[9]), bias = atoi(argv[10]); int64_t partials = atoll(argv[11]);
    size_t esz = dtype == 0 ? 4 : 2, epv = 16 / esz, vpr = F / epv, col_blocks = (vpr + 63) / 64;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    const float* scale = (const float*)load(dir + "/scale.bin", n_dst * 4);
    void* x = load(dir + "/x.bin", n_src * ld_x * esz); void* a = load(dir + "/a.bin", nnz * ld_a * esz); void* go = load(dir + "/go.bin", n_dst * F * esz);
    const float* w = (const float*)load(dir + "/w.bin", De * F * 4); const float* b = bias ? (const float*)load(dir + "/b.bin", F * 4) : nullptr;
    dgll_edge_proj_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.F = F; base.nnz = nnz; base.De = De;

    for (int op = 0; op < 3; ++op) for (int m = 0; m < 2; ++m) {
        const bool relu = op == DGLL_EF_ADD_RELU, mul = op == DGLL_EF_MUL;
        std::string tag = "_" + std::to_string(op) + "_" + std::to_string(m) + ".bin";
        void* out = guarded(n_dst * ld_x * esz); void* gx = guarded(n_src * ld_x * esz); void* ga = guarded(nnz * ld_a * esz);
        float* slabs = (float*)guarded(partials * (De + 1) * F * 4); float* part = (float*)guarded(col_blocks * nnz * De * 4);
        dgll_edge_proj_desc d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EFP_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
        d.x = x; d.ld_x = ld_x; d.a = a; d.ld_a = ld_a; d.weight = w; d.bias = b; d.out = out; d.ld_out = ld_x;
        run("forward", d);
        if (op != DGLL_EF_ADD) {
            d = base;
            d.op = op; d.scale = m ? scale : nullptr;
            d.pass = DGLL_EFP_COLS; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst; d.perm = perm;
            d.grad_out = go; d.ld_grad_out = F; d.grad_x = gx; d.ld_grad_x = ld_x; d.a = a; d.ld_a = ld_a; d.weight = w; d.bias = b;
            if (!nulls || relu) { d.x = x; d.ld_x = ld_x; }
            run("cols", d);
            save(dir + "/gx" + tag, gx, n_src * ld_x * esz);
        }
        d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EFP_PARAM; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
        d.grad_out = go; d.ld_grad_out = F; d.a = a; d.ld_a = ld_a; d.slabs = slabs; d.partials = partials;
        if (!nulls || relu || mul) { d.x = x; d.ld_x = ld_x; }
        if (!nulls || relu) { d.weight = w; d.bias = b; }
        run("param", d);
        d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EFP_DOTS; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
        d.grad_out = go; d.ld_grad_out = F; d.weight = w;
        if (col_blocks > 1) d.dots_part = part;
        if (!nulls || col_blocks == 1) { d.grad_a = ga; d.ld_grad_a = ld_a; }
        if (!nulls || relu || mul) { d.x = x; d.ld_x = ld_x; }
        if (!nulls || relu) { d.a = a; d.ld_a = ld_a; d.bias = b; }
        run("dots", d);
        save(dir + "/out" + tag, out, n_dst * ld_x * esz); save(dir + "/slabs" + tag, slabs, partials * (De + 1) * F * 4);
        if (col_blocks > 1) save(dir + "/gap" + tag, part, col_blocks * nnz * De * 4); else save(dir + "/ga" + tag, ga, nnz * ld_a * esz);
    }
    printf("emu ok\n");
    return 0;
}
