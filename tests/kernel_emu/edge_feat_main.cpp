// Runs the three passes of dgll_hip_edge_feat_pass (the unmodified edge_feat.hip, included below) on arrays read from DIR, for the three
// ops with and without the per-row scale, and writes the results back:  emu DIR n_dst n_src F dtype ld_e nulls
// Inputs: rowptr / col (A), trowptr / tcol / perm (A^T), scale fp32 [n_dst], x [n_src, F], go [n_dst, F] and e [nnz, ld_e] in the storage
// dtype (ld_e >= F: e and grad_e sit on that pitch).  nulls = 1: the operands a (pass, op) does not read are passed as NULL; 0: all are.
// Outputs per op o and scale flag m: out_o_m [n_dst, F], gx_o_m [n_src, F], ge_o_m [nnz, ld_e] (the columns past F keep the fill).
#include "edge_feat.hip"
#include "emu_runtime.hpp"
static void run(const char* what, const dgll_edge_feat_desc& d) {
    if (dgll_hip_edge_feat_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
}
int main(int argc, char** argv) {
    if (argc < 8) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); size_t F = atoll(argv[4]); int dtype = atoi(argv[5]); size_t ld_e = atoll(argv[6]);
    int nulls = atoi(argv[7]);
    size_t esz = dtype == 0 ? 4 : 2;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    const float* scale = (const float*)load(dir + "/scale.bin", n_dst * 4);
    void* x = load(dir + "/x.bin", n_src * F * esz); void* e = load(dir + "/e.bin", nnz * ld_e * esz); void* go = load(dir + "/go.bin", n_dst * F * esz);
    dgll_edge_feat_desc base; memset(&base, 0, sizeof base);
    base.dtype = dtype; base.F = F; base.nnz = nnz;

    for (int op = 0; op < 3; ++op) for (int m = 0; m < 2; ++m) {
        const bool relu = op == DGLL_EF_ADD_RELU, mul = op == DGLL_EF_MUL;
        std::string tag = "_" + std::to_string(op) + "_" + std::to_string(m) + ".bin";
        void* out = guarded(n_dst * F * esz); void* gx = guarded(n_src * F * esz); void* ge = guarded(nnz * ld_e * esz);
        dgll_edge_feat_desc d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EF_FORWARD; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
        d.x = x; d.ld_x = F; d.e = e; d.ld_e = ld_e; d.out = out; d.ld_out = F;
        run("forward", d);
        d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EF_COLS; d.rowptr = trowptr; d.col = tcol; d.n_rows = n_src; d.n_cols = n_dst;
        d.grad_out = go; d.ld_grad_out = F; d.grad_x = gx; d.ld_grad_x = F;
        if (!nulls || relu) { d.x = x; d.ld_x = F; }
        if (!nulls || relu || mul) { d.e = e; d.ld_e = ld_e; d.perm = perm; }
        run("cols", d);
        d = base;
        d.op = op; d.scale = m ? scale : nullptr;
        d.pass = DGLL_EF_EDGE; d.rowptr = rowptr; d.col = col; d.n_rows = n_dst; d.n_cols = n_src;
        d.grad_out = go; d.ld_grad_out = F; d.grad_e = ge; d.ld_grad_e = ld_e;
        if (!nulls || relu || mul) { d.x = x; d.ld_x = F; }
        if (!nulls || relu) { d.e = e; d.ld_e = ld_e; }
        run("edge", d);
        save(dir + "/out" + tag, out, n_dst * F * esz); save(dir + "/gx" + tag, gx, n_src * F * esz); save(dir + "/ge" + tag, ge, nnz * ld_e * esz);
    }
    printf("emu ok\n");
    return 0;
}
