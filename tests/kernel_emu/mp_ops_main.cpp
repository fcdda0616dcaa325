// Runs the six passes of dgll_hip_mp_pass (the unmodified mp_ops.hip, included below) on arrays read from DIR and writes the results
// back:  emu DIR n_dst n_src heads D dtype.  Inputs: rowptr / col (A), trowptr / tcol / perm (A^T), per-edge fp32 [nnz, heads] e
// (logits), w (weights), g (a gradient), per-row fp32 a [n_src, heads], b [n_dst, heads]; for D > 0 the node matrices x [n_src, F],
// y and gy [n_dst, F] in the storage dtype (D == 0: the per-edge passes alone).  Passes over A^T take perm, as the backwards of
// dgll_amd/ops_mp.py do.
#include "mp_ops.hip"
#include "emu_runtime.hpp"
static int run(const char* what, const dgll_mp_desc& d) {
    if (dgll_hip_mp_pass(nullptr, &d)) { fprintf(stderr, "%s: %s\n", what, dgll::last_error.c_str()); exit(1); }
    return 0;
}
int main(int argc, char** argv) {
    if (argc < 7) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); int heads = atoi(argv[4]), D = atoi(argv[5]), dtype = atoi(argv[6]);
    size_t esz = dtype == 0 ? 4 : 2, F = (size_t)heads * D, H = heads;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int64_t* perm = (const int64_t*)load(dir + "/perm.bin", nnz * 8);
    const float* e = (const float*)load(dir + "/e.bin", nnz * H * 4); const float* w = (const float*)load(dir + "/w.bin", nnz * H * 4);
    const float* g = (const float*)load(dir + "/g.bin", nnz * H * 4);
    const float* a = (const float*)load(dir + "/a.bin", n_src * H * 4); const float* b = (const float*)load(dir + "/b.bin", n_dst * H * 4);
    dgll_mp_desc base; memset(&base, 0, sizeof base);
    base.dtype = DGLL_F32; base.heads = heads; base.D = D; base.nnz = nnz;
    dgll_mp_desc A = base, T = base;
    A.rowptr = rowptr; A.col = col; A.n_rows = n_dst; A.n_cols = n_src;
    T.rowptr = trowptr; T.col = tcol; T.perm = perm; T.n_rows = n_src; T.n_cols = n_dst;

    // edge softmax and its backward, by destination (A) and by source (A^T with perm)
    const char* sm_name[2] = {"/sm.bin", "/smt.bin"}; const char* smb_name[2] = {"/smb.bin", "/smtb.bin"};
    for (int t = 0; t < 2; ++t) {
        dgll_mp_desc d = t ? T : A;
        float* sm = (float*)guarded(nnz * H * 4); float* smb = (float*)guarded(nnz * H * 4);
        d.pass = DGLL_MP_EDGE_SOFTMAX; d.e = e; d.ld_e = H; d.e_out = sm; d.ld_e_out = H; run("softmax", d);
        d.pass = DGLL_MP_EDGE_SOFTMAX_BWD; d.e = sm; d.e2 = g; d.ld_e2 = H; d.e_out = smb; run("softmax bwd", d);
        save(dir + sm_name[t], sm, nnz * H * 4); save(dir + smb_name[t], smb, nnz * H * 4);
    }
    {   // E_SUM over A and over A^T
        float* es = (float*)guarded(n_dst * H * 4); float* est = (float*)guarded(n_src * H * 4);
        dgll_mp_desc d = A; d.pass = DGLL_MP_E_SUM; d.e = w; d.ld_e = H; d.out = es; d.ld_out = H; run("e_sum", d);
        d = T; d.pass = DGLL_MP_E_SUM; d.e = w; d.ld_e = H; d.out = est; d.ld_out = H; run("e_sum^T", d);
        save(dir + "/es.bin", es, n_dst * H * 4); save(dir + "/est.bin", est, n_src * H * 4);
    }
    {   // U_ADD_V: both sides over A; over A^T with perm the row side alone (copy_e_sum's backward by source)
        float* uav = (float*)guarded(nnz * H * 4); float* uavt = (float*)guarded(nnz * H * 4);
        dgll_mp_desc d = A; d.pass = DGLL_MP_U_ADD_V; d.x = a; d.ld_x = H; d.y = b; d.ld_y = H; d.e_out = uav; d.ld_e_out = H; run("u_add_v", d);
        d = T; d.pass = DGLL_MP_U_ADD_V; d.y = a; d.ld_y = H; d.e_out = uavt; d.ld_e_out = H; run("u_add_v^T", d);
        save(dir + "/uav.bin", uav, nnz * H * 4); save(dir + "/uavt.bin", uavt, nnz * H * 4);
    }
    if (D > 0) {
        void* x = load(dir + "/x.bin", n_src * F * esz); void* y = load(dir + "/y.bin", n_dst * F * esz); void* gy = load(dir + "/gy.bin", n_dst * F * esz);
        void* mul = guarded(n_dst * F * esz); void* mult = guarded(n_src * F * esz); float* dot = (float*)guarded(nnz * H * 4);
        dgll_mp_desc d = A; d.dtype = dtype; d.pass = DGLL_MP_U_MUL_E_SUM; d.e = w; d.ld_e = H; d.x = x; d.ld_x = F; d.out = mul; d.ld_out = F;
        run("u_mul_e_sum", d);
        d = T; d.dtype = dtype; d.pass = DGLL_MP_U_MUL_E_SUM; d.e = w; d.ld_e = H; d.x = gy; d.ld_x = F; d.out = mult; d.ld_out = F;
        run("u_mul_e_sum^T", d);
        d = A; d.dtype = dtype; d.pass = DGLL_MP_U_DOT_V; d.x = x; d.ld_x = F; d.y = y; d.ld_y = F; d.e_out = dot; d.ld_e_out = H;
        run("u_dot_v", d);
        save(dir + "/mul.bin", mul, n_dst * F * esz); save(dir + "/mult.bin", mult, n_src * F * esz); save(dir + "/dot.bin", dot, nnz * H * 4);
    }
    printf("emu ok\n");
    return 0;
}
