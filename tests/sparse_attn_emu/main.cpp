// Runs the three passes of dgll_hip_sparse_attn_pass (the unmodified sparse_attn.hip, included below) on arrays read from DIR and
// writes the results back:  sparse_attn_emu DIR n_dst n_src heads D dtype scale kv_shared.  Inputs: rowptr / col (A), trowptr / tcol
// (A^T), q, k, v, g in the storage dtype (kv_shared: v is not read, k serves both).  The host stand-ins for the kernel's two headers are
// those of tests/gatv2_emu (copied next to this file by the test).  Every buffer ends at a PROT_NONE page, so an access past its end
// faults.
#include "sparse_attn.hip"
#include <sys/mman.h>
#include <vector>
namespace emu {
Fiber fib[256]; ucontext_t sched; int cur; dim3 bidx, gdim; uint64_t buf[256];
int wave_arrived[4], wave_gen[4], blk_arrived, blk_gen; std::function<void()> body;
void die(const char* m) { fprintf(stderr, "EMU FAIL: %s (block %u,%u thread %d)\n", m, bidx.x, bidx.y, cur); exit(2); }
static void entry() { body(); fib[cur].done = true; swapcontext(&fib[cur].ctx, &sched); }
void launch(dim3 grid, dim3 block, std::function<void()> fn) {
    if (block.x != 256) die("block size");
    body = fn; gdim = grid;
    for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
        bidx = dim3(bx, by);
        for (int w = 0; w < 4; ++w) wave_arrived[w] = 0;
        blk_arrived = 0;
        for (int i = 0; i < 256; ++i) {
            if (!fib[i].stack) fib[i].stack = (char*)malloc(1 << 17);
            getcontext(&fib[i].ctx); fib[i].ctx.uc_stack.ss_sp = fib[i].stack; fib[i].ctx.uc_stack.ss_size = 1 << 17; fib[i].ctx.uc_link = &sched;
            makecontext(&fib[i].ctx, entry, 0); fib[i].done = false;
        }
        for (bool any = true; any;) { any = false; for (int i = 0; i < 256; ++i) if (!fib[i].done) { any = true; cur = i; swapcontext(&sched, &fib[i].ctx); } }
        for (int w = 0; w < 4; ++w) if (wave_arrived[w]) die("lanes left waiting in a wave collective");
        if (blk_arrived) die("threads left waiting in __syncthreads");
    }
}
}
namespace dgll { std::string last_error; }
// buffer that ends at a PROT_NONE page: a read or write past its end faults
static void* guarded(size_t bytes) {
    size_t pg = 4096, body = (bytes + pg - 1) / pg * pg;
    char* base = (char*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    mprotect(base, pg, PROT_NONE); mprotect(base + pg + body, pg, PROT_NONE);
    memset(base + pg, 0xCD, body);
    return base + pg + (body - bytes);      // ends exactly at the guard page (16-byte aligned when bytes % 16 == 0)
}
static void* load(const std::string& path, size_t& bytes) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) { perror(path.c_str()); exit(1); }
    fseek(f, 0, SEEK_END); bytes = ftell(f); fseek(f, 0, SEEK_SET);
    void* p = guarded(bytes ? bytes : 16); if (bytes && fread(p, 1, bytes, f) != bytes) exit(1); fclose(f); return p;
}
static void save(const std::string& path, const void* p, size_t bytes) { FILE* f = fopen(path.c_str(), "wb"); fwrite(p, 1, bytes, f); fclose(f); }
int main(int argc, char** argv) {
    if (argc < 9) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]); int heads = atoi(argv[4]), D = atoi(argv[5]), dtype = atoi(argv[6]);
    float scale = atof(argv[7]); int shared = atoi(argv[8]);
    size_t esz = dtype == 0 ? 4 : 2, F = (size_t)heads * D, nb;
    dgll_attn_desc d; memset(&d, 0, sizeof d);
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", nb); const int32_t* col = (const int32_t*)load(dir + "/col.bin", nb);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", nb); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nb);
    void* q = load(dir + "/q.bin", nb); if (nb != n_dst * F * esz) { fprintf(stderr, "q size\n"); return 1; }
    void* k = load(dir + "/k.bin", nb); if (nb != n_src * F * esz) { fprintf(stderr, "k size\n"); return 1; }
    void* v = k;
    if (!shared) { v = load(dir + "/v.bin", nb); if (nb != n_src * F * esz) { fprintf(stderr, "v size\n"); return 1; } }
    void* g = load(dir + "/g.bin", nb); if (nb != n_dst * F * esz) { fprintf(stderr, "g size\n"); return 1; }
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
