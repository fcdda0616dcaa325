// Runs the three passes of dgll_hip_typed_spmm_pass (the unmodified typed_spmm.hip, included below) on arrays read from DIR and
// writes the results back:  typed_spmm_emu DIR n_dst n_src F B R dtype has_norm.  Inputs: rowptr / col / etype / norm (A), trowptr /
// tcol / tetype / tnorm (A^T, its own entry order), coeff fp32 [R, B], x [n_src, F] and dz [n_dst, B * F] in the storage dtype.
// Outputs: z [n_dst, B * F], dx [n_src, F], p fp32 [nnz, B rounded up to 4].  The host stand-ins for the kernel's two headers are
// those of tests/gatv2_emu (copied next to this file by the test).  Every buffer ends at a PROT_NONE page, so an access past its end
// faults; the outputs start as 0xCD bytes, so an element the kernel does not write shows.
#include "typed_spmm.hip"
#include <sys/mman.h>
#include <vector>
namespace emu {
Fiber fib[256]; ucontext_t sched; int cur; dim3 bidx, gdim; uint64_t buf[256];
int wave_arrived[4], wave_gen[4], blk_arrived, blk_gen; std::function<void()> body;
void die(const char* m) { fprintf(stderr, "EMU FAIL: %s (block %u,%u,%u thread %d)\n", m, bidx.x, bidx.y, bidx.z, cur); exit(2); }
static void entry() { body(); fib[cur].done = true; swapcontext(&fib[cur].ctx, &sched); }
void launch(dim3 grid, dim3 block, std::function<void()> fn) {
    if (block.x != 256) die("block size");
    body = fn; gdim = grid;
    for (unsigned bz = 0; bz < grid.z; ++bz) for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
        bidx = dim3(bx, by, bz);
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
static void* load(const std::string& path, size_t want) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) { perror(path.c_str()); exit(1); }
    fseek(f, 0, SEEK_END); size_t bytes = ftell(f); fseek(f, 0, SEEK_SET);
    if (bytes != want) { fprintf(stderr, "%s: %zu bytes, expected %zu\n", path.c_str(), bytes, want); exit(1); }
    void* p = guarded(bytes ? bytes : 16); if (bytes && fread(p, 1, bytes, f) != bytes) exit(1); fclose(f); return p;
}
static void save(const std::string& path, const void* p, size_t bytes) { FILE* f = fopen(path.c_str(), "wb"); fwrite(p, 1, bytes, f); fclose(f); }
int main(int argc, char** argv) {
    if (argc < 9) return 1;
    std::string dir = argv[1];
    int64_t n_dst = atoll(argv[2]), n_src = atoll(argv[3]), F = atoll(argv[4]); int B = atoi(argv[5]), R = atoi(argv[6]), dtype = atoi(argv[7]);
    int has_norm = atoi(argv[8]);
    size_t esz = dtype == 0 ? 4 : 2, ldp = (size_t)(B + 3) / 4 * 4;
    const int64_t* rowptr = (const int64_t*)load(dir + "/rowptr.bin", (n_dst + 1) * 8);
    const int64_t* trowptr = (const int64_t*)load(dir + "/trowptr.bin", (n_src + 1) * 8);
    size_t nnz = rowptr[n_dst];
    const int32_t* col = (const int32_t*)load(dir + "/col.bin", nnz * 4); const int32_t* tcol = (const int32_t*)load(dir + "/tcol.bin", nnz * 4);
    const int32_t* etype = (const int32_t*)load(dir + "/etype.bin", nnz * 4); const int32_t* tetype = (const int32_t*)load(dir + "/tetype.bin", nnz * 4);
    const float* norm = has_norm ? (const float*)load(dir + "/norm.bin", nnz * 4) : nullptr;
    const float* tnorm = has_norm ? (const float*)load(dir + "/tnorm.bin", nnz * 4) : nullptr;
    const float* coeff = (const float*)load(dir + "/coeff.bin", (size_t)R * B * 4);
    void* x = load(dir + "/x.bin", n_src * F * esz); void* dz = load(dir + "/dz.bin", n_dst * B * F * esz);
    void* z = guarded(n_dst * B * F * esz); void* dx = guarded(n_src * F * esz); float* p = (float*)guarded(nnz * ldp * 4);
    dgll_typed_desc d; memset(&d, 0, sizeof d);
    d.dtype = dtype; d.R = R; d.B = B; d.F = F; d.coeff = coeff; d.x = x; d.ld_x = F; d.dz = dz; d.ld_dz = B * F;
    d.pass = DGLL_TYPED_EXPAND; d.rowptr = rowptr; d.col = col; d.etype = etype; d.norm = norm; d.n_rows = n_dst; d.n_cols = n_src;
    d.out = z; d.ld_out = B * F;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "expand: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_TYPED_EDGE_DOTS; d.out = nullptr; d.ld_out = 0; d.p = p; d.ld_p = ldp; d.etype = nullptr; d.norm = nullptr; d.coeff = nullptr;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "dots: %s\n", dgll::last_error.c_str()); return 1; }
    d.pass = DGLL_TYPED_CONTRACT; d.rowptr = trowptr; d.col = tcol; d.etype = tetype; d.norm = tnorm; d.coeff = coeff; d.n_rows = n_src; d.n_cols = n_dst;
    d.out = dx; d.ld_out = F; d.p = nullptr; d.ld_p = 0; d.x = nullptr; d.ld_x = 0;
    if (dgll_hip_typed_spmm_pass(nullptr, &d)) { fprintf(stderr, "contract: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/z.bin", z, n_dst * B * F * esz); save(dir + "/dx.bin", dx, n_src * F * esz); save(dir + "/p.bin", p, nnz * ldp * 4);
    printf("emu ok\n");
    return 0;
}
