// The definitions behind the stand-in common.hpp, once for the three emulators (included by each *_main.cpp after its kernel source):
// the fiber scheduler that runs a workgroup in lock step, and guarded buffers for the arrays the passes read and write.
#pragma once
#include "common.hpp"
#include <sys/mman.h>
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
// buffer that ends exactly at a PROT_NONE page (16-byte aligned when bytes % 16 == 0): a read or write past its end faults.  It starts
// as 0xCD bytes, so an element of an output that the kernel does not write shows.
static void* guarded(size_t bytes) {
    size_t pg = 4096, body = (bytes + pg - 1) / pg * pg;
    char* base = (char*)mmap(nullptr, body + 2 * pg, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    mprotect(base, pg, PROT_NONE); mprotect(base + pg + body, pg, PROT_NONE);
    memset(base + pg, 0xCD, body);
    return base + pg + (body - bytes);
}
// a file of exactly `want` bytes into a guarded buffer
static void* load(const std::string& path, size_t want) {
    FILE* f = fopen(path.c_str(), "rb"); if (!f) { perror(path.c_str()); exit(1); }
    fseek(f, 0, SEEK_END); size_t bytes = ftell(f); fseek(f, 0, SEEK_SET);
    if (bytes != want) { fprintf(stderr, "%s: %zu bytes, expected %zu\n", path.c_str(), bytes, want); exit(1); }
    void* p = guarded(bytes ? bytes : 16); if (bytes && fread(p, 1, bytes, f) != bytes) exit(1); fclose(f); return p;
}
static void save(const std::string& path, const void* p, size_t bytes) { FILE* f = fopen(path.c_str(), "wb"); fwrite(p, 1, bytes, f); fclose(f); }
