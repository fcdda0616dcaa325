// Runs dgll_hip_fps (the unmodified fps.hip) on arrays read from DIR:  emu DIR n D dtype ld n_segs max_seg n_out
// In: x [n, ld], seg / outptr int64 [n_segs + 1], start int64 [n_segs].  Out: idx int64 and dmin fp32 [n_out].  Outputs
// start as 0xCD bytes and end at a guard page.
#include "fps.hip"
#include "emu_runtime.hpp"
int main(int argc, char** argv) {
    std::string dir = argc == 9 ? argv[1] : (exit(1), "");
    int64_t n = atoll(argv[2]), D = atoll(argv[3]); int dtype = atoi(argv[4]);
    int64_t ld = atoll(argv[5]), S = atoll(argv[6]), max_seg = atoll(argv[7]), n_out = atoll(argv[8]);
    const void* x = load(dir + "/x.bin", n * ld * (dtype == 0 ? 4 : 2));
    const int64_t* seg = (const int64_t*)load(dir + "/seg.bin", (S + 1) * 8);
    const int64_t* outptr = (const int64_t*)load(dir + "/outptr.bin", (S + 1) * 8);
    const int64_t* start = (const int64_t*)load(dir + "/start.bin", S * 8);
    int64_t* idx = (int64_t*)guarded(n_out * 8);
    float* dmin = (float*)guarded(n_out * 4); float* scratch = (float*)guarded(n * 4);
    if (dgll_hip_fps(nullptr, x, ld, dtype, n, D, seg, S, max_seg, outptr, start, idx, dmin, n_out, scratch)) { fprintf(stderr, "fps: %s\n", dgll::last_error.c_str()); return 1; }
    save(dir + "/idx.bin", idx, n_out * 8); save(dir + "/dmin.bin", dmin, n_out * 4);
    printf("emu ok\n");
    return 0;
}
