// Host stand-in for csrc/common.hpp: what csrc/row_tiles.hpp and the kernel files on it (gatv2.hip, sparse_attn.hip, typed_spmm.hip)
// need to compile with plain g++ and run in LOCK STEP on the CPU (tests/kernel_emu.py).  A workgroup is 256 fibers (ucontext), one per
// lane, scheduled round-robin; __shfl / __shfl_xor / readfirstlane are wave-level collectives and __syncthreads a workgroup-level one: a
// collective that not every lane reaches, a readfirstlane of a value that differs between lanes, and a 16-byte access to an unaligned
// address end the run with a message.  The kernel source and row_tiles.hpp are compiled UNMODIFIED (copied next to this file so that
// their `#include "common.hpp"` finds this one); the definitions are in emu_runtime.hpp.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <cmath>
#include <algorithm>
#include <functional>
#include <string>
#include <ucontext.h>
#include "dgll_hip.h"
using std::max; using std::min;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define DGLL_API extern "C"
typedef void* hipStream_t;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
namespace emu {
struct Fiber { ucontext_t ctx; char* stack; bool done; };
extern Fiber fib[256]; extern ucontext_t sched; extern int cur; extern dim3 bidx, gdim; extern uint64_t buf[256];
extern int wave_arrived[4], wave_gen[4], blk_arrived, blk_gen; extern std::function<void()> body;
void die(const char* m);
inline void yield() { swapcontext(&fib[cur].ctx, &sched); }
inline void wave_barrier() { int w = cur / 64, g = wave_gen[w]; if (++wave_arrived[w] == 64) { wave_arrived[w] = 0; wave_gen[w]++; } else { long s = 0; while (wave_gen[w] == g) { yield(); if (++s > 200000) die("wave-level collective not reached by all lanes"); } } }
inline void block_barrier() { int g = blk_gen; if (++blk_arrived == 256) { blk_arrived = 0; blk_gen++; } else { long s = 0; while (blk_gen == g) { yield(); if (++s > 200000) die("__syncthreads not reached by all threads"); } } }
template <class T> inline T shfl(T v, int src) { uint64_t b = 0; memcpy(&b, &v, sizeof(T)); buf[cur] = b; wave_barrier(); T r; memcpy(&r, &buf[(cur & ~63) + (src & 63)], sizeof(T)); wave_barrier(); return r; }
void launch(dim3 grid, dim3 block, std::function<void()> fn);
struct Tid { unsigned x; };
}
#define threadIdx (emu::Tid{(unsigned)emu::cur})
#define blockIdx emu::bidx
#define gridDim emu::gdim
template <class T> inline T __shfl(T v, int src) { return emu::shfl(v, src); }
template <class T> inline T __shfl_xor(T v, int off) { return emu::shfl(v, (emu::cur & 63) ^ off); }
inline void __syncthreads() { emu::block_barrier(); }
template <class T> inline T __builtin_amdgcn_readfirstlane(T v) { T f = emu::shfl(v, 0); if (memcmp(&f, &v, sizeof(T))) emu::die("readfirstlane of a non-uniform value"); return f; }
inline float __builtin_amdgcn_exp2f(float x) { return exp2f(x); }
inline float __builtin_amdgcn_logf(float x) { return log2f(x); }
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu::launch(g, b, [=]() { k(__VA_ARGS__); })
inline int hipGetLastError() { return 0; }
#define DGLL_HIP_TRY(e) do { (void)(e); } while (0)
namespace dgll { extern std::string last_error; inline void set_error(const std::string& m) { last_error = m; } }
#define DGLL_REQUIRE(cond, msg) do { if (!(cond)) { ::dgll::set_error(std::string(msg) + " [" #cond "]"); return DGLL_ERR_INVALID; } } while (0)
struct uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
namespace dgll {
constexpr int kWave = 64, kBlock = 256, kWavesPerBlock = 4;
typedef uint16_t bf16_t;
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline float bf16_lo(uint32_t p) { return __uint_as_float(p << 16); }
inline float bf16_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
inline uint32_t rne(float f) { uint32_t u = __float_as_uint(f); return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16; }
inline uint32_t pack_bf16x2(float lo, float hi) { return rne(lo) | (rne(hi) << 16); }
inline int64_t uniform64(int64_t v) { uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32)); return (int64_t)(((uint64_t)hi << 32) | lo); }
template <typename T, int EPV> struct VecIO;
template <> struct VecIO<float, 4> {
    typedef uint4 raw_t;
    static raw_t zero() { return make_uint4(0, 0, 0, 0); }
    static raw_t load(const float* p) { if ((uintptr_t)p & 15) emu::die("unaligned 16-byte load"); raw_t r; memcpy(&r, p, 16); return r; }
    static void unpack(const raw_t& r, float (&f)[4]) { f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w); }
    static void store(float* p, const float (&f)[4]) { if ((uintptr_t)p & 15) emu::die("unaligned 16-byte store"); memcpy(p, f, 16); }
};
template <> struct VecIO<bf16_t, 8> {
    typedef uint4 raw_t;
    static raw_t zero() { return make_uint4(0, 0, 0, 0); }
    static raw_t load(const bf16_t* p) { if ((uintptr_t)p & 15) emu::die("unaligned 16-byte load"); raw_t r; memcpy(&r, p, 16); return r; }
    static void unpack(const raw_t& r, float (&f)[8]) { f[0] = bf16_lo(r.x); f[1] = bf16_hi(r.x); f[2] = bf16_lo(r.y); f[3] = bf16_hi(r.y); f[4] = bf16_lo(r.z); f[5] = bf16_hi(r.z); f[6] = bf16_lo(r.w); f[7] = bf16_hi(r.w); }
    static void store(bf16_t* p, const float (&f)[8]) { if ((uintptr_t)p & 15) emu::die("unaligned 16-byte store"); uint4 r = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])); memcpy(p, &r, 16); }
};
}
