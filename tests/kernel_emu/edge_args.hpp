// Host stand-in for csrc/edge_args.hpp: the two helpers the attention kernels take from it.
#pragma once
#include "common.hpp"
namespace dgll {
inline float lrelu(float z, float alpha) { return z > 0.0f ? z : alpha * z; }
inline float head_sum(float v, int lph) { for (int off = 1; off < lph; off <<= 1) v += __shfl_xor(v, off); return v; }
}
