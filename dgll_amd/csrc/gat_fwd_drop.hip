// gat_fwd_drop.hip -- second-generation GAT pass 0 (forward) with the attention-dropout mask drawn in the kernel
// (gat2_kernel<..., DROP = true>, gat_dropout.hpp); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
bool gat2_launch_0d(int dtype, int lpr, int nh, dim3 grid, hipStream_t s, const EdgeArgs& a) {
    return gat2_launch_kind<0, false, true>(dtype, lpr, nh, grid, s, a, false);
}
}  // namespace dgll
