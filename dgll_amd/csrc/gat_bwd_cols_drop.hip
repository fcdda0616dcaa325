// gat_bwd_cols_drop.hip -- second-generation GAT pass 2 (backward over the rows of A^T) with the attention-dropout mask drawn in the kernel
// (gat2_kernel<..., DROP = true>, gat_dropout.hpp); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
bool gat2_launch_2d(int dtype, int lpr, int nh, dim3 grid, hipStream_t s, const EdgeArgs& a) {
    return gat2_launch_kind<2, false, true>(dtype, lpr, nh, grid, s, a, false);
}
}  // namespace dgll
