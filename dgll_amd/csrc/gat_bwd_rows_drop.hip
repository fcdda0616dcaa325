// gat_bwd_rows_drop.hip -- second-generation GAT pass 1 (backward over the rows of A, exact-dd form) with the attention-dropout mask drawn in the kernel
// (gat2_kernel<..., DROP = true>, gat_dropout.hpp); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
bool gat2_launch_3d(int dtype, int lpr, int nh, dim3 grid, hipStream_t s, const EdgeArgs& a) {
    return gat2_launch_kind<3, false, true>(dtype, lpr, nh, grid, s, a, false);
}
}  // namespace dgll
