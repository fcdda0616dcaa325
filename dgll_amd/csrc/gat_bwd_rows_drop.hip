// gat_bwd_rows_drop.hip -- second-generation GAT pass 1 (backward over the rows of A, exact-dd form) with the attention-dropout mask drawn in the kernel
// (gat2_kernel<..., DROP = true>, gat_dropout.hpp); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<3, false, true>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
