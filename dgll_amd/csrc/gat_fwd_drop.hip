// gat_fwd_drop.hip -- second-generation GAT pass 0 (forward) with the attention-dropout mask drawn in the kernel
// (gat2_kernel<..., DROP = true>, gat_dropout.hpp); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<0, false, true>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
