// gat_bwd_cols.hip -- second-generation GAT pass 2 (backward over the rows of A^T); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<2, false, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
