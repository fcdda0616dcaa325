// gat_bwd_rows.hip -- second-generation GAT pass 1 (backward over the rows of A); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<1, false, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
