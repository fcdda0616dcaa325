// gat_fwd.hip -- second-generation GAT pass 0 (forward); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<0, false, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
