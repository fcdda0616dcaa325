// gat_fwd_rowscore.hip -- second-generation GAT pass 0 (forward) in its row-score form: t_j = h_j . a2 formed from the gathered row
// (gat_kernel.hpp, TROW); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<0, true, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
