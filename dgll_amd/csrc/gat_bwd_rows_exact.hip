// gat_bwd_rows_exact.hip -- second-generation GAT pass 1 (backward over the rows of A) in its exact-dd form ALONE (KIND 3: dd_i from the
// pass's own dot products, no code of the stored-output form); the kernel template lives in gat_kernel.hpp.
#include "gat_kernel.hpp"

namespace dgll {
template bool gat2_launch<3, false, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
// the same pass with t_j formed from the gathered rows (gat_kernel.hpp, TROW)
template bool gat2_launch<3, true, false>(int, int, int, dim3, hipStream_t, const EdgeArgs&, bool);
}  // namespace dgll
