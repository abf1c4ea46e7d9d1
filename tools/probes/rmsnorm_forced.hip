// The rmsnorm translation unit alone, built twice by tools/rmsnorm_table.py with the LANES / BLOCK threshold forced to its extremes
// (-DRMSNORM_LANES_MAX=4608: every hidden up to 4608 runs LANES; =8: everything above 8 runs BLOCK), so that both forms can be timed on
// the same shapes and the value of SM_RMSNORM_LANES_MAX_HIDDEN chosen from a measurement.  Not part of libsparsifyme.so.
#include "../../sparsify.me_amd/csrc/rmsnorm.hip"

namespace sm {
void set_error(const char*, ...) {}
}  // namespace sm
