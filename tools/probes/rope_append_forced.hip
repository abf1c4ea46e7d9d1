// The rope_append translation unit alone, built twice by tools/rope_append_table.py with the BLOCK / WAVE threshold forced to its extremes
// (-DROPE_APPEND_BLOCK_MAX=2147483647: every token count runs BLOCK; =0: every count runs WAVE), so that both forms can be timed on the
// same shapes and the value of SM_ROPE_APPEND_BLOCK_MAX_TOKENS chosen from a measurement.  Not part of libsparsifyme.so.
#include "../../sparsify.me_amd/csrc/rope_append.hip"

namespace sm {
void set_error(const char*, ...) {}
}  // namespace sm
