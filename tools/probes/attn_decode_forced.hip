// The attn_decode translation unit alone, built three times by tools/attn_decode_table.py with the chunk forced (-DATTN_DECODE_CHUNK=128,
// 256, 512), so that the three chunk sizes can be timed on the same shapes and the value of SM_ATTN_DECODE_CHUNK chosen from a measurement.
// Not part of libsparsifyme.so.
#include "../../sparsify.me_amd/csrc/attn_decode.hip"

namespace sm {
void set_error(const char*, ...) {}
}  // namespace sm
