// simplify_sort.hip -- the stable (cell key, vertex id) radix sort of bslam_simplify_mesh (simplify_abi.inc), for gfx950.  A
// translation unit of its own: instantiated in badslam_hip.hip, next to the 32-bit sort of the surfel order, rocPRIM's 64-bit
// sort changes the register allocation of that sort's block kernel, and the device code of the existing calls is to stay as it is.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cstddef>
#include <cstdint>

namespace bslam {

// rocprim::radix_sort_pairs over all 64 key bits; temp == nullptr: *temp_bytes receives the scratch it needs and nothing runs.
hipError_t simplify_sort_pairs(void* temp, size_t* temp_bytes, const unsigned long long* keys, unsigned long long* sorted_keys, const uint32_t* ids,
                               uint32_t* sorted_ids, size_t count, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, sorted_keys, ids, sorted_ids, count, 0, 64, stream);
}

}  // namespace bslam
