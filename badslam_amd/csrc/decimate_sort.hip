// decimate_sort.hip -- the stable (64-bit key, slot) radix sort of bslam_decimate_mesh (decimate_abi.inc) over the key bits in use, for
// gfx950.  A translation unit of its own, like simplify_sort.hip and for its reason: an instantiation of rocPRIM's sort next to the
// project's kernels changes their register allocation, and the device code of the existing calls is to stay as it is.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cstddef>
#include <cstdint>

namespace bslam {

// rocprim::radix_sort_pairs over the key bits [0, end_bit); temp == nullptr: *temp_bytes receives the scratch it needs and nothing runs.
hipError_t decimate_sort_pairs(void* temp, size_t* temp_bytes, const unsigned long long* keys, unsigned long long* sorted_keys, const uint32_t* ids,
                               uint32_t* sorted_ids, size_t count, unsigned end_bit, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, sorted_keys, ids, sorted_ids, count, 0, end_bit, stream);
}

}  // namespace bslam
