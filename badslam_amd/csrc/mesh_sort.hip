// mesh_sort.hip -- the stable (64-bit key, 32-bit id) radix sort of the mesh operators (mesh_sort in mesh_abi.inc: bslam_simplify_mesh,
// bslam_decimate_mesh, bslam_smooth_mesh) over the key bits in use, for gfx950.  A translation unit of its own: instantiated in
// badslam_hip.hip, next to the 32-bit sort of the surfel order, rocPRIM's 64-bit sort changes the register allocation of that sort's
// block kernel and of the project's kernels, and their device code is to stay as it is.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <cstddef>
#include <cstdint>

namespace bslam {

// rocprim::radix_sort_pairs over the key bits [0, end_bit); temp == nullptr: *temp_bytes receives the scratch it needs and nothing runs.
hipError_t mesh_sort_pairs(void* temp, size_t* temp_bytes, const unsigned long long* keys, unsigned long long* sorted_keys, const uint32_t* ids,
                           uint32_t* sorted_ids, size_t count, unsigned end_bit, hipStream_t stream) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, sorted_keys, ids, sorted_ids, count, 0, end_bit, stream);
}

}  // namespace bslam
