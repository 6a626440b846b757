// TEST TOOLING ONLY: a device sweep of csrc/mds_math.hpp's fp32 m_asin beside the device library's asinf on the same arguments.
// Compiled by tests/test_gpu_rpy_short_arms.py with hipcc (the flags of the product build); never loaded by the package.
#include <hip/hip_runtime.h>

#include "../../multidronesim_amd/csrc/mds_math.hpp"

__global__ void k_asin_sweep(const float* x, float* mine, float* ref, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    mine[i] = mds::m_asin(x[i]);
    ref[i] = asinf(x[i]);
  }
}

// x, mine, ref: host arrays of n floats.  Returns 0, or the HIP error code of the first call that failed.
extern "C" int asin_sweep(const float* x, float* mine, float* ref, int n) {
  float *dx = nullptr, *dm = nullptr, *dr = nullptr;
  const size_t bytes = (size_t)n * sizeof(float);
  hipError_t e = hipMalloc(&dx, bytes);
  if (e == hipSuccess) e = hipMalloc(&dm, bytes);
  if (e == hipSuccess) e = hipMalloc(&dr, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_asin_sweep<<<dim3((n + 255) / 256), dim3(256)>>>(dx, dm, dr, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(mine, dm, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ref, dr, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(dx);
  (void)hipFree(dm);
  (void)hipFree(dr);
  return (int)e;
}
