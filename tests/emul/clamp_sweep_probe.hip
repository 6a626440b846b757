// TEST TOOLING ONLY: a device sweep of csrc/mds_math.hpp's fp32 m_clamp beside the two selects it stood for, on the same arguments
// and bounds.  Compiled by tests/test_gpu_step_clamps.py with hipcc (the flags of the product build); never loaded by the package.
#include <hip/hip_runtime.h>

#include "../../multidronesim_amd/csrc/mds_math.hpp"

// the bounds are kernel arguments, as the constants of a launch are: the compiler knows nothing about their values
__global__ void k_clamp_sweep(const float* x, float* mine, float* ref, int n, float lo, float hi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    mine[i] = mds::m_clamp(x[i], lo, hi);
    ref[i] = mds::m_min(mds::m_max(x[i], lo), hi);
  }
}

// x, mine, ref: host arrays of n floats.  Returns 0, or the HIP error code of the first call that failed.
extern "C" int clamp_sweep(const float* x, float* mine, float* ref, int n, float lo, float hi) {
  float *dx = nullptr, *dm = nullptr, *dr = nullptr;
  const size_t bytes = (size_t)n * sizeof(float);
  hipError_t e = hipMalloc(&dx, bytes);
  if (e == hipSuccess) e = hipMalloc(&dm, bytes);
  if (e == hipSuccess) e = hipMalloc(&dr, bytes);
  if (e == hipSuccess) e = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_clamp_sweep<<<dim3((n + 255) / 256), dim3(256)>>>(dx, dm, dr, n, lo, hi);
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
