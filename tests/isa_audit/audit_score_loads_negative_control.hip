// Negative control for tests/isa_audit/audit_score_loads.py: a barrier loop whose only global load is written `ok ? p[i] : 0` with
// a per-lane `ok` - the form the scorer's staging and dot-product loads had.  hipcc must not speculate the load, so it lands in an
// exec-mask region of its own and the wait behind it is a full `s_waitcnt vmcnt(0)`; the audit must report both.  Never launched.
#include <hip/hip_runtime.h>
namespace {
template <int A, int B, bool C, bool D, int E, int F>
__global__ void score_kernel(const float* x, float* out, int ntiles, int ncols) {
  __shared__ float buf[256];
  float acc = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    const int nvalid = ncols - 256 * t;
    const float v = (int)threadIdx.x < nvalid ? x[256 * t + threadIdx.x] : 0.f;
    buf[threadIdx.x] = v;
    __syncthreads();
    acc += buf[(threadIdx.x + 1) & 255];
    __syncthreads();
  }
  out[threadIdx.x] = acc;
}
}  // namespace
void launch(const float* x, float* out, int ntiles, int ncols) {
  hipLaunchKernelGGL((score_kernel<0, 0, false, false, 4, 0>), dim3(1), dim3(256), 0, 0, x, out, ntiles, ncols);
}
