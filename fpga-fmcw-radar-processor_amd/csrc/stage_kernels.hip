// stage_kernels.hip -- the small kernels of the stage entry points (fmcw_range_ct, fmcw_magnitude).
#include "cfar1d.hpp"
#include "handle.hpp"

namespace fmcw {

// inter (tiled) -> spec[fr][r][c] canonical corner-turner order.
__global__ void k_unblock(const float2* __restrict__ inter, float2* __restrict__ spec, int ns, int nc,
                          int T, int RB, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t per = (size_t)ns * nc;
  const size_t fr = i / per;
  const int rem = (int)(i - fr * per);
  const int r = rem / nc, c = rem - r * nc;
  const int ncb = nc / T;
  const size_t off = ((size_t)((r / RB) * ncb + c / T) * RB + (r % RB)) * T + (c % T);
  spec[i] = inter[fr * per + off];
}

__global__ void k_magnitude(const float2* __restrict__ iq, float* __restrict__ out, size_t n, int mode) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float2 X = iq[i];
  if (mode == FMCW_MAG_AMBM) {
    const float ai = fabsf(X.x), aq = fabsf(X.y);
    const float mx = fmaxf(ai, aq), mn = fminf(ai, aq);
    out[i] = mx + floorf(mn * 0.25f) + floorf(mn * 0.125f);
  } else {
    out[i] = mag_sqrt(X.x * X.x + X.y * X.y);
  }
}

int launch_unblock(const float2* inter, float2* spec, int ns, int nc, int T, int RB, size_t total, hipStream_t s) {
  hipLaunchKernelGGL(k_unblock, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, inter, spec, ns, nc, T, RB,
                     total);
  return check_launch("k_unblock");
}

int launch_magnitude(const float2* iq, float* out, size_t n, int mode, hipStream_t s) {
  hipLaunchKernelGGL(k_magnitude, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, iq, out, n, mode);
  return check_launch("k_magnitude");
}

}  // namespace fmcw
