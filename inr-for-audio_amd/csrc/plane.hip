// The loss-landscape plane (run.py:192-198, visualization=True): the loss at steps x steps weight
// settings theta_ij = theta + a_i d1 + b_j d2 around the fitted weights.  Per grid point one launch
// builds the parameters and the fp16 shadows of a scratch network (plane_point); the forward and the
// squared error are the training path's own kernels (capi.hip siren_plane_eval); plane_loss finishes
// a micro-batch's block partials into the point's fp64 slot.
#include "siren_common.h"
#include "siren_kernels.h"

namespace siren {

// theta_ij of one element: fma(b, d2, fma(a, d1, theta)), two correctly rounded fp32 fmas
__device__ __forceinline__ float plane_at(float t, float u, float v, float a, float b) {
  return __builtin_fmaf(b, v, __builtin_fmaf(a, u, t));
}

// Blocks [0, ntile): one 64x64 tile of a hidden weight each -- the fp32 value is formed once, stored
// to `out` and cast into both shadows by cast_weight's own tile body (cast_tile64), so the shadows are
// bit for bit siren_cast_weight(out).  Blocks [ntile, gridDim.x): the rest of the vector (first layer,
// biases, Snake a, head, alignment gaps) as float4, grid-stride over each piece.  Directions are zero
// in pads and gaps, so those keep theta's value (fma(b, 0, fma(a, 0, t)) = t).
__global__ void plane_point_kernel(const float* __restrict__ theta, const float* __restrict__ d1,
                                   const float* __restrict__ d2, float a, float b, float* __restrict__ out,
                                   PlaneSet ps, int H, int ntile) {
  __shared__ float tile[64][65];
  if ((int)blockIdx.x < ntile) {
    const int tw = H >> 6, per = tw * tw;
    const int l = blockIdx.x / per, t = blockIdx.x - l * per;
    const size_t base = (size_t)ps.w_off[l];
    const float* __restrict__ T = theta + base;
    const float* __restrict__ U = d1 + base;
    const float* __restrict__ V = d2 + base;
    float* __restrict__ O = out + base;
    cast_tile64(
        [=](size_t i) {
          const float w = plane_at(T[i], U[i], V[i], a, b);
          O[i] = w;
          return w;
        },
        H, H, (t / tw) * 64, (t % tw) * 64, ps.Wb[l], ps.WTb[l], tile);
    return;
  }
  const int64_t first = (int64_t)(blockIdx.x - ntile) * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)(gridDim.x - ntile) * blockDim.x;
  const float4* __restrict__ T4 = (const float4*)theta;
  const float4* __restrict__ U4 = (const float4*)d1;
  const float4* __restrict__ V4 = (const float4*)d2;
  float4* __restrict__ O4 = (float4*)out;
  for (int r = 0; r < ps.nrest; ++r) {
    const int64_t hi = ps.hi[r];
    for (int64_t i = ps.lo[r] + first; i < hi; i += stride) {
      const float4 t = T4[i], u = U4[i], v = V4[i];
      float4 o;
      o.x = plane_at(t.x, u.x, v.x, a, b);
      o.y = plane_at(t.y, u.y, v.y, a, b);
      o.z = plane_at(t.z, u.z, v.z, a, b);
      o.w = plane_at(t.w, u.w, v.w, a, b);
      O4[i] = o;
    }
  }
}

hipError_t plane_point(const float* theta, const float* d1, const float* d2, float a, float b, float* out,
                       const PlaneSet& ps, int H, hipStream_t s) {
  if (H < 64 || H % 64 || ps.n < 1 || ps.n > kMaxInner || ps.nrest < 0 || ps.nrest > kMaxInner + 1)
    return hipErrorInvalidValue;
  const int ntile = ps.n * (H / 64) * (H / 64);
  int64_t rest4 = 0;
  for (int r = 0; r < ps.nrest; ++r) rest4 += ps.hi[r] - ps.lo[r];
  int64_t nrest_blocks = (rest4 + 255) / 256;
  if (nrest_blocks > 256) nrest_blocks = 256;
  hipLaunchKernelGGL(plane_point_kernel, dim3(ntile + (int)nrest_blocks), dim3(256), 0, s, theta, d1, d2, a, b, out,
                     ps, H, ntile);
  return hipGetLastError();
}

// One block: thread t adds sse_part[t], sse_part[t + 256], ... in fp64, then a halving tree over the
// 256 sums -- the same order whatever ran before, so a plane is reproducible bit for bit.  The slot is
// this point's alone and the micro-batches' launches are ordered on one stream: a plain add.
__global__ void plane_loss_kernel(const float* __restrict__ sse_part, int nparts, double* __restrict__ slot) {
  __shared__ double acc[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) v += (double)sse_part[i];
  acc[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) slot[0] += acc[0];
}

hipError_t plane_loss(const float* sse_part, int nparts, double* slot, hipStream_t s) {
  if (nparts < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plane_loss_kernel, dim3(1), dim3(256), 0, s, sse_part, nparts, slot);
  return hipGetLastError();
}

}  // namespace siren
