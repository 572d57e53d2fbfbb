// Step caching (TeaCache) of the 50-step samplers (include/mmpl_hip.h: mmpl_dit_forward_*_cached, mmpl_rel_l1_rows): the two
// kernels the cached forward and its indicator add to the forward's own.
//   residual_sub: r = bf16(float(xL) - float(x0)), what a computed step leaves for the steps that reuse it
//   rel_l1_rows:  out[i] = sum_c |x[i+1,c] - x[i,c]| / sum_c |x[i,c]|, the distance between consecutive timestep embeddings
#include <stdint.h>

#include "../../include/mmpl_hip.h"
#include "host_util.h"

namespace {

// r[i] = bf16(float(xl[i]) - float(x0[i])): one fp32 subtraction, one rounding.  VEC: 8 elements (16 bytes) per lane and trip over
// the first n_vec * 8 elements; the scalar form takes elements first .. n - 1 (the tail, or everything when a pointer is not
// 16-byte aligned).
__global__ __launch_bounds__(256) void residual_sub_vec_kernel(const u32x4* xl, const u32x4* x0, u32x4* r, size_t n_vec) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (size_t)gridDim.x * 256) {
    const u32x4 a = xl[i], b = x0[i];
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float lo = bf2f((bf16_t)(a[k] & 0xffffu)) - bf2f((bf16_t)(b[k] & 0xffffu));
      const float hi = bf2f((bf16_t)(a[k] >> 16)) - bf2f((bf16_t)(b[k] >> 16));
      o[k] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
    }
    r[i] = o;
  }
}
__global__ __launch_bounds__(256) void residual_sub_scalar_kernel(const bf16_t* xl, const bf16_t* x0, bf16_t* r, size_t first, size_t n) {
  for (size_t i = first + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    r[i] = f2bf(bf2f(xl[i]) - bf2f(x0[i]));
}

// One 256-thread block per output i.  Summation order (fixed, so the result is the same bits on every run):
//   lane t of the block adds its columns t, t + 256, t + 512, ... in increasing order into two fp32 partials (numerator, denominator);
//   the 64 partials of a wave are combined by a butterfly, partner lane ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
//   thread 0 adds the four wave sums in wave order 0, 1, 2, 3 and divides once.
__global__ __launch_bounds__(256) void rel_l1_rows_kernel(const bf16_t* x, int ld, int d, float* out) {
  __shared__ float part[2][4];
  const bf16_t* a = x + (size_t)blockIdx.x * ld;
  const bf16_t* b = a + ld;
  float num = 0.f, den = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float va = bf2f(a[c]);
    num += fabsf(bf2f(b[c]) - va);
    den += fabsf(va);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    num += __shfl_xor(num, m, 64);
    den += __shfl_xor(den, m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = num;
    part[1][threadIdx.x >> 6] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float n4 = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    const float d4 = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    out[blockIdx.x] = n4 / d4;
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
int blocks_for(size_t n) { return (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256); }

}  // namespace

hipError_t mmpl_launch_residual_sub(const bf16_t* xl, const bf16_t* x0, bf16_t* r, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const bool vec = !misaligned(xl, 16) && !misaligned(x0, 16) && !misaligned(r, 16);
  const size_t n_vec = vec ? n / 8 : 0;
  if (n_vec)
    hipLaunchKernelGGL(residual_sub_vec_kernel, dim3(blocks_for(n_vec)), dim3(256), 0, s, (const u32x4*)xl, (const u32x4*)x0, (u32x4*)r, n_vec);
  if (n_vec * 8 < n)
    hipLaunchKernelGGL(residual_sub_scalar_kernel, dim3(blocks_for(n - n_vec * 8)), dim3(256), 0, s, xl, x0, r, n_vec * 8, n);
  return hipGetLastError();
}

hipError_t mmpl_launch_rel_l1_rows(const bf16_t* x, int ld, int rows, int d, float* out, hipStream_t s) {
  if (rows < 2) return hipSuccess;
  hipLaunchKernelGGL(rel_l1_rows_kernel, dim3(rows - 1), dim3(256), 0, s, x, ld, d, out);
  return hipGetLastError();
}

extern "C" int mmpl_rel_l1_rows(const void* x, int ld, int rows, int d, float* out_dev, mmpl_stream_t stream) {
  const char* me = "mmpl_rel_l1_rows";
  if (!x || !out_dev) return mmpl_set_error(me, "null argument");
  if (rows < 2) return mmpl_set_error(me, "rows < 2");
  if (d < 1) return mmpl_set_error(me, "non-positive size");
  if (ld < d) return mmpl_set_error(me, "ld < d");
  if (misaligned(x, 2) || misaligned(out_dev, 4)) return mmpl_set_error(me, "misaligned pointer");
  MMPL_HIP_TRY(mmpl_launch_rel_l1_rows((const bf16_t*)x, ld, rows, d, out_dev, (hipStream_t)stream), me);
  return 0;
}
