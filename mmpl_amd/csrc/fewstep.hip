// Few-step (Self-Forcing / CausVid) latent update: WanDiffusionWrapper._convert_flow_pred_to_x0 (utils/wan_wrapper.py:172-199)
// followed by FlowMatchScheduler.add_noise (utils/scheduler.py:160-176), as CausalInferencePipeline.inference chains them
// (pipeline/causal_inference.py:176-197).  One pass over the block's latents instead of ~10 PyTorch launches, and no host
// read-back: safe inside a stream capture.
//
// Numerics (bit-identical to PyTorch evaluating the reference's expressions):
//   x0   = bf16( float( double(xt) - sigma_t * double(flow) ) )      the reference's .double() chain; double -> bf16 goes
//                                                                     through float like c10::BFloat16's constructor
//   x'   = bf16( fp32(fp32(1 - s) * x0) + fp32(s * noise) )          add_noise: fp32 sigma against bf16 tensors
// Every operation rounds on its own: no FMA contraction in this file.
#include "../../include/mmpl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

#include "mmpl_error.h"

namespace {

MMPL_DEV bf16_t x0_of(bf16_t xt, bf16_t flow, double sigma_t) {
  const double prod = sigma_t * (double)bf2f(flow);
  const double d = (double)bf2f(xt) - prod;
  return f2bf((float)d);
}

MMPL_DEV bf16_t renoise(bf16_t x0, bf16_t noise, float s, float one_minus_s) {
  const float a = one_minus_s * bf2f(x0);
  const float b = s * bf2f(noise);
  return f2bf(a + b);
}

// one thread = 8 consecutive elements; vec = every pointer 16-byte aligned (else element-wise loads / stores)
template <bool kNoise, bool kVec>
__global__ void __launch_bounds__(256) fewstep_update_kernel(const bf16_t* __restrict__ flow, bf16_t* x, const bf16_t* __restrict__ noise,
                                                             bf16_t* x0_out, size_t n, double sigma_t, float s) {
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i0 >= n) return;
  const float oms = 1.0f - s;
  if (kVec && i0 + 8 <= n) {
    const bf16x8 fv = *reinterpret_cast<const bf16x8*>(flow + i0);
    const bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + i0);
    bf16x8 nv{};
    if (kNoise) nv = *reinterpret_cast<const bf16x8*>(noise + i0);
    bf16x8 ov, rv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16_t x0 = x0_of((bf16_t)xv[j], (bf16_t)fv[j], sigma_t);
      ov[j] = (short)x0;
      if (kNoise) rv[j] = (short)renoise(x0, (bf16_t)nv[j], s, oms);
    }
    *reinterpret_cast<bf16x8*>(x0_out + i0) = ov;
    if (kNoise) *reinterpret_cast<bf16x8*>(x + i0) = rv;
    return;
  }
  const size_t end = i0 + 8 < n ? i0 + 8 : n;   // ragged tail (or unaligned operands)
  for (size_t i = i0; i < end; ++i) {
    const bf16_t xt = x[i];
    const bf16_t x0 = x0_of(xt, flow[i], sigma_t);
    x0_out[i] = x0;
    if (kNoise) x[i] = renoise(x0, noise[i], s, oms);
  }
}

template <bool kNoise>
hipError_t launch(const bf16_t* flow, bf16_t* x, const bf16_t* noise, bf16_t* x0_out, size_t n, double sigma_t, float s, bool vec,
                  hipStream_t st) {
  const size_t threads = (n + 7) / 8;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (vec)
    hipLaunchKernelGGL((fewstep_update_kernel<kNoise, true>), grid, block, 0, st, flow, x, noise, x0_out, n, sigma_t, s);
  else
    hipLaunchKernelGGL((fewstep_update_kernel<kNoise, false>), grid, block, 0, st, flow, x, noise, x0_out, n, sigma_t, s);
  return hipGetLastError();
}

}  // namespace

extern "C" int mmpl_fewstep_update(const void* flow, void* x, const void* noise, void* x0_out, size_t n, double sigma_t,
                                   float sigma_next, mmpl_stream_t stream) {
  if (n == 0) return 0;
  if (!flow || !x || !x0_out) return mmpl_set_error("mmpl_fewstep_update", "null argument");
  if (n / 8 >= (size_t)0x7fffffff * 256) return mmpl_set_error("mmpl_fewstep_update", "n too large");
  const auto aligned = [](const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = aligned(flow) && aligned(x) && aligned(noise) && aligned(x0_out);
  const hipError_t e = noise ? launch<true>((const bf16_t*)flow, (bf16_t*)x, (const bf16_t*)noise, (bf16_t*)x0_out, n, sigma_t,
                                            sigma_next, vec, (hipStream_t)stream)
                             : launch<false>((const bf16_t*)flow, (bf16_t*)x, nullptr, (bf16_t*)x0_out, n, sigma_t, sigma_next, vec,
                                             (hipStream_t)stream);
  if (e != hipSuccess) return mmpl_set_error("mmpl_fewstep_update", hipGetErrorString(e));
  return 0;
}
