// CFG combine + one FlowDPMSolverMultistepScheduler.step (DPM-Solver++(2M), midpoint, flow_prediction, final sigma 0) of the
// denoise loop with sample_solver = 'dpm++' (pipeline/casual_fps_inference.py:366-374, wan/utils/fm_solvers.py:706-797).
// One pass over the stage's latents instead of ~15 PyTorch launches; the per-step scalars come from the host scheduler
// (mmpl_amd/scheduler.py) or, in the table form, from a device table, so that a whole denoise step stays ONE hipGraph.
//
// Numerics: one IEEE fp32 operation between the bf16 roundings PyTorch makes on the reference's native platform, where a 0-dim fp32
// scalar is not rounded to the tensor's dtype.  The reference upcasts `sample` to fp32 before the update (:760), so c1 * x is NOT
// rounded and the running sum stays in fp32 until the final cast; every product with a bf16 tensor (m0, D1) rounds.
//   f   = rbf(fu + rbf(g * rbf(fc - fu)))                      (fc when fu is NULL)
//   x0  = rbf(x - rbf(sigma_cur * f));   m1 <- m0;  m0 <- x0    convert_model_output :380-383, on the bf16 sample
//   order 1:  x' = rbf( c1 * x - rbf(c2 * m0) )                :466-468
//   order 2:  d1 = rbf(inv_r0 * rbf(m0 - m1))                  :547
//             x' = rbf( (c1 * x - rbf(c2 * m0)) - rbf((0.5f * c2) * d1) )      :551-553
// Every operation rounds on its own: no FMA contraction in this file.
#include "../../include/mmpl_hip.h"
#include "common.h"

#pragma clang fp contract(off)

#include "mmpl_error.h"

namespace {

struct DpmppPtrs {
  const bf16_t* flow_c; const bf16_t* flow_u;   // flow_u == null: flow_c is already the combined flow
  bf16_t* x;                                    // sample in / next sample out
  bf16_t* m0; bf16_t* m1;                       // solver history (updated in place)
  size_t n;
};

// one element; m0 / m1 in: the history before the step, out: after the rotation
MMPL_DEV bf16_t dpmpp_one(bf16_t fc, bf16_t fu, bool cfg, bf16_t xb, bf16_t& m0b, bf16_t& m1b, const MmplDpmppStep& st) {
  float f = bf2f(fc);
  if (cfg) {
    const float u = bf2f(fu);
    const float d = rbf(f - u);
    const float gd = rbf(st.guidance * d);
    f = rbf(u + gd);
  }
  const float x = bf2f(xb);
  const float sf = rbf(st.sigma_cur * f);
  const float m0 = rbf(x - sf);
  const float m1 = bf2f(m0b);
  m1b = m0b;
  m0b = f2bf(m0);
  const float c1x = st.c1 * x;
  const float t0 = rbf(st.c2 * m0);
  float acc = c1x - t0;
  if (st.order == 2) {
    const float dm = rbf(m0 - m1);
    const float d1 = rbf(st.inv_r0 * dm);
    const float hc2 = 0.5f * st.c2;
    const float t1 = rbf(hc2 * d1);
    acc = acc - t1;
  }
  return f2bf(acc);
}

// one thread = 8 consecutive elements; kVec = every pointer 16-byte aligned (else element-wise loads / stores)
template <bool kVec>
MMPL_DEV void dpmpp_body(const DpmppPtrs& a, const MmplDpmppStep& st) {
  const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i0 >= a.n) return;
  const bool cfg = a.flow_u != nullptr;
  if (kVec && i0 + 8 <= a.n) {
    const bf16x8 fv = *reinterpret_cast<const bf16x8*>(a.flow_c + i0);
    bf16x8 uv{};
    if (cfg) uv = *reinterpret_cast<const bf16x8*>(a.flow_u + i0);
    const bf16x8 xv = *reinterpret_cast<const bf16x8*>(a.x + i0);
    bf16x8 m0v = *reinterpret_cast<const bf16x8*>(a.m0 + i0);
    bf16x8 m1v, ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16_t m0 = (bf16_t)m0v[j], m1 = 0;
      ov[j] = (short)dpmpp_one((bf16_t)fv[j], (bf16_t)uv[j], cfg, (bf16_t)xv[j], m0, m1, st);
      m0v[j] = (short)m0;
      m1v[j] = (short)m1;
    }
    *reinterpret_cast<bf16x8*>(a.m1 + i0) = m1v;
    *reinterpret_cast<bf16x8*>(a.m0 + i0) = m0v;
    *reinterpret_cast<bf16x8*>(a.x + i0) = ov;
    return;
  }
  const size_t end = i0 + 8 < a.n ? i0 + 8 : a.n;   // ragged tail (or unaligned operands)
  for (size_t i = i0; i < end; ++i) {
    bf16_t m0 = a.m0[i], m1 = 0;
    const bf16_t o = dpmpp_one(a.flow_c[i], cfg ? a.flow_u[i] : (bf16_t)0, cfg, a.x[i], m0, m1, st);
    a.m1[i] = m1;
    a.m0[i] = m0;
    a.x[i] = o;
  }
}

template <bool kVec>
__global__ void __launch_bounds__(256) dpmpp_kernel(DpmppPtrs a, MmplDpmppStep st) { dpmpp_body<kVec>(a, st); }

template <bool kVec>
__global__ void __launch_bounds__(256) dpmpp_table_kernel(DpmppPtrs a, const MmplDpmppStep* table, const int* step, int n_steps) {
  const int s = *step;
  if (s >= n_steps || s < 0) return;     // a replay beyond the uploaded table must not apply garbage coefficients
  dpmpp_body<kVec>(a, table[s]);
}

// after the update (stream order): *step += 1, the NEXT step's timestep -> t_out[0..n_t)
__global__ void dpmpp_advance_kernel(int* step, float* t_out, const float* t_tab, int n_t, int n_steps) {
  const int cur = *step;
  if (cur >= n_steps || cur < 0) return;
  const int nxt = cur + 1;
  __syncthreads();                       // every lane has read *step before lane 0 overwrites it
  if (threadIdx.x == 0) *step = nxt;
  const float t = t_tab[nxt < n_steps ? nxt : n_steps - 1];
  for (int i = threadIdx.x; i < n_t; i += blockDim.x) t_out[i] = t;
}

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int fill(const char* where, DpmppPtrs& a, const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, size_t n) {
  if (!flow_cond || !x || !m0 || !m1) return mmpl_set_error(where, "null argument");
  if (n / 8 >= (size_t)0x7fffffff * 256) return mmpl_set_error(where, "n too large");
  a.flow_c = (const bf16_t*)flow_cond; a.flow_u = (const bf16_t*)flow_uncond; a.x = (bf16_t*)x; a.m0 = (bf16_t*)m0; a.m1 = (bf16_t*)m1;
  a.n = n;
  return 0;
}
bool vectorised(const DpmppPtrs& a) { return aligned16(a.flow_c) && aligned16(a.flow_u) && aligned16(a.x) && aligned16(a.m0) && aligned16(a.m1); }
dim3 grid_of(size_t n) {
  const size_t threads = (n + 7) / 8;
  return dim3((unsigned)(threads == 0 ? 1 : (threads + 255) / 256));
}

}  // namespace

extern "C" int mmpl_cfg_dpmpp_step(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, size_t n,
                                   const MmplDpmppStep* st, mmpl_stream_t stream) {
  if (!st) return mmpl_set_error("mmpl_cfg_dpmpp_step", "null step");
  DpmppPtrs a = {};
  if (fill("mmpl_cfg_dpmpp_step", a, flow_cond, flow_uncond, x, m0, m1, n)) return 1;
  if (st->order != 1 && st->order != 2) return mmpl_set_error("mmpl_cfg_dpmpp_step", "order must be 1 or 2");
  if (n == 0) return 0;
  if (vectorised(a))
    hipLaunchKernelGGL(dpmpp_kernel<true>, grid_of(n), dim3(256), 0, (hipStream_t)stream, a, *st);
  else
    hipLaunchKernelGGL(dpmpp_kernel<false>, grid_of(n), dim3(256), 0, (hipStream_t)stream, a, *st);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mmpl_set_error("mmpl_cfg_dpmpp_step", hipGetErrorString(e));
  return 0;
}

extern "C" int mmpl_cfg_dpmpp_step_table(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, size_t n,
                                         const MmplDpmppStep* table_dev, int* step_dev, float* timestep_dev,
                                         const float* timestep_table_dev, int n_timestep, int n_steps, mmpl_stream_t stream) {
  if (!table_dev || !step_dev || !timestep_dev || !timestep_table_dev || n_steps < 1 || n_timestep < 1)
    return mmpl_set_error("mmpl_cfg_dpmpp_step_table", "bad arguments");
  DpmppPtrs a = {};
  if (fill("mmpl_cfg_dpmpp_step_table", a, flow_cond, flow_uncond, x, m0, m1, n)) return 1;
  const hipStream_t s = (hipStream_t)stream;
  if (n != 0) {
    if (vectorised(a))
      hipLaunchKernelGGL(dpmpp_table_kernel<true>, grid_of(n), dim3(256), 0, s, a, table_dev, step_dev, n_steps);
    else
      hipLaunchKernelGGL(dpmpp_table_kernel<false>, grid_of(n), dim3(256), 0, s, a, table_dev, step_dev, n_steps);
  }
  hipLaunchKernelGGL(dpmpp_advance_kernel, dim3(1), dim3(64), 0, s, step_dev, timestep_dev, timestep_table_dev, n_timestep, n_steps);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mmpl_set_error("mmpl_cfg_dpmpp_step_table", hipGetErrorString(e));
  return 0;
}
