// The float32 latent chain of upstream Wan2.1 sampling (wan/text2video.py:182-250, wan/image2video.py:198-329): CFG combine + one
// FlowUniPCMultistepScheduler.step (fm_solvers_unipc.py:486-626 / 350-484) or one FlowDPMSolverMultistepScheduler.step
// (fm_solvers.py:706-797) on float32 latents and float32 solver state, with the forward's bf16 flows in and the bf16 rounding of
// the new latents out (x_bf16: what the next step's forwards read).  One pass per denoise step; the per-step scalars come from the
// host scheduler (mmpl_amd/scheduler.py) or, in the table form, from a device table, so that a whole step stays ONE hipGraph.
//
// Numerics: every operation is ONE IEEE fp32 operation in the order of the reference's tensor expressions.  The whole file is
// compiled with `#pragma clang fp contract(off)` and uses plain operators: no product is contracted into an FMA, `/` is the
// correctly rounded division.  fc, fu = the bf16 flows widened.
//   f      = fu + g * (fc - fu)                                             (fc when fu is NULL)
//   m_conv = x - sigma_cur * f
//   UniPC   corrector (use_corrector):  xt_ = c_c1 * last - c_c2 * m0;  d1t = m_conv - m0
//                                       acc = (order 2: c_rho0 * ((m1 - m0) / c_rk), order 1: 0) + c_rho_last * d1t
//                                       x   = xt_ - c_c3 * acc
//           m1 <- m0;  m0 <- m_conv;  last <- x
//           predictor:                  xt_ = p_c1 * x - p_c2 * m0
//                                       x'  = xt_ - p_c3 * (order 2: 0.5 * ((m1 - m0) / p_rk), order 1: 0)
//   DPM-Solver++(2M)   m1 <- m0;  m0 <- m_conv
//                      order 1:  x' = c1 * x - c2 * m0
//                      order 2:  x' = (c1 * x - c2 * m0) - (0.5 * c2) * (inv_r0 * (m0 - m1))
//   x_bf16 = bf16(x'), round to nearest even
// The two `+ 0` / `* 0` of the first-order branches are the reference's (`corr_res = 0`, `pred_res = 0`): they only decide the sign
// of a zero.  Denormal values are outside the contract.
#include "../../include/mmpl_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

MMPL_DEV float cfg_flow(float fc, float fu, bool cfg, float g) {
  if (!cfg) return fc;
  const float d = fc - fu;
  const float gd = g * d;
  return fu + gd;
}

struct UniPCF32 {
  static constexpr bool kLast = true;
  MmplUniPCStepF32 st;
  MMPL_DEV float guidance() const { return st.guidance; }
  // m0 / m1 / last in: the state before the step, out: after it; returns the next sample
  MMPL_DEV float operator()(float f, float x, float& m0, float& m1, float& last) const {
    const float sf = st.sigma_cur * f;
    const float mc = x - sf;                                          // convert_model_output
    if (st.use_corrector) {
      const float a0 = st.c_c1 * last;
      const float a1 = st.c_c2 * m0;
      const float xt_ = a0 - a1;
      const float d1t = mc - m0;
      float corr = 0.0f;
      if (st.corr_order == 2) {
        const float dm = m1 - m0;
        const float d1 = dm / st.c_rk;
        corr = st.c_rho0 * d1;
      }
      const float rd = st.c_rho_last * d1t;
      const float acc = corr + rd;
      const float ca = st.c_c3 * acc;
      x = xt_ - ca;
    }
    m1 = m0;
    m0 = mc;
    last = x;
    const float b0 = st.p_c1 * x;
    const float b1 = st.p_c2 * m0;
    const float xt_ = b0 - b1;
    float pr = 0.0f;
    if (st.pred_order == 2) {
      const float dm = m1 - m0;
      const float d1 = dm / st.p_rk;
      pr = 0.5f * d1;
    }
    const float cp = st.p_c3 * pr;
    return xt_ - cp;
  }
};

struct DpmppF32 {
  static constexpr bool kLast = false;
  MmplDpmppStep st;
  MMPL_DEV float guidance() const { return st.guidance; }
  MMPL_DEV float operator()(float f, float x, float& m0, float& m1, float&) const {
    const float sf = st.sigma_cur * f;
    const float mc = x - sf;
    m1 = m0;
    m0 = mc;
    const float c1x = st.c1 * x;
    const float t0 = st.c2 * m0;
    float acc = c1x - t0;
    if (st.order == 2) {
      const float dm = m0 - m1;
      const float d1 = st.inv_r0 * dm;
      const float hc2 = 0.5f * st.c2;
      const float t1 = hc2 * d1;
      acc = acc - t1;
    }
    return acc;
  }
};

// One lane = 8 consecutive elements per round of a grid-stride loop: one 16-byte access per bf16 operand, two per float operand.
// kVec = every pointer 16-byte aligned (else, and for the ragged tail, element-wise loads / stores).
template <bool kVec, class Solver>
MMPL_DEV void chain_body(const F32ChainPtrs& a, const Solver& sv) {
  const bool cfg = a.flow_u != nullptr;
  const float g = sv.guidance();
  const size_t stride = (size_t)gridDim.x * blockDim.x * 8;
  for (size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; i0 < a.n; i0 += stride) {
    if (kVec && i0 + 8 <= a.n) {
      const bf16x8 fv = *reinterpret_cast<const bf16x8*>(a.flow_c + i0);
      bf16x8 uv{};
      if (cfg) uv = *reinterpret_cast<const bf16x8*>(a.flow_u + i0);
      f32x4 xv[2], m0v[2], m1v[2], lv[2] = {};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        xv[h] = *reinterpret_cast<const f32x4*>(a.x + i0 + 4 * h);
        m0v[h] = *reinterpret_cast<const f32x4*>(a.m0 + i0 + 4 * h);
        m1v[h] = *reinterpret_cast<const f32x4*>(a.m1 + i0 + 4 * h);
        if (Solver::kLast) lv[h] = *reinterpret_cast<const f32x4*>(a.last + i0 + 4 * h);
      }
      bf16x8 ob;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float m0 = m0v[j >> 2][j & 3], m1 = m1v[j >> 2][j & 3], last = lv[j >> 2][j & 3];
        const float f = cfg_flow(bf2f((bf16_t)fv[j]), bf2f((bf16_t)uv[j]), cfg, g);
        const float o = sv(f, xv[j >> 2][j & 3], m0, m1, last);
        xv[j >> 2][j & 3] = o;
        m0v[j >> 2][j & 3] = m0;
        m1v[j >> 2][j & 3] = m1;
        lv[j >> 2][j & 3] = last;
        ob[j] = (short)f2bf(o);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        *reinterpret_cast<f32x4*>(a.m1 + i0 + 4 * h) = m1v[h];
        *reinterpret_cast<f32x4*>(a.m0 + i0 + 4 * h) = m0v[h];
        if (Solver::kLast) *reinterpret_cast<f32x4*>(a.last + i0 + 4 * h) = lv[h];
        *reinterpret_cast<f32x4*>(a.x + i0 + 4 * h) = xv[h];
      }
      if (a.x_bf16) *reinterpret_cast<bf16x8*>(a.x_bf16 + i0) = ob;
      continue;
    }
    const size_t end = i0 + 8 < a.n ? i0 + 8 : a.n;   // ragged tail (or unaligned operands)
    for (size_t i = i0; i < end; ++i) {
      float m0 = a.m0[i], m1 = a.m1[i], last = Solver::kLast ? a.last[i] : 0.0f;
      const float f = cfg_flow(bf2f(a.flow_c[i]), cfg ? bf2f(a.flow_u[i]) : 0.0f, cfg, g);
      const float o = sv(f, a.x[i], m0, m1, last);
      a.m1[i] = m1;
      a.m0[i] = m0;
      if (Solver::kLast) a.last[i] = last;
      a.x[i] = o;
      if (a.x_bf16) a.x_bf16[i] = f2bf(o);
    }
  }
}

template <bool kVec, class Solver>
__global__ void __launch_bounds__(256) chain_kernel(F32ChainPtrs a, Solver sv) { chain_body<kVec>(a, sv); }

template <bool kVec, class Solver, class Step>
__global__ void __launch_bounds__(256) chain_table_kernel(F32ChainPtrs a, const Step* table, const int* step, int n_steps) {
  const int s = *step;
  if (s >= n_steps || s < 0) return;     // a replay beyond the uploaded table must not apply garbage coefficients
  Solver sv;
  sv.st = table[s];
  chain_body<kVec>(a, sv);
}

// after the update (stream order): *step += 1, the NEXT step's timestep -> t_out[0..n_t)
__global__ void chain_advance_kernel(int* step, float* t_out, const float* t_tab, int n_t, int n_steps) {
  const int cur = *step;
  if (cur >= n_steps || cur < 0) return;
  const int nxt = cur + 1;
  __syncthreads();                       // every lane has read *step before lane 0 overwrites it
  if (threadIdx.x == 0) *step = nxt;
  const float t = t_tab[nxt < n_steps ? nxt : n_steps - 1];
  for (int i = threadIdx.x; i < n_t; i += blockDim.x) t_out[i] = t;
}

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool vectorised(const F32ChainPtrs& a) {
  return aligned16(a.flow_c) && aligned16(a.flow_u) && aligned16(a.x) && aligned16(a.m0) && aligned16(a.m1) && aligned16(a.last) &&
         aligned16(a.x_bf16);
}
dim3 grid_of(size_t n) {
  const size_t blocks = ((n + 7) / 8 + 255) / 256;
  return dim3((unsigned)(blocks == 0 ? 1 : (blocks > 8192 ? 8192 : blocks)));   // the loop strides over the rest
}

template <class Solver, class Step>
hipError_t launch(const F32ChainPtrs& a, const Step* st, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  Solver sv;
  sv.st = *st;
  if (vectorised(a))
    hipLaunchKernelGGL((chain_kernel<true, Solver>), grid_of(a.n), dim3(256), 0, s, a, sv);
  else
    hipLaunchKernelGGL((chain_kernel<false, Solver>), grid_of(a.n), dim3(256), 0, s, a, sv);
  return hipGetLastError();
}

template <class Solver, class Step>
hipError_t launch_table(const F32ChainPtrs& a, const Step* table, int* step, float* t_out, const float* t_tab, int n_t, int n_steps,
                        hipStream_t s) {
  if (a.n != 0) {
    if (vectorised(a))
      hipLaunchKernelGGL((chain_table_kernel<true, Solver, Step>), grid_of(a.n), dim3(256), 0, s, a, table, step, n_steps);
    else
      hipLaunchKernelGGL((chain_table_kernel<false, Solver, Step>), grid_of(a.n), dim3(256), 0, s, a, table, step, n_steps);
  }
  hipLaunchKernelGGL(chain_advance_kernel, dim3(1), dim3(64), 0, s, step, t_out, t_tab, n_t, n_steps);
  return hipGetLastError();
}

}  // namespace

hipError_t mmpl_launch_unipc_f32(const F32ChainPtrs& a, const MmplUniPCStepF32* st, hipStream_t s) { return launch<UniPCF32>(a, st, s); }
hipError_t mmpl_launch_dpmpp_f32(const F32ChainPtrs& a, const MmplDpmppStep* st, hipStream_t s) { return launch<DpmppF32>(a, st, s); }
hipError_t mmpl_launch_unipc_f32_table(const F32ChainPtrs& a, const MmplUniPCStepF32* table, int* step, float* t_out, const float* t_tab,
                                       int n_t, int n_steps, hipStream_t s) {
  return launch_table<UniPCF32>(a, table, step, t_out, t_tab, n_t, n_steps, s);
}
hipError_t mmpl_launch_dpmpp_f32_table(const F32ChainPtrs& a, const MmplDpmppStep* table, int* step, float* t_out, const float* t_tab,
                                       int n_t, int n_steps, hipStream_t s) {
  return launch_table<DpmppF32>(a, table, step, t_out, t_tab, n_t, n_steps, s);
}
