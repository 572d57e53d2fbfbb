// The samplers of the denoise loop: CFG combine + one solver step on the latents, ONE pass instead of ~15-25 PyTorch launches.
// Two solvers, FlowUniPCMultistepScheduler.step (fm_solvers_unipc.py:486-626 / 350-484; order <= 2, bh2, predict_x0) and
// FlowDPMSolverMultistepScheduler.step (fm_solvers.py:706-797; DPM-Solver++(2M), midpoint, flow_prediction, final sigma 0), each on
// two storage types of x / m0 / m1 / last:
//   bf16    the reference pipelines' chain (pipeline/casual_fps_inference.py:366-374): a bf16 rounding after every tensor operation
//   float   upstream Wan2.1 sampling (wan/text2video.py:182-250, wan/image2video.py:198-329): float32 latents and solver state, the
//           forward's bf16 flows in and the bf16 rounding of the new latents out (x_bf16: what the next step's forwards read)
// The per-step scalars come from the host scheduler (mmpl_amd/scheduler.py) in the public step structs of include/mmpl_hip.h or,
// in the table form, from a device table of the same structs, so that a whole denoise step stays ONE hipGraph.
//
// Numerics: every operation is ONE IEEE fp32 operation in the order of the reference's tensor expressions.  The whole file is
// compiled with `#pragma clang fp contract(off)` and uses plain operators: no product is contracted into an FMA, `/` is the
// correctly rounded division.  r() = round to bf16 (nearest even) for bf16 storage -- the roundings PyTorch makes on the
// reference's native platform, where a 0-dim fp32 scalar is not rounded to the tensor's dtype -- and the identity for float
// storage.  fc, fu = the bf16 flows widened.
//   f      = r(fu + r(g * r(fc - fu)))                                      (fc when fu is NULL)
//   m_conv = r(x - r(sigma_cur * f))                                        convert_model_output (fm_solvers.py:380-383)
//   DPM-Solver++(2M), both storage types:   m1 <- m0;  m0 <- m_conv
//     order 1:  x' = r( c1 * x - r(c2 * m0) )                                                     :466-468
//     order 2:  d1 = r(inv_r0 * r(m0 - m1))                                                       :547
//               x' = r( (c1 * x - r(c2 * m0)) - r((0.5f * c2) * d1) )                             :551-553
//     The reference upcasts `sample` to fp32 before the update (:760), so c1 * x is NOT rounded and the running sum stays in fp32
//     until the final cast; every product with a bf16 tensor (m0, D1) rounds.
//   UniPC, float storage (MmplUniPCStepF32: rk itself, the kernel DIVIDES as the reference does; rhos never rounded to bf16):
//     corrector (use_corrector):  xt_ = c_c1 * last - c_c2 * m0;  d1t = m_conv - m0
//                                 acc = (order 2: c_rho0 * ((m1 - m0) / c_rk), order 1: 0) + c_rho_last * d1t
//                                 x   = xt_ - c_c3 * acc
//     m1 <- m0;  m0 <- m_conv;  last <- x
//     predictor:                  xt_ = p_c1 * x - p_c2 * m0
//                                 x'  = xt_ - p_c3 * (order 2: 0.5 * ((m1 - m0) / p_rk), order 1: 0)
//     The two `+ 0` / `* 0` of the first-order branches are the reference's (`corr_res = 0`, `pred_res = 0`): they only decide the
//     sign of a zero.
//   UniPC, bf16 storage (MmplUniPCStep: 1 / rk, the kernel MULTIPLIES; every tensor op of fm_solvers_unipc.py:315-331 rounds):
//     corrector (use_corrector):  xt_ = r(r(c_c1 * last) - r(c_c2 * m0));  d1t = r(m_conv - m0)
//                                 acc = r(c_rho_last * d1t);  order 2: acc = r(r(c_rho0 * r(r(m1 - m0) * c_inv_rk)) + acc)
//                                 x   = r(xt_ - r(c_c3 * acc))
//     m1 <- m0;  m0 <- m_conv;  last <- x
//     predictor:                  x'  = r(r(p_c1 * x) - r(p_c2 * m0))
//                                 order 2: x' = r(x' - r(p_c3 * r(0.5f * r(r(m1 - m0) * p_inv_rk))))
//     The first-order branches skip the term, they do not add a zero: that, the reciprocal and the struct are why UniPC is two
//     functors where DPM-Solver++ is one template over r().
//   x_bf16 = bf16(x'), round to nearest even (float storage only)
// Denormal values are outside the contract.
#include "../../include/mmpl_hip.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

// the rounding after a tensor operation, by storage type
template <class T> MMPL_DEV float r(float v);
template <> MMPL_DEV float r<bf16_t>(float v) { return rbf(v); }
template <> MMPL_DEV float r<float>(float v) { return v; }

template <class T>
MMPL_DEV float cfg_flow(float fc, float fu, bool cfg, float g) {
  if (!cfg) return fc;
  const float d = r<T>(fc - fu);
  const float gd = r<T>(g * d);
  return r<T>(fu + gd);
}

// Solver<T, Step>: one step on one element of storage type T with the scalars of the public struct Step.
// m0 / m1 / last in: the state before the step, out: after it; returns the next sample.  For bf16 storage every value that leaves
// is already rounded to bf16, so the store's rounding changes no bit.
template <class T, class Step> struct Solver;

template <class T> struct Solver<T, MmplDpmppStep> {
  static constexpr bool kLast = false;
  MmplDpmppStep st;
  MMPL_DEV float operator()(float f, float x, float& m0, float& m1, float&) const {
    const float sf = r<T>(st.sigma_cur * f);
    const float mc = r<T>(x - sf);
    m1 = m0;
    m0 = mc;
    const float c1x = st.c1 * x;
    const float t0 = r<T>(st.c2 * m0);
    float acc = c1x - t0;
    if (st.order == 2) {
      const float dm = r<T>(m0 - m1);
      const float d1 = r<T>(st.inv_r0 * dm);
      const float hc2 = 0.5f * st.c2;
      const float t1 = r<T>(hc2 * d1);
      acc = acc - t1;
    }
    return r<T>(acc);
  }
};

template <> struct Solver<float, MmplUniPCStepF32> {
  static constexpr bool kLast = true;
  MmplUniPCStepF32 st;
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

template <> struct Solver<bf16_t, MmplUniPCStep> {
  static constexpr bool kLast = true;
  MmplUniPCStep st;
  MMPL_DEV float operator()(float f, float x, float& m0, float& m1, float& last) const {
    const float mc = rbf(x - rbf(st.sigma_cur * f));                  // convert_model_output
    if (st.use_corrector) {
      const float xt_ = rbf(rbf(st.c_c1 * last) - rbf(st.c_c2 * m0));
      const float d1t = rbf(mc - m0);
      float acc = rbf(st.c_rho_last * d1t);
      if (st.corr_order == 2) {
        const float d1 = rbf(rbf(m1 - m0) * st.c_inv_rk);
        acc = rbf(rbf(st.c_rho0 * d1) + acc);
      }
      x = rbf(xt_ - rbf(st.c_c3 * acc));
    }
    m1 = m0;
    m0 = mc;
    last = x;
    float xt = rbf(rbf(st.p_c1 * x) - rbf(st.p_c2 * m0));
    if (st.pred_order == 2) {
      const float d1 = rbf(rbf(m1 - m0) * st.p_inv_rk);
      xt = rbf(xt - rbf(st.p_c3 * rbf(0.5f * d1)));
    }
    return xt;
  }
};

// 8 consecutive elements of storage type T in registers: one 16-byte access for bf16 storage (get widens, set rounds), two for
// float.  The raw form is what is loaded, so no load waits for an earlier one to be converted.
template <class T> struct Vec8;
template <> struct Vec8<bf16_t> {
  bf16x8 v = {};
  MMPL_DEV void load(const bf16_t* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  MMPL_DEV void store(bf16_t* p) const { *reinterpret_cast<bf16x8*>(p) = v; }
  MMPL_DEV float get(int j) const { return bf2f((bf16_t)v[j]); }
  MMPL_DEV void set(int j, float f) { v[j] = (short)f2bf(f); }
};
template <> struct Vec8<float> {
  f32x4 v[2] = {};
  MMPL_DEV void load(const float* p) {
    v[0] = *reinterpret_cast<const f32x4*>(p);
    v[1] = *reinterpret_cast<const f32x4*>(p + 4);
  }
  MMPL_DEV void store(float* p) const {
    *reinterpret_cast<f32x4*>(p) = v[0];
    *reinterpret_cast<f32x4*>(p + 4) = v[1];
  }
  MMPL_DEV float get(int j) const { return v[j >> 2][j & 3]; }
  MMPL_DEV void set(int j, float f) { v[j >> 2][j & 3] = f; }
};
MMPL_DEV float load1(const bf16_t* p) { return bf2f(*p); }
MMPL_DEV float load1(const float* p) { return *p; }
MMPL_DEV void store1(bf16_t* p, float v) { *p = f2bf(v); }
MMPL_DEV void store1(float* p, float v) { *p = v; }

constexpr int kThreads = 256;              // every launch below; the kernels index with the constant, not with blockDim

// One lane = 8 consecutive elements per round of a grid-stride loop.
// kVec = every pointer 16-byte aligned (else, and for the ragged tail, element-wise loads / stores).
template <bool kVec, class T, class Step>
MMPL_DEV void step_body(const SamplerPtrs<T>& a, const Solver<T, Step>& sv) {
  constexpr bool kLast = Solver<T, Step>::kLast;
  const bool cfg = a.flow_u != nullptr;
  const float g = sv.st.guidance;
  const size_t stride = (size_t)gridDim.x * kThreads * 8;
  for (size_t i0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * 8; i0 < a.n; i0 += stride) {
    if (kVec && i0 + 8 <= a.n) {
      Vec8<bf16_t> fc, fu, xb;
      Vec8<T> x, m0, m1, last;
      fc.load(a.flow_c + i0);
      if (cfg) fu.load(a.flow_u + i0);
      x.load(a.x + i0);
      m0.load(a.m0 + i0);
      m1.load(a.m1 + i0);
      if (kLast) last.load(a.last + i0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float m0j = m0.get(j), m1j = m1.get(j), lastj = last.get(j);
        const float o = sv(cfg_flow<T>(fc.get(j), fu.get(j), cfg, g), x.get(j), m0j, m1j, lastj);
        m0.set(j, m0j);
        m1.set(j, m1j);
        last.set(j, lastj);
        x.set(j, o);
        xb.set(j, o);
      }
      m1.store(a.m1 + i0);
      m0.store(a.m0 + i0);
      if (kLast) last.store(a.last + i0);
      x.store(a.x + i0);
      if (sizeof(T) == 4 && a.x_bf16) xb.store(a.x_bf16 + i0);
      continue;
    }
    const size_t end = i0 + 8 < a.n ? i0 + 8 : a.n;   // ragged tail (or unaligned operands)
    for (size_t i = i0; i < end; ++i) {
      float m0 = load1(a.m0 + i), m1 = load1(a.m1 + i), last = kLast ? load1(a.last + i) : 0.0f;
      const float f = cfg_flow<T>(bf2f(a.flow_c[i]), cfg ? bf2f(a.flow_u[i]) : 0.0f, cfg, g);
      const float o = sv(f, load1(a.x + i), m0, m1, last);
      store1(a.m1 + i, m1);
      store1(a.m0 + i, m0);
      if (kLast) store1(a.last + i, last);
      store1(a.x + i, o);
      if (sizeof(T) == 4 && a.x_bf16) a.x_bf16[i] = f2bf(o);
    }
  }
}

template <bool kVec, class T, class Step>
__global__ void __launch_bounds__(kThreads) step_kernel(SamplerPtrs<T> a, Solver<T, Step> sv) { step_body<kVec>(a, sv); }

template <bool kVec, class T, class Step>
__global__ void __launch_bounds__(kThreads) step_table_kernel(SamplerPtrs<T> a, const Step* table, const int* step, int n_steps) {
  const int s = *step;
  if (s < 0 || s >= n_steps) return;     // a replay beyond the uploaded table must not apply garbage coefficients
  step_body<kVec>(a, Solver<T, Step>{table[s]});
}

// after the update (stream order): *step += 1, the NEXT step's timestep -> t_out[0..n_t)
__global__ void step_advance_kernel(int* step, float* t_out, const float* t_tab, int n_t, int n_steps) {
  const int cur = *step;
  if (cur < 0 || cur >= n_steps) return;
  const int nxt = cur + 1;
  __syncthreads();                       // every lane has read *step before lane 0 overwrites it
  if (threadIdx.x == 0) *step = nxt;
  const float t = t_tab[nxt < n_steps ? nxt : n_steps - 1];
  for (int i = threadIdx.x; i < n_t; i += blockDim.x) t_out[i] = t;
}

bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class T>
bool vectorised(const SamplerPtrs<T>& a) {
  return aligned16(a.flow_c) && aligned16(a.flow_u) && aligned16(a.x) && aligned16(a.m0) && aligned16(a.m1) && aligned16(a.last) &&
         aligned16(a.x_bf16);
}
dim3 grid_of(size_t n) {
  const size_t blocks = ((n + 7) / 8 + kThreads - 1) / kThreads;
  return dim3((unsigned)(blocks == 0 ? 1 : (blocks > 8192 ? 8192 : blocks)));   // the loop strides over the rest
}

}  // namespace

template <class T, class Step>
hipError_t mmpl_launch_sampler(const SamplerPtrs<T>& a, const Step* st, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const Solver<T, Step> sv{*st};
  if (vectorised(a))
    hipLaunchKernelGGL((step_kernel<true, T, Step>), grid_of(a.n), dim3(kThreads), 0, s, a, sv);
  else
    hipLaunchKernelGGL((step_kernel<false, T, Step>), grid_of(a.n), dim3(kThreads), 0, s, a, sv);
  return hipGetLastError();
}

template <class T, class Step>
hipError_t mmpl_launch_sampler_table(const SamplerPtrs<T>& a, const Step* table, int* step, float* t_out, const float* t_tab, int n_t,
                                     int n_steps, hipStream_t s) {
  if (a.n != 0) {
    if (vectorised(a))
      hipLaunchKernelGGL((step_table_kernel<true, T, Step>), grid_of(a.n), dim3(kThreads), 0, s, a, table, step, n_steps);
    else
      hipLaunchKernelGGL((step_table_kernel<false, T, Step>), grid_of(a.n), dim3(kThreads), 0, s, a, table, step, n_steps);
  }
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, s, step, t_out, t_tab, n_t, n_steps);
  return hipGetLastError();
}

// the four samplers
#define MMPL_SAMPLER(T, Step)                                                                                                  \
  template hipError_t mmpl_launch_sampler<T, Step>(const SamplerPtrs<T>&, const Step*, hipStream_t);                           \
  template hipError_t mmpl_launch_sampler_table<T, Step>(const SamplerPtrs<T>&, const Step*, int*, float*, const float*, int, int, \
                                                         hipStream_t);
MMPL_SAMPLER(bf16_t, MmplUniPCStep)
MMPL_SAMPLER(bf16_t, MmplDpmppStep)
MMPL_SAMPLER(float, MmplUniPCStepF32)
MMPL_SAMPLER(float, MmplDpmppStep)
#undef MMPL_SAMPLER
