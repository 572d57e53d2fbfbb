// Kernels of the TAEHV preview decoder ("Tiny AutoEncoder", demo_utils/taehv.py of the reference): a plain sequence of 3x3 / 1x1
// 2-D convolutions with ReLU on channels-last bf16 frames with a one-pixel zero border, fp32 accumulation on
// v_mfma_f32_16x16x32_bf16.
//
// One kernel serves all 35 convolutions.  It is the halo-tile implicit GEMM of the Wan VAE (conv_halo_kernel, vae_kernels.hip): a
// block owns an 8 x 32 pixel patch of one output frame, stages the patch's (8 + 2) x (32 + 2) halo in LDS 32 input channels at a time
// (planar: 16-byte channel chunk c of halo pixel p at c * HPLANE + p * 16, conflict-free for every tap shift) and the 9 taps read their
// A fragments from that image at constant offsets; the weights come fragment-major from global memory, one step ahead.  What this
// network adds:
//   * the K axis runs over TWO source frames (MemBlock's cat([x, past]) is never materialised: chunk c < C0 / 32 is staged from x,
//     the rest from past);
//   * nearest x2 up-sampling folded into the halo addressing (padded output pixel Y reads padded source pixel (Y + 1) >> 1, which
//     maps border to border), so an up-sampled frame never exists;
//   * epilogues: [+ bias] [+ skip] [ReLU], the skip value kept as the block's memory, and an output-channel -> frame split (TGrow);
//   * N tile 64 (4 fragments) for the 256 / 128 / 64-channel layers: the 64-channel levels, two thirds of the FLOPs, fill it exactly;
//     16 for the 3-channel head.
// Ragged sizes: the halo fetch clamps its coordinates into the padded frame, stores are predicated on the interior.
#include "common.h"
#include "kernels.h"
#include "taehv_kernels.h"

namespace {

constexpr int PH = 8, PW = 32, HH = PH + 2, HWD = PW + 2, HPIX = HH * HWD;   // 340 halo pixels
constexpr int HPLANE = 5632;              // bytes per channel-chunk plane: >= 340 * 16, a multiple of the 256-byte bank row
constexpr int NHALO = HPIX * 4;           // 16-byte chunks of one 32-channel halo image
constexpr int HLOADS = (NHALO + 255) / 256;

template <int NF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void taehv_conv_kernel(TaehvConvArgs g) {
  constexpr int BN = 16 * NF, MI = 4;
  __shared__ __attribute__((aligned(16))) char hsm[4 * HPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;   // wave w = patch rows 2w, 2w + 1 x all BN channels
  const int tiles_n = g.Nw / BN, npx = (g.Wo + PW - 1) / PW, npy = (g.Ho + PH - 1) / PH;
  const int tn = blockIdx.x % tiles_n;    // consecutive blocks: the N tiles of one patch (they share its halo in L2)
  int patch = blockIdx.x / tiles_n;
  const int x0 = (patch % npx) * PW; patch /= npx;
  const int y0 = (patch % npy) * PH;
  const int f = patch / npy;
  const int n0 = tn * BN;
  const int ntaps = g.ntaps, NJ = g.Nw >> 4;
  const int frow = lane & 15, fchunk = lane >> 4;

  int a_base[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_base[i] = fchunk * HPLANE + ((2 * wave + (i >> 1)) * HWD + (i & 1) * 16 + frow) * 16;
  f32x4 acc[MI][NF];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const bf16_t* wp = g.Wfrag + ((size_t)(n0 >> 4) * 64 + lane) * 8;
  auto load_w = [&](bf16x8 (&w)[NF], int chunk, int tap) {
    const bf16_t* p = wp + (size_t)(chunk * ntaps + min(tap, ntaps - 1)) * NJ * 512;
#pragma unroll
    for (int j = 0; j < NF; ++j) w[j] = *reinterpret_cast<const bf16x8*>(p + j * 512);
  };
  auto read_a = [&](bf16x8 (&a)[MI], int tap) {
    tap = ntaps == 1 ? 4 : min(tap, 8);   // a 1x1 conv is the centre tap
    const int tb = tap / 3, td = tap - 3 * tb;
    const char* Ac = hsm + (tb * HWD + td) * 16;
#pragma unroll
    for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Ac + a_base[i]);
  };
  auto mma = [&](const bf16x8 (&a)[MI], const bf16x8 (&w)[NF]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], a[i], acc[i][j], 0, 0, 0);
  };

  // the halo's source pixels: the same for every chunk of a source (both sources share the geometry)
  const int Hs = (g.up ? g.Ho >> 1 : g.Ho) + 2, Ws = (g.up ? g.Wo >> 1 : g.Wo) + 2;
  int hpix[HLOADS];
#pragma unroll
  for (int u = 0; u < HLOADS; ++u) {
    const int q = min(tid + 256 * u, NHALO - 1);      // (the surplus slots re-fetch the last chunk: no branches)
    const int hp = q >> 2, hy = hp / HWD, hx = hp - hy * HWD;
    int Y = min(y0 + hy, g.Ho + 1), X = min(x0 + hx, g.Wo + 1);
    if (g.up) { Y = (Y + 1) >> 1; X = (X + 1) >> 1; }
    hpix[u] = min(Y, Hs - 1) * Ws + min(X, Ws - 1);
  }
  const bf16_t* f0 = g.src0 + (size_t)f * g.fs0;
  const bf16_t* f1 = g.src1 ? g.src1 + (size_t)f * g.fs1 : f0;
  const int Ctot = g.C0 + g.C1;
#pragma unroll 1
  for (int c0 = 0; c0 < Ctot; c0 += 32) {
    const int chunk = c0 >> 5;
    const bool second = c0 >= g.C0;
    const bf16_t* fp = second ? f1 + (c0 - g.C0) : f0 + c0;
    const int C = second ? g.C1 : g.C0;
    bf16x8 w0[NF], w1[NF], a0[MI], a1[MI];
    load_w(w0, chunk, 0);
    if (c0) __syncthreads();                          // everybody is done reading the previous chunk's halo
    u32x4 hv[HLOADS];
#pragma unroll
    for (int u = 0; u < HLOADS; ++u) {
      const int q = min(tid + 256 * u, NHALO - 1);
      hv[u] = *reinterpret_cast<const u32x4*>(fp + (size_t)hpix[u] * C + (q & 3) * 8);
    }
#pragma unroll
    for (int u = 0; u < HLOADS; ++u) {
      const int q = min(tid + 256 * u, NHALO - 1);
      *reinterpret_cast<u32x4*>(hsm + (q & 3) * HPLANE + (q >> 2) * 16) = hv[u];
    }
    __syncthreads();
    read_a(a0, 0);
#pragma unroll 1
    for (int tap = 0; tap + 1 < ntaps; tap += 2) {    // ntaps = 9 | 1 (odd): the last tap is left in (a0, w0)
      load_w(w1, chunk, tap + 1); read_a(a1, tap + 1);
      __builtin_amdgcn_sched_barrier(0);
      mma(a0, w0);
      __builtin_amdgcn_sched_barrier(0);
      load_w(w0, chunk, tap + 2); read_a(a0, tap + 2);
      __builtin_amdgcn_sched_barrier(0);
      mma(a1, w1);
      __builtin_amdgcn_sched_barrier(0);
    }
    mma(a0, w0);
  }

  // ---- epilogue: lane = one output pixel x 4 consecutive output channels per fragment
  const int split = n0 / g.Nsplit, nd0 = n0 - split * g.Nsplit;       // the whole N tile lands in one destination frame
  bf16_t* dframe = g.dst + (size_t)(f * (g.Nw / g.Nsplit) + split) * g.fsd;
  const bool keep = g.keep != nullptr && f == g.T - 1;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int y = y0 + 2 * wave + (i >> 1), x = x0 + (i & 1) * 16 + frow;
    if (y >= g.Ho || x >= g.Wo) continue;
    const size_t pix = (size_t)(y + 1) * (g.Wo + 2) + (x + 1);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n = 16 * j + 4 * fchunk;             // within the tile
      if (n0 + n >= g.N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (g.bias) {
        const u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n0 + n);
        v[0] += bf2f(bb.x & 0xffff); v[1] += bf2f(bb.x >> 16); v[2] += bf2f(bb.y & 0xffff); v[3] += bf2f(bb.y >> 16);
      }
      if (g.skip) {
        const size_t so = pix * g.Nw + n0 + n;
        const u32x2 rr = *reinterpret_cast<const u32x2*>(g.skip + (size_t)f * g.fss + so);
        v[0] += bf2f(rr.x & 0xffff); v[1] += bf2f(rr.x >> 16); v[2] += bf2f(rr.y & 0xffff); v[3] += bf2f(rr.y >> 16);
        if (keep) *reinterpret_cast<u32x2*>(g.keep + so) = rr;
      }
      if (g.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      u32x2 o;
      o.x = pack2bf(v[0], v[1]);
      o.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<u32x2*>(dframe + pix * g.ldd + nd0 + n) = o;
    }
  }
}

__global__ void taehv_prep_kernel(const bf16_t* z, bf16_t* dst, int h, int w) {
  const int total = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int x = i % w, y = i / w;
    uint32_t o[8];
#pragma unroll
    for (int c = 0; c < 16; c += 2) {
      const float a = tanhf(bf2f(z[(size_t)c * total + i]) / 3.0f) * 3.0f;
      const float b = tanhf(bf2f(z[(size_t)(c + 1) * total + i]) / 3.0f) * 3.0f;
      o[c >> 1] = pack2bf(a, b);
    }
    u32x4* dp = reinterpret_cast<u32x4*>(dst + ((size_t)(y + 1) * (w + 2) + (x + 1)) * 32);
    dp[0] = u32x4{o[0], o[1], o[2], o[3]};
    dp[1] = u32x4{o[4], o[5], o[6], o[7]};
  }
}

__device__ __forceinline__ uint32_t taehv_u8(uint32_t bits) {
  const float v = fminf(1.f, fmaxf(0.f, bf2f((bf16_t)bits))) * 255.0f;
  return (uint32_t)v;
}

// one thread = one pixel: 8 bytes in; three floats (planar) or three bytes out
__global__ void taehv_px_out_kernel(const bf16_t* src, void* out, int fmt, int T, int H, int W, int t_out) {
  const long hw = (long)H * W, total = (long)T * hw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i / hw);
    const long p = i - (long)t * hw;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const u32x2 u = *reinterpret_cast<const u32x2*>(src + (((size_t)t * (H + 2) + (y + 1)) * (W + 2) + (x + 1)) * 4);
    if (fmt == 0) {
      float* o = (float*)out + (size_t)(t + t_out) * 3 * hw + p;
      o[0] = bf2f(u.x & 0xffff); o[hw] = bf2f(u.x >> 16); o[2 * hw] = bf2f(u.y & 0xffff);
    } else {
      unsigned char* o = (unsigned char*)out + ((size_t)(t + t_out) * hw + p) * 3;
      o[0] = (unsigned char)taehv_u8(u.x & 0xffff); o[1] = (unsigned char)taehv_u8(u.x >> 16); o[2] = (unsigned char)taehv_u8(u.y & 0xffff);
    }
  }
}

inline int grid_for(long n) {
  const long g = (n + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g == 0 ? 1 : g));
}

}  // namespace

hipError_t taehv_launch_conv(const TaehvConvArgs& g, hipStream_t s) {
  const int BN = g.Nw % 64 == 0 ? 64 : 16;
  if (g.T < 1 || g.Ho < 1 || g.Wo < 1 || (g.ntaps != 9 && g.ntaps != 1) || g.C0 < 32 || g.C0 % 32 || g.C1 % 32 || (g.C1 && !g.src1) ||
      g.Nw % BN || g.Nsplit % BN || g.Nw % g.Nsplit || g.N % 4 || g.N > g.Nw || g.ldd % 4 || (g.up && ((g.Ho | g.Wo) & 1)) ||
      (g.skip && g.N != g.Nw))
    return hipErrorInvalidValue;
  const long blocks = (long)(g.Nw / BN) * ((g.Wo + PW - 1) / PW) * ((g.Ho + PH - 1) / PH) * g.T;
  if (BN == 64) hipLaunchKernelGGL(taehv_conv_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, g);
  else hipLaunchKernelGGL(taehv_conv_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t taehv_launch_prep(const bf16_t* z, bf16_t* dst, int h, int w, hipStream_t s) {
  hipLaunchKernelGGL(taehv_prep_kernel, dim3(grid_for((long)h * w)), dim3(256), 0, s, z, dst, h, w);
  return hipGetLastError();
}

hipError_t taehv_launch_px_out(const bf16_t* src, void* out, int fmt, int T, int H, int W, int t_out, hipStream_t s) {
  hipLaunchKernelGGL(taehv_px_out_kernel, dim3(grid_for((long)T * H * W)), dim3(256), 0, s, src, out, fmt, T, H, W, t_out);
  return hipGetLastError();
}
