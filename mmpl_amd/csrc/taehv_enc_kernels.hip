// Kernels of the TAEHV ENCODER (the reference's demo_utils/taehv.py, TAEHV.encoder) that the decoder's taehv_conv_kernel cannot
// serve: the input layer, the stride-2 3x3 convolution and the latent output.  Everything else of the encoder (TPool's 1x1 convs,
// the MemBlocks, the 16-channel head) runs on taehv_launch_conv.  Same conventions as taehv_kernels.hip: padded channels-last bf16
// frames with a one-pixel zero border, v_mfma_f32_16x16x32_bf16 with the weights as the first operand (lane = 16 * k chunk + output
// row) and the pixels as the second (lane = 16 * k chunk + pixel), fp32 accumulation, one bf16 rounding per layer.
//
// taehv_conv_in_kernel: pixels -> conv 3->64 3x3 + bias + ReLU.  The 27 (tap, channel) products are ONE 32-wide K chunk,
//   k = (3 ky + kx) * 3 + c, k >= 27 zero, so a 16-pixel x 16-channel fragment is one MFMA.  A block owns an 8 x 32 pixel patch: it
//   stages the patch's 10 x 34 halo from the caller's pixels (float32 planar or uint8 interleaved) as bf16 [10][34][4] in LDS, zero
//   where the conv's padding lies, and every lane gathers its 8 k values per fragment from there with 2-byte reads.  The layer is
//   bound by its 128 bytes of output per pixel, not by that gather.
//
// taehv_conv_s2_kernel: 3x3 stride-2 conv, no bias: output (y, x) reads padded input rows 2y .. 2y + 2, columns 2x .. 2x + 2.  A
//   block owns an 8 x 16 patch of one output frame and stages its 17 x 33 input halo 32 channels at a time.  Output pixels that are
//   neighbours in x read input columns two apart, so the halo is kept in TWO column planes per 8-channel chunk: even input columns
//   in one, odd ones in the other, 16 bytes per pixel, row pitch 17.  Tap kx then reads plane kx & 1 at column index x + (kx >> 1):
//   the 16 pixels of a fragment are 16 consecutive 16-byte slots again, and with the chunk planes a multiple of 256 bytes apart every
//   16-lane group of a ds_read_b128 covers all 64 banks once -- conflict-free for all nine taps, as in taehv_conv_kernel.
//   LDS: 4 x 9472 = 37888 bytes per block, four blocks per CU.
//
// taehv_z_out_kernel: head frames [h + 2][w + 2][16] -> planar bf16 [16, h, w] per frame: the mirror of taehv_prep_kernel.
#include "common.h"
#include "kernels.h"
#include "taehv_kernels.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- input layer
constexpr int IPH = 8, IPW = 32, IHH = IPH + 2, IHW = IPW + 2;

__global__ __launch_bounds__(256) void taehv_conv_in_kernel(TaehvConvInArgs g) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[IHH * IHW * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npx = (g.W + IPW - 1) / IPW, npy = (g.H + IPH - 1) / IPH;
  int patch = blockIdx.x;
  const int x0 = (patch % npx) * IPW; patch /= npx;
  const int y0 = (patch % npy) * IPH;
  const int f = patch / npy;
  const int frow = lane & 15, fchunk = lane >> 4;
  const size_t hw = (size_t)g.H * g.W;

  for (int e = tid; e < IHH * IHW * 3; e += 256) {
    int c, hp;
    if (g.fmt == 0) { c = e / (IHH * IHW); hp = e - c * (IHH * IHW); }      // planar source: x fastest
    else { hp = e / 3; c = e - 3 * hp; }                                    // interleaved source: channel fastest
    const int hy = hp / IHW, hx = hp - hy * IHW;
    const int Y = y0 + hy - 1, X = x0 + hx - 1;
    float v = 0.f;
    if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
      if (g.fmt == 0) v = ((const float*)g.px)[((size_t)f * 3 + c) * hw + (size_t)Y * g.W + X];
      else v = __fdiv_rn((float)((const unsigned char*)g.px)[((size_t)f * hw + (size_t)Y * g.W + X) * 3 + c], 255.0f);
    }
    tile[hp * 4 + c] = f2bf(v);
  }

  bf16x8 w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const bf16x8*>(g.Wfrag + ((size_t)j * 64 + lane) * 8);
  int off[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = fchunk * 8 + e, tap = k / 3, c = k - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
    off[e] = k < 27 ? (ky * IHW + kx) * 4 + c : 0;                         // k >= 27 (chunk 3, e >= 3): read anything, use zero
  }
  __syncthreads();

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int base = ((2 * wave + (i >> 1)) * IHW + (i & 1) * 16 + frow) * 4;
    bf16x8 a;
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = fchunk * 8 + e < 27 ? (short)tile[base + off[e]] : (short)0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], a, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }

  bf16_t* dframe = g.dst + (size_t)f * g.fsd;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + 2 * wave + (i >> 1), x = x0 + (i & 1) * 16 + frow;
    if (y >= g.H || x >= g.W) continue;
    const size_t pix = (size_t)(y + 1) * (g.W + 2) + (x + 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = 16 * j + 4 * fchunk;
      const u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n);
      u32x2 o;
      o.x = pack2bf(fmaxf(acc[i][j][0] + bf2f(bb.x & 0xffff), 0.f), fmaxf(acc[i][j][1] + bf2f(bb.x >> 16), 0.f));
      o.y = pack2bf(fmaxf(acc[i][j][2] + bf2f(bb.y & 0xffff), 0.f), fmaxf(acc[i][j][3] + bf2f(bb.y >> 16), 0.f));
      *reinterpret_cast<u32x2*>(dframe + pix * 64 + n) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ stride-2 3x3 conv
constexpr int SPH = 8, SPW = 16, SHR = 2 * SPH + 1, SHC = 2 * SPW + 1, SPIX = SHR * SHC;   // 17 x 33 = 561 halo pixels
constexpr int SPITCH = SPW + 1;                  // pixels per plane row: 17 even columns (16 odd ones)
constexpr int SPPL = SHR * SPITCH * 16;          // 4624 bytes per column-parity plane
constexpr int SCPL = 9472;                       // bytes per 8-channel chunk: >= 2 * SPPL, a multiple of the 256-byte bank row
constexpr int SNH = SPIX * 4;                    // 16-byte chunks of one 32-channel halo image
constexpr int SLOADS = (SNH + 255) / 256;
static_assert(SCPL >= 2 * SPPL && SCPL % 256 == 0, "chunk plane");

__global__ __launch_bounds__(256) void taehv_conv_s2_kernel(TaehvConvS2Args g) {
  constexpr int MI = 2, NF = 4;
  __shared__ __attribute__((aligned(16))) char hsm[4 * SCPL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;   // wave w = patch rows 2w, 2w + 1 x 64 channels
  const int tiles_n = g.Nw / 64, npx = (g.Wo + SPW - 1) / SPW, npy = (g.Ho + SPH - 1) / SPH;
  const int tn = blockIdx.x % tiles_n;
  int patch = blockIdx.x / tiles_n;
  const int x0 = (patch % npx) * SPW; patch /= npx;
  const int y0 = (patch % npy) * SPH;
  const int f = patch / npy;
  const int n0 = tn * 64, NJ = g.Nw >> 4;
  const int frow = lane & 15, fchunk = lane >> 4;

  int a_base[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_base[i] = fchunk * SCPL + (2 * (2 * wave + i) * SPITCH + frow) * 16;
  f32x4 acc[MI][NF];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the halo's source pixels and LDS slots: the same for every channel chunk
  const int Hs = 2 * g.Ho + 2, Ws = 2 * g.Wo + 2;
  int hpix[SLOADS], hdst[SLOADS];
#pragma unroll
  for (int u = 0; u < SLOADS; ++u) {
    const int q = min(tid + 256 * u, SNH - 1);        // (the surplus slots re-fetch the last chunk: no branches)
    const int hp = q >> 2, hy = hp / SHC, hx = hp - hy * SHC;
    hpix[u] = min(2 * y0 + hy, Hs - 1) * Ws + min(2 * x0 + hx, Ws - 1);
    hdst[u] = (q & 3) * SCPL + (hx & 1) * SPPL + (hy * SPITCH + (hx >> 1)) * 16;
  }
  const bf16_t* fp = g.src + (size_t)f * g.fs;
  const bf16_t* wp = g.Wfrag + ((size_t)(n0 >> 4) * 64 + lane) * 8;
#pragma unroll 1
  for (int c0 = 0; c0 < g.C; c0 += 32) {
    if (c0) __syncthreads();                          // everybody is done reading the previous chunk's halo
    u32x4 hv[SLOADS];
#pragma unroll
    for (int u = 0; u < SLOADS; ++u) {
      const int q = min(tid + 256 * u, SNH - 1);
      hv[u] = *reinterpret_cast<const u32x4*>(fp + (size_t)hpix[u] * g.C + c0 + (q & 3) * 8);
    }
#pragma unroll
    for (int u = 0; u < SLOADS; ++u) *reinterpret_cast<u32x4*>(hsm + hdst[u]) = hv[u];
    __syncthreads();
    const bf16_t* wc = wp + (size_t)(c0 >> 5) * 9 * NJ * 512;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const char* Ac = hsm + (kx & 1) * SPPL + (ky * SPITCH + (kx >> 1)) * 16;
      bf16x8 w[NF], a[MI];
#pragma unroll
      for (int j = 0; j < NF; ++j) w[j] = *reinterpret_cast<const bf16x8*>(wc + (size_t)tap * NJ * 512 + j * 512);
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Ac + a_base[i]);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], a[i], acc[i][j], 0, 0, 0);
    }
  }

  bf16_t* dframe = g.dst + (size_t)f * g.fsd;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int y = y0 + 2 * wave + i, x = x0 + frow;
    if (y >= g.Ho || x >= g.Wo) continue;
    const size_t pix = (size_t)(y + 1) * (g.Wo + 2) + (x + 1);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n = n0 + 16 * j + 4 * fchunk;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (g.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      u32x2 o;
      o.x = pack2bf(v[0], v[1]);
      o.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<u32x2*>(dframe + pix * g.Nw + n) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- latent out
// one thread = one pixel: 32 bytes in, 16 planar bf16 out
__global__ void taehv_z_out_kernel(const bf16_t* src, bf16_t* out, int T, int h, int w, int f_out) {
  const long hw = (long)h * w, total = (long)T * hw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i / hw);
    const long p = i - (long)t * hw;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    const u32x4* sp = reinterpret_cast<const u32x4*>(src + (((size_t)t * (h + 2) + (y + 1)) * (w + 2) + (x + 1)) * 16);
    const u32x4 lo = sp[0], hi = sp[1];
    const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    bf16_t* o = out + (size_t)(t + f_out) * 16 * hw + p;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      o[(size_t)(2 * c) * hw] = (bf16_t)(v[c] & 0xffff);
      o[(size_t)(2 * c + 1) * hw] = (bf16_t)(v[c] >> 16);
    }
  }
}

}  // namespace

hipError_t taehv_launch_conv_in(const TaehvConvInArgs& g, hipStream_t s) {
  if (g.T < 1 || g.H < 1 || g.W < 1 || (g.fmt != 0 && g.fmt != 1) || !g.px || !g.Wfrag || !g.bias || !g.dst) return hipErrorInvalidValue;
  const long blocks = (long)((g.W + IPW - 1) / IPW) * ((g.H + IPH - 1) / IPH) * g.T;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(taehv_conv_in_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t taehv_launch_conv_s2(const TaehvConvS2Args& g, hipStream_t s) {
  if (g.T < 1 || g.Ho < 1 || g.Wo < 1 || g.C < 32 || g.C % 32 || g.Nw < 64 || g.Nw % 64 || !g.src || !g.Wfrag || !g.dst)
    return hipErrorInvalidValue;
  const long blocks = (long)(g.Nw / 64) * ((g.Wo + SPW - 1) / SPW) * ((g.Ho + SPH - 1) / SPH) * g.T;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(taehv_conv_s2_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t taehv_launch_z_out(const bf16_t* src, bf16_t* out, int T, int h, int w, int f_out, hipStream_t s) {
  const long g = ((long)T * h * w + 255) / 256;
  hipLaunchKernelGGL(taehv_z_out_kernel, dim3((unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g))), dim3(256), 0, s, src, out, T, h, w, f_out);
  return hipGetLastError();
}
