// Kernels of the Wan 3D causal VAE (decode + encode) on channels-last bf16 volumes.
//
// Every CausalConv3d / Conv2d is an implicit GEMM straight out of a zero-bordered ("padded") channels-last
// volume: output pixel m -> a base pixel in the padded source, each filter tap is a constant pixel offset from it, and
// the K axis is (tap, cin) with cin contiguous -- so the A operand rows are plain 64-byte runs of HBM and no im2col
// buffer ever exists.  The temporal "feat_cache" of the reference (vae.py:14, 207-216) is the first two time slots of
// each conv's persistent padded volume.  Tile 128x128x32, 4 waves, v_mfma_f32_16x16x32_bf16, XOR-swizzled LDS,
// register-staged double buffering (same structure as gemm.hip).  The norm / activation / resampling passes between
// convs are HBM-bound 16-byte-per-lane kernels that write directly into the next conv's padded volume.
#include "common.h"
#include "kernels.h"
#include "mmpl_config.h"
#include "vae_kernels.h"

namespace {

constexpr int BM = 128, BK = 32;        // the N tile is a template parameter of conv_igemm_kernel
constexpr int TILE_BYTES = BM * BK * 2;  // 8 KiB

// swizzled byte offset of 16-B chunk c (0..3) of row r inside a [128][32] bf16 tile: chunk' = c ^ ((-(r>>2)) & 3)
MMPL_DEV int swz(int r, int c) { return r * 64 + ((c ^ ((0 - (r >> 2)) & 3)) << 4); }

// NF = 16-column fragments per wave along N: 4 -> a 128-wide N tile, 3 -> 96-wide (the C = 96 layers of the decoder's full-resolution
// stage, 40 % of a decode's conv time, would otherwise multiply 32 padding columns per tile)
template <int NF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void conv_igemm_kernel(ConvArgs g) {
  constexpr int BN = 32 * NF;
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
  char* As = smem;
  char* Ws = smem + 2 * TILE_BYTES;
  const int tiles_m = (g.M + BM - 1) / BM;
  const int tm = blockIdx.x % tiles_m, tn = blockIdx.x / tiles_m;   // consecutive blocks share the weight panel
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // staging roles: 128 rows x 4 chunks = 512 chunks per operand -> 2 per thread
  const int srow = tid >> 2, schunk = tid & 3;
  const int K = g.ntaps * g.Cin;
  size_t a_base[2];
  const bf16_t* w_ptr[2];
  int lds_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = srow + 64 * j;
    const int m = min(m0 + row, g.M - 1);
    const int x = m % g.Wo, y = (m / g.Wo) % g.Ho, t = m / (g.Wo * g.Ho);
    a_base[j] = ((size_t)(t * g.st) * g.Hp + (size_t)y * g.sy) * g.Wp + (size_t)x * g.sx;   // pixel index
    w_ptr[j] = g.W + (size_t)min(n0 + row, g.N - 1) * K + schunk * 8;
    lds_off[j] = swz(row, schunk);
  }
  const int nt = K / BK;
  const int tiles_per_tap = g.Cin / BK;
  u32x4 ra[2], rw[2];
  auto load = [&](int t) {
    const int tap = t / tiles_per_tap, c0 = (t - tap * tiles_per_tap) * BK;
    const int toff = g.tap_off[tap];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ra[j] = *reinterpret_cast<const u32x4*>(g.src + (a_base[j] + toff) * g.Cin + c0 + schunk * 8);
      rw[j] = *reinterpret_cast<const u32x4*>(w_ptr[j] + (size_t)t * BK);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<u32x4*>(As + buf * TILE_BYTES + lds_off[j]) = ra[j];
      *reinterpret_cast<u32x4*>(Ws + buf * TILE_BYTES + lds_off[j]) = rw[j];
    }
  };
  load(0);
  store(0);
  __syncthreads();

  f32x4 acc[4][NF];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fchunk = lane >> 4;
  int a_off[4], w_off[NF];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_off[i] = swz(64 * wm + 16 * i + frow, fchunk);
#pragma unroll
  for (int j = 0; j < NF; ++j) w_off[j] = swz(16 * NF * wn + 16 * j + frow, fchunk);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) load(t + 1);
    const char* Ac = As + cur * TILE_BYTES;
    const char* Wc = Ws + cur * TILE_BYTES;
    bf16x8 af[4], wf[NF];
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const bf16x8*>(Ac + a_off[i]);
#pragma unroll
    for (int j = 0; j < NF; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(Wc + w_off[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    if (t + 1 < nt) store(cur ^ 1);
    __syncthreads();
  }
  // epilogue: lane holds column m (one output pixel) x 4 consecutive output channels per fragment
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 64 * wm + 16 * i + frow;
    if (m >= g.M) continue;
    const int x = m % g.Wo, y = (m / g.Wo) % g.Ho, t = m / (g.Wo * g.Ho);
    const size_t dpix = ((size_t)(t + g.dt0) * g.Hd + (y + g.dy0)) * g.Wd + (x + g.dx0);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int n = n0 + 16 * NF * wn + 16 * j + 4 * fchunk;
      if (n >= g.N) continue;
      float v[4];
      const u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n);
      v[0] = rbf(acc[i][j][0] + bf2f(bb.x & 0xffff)); v[1] = rbf(acc[i][j][1] + bf2f(bb.x >> 16));
      v[2] = rbf(acc[i][j][2] + bf2f(bb.y & 0xffff)); v[3] = rbf(acc[i][j][3] + bf2f(bb.y >> 16));
      if (g.res) {
        const u32x2 rr = *reinterpret_cast<const u32x2*>(g.res + (size_t)m * g.ldres + n);
        v[0] += bf2f(rr.x & 0xffff); v[1] += bf2f(rr.x >> 16); v[2] += bf2f(rr.y & 0xffff); v[3] += bf2f(rr.y >> 16);
      }
      u32x2 o;
      o.x = pack2bf(v[0], v[1]);
      o.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<u32x2*>(g.dst + dpix * g.ldd + g.dc0 + n) = o;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 3x3 (x kt) convolutions with stride 1 -- every ResidualBlock conv, the upsamplers' Conv2d, the heads: 93 % of a decode's FLOPs.
// conv_igemm_kernel re-reads every input pixel once per filter tap (the A operand of tap (a, b, d) is the tile's pixels shifted by
// one row / column / frame): at N = 96 that is 55 FLOP per byte brought into the CU, 19 GB of L2 -> register traffic per C = 96
// launch, and the kernel sat at 600-640 TFLOP/s bound by operand delivery, not by its MFMAs.  Here a block
// owns a SPATIAL patch of one output frame (8 rows x 32 columns = 256 pixels = 16 MFMA row fragments) and stages the patch's halo
// -- (8 + 2) x (32 + 2) pixels of each of the kt source frames, 32 input channels at a time -- in LDS ONCE; the 9 kt taps then read
// their A fragments from that one image at constant byte offsets ((a * 10 + b) * 34 + d pixels).  An input pixel is fetched
// 1.33 times per 32-channel chunk instead of 9 kt times: 6.8x (kt = 1) / 20x (kt = 3) less operand traffic per MFMA.  The small
// weight slice of a (tap, chunk) step never touches LDS: the host packs the weights fragment-major (ConvArgs.Wfrag) and every wave
// loads its 16 x 32 fragments with one coalesced 1 KiB load each, one step ahead -- L1 serves the block's other three waves.
// 4 waves, wave w = patch rows 2w, 2w + 1 x all BN channels; two blocks per CU (64 KiB LDS, 96 accumulator registers each), so one
// block's halo fetch runs under the other's MFMAs.
// LDS image: PLANAR -- 16-byte channel chunk c of halo pixel p (frame-major, then row, then column) at c * 16 KiB + p * 16.  A
// fragment read (16 consecutive pixels per 16-lane group, the four chunks on the four lane groups) then touches 16 consecutive
// 16-byte slots per ds_read_b128 service group whatever the tap's shift: conflict-free.  (Pixel-major -- 64 B per pixel -- is
// 2-way conflicted for every shift and no in-pixel swizzle repairs it: the service groups mix chunk c of pixels 0-3, 12-15 with
// chunk c + 1 of pixels 4-11.)
constexpr int PH = 8, PW = 32, HH = PH + 2, HWD = PW + 2, HPIX = HH * HWD;     // 340 halo pixels per frame
constexpr int HPLANE = 16384;               // bytes per channel-chunk plane (>= 3 * 340 * 16, a multiple of the 256-byte bank row)

template <int NF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_halo_kernel(ConvArgs g) {
  constexpr int BN = 16 * NF;
  // wave grid 4 x 1: wave w = patch rows 2w, 2w + 1 (64 pixels = 4 row fragments) x all BN channels.  (2 x 2 -- 128 pixels x BN / 2
  // per wave, half the weight loads per MFMA -- measured 3 % slower: profiles/r03m.)
  constexpr int WN = 1, WM = 4 / WN, MI = 16 / WM, NJ_W = NF / WN, ROWS_W = PH / WM;
  extern __shared__ __attribute__((aligned(16))) char hsm[];   // [4 chunk planes][kt * 340 pixels][16 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (g.N + BN - 1) / BN, npx = (g.Wo + PW - 1) / PW, npy = (g.Ho + PH - 1) / PH;
  const int tn = blockIdx.x % tiles_n;          // consecutive blocks: the N tiles of one patch (they share its halo in L2)
  int patch = blockIdx.x / tiles_n;
  const int x0 = (patch % npx) * PW; patch /= npx;
  const int y0 = (patch % npy) * PH;
  const int t0 = patch / npy;
  const int n0 = tn * BN + 16 * NJ_W * wn;      // this wave's first output channel
  const int kt = g.kt, ntaps = g.ntaps, NJ = (g.N + 15) >> 4;

  const int frow = lane & 15, fchunk = lane >> 4;
  int a_base[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_base[i] = fchunk * HPLANE + ((ROWS_W * wm + (i >> 1)) * HWD + (i & 1) * 16 + frow) * 16;

  f32x4 acc[MI][NJ_W];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ_W; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // weight fragments straight from global memory (host-packed: one contiguous 1 KiB wave load per 16 x 32 fragment) and A
  // fragments from the halo image, both one (tap) step ahead of the MFMAs that use them.  Nothing in a chunk phase writes LDS,
  // so the tap loop has no barrier: the 4 waves (and the CU's second block) drift freely and cover each other's latencies.
  const bf16_t* wp = g.Wfrag + ((size_t)(n0 >> 4) * 64 + lane) * 8;
  auto load_w = [&](bf16x8 (&w)[NJ_W], int chunk, int tap) {
    const bf16_t* p = wp + (size_t)(chunk * ntaps + min(tap, ntaps - 1)) * NJ * 512;
#pragma unroll
    for (int j = 0; j < NJ_W; ++j) w[j] = *reinterpret_cast<const bf16x8*>(p + j * 512);
  };
  auto read_a = [&](bf16x8 (&a)[MI], int tap) {
    tap = min(tap, ntaps - 1);
    const int ta = tap / 9, bd = tap - 9 * ta, tb = bd / 3, td = bd - 3 * tb;
    const char* Ac = hsm + ((ta * HH + tb) * HWD + td) * 16;
#pragma unroll
    for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(Ac + a_base[i]);
  };
  auto mma = [&](const bf16x8 (&a)[MI], const bf16x8 (&w)[NJ_W]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ_W; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], a[i], acc[i][j], 0, 0, 0);
  };

  const int nhalo = kt * HPIX * 4;              // 16-byte chunks of the halo image
  // the kt source frames of this output frame: consecutive frames of the volume, or (ring mode) whatever slots the host names
  const size_t fstride = (size_t)g.Hp * g.Wp * g.Cin;
  const bool ring = g.frame[0] != nullptr;
  const bf16_t* fp0 = ring ? g.frame[t0] : g.src + (size_t)t0 * fstride;
  const bf16_t* fp1 = ring ? g.frame[t0 + (kt > 1 ? 1 : 0)] : fp0 + fstride;
  const bf16_t* fp2 = ring ? g.frame[t0 + (kt > 2 ? 2 : 0)] : fp0 + 2 * fstride;
#pragma unroll 1
  for (int c0 = 0; c0 < g.Cin; c0 += 32) {
    const int chunk = c0 >> 5;
    bf16x8 w0[NJ_W], w1[NJ_W], a0[MI], a1[MI];
    load_w(w0, chunk, 0);
    if (c0) __syncthreads();                    // everybody is done reading the previous chunk's halo
    // ---- halo of this 32-channel chunk: up to 16 chunks of 16 B per thread, in two batches of 8 loads in flight
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 hv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = min(tid + 256 * (8 * h + u), nhalo - 1);     // (kt = 1: the surplus slots re-fetch the last chunk -- no branches)
        const int hp = q >> 2, f = hp / HPIX, r = hp - f * HPIX, hy = r / HWD, hx = r - hy * HWD;
        const size_t pix = (size_t)min(y0 + hy, g.Hp - 1) * g.Wp + min(x0 + hx, g.Wp - 1);
        const bf16_t* fp = f == 0 ? fp0 : (f == 1 ? fp1 : fp2);
        hv[u] = *reinterpret_cast<const u32x4*>(fp + pix * g.Cin + c0 + (q & 3) * 8);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = min(tid + 256 * (8 * h + u), nhalo - 1);
        *reinterpret_cast<u32x4*>(hsm + (q & 3) * HPLANE + (q >> 2) * 16) = hv[u];
      }
    }
    __syncthreads();
    read_a(a0, 0);
#pragma unroll 1
    for (int tap = 0; tap + 1 < ntaps; tap += 2) {   // ntaps = 9 | 27 (odd): the last tap is left in (a0, w0)
      // (the scheduling barriers pin "next step's loads first, then this step's 24 MFMAs": left alone, hipcc sinks the loads to
      // half a step before their use and the wave waits on L2 latency every step)
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
  // ---- epilogue with the consumer's RMS_norm + SiLU fused (N == 96: this block holds every channel of its pixels; a pixel's 96
  // values sit in the 4 lanes frow, frow + 16, frow + 32, frow + 48).  Same arithmetic and rounding points as norm_act_pad_kernel on
  // the bf16 value this conv stores (vae.py:51-54: x / clamp(bf16(||x||), 1e-12), * sqrt(C), * gamma, each a bf16 tensor; then SiLU);
  // only the order of the fp32 sum of squares differs.  The norm pass it replaces re-read the plain output from HBM and was
  // VALU-bound; here the same VALU work runs under the CU's other block's MFMAs.
  if constexpr (NF == 6) {
    if (g.ngamma) {
      float gm[NJ_W][4];
#pragma unroll
      for (int j = 0; j < NJ_W; ++j) {
        const u32x2 gg = *reinterpret_cast<const u32x2*>(g.ngamma + n0 + 16 * j + 4 * fchunk);
        gm[j][0] = bf2f(gg.x & 0xffff); gm[j][1] = bf2f(gg.x >> 16); gm[j][2] = bf2f(gg.y & 0xffff); gm[j][3] = bf2f(gg.y >> 16);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int y = y0 + ROWS_W * wm + (i >> 1), x = x0 + (i & 1) * 16 + frow;
        const bool live = y < g.Ho && x < g.Wo;
        const size_t m = ((size_t)t0 * g.Ho + min(y, g.Ho - 1)) * g.Wo + min(x, g.Wo - 1);
        float v[NJ_W][4];
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NJ_W; ++j) {
          const int n = n0 + 16 * j + 4 * fchunk;
          const u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n);
          v[j][0] = rbf(acc[i][j][0] + bf2f(bb.x & 0xffff)); v[j][1] = rbf(acc[i][j][1] + bf2f(bb.x >> 16));
          v[j][2] = rbf(acc[i][j][2] + bf2f(bb.y & 0xffff)); v[j][3] = rbf(acc[i][j][3] + bf2f(bb.y >> 16));
          if (g.res) {
            const u32x2 rr = *reinterpret_cast<const u32x2*>(g.res + m * g.ldres + n);
            v[j][0] = rbf(v[j][0] + bf2f(rr.x & 0xffff)); v[j][1] = rbf(v[j][1] + bf2f(rr.x >> 16));
            v[j][2] = rbf(v[j][2] + bf2f(rr.y & 0xffff)); v[j][3] = rbf(v[j][3] + bf2f(rr.y >> 16));
          }
          if (g.dst && live) {
            const size_t dpix = ((size_t)(t0 + g.dt0) * g.Hd + (y + g.dy0)) * g.Wd + (x + g.dx0);
            u32x2 o;
            o.x = pack2bf(v[j][0], v[j][1]);
            o.y = pack2bf(v[j][2], v[j][3]);
            *reinterpret_cast<u32x2*>(g.dst + dpix * g.ldd + g.dc0 + n) = o;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) sq += v[j][e] * v[j][e];
        }
        sq += __shfl_xor(sq, 16, 64);
        sq += __shfl_xor(sq, 32, 64);
        const float denom = fmaxf(rbf(sqrtf(sq)), 1e-12f);
        float rden = __frcp_rn(denom);
        rden = fmaf(fmaf(-denom, rden, 1.f), rden, rden);
        if (!live) continue;
        bf16_t* np = g.nframe[t0] + ((size_t)(y + 1) * (g.Wo + 2) + (x + 1)) * g.N;
#pragma unroll
        for (int j = 0; j < NJ_W; ++j) {
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float q = v[j][e] * rden;
            q = fmaf(fmaf(-q, denom, v[j][e]), rden, q);      // the correctly rounded fp32 quotient (see norm_act_pad_kernel)
            float nv = rbf(q);
            nv = rbf(nv * g.nscale);
            nv = rbf(nv * gm[j][e]);
            o[e] = __fdividef(nv, 1.0f + __expf(-nv));
          }
          u32x2 w;
          w.x = pack2bf(o[0], o[1]);
          w.y = pack2bf(o[2], o[3]);
          *reinterpret_cast<u32x2*>(np + n0 + 16 * j + 4 * fchunk) = w;
        }
      }
      return;
    }
  }
  // ---- epilogue: lane = one output pixel x 4 consecutive output channels per fragment (conv_igemm_kernel's)
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int y = y0 + ROWS_W * wm + (i >> 1), x = x0 + (i & 1) * 16 + frow;
    if (y >= g.Ho || x >= g.Wo) continue;
    const size_t m = ((size_t)t0 * g.Ho + y) * g.Wo + x;
    const size_t dpix = ((size_t)(t0 + g.dt0) * g.Hd + (y + g.dy0)) * g.Wd + (x + g.dx0);
#pragma unroll
    for (int j = 0; j < NJ_W; ++j) {
      const int n = n0 + 16 * j + 4 * fchunk;
      if (n >= g.N) continue;
      float v[4];
      const u32x2 bb = *reinterpret_cast<const u32x2*>(g.bias + n);
      v[0] = rbf(acc[i][j][0] + bf2f(bb.x & 0xffff)); v[1] = rbf(acc[i][j][1] + bf2f(bb.x >> 16));
      v[2] = rbf(acc[i][j][2] + bf2f(bb.y & 0xffff)); v[3] = rbf(acc[i][j][3] + bf2f(bb.y >> 16));
      if (g.res) {
        const u32x2 rr = *reinterpret_cast<const u32x2*>(g.res + m * g.ldres + n);
        v[0] += bf2f(rr.x & 0xffff); v[1] += bf2f(rr.x >> 16); v[2] += bf2f(rr.y & 0xffff); v[3] += bf2f(rr.y >> 16);
      }
      u32x2 o;
      o.x = pack2bf(v[0], v[1]);
      o.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<u32x2*>(g.dst + dpix * g.ldd + g.dc0 + n) = o;
    }
  }
}

// ---- RMS_norm (F.normalize over C * sqrt(C) * gamma, vae.py:51-54) [+ SiLU] -> padded destination.  LG lanes per pixel, 16 bytes
// (8 channels) per lane per pass: LG = 16 for C <= 128, 32 for C <= 256, else the whole wave with up to two passes (C <= 1024) --
// so a wave normalises 4 / 2 / 1 pixels and every lane moves data (with one pixel per wave the C = 96 layers of the decoder's
// full-resolution stage kept 12 of 64 lanes busy and the kernel ran at a quarter of the HBM rate: 27 % of a decode).
#ifndef VAE_NORM_FASTDIV
#define VAE_NORM_FASTDIV 1      // dev: 0 = the compiler's division sequences (A/B of the VALU cost)
#endif
template <int LG>
__global__ __launch_bounds__(256) void norm_act_pad_kernel(NormArgs a) {
  // NB pixels per lane group and pass, all their loads issued before the first reduction: one 16-byte load per lane in flight
  // kept a CU at 32 KiB outstanding -- half of what HBM latency x bandwidth asks for (the kernel ran at 2.6 TB/s)
  constexpr int PPW = 64 / LG, NIT = LG == 64 ? 2 : 1, NB = LG == 64 ? 1 : 2;
  const int lane = threadIdx.x & 63, sub = lane % LG;
  const int nchunk = a.C >> 3;
  long pixb[NB];
  bool live[NB];
  float v[NB][NIT][8];
  float sq[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    pixb[b] = (((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * NB + b) * PPW + lane / LG;
    live[b] = pixb[b] < a.npix;
    const bf16_t* sp = a.src + (size_t)(live[b] ? pixb[b] : 0) * a.C;
    sq[b] = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int ch = sub + LG * it;
      u32x4 u = {0u, 0u, 0u, 0u};
      if (live[b] && ch < nchunk) u = *reinterpret_cast<const u32x4*>(sp + ch * 8);
      v[b][it][0] = bf2f(u.x & 0xffff); v[b][it][1] = bf2f(u.x >> 16); v[b][it][2] = bf2f(u.y & 0xffff); v[b][it][3] = bf2f(u.y >> 16);
      v[b][it][4] = bf2f(u.z & 0xffff); v[b][it][5] = bf2f(u.z >> 16); v[b][it][6] = bf2f(u.w & 0xffff); v[b][it][7] = bf2f(u.w >> 16);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int it = 0; it < NIT; ++it)
#pragma unroll
      for (int j = 0; j < 8; ++j) sq[b] += v[b][it][j] * v[b][it][j];
    float denom = 1.f, rden = 1.f;
    if (a.gamma) {
#pragma unroll
      for (int o = LG / 2; o > 0; o >>= 1) sq[b] += __shfl_xor(sq[b], o, 64);    // sum over the pixel's LG lanes
      denom = fmaxf(rbf(sqrtf(sq[b])), 1e-12f);                                  // torch.norm output is a bf16 tensor, clamp_min(eps)
      // x / denom for every channel of the pixel: one reciprocal per pixel (v_rcp + a Newton step), then per element the
      // quotient with its residual folded back -- q = x r; q += (x - q d) r -- which is the correctly rounded fp32 quotient the
      // reference's division produces (the compiler's own division sequence is ~10 VALU instructions per element, and this
      // kernel is VALU-bound: two divisions, three bf16 roundings and an exponential per element)
      rden = __frcp_rn(denom);
      rden = fmaf(fmaf(-denom, rden, 1.f), rden, rden);
    }
    if (!live[b]) continue;
    const long pix = pixb[b];
    const int x = (int)(pix % a.W), y = (int)((pix / a.W) % a.H), t = (int)(pix / ((long)a.W * a.H));
    bf16_t* dp = a.dst + (((size_t)(t + a.dt0) * a.Hd + (y + a.dy0)) * a.Wd + (x + a.dx0)) * a.ldd;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int ch = sub + LG * it;
      if (ch >= nchunk) continue;
      float o[8];
      if (a.gamma) {
        const u32x4 gu = *reinterpret_cast<const u32x4*>(a.gamma + ch * 8);
        const float gm[8] = {bf2f(gu.x & 0xffff), bf2f(gu.x >> 16), bf2f(gu.y & 0xffff), bf2f(gu.y >> 16),
                             bf2f(gu.z & 0xffff), bf2f(gu.z >> 16), bf2f(gu.w & 0xffff), bf2f(gu.w >> 16)};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#if VAE_NORM_FASTDIV
          float q = v[b][it][j] * rden;
          q = fmaf(fmaf(-q, denom, v[b][it][j]), rden, q);
          float n = rbf(q);                           // x / norm      (bf16 tensor)
          n = rbf(n * a.scale);                       // * sqrt(C)
          n = rbf(n * gm[j]);                         // * gamma
          o[j] = a.silu ? __fdividef(n, 1.0f + __expf(-n)) : n;      // (rounded to bf16 by the pack below)
#else
          float n = rbf(v[b][it][j] / denom);
          n = rbf(n * a.scale);
          n = rbf(n * gm[j]);
          o[j] = a.silu ? silu(n) : n;
#endif
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = v[b][it][j];
      }
      u32x4 w;
      w.x = pack2bf(o[0], o[1]); w.y = pack2bf(o[2], o[3]); w.z = pack2bf(o[4], o[5]); w.w = pack2bf(o[6], o[7]);
      *reinterpret_cast<u32x4*>(dp + ch * 8) = w;
    }
  }
}

// ---- nearest 2x spatial upsample (+ optional temporal de-interleave of a time_conv output [T,H,W,2C] -> frames
// 2t, 2t+1 taking channel halves, vae.py:134-137) into a padded destination.
__global__ void upsample_pad_kernel(UpArgs a) {
  const long nchunk_c = a.C >> 3;
  const long total = (long)a.To * (2 * a.H) * (2 * a.W) * nchunk_c;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % nchunk_c);
    long p = i / nchunk_c;
    const int X = (int)(p % (2 * a.W)); p /= (2 * a.W);
    const int Y = (int)(p % (2 * a.H));
    const int T = (int)(p / (2 * a.H));
    const int ts = a.interleave ? (T >> 1) : T, half = a.interleave ? (T & 1) : 0;
    const bf16_t* sp = a.src + (((size_t)ts * a.H + (Y >> 1)) * a.W + (X >> 1)) * a.lds + half * a.C + c * 8;
    bf16_t* dp = a.dst + (((size_t)T * a.Hd + (Y + 1)) * a.Wd + (X + 1)) * a.C + c * 8;
    *reinterpret_cast<u32x4*>(dp) = *reinterpret_cast<const u32x4*>(sp);
  }
}

// ---- z prep: latent [F,16,h,w] -> (z / inv_std + mean) -> conv2 (1x1x1, 16->16) -> decoder.conv1's padded volume
// (channels padded 16 -> 32 with zeros).   vae.py:548-554
__global__ void z_prep_kernel(ZPrepArgs a) {
  const long total = (long)a.F * a.h * a.w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % a.w), y = (int)((i / a.w) % a.h), f = (int)(i / ((long)a.w * a.h));
    float z[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const float v = bf2f(a.z[(((size_t)f * 16 + c) * a.h + y) * a.w + x]);
      z[c] = rbf(rbf(v / a.inv_std[c]) + a.mean[c]);
    }
    bf16_t* dp = a.dst + (((size_t)(f + a.dt0) * (a.h + 2) + (y + 1)) * (a.w + 2) + (x + 1)) * 32;
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) acc += z[c] * bf2f(a.w2[o * 16 + c]);
      dp[o] = f2bf(acc + bf2f(a.b2[o]));
    }
  }
}

// ---- head output [T,H,W,4] bf16 -> float32 [T,3,H,W] (frame offset t_out), clamp(-1,1)   wan_wrapper.py:108
__global__ void px_out_kernel(const bf16_t* src, float* out, int T, int H, int W, int t_out) {
  const long total = (long)T * H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long hw = (long)H * W;
    const int t = (int)(i / hw);
    const long p = i - (long)t * hw;
    const u32x2 u = *reinterpret_cast<const u32x2*>(src + i * 4);
    const float v[3] = {bf2f(u.x & 0xffff), bf2f(u.x >> 16), bf2f(u.y & 0xffff)};
#pragma unroll
    for (int c = 0; c < 3; ++c) out[((size_t)(t + t_out) * 3 + c) * hw + p] = fminf(1.f, fmaxf(-1.f, v[c]));
  }
}

// ---- head output [T,H,W,4] bf16 -> uint8 [T,H,W,3] (frame offset t_out): the float path's clamp(-1,1), then what the pipeline and
// the CLI do to those frames in PyTorch, (x * 0.5 + 0.5).clamp(0, 1) and (v * 255.0).clamp(0, 255).to(uint8), in the same fp32
// operations, order and rounding (multiply and add kept apart), truncated.  One lane = 4 consecutive pixels: two 16-byte loads, 12
// bytes out as three dwords (W is a multiple of 8, so a group never straddles a row and starts 4-byte aligned).
__device__ __forceinline__ uint32_t px_u8(uint32_t bits) {
#pragma clang fp contract(off)
  float v = fminf(1.f, fmaxf(-1.f, bf2f(bits)));
  v = v * 0.5f;
  v = v + 0.5f;
  v = fminf(1.f, fmaxf(0.f, v));
  v = v * 255.0f;
  v = fminf(255.f, fmaxf(0.f, v));
  return (uint32_t)v;
}

__global__ void px_out_u8_kernel(const bf16_t* src, unsigned char* out, int T, int H, int W, int t_out) {
  const long hw = (long)H * W;
  const long groups = (long)T * hw / 4;
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)t_out * hw * 3);
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(src + g * 16);
    const u32x4 b = *reinterpret_cast<const u32x4*>(src + g * 16 + 8);
    // pixel j = channels (lo, hi) of word 2j and lo of word 2j + 1
    const uint32_t r0 = px_u8(a.x & 0xffff), g0 = px_u8(a.x >> 16), b0 = px_u8(a.y & 0xffff);
    const uint32_t r1 = px_u8(a.z & 0xffff), g1 = px_u8(a.z >> 16), b1 = px_u8(a.w & 0xffff);
    const uint32_t r2 = px_u8(b.x & 0xffff), g2 = px_u8(b.x >> 16), b2 = px_u8(b.y & 0xffff);
    const uint32_t r3 = px_u8(b.z & 0xffff), g3 = px_u8(b.z >> 16), b3 = px_u8(b.w & 0xffff);
    uint32_t* d = dst + g * 3;
    d[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
    d[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
    d[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
  }
}

// ---- pixels [3,Ttot,H,W] bf16 (frames t0..t0+T) -> padded channels-last volume [.., H+2, W+2, 32] (c >= 3 zero)
__global__ void px_in_kernel(const bf16_t* px, bf16_t* dst, int Ttot, int t0, int T, int H, int W, int dt0) {
  const long total = (long)T * H * W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long hw = (long)H * W;
    const int t = (int)(i / hw);
    const long p = i - (long)t * hw;
    const int y = (int)(p / W), x = (int)(p % W);
    bf16_t* dp = dst + (((size_t)(t + dt0) * (H + 2) + (y + 1)) * (W + 2) + (x + 1)) * 32;
#pragma unroll
    for (int c = 0; c < 3; ++c) dp[c] = px[((size_t)c * Ttot + (t0 + t)) * hw + p];
  }
}

// ---- mu = ((conv1_1x1x1(enc)[0:16]) - mean) * inv_std   vae.py:536-541;  enc: [F*h*w, 32] -> out float32 [F,16,h,w]
__global__ void mu_out_kernel(MuArgs a) {
  const bf16_t* enc = a.enc; const bf16_t* w1 = a.w1; const bf16_t* b1 = a.b1; float* out = a.out;
  const float* mean = a.mean; const float* inv_std = a.inv_std;
  const int F = a.F, f_out = a.f_out, h = a.h, w = a.w;
  const long total = (long)F * h * w;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long hw = (long)h * w;
    const int f = (int)(i / hw);
    const long p = i - (long)f * hw;
    float e[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) e[c] = bf2f(enc[i * 32 + c]);
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < 32; ++c) acc += e[c] * bf2f(w1[o * 32 + c]);
      const float mu = rbf(acc + bf2f(b1[o]));
      out[((size_t)(f + f_out) * 16 + o) * hw + p] = rbf(rbf(mu - mean[o]) * inv_std[o]);
    }
  }
}

// ---- row softmax of fp32 scores [rows, ld] (cols valid, zero-fills the tail up to ldp) -> bf16 P [rows, ldp]
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* s, int ld, bf16_t* p, int ldp, int rows, int cols) {
  const int row = blockIdx.x;
  const float* sp = s + (size_t)row * ld;
  __shared__ float red[4];
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, sp[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int c = threadIdx.x; c < cols; c += 256) sum += __expf(sp[c] - mx);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  const float inv = 1.f / (red[0] + red[1] + red[2] + red[3]);
  bf16_t* pp = p + (size_t)row * ldp;
  for (int c = threadIdx.x; c < ldp; c += 256) pp[c] = c < cols ? f2bf(__expf(sp[c] - mx) * inv) : (bf16_t)0;
}

// ---- transpose v [rows, C] (row stride ld) -> vt [C, ldt] (zero tail)
__global__ void transpose_kernel(const bf16_t* v, int ld, bf16_t* vt, int ldt, int rows, int C) {
  __shared__ bf16_t tile[32][33];
  const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 8 rows per pass
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < rows && c < C) ? v[(size_t)r * ld + c] : (bf16_t)0;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < ldt) vt[(size_t)c * ldt + r] = tile[tx][k];
  }
}

inline int grid_for(long n, int block = 256) {
  long g = (n + block - 1) / block;
  return (int)(g > 8192 ? 8192 : (g == 0 ? 1 : g));
}

}  // namespace

namespace {
template <int NF>
hipError_t launch_halo(const ConvArgs& g, hipStream_t s) {
  constexpr int smem = 4 * HPLANE;
  if (hipError_t e = mmpl_dyn_smem_once(reinterpret_cast<const void*>(conv_halo_kernel<NF>), smem); e != hipSuccess) return e;
  const int To = g.M / (g.Ho * g.Wo);
  const long blocks = (long)((g.N + 16 * NF - 1) / (16 * NF)) * ((g.Wo + PW - 1) / PW) * ((g.Ho + PH - 1) / PH) * To;
  hipLaunchKernelGGL(conv_halo_kernel<NF>, dim3((unsigned)blocks), dim3(256), smem, s, g);
  return hipGetLastError();
}
}  // namespace

// 3x3 (x 1 | 3) filters at stride 1 out of a volume padded by one pixel, fragment-packed weights bound, a width the kernel is built for
bool vae_conv_uses_halo(const ConvArgs& g) {
  return g.Wfrag != nullptr && g.kh == 3 && g.kw == 3 && (g.kt == 1 || g.kt == 3) && g.st == 1 && g.sy == 1 &&
         g.sx == 1 && g.Hp == g.Ho + 2 && g.Wp == g.Wo + 2 && g.M > 0 && g.M % (g.Ho * g.Wo) == 0 && g.Cin % 32 == 0 && (g.N % 96 == 0 || g.N <= 16);
}

VaeConvKernel vae_conv_kernel(const ConvArgs& g) {
  if (g.Cin % 32 || g.N % 4 || g.ntaps < 1 || g.ntaps > 27) return VAE_CONV_NONE;
  if (g.frame[0] != nullptr && !vae_conv_uses_halo(g)) return VAE_CONV_NONE;              // only conv_halo_kernel reads ring slots
  if (vae_conv_uses_halo(g)) {
    if (g.N % 96 == 0) return VAE_CONV_HALO6;                 // 96, 192, 384: every ResidualBlock / upsampler conv of the Wan VAE
    if (g.N <= 16) return VAE_CONV_HALO1;                     // the decoder head (96 -> 3, padded to 4): one 16-column fragment
    // (a 128-wide variant spills 18 registers and a 32-wide one does not fit hipcc's allocator at all: the remaining
    // widths -- the encoder head's N = 32 -- stay on the plain kernel; 0.1 % of the FLOPs)
  }
  return (g.N % 96 == 0 && g.N % 128 != 0) ? VAE_CONV_IGEMM3 : VAE_CONV_IGEMM4;   // 96, 288, ...: no padding columns with the 96-wide tile
}

hipError_t vae_launch_conv(const ConvArgs& g, hipStream_t s) {
  if (g.M <= 0) return hipSuccess;
  switch (vae_conv_kernel(g)) {
    case VAE_CONV_HALO6: return launch_halo<6>(g, s);
    case VAE_CONV_HALO1: return launch_halo<1>(g, s);
    case VAE_CONV_IGEMM3:
      hipLaunchKernelGGL(conv_igemm_kernel<3>, dim3(((g.M + BM - 1) / BM) * (g.N / 96)), dim3(256), 0, s, g);
      return hipGetLastError();
    case VAE_CONV_IGEMM4:
      hipLaunchKernelGGL(conv_igemm_kernel<4>, dim3(((g.M + BM - 1) / BM) * ((g.N + 127) / 128)), dim3(256), 0, s, g);
      return hipGetLastError();
    default: return hipErrorInvalidValue;
  }
}
hipError_t vae_launch_norm(const NormArgs& a, hipStream_t s) {
  if (a.npix <= 0) return hipSuccess;
  if (a.C % 8 || a.C > 1024) return hipErrorInvalidValue;
  if (a.C <= 128) hipLaunchKernelGGL(norm_act_pad_kernel<16>, dim3((unsigned)((a.npix + 31) / 32)), dim3(256), 0, s, a);
  else if (a.C <= 256) hipLaunchKernelGGL(norm_act_pad_kernel<32>, dim3((unsigned)((a.npix + 15) / 16)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(norm_act_pad_kernel<64>, dim3((unsigned)((a.npix + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t vae_launch_upsample(const UpArgs& a, hipStream_t s) {
  const long n = (long)a.To * 4 * a.H * a.W * (a.C / 8);
  hipLaunchKernelGGL(upsample_pad_kernel, dim3(grid_for(n)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t vae_launch_zprep(const ZPrepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(z_prep_kernel, dim3(grid_for((long)a.F * a.h * a.w)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t vae_launch_px_out(const bf16_t* src, float* out, int T, int H, int W, int t_out, hipStream_t s) {
  hipLaunchKernelGGL(px_out_kernel, dim3(grid_for((long)T * H * W)), dim3(256), 0, s, src, out, T, H, W, t_out);
  return hipGetLastError();
}
hipError_t vae_launch_px_out_u8(const bf16_t* src, unsigned char* out, int T, int H, int W, int t_out, hipStream_t s) {
  if (W % 4 || ((uintptr_t)out & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(px_out_u8_kernel, dim3(grid_for((long)T * H * W / 4)), dim3(256), 0, s, src, out, T, H, W, t_out);
  return hipGetLastError();
}
hipError_t vae_launch_px_in(const bf16_t* px, bf16_t* dst, int Ttot, int t0, int T, int H, int W, int dt0, hipStream_t s) {
  hipLaunchKernelGGL(px_in_kernel, dim3(grid_for((long)T * H * W)), dim3(256), 0, s, px, dst, Ttot, t0, T, H, W, dt0);
  return hipGetLastError();
}
hipError_t vae_launch_mu_out(const MuArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mu_out_kernel, dim3(grid_for((long)a.F * a.h * a.w)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t vae_launch_softmax(const float* sc, int ld, bf16_t* p, int ldp, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(rows), dim3(256), 0, s, sc, ld, p, ldp, rows, cols);
  return hipGetLastError();
}
hipError_t vae_launch_transpose(const bf16_t* v, int ld, bf16_t* vt, int ldt, int rows, int C, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3((ldt + 31) / 32, (C + 31) / 32), dim3(256), 0, s, v, ld, vt, ldt, rows, C);
  return hipGetLastError();
}
