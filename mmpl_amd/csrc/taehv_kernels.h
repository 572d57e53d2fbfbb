// Launcher interface of the TAEHV preview-decoder kernels (taehv_kernels.hip), used by taehv.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

// 3x3 (or 1x1) stride-1 convolution over padded channels-last FRAMES: every activation of the tiny decoder is a run of frames
// [H + 2][W + 2][C] bf16 whose one-pixel border stays zero (the workspace is cleared once per video, kernels write interiors only).
struct TaehvConvArgs {
  // K axis = the channels of src0, then those of src1 (MemBlock's cat([x, past]) without the cat).  Output frame f reads
  // src0 + f * fs0 and src1 + f * fs1 (elements).  up = 1: the sources are at HALF the output resolution, frames
  // [Ho / 2 + 2][Wo / 2 + 2][C], and nearest x2 up-sampling is folded into the halo addressing.
  const bf16_t* src0; const bf16_t* src1;
  long fs0, fs1;
  int C0, C1, up;
  int ntaps;             // 9 (3x3) | 1 (1x1: the centre tap)
  const bf16_t* Wfrag;   // [(C0 + C1) / 32][ntaps][Nw / 16][64 lanes][8], lane = 16 * (8-channel k chunk) + row (VaeEngine._frag_pack's layout)
  const bf16_t* bias;    // [Nw] or null
  int Nw;                // output channels of the weight matrix, a multiple of the kernel's N tile (64; 16 for the head)
  int N;                 // channels stored per output pixel group (< Nw only for the head: 3 padded to 4 of 16)
  int T, Ho, Wo;         // output frames of this launch and their interior size
  // destination frames [Ho + 2][Wo + 2][ldd]: output channel n of frame f -> frame f * (Nw / Nsplit) + n / Nsplit, channel n % Nsplit
  // (TGrow: one 1x1 conv to stride * C channels = stride consecutive frames of C).  Nsplit is a multiple of the N tile.
  bf16_t* dst; long fsd; int ldd, Nsplit;
  int relu;
  // MemBlock's last conv: + skip (the block's input x, frames [Ho + 2][Wo + 2][Nw]) before the ReLU; the skip value of the launch's
  // LAST frame is also copied to `keep` (one frame): the block's memory for the next call
  const bf16_t* skip; long fss;
  bf16_t* keep;
};
hipError_t taehv_launch_conv(const TaehvConvArgs& g, hipStream_t s);

// latent frame z [16, h, w] bf16 -> tanh(z / 3) * 3 -> interior of a padded frame [h + 2][w + 2][32] (channels 16..31 stay zero)
hipError_t taehv_launch_prep(const bf16_t* z, bf16_t* dst, int h, int w, hipStream_t s);
// head frames [T][H + 2][W + 2][4] bf16 -> fmt 0: float32 [T, 3, H, W] raw; fmt 1: uint8 [T, H, W, 3] = (x.clamp(0, 1) * 255) truncated;
// frames written at t_out of out
hipError_t taehv_launch_px_out(const bf16_t* src, void* out, int fmt, int T, int H, int W, int t_out, hipStream_t s);

// ---- the encoder's own kernels (taehv_enc_kernels.hip), used by taehv_enc.hip
// input layer: pixels -> conv 3->64 3x3 + bias + ReLU -> interiors of T frames [H + 2][W + 2][64] of stride fsd (elements)
struct TaehvConvInArgs {
  const void* px; int fmt;   // fmt 0: float32 [T, 3, H, W] in [0, 1]; 1: uint8 [T, H, W, 3], read as bf16(u / 255)
  const bf16_t* Wfrag;       // the packed [64, 32] matrix, k = (3 ky + kx) * 3 + c, k >= 27 zero: one fragment-major chunk, ntaps 1
  const bf16_t* bias;        // [64]
  int T, H, W;
  bf16_t* dst; long fsd;
};
hipError_t taehv_launch_conv_in(const TaehvConvInArgs& g, hipStream_t s);

// 3x3 stride-2 conv without bias: source frames [2 Ho + 2][2 Wo + 2][C] of stride fs -> interiors of frames [Ho + 2][Wo + 2][Nw] of
// stride fsd; output (y, x) reads padded source rows 2y .. 2y + 2, columns 2x .. 2x + 2
struct TaehvConvS2Args {
  const bf16_t* src; long fs; int C;
  const bf16_t* Wfrag;       // [C / 32][9][Nw / 16][64 lanes][8], as TaehvConvArgs::Wfrag
  int Nw;                    // output channels, a multiple of 64
  int T, Ho, Wo;
  bf16_t* dst; long fsd;
  int relu;
};
hipError_t taehv_launch_conv_s2(const TaehvConvS2Args& g, hipStream_t s);

// head frames [T][h + 2][w + 2][16] bf16 -> planar bf16 [T, 16, h, w] written at frame f_out of out
hipError_t taehv_launch_z_out(const bf16_t* src, bf16_t* out, int T, int h, int w, int f_out, hipStream_t s);
