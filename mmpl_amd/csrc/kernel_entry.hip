// Kernel-level entry points of the VAE / TAEHV launchers, of the GEMM in all its forms, of the attention kernels in all their
// paths, of the norm / RoPE / elementwise kernels and of the umT5 / CLIP glue kernels (include/mmpl_hip.h, "kernel-level entry points
// for tests and tools"): one launch of vae_kernels.hip / taehv_kernels.hip / gemm.hip / attention.hip + attn_w64.hip /
// elementwise.hip / t5.hip / i2v.hip on plain arguments, the way mmpl_gemm / mmpl_layernorm expose the DiT kernels.
// They fill the launchers' argument structs and do no arithmetic of their own.  Every check below runs before the first HIP call:
// a rejected call launches nothing.  The checks bound what a kernel can reach by the sizes the caller states (the header says,
// per entry, how large each buffer must be for them); alignment is checked because the kernels move 8 or 16 bytes per access.
#include <stdint.h>

#include "../../include/mmpl_hip.h"
#include "host_util.h"
#include "taehv_kernels.h"
#include "vae_kernels.h"

namespace {
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
// a * b * c pixels (each factor >= 1) past what an int holds: the kernels walk pixels in a long and split them into int coordinates
inline bool too_many(long a, long b, long c) { return a * b > 0x7fffffffL || a * b * c > 0x7fffffffL; }
}  // namespace

#define REJECT(cond, where, what) \
  do { if (cond) return mmpl_set_error(where, what); } while (0)
#define LAUNCH(expr, where)                                                       \
  do {                                                                            \
    hipError_t e__ = (expr);                                                      \
    if (e__ != hipSuccess) return mmpl_set_error(where, hipGetErrorString(e__));  \
    return 0;                                                                     \
  } while (0)

extern "C" {

int mmpl_vae_conv(const void* src, const void* const* frames, int n_frames, int Cin, int Hp, int Wp, int st, int sy, int sx, int kt,
                  int kh, int kw, const void* W, const void* Wfrag, const void* bias, int To, int Ho, int Wo, int N, void* dst, int Hd,
                  int Wd, int ldd, int dt0, int dy0, int dx0, const void* res, int ldres, const void* ngamma, float nscale,
                  void* const* nframes, int* kernel_out, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_conv";
  if (kernel_out) *kernel_out = 0;
  REJECT(!W || !bias || (!src && !frames), me, "null argument");
  REJECT(Cin < 32 || Hp < 1 || Wp < 1 || To < 1 || Ho < 1 || Wo < 1 || N < 4, me, "non-positive size");
  REJECT(st < 1 || sy < 1 || sx < 1 || kt < 1 || kt > 3 || kh < 1 || kh > 3 || kw < 1 || kw > 3, me, "stride / filter extent out of range");
  REJECT(Cin % 32 || N % 4, me, "Cin % 32 or N % 4");
  REJECT((long)(Ho - 1) * sy + kh > Hp || (long)(Wo - 1) * sx + kw > Wp, me, "the taps leave the padded source frame");
  REJECT(too_many(To, Ho, Wo), me, "too many output pixels");
  REJECT(misaligned(src, 16) || misaligned(W, 16) || misaligned(Wfrag, 16) || misaligned(bias, 8) || misaligned(dst, 8) ||
         misaligned(res, 8) || misaligned(ngamma, 8), me, "misaligned pointer");
  REJECT(!dst && !ngamma, me, "null destination");
  if (dst) {
    REJECT(Hd < 1 || Wd < 1 || dt0 < 0 || dy0 < 0 || dx0 < 0 || dy0 + Ho > Hd || dx0 + Wo > Wd, me, "the output leaves the destination frame");
    REJECT(ldd < N || ldd % 4, me, "ldd < N or ldd % 4");
  }
  REJECT(res && (ldres < N || ldres % 4), me, "ldres < N or ldres % 4");
  ConvArgs g = {};
  if (frames) {
    REJECT(n_frames < 1 || n_frames > 8, me, "more than 8 ring frames");
    REJECT(n_frames != To + kt - 1, me, "a ring needs To + kt - 1 frames");
    for (int j = 0; j < n_frames; ++j) {
      REJECT(!frames[j] || misaligned(frames[j], 16), me, "null or misaligned ring frame");
      g.frame[j] = (const bf16_t*)frames[j];
    }
  }
  g.src = (const bf16_t*)src; g.Cin = Cin; g.Hp = Hp; g.Wp = Wp; g.st = st; g.sy = sy; g.sx = sx; g.ntaps = kt * kh * kw;
  g.kt = kt; g.kh = kh; g.kw = kw;
  int k = 0;
  for (int a = 0; a < kt; ++a)
    for (int b = 0; b < kh; ++b)
      for (int d = 0; d < kw; ++d) g.tap_off[k++] = (a * Hp + b) * Wp + d;
  g.W = (const bf16_t*)W; g.Wfrag = (const bf16_t*)Wfrag; g.bias = (const bf16_t*)bias;
  g.M = To * Ho * Wo; g.N = N; g.Ho = Ho; g.Wo = Wo;
  g.dst = (bf16_t*)dst; g.Hd = Hd; g.Wd = Wd; g.ldd = ldd; g.dt0 = dt0; g.dy0 = dy0; g.dx0 = dx0; g.dc0 = 0;
  g.res = (const bf16_t*)res; g.ldres = ldres;
  const VaeConvKernel which = vae_conv_kernel(g);
  REJECT(which == VAE_CONV_NONE, me, "invalid argument");          // the launcher's own rejections (ring frames on a non-halo shape, ...)
  if (ngamma) {
    REJECT(which != VAE_CONV_HALO6 || N != 96, me, "the fused norm epilogue exists for conv_halo_kernel<6> at N == 96 only");
    REJECT(!nframes || To > 8, me, "more than 8 norm frames");
    g.ngamma = (const bf16_t*)ngamma; g.nscale = nscale;
    for (int t = 0; t < To; ++t) {
      REJECT(!nframes[t] || misaligned(nframes[t], 8), me, "null or misaligned norm frame");
      g.nframe[t] = (bf16_t*)nframes[t];
    }
  }
  if (kernel_out) *kernel_out = (int)which;
  LAUNCH(vae_launch_conv(g, (hipStream_t)stream), me);
}

int mmpl_vae_norm(const void* src, int T, int H, int W, int C, const void* gamma, float scale, int silu, void* dst, int Hd, int Wd,
                  int ldd, int dt0, int dy0, int dx0, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_norm";
  REJECT(!src || !dst, me, "null argument");
  REJECT(T < 1 || H < 1 || W < 1 || C < 8, me, "non-positive size");
  REJECT(C % 8 || C > 1024, me, "C % 8 or C > 1024");
  REJECT(too_many(T, H, W), me, "too many pixels");
  REJECT(ldd < C || ldd % 8, me, "ldd < C or ldd % 8");
  REJECT(Hd < 1 || Wd < 1 || dt0 < 0 || dy0 < 0 || dx0 < 0 || dy0 + H > Hd || dx0 + W > Wd, me, "the output leaves the destination frame");
  REJECT(misaligned(src, 16) || misaligned(gamma, 16) || misaligned(dst, 16), me, "misaligned pointer");
  NormArgs a{(const bf16_t*)src, (long)T * H * W, C, H, W, (const bf16_t*)gamma, scale, silu ? 1 : 0, (bf16_t*)dst, Hd, Wd, ldd, dt0, dy0, dx0};
  LAUNCH(vae_launch_norm(a, (hipStream_t)stream), me);
}

int mmpl_vae_upsample(const void* src, int lds, int C, int H, int W, int To, int interleave, void* dst, int Hd, int Wd,
                      mmpl_stream_t stream) {
  const char* me = "mmpl_vae_upsample";
  REJECT(!src || !dst, me, "null argument");
  REJECT(C < 8 || H < 1 || W < 1 || To < 1, me, "non-positive size");
  REJECT(C % 8 || lds % 8 || lds < (interleave ? 2 * C : C), me, "C % 8, lds % 8 or lds too small");
  REJECT(interleave && (To & 1), me, "interleave needs an even To");
  REJECT(H > 0x3fffffff || W > 0x3fffffff || too_many(To, 2L * H, 2L * W), me, "too many output pixels");
  REJECT(Hd != 2 * H + 2 || Wd != 2 * W + 2, me, "the destination frame is [2H + 2, 2W + 2]");
  REJECT(misaligned(src, 16) || misaligned(dst, 16), me, "misaligned pointer");
  UpArgs a{(const bf16_t*)src, lds, C, H, W, To, interleave ? 1 : 0, (bf16_t*)dst, Hd, Wd};
  LAUNCH(vae_launch_upsample(a, (hipStream_t)stream), me);
}

int mmpl_vae_softmax(const void* scores, int ld, void* p, int ldp, int rows, int cols, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_softmax";
  REJECT(!scores || !p, me, "null argument");
  REJECT(rows < 1 || cols < 1, me, "non-positive size");
  REJECT(ld < cols || ldp < cols, me, "ld < cols or ldp < cols");
  REJECT(misaligned(scores, 4) || misaligned(p, 2), me, "misaligned pointer");
  LAUNCH(vae_launch_softmax((const float*)scores, ld, (bf16_t*)p, ldp, rows, cols, (hipStream_t)stream), me);
}

int mmpl_vae_transpose(const void* v, int ld, void* vt, int ldt, int rows, int C, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_transpose";
  REJECT(!v || !vt, me, "null argument");
  REJECT(rows < 1 || C < 1, me, "non-positive size");
  REJECT(ld < C || ldt < rows, me, "ld < C or ldt < rows");
  REJECT(C > 65535 * 32, me, "C too large");
  REJECT(misaligned(v, 2) || misaligned(vt, 2), me, "misaligned pointer");
  LAUNCH(vae_launch_transpose((const bf16_t*)v, ld, (bf16_t*)vt, ldt, rows, C, (hipStream_t)stream), me);
}

int mmpl_vae_zprep(const void* z, int F, int h, int w, const float* mean, const float* inv_std, const void* w2, const void* b2, void* dst,
                   int dt0, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_zprep";
  REJECT(!z || !mean || !inv_std || !w2 || !b2 || !dst, me, "null argument");
  REJECT(F < 1 || h < 1 || w < 1 || dt0 < 0, me, "non-positive size");
  REJECT(too_many(F, h, w), me, "too many pixels");
  REJECT(misaligned(z, 2) || misaligned(w2, 2) || misaligned(b2, 2) || misaligned(dst, 2), me, "misaligned pointer");
  ZPrepArgs a = {};
  a.z = (const bf16_t*)z; a.F = F; a.h = h; a.w = w;
  for (int i = 0; i < 16; ++i) { a.mean[i] = mean[i]; a.inv_std[i] = inv_std[i]; }
  a.w2 = (const bf16_t*)w2; a.b2 = (const bf16_t*)b2; a.dst = (bf16_t*)dst; a.dt0 = dt0;
  LAUNCH(vae_launch_zprep(a, (hipStream_t)stream), me);
}

int mmpl_vae_mu_out(const void* enc, const void* w1, const void* b1, const float* mean, const float* inv_std, void* out, int F,
                    int f_out, int h, int w, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_mu_out";
  REJECT(!enc || !w1 || !b1 || !mean || !inv_std || !out, me, "null argument");
  REJECT(F < 1 || h < 1 || w < 1 || f_out < 0, me, "non-positive size");
  REJECT(too_many(F, h, w), me, "too many pixels");
  REJECT(misaligned(enc, 2) || misaligned(w1, 2) || misaligned(b1, 2) || misaligned(out, 4), me, "misaligned pointer");
  MuArgs a = {};
  a.enc = (const bf16_t*)enc; a.w1 = (const bf16_t*)w1; a.b1 = (const bf16_t*)b1; a.out = (float*)out;
  for (int i = 0; i < 16; ++i) { a.mean[i] = mean[i]; a.inv_std[i] = inv_std[i]; }
  a.F = F; a.f_out = f_out; a.h = h; a.w = w;
  LAUNCH(vae_launch_mu_out(a, (hipStream_t)stream), me);
}

int mmpl_vae_px_in(const void* px, void* dst, int Ttot, int t0, int T, int H, int W, int dt0, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_px_in";
  REJECT(!px || !dst, me, "null argument");
  REJECT(Ttot < 1 || T < 1 || H < 1 || W < 1 || t0 < 0 || dt0 < 0, me, "non-positive size");
  REJECT((long)t0 + T > Ttot, me, "t0 + T > Ttot");
  REJECT(too_many(T, H, W), me, "too many pixels");
  REJECT(misaligned(px, 2) || misaligned(dst, 2), me, "misaligned pointer");
  LAUNCH(vae_launch_px_in((const bf16_t*)px, (bf16_t*)dst, Ttot, t0, T, H, W, dt0, (hipStream_t)stream), me);
}

int mmpl_vae_px_out(const void* src, void* out, int T, int H, int W, int t_out, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_px_out";
  REJECT(!src || !out, me, "null argument");
  REJECT(T < 1 || H < 1 || W < 1 || t_out < 0, me, "non-positive size");
  REJECT(too_many(T, H, W), me, "too many pixels");
  REJECT(misaligned(src, 8) || misaligned(out, 4), me, "misaligned pointer");
  LAUNCH(vae_launch_px_out((const bf16_t*)src, (float*)out, T, H, W, t_out, (hipStream_t)stream), me);
}

int mmpl_vae_px_out_u8(const void* src, void* out, int T, int H, int W, int t_out, mmpl_stream_t stream) {
  const char* me = "mmpl_vae_px_out_u8";
  REJECT(!src || !out, me, "null argument");
  REJECT(T < 1 || H < 1 || W < 1 || t_out < 0, me, "non-positive size");
  REJECT(too_many(T, H, W), me, "too many pixels");
  REJECT(W % 8, me, "W % 8 (a lane's 4 pixels stay within a row)");
  REJECT(((long)T * H * W) % 4, me, "T * H * W % 4");          // (follows from W % 8; stated because the kernel counts groups of 4 pixels)
  REJECT(misaligned(src, 16) || misaligned(out, 4), me, "misaligned pointer");
  LAUNCH(vae_launch_px_out_u8((const bf16_t*)src, (unsigned char*)out, T, H, W, t_out, (hipStream_t)stream), me);
}

// One launch of mmpl_launch_gemm in any of the forms the forwards use (include/mmpl_hip.h).  The plan is the launcher's own
// (mmpl_gemm_plan, which mmpl_launch_gemm consults for every choice); it is computed after the checks, because the 256 x 256
// kernels' plan asks the device for its CU count.
int mmpl_gemm_ex(const void* A, int lda, const void* W, int ldw, const void* bias, void* C, int ldc, int M, int N, int K, int epi,
                 const void* res, int ldres, const void* gate, int gate_frame_stride, int rows_per_frame, float alpha, int batch,
                 long long sA, long long sW, long long sC, void* const* v_dst, int n_v_dst, int v_col0, int v_ld, void* scratch,
                 size_t scratch_bytes, void* tile_counter, int* plan_out, mmpl_stream_t stream) {
  const char* me = "mmpl_gemm_ex";
  if (plan_out)
    for (int i = 0; i < 6; ++i) plan_out[i] = 0;
  REJECT(epi < EPI_BIAS || epi > EPI_BIAS_VPAGES, me, "unknown epilogue");
  REJECT(!A || !W || !C, me, "null argument");
  REJECT((epi == EPI_GATE_RES && (!res || !gate)) || (epi == EPI_RES && !res) || (epi == EPI_BIAS_VPAGES && !v_dst), me, "missing epilogue operand");
  REJECT(M < 1 || N < 1 || K < 1, me, "non-positive size");
  REJECT(K % 64, me, "K % 64");
  REJECT(N % 4, me, "N % 4");
  REJECT(lda % 8, me, "lda % 8");
  REJECT(lda < K, me, "lda < K");
  REJECT(ldw % 8, me, "ldw % 8");
  REJECT(ldw < K, me, "ldw < K");
  REJECT(batch < 1, me, "batch < 1");
  REJECT(batch > 65535, me, "batch > 65535");
  REJECT(ldc % 4, me, "ldc % 4");
  REJECT(batch == 1 && ldc < N, me, "ldc < N");
  REJECT(epi == EPI_F32_SCALE && bias, me, "the fp32 epilogue takes no bias");
  const bool has_res = epi == EPI_GATE_RES || epi == EPI_RES;
  REJECT(has_res && ldres < N, me, "ldres < N");
  REJECT(has_res && ldres % 4, me, "ldres % 4");
  REJECT((epi == EPI_GATE_RES || epi == EPI_BIAS_VPAGES) && rows_per_frame < 1, me, "rows_per_frame < 1");
  if (epi == EPI_GATE_RES) {
    REJECT(gate_frame_stride < 0, me, "gate_frame_stride < 0");
    REJECT(gate_frame_stride % 4, me, "gate_frame_stride % 4");
    // (0: one gate row for every frame; otherwise the frames' rows must not overlap)
    REJECT(M > rows_per_frame && gate_frame_stride != 0 && gate_frame_stride < N, me, "gate_frame_stride < N with more than one frame");
  }
  REJECT(misaligned(A, 16), me, "A not 16-byte aligned");
  REJECT(misaligned(W, 16), me, "W not 16-byte aligned");
  REJECT(misaligned(C, epi == EPI_F32_SCALE ? 16 : 8), me, epi == EPI_F32_SCALE ? "fp32 C not 16-byte aligned" : "C not 8-byte aligned");
  REJECT(misaligned(bias, 8), me, "bias not 8-byte aligned");
  REJECT(has_res && misaligned(res, 8), me, "res not 8-byte aligned");
  REJECT(epi == EPI_GATE_RES && misaligned(gate, 8), me, "gate not 8-byte aligned");
  GemmArgs g = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W, ldw, (const bf16_t*)bias, (bf16_t*)C, ldc, M, N, K, epi);
  g.res = (const bf16_t*)res; g.ldres = ldres; g.gate = (const bf16_t*)gate;
  g.gate_frame_stride = gate_frame_stride; g.rows_per_frame = rows_per_frame > 0 ? rows_per_frame : 1; g.alpha = alpha;
  g.batch = batch; g.sA = (long)sA; g.sW = (long)sW; g.sC = (long)sC;
  if (batch > 1) {
    REJECT(has_res || epi == EPI_BIAS_VPAGES, me, "the batched form has no residual and no pages");
    REJECT(sA < 0 || sW < 0 || sC < 0, me, "negative batch stride");
    REJECT(sA % 8, me, "sA % 8");
    REJECT(sW % 8, me, "sW % 8");
    REJECT(sC % 4, me, "sC % 4");
  }
  if (epi == EPI_BIAS_VPAGES) {
    REJECT(n_v_dst < 1, me, "n_v_dst < 1");
    REJECT(n_v_dst > 8, me, "more than 8 pages");
    REJECT((long)n_v_dst * rows_per_frame < M, me, "the pages hold fewer than M rows");
    REJECT(v_col0 % 4, me, "v_col0 % 4");
    REJECT(v_col0 <= 0 || v_col0 >= N, me, "v_col0 outside (0, N)");
    REJECT(v_ld < N - v_col0, me, "v_ld < N - v_col0");
    REJECT(v_ld % 4, me, "v_ld % 4");
    for (int i = 0; i < n_v_dst; ++i) {
      REJECT(!v_dst[i], me, "null page");
      REJECT(misaligned(v_dst[i], 8), me, "page not 8-byte aligned");
      g.v_dst[i] = (bf16_t*)v_dst[i];
    }
    g.v_col0 = v_col0; g.v_ld = v_ld;
  }
  if (scratch) {
    REJECT(scratch_bytes < mmpl_gemm_scratch_bytes(), me, "scratch smaller than mmpl_gemm_scratch_bytes()");
    REJECT(misaligned(scratch, 256), me, "scratch must be 256-byte aligned");
    g.tile_counter = (int*)scratch;                        // the layout mmpl_gemm_scratch documents
    g.splitk_cnt = g.tile_counter + 64;
    g.splitk_ws = (float*)((char*)scratch + 2048);
  } else {
    REJECT(misaligned(tile_counter, 4), me, "tile_counter not 4-byte aligned");
    g.tile_counter = (int*)tile_counter;
  }
  // (today the launcher sends every batched GEMM to the small kernel, the only one that reads the batch strides: this guards that)
  const GemmPlan p = mmpl_gemm_plan(g);
  REJECT(batch > 1 && p.kernel != GEMM_KERNEL_SMALL, me, "batched GEMMs run on the small kernel only");
  if (plan_out) {
    plan_out[0] = p.kernel; plan_out[1] = p.tail; plan_out[2] = p.staged_epilogue; plan_out[3] = p.main_blocks;
    plan_out[4] = p.tail_blocks; plan_out[5] = p.splitk_s;
  }
  LAUNCH(mmpl_launch_gemm(g, (hipStream_t)stream), me);
}

// What mmpl_attn_fwd_ex and mmpl_attn_fwd_groups_ex check on the arguments they share, in the order both report it, and the AttnArgs
// those arguments fill (Lq: the rows of one launch or of one group; last_row_copies: 0 for a grouped launch).
static int attn_entry_common(const char* me, const void* q, int ldq, void* o, int ldo, int ldk, int ldv, int page_rows, int Lq, int num_heads,
                             float softmax_scale, void* workspace, size_t workspace_bytes, int variant, int q_prescaled, int last_row_copies,
                             void* history, void* stats_dev, AttnArgs& a) {
  REJECT(!(softmax_scale > 0.f) || softmax_scale > 3.0e38f, me, "softmax_scale must be positive and finite");
  REJECT(variant != ATTN_AUTO && variant != ATTN_LOCKSTEP && variant != ATTN_W64 && variant != ATTN_W64 + 1, me, "unknown kernel variant");
  REJECT(ldq % 8, me, "ldq % 8");
  REJECT(ldo % 8, me, "ldo % 8");
  REJECT(ldk % 8, me, "ldk % 8");
  REJECT(ldv % 8, me, "ldv % 8");
  REJECT(ldq < 128 * num_heads, me, "ldq < 128 * num_heads");
  REJECT(ldo < 128 * num_heads, me, "ldo < 128 * num_heads");
  REJECT(ldk < 128 * num_heads, me, "ldk < 128 * num_heads");
  REJECT(ldv < 128 * num_heads, me, "ldv < 128 * num_heads");
  REJECT(misaligned(q, 16), me, "q not 16-byte aligned");
  REJECT(misaligned(o, 16), me, "o not 16-byte aligned");
  REJECT(last_row_copies < 0, me, "last_row_copies < 0");
  REJECT(misaligned(workspace, 16), me, "workspace not 16-byte aligned");
  REJECT(misaligned(history, 2), me, "history not 2-byte aligned");
  REJECT(misaligned(stats_dev, 8), me, "stats not 8-byte aligned");
  a = attn_args((const bf16_t*)q, ldq, (bf16_t*)o, ldo, ldk, ldv, page_rows, Lq, num_heads, softmax_scale);
  a.split_ws = (float*)workspace; a.split_ws_bytes = workspace ? workspace_bytes : 0;
  a.variant = variant > ATTN_W64 ? ATTN_W64 : variant;
  a.q_prescaled = variant == ATTN_W64 + 1 || q_prescaled != 0;
  a.last_row_copies = last_row_copies;
  a.history = (unsigned char*)history;
  a.redo_stats = (unsigned long long*)stats_dev;
  return 0;
}

// One launch of mmpl_launch_attention with everything AttnArgs carries (include/mmpl_hip.h).  The plan is the launcher's own
// (mmpl_attn_plan, which mmpl_launch_attention consults for every choice); it is computed after the checks, because the plan of
// the cross and the w64 kernel asks the device for its CU count.
int mmpl_attn_fwd_ex(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                     const unsigned char* page_group, int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads,
                     float softmax_scale, void* workspace, size_t workspace_bytes, int variant, int q_prescaled, int cross,
                     int last_row_copies, void* history, void* stats_dev, int* plan_out, mmpl_stream_t stream) {
  const char* me = "mmpl_attn_fwd_ex";
  if (plan_out)
    for (int i = 0; i < 8; ++i) plan_out[i] = 0;
  REJECT(!q || !o || !k_pages || !v_pages, me, "null argument");
  REJECT(n_pages < 1, me, "n_pages < 1");
  REJECT(n_pages > MMPL_MAX_PAGES, me, "more than 24 pages");
  REJECT(page_rows < 1 || Lq < 1 || num_heads < 1, me, "non-positive size");
  AttnArgs a;
  if (int e = attn_entry_common(me, q, ldq, o, ldo, ldk, ldv, page_rows, Lq, num_heads, softmax_scale, workspace, workspace_bytes, variant,
                                q_prescaled, last_row_copies, history, stats_dev, a))
    return e;
  a.n_pages = n_pages;
  for (int i = 0; i < n_pages; ++i) {
    REJECT(!k_pages[i] || !v_pages[i], me, "null page");
    REJECT(misaligned(k_pages[i], 16) || misaligned(v_pages[i], 16), me, "page not 16-byte aligned");
    a.k_pages[i] = (const bf16_t*)k_pages[i]; a.v_pages[i] = (const bf16_t*)v_pages[i];
    a.page_group[i] = page_group ? page_group[i] : 0;
  }
  a.cross = cross != 0;
  const int resolved = mmpl_attn_resolve_variant(a);          // (no HIP call: the arguments and the run-time switches)
  REJECT(a.q_prescaled && resolved != ATTN_W64, me, "a prescaled q runs on the 64-rows-per-wave kernel only");
  REJECT(last_row_copies > 1 && resolved != ATTN_LOCKSTEP, me, "last_row_copies > 1 runs on the lock-step kernel only");
  REJECT(last_row_copies > 1 && n_pages != 1, me, "last_row_copies > 1 with more than one page");
  const AttnPlan p = mmpl_attn_plan(a);
  REJECT(p.invalid, me, "invalid argument");                  // the launcher's own rejections, all stated above: a guard
  if (plan_out) {
    plan_out[0] = p.kernel; plan_out[1] = p.n_pages; plan_out[2] = p.kv_tiles; plan_out[3] = p.main_blocks;
    plan_out[4] = p.tail_items; plan_out[5] = p.sp; plan_out[6] = p.qb_per_block; plan_out[7] = p.blocks_per_head;
  }
  LAUNCH(mmpl_launch_attention(a, (hipStream_t)stream), me);
}

// mmpl_launch_attention_groups on plain arguments: mmpl_attn_fwd_ex's checks of the common arguments and of every page.
int mmpl_attn_fwd_groups_ex(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                            const unsigned char* page_group, const int* group_n_pages, int n_groups, int group_rows, int ldk, int ldv,
                            int page_rows, int num_heads, float softmax_scale, void* workspace, size_t workspace_bytes, int variant,
                            int q_prescaled, void* history, void* stats_dev, int* plan_out, mmpl_stream_t stream) {
  const char* me = "mmpl_attn_fwd_groups_ex";
  if (plan_out)
    for (int i = 0; i < 10; ++i) plan_out[i] = 0;
  REJECT(!q || !o || !k_pages || !v_pages || !group_n_pages, me, "null argument");
  REJECT(n_groups < 1, me, "n_groups < 1");
  REJECT(n_groups > MMPL_MAX_GROUPS, me, "more than 8 groups");
  REJECT(page_rows < 1 || group_rows < 1 || num_heads < 1, me, "non-positive size");
  AttnArgs a;
  if (int e = attn_entry_common(me, q, ldq, o, ldo, ldk, ldv, page_rows, group_rows, num_heads, softmax_scale, workspace, workspace_bytes,
                                variant, q_prescaled, 0, history, stats_dev, a))
    return e;
  REJECT(a.q_prescaled && mmpl_attn_resolve_variant(a) != ATTN_W64, me, "a prescaled q runs on the 64-rows-per-wave kernel only");
  AttnGroupPages lists[MMPL_MAX_GROUPS] = {};
  for (int g = 0, at = 0; g < n_groups; ++g) {
    REJECT(group_n_pages[g] < 1, me, "a group with n_pages < 1");
    REJECT(group_n_pages[g] > MMPL_MAX_PAGES, me, "a group with more than 24 pages");
    lists[g].n_pages = group_n_pages[g];
    for (int i = 0; i < group_n_pages[g]; ++i, ++at) {
      REJECT(!k_pages[at] || !v_pages[at], me, "null page");
      REJECT(misaligned(k_pages[at], 16) || misaligned(v_pages[at], 16), me, "page not 16-byte aligned");
      lists[g].k_pages[i] = (const bf16_t*)k_pages[at]; lists[g].v_pages[i] = (const bf16_t*)v_pages[at];
      lists[g].page_group[i] = page_group ? page_group[at] : 0;
    }
  }
  const AttnGroupPlan gp = mmpl_attn_groups_plan(a, n_groups, lists);
  REJECT(gp.invalid, me, "invalid argument");                 // the launcher's own rejections, all stated above: a guard
  if (plan_out) {
    const AttnPlan& p = gp.p;
    plan_out[0] = p.kernel; plan_out[1] = p.n_pages; plan_out[2] = p.kv_tiles; plan_out[3] = p.main_blocks;
    plan_out[4] = p.tail_items; plan_out[5] = p.sp; plan_out[6] = p.qb_per_block; plan_out[7] = p.blocks_per_head;
    plan_out[8] = gp.grouped; plan_out[9] = gp.items;
  }
  LAUNCH(mmpl_launch_attention_groups(a, n_groups, lists, (hipStream_t)stream), me);
}

int mmpl_taehv_conv(const void* src0, const void* src1, long long fs0, long long fs1, int C0, int C1, int up, int ntaps,
                    const void* Wfrag, const void* bias, int Nw, int N, int T, int Ho, int Wo, void* dst, long long fsd, int ldd,
                    int Nsplit, int relu, const void* skip, long long fss, void* keep, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_conv";
  REJECT(!src0 || !Wfrag || !dst || (C1 > 0 && !src1), me, "null argument");
  REJECT(T < 1 || Ho < 1 || Wo < 1 || C0 < 32 || C1 < 0 || Nw < 16 || N < 4 || Nsplit < 16 || ldd < 4, me, "non-positive size");
  REJECT(fs0 < 0 || fs1 < 0 || fsd < 0 || fss < 0, me, "negative frame stride");
  REJECT(fs0 % 8 || fs1 % 8 || fsd % 4 || fss % 4, me, "frame stride not a multiple of the access width");
  REJECT(keep && !skip, me, "keep without skip");
  const int BN = Nw % 64 == 0 ? 64 : 16;
  // the launcher's own rejections, repeated here so that nothing below divides by a bad Nsplit
  REJECT((ntaps != 9 && ntaps != 1) || C0 % 32 || C1 % 32 || Nw % BN || Nsplit % BN || Nw % Nsplit || N % 4 || N > Nw || ldd % 4 ||
         (up && ((Ho | Wo) & 1)) || (skip && N != Nw), me, "invalid argument");
  REJECT(Nsplit != Nw && N != Nw, me, "a frame split stores every channel (N == Nw)");
  REJECT(ldd < (N < Nsplit ? N : Nsplit), me, "ldd smaller than the channels stored per pixel");
  REJECT(misaligned(src0, 16) || misaligned(src1, 16) || misaligned(Wfrag, 16) || misaligned(bias, 8) || misaligned(dst, 8) ||
         misaligned(skip, 8) || misaligned(keep, 8), me, "misaligned pointer");
  TaehvConvArgs g = {};
  g.src0 = (const bf16_t*)src0; g.src1 = (const bf16_t*)src1; g.fs0 = (long)fs0; g.fs1 = (long)fs1; g.C0 = C0; g.C1 = C1; g.up = up ? 1 : 0;
  g.ntaps = ntaps; g.Wfrag = (const bf16_t*)Wfrag; g.bias = (const bf16_t*)bias; g.Nw = Nw; g.N = N; g.T = T; g.Ho = Ho; g.Wo = Wo;
  g.dst = (bf16_t*)dst; g.fsd = (long)fsd; g.ldd = ldd; g.Nsplit = Nsplit; g.relu = relu ? 1 : 0;
  g.skip = (const bf16_t*)skip; g.fss = (long)fss; g.keep = (bf16_t*)keep;
  LAUNCH(taehv_launch_conv(g, (hipStream_t)stream), me);
}

int mmpl_taehv_prep(const void* z, void* dst, int h, int w, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_prep";
  REJECT(!z || !dst, me, "null argument");
  REJECT(h < 1 || w < 1 || (long)h * w > 0x7fffffffL / 64, me, "non-positive size");
  REJECT(misaligned(z, 2) || misaligned(dst, 16), me, "misaligned pointer");
  LAUNCH(taehv_launch_prep((const bf16_t*)z, (bf16_t*)dst, h, w, (hipStream_t)stream), me);
}

int mmpl_taehv_px_out(const void* src, void* out, int out_format, int T, int H, int W, int t_out, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_px_out";
  REJECT(!src || !out, me, "null argument");
  REJECT(out_format != 0 && out_format != 1, me, "unknown out_format");
  REJECT(T < 1 || H < 1 || W < 1 || t_out < 0, me, "non-positive size");
  REJECT(too_many(T, H + 2L, W + 2L), me, "too many pixels");
  REJECT(misaligned(src, 8) || misaligned(out, out_format == 0 ? 4 : 1), me, "misaligned pointer");
  LAUNCH(taehv_launch_px_out((const bf16_t*)src, out, out_format, T, H, W, t_out, (hipStream_t)stream), me);
}

int mmpl_taehv_conv_in(const void* px, int in_format, const void* Wfrag, const void* bias, int T, int H, int W, void* dst,
                       long long fsd, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_conv_in";
  REJECT(!px || !Wfrag || !bias || !dst, me, "null argument");
  REJECT(in_format != 0 && in_format != 1, me, "unknown in_format");
  REJECT(T < 1 || H < 1 || W < 1 || too_many(T, H, W), me, "non-positive size");
  REJECT(fsd < 0 || fsd % 4, me, "frame stride not a multiple of the access width");
  REJECT(misaligned(px, in_format == 0 ? 4 : 1) || misaligned(Wfrag, 16) || misaligned(bias, 8) || misaligned(dst, 8), me,
         "misaligned pointer");
  TaehvConvInArgs g = {};
  g.px = px; g.fmt = in_format; g.Wfrag = (const bf16_t*)Wfrag; g.bias = (const bf16_t*)bias; g.T = T; g.H = H; g.W = W;
  g.dst = (bf16_t*)dst; g.fsd = (long)fsd;
  LAUNCH(taehv_launch_conv_in(g, (hipStream_t)stream), me);
}

int mmpl_taehv_conv_s2(const void* src, long long fs, int C, const void* Wfrag, int Nw, int T, int Ho, int Wo, void* dst,
                       long long fsd, int relu, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_conv_s2";
  REJECT(!src || !Wfrag || !dst, me, "null argument");
  REJECT(T < 1 || Ho < 1 || Wo < 1 || C < 32 || Nw < 64 || too_many(T, 2L * Ho + 2, 2L * Wo + 2), me, "non-positive size");
  REJECT(C % 32 || Nw % 64, me, "invalid argument");
  REJECT(fs < 0 || fsd < 0 || fs % 8 || fsd % 4, me, "frame stride not a multiple of the access width");
  REJECT(misaligned(src, 16) || misaligned(Wfrag, 16) || misaligned(dst, 8), me, "misaligned pointer");
  TaehvConvS2Args g = {};
  g.src = (const bf16_t*)src; g.fs = (long)fs; g.C = C; g.Wfrag = (const bf16_t*)Wfrag; g.Nw = Nw; g.T = T; g.Ho = Ho; g.Wo = Wo;
  g.dst = (bf16_t*)dst; g.fsd = (long)fsd; g.relu = relu ? 1 : 0;
  LAUNCH(taehv_launch_conv_s2(g, (hipStream_t)stream), me);
}

int mmpl_taehv_z_out(const void* src, void* out, int T, int h, int w, int f_out, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_z_out";
  REJECT(!src || !out, me, "null argument");
  REJECT(T < 1 || h < 1 || w < 1 || f_out < 0 || too_many(T, h + 2L, w + 2L), me, "non-positive size");
  REJECT(misaligned(src, 16) || misaligned(out, 2), me, "misaligned pointer");
  LAUNCH(taehv_launch_z_out((const bf16_t*)src, (bf16_t*)out, T, h, w, f_out, (hipStream_t)stream), me);
}

// One launch of mmpl_launch_layernorm (include/mmpl_hip.h).  The plan is the launcher's own (mmpl_ln_plan, which mmpl_launch_layernorm
// consults for every choice); it is computed after the checks, because a pipelined kernel's plan asks the device for its occupancy.
int mmpl_layernorm_ex(const void* x, int ldx, void* y, int ldy, int rows, int d, float eps, const void* scale, const void* shift,
                      int mod_frame_stride, int rows_per_frame, const void* w, const void* b, int pipeline, int groups_per_block,
                      int* plan_out, mmpl_stream_t stream) {
  const char* me = "mmpl_layernorm_ex";
  if (plan_out)
    for (int i = 0; i < 7; ++i) plan_out[i] = 0;
  REJECT(!x || !y, me, "null argument");
  REJECT(!w && (!scale || !shift), me, "need (scale, shift) or (w, b)");
  REJECT(w && !b, me, "w without b");
  REJECT(rows < 1 || d < 1, me, "non-positive size");
  REJECT(d % 8, me, "d % 8");
  REJECT(d > 5120, me, "d > 5120");
  REJECT(ldx % 8, me, "ldx % 8");
  REJECT(ldx < d, me, "ldx < d");
  REJECT(ldy % 8, me, "ldy % 8");
  REJECT(ldy < d, me, "ldy < d");
  if (!w) {
    REJECT(rows_per_frame < 1, me, "rows_per_frame < 1");
    REJECT(mod_frame_stride < 0, me, "mod_frame_stride < 0");
    REJECT(mod_frame_stride % 8, me, "mod_frame_stride % 8");
  }
  REJECT(misaligned(x, 16), me, "x not 16-byte aligned");
  REJECT(misaligned(y, 16), me, "y not 16-byte aligned");
  REJECT(w ? misaligned(w, 16) || misaligned(b, 16) : misaligned(scale, 16) || misaligned(shift, 16), me, "column vector not 16-byte aligned");
  REJECT(pipeline < -1 || pipeline > 1, me, "pipeline outside -1 .. 1");
  REJECT(pipeline == 1 && (d / 8 + 63) / 64 < 6, me, "the pipelined kernel exists from NIT 6 (d > 2560) only");
  REJECT(groups_per_block < 0, me, "groups_per_block < 0");
  LnArgs a = ln_args((const bf16_t*)x, ldx, (bf16_t*)y, ldy, rows, d, eps);
  a.scale = (const bf16_t*)scale; a.shift = (const bf16_t*)shift; a.mod_frame_stride = mod_frame_stride;
  a.rows_per_frame = rows_per_frame > 0 ? rows_per_frame : 1; a.w = (const bf16_t*)w; a.b = (const bf16_t*)b;
  // (which kernel runs is the plan's decision, made on the host alone: the last check still precedes the first HIP call)
  REJECT(groups_per_block && !mmpl_ln_pipelined(a, pipeline), me, "groups_per_block with the one-row-per-wave kernel");
  const RowPassPlan p = mmpl_ln_plan(a, pipeline, groups_per_block);
  REJECT(p.invalid, me, "invalid argument");                  // the launcher's own rejections, all stated above: a guard
  if (plan_out) {
    plan_out[0] = p.kernel; plan_out[1] = p.nit; plan_out[2] = p.full; plan_out[3] = p.resident; plan_out[4] = p.groups_per_block;
    plan_out[5] = p.grid_x; plan_out[6] = p.grid_y;
  }
  LAUNCH(mmpl_launch_layernorm(a, (hipStream_t)stream, pipeline, groups_per_block), me);
}

// One launch of mmpl_launch_qknorm with everything QkNormArgs carries (include/mmpl_hip.h); with rope == 0 and k == NULL the
// arguments are exactly those mmpl_launch_rmsnorm builds.
int mmpl_qknorm_ex(void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* wq, const void* wk, int rows, int d,
                   float eps, float q_scale, int rope, const float* cos_tab, const float* sin_tab, int n_frames, const int* frame_ids,
                   const int* frame_base_dev, void* const* k_dst, void* const* v_dst, int rows_per_frame, int grid_w,
                   int groups_per_block, int* plan_out, mmpl_stream_t stream) {
  const char* me = "mmpl_qknorm_ex";
  if (plan_out)
    for (int i = 0; i < 7; ++i) plan_out[i] = 0;
  REJECT(!q || !wq, me, "null argument");
  REJECT(v && !k, me, "v without k");
  REJECT(k && (!wk || !k_dst), me, "k without wk or k_dst");
  REJECT(v && !v_dst, me, "v without v_dst");
  REJECT(rows < 1 || d < 1, me, "non-positive size");
  REJECT(d % 128, me, "d % 128");
  REJECT(d > 5120, me, "d > 5120");
  REJECT(ldq % 8, me, "ldq % 8");
  REJECT(ldq < d, me, "ldq < d");
  REJECT(k && ldk % 8, me, "ldk % 8");
  REJECT(k && ldk < d, me, "ldk < d");
  REJECT(v && ldv % 8, me, "ldv % 8");
  REJECT(v && ldv < d, me, "ldv < d");
  REJECT(misaligned(q, 16), me, "q not 16-byte aligned");
  REJECT(misaligned(k, 16), me, "k not 16-byte aligned");
  REJECT(misaligned(v, 16), me, "v not 16-byte aligned");
  REJECT(misaligned(wq, 16) || misaligned(wk, 16), me, "gain not 16-byte aligned");
  REJECT(n_frames < 1 || n_frames > 8, me, "n_frames outside 1 .. 8");
  if (rope) {
    REJECT(!cos_tab || !sin_tab || !frame_ids, me, "rope without tables or frame ids");
    REJECT(misaligned(cos_tab, 4) || misaligned(sin_tab, 4) || misaligned(frame_base_dev, 4), me, "table or frame base not 4-byte aligned");
    REJECT(rows_per_frame < 1, me, "rows_per_frame < 1");
    REJECT((long)n_frames * rows_per_frame != rows, me, "rows != n_frames * rows_per_frame");
    REJECT(grid_w < 1, me, "grid_w < 1");
    REJECT(grid_w > 1024, me, "grid_w > 1024");
    REJECT((rows_per_frame - 1) / grid_w > 1023, me, "more than 1024 grid rows");
  }
  REJECT(groups_per_block < 0, me, "groups_per_block < 0");
  QkNormArgs a = {};
  a.q = (bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = k ? ldk : 0; a.v = (const bf16_t*)v; a.ldv = v ? ldv : 0;
  a.wq = (const bf16_t*)wq; a.wk = (const bf16_t*)wk; a.rows = rows; a.d = d; a.eps = eps; a.q_scale = q_scale; a.rope = rope ? 1 : 0;
  // without rope every row belongs to local frame 0: the one geometry mmpl_launch_rmsnorm states
  a.rows_per_frame = rope ? rows_per_frame : rows; a.grid_w = rope ? grid_w : 1;
  if (rope) {
    a.cos_tab = cos_tab; a.sin_tab = sin_tab; a.frame_base = frame_base_dev;
    for (int i = 0; i < n_frames; ++i) a.frame_ids[i] = frame_ids[i];
  }
  for (int i = 0; k && i < (rope ? n_frames : 1); ++i) {
    REJECT(!k_dst[i] || (v && !v_dst[i]), me, "null page");
    REJECT(misaligned(k_dst[i], 16) || (v && misaligned(v_dst[i], 16)), me, "page not 16-byte aligned");
    a.k_dst[i] = (bf16_t*)k_dst[i];
    if (v) a.v_dst[i] = (bf16_t*)v_dst[i];
  }
  const RowPassPlan p = mmpl_qknorm_plan(a, groups_per_block);
  REJECT(p.invalid, me, "invalid argument");                  // the launcher's own rejections, all stated above: a guard
  if (plan_out) {
    plan_out[0] = p.kernel; plan_out[1] = p.nit; plan_out[2] = p.full; plan_out[3] = p.resident; plan_out[4] = p.groups_per_block;
    plan_out[5] = p.grid_x; plan_out[6] = p.grid_y;
  }
  LAUNCH(mmpl_launch_qknorm(a, (hipStream_t)stream, groups_per_block), me);
}

// The small kernels of elementwise.hip, one launch each on plain arguments.
int mmpl_modulation(const void* mod, long long mod_layer_stride, const void* e, int e_frame_stride, int bcast, void* emod, int n_layers,
                    int n_frames, int nmod, int d, mmpl_stream_t stream) {
  const char* me = "mmpl_modulation";
  REJECT(!mod || !e || !emod, me, "null argument");
  REJECT(n_layers < 1 || n_frames < 1 || nmod < 1 || d < 1, me, "non-positive size");
  REJECT(mod_layer_stride < 0 || e_frame_stride < 0, me, "negative stride");
  REJECT(too_many(n_layers, n_frames, (long)nmod * d) || (long)nmod * d > 0x7fffffffL, me, "too many elements");
  REJECT(misaligned(mod, 2) || misaligned(e, 2) || misaligned(emod, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_modulation((const bf16_t*)mod, (size_t)mod_layer_stride, (const bf16_t*)e, e_frame_stride, bcast ? 1 : 0, (bf16_t*)emod,
                                n_layers, n_frames, nmod, d, (hipStream_t)stream), me);
}

int mmpl_patchify(const void* x, void* a, int lda, int F, int C, int h, int w, mmpl_stream_t stream) {
  const char* me = "mmpl_patchify";
  REJECT(!x || !a, me, "null argument");
  REJECT(F < 1 || C < 1 || h < 1 || w < 1, me, "non-positive size");
  REJECT((h | w) & 1, me, "odd h or w");
  REJECT(C > 0x1fffffff || lda < 4 * C, me, "lda < 4 C");
  REJECT(too_many(F, h, w), me, "too many pixels");
  REJECT(misaligned(x, 2) || misaligned(a, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_patchify((const bf16_t*)x, (bf16_t*)a, lda, F, C, h, w, (hipStream_t)stream), me);
}

int mmpl_patchify2(const void* x, const void* y, void* a, int lda, int F, int Cx, int Cy, int h, int w, mmpl_stream_t stream) {
  const char* me = "mmpl_patchify2";
  REJECT(!x || !y || !a, me, "null argument");
  REJECT(F < 1 || Cx < 1 || Cy < 1 || h < 1 || w < 1, me, "non-positive size");
  REJECT((h | w) & 1, me, "odd h or w");
  REJECT(Cx > 0x0fffffff || Cy > 0x0fffffff || lda < 4 * (Cx + Cy), me, "lda < 4 (Cx + Cy)");
  REJECT(too_many(F, h, w), me, "too many pixels");
  REJECT(misaligned(x, 2) || misaligned(y, 2) || misaligned(a, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_patchify2((const bf16_t*)x, (const bf16_t*)y, (bf16_t*)a, lda, F, Cx, Cy, h, w, (hipStream_t)stream), me);
}

int mmpl_unpatchify(const void* y, int ldy, void* out, int F, int C, int h, int w, mmpl_stream_t stream) {
  const char* me = "mmpl_unpatchify";
  REJECT(!y || !out, me, "null argument");
  REJECT(F < 1 || C < 1 || h < 1 || w < 1, me, "non-positive size");
  REJECT((h | w) & 1, me, "odd h or w");
  REJECT(C > 0x1fffffff || ldy < 4 * C, me, "ldy < 4 C");
  REJECT(too_many(F, h, w), me, "too many pixels");
  REJECT(misaligned(y, 2) || misaligned(out, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_unpatchify((const bf16_t*)y, ldy, (bf16_t*)out, F, C, h, w, (hipStream_t)stream), me);
}

int mmpl_sinusoid(const float* t, void* out, int F, int freq_dim, mmpl_stream_t stream) {
  const char* me = "mmpl_sinusoid";
  REJECT(!t || !out, me, "null argument");
  REJECT(F < 1 || freq_dim < 2, me, "non-positive size");
  REJECT(freq_dim & 1, me, "odd freq_dim");
  REJECT((long)F * (freq_dim / 2) > 0x7fffffffL - 256, me, "too many elements");
  REJECT(misaligned(t, 4) || misaligned(out, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_sinusoid(t, (bf16_t*)out, F, freq_dim, (hipStream_t)stream), me);
}

int mmpl_silu(const void* x, void* y, size_t n, mmpl_stream_t stream) {
  const char* me = "mmpl_silu";
  REJECT(!x || !y, me, "null argument");
  REJECT(n < 1, me, "non-positive size");
  REJECT(misaligned(x, 2) || misaligned(y, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_silu((const bf16_t*)x, (bf16_t*)y, n, (hipStream_t)stream), me);
}

int mmpl_rows_equal_last(const void* x, int ld, int rows, int d, int* flags_dev, mmpl_stream_t stream) {
  const char* me = "mmpl_rows_equal_last";
  REJECT(!x || !flags_dev, me, "null argument");
  REJECT(rows < 1, me, "rows < 1");
  REJECT(d < 1, me, "non-positive size");
  REJECT(d % 8, me, "d % 8");
  REJECT(ld % 8, me, "ld % 8");
  REJECT(ld < d, me, "ld < d");
  REJECT(misaligned(x, 16) || misaligned(flags_dev, 4), me, "misaligned pointer");
  LAUNCH(mmpl_launch_rows_equal_last((const bf16_t*)x, ld, rows, d, flags_dev, (hipStream_t)stream), me);
}

// The glue kernels of t5.hip and i2v.hip, one launch each on plain arguments: the launchers mmpl_t5_encode, mmpl_i2v_* and
// mmpl_clip_visual call.
int mmpl_t5_gather(const int* ids, const void* emb, void* out, int L, int dim, mmpl_stream_t stream) {
  const char* me = "mmpl_t5_gather";
  REJECT(!ids || !emb || !out, me, "null argument");
  REJECT(L < 1 || dim < 1, me, "non-positive size");
  REJECT(dim % 8, me, "dim % 8");
  REJECT(misaligned(emb, 16), me, "emb not 16-byte aligned");
  REJECT(misaligned(out, 16), me, "out not 16-byte aligned");
  REJECT(misaligned(ids, 4), me, "ids not 4-byte aligned");
  LAUNCH(mmpl_launch_t5_gather(ids, (const bf16_t*)emb, (bf16_t*)out, L, dim, (hipStream_t)stream), me);
}

int mmpl_t5_softmax(const float* scores, const void* pos_emb, const int* bucket, const int* mask, void* p, int H, int L,
                    mmpl_stream_t stream) {
  const char* me = "mmpl_t5_softmax";
  REJECT(!scores || !pos_emb || !bucket || !mask || !p, me, "null argument");
  REJECT(H < 1 || L < 1, me, "non-positive size");
  REJECT(L % 64, me, "L % 64");
  REJECT((long)H * L > 0x7fffffffL, me, "H * L exceeds the grid");
  REJECT(misaligned(scores, 4) || misaligned(bucket, 4) || misaligned(mask, 4), me, "scores, bucket or mask not 4-byte aligned");
  REJECT(misaligned(pos_emb, 2) || misaligned(p, 2), me, "pos_emb or p not 2-byte aligned");
  LAUNCH(mmpl_launch_t5_softmax(scores, (const bf16_t*)pos_emb, bucket, mask, (bf16_t*)p, H, L, (hipStream_t)stream), me);
}

int mmpl_t5_transpose(const void* v, int ld, void* vt, int L, int c, int H, mmpl_stream_t stream) {
  const char* me = "mmpl_t5_transpose";
  REJECT(!v || !vt, me, "null argument");
  REJECT(L < 1 || c < 1 || H < 1, me, "non-positive size");
  REJECT((long)ld < (long)H * c, me, "ld < H * c");
  REJECT(H > 65535 || (c + 31) / 32 > 65535, me, "H or c / 32 exceeds the grid");
  REJECT(misaligned(v, 2) || misaligned(vt, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_t5_transpose((const bf16_t*)v, ld, (bf16_t*)vt, L, c, H, (hipStream_t)stream), me);
}

int mmpl_t5_gated(void* f, const void* g, size_t n, mmpl_stream_t stream) {
  const char* me = "mmpl_t5_gated";
  REJECT(!f || !g, me, "null argument");
  REJECT(n < 1, me, "non-positive size");
  REJECT(misaligned(f, 2) || misaligned(g, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_t5_gated((bf16_t*)f, (const bf16_t*)g, n, (hipStream_t)stream), me);
}

int mmpl_t5_zero_pad(void* out, const int* mask, int L, int dim, mmpl_stream_t stream) {
  const char* me = "mmpl_t5_zero_pad";
  REJECT(!out || !mask, me, "null argument");
  REJECT(L < 1 || dim < 1, me, "non-positive size");
  REJECT(misaligned(out, 2), me, "out not 2-byte aligned");
  REJECT(misaligned(mask, 4), me, "mask not 4-byte aligned");
  LAUNCH(mmpl_launch_t5_zero_pad((bf16_t*)out, mask, L, dim, (hipStream_t)stream), me);
}

int mmpl_gelu_erf(void* x, size_t n, mmpl_stream_t stream) {
  const char* me = "mmpl_gelu_erf";
  REJECT(!x, me, "null argument");
  REJECT(n < 1, me, "non-positive size");
  REJECT(misaligned(x, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_gelu_erf((bf16_t*)x, n, (hipStream_t)stream), me);
}

int mmpl_add(void* a, const void* b, size_t n, mmpl_stream_t stream) {
  const char* me = "mmpl_add";
  REJECT(!a || !b, me, "null argument");
  REJECT(n < 1, me, "non-positive size");
  REJECT(misaligned(a, 2) || misaligned(b, 2), me, "misaligned pointer");
  LAUNCH(mmpl_launch_add((bf16_t*)a, (const bf16_t*)b, n, (hipStream_t)stream), me);
}

}  // extern "C"
