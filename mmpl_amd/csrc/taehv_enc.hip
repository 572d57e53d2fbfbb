// TAEHV encoder (the reference's demo_utils/taehv.py, TAEHV.encode_video, checkpoint taew2_1.pth): host orchestration + C ABI
// (include/mmpl_hip.h, mmpl_taehv_enc_* / mmpl_taehv_encode).  The mirror of taehv.hip.
//
//   conv 3->64 + ReLU -> [TPool(2) -> conv 64->64 stride 2] -> 3 MemBlock(64) -> [TPool(2) -> conv stride 2] -> 3 MemBlock(64)
//   -> [TPool(1) -> conv stride 2] -> 3 MemBlock(64) -> conv 64->16;  TPool(s) = a bias-free 1x1 conv over s consecutive frames
//   concatenated on the channel axis; MemBlock as in the decoder, past = the block's input one frame earlier at that level.
//
// Pixel frames are encoded in groups of up to 3 latent frames (12 pixel frames; 6 / 3 / 3 frames at the 1/2, 1/4 and 1/8 levels).
// The full-resolution level -- the input layer, the first TPool and the first stride-2 conv -- runs one latent frame's 4 pixel
// frames at a time, so only 4 + 2 full-resolution 64-channel frames ever exist; its 2 output frames land in the run of the first
// MemBlock, which then sees the whole group in one launch per layer.  TPool is the decoder's 1x1 conv with the even frame as src0
// and the odd one as src1 (a call takes a multiple of 4 frames, so a pair never straddles two calls).  Each MemBlock owns a run of
// padded frames [memory, x_0 .. x_{T-1}] exactly as in taehv.hip.  The nine memories live at fixed offsets of the caller's
// workspace, so a call is a fixed launch sequence on fixed addresses: capturable, and a captured call replays as "the next frames".
#include <string>
#include <vector>

#include "../../include/mmpl_hip.h"
#include "taehv_host.h"

namespace {

const int NLEV = 3, C = 64;
const int POOL[3] = {2, 2, 1};             // TPool stride entering level l
const int FIRST[3] = {2, 7, 12};           // nn.Sequential index of each level's TPool (then the stride-2 conv, then 3 MemBlocks)
const int GROUP = 3;                       // latent frames per launch sequence; sizes the workspace

std::vector<std::string> build_names() {
  std::vector<std::string> n;
  auto wb = [&](const std::string& p) { n.push_back(p + ".weight"); n.push_back(p + ".bias"); };
  wb("encoder.0");
  for (int l = 0; l < NLEV; ++l) {
    n.push_back("encoder." + std::to_string(FIRST[l]) + ".conv.weight");       // TPool
    n.push_back("encoder." + std::to_string(FIRST[l] + 1) + ".weight");        // stride-2 conv, no bias
    for (int b = 0; b < 3; ++b)
      for (int c = 0; c < 3; ++c) wb("encoder." + std::to_string(FIRST[l] + 2 + b) + ".conv." + std::to_string(2 * c));
  }
  wb("encoder.17");
  return n;
}

}  // namespace

struct MmplTaehvEnc : TaehvHandle {};

namespace {

// TPool(S) over T output frames: frame t = W . cat[src frame S t, .., S t + S - 1]
void tpool(TaehvRun& r, const bf16_t* src, size_t fs, int S, const bf16_t* wf, int T, int H, int W, bf16_t* dst) {
  TaehvConvArgs g = {};
  g.src0 = src; g.fs0 = (long)(S * fs); g.C0 = C; g.ntaps = 1; g.Wfrag = wf; g.Nw = g.N = g.Nsplit = g.ldd = C;
  if (S == 2) { g.src1 = src + fs; g.fs1 = (long)(2 * fs); g.C1 = C; }
  g.T = T; g.Ho = H; g.Wo = W; g.dst = dst; g.fsd = (long)fs;
  r.conv(g);
}
void conv_s2(TaehvRun& r, const bf16_t* src, size_t fs, const bf16_t* wf, int T, int Ho, int Wo, bf16_t* dst, size_t fsd) {
  TaehvConvS2Args g = {};
  g.src = src; g.fs = (long)fs; g.C = C; g.Wfrag = wf; g.Nw = C; g.T = T; g.Ho = Ho; g.Wo = Wo; g.dst = dst; g.fsd = (long)fsd;
  if (!r.dry) r.chk(taehv_launch_conv_s2(g, r.s), "taehv_enc conv_s2");
}

// 4 n pixel frames (n <= GROUP latent frames) -> n latent frames at f_out of z_out.  The dry pass (r.dry) only lays the workspace
// out; the layout is that of a full group whatever n is, so every memory keeps its address from call to call.
void encode_group(TaehvRun& r, const void* px, int fmt, int n, bf16_t* z_out, int f_out) {
  const int h = r.v->lat_h, w = r.v->lat_w;
  int H = 8 * h, W = 8 * w;
  r.rewind();
  // the full-resolution level, one latent frame (4 pixel frames) at a time
  size_t f8, fs;
  bf16_t* full = r.frames(4, H, W, C, &f8);
  bf16_t* half = r.frames(2, H, W, C);
  const bf16_t* w_in = r.next_w();
  const bf16_t* b_in = r.next_w();
  const bf16_t* w_pool = r.next_w();
  const bf16_t* w_s2 = r.next_w();
  int T = 2 * n, Ta = 2 * GROUP;            // frames at the current level: this call's, and the layout's
  // x: where the current level's first MemBlock finds its input frames (slot 0 of each run is the memory)
  bf16_t* x = r.frames(1 + Ta, H / 2, W / 2, C, &fs);
  const size_t px_stride = (size_t)4 * 3 * H * W * (fmt == 0 ? sizeof(float) : 1);
  for (int i = 0; i < n; ++i) {
    TaehvConvInArgs g = {};
    g.px = (const char*)px + (size_t)i * px_stride; g.fmt = fmt; g.Wfrag = w_in; g.bias = b_in; g.T = 4; g.H = H; g.W = W;
    g.dst = full; g.fsd = (long)f8;
    if (!r.dry) r.chk(taehv_launch_conv_in(g, r.s), "taehv_enc conv_in");
    tpool(r, full, f8, 2, w_pool, 2, H, W, half);
    conv_s2(r, half, f8, w_s2, 2, H / 2, W / 2, x + fs * (1 + 2 * i), fs);
  }
  H /= 2; W /= 2;
  for (int l = 0; l < NLEV; ++l) {
    bf16_t* t1 = r.frames(Ta, H, W, C);
    bf16_t* t2 = r.frames(Ta, H, W, C);
    for (int b = 0; b < 3; ++b) x = memblock(r, x, t1, t2, fs, C, T, Ta, H, W, b == 2);
    if (l == NLEV - 1) break;
    // level change: TPool at this resolution, then the stride-2 conv into the next level's first run
    const int S = POOL[l + 1];
    bf16_t* pooled = r.frames(Ta / S, H, W, C);
    tpool(r, x, fs, S, r.next_w(), T / S, H, W, pooled);
    T /= S; Ta /= S; H /= 2; W /= 2;
    size_t fsn;
    bf16_t* nx = r.frames(1 + Ta, H, W, C, &fsn);
    conv_s2(r, pooled, fs, r.next_w(), T, H, W, nx + fsn, fsn);
    x = nx;
    fs = fsn;
  }
  // the head: conv 64->16 + bias, then planar latents
  size_t fz;
  bf16_t* head = r.frames(Ta, H, W, 16, &fz);
  TaehvConvArgs q = {};
  q.src0 = x; q.fs0 = (long)fs; q.C0 = C; q.ntaps = 9; q.Wfrag = r.next_w(); q.bias = r.next_w(); q.Nw = q.Nsplit = q.N = q.ldd = 16;
  q.T = T; q.Ho = H; q.Wo = W; q.dst = head; q.fsd = (long)fz;
  r.conv(q);
  if (!r.dry) r.chk(taehv_launch_z_out(head, z_out, T, H, W, f_out, r.s), "taehv_enc z_out");
}

size_t layout_bytes(TaehvHandle* v) {
  TaehvRun r(v, nullptr, nullptr, "taehv_enc conv");
  encode_group(r, nullptr, 0, GROUP, nullptr, 0);
  return r.k.off;
}

}  // namespace

extern "C" {

int mmpl_taehv_enc_num_weights(void) { return (int)build_names().size(); }

const char* mmpl_taehv_enc_weight_name(int i) {
  static std::vector<std::string> names = build_names();
  return (i >= 0 && i < (int)names.size()) ? names[i].c_str() : nullptr;
}

int mmpl_taehv_enc_create(int lat_h, int lat_w, MmplTaehvEnc** out) {
  if (!out || lat_h < 1 || lat_w < 1 || lat_h > 4096 || lat_w > 4096) return mmpl_set_error("mmpl_taehv_enc_create", "bad arguments");
  *out = taehv_new<MmplTaehvEnc>(lat_h, lat_w, layout_bytes);
  return 0;
}

void mmpl_taehv_enc_destroy(MmplTaehvEnc* v) { delete v; }

int mmpl_taehv_enc_bind_weights(MmplTaehvEnc* v, const void* const* ptrs, int n) {
  return taehv_bind(v, ptrs, n, mmpl_taehv_enc_num_weights(), "mmpl_taehv_enc_bind_weights");
}

size_t mmpl_taehv_enc_workspace_bytes(MmplTaehvEnc* v) { return v ? v->need : 0; }

int mmpl_taehv_enc_reset(MmplTaehvEnc* v) { return taehv_reset(v, "mmpl_taehv_enc_reset"); }

int mmpl_taehv_encode(MmplTaehvEnc* v, const void* px, int in_format, int n_frames, void* z_out, int* n_latents_out, void* ws,
                      size_t ws_bytes, mmpl_stream_t stream) {
  const char* me = "mmpl_taehv_encode";
  if (!v) return mmpl_set_error(me, "null argument");
  if (v->w.empty()) return mmpl_set_error(me, "weights not bound");
  if (n_frames < 4 || n_frames % 4) return mmpl_set_error(me, "n_frames must be a multiple of 4, at least 4");
  if (in_format != 0 && in_format != 1) return mmpl_set_error(me, "unknown in_format");
  if (!px || !z_out) return mmpl_set_error(me, "null argument");
  if (taehv_bind_workspace(v, ws, ws_bytes, (hipStream_t)stream, me)) return 1;
  TaehvRun r(v, ws, (hipStream_t)stream, "taehv_enc conv");
  const int n_lat = n_frames / 4;
  const size_t pf = (size_t)3 * 64 * v->lat_h * v->lat_w * (in_format == 0 ? sizeof(float) : 1);   // bytes of one pixel frame
  for (int i = 0; i < n_lat; i += GROUP)
    encode_group(r, (const char*)px + (size_t)4 * i * pf, in_format, n_lat - i < GROUP ? n_lat - i : GROUP, (bf16_t*)z_out, i);
  if (n_latents_out) *n_latents_out = n_lat;
  return r.report();
}

}  // extern "C"
