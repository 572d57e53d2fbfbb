// TAEHV preview decoder ("Tiny AutoEncoder", the reference's demo_utils/taehv.py, checkpoint taew2_1.pth): host orchestration +
// C ABI (include/mmpl_hip.h, mmpl_taehv_*).  Decoder only.
//
//   Clamp -> conv 16->256 + ReLU -> 3 MemBlock(256) -> [Upsample x2 -> TGrow(256, 1) -> conv 256->128] -> 3 MemBlock(128)
//   -> [Upsample x2 -> TGrow(128, 2) -> conv 128->64] -> 3 MemBlock(64) -> [Upsample x2 -> TGrow(64, 2) -> conv 64->64] -> ReLU
//   -> conv 64->3;  MemBlock(x, past) = ReLU(conv(ReLU(conv(ReLU(conv(cat[x, past]))))) + x), past = the block's input one frame
//   earlier at that level (zeros for a video's first frame).
//
// Latent frames are decoded in groups of up to 3 (1 / 1 / 2 / 4 frames per latent frame at the four levels, see decode_group).
// Each MemBlock owns a run of padded frames [memory, x_0 .. x_{T-1}]: its first conv reads (x_t, x_{t-1}) as two K ranges, its
// last conv adds x_t back and copies x_{T-1} into the memory slot for the next group.  The level change runs TGrow's 1x1 conv
// at the LOW resolution (a 1x1 conv commutes with nearest up-sampling) and folds the up-sampling into the 3x3 conv's source
// addressing.  The nine memories live at fixed offsets of the caller's workspace, so a call is a fixed launch sequence on fixed
// addresses: capturable, and a captured call replays as "the next latent frames".
#include <string>
#include <vector>

#include "../../include/mmpl_hip.h"
#include "taehv_host.h"

namespace {

const int NLEV = 3;
const int CH[4] = {256, 128, 64, 64};      // channels at 1x / 2x / 4x / 8x resolution
const int GROW[3] = {1, 2, 2};             // TGrow stride leaving level l
const int FIRST_BLOCK[3] = {3, 9, 15};     // nn.Sequential index of each level's first MemBlock
const int GROUP = 3;                       // latent frames per launch sequence (the few-step pipeline's block); sizes the workspace

std::vector<std::string> build_names() {
  std::vector<std::string> n;
  auto wb = [&](const std::string& p) { n.push_back(p + ".weight"); n.push_back(p + ".bias"); };
  wb("decoder.1");
  for (int l = 0; l < NLEV; ++l) {
    for (int b = 0; b < 3; ++b)
      for (int c = 0; c < 3; ++c) wb("decoder." + std::to_string(FIRST_BLOCK[l] + b) + ".conv." + std::to_string(2 * c));
    n.push_back("decoder." + std::to_string(FIRST_BLOCK[l] + 4) + ".conv.weight");   // TGrow
    n.push_back("decoder." + std::to_string(FIRST_BLOCK[l] + 5) + ".weight");        // conv to the next level, no bias
  }
  wb("decoder.22");
  return n;
}

}  // namespace

struct MmplTaehv : TaehvHandle {};

namespace {

// n <= GROUP consecutive latent frames -> 4 n pixel frames at t_out of out.  The dry pass (r.dry) only lays the workspace out;
// the layout is that of a full group whatever n is, so every memory keeps its address from call to call.
// The frames of a group go through each layer in ONE launch (n / n / 2n frames at the first three levels): at 480p a single
// frame is 128 blocks at the 256-channel level and 210 at the next -- less than one block per CU.  Only the 8x level (4 frames per
// latent frame, 1560 patches each at 480p) runs one latent frame at a time, so its buffers stay those of one latent frame.
void decode_group(TaehvRun& r, const bf16_t* z, int n, void* out, int fmt, int t_out) {
  int H = r.v->lat_h, W = r.v->lat_w, T = n, Ta = GROUP;     // frames at this level: this call's, and the layout's
  r.rewind();
  size_t fs, fz;
  bf16_t* zin = r.frames(Ta, H, W, 32, &fz);
  // x: where the current level's first MemBlock finds its input frames (slot 0 of each run is the memory)
  bf16_t* x = r.frames(1 + Ta, H, W, CH[0], &fs);
  if (!r.dry)
    for (int i = 0; i < n; ++i) r.chk(taehv_launch_prep(z + (size_t)i * 16 * H * W, zin + i * fz, H, W, r.s), "taehv prep");
  {
    TaehvConvArgs g = {};
    g.src0 = zin; g.fs0 = fz; g.C0 = 32; g.ntaps = 9; g.Wfrag = r.next_w(); g.bias = r.next_w(); g.Nw = g.N = g.Nsplit = g.ldd = CH[0];
    g.T = T; g.Ho = H; g.Wo = W; g.dst = x + fs; g.fsd = fs; g.relu = 1;
    r.conv(g);
  }
  for (int l = 0; l < NLEV; ++l) {
    const int C = CH[l];
    bf16_t* t1 = r.frames(Ta, H, W, C);
    bf16_t* t2 = r.frames(Ta, H, W, C);
    for (int b = 0; b < 3; ++b) x = memblock(r, x, t1, t2, fs, C, T, Ta, H, W, b == 2);
    // level change: TGrow at this resolution (C -> GROW * C channels = GROW frames), then the up-sampling 3x3 conv
    const int S = GROW[l], Cn = CH[l + 1];
    bf16_t* grown = r.frames(Ta * S, H, W, C);
    {
      TaehvConvArgs g = {};
      g.src0 = x; g.fs0 = fs; g.C0 = C; g.ntaps = 1; g.Wfrag = r.next_w(); g.Nw = g.N = S * C; g.Nsplit = g.ldd = C;
      g.T = T; g.Ho = H; g.Wo = W; g.dst = grown; g.fsd = fs;
      r.conv(g);
    }
    T *= S; Ta *= S; H *= 2; W *= 2;
    TaehvConvArgs g = {};
    g.fs0 = fs; g.C0 = C; g.up = 1; g.ntaps = 9; g.Wfrag = r.next_w(); g.Nw = g.N = g.Nsplit = g.ldd = Cn; g.Ho = H; g.Wo = W;
    if (l < NLEV - 1) {
      size_t fsn;
      bf16_t* nx = r.frames(1 + Ta, H, W, Cn, &fsn);
      g.src0 = grown; g.T = T; g.dst = nx + fsn; g.fsd = fsn;
      r.conv(g);
      x = nx;
      fs = fsn;
      continue;
    }
    // the 8x level, one latent frame (4 frames) at a time: conv 64->64 + the ReLU in front of the head, the head, the output format
    const int per = T / n;
    size_t f8, fh;
    bf16_t* full = r.frames(per, H, W, Cn, &f8);
    bf16_t* head = r.frames(per, H, W, 4, &fh);
    const bf16_t* wh = r.next_w();
    const bf16_t* bh = r.next_w();
    for (int i = 0; i < n; ++i) {
      g.src0 = grown + (size_t)i * per * fs; g.T = per; g.dst = full; g.fsd = f8; g.relu = 1;
      r.conv(g);
      TaehvConvArgs q = {};
      q.src0 = full; q.fs0 = f8; q.C0 = Cn; q.ntaps = 9; q.Wfrag = wh; q.bias = bh; q.Nw = q.Nsplit = 16; q.N = q.ldd = 4;
      q.T = per; q.Ho = H; q.Wo = W; q.dst = head; q.fsd = fh;
      r.conv(q);
      if (!r.dry) r.chk(taehv_launch_px_out(head, out, fmt, per, H, W, t_out + per * i, r.s), "taehv px_out");
    }
  }
}

size_t layout_bytes(TaehvHandle* v) {
  TaehvRun r(v, nullptr, nullptr, "taehv conv");
  decode_group(r, nullptr, GROUP, nullptr, 0, 0);
  return r.k.off;
}

}  // namespace

extern "C" {

int mmpl_taehv_num_weights(void) { return (int)build_names().size(); }

const char* mmpl_taehv_weight_name(int i) {
  static std::vector<std::string> names = build_names();
  return (i >= 0 && i < (int)names.size()) ? names[i].c_str() : nullptr;
}

int mmpl_taehv_create(int lat_h, int lat_w, MmplTaehv** out) {
  if (!out || lat_h < 1 || lat_w < 1) return mmpl_set_error("mmpl_taehv_create", "bad arguments");
  *out = taehv_new<MmplTaehv>(lat_h, lat_w, layout_bytes);
  return 0;
}

void mmpl_taehv_destroy(MmplTaehv* v) { delete v; }

int mmpl_taehv_bind_weights(MmplTaehv* v, const void* const* ptrs, int n) {
  return taehv_bind(v, ptrs, n, mmpl_taehv_num_weights(), "mmpl_taehv_bind_weights");
}

size_t mmpl_taehv_workspace_bytes(MmplTaehv* v) { return v ? v->need : 0; }

int mmpl_taehv_reset(MmplTaehv* v) { return taehv_reset(v, "mmpl_taehv_reset"); }

int mmpl_taehv_decode(MmplTaehv* v, const void* z, int n_frames, void* out, int out_format, int* n_px_frames_out, void* ws,
                      size_t ws_bytes, mmpl_stream_t stream) {
  if (!v) return mmpl_set_error("mmpl_taehv_decode", "null argument");
  if (v->w.empty()) return mmpl_set_error("mmpl_taehv_decode", "weights not bound");
  if (n_frames < 1) return mmpl_set_error("mmpl_taehv_decode", "n_frames < 1");
  if (out_format != 0 && out_format != 1) return mmpl_set_error("mmpl_taehv_decode", "unknown out_format");
  if (!z || !out) return mmpl_set_error("mmpl_taehv_decode", "null argument");
  if (taehv_bind_workspace(v, ws, ws_bytes, (hipStream_t)stream, "mmpl_taehv_decode")) return 1;
  TaehvRun r(v, ws, (hipStream_t)stream, "taehv conv");
  const size_t zf = (size_t)16 * v->lat_h * v->lat_w;
  for (int i = 0; i < n_frames; i += GROUP)
    decode_group(r, (const bf16_t*)z + i * zf, n_frames - i < GROUP ? n_frames - i : GROUP, out, out_format, 4 * i);
  if (n_px_frames_out) *n_px_frames_out = 4 * n_frames;
  return r.report();
}

}  // extern "C"
