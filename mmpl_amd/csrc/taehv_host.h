// What the TAEHV decoder (taehv.hip) and encoder (taehv_enc.hip) share on the host: the handle, the state of one call's launch
// sequence, the MemBlock and the bodies of create / bind / reset / "first call of a video".  Each side keeps its own level logic.
#pragma once
#include "host_util.h"
#include "taehv_kernels.h"

// MmplTaehv and MmplTaehvEnc derive from this, so the two opaque ABI types stay distinct.
struct TaehvHandle {
  int lat_h = 0, lat_w = 0;
  std::vector<const bf16_t*> w;
  size_t need = 0;
  void* ws = nullptr;     // the workspace the current video's memories live in; null = none yet (after create / reset)
};

// One call's walk over the network.  The dry pass (no workspace, no launches) only lays the workspace out.
struct TaehvRun : ErrLatch {
  TaehvHandle* v;
  Carver k;
  hipStream_t s;
  bool dry;
  const char* conv_where;   // how a failed conv launch is reported
  int wi = 0;               // next weight slot, in build_names() order
  TaehvRun(TaehvHandle* v_, void* ws, hipStream_t s_, const char* conv_where_) : v(v_), k(ws), s(s_), dry(ws == nullptr), conv_where(conv_where_) {}
  void rewind() { k.off = 0; wi = 0; }        // every group starts at the same offsets and the first weight
  // n zero-bordered channels-last frames [H + 2][W + 2][C]
  bf16_t* frames(int n, int H, int W, int C, size_t* stride = nullptr) {
    const size_t fr = (size_t)(H + 2) * (W + 2) * C;
    if (stride) *stride = fr;
    return k.take<bf16_t>(n * fr);
  }
  const bf16_t* next_w() { return dry ? nullptr : v->w[wi++]; }
  void conv(TaehvConvArgs& g) {
    if (!dry) chk(taehv_launch_conv(g, s), conv_where);
  }
};

// MemBlock(x, past) = ReLU(conv(ReLU(conv(ReLU(conv(cat[x, past]))))) + x) over T frames of C channels.  x is the block's run
// [memory, x_0 .. x_{Ta-1}] (frame stride fs), t1 / t2 the level's two scratch runs.  The first conv reads (x_t, x_{t-1}) as two K
// ranges, the last one adds x_t back and copies x_{T-1} into the memory slot for the next group.  The output is carved here: the
// next block's run, or after the last block of a level a plain run of Ta frames.  Returns where the next layer finds its input.
inline bf16_t* memblock(TaehvRun& r, bf16_t* x, bf16_t* t1, bf16_t* t2, size_t fs, int C, int T, int Ta, int H, int W, bool last_of_level) {
  bf16_t* y = last_of_level ? r.frames(Ta, H, W, C) : r.frames(1 + Ta, H, W, C) + fs;
  TaehvConvArgs g = {};
  g.ntaps = 9; g.Nw = g.N = g.Nsplit = g.ldd = C; g.T = T; g.Ho = H; g.Wo = W; g.fsd = (long)fs; g.relu = 1;
  TaehvConvArgs c1 = g, c2 = g, c3 = g;
  c1.src0 = x + fs; c1.src1 = x; c1.fs0 = c1.fs1 = (long)fs; c1.C0 = c1.C1 = C; c1.Wfrag = r.next_w(); c1.bias = r.next_w(); c1.dst = t1;
  c2.src0 = t1; c2.fs0 = (long)fs; c2.C0 = C; c2.Wfrag = r.next_w(); c2.bias = r.next_w(); c2.dst = t2;
  c3.src0 = t2; c3.fs0 = (long)fs; c3.C0 = C; c3.Wfrag = r.next_w(); c3.bias = r.next_w(); c3.dst = y;
  c3.skip = x + fs; c3.fss = (long)fs; c3.keep = x;
  r.conv(c1); r.conv(c2); r.conv(c3);
  return last_of_level ? y : y - fs;
}

// The bodies of mmpl_taehv[_enc]_{create, bind_weights, reset}; `me` is the entry's name in the error text
template <class Handle>
Handle* taehv_new(int lat_h, int lat_w, size_t (*layout_bytes)(TaehvHandle*)) {
  Handle* v = new Handle();
  v->lat_h = lat_h;
  v->lat_w = lat_w;
  v->need = layout_bytes(v);
  return v;
}
inline int taehv_bind(TaehvHandle* v, const void* const* ptrs, int n, int want, const char* me) {
  if (!v || !ptrs) return mmpl_set_error(me, "wrong pointer count");
  return bind_weight_ptrs(v->w, ptrs, n, want, me);
}
inline int taehv_reset(TaehvHandle* v, const char* me) {
  if (!v) return mmpl_set_error(me, "null argument");
  v->ws = nullptr;          // the next call binds a workspace again and clears it: zero memories
  return 0;
}
// The last checks of a decode / encode call, and on the first call of a video the zeroed memories (and frame borders).
inline int taehv_bind_workspace(TaehvHandle* v, void* ws, size_t ws_bytes, hipStream_t s, const char* me) {
  if (!ws || ws_bytes < v->need) return mmpl_set_error(me, "workspace too small");
  if (v->ws && v->ws != ws) return mmpl_set_error(me, "workspace differs from the one this video's memories live in (reset first)");
  if (!v->ws) {
    if (hipMemsetAsync(ws, 0, v->need, s) != hipSuccess) return mmpl_set_error(me, "memset failed");
    v->ws = ws;
  }
  return 0;
}
