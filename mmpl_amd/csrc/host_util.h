// Host-side scaffolding shared by every engine's orchestration (api.hip, t5.hip, vae.hip, taehv*.hip, i2v.hip): workspace carving,
// weight binding, first-error capture and the three launcher argument structs that are filled in many places.  Host only, header only.
#pragma once
#include <stddef.h>

#include <vector>

#include "kernels.h"
#include "mmpl_error.h"

inline size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// Hands out consecutive 256-byte-aligned pieces of a caller's workspace.  With a null base it only counts (a size query).
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <class T> T* take(size_t elems) {
    T* p = (T*)(base + off);
    off += round256(elems * sizeof(T));
    return p;
  }
};

// The body of every mmpl_*_bind_weights: w is replaced only when all n == want pointers are there, so a refused bind leaves the
// handle as it was (still unbound if it was unbound).
inline int bind_weight_ptrs(std::vector<const bf16_t*>& w, const void* const* ptrs, int n, int want, const char* where) {
  if (!ptrs) return mmpl_set_error(where, "null argument");
  if (n != want) return mmpl_set_error(where, "wrong pointer count");
  for (int i = 0; i < n; ++i)
    if (!ptrs[i]) return mmpl_set_error(where, "null weight pointer");
  w.assign((const bf16_t* const*)ptrs, (const bf16_t* const*)ptrs + n);
  return 0;
}

// The first failed HIP call of a launch sequence that runs to its end whatever happens, and where it was.
struct ErrLatch {
  hipError_t err = hipSuccess;
  const char* where = "";
  void chk(hipError_t e, const char* w) { if (e != hipSuccess && err == hipSuccess) { err = e; where = w; } }
  int report() const { return err == hipSuccess ? 0 : mmpl_set_error(where, hipGetErrorString(err)); }
};

// C = epi(A . W^T + bias) with every other field at its neutral value: zero, but alpha = 1 and one row per frame.  Callers set the
// rest by name, so a field added to GemmArgs moves no call site.
inline GemmArgs gemm_args(const bf16_t* A, int lda, const bf16_t* W, int ldw, const bf16_t* bias, bf16_t* C, int ldc, int M, int N, int K,
                          int epi) {
  GemmArgs g = {};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.epi = epi;
  g.rows_per_frame = 1;
  g.alpha = 1.0f;
  return g;
}

// LayerNorm of x into y; the caller names its form: (scale, shift, mod_frame_stride, rows_per_frame) or (w, b).
inline LnArgs ln_args(const bf16_t* x, int ldx, bf16_t* y, int ldy, int rows, int d, float eps) {
  LnArgs a = {};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.rows = rows; a.d = d; a.eps = eps;
  a.rows_per_frame = 1;
  return a;
}

// o = softmax(scale . q k^T) v over H heads of 128, Lq query rows, pages of page_rows rows; everything else zero.  The caller names
// its pages (n_pages, k_pages, v_pages, page_group) and whatever else the launch uses.
inline AttnArgs attn_args(const bf16_t* q, int ldq, bf16_t* o, int ldo, int ldk, int ldv, int page_rows, int Lq, int H, float scale) {
  AttnArgs a = {};
  a.q = q; a.ldq = ldq; a.o = o; a.ldo = ldo; a.ldk = ldk; a.ldv = ldv; a.page_rows = page_rows; a.Lq = Lq; a.H = H; a.scale = scale;
  return a;
}
