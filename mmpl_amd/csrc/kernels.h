// Internal launcher interface between the C-ABI layer (api.hip) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

// ---------------------------------------------------------------- per-device launcher state (device_state.hip)
hipError_t mmpl_dyn_smem_once(const void* func, int bytes);   // hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel)
int mmpl_cus_per_xcd();                                       // CUs / 8 of the current device

// ---------------------------------------------------------------- GEMM (gemm.hip)
enum GemmEpi { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_SILU = 2, EPI_GATE_RES = 3, EPI_RES = 4, EPI_F32_SCALE = 5,
               EPI_BIAS_VPAGES = 6 };   // bias; columns >= v_col0 go to per-frame pages instead of C (the V third of the fused qkv)
struct GemmArgs {
  const bf16_t* A; int lda;      // [M, K]
  const bf16_t* W; int ldw;      // [N, K]  (nn.Linear weight)
  const bf16_t* bias;            // [N] or null
  bf16_t* C; int ldc;            // [M, N]
  int M, N, K;
  int epi;
  const bf16_t* res; int ldres;  // residual x for EPI_GATE_RES / EPI_RES (may alias C)
  const bf16_t* gate;            // per-frame gate vectors: gate[frame * gate_frame_stride + n]
  int gate_frame_stride;
  int rows_per_frame;
  float alpha;                   // EPI_F32_SCALE: C is float*, C = alpha * acc (no bias)
  int group;                     // M-tile group size of the block order (set by the launcher)
  int batch;                     // > 1: batched (blockIdx.y); element strides below; small-problem kernel only
  long sA, sW, sC;
  // EPI_BIAS_VPAGES: row m, column n >= v_col0 is written to v_dst[m / rows_per_frame] + (m % rows_per_frame) * v_ld + n - v_col0
  bf16_t* v_dst[8]; int v_col0, v_ld;
  int staged_epilogue;           // v6: LDS-staged 16-byte epilogue (set by the launcher when every pointer / stride allows it)
  // v6, optional: 8 device ints (one per XCD), zero when the launch starts and left zero by it.  With it the kernel is launched
  // once per CU and its blocks take tiles of their XCD's share from these tickets until none is left (gemm.hip); the
  // launches that share a counter must be ordered (one stream).  Null: one block per tile.
  int* tile_counter;
  int pf_dist;                   // v6: L2 prefetch distance in k-tiles (0 = off; set by the launcher)
  int sync_sweeps;               // v6: deal whole M-groups to the XCDs so that all of them sweep W's column panels together (set by the launcher)
  // v6, optional (needs tile_counter too): scratch for the split-K launch of the partial last round of tiles (gemm.hip).
  // splitk_ws: mmpl_gemm_splitk_ws_bytes() of fp32 partials; splitk_cnt: 256 device ints, zero when a launch starts and left zero.
  float* splitk_ws; int* splitk_cnt;
  int splitk_s, splitk_tb, splitk_per;   // set by the launcher: parts per tile (1 = no split), tail tiles per XCD (max), CUs per XCD
};
size_t mmpl_gemm_splitk_ws_bytes();
// What mmpl_launch_gemm does with a GemmArgs: every choice of the launchers is made by mmpl_gemm_plan and nowhere else (the launchers
// read it from the plan; mmpl_gemm_ex reports it to the tests).  Pure host arithmetic except for the CU count of the current device,
// which is looked up only when the 256 x 256 kernels are chosen.
enum GemmKernel { GEMM_KERNEL_SMALL = 1, GEMM_KERNEL_V2 = 2, GEMM_KERNEL_V6 = 3, GEMM_KERNEL_V8 = 4 };
enum GemmTail { GEMM_TAIL_NONE = 0, GEMM_TAIL_SPLITK = 1,
                GEMM_TAIL_128_8 = 2,    // gemm_tail128_kernel<EPI, true>: the DMA-ring body, 8 tile buffers of LDS, one block per CU
                GEMM_TAIL_128_4 = 3 };  // gemm_tail128_kernel<EPI, false>: the register-staged body, 4 tile buffers, two blocks per CU
struct GemmPlan {
  int kernel;             // GemmKernel of the main launch (also when the main launch is skipped: the kernel whose tile order the tail follows)
  int tail;               // GemmTail: the second launch for the partial last round of tiles
  int staged_epilogue;    // v6 / v8 (and the split-K tail): LDS-staged 16-byte epilogue; 0 = the direct 8-byte one
  int main_blocks;        // blocks of the main launch (small kernel: tiles x batch); 0 = the main launch is skipped
  int tail_blocks;        // blocks of the tail launch (0 without a tail)
  int splitk_s;           // parts per tail tile of the split-K launch (1 = no split; GemmArgs.splitk_s is 4 for a 128 x 128 tail as well)
  // the rest is what the launchers need beside the above
  int tickets;            // the main launch draws its tiles from GemmArgs.tile_counter (persistent blocks)
  int group;              // GemmArgs.group
  int tail_tiles;         // GemmArgs.splitk_tb: tail tiles per XCD (max)
  int cus_per_xcd;        // GemmArgs.splitk_per
};
GemmPlan mmpl_gemm_plan(const GemmArgs& g);
bool mmpl_xcd_dispatch_ok(bool may_probe);   // device_state.hip: workgroup b runs on XCD b & 7 (probed once per device, never inside a capture)
hipError_t mmpl_launch_gemm(const GemmArgs& g, hipStream_t s);

// ---------------------------------------------------------------- attention (attention.hip)
constexpr int MMPL_MAX_PAGES = 24;
constexpr int ATTN_QB = 256, ATTN_KVB = 64;            // query rows per block (work item), rows per KV tile: every attention kernel
constexpr float ATTN_LOG2E = 1.4426950408889634f;      // the kernels compute p = exp2((s - m) * scale * log2(e))
struct AttnArgs {
  const bf16_t* q; int ldq;       // row r, head h at q + r*ldq + h*128
  bf16_t* o; int ldo;
  const bf16_t* k_pages[MMPL_MAX_PAGES];   // page p: row j, head h at k_pages[p] + j*ldk + h*128
  const bf16_t* v_pages[MMPL_MAX_PAGES];
  int ldk, ldv;
  int n_pages, page_rows;
  int page_rows_each[MMPL_MAX_PAGES];   // attn_w64_kernel only, filled by mmpl_launch_attention: rows of page p (merged runs of slots differ in length)
  // host side only (merge_contiguous_pages): which ALLOCATION page p lies in, as the caller knows it (the DiT forward: 0 = KV-cache
  // slots, 1 = the stage's scratch pages).  Pages are ordered by (group, address) and merged within a group only, so the order and
  // the tile boundaries the kernel sees -- hence the fp32 summation order, hence the bits -- do not depend on where the allocator
  // happened to put one allocation relative to another (a fresh process and a long-lived one must agree: tests/test_wavefront_gpu.py).
  unsigned char page_group[MMPL_MAX_PAGES];
  int Lq, H;
  float scale;                     // softmax scale (1/sqrt(128))
  int cross;                       // 1: text cross-attention launch (symbol tag only)
  float* split_ws; size_t split_ws_bytes;   // optional scratch for the split-KV tail round (nullptr: never split)
  int variant;                     // ATTN_* kernel selector (0 = auto)
  int q_prescaled;                 // q was already multiplied by scale * log2(e) by its producer (ATTN_W64 only)
  // attn_fwd_kernel with ONE page only: the page's last row stands for `last_row_copies` identical keys (same K row, same V row):
  // its score gets + ln(copies) / scale, i.e. its softmax weight is multiplied by copies.  0 / 1 = a plain row.
  int last_row_copies;
  // attn_w64_kernel, optional: five device counters {blocks run, blocks whose FAST pass failed and were redone by the GENERAL pass,
  // WAVES (64 query rows) that held a failing row themselves, blocks their history sent straight to the GENERAL pass, blocks whose
  // FAST pass held on the references their history remembered} (how data-dependent is the kernel's time on THIS input? -- bench.py --heavy-tail)
  unsigned long long* redo_stats;
  // attn_w64_kernel, optional: mmpl_attn_history_bytes(Lq, H) bytes carried by the caller from one launch to the next launch of the same
  // attention (same layer, CFG branch and stage shape); all zero = no history.  [H * ceil(Lq / 256) * 4] state bytes (head, query block,
  // split part), padded to 256 B, then per state byte 128 int16 lane references (attn_w64.hip).  nullptr: stateless.
  unsigned char* history;
  short* history_mem;              // set by mmpl_launch_attention: history + the padded state bytes
};
// Work item `local` of XCD `xcd` -> (head, query block) for attn_w64_kernel / attn_merge_kernel (the hardware deals workgroups
// round-robin to the 8 XCDs: blockIdx & 7).  H % 8 == 0: XCD x owns heads x, x+8, ...; any other head count (Wan 1.3B: 12):
// XCD x owns the x-th contiguous chunk of ceil(n_qb*H / 8) items of the head-major (head, query block) list, so the blocks
// sharing one L2 work on at most a few heads; false = past the end of the list (the last XCD's chunk can be short).
__device__ __forceinline__ bool mmpl_attn_item(int H, int n_qb, int xcd, int local, int& head, int& qb) {
  if ((H & 7) == 0) {
    head = xcd + 8 * (local / n_qb);
    qb = local % n_qb;
    return head < H;
  }
  const int total = n_qb * H, per = (total + 7) >> 3, item = xcd * per + local;
  if (local >= per || item >= total) return false;
  head = item / n_qb;
  qb = item % n_qb;
  return true;
}
// Grouped launch of attn_w64_kernel (attn_w64_groups.hip): n_groups independent attentions of equal shape in ONE launch -- the
// samples of a batched few-step forward, whose query rows must see their own sample's cache slots only.  `a` is an ordinary AttnArgs
// with Lq = the rows of ONE group (any count: every group has ceil(Lq / 256) query blocks of its own, the last one partial, no block
// straddles two groups); group g's queries are rows g * Lq .. of a.q / a.o, and it walks pages page_first[g] .. page_first[g + 1] - 1
// of a.k_pages / a.v_pages / a.page_rows_each (each group's list merged and ordered by itself; a.n_pages = page_first[n_groups] <=
// MMPL_MAX_PAGES).  (group, head) is a virtual head of mmpl_attn_item's decode: n_groups * H of them.  Stateless: a.history is NULL.
// A second struct, not fields of AttnArgs: an ungrouped launch carries and runs exactly what it did before this existed.
constexpr int MMPL_MAX_GROUPS = 8;
struct AttnGroupArgs {
  AttnArgs a;
  int n_groups;
  int page_first[MMPL_MAX_GROUPS + 1];
};
// The split-KV partial of one (tail query block, KV part): what a split block of attn_w64_kernel writes and attn_merge_kernel reads.
// FLOATS fp32: O of query row r (relative to the part's reference m) at o(r) .. + 128, then m (raw score units) and l of the 256
// rows at m(r) and l(r).  split_ws holds them as [tail block][part].
struct AttnPartial {
  static constexpr int FLOATS = ATTN_QB * (128 + 2);
  static constexpr size_t BYTES = FLOATS * sizeof(float);
  static constexpr size_t o(int r) { return (size_t)r * 128; }
  static constexpr int m(int r) { return ATTN_QB * 128 + r; }
  static constexpr int l(int r) { return ATTN_QB * 129 + r; }
};
enum { ATTN_AUTO = 0, ATTN_LOCKSTEP = 1, ATTN_W64 = 3 };      // (2 was the round-1 ping-pong kernel, removed)
// The kernel ATTN_AUTO resolves to for a self-attention launch whose producer can fold the softmax scale into q before q is
// rounded to bf16 (the DiT forward: qknorm_kernel's q_scale).  ATTN_W64 computes exp2(K.q) without a per-score multiply, so it
// wants q = bf16(q_fp32 * scale * log2(e)); handing it a bf16 q to prescale itself costs a second rounding of q, which shows
// on sharp softmax rows (large QK-norm gains) -- a raw-q ATTN_AUTO launch (the attention() seam) therefore takes ATTN_LOCKSTEP.
int mmpl_attention_self_variant();
// attn_w64.hip (4 waves x 64 query rows, one wave per SIMD): the kernel pair {whole KV range, one split-KV part} that takes Args
// (+ local_base, sp).  AttnArgs: attn_w64.hip; AttnGroupArgs: attn_w64_groups.hip, the grouped instantiations of the same body.
int mmpl_attention_w64_smem();
template <class Args> struct AttnW64Kernels { void (*split)(Args, int, int); void (*main)(Args, int, int); };
template <class Args> AttnW64Kernels<Args> mmpl_attention_w64_kernels();
inline size_t mmpl_attention_split_ws_bytes() { return 256 * AttnPartial::BYTES; }   // <= one block per CU in the tail round
// What mmpl_launch_attention does with an AttnArgs: every choice of the launcher is made by mmpl_attn_plan and nowhere else (the
// launcher reads it from the plan; mmpl_attn_fwd_ex reports it to the tests).  Host arithmetic on the arguments and the run-time
// switches (mmpl_config.h); the CU count of the current device is looked up only for a valid launch of the cross or the w64 kernel.
enum AttnKernel { ATTN_KERNEL_NONE = 0,      // Lq <= 0: nothing is launched
                  ATTN_KERNEL_LOCKSTEP = 1,  // attn_fwd_kernel<cross>
                  ATTN_KERNEL_CROSS1 = 2, ATTN_KERNEL_CROSS2 = 3,   // attn_cross_kernel<1 | 2>
                  ATTN_KERNEL_W64 = 4 };     // attn_w64_kernel (+ the split launch and attn_merge_kernel when sp > 1)
struct AttnPlan {
  int invalid;            // the launcher answers hipErrorInvalidValue and launches nothing (the fields below are then 0)
  int kernel;             // AttnKernel
  int n_pages;            // pages the kernel walks (w64: after merge_contiguous_pages)
  int kv_tiles;           // 64-row KV tiles per query block
  int main_blocks;        // blocks of the main launch (w64: grid padding included)
  int tail_items;         // w64: query blocks per XCD that run split in the tail round (0 = no split)
  int sp;                 // w64: KV parts per tail query block (1 = no split)
  int qb_per_block;       // cross kernel: 256-row query blocks per block
  int blocks_per_head;    // cross kernel
  AttnArgs args;          // what the kernels receive: pages merged and ordered, page_rows_each and history_mem filled
};
// The ATTN_* kernel an AttnArgs resolves to (ATTN_AUTO: the text cross-attention and every raw q -> ATTN_LOCKSTEP).
int mmpl_attn_resolve_variant(const AttnArgs& a);
AttnPlan mmpl_attn_plan(const AttnArgs& a);
inline size_t mmpl_attention_history_states(int Lq, int H) { return (size_t)H * ((Lq + ATTN_QB - 1) / ATTN_QB) * 4; }
inline size_t mmpl_attention_history_state_bytes(int Lq, int H) { return (mmpl_attention_history_states(Lq, H) + 255) & ~(size_t)255; }
inline size_t mmpl_attention_history_bytes(int Lq, int H) { return mmpl_attention_history_state_bytes(Lq, H) + mmpl_attention_history_states(Lq, H) * 128 * sizeof(short); }
hipError_t mmpl_launch_attention(const AttnArgs& a, hipStream_t s);
// n_groups attentions of equal shape (AttnGroupArgs above), as the caller states them: `common` is the AttnArgs of ONE group (q / o:
// group 0's first row; Lq = rows of a group; its own page fields are ignored), lists[g] the pages of group g.  common.history, when
// not NULL, is n_groups regions of mmpl_attention_history_bytes(Lq, H), group g's at g times that.
struct AttnGroupPages {
  int n_pages;
  const bf16_t* k_pages[MMPL_MAX_PAGES]; const bf16_t* v_pages[MMPL_MAX_PAGES];
  unsigned char page_group[MMPL_MAX_PAGES];
};
// Every choice of mmpl_launch_attention_groups is made here.  Each group's list is planned by itself first (mmpl_attn_plan: checks,
// order, merge).  ONE grouped launch needs every group on attn_w64_kernel (so not MMPL_ATTN_V1), no history and at most MMPL_MAX_PAGES
// merged pages in all; anything else runs as one mmpl_launch_attention per group (grouped == 0), which computes the same.  The grouped
// launch's split-KV tail is the one tail rule (attention.hip: plan_tail) on the n_groups * H virtual heads and on the shortest group's
// KV tiles.
struct AttnGroupPlan {
  int invalid;            // the launcher answers hipErrorInvalidValue and launches nothing
  int grouped;            // 1: one grouped launch of `ga` by `p`; 0: n_groups launches of single[g]
  int n_groups, items;    // items: (group, head, query block) work items in all
  AttnPlan p;             // grouped: kernel, n_pages (all groups), kv_tiles (the longest group's), main_blocks, tail_items, sp;
                          // per group: group 0's plan
  AttnGroupArgs ga;
  AttnArgs single[MMPL_MAX_GROUPS];   // what each group's own launch receives (before its own plan)
};
AttnGroupPlan mmpl_attn_groups_plan(const AttnArgs& common, int n_groups, const AttnGroupPages* lists);
hipError_t mmpl_launch_attention_groups(const AttnArgs& common, int n_groups, const AttnGroupPages* lists, hipStream_t s);

// ---------------------------------------------------------------- norms / rope / elementwise (elementwise.hip)
// LayerNorm (eps, fp32 stats) fused with per-frame modulation  y = bf16(bf16(LN(x)) * bf16(1+scale)) + shift
// or with an affine (w, b).  mod pointers index [frame * mod_frame_stride + col].
struct LnArgs {
  const bf16_t* x; int ldx;
  bf16_t* y; int ldy;
  int rows, d;
  float eps;
  const bf16_t* scale; const bf16_t* shift; int mod_frame_stride; int rows_per_frame;  // modulation form
  const bf16_t* w; const bf16_t* b;                                                    // affine form (if w != null)
};
// What mmpl_launch_layernorm / mmpl_launch_qknorm do with their arguments: every choice of the two launchers is made by mmpl_ln_plan /
// mmpl_qknorm_plan and nowhere else (the launchers read it from the plan; mmpl_layernorm_ex / mmpl_qknorm_ex report it to the tests).
// Host arithmetic on the arguments and the run-time switches (mmpl_config.h); a pipelined kernel's resident blocks come from the
// occupancy query and the CU count of the current device, once per instantiation.
enum RowPassKernel { ROWPASS_KERNEL_NONE = 0,          // rows <= 0: nothing is launched
                     ROWPASS_KERNEL_LN = 1,            // layernorm_kernel<NIT>: one row per wave
                     ROWPASS_KERNEL_LN_PIPELINED = 2,  // layernorm_pipelined_kernel<NIT, FULL>
                     ROWPASS_KERNEL_QKNORM = 3 };      // qknorm_kernel<NIT, FULL>
struct RowPassPlan {
  int invalid;            // the launcher answers hipErrorInvalidValue and launches nothing (the fields below are then 0)
  int kernel;             // RowPassKernel
  int nit;                // NIT as instantiated: 1, 2, 3, 4, 6, 8 or 10
  int full;               // FULL (pipelined kernels): d == 512 NIT, rows % 4 == 0 (LayerNorm's modulation form: rows_per_frame % 4 == 0 too)
  int resident;           // pipelined kernels: the blocks counted resident at once (blocks per CU x CUs)
  int groups_per_block;   // 4-row groups per block (layernorm_kernel: 1)
  int grid_x, grid_y;
};
// Two host-side overrides travel beside the argument structs (those are kernel arguments), for the kernel-level tests; the product
// passes the defaults everywhere.  pipeline: -1 = the launcher's choice (NIT >= 6 and rows >= MMPL_LN_PIPELINE_MIN_ROWS), 0 = never,
// 1 = always -- still only where NIT >= 6, else invalid.  groups_per_block: 0 = the launcher's choice (one round of resident blocks);
// > 0 with a pipelined kernel only.
bool mmpl_ln_pipelined(const LnArgs& a, int pipeline = -1);   // the plan's kernel choice by itself: no HIP call
RowPassPlan mmpl_ln_plan(const LnArgs& a, int pipeline = -1, int groups_per_block = 0);
hipError_t mmpl_launch_layernorm(const LnArgs& a, hipStream_t s, int pipeline = -1, int groups_per_block = 0);

// Full-dim RMSNorm (+ optional 3-axis RoPE, + optional K/V page write) on the fused qkv projection.
struct QkNormArgs {
  bf16_t* q; int ldq;                 // in/out (in place)
  const bf16_t* k; int ldk;           // in (null: q only)
  const bf16_t* v; int ldv;           // in
  const bf16_t* wq; const bf16_t* wk; // RMSNorm gains [d]
  int rows, d;
  float eps;
  float q_scale;                      // q is multiplied by this after RoPE, before its (single) rounding to bf16; 0 = 1
  int rope;                           // 0: no rope (cross-attn q / context k)
  const float* cos_tab; const float* sin_tab;  // [1024][64] fp32
  int frame_ids[MMPL_MAX_PAGES];      // temporal rope position per local frame (relative to *frame_base when that is set); a stage of
                                      // mmpl_dit_forward uses the first 8 at most, the whole clip of mmpl_dit_forward_full up to all of them
  const int* frame_base;              // device int added to every frame id when the kernel RUNS (a captured launch is replayed at
                                      // another position by rewriting it in stream order); NULL = 0.  The sum is clamped to the tables' 0..1023
  bf16_t* k_dst[MMPL_MAX_PAGES]; bf16_t* v_dst[MMPL_MAX_PAGES]; // per local frame destination page base (row stride = d); k_out for no-page mode
  int rows_per_frame, grid_w;
};
RowPassPlan mmpl_qknorm_plan(const QkNormArgs& a, int groups_per_block = 0);
hipError_t mmpl_launch_qknorm(const QkNormArgs& a, hipStream_t s, int groups_per_block = 0);

// rmsnorm of a plain [rows, d] matrix in place (context K)
// out_scale != 0: the normalised row is multiplied by it before its (single) rounding (a q that feeds ATTN_W64: scale * log2 e)
hipError_t mmpl_launch_rmsnorm(bf16_t* x, int ldx, const bf16_t* w, int rows, int d, float eps, hipStream_t s, float out_scale = 0.f);

// emod[l][f][k][:] = bf16(mod[l*mod_layer_stride + k*d + :] + e[f*e_frame_stride + (bcast ? : : k*d + :)])   (k < nmod)
hipError_t mmpl_launch_modulation(const bf16_t* mod, size_t mod_layer_stride, const bf16_t* e, int e_frame_stride, int bcast,
                                  bf16_t* emod, int n_layers, int n_frames, int nmod, int d, hipStream_t s);
// patchify: x[F, C, h, w] -> A[F*gh*gw, lda]  (col = c*4 + ph*2 + pw; columns >= 4 C are zero: K padded to a multiple of 64)
hipError_t mmpl_launch_patchify(const bf16_t* x, bf16_t* a, int lda, int F, int C, int h, int w, hipStream_t s);
// patchify2: patchify of cat([x[F, Cx, h, w], y[F, Cy, h, w]], channel axis) without the concatenated tensor: the same A, bit for bit
hipError_t mmpl_launch_patchify2(const bf16_t* x, const bf16_t* y, bf16_t* a, int lda, int F, int Cx, int Cy, int h, int w, hipStream_t s);
// unpatchify: y[F*gh*gw, 4*C] (col = (ph*2+pw)*C + c) -> out[F, C, h, w]
// a = bf16(a + b), n elements (i2v.hip)
hipError_t mmpl_launch_add(bf16_t* a, const bf16_t* b, size_t n, hipStream_t s);
// x = bf16(0.5 x (1 + erf(x / sqrt 2))) in place, n elements (i2v.hip: torch.nn.GELU())
hipError_t mmpl_launch_gelu_erf(bf16_t* x, size_t n, hipStream_t s);
hipError_t mmpl_launch_unpatchify(const bf16_t* y, int ldy, bf16_t* out, int F, int C, int h, int w, hipStream_t s);
// sinusoidal timestep embedding (fp64 math): t[F] fp32 -> out[F, freq_dim] bf16 ([cos | sin])
hipError_t mmpl_launch_zero_ints(int* p, int n, hipStream_t s);
// MMPL_CHECK_SHARE=1 (api.hip: the guard of mmpl_dit_forward's share_in promise).  chk: 5 device uint64 = {producer fingerprint[2],
// consumer fingerprint[2], mismatch count}; a fingerprint is accumulated over a list of equally sized pages (K pages, then V pages).
struct PageList { const void* p[MMPL_MAX_PAGES]; int n; };
hipError_t mmpl_launch_share_check_zero(unsigned long long* chk, int which, hipStream_t s);
hipError_t mmpl_launch_pages_fingerprint(const PageList& pl, size_t bytes_per_page, unsigned long long* chk, int which, hipStream_t s);
hipError_t mmpl_launch_share_check_compare(unsigned long long* chk, hipStream_t s);
// flags[r] = (row r of x[rows, d] == row rows - 1, bitwise)
hipError_t mmpl_launch_rows_equal_last(const bf16_t* x, int ld, int rows, int d, int* flags, hipStream_t s);
hipError_t mmpl_launch_sinusoid(const float* t, bf16_t* out, int F, int freq_dim, hipStream_t s);
hipError_t mmpl_launch_silu(const bf16_t* x, bf16_t* y, size_t n, hipStream_t s);
// step caching (step_cache.hip).  r = bf16(float(xl) - float(x0)), n elements: 16 bytes per lane where all three are 16-byte aligned
hipError_t mmpl_launch_residual_sub(const bf16_t* xl, const bf16_t* x0, bf16_t* r, size_t n, hipStream_t s);
// out[i] = sum_c |x[i+1,c] - x[i,c]| / sum_c |x[i,c]| for i < rows - 1 (fp32, fixed order: mmpl_rel_l1_rows in the public header)
hipError_t mmpl_launch_rel_l1_rows(const bf16_t* x, int ld, int rows, int d, float* out, hipStream_t s);

// The samplers (sampler.hip): CFG combine + one UniPC / DPM-Solver++ step on x / m0 / m1 / last of storage type T (bf16_t or float)
// with bf16 flows; the formulas are in sampler.hip's header and at the entries in include/mmpl_hip.h.  Defined for the four pairs
// (bf16_t, MmplUniPCStep), (bf16_t, MmplDpmppStep), (float, MmplUniPCStepF32), (float, MmplDpmppStep).  The caller has checked the
// pointers; a.last is unused by DPM-Solver++.
template <class T>
struct SamplerPtrs {
  const bf16_t* flow_c; const bf16_t* flow_u;   // flow_u == null: flow_c is already the combined flow
  T* x;                                         // sample in / next sample out
  T* m0; T* m1; T* last;                        // solver state (updated in place)
  bf16_t* x_bf16;                               // float storage only: the bf16 rounding of the new x (may be null)
  size_t n;
};
// st: host memory, the scalars computed on the host exactly as the reference does
template <class T, class Step>
hipError_t mmpl_launch_sampler(const SamplerPtrs<T>& a, const Step* st, hipStream_t s);
// Device-resident form for a hipGraph of a whole denoise step: the scalars of step *step come from table[*step] (device memory,
// n_steps rows), then *step is advanced and the NEXT step's timestep is written to t_out[0..n_t) (the tensor the two DiT forwards
// of the next replay read).  A counter outside 0 .. n_steps - 1 changes nothing.
template <class T, class Step>
hipError_t mmpl_launch_sampler_table(const SamplerPtrs<T>& a, const Step* table, int* step, float* t_out, const float* t_tab, int n_t,
                                     int n_steps, hipStream_t s);

// ---------------------------------------------------------------- umT5 glue (t5.hip): the launches of mmpl_t5_encode, one each
// out[l][:] = emb[ids[l]][:]   (dim % 8 == 0, 16 bytes per access; ids in [0, vocab))
hipError_t mmpl_launch_t5_gather(const int* ids, const bf16_t* emb, bf16_t* out, int L, int dim, hipStream_t s);
// sc fp32 [H][L][L] -> p bf16 [H][L][L]: softmax over j of bf16(bf16(sc) + bias), bias = pos_emb[bucket[j - i + L - 1] * H + h] or
// finfo(bf16).min where mask[j] == 0; one block per (h, i)
hipError_t mmpl_launch_t5_softmax(const float* sc, const bf16_t* pos_emb, const int* bucket, const int* mask, bf16_t* p, int H, int L,
                                  hipStream_t s);
// v [L][ld] (head h at column h * c) -> vt [H][c][L]
hipError_t mmpl_launch_t5_transpose(const bf16_t* v, int ld, bf16_t* vt, int L, int c, int H, hipStream_t s);
// f = bf16(f * GELU_tanh(g)) with every tensor op of the reference rounded to bf16, n elements
hipError_t mmpl_launch_t5_gated(bf16_t* f, const bf16_t* g, size_t n, hipStream_t s);
// out [L][dim]: rows l with mask[l] == 0 are zeroed
hipError_t mmpl_launch_t5_zero_pad(bf16_t* out, const int* mask, int L, int dim, hipStream_t s);
