/* libmmpl_hip.so -- C ABI of the MI355X-native MMPL denoising hot path.
 *
 * The reference (Tele-AI/MMPL) has no FFI: its seams are Python signatures.  Each entry point
 * below names the reference interface it replaces (paths relative to the reference root); the Python mirror
 * in mmpl_amd/ binds them with ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions: every pointer marked "dev" is a borrowed device pointer (e.g. torch.Tensor.data_ptr()); nothing
 * is retained after the call returns except by mmpl_dit_bind_weights (which stores the weight pointers) and
 * nothing is allocated on the device except two 256 KiB RoPE tables owned by the handle (and, under MMPL_CHECK_SHARE=1, 64 bytes of
 * check state).  All tensors are
 * bfloat16 unless stated.  Every call takes the HIP stream to enqueue on and is asynchronous with respect to
 * the host.  Return value: 0 = ok, non-zero = error (text via mmpl_last_error(), thread-local).
 */
#ifndef MMPL_HIP_H
#define MMPL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmpl_stream_t; /* hipStream_t */

typedef struct MmplDitConfig {
  int dim, ffn_dim, num_heads, num_layers; /* wan/configs/wan_t2v_14B.py:17-25 */
  int text_dim, freq_dim, in_dim, out_dim, text_len;
  float eps;
  int lat_h, lat_w;   /* latent frame size: 60x104 (480p, the reference's literal 1560 tokens) or 90x160 (720p) */
  int max_frames;     /* largest stage (7) */
} MmplDitConfig;

typedef struct MmplDit MmplDit;

/* Number of weight pointers mmpl_dit_bind_weights expects, and the name of slot i (reference state_dict key,
 * "blocks.N." prefix for per-layer slots; packed slots say how they are packed). */
int mmpl_dit_num_weights(const MmplDitConfig* cfg);
const char* mmpl_dit_weight_name(int slot_in_layer_or_global, int per_layer);

/* CausalFPSWanModel.__init__ (wan/modules/causal_fps_model.py:409-530): geometry + RoPE tables. */
int mmpl_dit_create(const MmplDitConfig* cfg, MmplDit** out);
void mmpl_dit_destroy(MmplDit* h);
/* load_state_dict seam (Wan_fps_inference_1gpu.py:66-68): stores n borrowed dev pointers, order = weight slots. */
int mmpl_dit_bind_weights(MmplDit* h, const void* const* dev_ptrs, int n);

size_t mmpl_dit_workspace_bytes(const MmplDit* h, int n_frames);
size_t mmpl_dit_context_workspace_bytes(const MmplDit* h);

/* text_embedding + per-layer cross-attn K/V (causal_fps_model.py:780-786, model.py:175-180), once per prompt.
 * context: dev [text_len, text_dim] zero-padded; cross_k/cross_v: dev out [num_layers, text_len, dim].
 * distinct_rows (host out, may be NULL): n such that rows n .. text_len-1 of the EMBEDDED context are bitwise identical (the
 * reference zero-pads the T5 output and attends over the padding unmasked, utils/wan_wrapper.py:46-47, model.py:189, so after
 * the text embedding the padded tail is one repeated row, and so are its K and V rows in every block); text_len when the tail
 * does not repeat.  Determined on the device with one 2 KiB read-back (synchronises `stream`); inside a stream capture nothing
 * is read back and text_len is reported.  It is a property of the K/V CONTENTS: it stays valid for any copy of cross_k/cross_v
 * and is what mmpl_dit_forward takes as `cross_rows`. */
int mmpl_dit_precompute_context(MmplDit* h, const void* context, void* cross_k, void* cross_v, void* workspace,
                                size_t workspace_bytes, int* distinct_rows, mmpl_stream_t stream);

/* Wan-I2V model type (WanModel(model_type='i2v'), wan/modules/model.py:563-616,672-712): in_dim = 36 (x and the
 * conditioning video y concatenated on the channel axis, model.py:680-681 -- the caller concatenates for mmpl_dit_forward;
 * mmpl_dit_forward_full_i2v takes the two as they are) and every block's
 * cross-attention also attends to the 257 projected CLIP tokens (WanI2VCrossAttention, model.py:224-266).  The image
 * K / V depend only on the image: img_k[l] = norm_k_img(k_img(img_emb(clip_fea))), img_v[l] = v_img(...), built with
 * mmpl_i2v_img_proj + mmpl_i2v_img_kv per layer; dev [num_layers, n_img_tokens, dim], borrowed until replaced.
 * NULL, NULL restores the text-only cross-attention. */
int mmpl_dit_set_image_kv(MmplDit* h, const void* img_k, const void* img_v, int n_img_tokens);

/* Optional diagnostics of the self-attention kernel's data dependence.  attn_w64_kernel runs a max-free FAST softmax pass per
 * 256-row query block and redoes the block with the GENERAL (running-reference) pass if any row sum left [2^-100, 2^100].
 * stats_dev: 5 x uint64 in device memory (borrowed; zero them yourself), incremented by every self-attention launch of
 * mmpl_dit_forward on this handle, inside hipGraph replays too: [0] += blocks run, [1] += blocks whose FAST pass failed and that were
 * redone (both passes paid), [2] += waves (64 of a block's 256 query rows) that held a failing row themselves -- the unit a
 * finer-grained redo would pay for, [3] += blocks their history sent straight to the GENERAL pass, [4] += blocks whose FAST pass held
 * on the references their history remembered (`attn_history`).  NULL switches it off. */
int mmpl_dit_set_attn_stats(MmplDit* h, void* stats_dev);

/* CausalFPSWanModel._forward_inference (causal_fps_model.py:708-837) behind WanFPSWrapper.forward
 * (utils/wan_wrapper.py:422-493).
 *   x_in / out : dev [n_frames, in_dim, lat_h, lat_w] / [n_frames, 16, lat_h, lat_w]  (the pipeline's [B=1, F, C, H, W] layout)
 *   t_dev      : dev float32 [n_frames]
 *   frame_ids  : host, RoPE temporal index per frame (= current_start / frame_seqlen)
 *   write_slots: host, KV slot each frame's K/V is written to before attending; all -1 = do not persist
 *                (the reference's [13..18] stage, causal_fps_model.py:254-264)
 *   visible_slots: host, cache slots attended (attention_vis_index after the 19,20 -> 13,14 remap)
 *   k_cache / v_cache: dev [num_layers, n_slots * S, dim], mutated in place like the reference's kv_cache
 *   cross_k / cross_v: from mmpl_dit_precompute_context (or any copy of them)
 *   cross_rows : the caller's statement that rows cross_rows .. text_len-1 of every layer of cross_k (and of cross_v) are copies
 *                of row cross_rows -- the `distinct_rows` mmpl_dit_precompute_context reported for these contents.  The text
 *                cross-attention then attends over rows 0 .. cross_rows with the last one weighted text_len - cross_rows times:
 *                the same softmax, (text_len - cross_rows - 1) fewer keys.  text_len (or any value outside [0, text_len - 2])
 *                = attend over all text_len rows, which is always correct.
 *   share_out / share_in (both may be NULL, at most one non-NULL): dev [n_frames * S, dim] bf16.  Block 0's self-attention sees
 *                nothing that differs between the two branches of classifier-free guidance (same latents, same timestep, and -- by
 *                induction -- the same layer-0 K / V in both caches), only the text context differs and that enters after it.
 *                share_out: this forward also leaves x as it is after block 0's self-attention residual there.  share_in: the
 *                caller's statement that ANOTHER forward on the same x_in / t / frame_ids / write_slots / visible_slots, whose
 *                layer-0 cache contents equal this one's, produced it: block 0's attention and output projection are skipped and
 *                x continues from share_in (this forward's own layer-0 K / V slots are still written).  Same kernels on the same
 *                inputs: the result is bit-identical to computing it.  MMPL_CHECK_SHARE=1 (environment, read when the library is
 *                first used; a debug switch) turns the statement into a check: the share_out and the share_in forward each
 *                fingerprint the layer-0 K / V slots they attend to on the device (one pass over them), the share_in forward
 *                compares; outside a stream capture it then fails with an error on a mismatch, inside one the mismatch is counted
 *                on the device (mmpl_dit_share_check_failures).
 *   attn_history (may be NULL): dev, mmpl_dit_attn_history_bytes(h, n_frames) bytes owned by the caller: per (layer, head, 256-row query
 *                block, split part) of the self-attention one state byte and 128 int16 lane references -- what this attention's
 *                previous launch learned.  Hand the same buffer to every forward of one (CFG branch, stage) -- consecutive denoise
 *                steps see the same K / V and nearly the same q -- and zero it when the stage changes.  A query block whose max-free
 *                FAST softmax pass failed (heavy-tailed scores) then stops paying for both passes: from its first failure on every pass
 *                leaves each lane's mean log-sum-exp, the next FAST pass takes that as its reference and holds wherever the scores'
 *                range is; a block that fails even so goes straight to the GENERAL pass for 7, then 15, then 30 launches between
 *                retries.  Both passes are the exact softmax up to rounding, so any contents give a correct result -- but which pass
 *                runs, against which reference, decides the rounding: with a history the output bits depend on the launches before
 *                (two identical sequences of launches from a zeroed history are bit-identical, eager or replayed from a hipGraph; a
 *                block that never fails never leaves the zero state and computes the stateless kernel's bits); NULL = stateless, every
 *                launch bit-reproducible by itself. */
int mmpl_dit_forward(MmplDit* h, const void* x_in, const float* t_dev, int n_frames, const int* frame_ids,
                     const int* write_slots, const int* visible_slots, int n_visible, void* k_cache, void* v_cache,
                     int n_slots, const void* cross_k, const void* cross_v, int cross_rows, void* share_out, const void* share_in,
                     void* attn_history, void* out, void* workspace, size_t workspace_bytes, mmpl_stream_t stream);
/* mmpl_dit_forward with the RoPE position base as DEVICE data.  frame_base_dev: dev, one int (NULL = mmpl_dit_forward, bit for
 * bit); `frame_ids` are then RELATIVE to it: frame i is rotated at temporal position frame_ids[i] + *frame_base_dev.  The int is
 * read by the device when the forward EXECUTES, not when it is launched or captured: a forward captured into a hipGraph is
 * replayed at another position in time by writing the int in stream order before the replay -- the slots, shapes and every other
 * argument of the launch stay what was captured.  The host cannot see the base at replay time, so keeping frame_ids[i] + base
 * inside the RoPE tables (0 .. 1023) is the caller's job; the kernel clamps the sum to that range, so a stale base rotates with
 * the wrong angle but reads nothing outside the tables. */
int mmpl_dit_forward_at(MmplDit* h, const void* x_in, const float* t_dev, int n_frames, const int* frame_ids,
                        const int* write_slots, const int* visible_slots, int n_visible, void* k_cache, void* v_cache,
                        int n_slots, const void* cross_k, const void* cross_v, int cross_rows, void* share_out, const void* share_in,
                        void* attn_history, void* out, void* workspace, size_t workspace_bytes, const int* frame_base_dev,
                        mmpl_stream_t stream);
/* mmpl_dit_forward_at over a BATCH: n_groups independent samples of frames_per_group frames each, in the launches of ONE forward over
 * n_frames = n_groups * frames_per_group frames.  Everything but attention works per row or per frame already, and every sample's
 * K / V slots lie in the one cache allocation, so the batch is an ordinary forward except that the self-attention is block-diagonal:
 * the query rows of sample g see sample g's visible slots only (one grouped launch of attn_w64_kernel, see mmpl_attn_fwd_groups_ex).
 *   x_in / out, t_dev, frame_ids, write_slots: per frame as mmpl_dit_forward_at, sample-major (frame g * frames_per_group + i is frame i of
 *                sample g); n_frames <= cfg.max_frames.
 *   visible_slots: host, n_groups lists of n_visible slots each, back to back.  The caller gives each sample slots of its own (sample g
 *                of a window of W slots: g * W .. g * W + W - 1 of a cache of n_groups * W); write slots of different samples must differ.
 *   cross_k / cross_v: host arrays of n_groups device pointers.  When every sample's pair is the same pointers (one prompt for all) the
 *                text cross-attention is the ONE launch of mmpl_dit_forward_at over all rows; otherwise one such launch per sample on
 *                that sample's rows.  cross_rows is one statement for all samples: it must hold for each of them (the largest of the
 *                samples' `distinct_rows` does).
 * Rejected before the first launch, each with its own message: n_groups < 1, n_frames > max_frames, a non-NULL share_out / share_in /
 * attn_history (pass NULL), an i2v handle (image K / V attached), a visible or write slot outside [0, n_slots), write slots of two
 * samples that coincide.  n_groups == 1 launches what mmpl_dit_forward_at launches, bit for bit.  The workspace is
 * mmpl_dit_workspace_bytes(h, n_frames).  Sample g's result equals a mmpl_dit_forward_at call on that sample alone up to the choices
 * the GEMM and the attention launchers make from the row count (tile order, split tails): bit-equal where those agree. */
int mmpl_dit_forward_groups(MmplDit* h, const void* x_in, const float* t_dev, int n_groups, int frames_per_group, const int* frame_ids,
                            const int* write_slots, const int* visible_slots, int n_visible, void* k_cache, void* v_cache, int n_slots,
                            const void* const* cross_k, const void* const* cross_v, int cross_rows, void* share_out, const void* share_in,
                            void* attn_history, void* out, void* workspace, size_t workspace_bytes, const int* frame_base_dev,
                            mmpl_stream_t stream);
size_t mmpl_dit_attn_history_bytes(const MmplDit* h, int n_frames);
/* The non-causal WanModel.forward (model.py, behind WanDiffusionWrapper(is_causal=False).forward, utils/wan_wrapper.py) over a WHOLE
 * clip: the blocks of mmpl_dit_forward with frame i rotated at temporal position i, every frame attending to every frame, and no
 * KV cache -- the K and V of the layer being computed live in the workspace as one contiguous [n_frames * S, dim] pair that every
 * layer reuses (a persistent per-layer cache of a 21-frame 14B / 720p clip would be 40 x 75 600 x 5 120 x 2 B = 31 GB per tensor).
 *   x_in / out : as mmpl_dit_forward
 *   t_dev      : dev, ONE float32: the clip's timestep, read when the forward executes.  Its embedding and the modulation vectors
 *                derived from it are computed once and read by every frame; the bits are those of mmpl_dit_forward given the same
 *                timestep in every frame.
 *   n_frames   : 1 .. 24, independent of cfg.max_frames (which stays the largest stage of mmpl_dit_forward)
 *   cross_k / cross_v / cross_rows / share_out / share_in / attn_history: the contracts of mmpl_dit_forward (attn_history is
 *                mmpl_dit_attn_history_bytes(h, n_frames) bytes; with no cache there is no layer-0 K / V to differ between the two
 *                CFG branches, so share_in needs only the same x_in and timestep)
 *   workspace  : dev, 256-byte aligned, at least mmpl_dit_full_workspace_bytes(h, n_frames) bytes (0 for an n_frames out of range):
 *                [GEMM tickets | x | LayerNorm out | qkv or ffn hidden | attention out | K | V | patches | timestep embedding,
 *                modulation vectors (one row each) | head out | split-K partials]
 * Equal, bit for bit, to mmpl_dit_forward on a zeroed cache with frame_ids = write_slots = visible_slots = 0 .. n_frames-1.
 * No allocation, no synchronisation and no host read: capturable into a hipGraph.  A null pointer, an n_frames outside 1 .. 24, a
 * workspace that is too small, both share_* set or a handle without weights are rejected before the first launch. */
size_t mmpl_dit_full_workspace_bytes(const MmplDit* h, int n_frames);
int mmpl_dit_forward_full(MmplDit* h, const void* x_in, const float* t_dev, int n_frames, const void* cross_k, const void* cross_v,
                          int cross_rows, void* share_out, const void* share_in, void* attn_history, void* out, void* workspace,
                          size_t workspace_bytes, mmpl_stream_t stream);
/* mmpl_dit_forward_full for the Wan-I2V model type (WanModel(model_type='i2v') sampled over the whole clip, wan/image2video.py), with
 * the two halves of its input as two tensors: the 36-channel cat([x, y]) of model.py:680-681 is never built -- the patch embedding
 * reads both (mmpl_patchify2) -- so a sampler updates the 16-channel latents in place while y stays where it is.
 *   x_in       : dev [n_frames, 16, lat_h, lat_w], the latents
 *   y_in       : dev [n_frames, in_dim - 16, lat_h, lat_w], the conditioning video (mask + encoded first frame), frame-major
 *   everything else: the contract of mmpl_dit_forward_full, its workspace size included.  Both CFG branches of an I2V step see the
 *                same image, so block 0's self-attention is still the same computation in both: share_out / share_in keep their
 *                meaning.  The image cross-attention's output goes to the workspace's K area, which in this layout holds the layer's
 *                own K and is dead once the self-attention has run.
 * Equal, bit for bit, to mmpl_dit_forward_full on the same handle given the concatenation.  Also rejected before the first launch:
 * a handle whose in_dim is not 36, a handle without image K / V (mmpl_dit_set_image_kv first), a null y_in. */
int mmpl_dit_forward_full_i2v(MmplDit* h, const void* x_in, const void* y_in, const float* t_dev, int n_frames, const void* cross_k,
                              const void* cross_v, int cross_rows, void* share_out, const void* share_in, void* attn_history,
                              void* out, void* workspace, size_t workspace_bytes, mmpl_stream_t stream);
/* The handle's RoPE tables (mmpl_dit_create: cos / sin of position * theta^(-2j / dims), theta 1e4, dims 44 | 42 | 42 of the 128-wide
 * head, computed in double and stored as float32), for tests and tools that make the forward's QK-norm launch themselves
 * (mmpl_qknorm_ex): copies the two [1024][64] float32 tables into the caller's device buffers cos_out / sin_out (256 KiB each),
 * asynchronously on `stream`.  A null argument is rejected before the first HIP call. */
int mmpl_dit_rope_tables(const MmplDit* h, float* cos_out, float* sin_out, mmpl_stream_t stream);
/* MMPL_CHECK_SHARE=1: number of share_in forwards (eager or replayed) since the last call whose layer-0 K / V fingerprint differed
 * from their share_out forward's; synchronises `stream` and resets the count.  0 when the switch is off. */
int mmpl_dit_share_check_failures(MmplDit* h, long long* count, mmpl_stream_t stream);

/* ---- step caching (TeaCache) of the 50-step samplers.  A denoise step whose timestep embedding has barely moved since the last
 * computed step skips the transformer blocks: it adds the residual that step left (x after the last block - x after the patch
 * embedding) to its own patch embedding and runs only the head.  Which steps skip depends on the timesteps and the weights alone
 * (mmpl_dit_time_embed + mmpl_rel_l1_rows below), so the host knows it before sampling starts.
 * mmpl_dit_forward_at_cached / mmpl_dit_forward_full_cached: every argument of mmpl_dit_forward_at / mmpl_dit_forward_full (y_in NULL)
 * or mmpl_dit_forward_full_i2v (y_in non-NULL) under its contract there, plus
 *   residual   : dev [n_frames * S, dim] bf16, mmpl_dit_step_cache_bytes(h, n_frames) bytes, 256-byte aligned, owned by the caller: one per
 *                (CFG branch, stage shape)
 *   cache_mode : 0 OFF    -- `residual` is ignored; the launches of the uncached entry, bit for bit.
 *                1 RECORD -- the launches of the uncached entry (out, the cache writes, share_out / share_in and attn_history are what
 *                            they are there, bit for bit), then after the last block the patch-embedding GEMM once more into the
 *                            LayerNorm buffer (dead there; its input patches are still in the workspace, so x_0 has the bits the
 *                            first run gave) and residual[r,c] = bf16(float(x_L[r,c]) - float(x_0[r,c])): one fp32 subtraction, one
 *                            rounding.  The workspace sizes do not change.
 *                2 REUSE  -- patchify (patchify2 with y_in), the patch-embedding GEMM with `residual` as its residual operand
 *                            (epilogue 4: x = bf16(acc + bias + residual), one rounding), the timestep embedding and the head
 *                            modulation, the head, unpatchify.  No block runs and no K / V is written: write_slots and
 *                            visible_slots are validated but nothing is persisted; cross_k, cross_v, share_out, share_in and
 *                            attn_history may be NULL and are ignored.
 * Rejected before the first launch, each with its own message: a cache_mode outside 0 .. 2; in mode 1 or 2 a NULL residual or one
 * that is not 256-byte aligned; and everything the uncached entry rejects.  mmpl_dit_forward_groups has no cached form. */
size_t mmpl_dit_step_cache_bytes(const MmplDit* h, int n_frames);
int mmpl_dit_forward_at_cached(MmplDit* h, const void* x_in, const float* t_dev, int n_frames, const int* frame_ids,
                               const int* write_slots, const int* visible_slots, int n_visible, void* k_cache, void* v_cache,
                               int n_slots, const void* cross_k, const void* cross_v, int cross_rows, void* share_out, const void* share_in,
                               void* attn_history, void* out, void* workspace, size_t workspace_bytes, const int* frame_base_dev,
                               mmpl_stream_t stream, int cache_mode, void* residual);
int mmpl_dit_forward_full_cached(MmplDit* h, const void* x_in, const float* t_dev, int n_frames, const void* cross_k, const void* cross_v,
                                 int cross_rows, void* share_out, const void* share_in, void* attn_history, void* out, void* workspace,
                                 size_t workspace_bytes, mmpl_stream_t stream, const void* y_in, int cache_mode, void* residual);
/* The timestep embedding of n_t timesteps at once: the sinusoid, time_embedding.0 (+ SiLU), time_embedding.2 -> e_out [n_t, dim] bf16,
 * and SiLU + time_projection.1 -> e0_out [n_t, 6 * dim] bf16 (NULL = not wanted): the launches a forward makes for its own
 * timesteps.  Row i of those GEMMs depends on row i of their input alone, so row i has the bits a forward computes for t_dev[i].
 *   t_dev      : dev float32 [n_t], 1 <= n_t <= 4096
 *   workspace  : dev, 256-byte aligned, at least mmpl_dit_time_embed_workspace_bytes(h, n_t) bytes */
size_t mmpl_dit_time_embed_workspace_bytes(const MmplDit* h, int n_t);
int mmpl_dit_time_embed(MmplDit* h, const float* t_dev, int n_t, void* e_out, void* e0_out, void* workspace, size_t workspace_bytes,
                        mmpl_stream_t stream);
/* out_dev[i] = (sum_c |x[i+1,c] - x[i,c]|) / (sum_c |x[i,c]|), i < rows - 1: the relative L1 distance of consecutive rows of the bf16
 * matrix x [rows, d] (row stride ld elements), in float32 -- the step-cache indicator over the rows of mmpl_dit_time_embed.
 * Deterministic, no float atomics.  Summation order of both sums: one 256-thread block per i; thread t adds the terms of columns
 * t, t + 256, t + 512, ... in increasing order; the 64 partials of a wave combine by a butterfly (partner lane ^ 32, then ^ 16, ^ 8,
 * ^ 4, ^ 2, ^ 1); the four wave sums are added in wave order 0, 1, 2, 3; then ONE IEEE division.  A zero row i gives inf or nan as
 * that division does.  rows >= 2, d >= 1, ld >= d. */
int mmpl_rel_l1_rows(const void* x, int ld, int rows, int d, float* out_dev, mmpl_stream_t stream);

/* attention() seam (wan/modules/attention.py:139-185) over paged K/V.  q/o: row r, head h at base + r*ld + h*128; every base
 * 16-byte aligned, every leading dimension a multiple of 8 elements (rows are read and written 16 bytes per lane).
 * k_pages/v_pages: host arrays of n_pages dev pointers, each page = page_rows rows of stride ldk/ldv.
 * Softmax does not depend on the order of the keys, the fp32 accumulation does: the 64-rows-per-wave kernel visits the pages in
 * ADDRESS order (back-to-back pages are merged), so a result is bit-reproducible for a given relative placement of the pages.
 * (mmpl_dit_forward keeps its two allocations -- cache slots, scratch pages -- apart, so ITS bits do not depend on placement.) */
int mmpl_attn_fwd(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                  int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads, float softmax_scale,
                  mmpl_stream_t stream);
/* Same, with scratch for the split-KV tail round (mmpl_attn_workspace_bytes() is always enough; NULL = mmpl_attn_fwd):
 * when the query blocks do not fill the last round of one-block-per-CU evenly, the leftover blocks are run as 2..4 blocks
 * over disjoint KV ranges plus a merge, which shortens the launch by up to one block time. */
size_t mmpl_attn_workspace_bytes(void);
int mmpl_attn_fwd_ws(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                     int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads, float softmax_scale,
                     void* workspace, size_t workspace_bytes, mmpl_stream_t stream);

/* Same, with the kernel chosen by the caller (tests and A/B runs): variant 0 = what mmpl_attn_fwd_ws picks (the lock-step
 * kernel for a raw q), 1 = lock-step 8 x 32 rows (the kernel the text cross-attention uses), 2 = removed (round 1's ping-pong
 * kernel: error), 3 = 4 waves x 64
 * rows (the DiT forward's self-attention kernel) on a raw q, 4 = the same on a q its producer already multiplied by
 * softmax_scale * log2(e) before rounding it to bf16 (what mmpl_dit_forward does: one rounding of q instead of two).
 * cross != 0 tags the launch as a text cross-attention launch (kernel symbol of variant 1 only).  Unknown variant: error. */
int mmpl_attn_fwd_variant(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                          int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads, float softmax_scale,
                          void* workspace, size_t workspace_bytes, int variant, int cross, mmpl_stream_t stream);

/* The DiT forward's self-attention launch by itself (variant 4 above: attn_w64_kernel on a q its producer multiplied by
 * softmax_scale * log2(e) before rounding it to bf16), with the two optional pieces of state mmpl_dit_forward threads through it:
 * history = mmpl_attn_history_bytes(Lq, num_heads) device bytes (see mmpl_dit_forward's attn_history; NULL = stateless) and
 * stats_dev = 5 x uint64 (see mmpl_dit_set_attn_stats; NULL = off). */
size_t mmpl_attn_history_bytes(int Lq, int num_heads);
int mmpl_attn_fwd_history(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                          int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads, float softmax_scale,
                          void* workspace, size_t workspace_bytes, void* history, void* stats_dev, mmpl_stream_t stream);

/* nn.Linear (+ fused epilogue). epi: 0 bias, 1 bias+GELU(tanh), 2 bias+SiLU, 3 x + (y*gate[frame]) , 4 x + y */
int mmpl_gemm(const void* A, int lda, const void* W, int ldw, const void* bias, void* C, int ldc, int M, int N, int K,
              int epi, const void* res, int ldres, const void* gate, int gate_frame_stride, int rows_per_frame,
              mmpl_stream_t stream);
/* The same GEMM with dynamic tile scheduling for the large-problem kernel: tile_counter = 8 device ints (one per XCD) that are
 * zero when the launch starts (the launch leaves them zero); the kernel is then launched once per CU and its blocks draw
 * tiles of their XCD's share until none is left, instead of one block per tile in lock-step rounds.  Launches sharing a
 * counter must be stream-ordered.  NULL = mmpl_gemm.  (mmpl_dit_forward keeps such a counter in its workspace.) */
int mmpl_gemm_tickets(const void* A, int lda, const void* W, int ldw, const void* bias, void* C, int ldc, int M, int N, int K,
                      int epi, const void* res, int ldres, const void* gate, int gate_frame_stride, int rows_per_frame,
                      void* tile_counter, mmpl_stream_t stream);
/* mmpl_gemm_tickets + a split-K launch for the partial last round of tiles (a GEMM of R * 256 + t tiles on 256 CUs otherwise takes
 * R + 1 rounds however small t is: the Wan 1.3B block GEMMs, every model's 2-frame stage): when the leftover tiles fit one round in
 * 2-4 parts each, they are computed as that many blocks over a share of K each, fp32 partials in `scratch`, summed in part order by
 * the part that finishes last (deterministic), which then runs the ordinary epilogue.  scratch: mmpl_gemm_scratch_bytes() device
 * bytes whose first 2048 are zero when a launch starts (every launch leaves them zero): [8 tile tickets | pad to 256 B | 256 tile
 * counters | pad to 2048 B | partials].  Launches sharing a scratch must be stream-ordered.  (mmpl_dit_forward keeps one in its
 * workspace.) */
size_t mmpl_gemm_scratch_bytes(void);
/* Diagnostic: 1 if workgroup b of a launch runs on XCD b & 7 on the current device (checked on the hardware once per device), else
 * 0.  The tile / head orders use that mapping for L2 locality only; since round 4 no kernel depends on it for correctness (the
 * split-K launch exchanges its partials with system-scope accesses).  Synchronises on first use: not inside a stream capture. */
int mmpl_device_xcd_round_robin(void);
/* Calibration of the box a measurement runs on: the rate (TFLOP/s, dense bf16) the current device sustains on nothing but
 * back-to-back MFMAs on random operands, one wave per SIMD, accumulators in the accumulator file; shape 32 =
 * v_mfma_f32_32x32x16_bf16 (the attention kernels), 16 = v_mfma_f32_16x16x32_bf16 (GEMM, VAE).  Runs for about `seconds` on the
 * null stream and synchronises; reports the second half of the run.  MI355X is power-limited under dense MFMA streams, so this --
 * not the nominal 2.5 PFLOP/s -- is the ceiling wall clock can be priced against on THIS box (bench.py `roofline.sustained_probe_tflops`). */
int mmpl_probe_mfma_tflops(int shape, double seconds, double* tflops);
int mmpl_gemm_scratch(const void* A, int lda, const void* W, int ldw, const void* bias, void* C, int ldc, int M, int N, int K,
                      int epi, const void* res, int ldres, const void* gate, int gate_frame_stride, int rows_per_frame,
                      void* scratch, size_t scratch_bytes, mmpl_stream_t stream);

/* WanLayerNorm (+ per-frame modulation or affine) (wan/modules/model.py:89-99, causal_fps_model.py:343,352,355) */
int mmpl_layernorm(const void* x, int ldx, void* y, int ldy, int rows, int d, float eps, const void* scale,
                   const void* shift, int mod_frame_stride, int rows_per_frame, const void* w, const void* b,
                   mmpl_stream_t stream);

/* WanRMSNorm over the full dim on q (in place) and k, causal_fps_rope_apply, KV slot write
 * (model.py:70-86, causal_fps_model.py:27-55, 211-217).  k_dst/v_dst: host arrays of n_frames dev page pointers. */
int mmpl_qknorm_rope(MmplDit* h, void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* wq,
                     const void* wk, int n_frames, const int* frame_ids, void* const* k_dst, void* const* v_dst,
                     mmpl_stream_t stream);
/* Same, with the temporal position of frame i = frame_ids[i] + *frame_base_dev (dev, one int, read when the kernel runs; the sum
 * is clamped to 0 .. 1023; NULL = mmpl_qknorm_rope, bit for bit).  See mmpl_dit_forward_at. */
int mmpl_qknorm_rope_at(MmplDit* h, void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* wq,
                        const void* wk, int n_frames, const int* frame_ids, void* const* k_dst, void* const* v_dst,
                        const int* frame_base_dev, mmpl_stream_t stream);

/* CFG combine + FlowUniPCMultistepScheduler.step (casual_fps_inference.py:366-374, fm_solvers_unipc.py:655-739) */
typedef struct MmplUniPCStep {
  float guidance, sigma_cur;
  int use_corrector, corr_order;
  float c_c1, c_c2, c_c3, c_inv_rk, c_rho0, c_rho_last;
  int pred_order;
  float p_c1, p_c2, p_c3, p_inv_rk;
} MmplUniPCStep;
/* flow_cond, x, m0, m1, last_sample: dev bf16 [n], none of them NULL (rejected before the launch); flow_uncond NULL = flow_cond is
 * already the combined flow. */
int mmpl_cfg_unipc_step(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* last_sample,
                        size_t n, const MmplUniPCStep* s, mmpl_stream_t stream);
/* Device-resident form, for ONE hipGraph per denoise step (2 DiT forwards + this) replayed sampling_steps times with no
 * host work in between: the scalars of step *step_dev are read from table_dev[*step_dev] (n_steps entries, device memory),
 * then *step_dev += 1 and the next step's timestep (timestep_table_dev[*step_dev]) is written to timestep_dev[0..n_timestep)
 * -- the tensor the forwards of the next replay read. */
int mmpl_cfg_unipc_step_table(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* last_sample,
                              size_t n, const MmplUniPCStep* table_dev, int* step_dev, float* timestep_dev,
                              const float* timestep_table_dev, int n_timestep, int n_steps, mmpl_stream_t stream);

/* CFG combine + FlowDPMSolverMultistepScheduler.step (sample_solver = 'dpm++': casual_fps_inference.py:366-374,
 * wan/utils/fm_solvers.py:706-797 as the pipeline configures it: DPM-Solver++(2M), midpoint, flow_prediction, final sigma 0).
 * Per element of n bf16 values, rbf = round to bf16, every other operation one IEEE fp32 operation (DESIGN.md "DPM-Solver++"):
 *   f  = rbf(fu + rbf(guidance * rbf(fc - fu)))                    (fc when flow_uncond is NULL)
 *   x0 = rbf(x - rbf(sigma_cur * f));  m1 <- m0;  m0 <- x0
 *   order 1:  x <- rbf(c1 * x - rbf(c2 * m0))
 *   order 2:  d1 = rbf(inv_r0 * rbf(m0 - m1));  x <- rbf((c1 * x - rbf(c2 * m0)) - rbf((0.5f * c2) * d1))
 * The scalars are finite on every step of a schedule (mmpl_amd/scheduler.py computes them); order is 1 or 2. */
typedef struct MmplDpmppStep {
  float guidance, sigma_cur;
  int order;
  float c1, c2, inv_r0;
} MmplDpmppStep;
/* flow_cond, x, m0, m1: dev bf16 [n], none of them NULL (rejected before the launch); flow_uncond NULL = flow_cond is already the
 * combined flow.  16 bytes per lane when every pointer is 16-byte aligned, element-wise otherwise. */
int mmpl_cfg_dpmpp_step(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, size_t n,
                        const MmplDpmppStep* s, mmpl_stream_t stream);
/* Device-resident form, the protocol of mmpl_cfg_unipc_step_table: the scalars of step *step_dev are read from
 * table_dev[*step_dev] (n_steps entries, device memory), then *step_dev += 1 and the next step's timestep
 * (timestep_table_dev[*step_dev]) is written to timestep_dev[0..n_timestep).  Once *step_dev has reached n_steps a launch changes
 * nothing. */
int mmpl_cfg_dpmpp_step_table(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, size_t n,
                              const MmplDpmppStep* table_dev, int* step_dev, float* timestep_dev,
                              const float* timestep_table_dev, int n_timestep, int n_steps, mmpl_stream_t stream);

/* The float32 latent chain of upstream Wan2.1 sampling (wan/text2video.py:182-250, wan/image2video.py:198-329): the latents, the CFG
 * combine and every tensor operation of the multistep solver stay in float32; only the flows are bf16 (the forward's output) and
 * only the forward's input is rounded to bf16 (x_bf16, what autocast does to the latents at the patch embedding).
 * Per element of n values, every operation below is ONE IEEE fp32 operation (round to nearest even), in the order of the reference's
 * tensor expressions; the device code is compiled with `#pragma clang fp contract(off)` and plain operators, so nothing is contracted
 * into an FMA and `/` is the correctly rounded division.  fc, fu: the bf16 flows widened (exact).
 *   f      = fu + guidance * (fc - fu)                                      (fc when flow_uncond is NULL)
 *   m_conv = x - sigma_cur * f
 * UniPC (fm_solvers_unipc.py:486-626, 350-484; order <= 2, bh2, predict_x0), `last` = last_sample:
 *   corrector, if use_corrector:
 *     xt_ = c_c1 * last - c_c2 * m0;   d1t = m_conv - m0
 *     corr_order 1:  acc = 0 + c_rho_last * d1t
 *     corr_order 2:  acc = c_rho0 * ((m1 - m0) / c_rk) + c_rho_last * d1t
 *     x   = xt_ - c_c3 * acc
 *   m1 <- m0;  m0 <- m_conv;  last <- x
 *   predictor:
 *     xt_ = p_c1 * x - p_c2 * m0
 *     pred_order 1:  x <- xt_ - p_c3 * 0
 *     pred_order 2:  x <- xt_ - p_c3 * (0.5 * ((m1 - m0) / p_rk))
 * DPM-Solver++(2M) (fm_solvers.py:706-797, midpoint), MmplDpmppStep as it is:
 *   m1 <- m0;  m0 <- m_conv
 *   order 1:  x <- c1 * x - c2 * m0
 *   order 2:  x <- (c1 * x - c2 * m0) - (0.5 * c2) * (inv_r0 * (m0 - m1))          (the reference multiplies by 1.0 / r0)
 * then x_bf16 <- bf16(x), round to nearest even, unless x_bf16 is NULL.
 * UniPC DIVIDES by rk where the reference divides, and the rhos are float32 (not rounded to bf16): MmplUniPCStepF32 carries c_rk /
 * p_rk (unused, any non-zero value, where the order is 1).  The scalars are finite on every step (mmpl_amd/scheduler.py computes
 * them).  Denormal inputs, scalars or intermediate results are outside the contract. */
typedef struct MmplUniPCStepF32 {
  float guidance, sigma_cur;
  int use_corrector, corr_order;
  float c_c1, c_c2, c_c3, c_rk, c_rho0, c_rho_last;
  int pred_order;
  float p_c1, p_c2, p_c3, p_rk;
} MmplUniPCStepF32;
/* flow_cond, flow_uncond: dev bf16 [n] (flow_uncond NULL = flow_cond is already the combined flow); x, m0, m1, last_sample: dev
 * float32 [n], updated in place, 4-byte aligned; x_bf16: dev bf16 [n] out or NULL.  Rejected before any launch: a NULL among
 * flow_cond / x / m0 / m1 / last_sample / s, a float pointer that is not 4-byte aligned, an order outside 1..2.  16 bytes per lane
 * when every pointer is 16-byte aligned, element-wise otherwise.  No allocation, no host read: capturable. */
int mmpl_cfg_unipc_step_f32(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* last_sample,
                            void* x_bf16, size_t n, const MmplUniPCStepF32* s, mmpl_stream_t stream);
int mmpl_cfg_dpmpp_step_f32(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* x_bf16, size_t n,
                            const MmplDpmppStep* s, mmpl_stream_t stream);
/* Device-resident forms, the protocol of mmpl_cfg_unipc_step_table: the scalars of step *step_dev are read from
 * table_dev[*step_dev] (n_steps entries, device memory), then *step_dev += 1 and the next step's timestep
 * (timestep_table_dev[*step_dev]) is written to timestep_dev[0..n_timestep).  Once *step_dev has reached n_steps a launch changes
 * nothing, x_bf16 included.  Also rejected: a NULL table / counter / timestep pointer, n_steps < 1, n_timestep < 0. */
int mmpl_cfg_unipc_step_f32_table(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* last_sample,
                                  void* x_bf16, size_t n, const MmplUniPCStepF32* table_dev, int* step_dev, float* timestep_dev,
                                  const float* timestep_table_dev, int n_timestep, int n_steps, mmpl_stream_t stream);
int mmpl_cfg_dpmpp_step_f32_table(const void* flow_cond, const void* flow_uncond, void* x, void* m0, void* m1, void* x_bf16, size_t n,
                                  const MmplDpmppStep* table_dev, int* step_dev, float* timestep_dev,
                                  const float* timestep_table_dev, int n_timestep, int n_steps, mmpl_stream_t stream);

/* Few-step (Self-Forcing / CausVid) latent update of CausalInferencePipeline.inference (pipeline/causal_inference.py:176-197):
 * WanDiffusionWrapper._convert_flow_pred_to_x0 (utils/wan_wrapper.py:172-199) then FlowMatchScheduler.add_noise
 * (utils/scheduler.py:160-176), per element of n bf16 values:
 *   x0_out = bf16(float(double(x) - sigma_t * double(flow)))                       (the reference's fp64 chain)
 *   x      = bf16(fp32(fp32(1 - sigma_next) * x0) + fp32(sigma_next * noise))    only if noise != NULL (fp32 rounding per op)
 * flow / x / noise / x0_out: dev bf16 [n]; x0_out may point into the middle of a larger latent (any alignment: 16-byte aligned
 * operands take the vector path).  No host read-back, no allocation: capturable. */
int mmpl_fewstep_update(const void* flow, void* x, const void* noise, void* x0_out, size_t n, double sigma_t, float sigma_next,
                        mmpl_stream_t stream);

/* ---- Wan 3D causal VAE (wan/modules/vae.py:483-569 behind WanVAEWrapper, utils/wan_wrapper.py:54-113) ----
 * Weights: mmpl_vae_num_weights() dev pointers in the order of mmpl_vae_weight_name(i): the reference's state_dict keys, conv
 * weights repacked host-side to [Cout, taps * Cin] (tap-major, Cin contiguous; Cin 3/16 zero-padded to 32, decoder.head Cout
 * 3 -> 4).  Every 3x3(x3) stride-1 conv is listed TWICE: "<conv>.weight" as above and a synthetic entry "<conv>.weight.frag" =
 * the same [Cout, taps * Cin] matrix in the fragment-major packing conv_halo_kernel loads (Cout zero-padded to a multiple of 16):
 * element (n, tap, c) at ((((c / 32) * taps + tap) * (Cout_pad / 16) + n / 16) * 4 + (c % 32) / 8) * 16 + n % 16) * 8 + c % 8,
 * i.e. per (32-channel chunk, tap, 16-row group) the 64 lanes' 16 bytes back to back, lane = 16 * (8-channel k chunk) + row
 * (mmpl_amd/vae.py VaeEngine._frag_pack is the reference packer).  bind_weights rejects any other count: a caller that binds
 * by state-dict name must produce the .frag entries too.
 * mode 0 = decode, 1 = encode.  mean / inv_std: host float[16] (bf16-rounded values of the wrapper's scale tensors).
 * Geometry: any lat_h, lat_w >= 2.  The attention of the middle blocks runs over lat_h * lat_w tokens; where that is no multiple
 * of 4 (3 x 5) the scores GEMM, which stores four columns at a time, runs over the token count rounded up to 4 against zero key
 * rows whose scores the softmax does not read. */
typedef struct MmplVae MmplVae;
int mmpl_vae_num_weights(void);
const char* mmpl_vae_weight_name(int i);
int mmpl_vae_create(int lat_h, int lat_w, MmplVae** out);
void mmpl_vae_destroy(MmplVae* v);
int mmpl_vae_bind_weights(MmplVae* v, const void* const* dev_ptrs, int n);
size_t mmpl_vae_workspace_bytes(MmplVae* v, int mode);
/* WanVAE_.decode: z dev bf16 [n_frames, 16, lat_h, lat_w] -> out dev float32 [1 + 4(n_frames-1), 3, 8 lat_h, 8 lat_w], clamped */
int mmpl_vae_decode(MmplVae* v, const void* z, int n_frames, const float* mean, const float* inv_std, void* out, void* workspace,
                    size_t workspace_bytes, mmpl_stream_t stream);
/* WanVAE_.encode: px dev bf16 [3, n_px_frames = 1 + 4k, 8 lat_h, 8 lat_w] -> out dev float32 [1 + k, 16, lat_h, lat_w] (normalised mu) */
int mmpl_vae_encode(MmplVae* v, const void* px, int n_px_frames, const float* mean, const float* inv_std, void* out, void* workspace,
                    size_t workspace_bytes, mmpl_stream_t stream);

/* ---- streaming decode: WanVAE_.cached_decode / clear_cache (wan/modules/vae.py:571-609) behind
 * WanVAEWrapper.decode_to_pixel(use_cache=True) (utils/wan_wrapper.py:90-113) ----
 * A MmplVaeStream is one decoded video in progress: every causal conv's feature cache (the reference's feat_map) stays in the
 * caller's workspace between calls, the handle keeps where each cache ring stands and how many latent frames went through.
 * The handle borrows the MmplVae it was created on (destroy the stream first) and can be created before the weights are bound. */
typedef struct MmplVaeStream MmplVaeStream;
int mmpl_vae_stream_create(MmplVae* v, MmplVaeStream** out);
void mmpl_vae_stream_destroy(MmplVaeStream* s);
/* WanVAE_.clear_cache: the next mmpl_vae_stream_decode starts a new video (and may bind another workspace).  Host-side only. */
int mmpl_vae_stream_reset(MmplVaeStream* s);
/* WanVAE_.cached_decode: decodes n_frames >= 1 MORE latent frames of the current video, z dev bf16 [n_frames, 16, lat_h, lat_w].
 * Writes 1 + 4(n_frames-1) pixel frames when these are the video's first frames (after create / reset), else 4 n_frames, and
 * reports the count in *n_px_frames_out (may be NULL).  out_format 0: dev float32 [T, 3, 8 lat_h, 8 lat_w] clamped to [-1, 1]
 * (mmpl_vae_decode's output: a video decoded in any split is bit-identical to the one-shot decode); out_format 1: dev uint8
 * [T, 8 lat_h, 8 lat_w, 3] (4-byte aligned) = those frames through (x * 0.5 + 0.5).clamp(0, 1) and
 * (v * 255.0).clamp(0, 255).to(uint8) of pipeline/causal_inference.py:256 and the video writer, in the same fp32 operations.
 * workspace: caller-owned, mmpl_vae_workspace_bytes(v, 0) bytes, holds the video's cache: it must be the SAME pointer from one
 * reset to the next (another pointer or a smaller size is an error, never a silent restart) and nothing else may write it in
 * between.  It is cleared (asynchronously, on `stream`) by the first decode after create / reset only.  All argument checks
 * run before the first HIP call.  No host read-back, no allocation. */
int mmpl_vae_stream_decode(MmplVaeStream* s, const void* z, int n_frames, const float* mean, const float* inv_std, void* out,
                           int out_format, int* n_px_frames_out, void* workspace, size_t workspace_bytes, mmpl_stream_t stream);

/* ---- TAEHV preview decoder: the decoder half of demo_utils/taehv.py (TAEHV.decode_video, checkpoint taew2_1.pth), the cheap
 * decoder for block-wise few-step output ----
 * Weights: mmpl_taehv_num_weights() dev pointers in the order of mmpl_taehv_weight_name(i) = exactly the reference's
 * "decoder.*" state-dict keys.  Every "*.weight" is bound in the fragment-major packing described above for "<conv>.weight.frag"
 * (Cin 16 zero-padded to 32 for decoder.1, Cout 3 zero-padded to 16 for decoder.22; a MemBlock's first conv keeps the reference's
 * input-channel order [x, past]); biases are bf16 [Cout] (decoder.22.bias zero-padded to 4).  mmpl_amd/taehv.py is the
 * reference packer.  mmpl_taehv_create and mmpl_taehv_workspace_bytes make no HIP call.
 * mmpl_taehv_decode CONTINUES the current video: z dev bf16 [n_frames, 16, lat_h, lat_w] in the pipeline's normalised latent space
 * (no mean / std) are its NEXT n_frames >= 1 latent frames; the first call after create / reset treats its first latent as the
 * video's first (zero memories).  Every call writes 4 n_frames pixel frames -- untrimmed, like the reference's decode_video -- and
 * reports the count in *n_px_frames_out (may be NULL).  out_format 0: dev float32 [T, 3, 8 lat_h, 8 lat_w], the network's raw
 * output (nominally [0, 1], unclamped, bf16-rounded); out_format 1: dev uint8 [T, 8 lat_h, 8 lat_w, 3] = (x.clamp(0, 1) * 255)
 * truncated, from the same bf16 value.  A video decoded in any split is bit-identical to the one-shot decode.
 * workspace: caller-owned, mmpl_taehv_workspace_bytes(v) bytes, holds the nine MemBlock memories: it must be the SAME pointer
 * from one reset to the next (another pointer or a smaller size is an error, never a silent restart) and nothing else may write
 * it in between.  It is cleared (asynchronously, on `stream`) by the first decode after create / reset only.  All argument
 * checks run before the first HIP call.  Everything is queued on `stream`: no host synchronisation, no read-back, no allocation,
 * and the launch sequence and every address are the same from call to call, so a call (not a video's first) can be captured
 * into a hipGraph and replayed as "the next latent frames". */
typedef struct MmplTaehv MmplTaehv;
int mmpl_taehv_num_weights(void);
const char* mmpl_taehv_weight_name(int i);
int mmpl_taehv_create(int lat_h, int lat_w, MmplTaehv** out);
void mmpl_taehv_destroy(MmplTaehv* v);
int mmpl_taehv_bind_weights(MmplTaehv* v, const void* const* dev_ptrs, int n);
size_t mmpl_taehv_workspace_bytes(MmplTaehv* v);
/* The next mmpl_taehv_decode starts a new video (and may bind another workspace).  Host-side only. */
int mmpl_taehv_reset(MmplTaehv* v);
int mmpl_taehv_decode(MmplTaehv* v, const void* z, int n_frames, void* out, int out_format, int* n_px_frames_out, void* workspace,
                      size_t workspace_bytes, mmpl_stream_t stream);

/* ---- TAEHV encoder: the other half of demo_utils/taehv.py (TAEHV.encode_video), pixels -> the streamed block's latents ----
 * A handle of its own.  Weights: mmpl_taehv_enc_num_weights() dev pointers in the order of mmpl_taehv_enc_weight_name(i) = exactly
 * the reference's "encoder.*" state-dict keys.  Every "*.weight" is bound fragment-major as for the decoder (a MemBlock's first conv
 * and TPool(2) keep the reference's input-channel order, [x, past] and [frame 2t, frame 2t + 1]); encoder.0.weight is bound as the
 * packed matrix [64, 32], column k = (3 ky + kx) * 3 + c, columns 27 .. 31 zero, as ONE fragment-major chunk with ntaps = 1;
 * encoder.17.weight has 16 rows; biases are bf16 [Cout].  mmpl_amd/taehv.py is the reference packer.  mmpl_taehv_enc_create and
 * mmpl_taehv_enc_workspace_bytes make no HIP call.
 * mmpl_taehv_encode CONTINUES the current video: px are its NEXT n_frames pixel frames, in_format 0: dev float32
 * [n_frames, 3, 8 lat_h, 8 lat_w] in [0, 1]; in_format 1: dev uint8 [n_frames, 8 lat_h, 8 lat_w, 3], read as bf16(u / 255).
 * n_frames must be >= 4 and a multiple of 4 (4 pixel frames per latent frame; a frame pair of the temporal pooling never straddles
 * two calls); anything else is an error.  z_out receives dev bf16 [n_frames / 4, 16, lat_h, lat_w] in the pipeline's normalised
 * latent space (no mean / std); the count goes to *n_latents_out (may be NULL).  The first call after create / reset starts from
 * zero memories.  A video encoded in any split is bit-identical to the one-shot encode.
 * workspace: caller-owned, mmpl_taehv_enc_workspace_bytes(e) bytes, holds the nine MemBlock memories: the SAME pointer from one
 * reset to the next (another pointer or a smaller size is an error), written by nothing else in between, cleared (asynchronously,
 * on `stream`) by the first encode after create / reset only.  All argument checks run before the first HIP call.  Everything is
 * queued on `stream`: no host synchronisation, no read-back, no allocation; the launch sequence and every address are the same from
 * call to call, so a call (not a video's first) can be captured into a hipGraph and replayed as "the next frames". */
typedef struct MmplTaehvEnc MmplTaehvEnc;
int mmpl_taehv_enc_num_weights(void);
const char* mmpl_taehv_enc_weight_name(int i);
int mmpl_taehv_enc_create(int lat_h, int lat_w, MmplTaehvEnc** out);
void mmpl_taehv_enc_destroy(MmplTaehvEnc* e);
int mmpl_taehv_enc_bind_weights(MmplTaehvEnc* e, const void* const* dev_ptrs, int n);
size_t mmpl_taehv_enc_workspace_bytes(MmplTaehvEnc* e);
/* The next mmpl_taehv_encode starts a new video (and may bind another workspace).  Host-side only. */
int mmpl_taehv_enc_reset(MmplTaehvEnc* e);
int mmpl_taehv_encode(MmplTaehvEnc* e, const void* px, int in_format, int n_frames, void* z_out, int* n_latents_out, void* workspace,
                      size_t workspace_bytes, mmpl_stream_t stream);

/* ---- umT5 text encoder (wan/modules/t5.py:267-312 behind WanTextEncoder, utils/wan_wrapper.py:15-51) ----
 * Weights (bf16 dev pointers): [token_embedding.weight, norm.weight] then per block
 * [norm1.weight, pack:attn.{q,k,v}.weight[3*dim_attn,dim], attn.o.weight, pos_embedding.embedding.weight[num_buckets,heads],
 *  norm2.weight, ffn.gate.0.weight, ffn.fc1.weight, ffn.fc2.weight].
 * mmpl_t5_encode: ids / mask dev int32 [text_len]; bucket dev int32 [2*text_len-1] = relative-position bucket of (j - i)
 * at index j - i + text_len - 1 (t5.py:240-264, computed host-side); out dev bf16 [text_len, dim], padding rows zeroed.
 * Unbound weights, a null ids / mask / bucket / out / workspace ("null argument") and a workspace that is too small are rejected
 * before the first HIP call.  mmpl_t5_workspace_bytes(NULL) is 0. */
typedef struct MmplT5Config {
  int vocab, dim, dim_attn, dim_ffn, num_heads, num_layers, num_buckets, text_len;
  float eps;
} MmplT5Config;
typedef struct MmplT5 MmplT5;
int mmpl_t5_num_weights(const MmplT5Config* cfg);
int mmpl_t5_create(const MmplT5Config* cfg, MmplT5** out);
void mmpl_t5_destroy(MmplT5* h);
int mmpl_t5_bind_weights(MmplT5* h, const void* const* dev_ptrs, int n);
size_t mmpl_t5_workspace_bytes(const MmplT5* h);
int mmpl_t5_encode(MmplT5* h, const int* ids, const int* mask, const int* bucket, void* out, void* workspace,
                   size_t workspace_bytes, mmpl_stream_t stream);

/* ---- Wan-I2V image cross-attention (wan/modules/model.py:224-266 WanI2VCrossAttention, :469-481 MLPProj).
 * mmpl_i2v_img_proj : clip_fea [n_tok=257, clip_dim=1280] -> context_img [n_tok, dim]; w = {proj.0.weight, proj.0.bias,
 *                     proj.1.weight, proj.1.bias, proj.3.weight, proj.3.bias, proj.4.weight, proj.4.bias} (LayerNorm eps 1e-5,
 *                     erf-GELU -- torch defaults).
 * mmpl_i2v_img_kv   : k_img = norm_k_img(k_img(context_img)), v_img = v_img(context_img)  (once per prompt and layer).
 * mmpl_i2v_cross_attn: out = o(attention(q, k_txt, v_txt) + attention(q, k_img, v_img)), q = norm_q(q(x)); x, out [Lq, dim]. */
size_t mmpl_i2v_img_proj_workspace_bytes(int n_tok, int clip_dim, int dim);
int mmpl_i2v_img_proj(const void* clip_fea, int n_tok, int clip_dim, int dim, const void* const* w, void* out, void* workspace,
                      size_t workspace_bytes, mmpl_stream_t stream);
int mmpl_i2v_img_kv(const void* ctx_img, int n_tok, int dim, const void* wk, const void* bk, const void* wv, const void* bv,
                    const void* norm_k_img_w, float eps, void* k_out, void* v_out, mmpl_stream_t stream);
size_t mmpl_i2v_cross_attn_workspace_bytes(int Lq, int dim);
int mmpl_i2v_cross_attn(const void* x, int Lq, int dim, const void* wq, const void* bq, const void* norm_q_w, float eps,
                        const void* k_txt, const void* v_txt, int n_txt, const void* k_img, const void* v_img, int n_img,
                        const void* wo, const void* bo, void* out, void* workspace, size_t workspace_bytes, mmpl_stream_t stream);

/* CLIP ViT-H/14 vision tower of Wan-I2V: VisionTransformer.forward(x, use_31_block=True) (wan/modules/clip.py:209-327) behind
 * CLIPModel.visual (clip.py:527-542; the bicubic resize / normalisation / im2col are the caller's).
 *   patches : dev [n_patch, pk] bf16, im2col of the normalised image in (c, ky, kx) order, K zero-padded to a multiple of 64
 *   gw      : 5 dev pointers  patch_embedding.weight [dim, pk], cls_embedding [dim], pos_embedding [n_patch+1, dim], pre_norm.{weight,bias}
 *   lw      : 12 per block    norm1.{weight,bias}, to_qkv.{weight [3*heads*128, dim], bias}, proj.{weight [dim, heads*128], bias},
 *                             norm2.{weight,bias}, mlp.0.{weight,bias}, mlp.2.{weight,bias} -- heads padded from head_dim to 128
 *   out     : dev [n_patch+1, dim] bf16, the tokens after n_blocks blocks (31 of the 32 for Wan-I2V) */
size_t mmpl_clip_visual_workspace_bytes(int n_tok, int dim, int mlp_dim, int heads);
int mmpl_clip_visual(const void* patches, int n_patch, int pk, int dim, int mlp_dim, int heads, int head_dim, int n_blocks,
                     const void* const* gw, const void* const* lw, float eps, void* out, void* workspace, size_t workspace_bytes,
                     mmpl_stream_t stream);

/* ---- Kernel-level entry points of the VAE / TAEHV kernels, for kernel-level tests and tools (tests/test_vae_kernels_gpu.py,
 * tests/test_taehv_kernels_gpu.py) ----
 * One launch of vae_kernels.hip / taehv_kernels.hip on plain arguments, as mmpl_gemm / mmpl_layernorm are for the DiT kernels.  The
 * product never calls them (mmpl_vae_* / mmpl_taehv_* drive the same launchers); they add no arithmetic.  All pointers are device
 * bf16 unless stated.  Every argument check runs before the first HIP call and a rejected call launches nothing: null pointers,
 * non-positive sizes, more than 2^31 - 1 pixels in one launch (mmpl_vae_conv / _norm / _upsample / _zprep / _mu_out / _px_in / _px_out / _px_out_u8, mmpl_taehv_px_out; mmpl_taehv_prep: 2^25 - 1),
 * misaligned pointers (the kernels move 8 / 16 bytes per access), more than 8 ring or norm frames, and whatever the launcher itself
 * rejects.  The checks bound what a kernel reaches by the sizes stated in the call; "reach" below is how large
 * each buffer must then be.
 *
 * mmpl_vae_conv: one CausalConv3d / Conv2d as vae.hip's conv() / cached_conv3() launch it.  tap (a, b, d) reads the padded source
 * pixel (t * st + a, y * sy + b, x * sx + d) of output pixel (t, y, x): the caller has applied the zero padding.
 *   src     [Tp, Hp, Wp, Cin], Tp = (To - 1) * st + kt frames; required (Ho - 1) * sy + kh <= Hp, (Wo - 1) * sx + kw <= Wp, Cin % 32 == 0.
 *   frames  NULL, or a host array of n_frames = To + kt - 1 <= 8 pointers: source frame j is frames[j] ([Hp, Wp, Cin]) instead of
 *           src + j * Hp * Wp * Cin (src may then be NULL).  Only conv_halo_kernel reads ring slots: any other shape is rejected.
 *   W       [N, kt * kh * kw * Cin] (tap-major, Cin contiguous), always required.  N % 4 == 0.
 *   Wfrag   NULL or the fragment-major packing of W (see "<conv>.weight.frag" above): Cin / 32 * ntaps * ceil(N / 16) * 16 * 32
 *           elements, i.e. the rows are zero-padded to a multiple of 16.  With it, a 3x3(x3 | x1) stride-1 conv out of a source padded
 *           by one pixel (Hp == Ho + 2, Wp == Wo + 2) with N % 96 == 0 or N <= 16 takes conv_halo_kernel.
 *   bias    [N]; read four values at a time (N % 4 == 0: the decoder head's three channels are padded to four in W, Wfrag and bias).
 *   dst     [>= dt0 + To, Hd, Wd, ldd]: output (t, y, x, n) -> (t + dt0, y + dy0, x + dx0, n); required dy0 + Ho <= Hd, dx0 + Wo <= Wd,
 *           ldd >= N, ldd % 4 == 0.  Nothing else of dst is written.  NULL only with ngamma.
 *   res     NULL or plain [To * Ho * Wo, ldres], ldres >= N: out = bf16(bf16(acc + bias) + res).
 *   ngamma  NULL or [96]: the consumer's RMS_norm * nscale * gamma + SiLU of the bf16 output, written to the interior of
 *           nframes[t] ([Ho + 2, Wo + 2, 96], t < To <= 8, host array of device pointers).  conv_halo_kernel<6> at N == 96 only.
 *   kernel_out (host, may be NULL): the kernel the launcher chose, 1 conv_igemm_kernel<3>, 2 conv_igemm_kernel<4>,
 *           3 conv_halo_kernel<6>, 4 conv_halo_kernel<1>; 0 when the call was rejected. */
int mmpl_vae_conv(const void* src, const void* const* frames, int n_frames, int Cin, int Hp, int Wp, int st, int sy, int sx, int kt,
                  int kh, int kw, const void* W, const void* Wfrag, const void* bias, int To, int Ho, int Wo, int N, void* dst, int Hd,
                  int Wd, int ldd, int dt0, int dy0, int dx0, const void* res, int ldres, const void* ngamma, float nscale,
                  void* const* nframes, int* kernel_out, mmpl_stream_t stream);
/* norm_act_pad_kernel: src plain [T * H * W, C] (C % 8 == 0, C <= 1024) -> dst [>= dt0 + T, Hd, Wd, ldd] at (t + dt0, y + dy0, x + dx0),
 * channels [0, C) (ldd >= C, ldd % 8 == 0).  gamma NULL: a copy; else [C]: RMS_norm (x / bf16(||x||), * scale, * gamma, each rounded
 * to bf16), then SiLU if silu. */
int mmpl_vae_norm(const void* src, int T, int H, int W, int C, const void* gamma, float scale, int silu, void* dst, int Hd, int Wd,
                  int ldd, int dt0, int dy0, int dx0, mmpl_stream_t stream);
/* upsample_pad_kernel: src [Ts, H, W, lds] -> nearest x2 into the interior of dst [To, Hd = 2H + 2, Wd = 2W + 2, C].  interleave 0:
 * Ts = To, lds >= C; 1: Ts = To / 2, lds >= 2C and output frame T takes channels [(T & 1) * C, +C) of source frame T / 2. */
int mmpl_vae_upsample(const void* src, int lds, int C, int H, int W, int To, int interleave, void* dst, int Hd, int Wd,
                      mmpl_stream_t stream);
/* softmax_rows_kernel: scores dev float32 [rows, ld] (cols valid) -> p bf16 [rows, ldp], columns [cols, ldp) zeroed. */
int mmpl_vae_softmax(const void* scores, int ld, void* p, int ldp, int rows, int cols, mmpl_stream_t stream);
/* transpose_kernel: v [rows, C] (row stride ld >= C) -> vt [C, ldt], ldt >= rows, columns [rows, ldt) zeroed. */
int mmpl_vae_transpose(const void* v, int ld, void* vt, int ldt, int rows, int C, mmpl_stream_t stream);
/* z_prep_kernel: z [F, 16, h, w] -> bf16(bf16(z / inv_std) + mean) -> 1x1x1 conv w2 [16, 16] + b2 [16] -> channels [0, 16) of the
 * interior of dst [>= dt0 + F, h + 2, w + 2, 32] at frame f + dt0.  mean / inv_std: host float[16]. */
int mmpl_vae_zprep(const void* z, int F, int h, int w, const float* mean, const float* inv_std, const void* w2, const void* b2, void* dst,
                   int dt0, mmpl_stream_t stream);
/* mu_out_kernel: enc [F * h * w, 32] -> rows [0, 16) of the 1x1x1 conv w1 [32, 32] + b1 [32] -> (mu - mean) * inv_std ->
 * out dev float32 [>= f_out + F, 16, h, w] at frame f + f_out.  mean / inv_std: host float[16]. */
int mmpl_vae_mu_out(const void* enc, const void* w1, const void* b1, const float* mean, const float* inv_std, void* out, int F,
                    int f_out, int h, int w, mmpl_stream_t stream);
/* px_in_kernel: px [3, Ttot, H, W] (t0 + T <= Ttot) -> channels [0, 3) of the interior of dst [>= dt0 + T, H + 2, W + 2, 32]: frame
 * t0 + t goes to frame dt0 + t.  Three channels per pixel are written and nothing else: border, channels [3, 32) and the frames in
 * front of dt0 keep what they held.  2-byte accesses. */
int mmpl_vae_px_in(const void* px, void* dst, int Ttot, int t0, int T, int H, int W, int dt0, mmpl_stream_t stream);
/* px_out_kernel: src [T, H, W, 4] (8-byte aligned; the fourth channel is the decoder head's padding and is dropped) ->
 * out dev float32 [>= t_out + T, 3, H, W] at frame t + t_out, clamp(-1, 1) of the bf16 value. */
int mmpl_vae_px_out(const void* src, void* out, int T, int H, int W, int t_out, mmpl_stream_t stream);
/* px_out_u8_kernel: src [T, H, W, 4] (16-byte aligned) -> out dev uint8 [>= t_out + T, H, W, 3] (4-byte aligned) at frame t + t_out:
 * (x.clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1), then (v * 255.0).clamp(0, 255) truncated, in float32.  A lane converts 4 consecutive
 * pixels: W % 8 == 0 and T * H * W % 4 == 0 are required. */
int mmpl_vae_px_out_u8(const void* src, void* out, int T, int H, int W, int t_out, mmpl_stream_t stream);
/* taehv_conv_kernel, TaehvConvArgs (taehv_kernels.h) field for field: a 3x3 (ntaps 9) or 1x1 (ntaps 1) conv over padded frames
 * [Ho + 2, Wo + 2, C] with a zero border, out = bf16(relu?(acc + bias? + skip?)).
 *   src0 / src1  output frame f reads src0 + f * fs0 (C0 channels) and, when C1 > 0, src1 + f * fs1 (C1 channels) as one K axis
 *           (elements; fs % 8 == 0).  up = 1: the source frames are [Ho / 2 + 2, Wo / 2 + 2, C] and nearest x2 is folded in.
 *   Wfrag   the fragment-major packing of [Nw, ntaps * (C0 + C1)]: (C0 + C1) / 32 * ntaps * Nw * 32 elements, Nw % 64 == 0 or % 16.
 *   bias    NULL or [N rounded up to 4].  N <= Nw channels are stored per pixel (N % 4 == 0).
 *   dst     T * (Nw / Nsplit) frames [Ho + 2, Wo + 2, ldd] of stride fsd: channel n of frame f -> frame f * (Nw / Nsplit) + n / Nsplit,
 *           channel n % Nsplit; interiors only.  ldd >= min(N, Nsplit).
 *   skip    NULL or T frames [Ho + 2, Wo + 2, Nw] of stride fss (N == Nw); keep: NULL or one such frame, receives the interior of
 *           the skip of frame T - 1. */
int mmpl_taehv_conv(const void* src0, const void* src1, long long fs0, long long fs1, int C0, int C1, int up, int ntaps,
                    const void* Wfrag, const void* bias, int Nw, int N, int T, int Ho, int Wo, void* dst, long long fsd, int ldd,
                    int Nsplit, int relu, const void* skip, long long fss, void* keep, mmpl_stream_t stream);
/* taehv_prep_kernel: z [16, h, w] -> bf16(tanh(z / 3) * 3) -> channels [0, 16) of the interior of dst [h + 2, w + 2, 32] (16-byte aligned). */
int mmpl_taehv_prep(const void* z, void* dst, int h, int w, mmpl_stream_t stream);
/* taehv_px_out_kernel: head frames src [T, H + 2, W + 2, 4] (8-byte aligned; interiors are read, the fourth channel is the head's
 * padding and is dropped) -> out at frame t + t_out.  out_format 0: dev float32 [>= t_out + T, 3, H, W] (4-byte aligned), the bf16
 * value as it is (no clamp; NaN and inf pass through); 1: dev uint8 [>= t_out + T, H, W, 3] = (x.clamp(0, 1) * 255) truncated, in
 * float32 from the same bf16 value.  One thread per pixel, 1- and 4-byte stores: no condition on W.  At most 2^31 - 1 pixels. */
int mmpl_taehv_px_out(const void* src, void* out, int out_format, int T, int H, int W, int t_out, mmpl_stream_t stream);
/* taehv_conv_in_kernel (taehv_enc_kernels.hip), the encoder's input layer: conv 3->64 3x3 (zero padding 1) + bias + ReLU straight
 * from the caller's pixels.  px: in_format 0 dev float32 [T, 3, H, W] (4-byte aligned); 1 dev uint8 [T, H, W, 3], read as
 * bf16(u / 255).  Wfrag: the packed [64, 32] matrix (k = (3 ky + kx) * 3 + c, k >= 27 zero) fragment-major, 2048 elements; bias [64].
 * dst: T frames [H + 2, W + 2, 64] of stride fsd (elements, % 4), interiors only. */
int mmpl_taehv_conv_in(const void* px, int in_format, const void* Wfrag, const void* bias, int T, int H, int W, void* dst,
                       long long fsd, mmpl_stream_t stream);
/* taehv_conv_s2_kernel: 3x3 stride-2 conv without bias, out = bf16(relu?(acc)): output (y, x) reads padded source rows 2y .. 2y + 2,
 * columns 2x .. 2x + 2.  src: T frames [2 Ho + 2, 2 Wo + 2, C] of stride fs (elements, % 8), C % 32 == 0; Wfrag: the fragment-major
 * packing of [Nw, 9 C], Nw % 64 == 0; dst: T frames [Ho + 2, Wo + 2, Nw] of stride fsd (% 4), interiors only. */
int mmpl_taehv_conv_s2(const void* src, long long fs, int C, const void* Wfrag, int Nw, int T, int Ho, int Wo, void* dst,
                       long long fsd, int relu, mmpl_stream_t stream);
/* taehv_z_out_kernel: head frames src [T, h + 2, w + 2, 16] (16-byte aligned) -> out bf16 [>= f_out + T, 16, h, w] at frame f_out. */
int mmpl_taehv_z_out(const void* src, void* out, int T, int h, int w, int f_out, mmpl_stream_t stream);
/* The GEMM (gemm.hip) in every form the DiT forward, T5, CLIP and the VAE launch it, for tests/test_gemm_forms_gpu.py: the arguments
 * of mmpl_gemm_scratch plus what only the internal callers could set.  mmpl_gemm / _tickets / _scratch are unchanged.
 *   epi     0-4 as mmpl_gemm; 5: C is dev float32 [M, ldc], C = float(alpha * acc), 16-byte aligned, bias must be NULL; 6: bias, and the columns
 *           n >= v_col0 of row m go to v_dst[m / rows_per_frame] + (m % rows_per_frame) * v_ld + (n - v_col0) instead of C, whose
 *           columns >= v_col0 are not written (the V third of the fused qkv projection into per-frame KV pages).
 *   A       [M, lda], W [N, ldw]: lda, ldw % 8 == 0 and >= K, K % 64 == 0, 16-byte aligned.  bias NULL (= 0) or [N].  N % 4 == 0.
 *   C       [M, ldc], ldc % 4 == 0, ldc >= N; rows m < M, columns n < N are written and nothing else.  8-byte aligned, as are res, gate,
 *           bias and the pages; when any of them (or N, a stride, v_col0, v_ld) is not 8-element aligned the 256 x 256 kernels take
 *           their direct 8-byte epilogue instead of the LDS-staged 16-byte one, as they do for epi 3 with rows_per_frame < 128.
 *   res     epi 3 / 4: [M, ldres], ldres >= N, ldres % 4 == 0; may be C itself.  gate (epi 3): [ceil(M / rows_per_frame),
 *           gate_frame_stride] with N valid columns, gate_frame_stride % 4 == 0; row m uses gate row m / rows_per_frame.  With more
 *           than one frame (M > rows_per_frame) gate_frame_stride is >= N, or 0 for one gate row shared by every frame; gate holds
 *           (frames - 1) * gate_frame_stride + N elements.
 *   alpha   epi 5 only.
 *   batch   >= 1.  batch > 1 (epi 0, 1, 2, 5; small-problem kernel only, which the launcher then always picks): problem b reads
 *           A + b * sA, W + b * sW and writes C + b * sC (elements of C's type); sA, sW % 8 == 0, sC % 4 == 0.  A must hold
 *           (batch - 1) * sA + (M - 1) * lda + K elements, W likewise, C (batch - 1) * sC + (M - 1) * ldc + N.
 *   v_dst   epi 6: host array of 1 <= n_v_dst <= 8 device pages with n_v_dst * rows_per_frame >= M; page f holds
 *           min(rows_per_frame, M - f * rows_per_frame) rows of v_ld >= N - v_col0 elements (v_ld, v_col0 % 4 == 0, 0 < v_col0 < N),
 *           of which the first N - v_col0 are written.
 *   scratch NULL, or mmpl_gemm_scratch_bytes() device bytes, 256-byte aligned, as for mmpl_gemm_scratch (first 2048 bytes zero before
 *           and after every launch).  With scratch NULL: tile_counter NULL, or 8 device ints as for mmpl_gemm_tickets.
 *   plan_out NULL or 6 host ints, filled from the launcher's own plan before the launch (all 0 when the call is rejected):
 *           [0] kernel: 1 gemm_bf16_kernel (128 x 128, small problems and every batched one), 2 gemm_bf16_v2_kernel (256 x 128),
 *               3 gemm_bf16_v6_kernel, 4 gemm_bf16_v8_kernel (256 x 256);
 *           [1] tail launch for the partial last round of 256 x 256 tiles: 0 none, 1 split-K, 2 128 x 128 quadrants on the DMA-ring
 *               body (8 tile buffers of LDS), 3 the same on the register-staged body (4 tile buffers);
 *           [2] 1 = LDS-staged epilogue (main launch and split-K tail; the 128 x 128 quadrants of a tail always store directly);
 *           [3] blocks of the main launch (0: skipped, every tile runs in the tail launch);
 *           [4] blocks of the tail launch; [5] split-K parts per tail tile (1 = no split).
 * Every check runs before the first HIP call and a rejected call launches nothing. */
int mmpl_gemm_ex(const void* A, int lda, const void* W, int ldw, const void* bias, void* C, int ldc, int M, int N, int K, int epi,
                 const void* res, int ldres, const void* gate, int gate_frame_stride, int rows_per_frame, float alpha, int batch,
                 long long sA, long long sW, long long sC, void* const* v_dst, int n_v_dst, int v_col0, int v_ld, void* scratch,
                 size_t scratch_bytes, void* tile_counter, int* plan_out, mmpl_stream_t stream);

/* The attention kernels (attention.hip, attn_w64.hip) on every path mmpl_dit_forward can take through them, for
 * tests/test_attn_exact_gpu.py: the arguments of mmpl_attn_fwd_variant plus what only the internal callers could set.
 * mmpl_attn_fwd / _ws / _variant / _history are unchanged.
 *   q, o, pages  as mmpl_attn_fwd; additionally every ld >= 128 * num_heads, so the stated sizes bound what a launch reaches:
 *           q [Lq, ldq], o [Lq, ldo] (rows < Lq, columns < 128 * num_heads are written and nothing else), page p [page_rows, ldk / ldv].
 *   page_group   NULL (one group) or a host array of n_pages bytes: the allocation page p lies in.  The 64-rows-per-wave kernel
 *           orders the pages by (group, address) and merges back-to-back pages of one group into one longer page.
 *   variant 0 / 1 / 3 / 4 as mmpl_attn_fwd_variant; q_prescaled != 0 with variant 0 or 3 = the caller multiplied q by
 *           softmax_scale * log2(e) before rounding it (variant 4 is variant 3 with q_prescaled; variant 0 with q_prescaled is what
 *           mmpl_dit_forward's self-attention passes).  A prescaled q that resolves to the lock-step kernel is an error.
 *   cross   != 0: a text cross-attention launch.  With the lock-step kernel, ONE page and page_rows <= 128 this is attn_cross_kernel.
 *   last_row_copies  0 / 1: plain.  > 1 (lock-step kernels, one page): the page's last row stands for that many identical keys.
 *   workspace    NULL or scratch for the split-KV tail round (mmpl_attn_workspace_bytes() is always enough), 16-byte aligned.
 *   history, stats_dev  as mmpl_attn_fwd_history (64-rows-per-wave kernel; ignored by the others).
 *   plan_out NULL or 8 host ints, filled from the launcher's own plan before the launch (all 0 when the call is rejected):
 *           [0] kernel: 1 attn_fwd_kernel, 2 attn_cross_kernel<1>, 3 attn_cross_kernel<2>, 4 attn_w64_kernel;
 *           [1] pages the kernel walks (4: after the merge); [2] 64-row KV tiles per query block; [3] blocks of the main launch;
 *           [4] kernel 4: query blocks per XCD that run split over the KV tiles in the tail round (0 = none); [5] their parts (1 = none);
 *           [6] kernels 2, 3: 256-row query blocks per block; [7] blocks per head.
 * Every check runs before the first HIP call and a rejected call launches nothing. */
int mmpl_attn_fwd_ex(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                     const unsigned char* page_group, int ldk, int ldv, int n_pages, int page_rows, int Lq, int num_heads,
                     float softmax_scale, void* workspace, size_t workspace_bytes, int variant, int q_prescaled, int cross,
                     int last_row_copies, void* history, void* stats_dev, int* plan_out, mmpl_stream_t stream);

/* n_groups self-attentions of equal shape in one call, for tests/test_attn_groups_gpu.py: the samples of a batched forward, each
 * seeing its own pages only.  The arguments of mmpl_attn_fwd_ex (without cross and last_row_copies) plus the groups:
 *   q, o    [n_groups * group_rows, ld]: group g's queries are rows g * group_rows .. (group_rows need not be a multiple of 256: every
 *           group has ceil(group_rows / 256) query blocks of its own).  Rows past n_groups * group_rows and columns >= 128 * num_heads
 *           of o are not written.
 *   group_n_pages  host array of n_groups ints, each 1 .. 24; k_pages, v_pages, page_group (or NULL): host arrays of their sum, the
 *           groups' lists back to back; every page [page_rows, ldk / ldv].
 *   history NULL, or n_groups regions of mmpl_attn_history_bytes(group_rows, num_heads) bytes, group g's at g times that.
 * One grouped launch of attn_w64_kernel's body (attn_w64_groups_kernel: (group, head) is a virtual head of the work-item decode)
 * runs when every group resolves to the 64-rows-per-wave kernel, history is NULL and the groups' lists, each merged by itself, hold
 * at most 24 pages in all; otherwise the call makes one launch of mmpl_attn_fwd_ex's kind per group, which computes the same
 * (the lock-step variant, MMPL_ATTN_V1, a history, more than 24 merged pages).  Block for block the grouped launch does what the
 * per-group launches do, so the results are bit-equal wherever neither splits its tail round.
 *   plan_out NULL or 10 host ints (all 0 when the call is rejected): [0] .. [7] as mmpl_attn_fwd_ex -- of the grouped launch
 *           ([1] merged pages of all groups, [2] KV tiles of the longest group; the split-KV tail is decided by the same rule from
 *           the total item count and the shortest group's tiles), or of group 0's launch on the per-group path;
 *           [8] 1 = one grouped launch, 0 = one launch per group; [9] work items n_groups * num_heads * ceil(group_rows / 256).
 * Every check runs before the first HIP call and a rejected call launches nothing. */
int mmpl_attn_fwd_groups_ex(const void* q, int ldq, void* o, int ldo, const void* const* k_pages, const void* const* v_pages,
                            const unsigned char* page_group, const int* group_n_pages, int n_groups, int group_rows, int ldk, int ldv,
                            int page_rows, int num_heads, float softmax_scale, void* workspace, size_t workspace_bytes, int variant,
                            int q_prescaled, void* history, void* stats_dev, int* plan_out, mmpl_stream_t stream);

/* The norm / RoPE / elementwise kernels (elementwise.hip) one launch at a time, for tests/test_rowpass_exact_gpu.py.  mmpl_layernorm,
 * mmpl_qknorm_rope and mmpl_qknorm_rope_at are unchanged.  Every check runs before the first HIP call, with one message per check; a
 * rejected call launches nothing and leaves plan_out all 0.  Rows are moved 16 bytes per lane: x, y, q, k, v, the column vectors,
 * the gains and the pages are 16-byte aligned and every ld a multiple of 8 elements.
 *
 * mmpl_layernorm_ex: the arguments of mmpl_layernorm plus two host-side overrides and the plan.
 *   x [rows, ldx], y [rows, ldy]: ldx, ldy >= d; d % 8 == 0, d <= 5120; columns < d of rows < rows are read / written, nothing else.
 *   modulation form (w NULL): row r takes frame r / rows_per_frame; scale and shift each hold
 *           (ceil(rows / rows_per_frame) - 1) * mod_frame_stride + d elements; mod_frame_stride >= 0 and % 8 == 0, rows_per_frame >= 1.
 *   affine form: w and b [d].
 *   pipeline  -1: the launcher's choice (layernorm_pipelined_kernel where NIT = ceil(d / 512) >= 6 and rows >= MMPL_LN_PIPELINE_MIN_ROWS),
 *           0: never, 1: always -- still only where NIT >= 6, otherwise rejected.
 *   groups_per_block  0: the launcher's choice (one round of resident blocks); > 0: that many 4-row groups per block, with the
 *           pipelined kernel only (otherwise rejected).
 *   plan_out NULL or 7 host ints, filled from the launcher's own plan before the launch:
 *           [0] kernel: 1 layernorm_kernel, 2 layernorm_pipelined_kernel, 3 qknorm_kernel; [1] NIT as instantiated (1, 2, 3, 4, 6, 8, 10);
 *           [2] FULL (kernels 2, 3); [3] kernels 2, 3: the blocks counted resident at once; [4] 4-row groups per block;
 *           [5] grid x; [6] grid y.
 *
 * mmpl_qknorm_ex: all of the QK-norm launch as mmpl_dit_forward makes it.  q [rows, ldq] in place; k NULL or [rows, ldk], normed
 * (and rotated) into the pages; v NULL or [rows, ldv], copied into the pages (needs k); each ld >= d, d % 128 == 0, d <= 5120.
 *   wq, wk  gains [d] (wk with k).  q_scale: q is multiplied by it before its one rounding; 0 = 1.
 *   rope != 0: cos_tab / sin_tab are dev float32 [1024][64], 4-byte aligned: row = position, column = rotary pair of the 128-wide head;
 *           pairs 0-21 take the frame's position frame_ids[f] + *frame_base_dev clamped to 0 .. 1023 (frame_ids: host, n_frames ints;
 *           frame_base_dev: dev int or NULL = 0), pairs 22-42 the token's grid row, 43-63 its grid column, token t of a frame at
 *           (t / grid_w, t % grid_w).  Required: rows == n_frames * rows_per_frame, 1 <= grid_w <= 1024 and
 *           (rows_per_frame - 1) / grid_w <= 1023 (only the frame position is clamped).  Row r belongs to frame r / rows_per_frame
 *           and goes to row r % rows_per_frame of k_dst / v_dst[frame] (host arrays of n_frames dev pages of rows_per_frame rows of d).
 *   rope == 0: no rotation; every row r goes to row r of k_dst[0] / v_dst[0] ([rows, d]); rows_per_frame and grid_w are ignored.
 *           With k NULL this is the plain in-place RMSNorm of T5, CLIP / i2v, the context K and the cross-attention q.
 *   n_frames  1 .. 8 in either case.  groups_per_block, plan_out: as above (grid y = 1 + k + v).
 *
 * mmpl_modulation: emod[l][f][k][:] = bf16(mod[l * mod_layer_stride + k * d + :] + e[f * e_frame_stride + (bcast ? : : k * d + :)]),
 *   k < nmod.  mod holds (n_layers - 1) * mod_layer_stride + nmod * d elements, e (n_frames - 1) * e_frame_stride + (bcast ? d : nmod * d),
 *   emod n_layers * n_frames * nmod * d.
 * mmpl_patchify: x [F, C, h, w] -> a [F * h/2 * w/2, lda], column c * 4 + ph * 2 + pw; columns >= 4 C are zeroed.  h, w even, lda >= 4 C.
 * mmpl_patchify2: mmpl_patchify of the channel concatenation of x [F, Cx, h, w] and y [F, Cy, h, w], which is never built: channels
 *   0 .. Cx-1 are x's, Cx .. Cx+Cy-1 are y's, columns >= 4 (Cx + Cy) are zeroed.  h, w even, lda >= 4 (Cx + Cy).  The same a, bit for bit.
 * mmpl_unpatchify: y [F * h/2 * w/2, ldy], column (ph * 2 + pw) * C + c -> out [F, C, h, w].  h, w even, ldy >= 4 C.
 * mmpl_sinusoid: t dev float32 [F] -> out [F, freq_dim] = [cos | sin] of t * 10000^(-k / (freq_dim / 2)) in double.  freq_dim even.
 * mmpl_silu: y[i] = bf16(x[i] / (1 + exp(-x[i]))), n elements.
 * mmpl_rows_equal_last: flags_dev[r] (dev int32 [rows]) = row r of x [rows, ld] equals row rows - 1 in its first d columns, bit for
 *   bit.  rows >= 1, d % 8 == 0, ld % 8 == 0, ld >= d, x 16-byte aligned. */
int mmpl_layernorm_ex(const void* x, int ldx, void* y, int ldy, int rows, int d, float eps, const void* scale, const void* shift,
                      int mod_frame_stride, int rows_per_frame, const void* w, const void* b, int pipeline, int groups_per_block,
                      int* plan_out, mmpl_stream_t stream);
int mmpl_qknorm_ex(void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* wq, const void* wk, int rows, int d,
                   float eps, float q_scale, int rope, const float* cos_tab, const float* sin_tab, int n_frames, const int* frame_ids,
                   const int* frame_base_dev, void* const* k_dst, void* const* v_dst, int rows_per_frame, int grid_w,
                   int groups_per_block, int* plan_out, mmpl_stream_t stream);
int mmpl_modulation(const void* mod, long long mod_layer_stride, const void* e, int e_frame_stride, int bcast, void* emod, int n_layers,
                    int n_frames, int nmod, int d, mmpl_stream_t stream);
int mmpl_patchify(const void* x, void* a, int lda, int F, int C, int h, int w, mmpl_stream_t stream);
int mmpl_patchify2(const void* x, const void* y, void* a, int lda, int F, int Cx, int Cy, int h, int w, mmpl_stream_t stream);
int mmpl_unpatchify(const void* y, int ldy, void* out, int F, int C, int h, int w, mmpl_stream_t stream);
int mmpl_sinusoid(const float* t, void* out, int F, int freq_dim, mmpl_stream_t stream);
int mmpl_silu(const void* x, void* y, size_t n, mmpl_stream_t stream);
int mmpl_rows_equal_last(const void* x, int ld, int rows, int d, int* flags_dev, mmpl_stream_t stream);

/* The glue kernels of the umT5 encoder (t5.hip) and of the CLIP / i2v path (i2v.hip) one launch at a time, for
 * tests/test_glue_exact_gpu.py: the launches mmpl_t5_encode, mmpl_i2v_img_proj, mmpl_i2v_cross_attn and mmpl_clip_visual make, with
 * their grid geometry.  Every check runs before the first HIP call, with one message per check; a rejected call launches nothing.
 * Tensors are dev bf16 unless stated; ids, bucket and mask are dev int32.
 *
 * mmpl_t5_gather: out[l][:] = emb[ids[l]][:], 16 bytes per access.  ids [L]; emb [vocab, dim]; out [L, dim]; dim % 8 == 0; emb and
 *   out 16-byte aligned.  PRECONDITION: every ids[l] lies in [0, vocab) -- the ids are device memory, which the entry cannot read,
 *   and an id outside the table makes the kernel read outside emb (T5Engine.encode checks the ids on the host).
 * mmpl_t5_softmax: scores dev float32 [H][L][L] -> p [H][L][L]; row (h, i), key j: bf16(bf16(scores) + bias), bias =
 *   pos_emb[bucket[j - i + L - 1] * H + h], or finfo(bfloat16).min where mask[j] == 0; softmax over j in fp32, rounded once.
 *   pos_emb [num_buckets, H]; bucket [2 L - 1] with every value in [0, num_buckets) (a PRECONDITION, like the ids); mask [L].
 *   L % 64 == 0 (the rule of mmpl_t5_create); H * L blocks must fit the grid.
 * mmpl_t5_transpose: v [L, ld], head h at column h * c -> vt [H][c][L].  ld >= H * c; v holds (L - 1) * ld + H * c elements, vt
 *   H * c * L.  (mmpl_t5_encode passes the V third of the fused qkv: v = qkv + 2 H c, ld = 3 H c.)
 * mmpl_t5_gated: f[i] = bf16(f[i] * gelu_tanh(g[i])), every tensor op of the reference's GELU rounded to bf16; f, g [n], f in place.
 * mmpl_t5_zero_pad: out [L, dim] in place: rows l with mask[l] == 0 become +0; mask [L].
 * mmpl_gelu_erf: x[i] = bf16(0.5 x[i] (1 + erf(x[i] / sqrt 2))) in fp32, in place; x [n].
 * mmpl_add: a[i] = bf16(a[i] + b[i]), one fp32 add; a, b [n], a in place. */
int mmpl_t5_gather(const int* ids, const void* emb, void* out, int L, int dim, mmpl_stream_t stream);
int mmpl_t5_softmax(const float* scores, const void* pos_emb, const int* bucket, const int* mask, void* p, int H, int L,
                    mmpl_stream_t stream);
int mmpl_t5_transpose(const void* v, int ld, void* vt, int L, int c, int H, mmpl_stream_t stream);
int mmpl_t5_gated(void* f, const void* g, size_t n, mmpl_stream_t stream);
int mmpl_t5_zero_pad(void* out, const int* mask, int L, int dim, mmpl_stream_t stream);
int mmpl_gelu_erf(void* x, size_t n, mmpl_stream_t stream);
int mmpl_add(void* a, const void* b, size_t n, mmpl_stream_t stream);

/* Optional per-kernel-class hipEvent timing (bench.py's live roofline numbers; off by default, not thread-safe).
 * kinds: 0 gemm, 1 self-attention, 2 cross-attention, 3 layernorm, 4 qk-norm/rope/kv-write, 5 elementwise, 6 cfg+unipc,
 * 7 vae.  on = 0 off, 1 every kind, > 1: only the kinds in the bit mask (on >> 1) (e.g. 2 << 1 | ... ; bench.py times the
 * self-attention only unless --profile-all, an event pair per op costs ~0.5 % of a step when every op is timed).
 * mmpl_profile_read synchronises the device, sums the event pairs recorded since enable/last read. */
int mmpl_profile_enable(int on);
int mmpl_profile_read(int n_kinds, double* ms, double* flops, long long* launches);

const char* mmpl_last_error(void);
const char* mmpl_version(void);

#ifdef __cplusplus
}
#endif
#endif
