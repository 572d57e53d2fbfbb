"""Host-side handle of the HIP Wan DiT forward (libmmpl_hip.so: mmpl_dit_*).

Mirrors what ``CausalFPSWanModel`` (MMPL_t2v/wan/modules/causal_fps_model.py:398-530, 708-837) offers the
wrapper: construct from the model dims, ``load_state_dict`` with the reference's keys, run one inference
forward against a per-layer KV cache.  PyTorch only owns the device memory here; all compute is in the library.

``model_type='i2v'`` (wan/modules/model.py:563-616: in_dim 36, ``img_emb`` = MLPProj(1280, dim), every block's
cross-attention a ``WanI2VCrossAttention``) adds the image stream: ``precompute_image_context(clip_fea)`` builds the
per-layer image K / V once per image, ``set_image_kv`` attaches them, and ``forward`` takes x with the conditioning video
``y`` concatenated on the channel axis (model.py:680-681); ``forward_full`` takes the two as separate tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib

# The library's packed weight slots, under the names mmpl_dit_weight_name reports: (g, layer prefix, num_layers, dim) -> tensor
_PACKERS = {
    "pack:blocks.*.modulation[L,6,dim]": lambda g, p, L, dim: torch.stack([g(f"blocks.{i}.modulation").reshape(6, dim) for i in range(L)]),
    "pack:self_attn.{q,k,v}.weight[3dim,dim]": lambda g, p, L, dim: torch.cat([g(p + f"self_attn.{x}.weight") for x in "qkv"]),
    "pack:self_attn.{q,k,v}.bias[3dim]": lambda g, p, L, dim: torch.cat([g(p + f"self_attn.{x}.bias") for x in "qkv"]),
}


def weight_slot_names(lib, per_layer: int) -> List[str]:
    """The library's global (per_layer 0) or per-layer (1) weight slots, in bind order."""
    names: List[str] = []
    while (n := lib.mmpl_dit_weight_name(len(names), per_layer)) is not None:
        names.append(n.decode())
    return names


def slot_tensors(lib, g, num_layers: int, dim: int, in_dim: int) -> List[torch.Tensor]:
    """What mmpl_dit_bind_weights takes, in the order the library reports its slots.  `g(key)` fetches one state-dict tensor; a plain
    slot name is that key ("blocks.N." in front of a per-layer one), a "pack:" one is built by its packer."""
    def slot(name: str, p: str = "") -> torch.Tensor:
        if name.startswith("pack:"):
            if name not in _PACKERS:
                raise KeyError(f"mmpl_dit_weight_name reports the packed slot {name!r}, which DitEngine has no packer for")
            return _PACKERS[name](g, p, num_layers, dim).contiguous()
        t = g(p + name)
        if name == "patch_embedding.weight":
            t = t.reshape(t.shape[0], -1)
            pe_k = (t.shape[1] + 63) // 64 * 64         # K of the patch GEMM: 4 * in_dim padded to a multiple of 64 (zeros)
            assert t.shape[1] == 4 * in_dim, (tuple(t.shape), in_dim)
            t = torch.nn.functional.pad(t, (0, pe_k - t.shape[1])).contiguous()
        return t

    per_layer = weight_slot_names(lib, 1)
    return [slot(n) for n in weight_slot_names(lib, 0)] + [slot(n, f"blocks.{i}.") for i in range(num_layers) for n in per_layer]


# DitEngine.forward(cache_mode=...): the step-cache modes of mmpl_dit_forward_*_cached (include/mmpl_hip.h)
CACHE_OFF, CACHE_RECORD, CACHE_REUSE = 0, 1, 2


class CrossKV(tuple):
    """(cross_k, cross_v) of one prompt, each [num_layers, text_len, dim], plus `rows`: rows `rows .. text_len-1` of every layer are
    copies of row `rows` (the zero-padded tail of the text context after the text embedding; `text_len` = no repeated tail).
    Unpacks like the plain pair; `rows` is a statement about the CONTENTS, so hand it on with any copy of them
    (`DitEngine.forward(..., cross_rows=kv.rows)`); a forward that is not given it attends over all text_len rows."""

    def __new__(cls, k: torch.Tensor, v: torch.Tensor, rows: int):
        self = super().__new__(cls, (k, v))
        self.rows = int(rows)
        return self


class DitEngine:
    def __init__(self, cfg: dict, lat_h: int, lat_w: int, device="cuda:0", max_frames: int = 7):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:      # 'cuda' != 'cuda:0' for torch.device.__eq__: normalise once
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lat_h, self.lat_w = lat_h, lat_w
        self.S = (lat_h // 2) * (lat_w // 2)
        self.dim, self.L = cfg["dim"], cfg["num_layers"]
        self.text_len = cfg.get("text_len", 512)
        self.text_dim = cfg.get("text_dim", 4096)
        self.max_frames = max_frames
        self.model_type = cfg.get("model_type", "t2v")
        assert self.model_type in ("t2v", "i2v")
        self.in_dim = cfg.get("in_dim", 36 if self.model_type == "i2v" else 16)
        self.clip_dim = cfg.get("clip_dim", 1280)
        lib = _lib.load()
        self._lib = lib
        c = _lib.MmplDitConfig(dim=cfg["dim"], ffn_dim=cfg["ffn_dim"], num_heads=cfg["num_heads"],
                               num_layers=cfg["num_layers"], text_dim=self.text_dim, freq_dim=cfg.get("freq_dim", 256),
                               in_dim=self.in_dim, out_dim=16, text_len=self.text_len, eps=cfg.get("eps", 1e-6), lat_h=lat_h,
                               lat_w=lat_w, max_frames=max_frames)
        self._c = c
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.mmpl_dit_create(C.byref(c), C.byref(h)), "mmpl_dit_create")
        self._h = h
        self._weights: List[torch.Tensor] = []
        self._ws: Dict[int, torch.Tensor] = {}
        self._ws2: Optional[torch.Tensor] = None
        self._ws_full: Dict[Tuple[int, bool], torch.Tensor] = {}    # forward_full: (frame count, second) -> scratch
        self._share: Optional[torch.Tensor] = None
        self._ctx_ws: Optional[torch.Tensor] = None
        self._i2v_w: Optional[dict] = None                 # img_emb + per-layer k_img / v_img / norm_k_img (model_type 'i2v')
        self._img_kv: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        self._attn_stats: Optional[torch.Tensor] = None
        self._warm = set()                                 # stage shapes (n_frames) that ran eagerly once: capture()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.mmpl_dit_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = "") -> None:
        """sd uses the reference's CausalFPSWanModel keys (optionally prefixed, e.g. 'model.' in MMPL .pt files,
        Wan_fps_inference_1gpu.py:66-68).  q/k/v are packed into one [3*dim, dim] operand."""
        dev, bf = self.device, torch.bfloat16

        def g(k):
            return sd[prefix + k].to(device=dev, dtype=bf).contiguous()

        w = slot_tensors(self._lib, g, self.L, self.dim, self.in_dim)
        n = self._lib.mmpl_dit_num_weights(C.byref(self._c))
        assert len(w) == n, (len(w), n)
        _lib.bind_weights(self._lib.mmpl_dit_bind_weights, self._h, w, "mmpl_dit_bind_weights")
        self._weights = w      # keep alive: the library borrows the pointers
        if self.model_type == "i2v":
            self._i2v_w = dict(
                img_emb=[g("img_emb." + k) for k in ("proj.0.weight", "proj.0.bias", "proj.1.weight", "proj.1.bias", "proj.3.weight",
                                                     "proj.3.bias", "proj.4.weight", "proj.4.bias")],
                layers=[[g(f"blocks.{i}.cross_attn." + k) for k in ("k_img.weight", "k_img.bias", "v_img.weight", "v_img.bias",
                                                                     "norm_k_img.weight")] for i in range(self.L)])

    # ------------------------------------------------------------------ diagnostics
    def enable_attn_stats(self) -> torch.Tensor:
        """Count the self-attention kernel's query blocks and what its data-dependent softmax passes did with them: int64 [5] on the
        device = {blocks, blocks whose max-free FAST pass failed and that the GENERAL pass redid (both paid), waves (64 rows) that
        held a failing row, blocks their history sent straight to the GENERAL pass, blocks whose FAST pass held on the references
        their history remembered}, incremented by every later forward.
        The counter's address is a kernel argument: a hipGraph captured while stats are on keeps counting on every replay
        whatever `disable_attn_stats` says later, and one captured while they are off never counts.  One atomic per 256-row
        block; `bench.py` switches it on for its diagnostic modes only."""
        if self._attn_stats is None:
            self._attn_stats = torch.zeros(5, dtype=torch.int64, device=self.device)
        _lib.check(self._lib.mmpl_dit_set_attn_stats(self._h, _lib.ptr(self._attn_stats)), "mmpl_dit_set_attn_stats")
        return self._attn_stats

    def disable_attn_stats(self) -> None:
        """Later eager forwards and later captures stop counting (graphs captured before keep their setting)."""
        _lib.check(self._lib.mmpl_dit_set_attn_stats(self._h, None), "mmpl_dit_set_attn_stats")

    def read_attn_stats(self, reset: bool = False) -> Tuple[int, int, int, int, int]:
        """(blocks run, blocks redone, waves that held a failing row, blocks sent straight to GENERAL, blocks whose FAST pass held on
        remembered references) since the counters were last zeroed."""
        if self._attn_stats is None:
            raise RuntimeError("DitEngine.read_attn_stats: enable_attn_stats() was never called on this engine")
        vals = tuple(int(v) for v in self._attn_stats.cpu())
        if reset:
            self._attn_stats.zero_()
        return vals

    def new_attn_history(self, n_frames: Optional[int] = None) -> torch.Tensor:
        """Zeroed history of the self-attention's softmax passes for `forward(attn_history=...)`: a state byte and 128 int16 lane
        references per (layer, head, 256-row query block, split part), sized for stages of up to `n_frames` frames (default: the
        engine's largest; ~160 MB for Wan 14B at 720p).  One buffer per (CFG branch, stage); `zero_()` it when the stage changes
        (include/mmpl_hip.h)."""
        n = self._lib.mmpl_dit_attn_history_bytes(self._h, self.max_frames if n_frames is None else n_frames)
        return torch.zeros(n, dtype=torch.uint8, device=self.device)

    def share_check_failures(self) -> int:
        """MMPL_CHECK_SHARE=1: share_in forwards since the last call whose layer-0 K / V differed from their share_out forward's
        (synchronises; 0 when the switch is off)."""
        n = C.c_longlong(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_dit_share_check_failures(self._h, C.byref(n), _lib.stream_ptr()), "mmpl_dit_share_check_failures")
        return n.value

    # ------------------------------------------------------------------ caches
    def new_kv_cache(self, n_slots: int = 15) -> Tuple[torch.Tensor, torch.Tensor]:
        """[num_layers, n_slots*S, dim] K and V; layer l is the reference's kv_cache[l]['k'] viewed [1, n_slots*S, H, 128]
        (casual_fps_inference.py:453-480)."""
        shape = (self.L, n_slots * self.S, self.dim)
        return (torch.zeros(shape, dtype=torch.bfloat16, device=self.device),
                torch.zeros(shape, dtype=torch.bfloat16, device=self.device))

    def precompute_context(self, context: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> CrossKV:
        """context: [L<=text_len, text_dim] -> per-layer cross-attention K, V [num_layers, text_len, dim] as a `CrossKV` (unpacks as
        (K, V); `.rows` = the leading rows that are distinct, see CrossKV).  `out`: write into these two buffers instead of new ones."""
        ctx = torch.zeros(self.text_len, self.text_dim, dtype=torch.bfloat16, device=self.device)
        ctx[:context.shape[0]] = context.to(device=self.device, dtype=torch.bfloat16)
        if out is None:
            ck = torch.empty(self.L, self.text_len, self.dim, dtype=torch.bfloat16, device=self.device)
            cv = torch.empty_like(ck)
        else:
            ck, cv = out
            for t in (ck, cv):
                assert t.shape == (self.L, self.text_len, self.dim) and t.dtype == torch.bfloat16 and t.is_contiguous() and t.device == self.device
        if self._ctx_ws is None:
            self._ctx_ws = torch.empty(self._lib.mmpl_dit_context_workspace_bytes(self._h), dtype=torch.uint8, device=self.device)
        rows = C.c_int(self.text_len)
        with torch.cuda.device(self.device):          # the stream handed to the library is this device's current stream
            _lib.check(self._lib.mmpl_dit_precompute_context(self._h, _lib.ptr(ctx), _lib.ptr(ck), _lib.ptr(cv), _lib.ptr(self._ctx_ws),
                                                             self._ctx_ws.numel(), C.byref(rows), _lib.stream_ptr()), "precompute_context")
        return CrossKV(ck, cv, rows.value)

    def precompute_image_context(self, clip_fea: torch.Tensor,
                                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """clip_fea: [257, clip_dim] (CLIP ViT-H penultimate-block tokens, clip.py:541) -> per-layer image (K, V)
        [num_layers, 257, dim]: img_emb (MLPProj, model.py:469-481), then k_img / norm_k_img and v_img of every block
        (model.py:251-252).  Once per image, like precompute_context once per prompt.  `out`: write into these two buffers instead
        of new ones -- the pair a captured graph holds by address (`set_image_kv`) is refreshed in place for the next image."""
        if self._i2v_w is None:
            raise RuntimeError("DitEngine: not an i2v model (or weights not loaded)")
        lib, d = self._lib, self.dim
        fea = clip_fea.to(device=self.device, dtype=torch.bfloat16).contiguous()
        n = fea.shape[0]
        assert fea.shape == (n, self.clip_dim)
        ctx_img = torch.empty(n, d, dtype=torch.bfloat16, device=self.device)
        ws = torch.empty(lib.mmpl_i2v_img_proj_workspace_bytes(n, self.clip_dim, d), dtype=torch.uint8, device=self.device)
        arr = (C.c_void_p * 8)(*[t.data_ptr() for t in self._i2v_w["img_emb"]])
        if out is None:
            img_k = torch.empty(self.L, n, d, dtype=torch.bfloat16, device=self.device)
            img_v = torch.empty_like(img_k)
        else:
            img_k, img_v = out
            for t in (img_k, img_v):
                assert t.shape == (self.L, n, d) and t.dtype == torch.bfloat16 and t.is_contiguous() and t.device == self.device
        with torch.cuda.device(self.device):
            _lib.check(lib.mmpl_i2v_img_proj(_lib.ptr(fea), n, self.clip_dim, d, arr, _lib.ptr(ctx_img), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr()), "mmpl_i2v_img_proj")
            for l, (kw, kb, vw, vb, nk) in enumerate(self._i2v_w["layers"]):
                _lib.check(lib.mmpl_i2v_img_kv(_lib.ptr(ctx_img), n, d, _lib.ptr(kw), _lib.ptr(kb), _lib.ptr(vw), _lib.ptr(vb), _lib.ptr(nk),
                                               self.cfg.get("eps", 1e-6), _lib.ptr(img_k[l]), _lib.ptr(img_v[l]), _lib.stream_ptr()),
                           "mmpl_i2v_img_kv")
        return img_k, img_v

    def set_image_kv(self, img_k: Optional[torch.Tensor], img_v: Optional[torch.Tensor]) -> None:
        """Attach (or, with None, detach) the per-layer image K / V that every later forward's cross-attention also attends to."""
        if img_k is None:
            _lib.check(self._lib.mmpl_dit_set_image_kv(self._h, None, None, 0), "mmpl_dit_set_image_kv")
            self._img_kv = None
            return
        assert img_k.shape == img_v.shape and img_k.shape[0] == self.L and img_k.shape[2] == self.dim and img_k.is_contiguous()
        _lib.check(self._lib.mmpl_dit_set_image_kv(self._h, _lib.ptr(img_k), _lib.ptr(img_v), img_k.shape[1]), "mmpl_dit_set_image_kv")
        self._img_kv = (img_k, img_v)      # keep alive: the library borrows the pointers

    def workspace(self, n_frames: int) -> torch.Tensor:
        if n_frames not in self._ws:
            nbytes = self._lib.mmpl_dit_workspace_bytes(self._h, n_frames)
            # one buffer sized for the largest stage serves all stages
            big = max(self._ws.values(), key=lambda t: t.numel(), default=None)
            if big is not None and big.numel() >= nbytes:
                self._ws[n_frames] = big
            else:
                self._ws[n_frames] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws[n_frames]

    def shared_block0_buffer(self, n_frames: int) -> torch.Tensor:
        """[n_frames * S, dim] bf16: x after block 0's self-attention residual, handed from the cond forward of a denoise step
        (`share_out`) to the uncond one (`share_in`).  One buffer, sized for the largest stage seen so far."""
        n = n_frames * self.S * self.dim
        if self._share is None or self._share.numel() < n:
            self._share = torch.empty(n, dtype=torch.bfloat16, device=self.device)
        return self._share

    def second_workspace(self, n_frames: int) -> torch.Tensor:
        """A private scratch buffer for a forward that runs CONCURRENTLY with another one of this engine (the uncond branch of a
        denoise step on a second stream): one buffer, sized for the largest stage seen so far, allocated outside any capture."""
        nbytes = self._lib.mmpl_dit_workspace_bytes(self._h, n_frames)
        if self._ws2 is None or self._ws2.numel() < nbytes:
            self._ws2 = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws2

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, t: torch.Tensor, frame_ids: Sequence[int], write_slots: Sequence[int],
                visible_slots: Sequence[int], k_cache: torch.Tensor, v_cache: torch.Tensor, cross_k: torch.Tensor,
                cross_v: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                cross_rows: Optional[int] = None, share_out: Optional[torch.Tensor] = None,
                share_in: Optional[torch.Tensor] = None, attn_history: Optional[torch.Tensor] = None,
                frame_base: Optional[torch.Tensor] = None, cache_mode: int = CACHE_OFF,
                residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x: [nF, in_dim, lat_h, lat_w] bf16 (i2v: x and y concatenated on the channel axis); t: [nF] float32 (device).
        Returns the flow prediction [nF, 16, lat_h, lat_w].
        `cross_rows`: the `CrossKV.rows` that belongs to the CONTENTS of cross_k / cross_v (rows cross_rows .. text_len-1 repeat one
        row): the text cross-attention then runs over cross_rows + 1 keys.  None = attend over all text_len rows.
        `share_out` / `share_in` ([nF * S, dim] bf16, see `shared_block0_buffer`): the two branches of classifier-free guidance run
        block 0's self-attention on identical inputs; the first forward leaves x after that residual in `share_out`, the second
        takes it as `share_in` and skips the attention and its output projection (include/mmpl_hip.h; bit-identical).
        `attn_history` (`new_attn_history()`): what the self-attention's softmax passes did on the previous forward of this (CFG
        branch, stage); blocks whose FAST pass failed then start in the GENERAL pass.  The output bits then depend on the forwards
        before (include/mmpl_hip.h); None = stateless.
        `workspace`: a private scratch buffer (>= workspace_bytes(nF)) for a forward that runs concurrently with another
        one on a different stream (cond / uncond); default: the engine's own.
        `frame_base`: an int32 device scalar; `frame_ids` are then relative to it (RoPE position = frame_ids[i] + its value WHEN THE
        KERNELS RUN, clamped to the tables' 0..1023): a forward captured into a hipGraph is replayed at another position in time by
        writing the scalar in stream order before the replay (mmpl_dit_forward_at).  None = absolute frame_ids.
        `cache_mode` / `residual` (`new_step_cache(nF)`): step caching, mmpl_dit_forward_at_cached -- CACHE_RECORD: this forward
        plus x after the last block minus x after the patch embedding left in `residual`; CACHE_REUSE: the patch embedding plus
        `residual`, then the head: no block runs, no K / V is written, the caches and cross K / V may be None.  CACHE_OFF (the
        default) is the uncached entry."""
        nF = x.shape[0]
        assert x.is_contiguous() and x.dtype == torch.bfloat16 and x.shape[1:] == (self.in_dim, self.lat_h, self.lat_w)
        assert t.dtype == torch.float32 and t.numel() == nF and t.is_cuda
        if self.model_type == "i2v" and self._img_kv is None:
            raise RuntimeError("DitEngine: an i2v model needs set_image_kv(*precompute_image_context(clip_fea)) before forward")
        if frame_base is not None:
            assert frame_base.dtype == torch.int32 and frame_base.numel() == 1 and frame_base.device == x.device, (frame_base.dtype, tuple(frame_base.shape))
        out = self._checked_out(x, share_out, share_in, attn_history, out)
        ws = self.workspace(nF) if workspace is None else workspace
        n_slots = k_cache.shape[1] // self.S
        ia = lambda v: (C.c_int * len(v))(*[int(i) for i in v])
        self._check_residual(cache_mode, residual, nF, x.device)
        with torch.cuda.device(self.device):          # the stream handed to the library is this device's current stream
            args = (self._h, _lib.ptr(x), _lib.ptr(t), nF, ia(frame_ids), ia(write_slots), ia(visible_slots), len(visible_slots),
                    _lib.ptr(k_cache), _lib.ptr(v_cache), n_slots, _lib.ptr(cross_k), _lib.ptr(cross_v),
                    self.text_len if cross_rows is None else int(cross_rows), _lib.ptr(share_out), _lib.ptr(share_in),
                    _lib.ptr(attn_history), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.ptr(frame_base), _lib.stream_ptr())
            if cache_mode == CACHE_OFF:
                _lib.check(self._lib.mmpl_dit_forward_at(*args), "mmpl_dit_forward")
            else:
                _lib.check(self._lib.mmpl_dit_forward_at_cached(*args, int(cache_mode), _lib.ptr(residual)), "mmpl_dit_forward_at_cached")
        return out

    def forward_groups(self, x: torch.Tensor, t: torch.Tensor, n_groups: int, frame_ids: Sequence[int], write_slots: Sequence[int],
                       visible_slots: Sequence[Sequence[int]], k_cache: torch.Tensor, v_cache: torch.Tensor,
                       cross: Sequence[Tuple[torch.Tensor, torch.Tensor]], out: Optional[torch.Tensor] = None,
                       workspace: Optional[torch.Tensor] = None, cross_rows: Optional[int] = None,
                       frame_base: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`forward` over a batch of `n_groups` independent samples in the launches of one forward (mmpl_dit_forward_groups).
        x: [n_groups * F, in_dim, lat_h, lat_w], sample-major; t, frame_ids, write_slots: per frame, likewise.  visible_slots: one list
        per sample, all of one length -- each sample attends to ITS slots of the one cache only, so give sample g slots of its own
        (`KVCache(engine, W, batch=G)`: g * W ..).  cross: one (cross_k, cross_v) per sample; when all are the same tensors the text
        cross-attention is one launch over all rows, else one per sample.  cross_rows: must hold for every sample's contents (the
        largest of their `CrossKV.rows`).  n_groups * F <= max_frames.  No share buffers, no attention history, no i2v."""
        nF = x.shape[0]
        assert n_groups >= 1 and nF % n_groups == 0, (n_groups, nF)
        assert x.is_contiguous() and x.dtype == torch.bfloat16 and x.shape[1:] == (self.in_dim, self.lat_h, self.lat_w)
        assert t.dtype == torch.float32 and t.numel() == nF and t.is_cuda
        assert len(visible_slots) == n_groups and len({len(v) for v in visible_slots}) == 1 and len(cross) == n_groups
        assert len(frame_ids) == nF and len(write_slots) == nF
        if frame_base is not None:
            assert frame_base.dtype == torch.int32 and frame_base.numel() == 1 and frame_base.device == x.device
        out = self._checked_out(x, None, None, None, out)
        ws = self.workspace(nF) if workspace is None else workspace
        n_slots = k_cache.shape[1] // self.S
        ia = lambda v: (C.c_int * max(len(v), 1))(*[int(i) for i in v])
        pa = lambda ts: (C.c_void_p * n_groups)(*[tt.data_ptr() for tt in ts])
        with torch.cuda.device(self.device):          # the stream handed to the library is this device's current stream
            _lib.check(self._lib.mmpl_dit_forward_groups(
                self._h, _lib.ptr(x), _lib.ptr(t), n_groups, nF // n_groups, ia(frame_ids), ia(write_slots),
                ia([s for v in visible_slots for s in v]), len(visible_slots[0]), _lib.ptr(k_cache), _lib.ptr(v_cache), n_slots,
                pa([c[0] for c in cross]), pa([c[1] for c in cross]), self.text_len if cross_rows is None else int(cross_rows),
                None, None, None, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.ptr(frame_base), _lib.stream_ptr()),
                "mmpl_dit_forward_groups")
        return out

    def _checked_out(self, x: torch.Tensor, share_out, share_in, attn_history, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Both forwards' checks of the optional tensors (share buffers, attention history) against x's frame count and device;
        returns `out`, allocated when None."""
        nF = x.shape[0]
        for sh in (share_out, share_in):
            assert sh is None or (sh.dtype == torch.bfloat16 and sh.is_contiguous() and sh.numel() >= nF * self.S * self.dim and sh.device == x.device)
        if attn_history is not None:
            need = self._lib.mmpl_dit_attn_history_bytes(self._h, nF)
            assert attn_history.dtype == torch.uint8 and attn_history.is_contiguous() and attn_history.numel() >= need and attn_history.device == x.device
        if out is None:
            out = torch.empty(nF, 16, self.lat_h, self.lat_w, dtype=torch.bfloat16, device=x.device)
        return out

    # ------------------------------------------------------------------ step caching
    def new_step_cache(self, n_frames: int) -> torch.Tensor:
        """[n_frames * S, dim] bf16 for `forward(..., cache_mode=, residual=)` / `forward_full`: what a CACHE_RECORD forward leaves and
        a CACHE_REUSE forward adds (mmpl_dit_step_cache_bytes).  One per (CFG branch, stage shape)."""
        n = self._lib.mmpl_dit_step_cache_bytes(self._h, n_frames)
        return torch.empty(n // 2, dtype=torch.bfloat16, device=self.device)

    def _check_residual(self, cache_mode: int, residual: Optional[torch.Tensor], nF: int, device) -> None:
        if cache_mode != CACHE_OFF and residual is not None:
            assert residual.dtype == torch.bfloat16 and residual.is_contiguous() and residual.device == device
            assert residual.numel() >= nF * self.S * self.dim, (residual.numel(), nF * self.S * self.dim)

    def time_embed(self, t: torch.Tensor, want_e0: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """t: [n] float32 on the device -> (e [n, dim], e0 [n, 6 * dim] or None) bf16: the timestep embedding and its projection as a
        forward at timestep t[i] computes them (mmpl_dit_time_embed: the same launches, row for row)."""
        assert t.dtype == torch.float32 and t.dim() == 1 and t.is_contiguous() and t.device == self.device
        n = t.numel()
        e = torch.empty(n, self.dim, dtype=torch.bfloat16, device=self.device)
        e0 = torch.empty(n, 6 * self.dim, dtype=torch.bfloat16, device=self.device) if want_e0 else None
        nbytes = self._lib.mmpl_dit_time_embed_workspace_bytes(self._h, n)
        if nbytes == 0:
            raise ValueError(f"DitEngine.time_embed: {n} timesteps is outside 1 .. 4096")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_dit_time_embed(self._h, _lib.ptr(t), n, _lib.ptr(e), _lib.ptr(e0), _lib.ptr(ws), ws.numel(),
                                                     _lib.stream_ptr()), "mmpl_dit_time_embed")
        return e, e0

    def rel_l1_rows(self, x: torch.Tensor) -> torch.Tensor:
        """x: [rows >= 2, d] bf16 (row stride x.stride(0)) -> float32 [rows - 1]: sum |x[i+1] - x[i]| / sum |x[i]| (mmpl_rel_l1_rows)."""
        assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= 2 and x.is_cuda
        out = torch.empty(x.shape[0] - 1, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(self._lib.mmpl_rel_l1_rows(_lib.ptr(x), x.stride(0), x.shape[0], x.shape[1], _lib.ptr(out), _lib.stream_ptr()),
                       "mmpl_rel_l1_rows")
        return out

    # ------------------------------------------------------------------ whole-clip (bidirectional) forward
    def full_workspace(self, n_frames: int, second: bool = False) -> torch.Tensor:
        """Scratch of `forward_full` at `n_frames` frames: one buffer per frame count, allocated on first use (outside any capture).
        `second`: a private one for a forward that runs CONCURRENTLY with another (the uncond branch of a CFG step on a second
        stream)."""
        key = (n_frames, bool(second))
        if key not in self._ws_full:
            nbytes = self._lib.mmpl_dit_full_workspace_bytes(self._h, n_frames)
            if nbytes == 0:
                raise ValueError(f"DitEngine.forward_full: n_frames = {n_frames} is outside 1 .. 24")
            self._ws_full[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws_full[key]

    def forward_full(self, x: torch.Tensor, t: torch.Tensor, cross_k: torch.Tensor, cross_v: torch.Tensor,
                     cross_rows: Optional[int] = None, out: Optional[torch.Tensor] = None, share_out: Optional[torch.Tensor] = None,
                     share_in: Optional[torch.Tensor] = None, attn_history: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, cache_mode: int = CACHE_OFF,
                     residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The non-causal forward over a whole clip (mmpl_dit_forward_full): x [nF, 16, lat_h, lat_w] bf16 with nF up to 24
        whatever `max_frames`; t: ONE float32 on the device, the clip's timestep.  Frame i is rotated at temporal position i, every
        frame attends to every frame, and there is no KV cache: the layer's K / V live in the workspace.  Returns the flow
        prediction [nF, 16, lat_h, lat_w].  `cross_rows`, `share_out`, `share_in`, `attn_history` as in `forward`; `workspace`: a
        private scratch (`full_workspace(nF, second=True)`) for a forward that runs concurrently with another one.
        `y`: the i2v model type's conditioning video, [nF, in_dim - 16, lat_h, lat_w] bf16, frame-major like x and read next to it
        (mmpl_dit_forward_full_i2v: x and y are never concatenated); required there -- with `set_image_kv` done --, None for t2v.
        `cache_mode` / `residual`: step caching as in `forward` (mmpl_dit_forward_full_cached)."""
        nF = x.shape[0]
        i2v = self.model_type == "i2v"
        if i2v and y is None:
            raise ValueError("DitEngine.forward_full: an i2v model needs y, the conditioning video [nF, in_dim - 16, lat_h, lat_w]")
        if not i2v and y is not None:
            raise ValueError("DitEngine.forward_full: y belongs to the i2v model type; this is a t2v model")
        if i2v and self._img_kv is None:
            raise RuntimeError("DitEngine: an i2v model needs set_image_kv(*precompute_image_context(clip_fea)) before forward_full")
        assert x.is_contiguous() and x.dtype == torch.bfloat16 and x.shape[1:] == (16, self.lat_h, self.lat_w)
        if i2v:
            assert y.is_contiguous() and y.dtype == torch.bfloat16 and y.shape == (nF, self.in_dim - 16, self.lat_h, self.lat_w) and y.device == x.device
        assert t.dtype == torch.float32 and t.numel() == 1 and t.device == x.device
        ws = self.full_workspace(nF) if workspace is None else workspace
        out = self._checked_out(x, share_out, share_in, attn_history, out)
        assert out.is_contiguous() and out.dtype == torch.bfloat16 and out.shape == (nF, 16, self.lat_h, self.lat_w)
        tail = (nF, _lib.ptr(cross_k), _lib.ptr(cross_v), self.text_len if cross_rows is None else int(cross_rows), _lib.ptr(share_out),
                _lib.ptr(share_in), _lib.ptr(attn_history), _lib.ptr(out), _lib.ptr(ws), ws.numel())
        self._check_residual(cache_mode, residual, nF, x.device)
        with torch.cuda.device(self.device):          # the stream handed to the library is this device's current stream
            if cache_mode != CACHE_OFF:
                _lib.check(self._lib.mmpl_dit_forward_full_cached(self._h, _lib.ptr(x), _lib.ptr(t), *tail, _lib.stream_ptr(), _lib.ptr(y),
                                                                  int(cache_mode), _lib.ptr(residual)), "mmpl_dit_forward_full_cached")
            elif i2v:
                _lib.check(self._lib.mmpl_dit_forward_full_i2v(self._h, _lib.ptr(x), _lib.ptr(y), _lib.ptr(t), *tail, _lib.stream_ptr()),
                           "mmpl_dit_forward_full_i2v")
            else:
                _lib.check(self._lib.mmpl_dit_forward_full(self._h, _lib.ptr(x), _lib.ptr(t), *tail, _lib.stream_ptr()),
                           "mmpl_dit_forward_full")
        return out

    # ------------------------------------------------------------------ hipGraph
    def capture(self, x: torch.Tensor, t: torch.Tensor, frame_ids, write_slots, visible_slots, k_cache, v_cache, cross_k, cross_v,
                out: torch.Tensor, pre=None, cross_rows: Optional[int] = None,
                attn_history: Optional[torch.Tensor] = None, cache_mode: int = CACHE_OFF,
                residual: Optional[torch.Tensor] = None) -> "torch.cuda.CUDAGraph":
        """Capture one forward (fixed stage shape, slot table and buffers) into a hipGraph.  The forward is a pure launch
        sequence -- no host sync, no allocation -- so replaying it costs one graph launch instead of ~13 launches per
        layer.  `x`, `t`, `out` and the caches are captured BY ADDRESS: update their contents in place between replays
        (that is what the denoise loop does: latents and the timestep change, the shapes never do).
        `pre`: launches recorded in front of the forward (the i2v model type refreshes the latent channels of its 36-channel
        input buffer there).
        The first capture of a stage shape on this engine runs the forward once eagerly, ahead of the capture (see below), on the
        caller's own buffers: it writes `out` and the caches' write slots, and it runs with the caller's `attn_history`, so it
        ADVANCES that history by one forward before any replay does.  A caller whose bits must not depend on whether the shape was
        warm zeroes the history after capture() (the pipeline does, at every stage boundary).
        `cache_mode` / `residual`: the captured forward's step-cache mode and buffer (`forward`)."""
        self.workspace(x.shape[0])                      # allocate outside the capture
        if x.shape[0] not in self._warm:                # one eager call per (engine, stage shape): the kernels a shape selects (pipelined
            # LayerNorm from 16 384 rows, the v8 GEMM variants, attn_cross_kernel<NT>, the split-KV tail) set their dynamic-LDS
            # attribute / query their occupancy on first launch -- outside the capture, not inside it
            if pre is not None:
                pre()
            self.forward(x, t, frame_ids, write_slots, visible_slots, k_cache, v_cache, cross_k, cross_v, out=out, cross_rows=cross_rows,
                         attn_history=attn_history, cache_mode=cache_mode, residual=residual)
            self._warm.add(x.shape[0])
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if pre is not None:
                pre()
            self.forward(x, t, frame_ids, write_slots, visible_slots, k_cache, v_cache, cross_k, cross_v, out=out, cross_rows=cross_rows,
                         attn_history=attn_history, cache_mode=cache_mode, residual=residual)
        return g

