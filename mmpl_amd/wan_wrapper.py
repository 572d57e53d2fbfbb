"""Model wrappers with the reference's names and call shapes (MMPL_t2v/utils/wan_wrapper.py), on the HIP engines.

  * ``WanFPSWrapper``   (:317-515)  generator: forward(noisy, conditional_dict, timestep, kv_cache, crossattn_cache,
                                    current_start, cache_start) -> (flow_pred, pred_x0)
  * ``WanVAEWrapper``   (:54-113)   decode_to_pixel / encode_to_latent
  * ``WanTextEncoder``  (:15-51)    tokenizer -> HIP umT5-xxl engine (mmpl_amd/t5.py) -> padding rows zeroed

``WanFPSWrapper`` also serves the Wan-I2V model type (``config.json`` model_type 'i2v', wan/modules/model.py:563-616):
``forward`` / ``capture`` take ``clip_fea`` and ``y`` (kwargs like ``WanModel.forward``, model.py:626-640, or entries of
``conditional_dict``), build the image K / V once per ``clip_fea`` and concatenate the stage's frames of ``y`` to the
latents on the channel axis (model.py:680-681).

KV caches keep the reference's shape of a list of per-layer dicts (``k``, ``v``, ``attention_vis_index`` ...,
pipeline/casual_fps_inference.py:453-501) so pipeline-style code runs unchanged, but the per-layer tensors are views
into ONE allocation per cache that the HIP forward addresses through its slot table.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch

from . import _lib
from .dit import DitEngine
from .geometry import Geometry
from .scheduler import FlowMatchScheduler
from .stage_plan import StagePlan, slot_of
from .synthetic import WAN_CONFIGS

local_wan_path = "../wan_models"


def _state_dict_or_disk(state_dict: Optional[dict], path: str) -> Optional[dict]:
    """`state_dict`, or, without one, the checkpoint at `path` (None where there is no such file)."""
    if state_dict is None and os.path.exists(path):
        from .checkpoints import read_state_dict
        state_dict = read_state_dict(path)
    return state_dict


def _unbatched(pe: torch.Tensor) -> torch.Tensor:
    """Rows of embeddings ([T, D]: prompt_embeds, clip_fea), or the reference's batch of one of them ([1, T, D]) -> [T, D]."""
    return pe[0] if pe.dim() == 3 else pe


def _source(t: torch.Tensor) -> tuple:
    """What to remember of a tensor something is built from: the object and its version counter."""
    return t, t._version


def _built_from(src: Optional[tuple], t: torch.Tensor) -> bool:
    """Is `src` (a `_source`, or None) this very tensor object, not written in place since?  What was built from it is then still its."""
    return src is not None and src[0] is t and src[1] == t._version


def _conditioning_video(y, engine: DitEngine, who: str) -> torch.Tensor:
    """The i2v model type's `y` as the reference passes it ([20, F, h, w], a list of one such, or [1, 20, F, h, w]) -> the validated
    [20, F, h, w]; ValueError (in the name of the wrapper `who`) for any other shape."""
    yy = y[0] if isinstance(y, (list, tuple)) or y.dim() == 5 else y
    e = engine
    if yy.dim() != 4 or yy.shape[0] != e.in_dim - 16 or tuple(yy.shape[2:]) != (e.lat_h, e.lat_w):
        raise ValueError(f"{who}: y is {tuple(yy.shape)}, expected [{e.in_dim - 16}, F, {e.lat_h}, {e.lat_w}]")
    return yy


class KVCache(list):
    """list of per-layer dicts like the reference's kv_cache; `k_all` / `v_all`: [L, batch*n_slots*S, dim].  ``batch`` samples
    share the one allocation, sample g owning frame slots ``g*n_slots .. g*n_slots + n_slots - 1`` (DitEngine.forward_groups); the
    per-layer views are the reference's [batch, n_slots*S, H, 128]."""

    def __init__(self, engine: DitEngine, n_slots: int = 15, batch: int = 1):
        super().__init__()
        self.engine = engine
        self.n_slots, self.batch = int(n_slots), int(batch)
        self.k_all, self.v_all = engine.new_kv_cache(self.batch * self.n_slots)
        self.vis: List[int] = []          # token offsets, shared by every layer (the reference keeps L identical copies)
        # what the self-attention's softmax passes did on this branch's previous forward (DitEngine.new_attn_history): travels with
        # the cache because it is per CFG branch; the pipeline zeroes it at every stage boundary.  None = stateless attention.
        self.attn_history: Optional[torch.Tensor] = None
        H = engine.cfg["num_heads"]
        for l in range(engine.L):
            self.append({"k": self.k_all[l].view(self.batch, -1, H, 128), "v": self.v_all[l].view(self.batch, -1, H, 128),
                         "global_end_index": torch.tensor([0], dtype=torch.long),
                         "local_end_index": torch.tensor([0], dtype=torch.long),
                         "attention_vis_index": self.vis})

    def reset(self):
        self.vis.clear()
        self.reset_attn_history()

    def enable_attn_history(self, on: bool = True):
        if on and self.attn_history is None:
            self.attn_history = self.engine.new_attn_history()
        elif not on:
            self.attn_history = None

    def reset_attn_history(self):
        if self.attn_history is not None:
            self.attn_history.zero_()


class CrossAttnCache(list):
    """list of per-layer dicts {"k","v","is_init"}; K/V for all layers are filled by one precompute call per sample.  ``batch``
    samples: `k_b` / `v_b` [batch, L, text_len, dim], `k_all` / `v_all` sample 0's; the per-layer views are [batch, text_len, H, 128]."""

    def __init__(self, engine: DitEngine, batch: int = 1):
        super().__init__()
        self.engine, self.batch = engine, int(batch)
        self.k_b = torch.zeros(self.batch, engine.L, engine.text_len, engine.dim, dtype=torch.bfloat16, device=engine.device)
        self.v_b = torch.zeros_like(self.k_b)
        self.k_all, self.v_all = self.k_b[0], self.v_b[0]
        self.rows = engine.text_len       # rows `rows .. text_len-1` of k_all / v_all repeat one row (CrossKV.rows of the contents)
        self.shared = self.batch == 1     # every sample reads sample 0's K / V (one prompt for all): `pairs`
        H = engine.cfg["num_heads"]
        for l in range(engine.L):
            self.append({"k": self.k_b[:, l].view(self.batch, -1, H, 128), "v": self.v_b[:, l].view(self.batch, -1, H, 128), "is_init": False})

    @property
    def is_init(self) -> bool:
        return all(b["is_init"] for b in self)

    def fill(self, prompt_embeds: torch.Tensor, shared: bool = False):
        """prompt_embeds: [T, D], or a text encoder's [batch, T, D].  ``shared``: the caller's statement that every sample's prompt is
        the same one -- sample 0's K / V are computed and serve all (the forward's text cross-attention is then one launch)."""
        pe = prompt_embeds.unsqueeze(0) if prompt_embeds.dim() == 2 else prompt_embeds
        if self.batch > 1 and pe.shape[0] != self.batch:
            raise ValueError(f"CrossAttnCache: {pe.shape[0]} prompts for a batch of {self.batch}")
        self.shared = bool(shared) or self.batch == 1
        rows = [self.engine.precompute_context(pe[g], out=(self.k_all, self.v_all) if g == 0 else (self.k_b[g], self.v_b[g])).rows
                for g in range(1 if self.shared else self.batch)]
        self.rows = max(rows)             # (the statement holds for every sample at the largest of their counts)
        for b in self:
            b["is_init"] = True

    def pairs(self):
        """(cross_k, cross_v) per sample, as DitEngine.forward_groups takes them."""
        return [(self.k_b[0 if self.shared else g], self.v_b[0 if self.shared else g]) for g in range(self.batch)]


class _HeldGraph:
    """A hipGraph together with the buffers it captured BY ADDRESS that nobody else owns (the i2v model type's 36-channel input:
    allocated outside the capture, so it would go back to the allocator -- and be overwritten -- once capture() returns)."""

    def __init__(self, graph, *keep):
        self.graph, self.keep = graph, keep

    def replay(self):
        self.graph.replay()


class _ModelHandle:
    """What the pipeline touches on `generator.model` (num_frame_per_block, parameters())."""

    def __init__(self, engine: DitEngine):
        self.engine = engine
        self.num_frame_per_block = 1

    def parameters(self):
        return iter(self.engine._weights)


class _GeneratorBase(torch.nn.Module):
    """What the two generator wrappers share: the model config (``model_config``, else the diffusers directory under
    ``local_wan_path``, else ``WAN_CONFIGS`` by name), the ``DitEngine`` with the directory's weights, the training-time
    ``FlowMatchScheduler`` and the nn.Module-compatible entry points the entry scripts use."""

    def __init__(self, model_name, timestep_shift, is_causal, model_config, geometry, device, max_frames: int = 7):
        super().__init__()
        self.geometry = geometry or Geometry.named("480p")
        from .checkpoints import read_diffusers_dir
        # <Model>.from_pretrained(...) (wan_wrapper.py:127-133, 328-330); local_wan_path is read now, not at import
        disk_cfg, disk_sd = read_diffusers_dir(f"{local_wan_path}/{model_name}/")
        cfg = disk_cfg if model_config is None else model_config
        if cfg is None:
            cfg = WAN_CONFIGS["14B" if "14B" in model_name else "1.3B"]
        self.engine = DitEngine(cfg, self.geometry.lat_h, self.geometry.lat_w, device, max_frames=max_frames)
        if disk_sd is not None:
            self.engine.load_state_dict(disk_sd)
        self.model_type = self.engine.model_type
        self._clip_src = None                 # i2v: the `_source` of the clip_fea the image K / V were built from
        self.uniform_timestep = not is_causal
        self.scheduler = FlowMatchScheduler(shift=timestep_shift, sigma_min=0.0, extra_one_step=True)
        self.scheduler.set_timesteps(1000, training=True)
        self.seq_len = self.geometry.frame_seqlen * self.geometry.frames_per_chunk      # the reference's 32760

    def load_state_dict(self, state_dict, strict: bool = True):
        """MMPL .pt checkpoints hold {'generator': {'model.<key>': tensor}} (Wan_fps_inference_1gpu.py:66-68)."""
        from .checkpoints import strip_generator_prefix
        self.engine.load_state_dict(strip_generator_prefix(state_dict))
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def to(self, *args, **kwargs):
        return self                       # weights already live on the GPU in bf16

    def get_scheduler(self) -> FlowMatchScheduler:
        return self.scheduler

    def new_crossattn_cache(self, batch: int = 1) -> CrossAttnCache:
        return CrossAttnCache(self.engine, batch)


class WanFPSWrapper(_GeneratorBase):
    def __init__(self, model_name="Wan2.1-T2V-14B", timestep_shift=8.0, is_causal=False, local_attn_size=-1, sink_size=0,
                 *, model_config: Optional[dict] = None, geometry: Optional[Geometry] = None, device="cuda:0"):
        assert is_causal, "only the causal FPS generator is on the hot path"
        super().__init__(model_name, timestep_shift, is_causal, model_config, geometry, device)
        self.model = _ModelHandle(self.engine)

    def new_kv_cache(self, n_slots: int = 15) -> KVCache:
        return KVCache(self.engine, n_slots)

    def _image_stream(self, frames, conditional_dict, clip_fea, y):
        """Wan-I2V model type: make sure the engine's image K/V belong to this `clip_fea` (MLPProj + per-block k_img / v_img,
        once per image) and return the stage's slice of the conditioning video, [nF, 20, h, w] bf16 (None for t2v)."""
        if self.model_type != "i2v":
            return None
        clip_fea = conditional_dict.get("clip_fea") if clip_fea is None else clip_fea
        y = conditional_dict.get("y") if y is None else y
        if clip_fea is None or y is None:
            raise ValueError("WanFPSWrapper: an i2v model needs clip_fea and y (model.py:672-673)")
        if not _built_from(self._clip_src, clip_fea):
            self.engine.set_image_kv(*self.engine.precompute_image_context(_unbatched(clip_fea)))
            self._clip_src = _source(clip_fea)
        yy = _conditioning_video(y, self.engine, "WanFPSWrapper")
        # (a stack of views: no host-built index tensor, so this also runs inside a hipGraph capture)
        return torch.stack([yy[:, f] for f in frames], dim=0).to(device=self.engine.device, dtype=torch.bfloat16)

    def _stage(self, x, conditional_dict, kv_cache, crossattn_cache, current_start, clip_fea, y):
        """What `forward` and `capture` do before the engine call: fill the cross-attention cache on first use (model.py:175-180),
        make the stage's frames visible (causal_fps_model.py:209,219 / 255), bring `x` ([nF, 16, h, w]) to contiguous bf16 and
        build the i2v model type's image stream.  -> (x, frames, visible slots, ys)"""
        S = self.engine.S
        if not crossattn_cache.is_init:
            crossattn_cache.fill(conditional_dict["prompt_embeds"])
        starts = [int(s) for s in current_start]
        frames = [s // S for s in starts]
        vis = kv_cache.vis
        if 15 * S not in starts:
            for s in starts:
                if s not in vis:
                    vis.append(s)
        if x.dtype != torch.bfloat16 or not x.is_contiguous():
            x = x.to(torch.bfloat16).contiguous()
        return x, frames, [slot_of(o // S) for o in vis], self._image_stream(frames, conditional_dict, clip_fea, y)

    def capture(self, noisy_image_or_video, conditional_dict, timestep, kv_cache, crossattn_cache, current_start, out,
                clip_fea=None, y=None, cache_mode: int = 0, residual: Optional[torch.Tensor] = None):
        """hipGraph of this exact forward (fixed buffers / stage shape); returns the graph, replay() re-runs it on the
        current contents of `noisy_image_or_video`, `timestep` and the caches.  `cache_mode` / `residual`: step caching
        (DitEngine.forward)."""
        assert noisy_image_or_video.is_contiguous() and noisy_image_or_video.dtype == torch.bfloat16
        assert timestep.dtype == torch.float32 and timestep.is_contiguous() and out.is_contiguous()
        x, frames, visible, ys = self._stage(noisy_image_or_video[0], conditional_dict, kv_cache, crossattn_cache, current_start,
                                             clip_fea, y)
        pre = None
        if ys is not None:                    # static 36-channel input; the graph refreshes its latent channels before the forward
            lat, x = x, torch.cat([x, ys], dim=1).contiguous()
            pre = lambda: x[:, :16].copy_(lat)
        g = self.engine.capture(x, timestep.view(-1), frames, StagePlan.write_slots(frames), visible, kv_cache.k_all, kv_cache.v_all,
                                crossattn_cache.k_all, crossattn_cache.v_all, out[0], pre=pre, cross_rows=crossattn_cache.rows,
                                attn_history=kv_cache.attn_history, cache_mode=cache_mode, residual=residual)
        return g if ys is None else _HeldGraph(g, x)

    def forward(self, noisy_image_or_video: torch.Tensor, conditional_dict: dict, timestep: torch.Tensor,
                kv_cache: Optional[KVCache] = None, crossattn_cache: Optional[CrossAttnCache] = None,
                current_start=None, classify_mode=False, concat_time_embeddings=False, clean_x=None, aug_t=None,
                cache_start=None, out: Optional[torch.Tensor] = None, return_x0: bool = False, clip_fea=None, y=None,
                workspace: Optional[torch.Tensor] = None, share_out: Optional[torch.Tensor] = None,
                share_in: Optional[torch.Tensor] = None, cache_mode: int = 0, residual: Optional[torch.Tensor] = None):
        assert kv_cache is not None and crossattn_cache is not None, "the FPS path always runs with caches"
        assert noisy_image_or_video.shape[0] == 1, "batch size 1 (as every reference entry point)"
        lat, frames, visible, ys = self._stage(noisy_image_or_video[0], conditional_dict, kv_cache, crossattn_cache, current_start,
                                               clip_fea, y)
        x = lat if ys is None else torch.cat([lat, ys], dim=1).contiguous()       # model.py:680-681
        t = timestep.reshape(-1).to(device=x.device, dtype=torch.float32)
        flow = self.engine.forward(x, t, frames, StagePlan.write_slots(frames), visible,
                                   kv_cache.k_all, kv_cache.v_all, crossattn_cache.k_all, crossattn_cache.v_all,
                                   out=None if out is None else out[0], cross_rows=crossattn_cache.rows, workspace=workspace,
                                   share_out=share_out, share_in=share_in, attn_history=kv_cache.attn_history,
                                   cache_mode=cache_mode, residual=residual)
        flow_pred = flow.unsqueeze(0)
        pred_x0 = None
        if return_x0:                                                     # wan_wrapper.py:373-397 (unused by the pipeline)
            sig = self.scheduler.sigmas.double().to(x.device)
            ts = self.scheduler.timesteps.double().to(x.device)
            tid = torch.argmin((ts.unsqueeze(0) - t.double().unsqueeze(1)).abs(), dim=1)
            pred_x0 = (lat.double() - sig[tid].reshape(-1, 1, 1, 1) * flow.double()).to(flow.dtype).unsqueeze(0)
        return flow_pred, pred_x0


class WanTextEncoder(torch.nn.Module):
    """utils/wan_wrapper.py:15-51 on the HIP umT5 engine (mmpl_amd/t5.py): tokenizer (seq_len 512, whitespace clean,
    tokenizers.py:38-82) -> encoder -> padding rows zeroed.  The engine computes in bf16 (the reference's generate.py
    T5 dtype, wan/configs/shared_config.py; its fps wrapper upcasts the same bf16 checkpoint to fp32 on the CPU -- the
    difference is the bf16 rounding the DiT's text_embedding applies to the context anyway; tests/test_t5_gpu.py).

    ``encode_fn(prompts) -> [B, 512, 4096]`` overrides everything (precomputed embeddings); otherwise pass
    ``state_dict`` or let it load ``models_t5_umt5-xxl-enc-bf16.pth`` from ``local_wan_path``."""

    def __init__(self, encode_fn=None, state_dict: Optional[dict] = None, pretrained_path: Optional[str] = None,
                 tokenizer=None, tokenizer_path: Optional[str] = None, cfg: Optional[dict] = None, text_len: int = 512,
                 device="cuda:0"):
        super().__init__()
        self.encode_fn = encode_fn
        self.text_len = text_len
        self.tokenizer = tokenizer
        self.tokenizer_path = tokenizer_path or f"{local_wan_path}/Wan2.1-T2V-14B/google/umt5-xxl/"
        self.model = None
        if encode_fn is not None:
            return
        state_dict = _state_dict_or_disk(state_dict, pretrained_path or f"{local_wan_path}/Wan2.1-T2V-14B/models_t5_umt5-xxl-enc-bf16.pth")
        if state_dict is not None:
            from .checkpoints import infer_t5_config
            from .t5 import T5Engine
            self.model = T5Engine(cfg or infer_t5_config(state_dict), text_len=text_len, device=device)
            self.model.load_state_dict(state_dict)

    def to(self, *args, **kwargs):
        return self

    @staticmethod
    def _clean(text: str) -> str:
        """clean='whitespace' (tokenizers.py:12-21); ftfy.fix_text is applied when ftfy is installed."""
        import html
        import re
        try:
            import ftfy
            text = ftfy.fix_text(text)
        except ImportError:
            pass
        text = html.unescape(html.unescape(text)).strip()
        return re.sub(r"\s+", " ", text).strip()

    def tokenize(self, text_prompts: List[str]):
        if self.tokenizer is None:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self.tokenizer_path)
        enc = self.tokenizer([self._clean(p) for p in text_prompts], return_tensors="pt", padding="max_length", truncation=True,
                             max_length=self.text_len, add_special_tokens=True)
        return enc.input_ids, enc.attention_mask

    def forward(self, text_prompts: List[str]) -> dict:
        if self.encode_fn is not None:
            return {"prompt_embeds": self.encode_fn(text_prompts)}
        if self.model is None:
            raise RuntimeError("WanTextEncoder: no umT5 weights (models_t5_umt5-xxl-enc-bf16.pth not found and no state_dict / "
                               "encode_fn given)")
        ids, mask = self.tokenize(text_prompts)
        return {"prompt_embeds": self.model.encode(ids, mask)}      # padding rows zeroed inside mmpl_t5_encode


class SyntheticTextEncoder(WanTextEncoder):
    """Deterministic stand-in used by tests / bench: a prompt hashes to a seed for N(0,1) embeddings, pad rows zeroed."""

    def __init__(self, text_dim=4096, device="cuda:0", n_valid=64):
        super().__init__(encode_fn=self._encode)
        self.text_dim, self.dev, self.n_valid = text_dim, device, n_valid

    def _encode(self, text_prompts: List[str]) -> torch.Tensor:
        import zlib
        from .synthetic import philox_normal
        outs = []
        for p in text_prompts:
            e = philox_normal([512, self.text_dim], zlib.crc32(p.encode("utf-8")))
            e[self.n_valid:] = 0
            outs.append(e)
        return torch.stack(outs).to(self.dev)


class WanVAEWrapper(torch.nn.Module):
    """utils/wan_wrapper.py:54-113 on the HIP Wan 3D-VAE engine (mmpl_amd/vae.py)."""

    mean = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508,
            0.4134, -0.0715, 0.5517, -0.3632, -0.1922, -0.9497, 0.2503, -0.2921]
    std = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743,
           3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253, 2.8251, 1.9160]

    def __init__(self, geometry: Optional[Geometry] = None, device="cuda:0", state_dict: Optional[dict] = None,
                 pretrained_path: Optional[str] = None):
        super().__init__()
        from .vae import VaeEngine
        self.geometry = geometry or Geometry.named("480p")
        self.model = VaeEngine(self.geometry.lat_h, self.geometry.lat_w, device)
        state_dict = _state_dict_or_disk(state_dict, pretrained_path or f"{local_wan_path}/Wan2.1-T2V-14B/Wan2.1_VAE.pth")
        if state_dict is not None:
            self.model.load_state_dict(state_dict)

    def to(self, *args, **kwargs):
        return self

    def encode_to_latent(self, pixel: torch.Tensor) -> torch.Tensor:
        """pixel [B, 3, T, H, W] in [-1, 1] -> latent [B, F, 16, h, w] float32 (normalised mu)."""
        self.model.clear_cache()                                     # WanVAE_.encode ends with clear_cache() (vae.py:542)
        return torch.stack([self.model.encode(u, self.mean, self.std).float() for u in pixel], dim=0)

    def decode_to_pixel(self, latent: torch.Tensor, use_cache: bool = False) -> torch.Tensor:
        """latent [B, F, 16, h, w] -> pixel [B, T, 3, 8h, 8w] float32 clamped to [-1, 1].

        ``use_cache=True`` (WanVAE_.cached_decode, batch 1): the latent frames CONTINUE the video of the earlier cached calls --
        every one of them yields 4 pixel frames unless it is the first since ``self.model.clear_cache()``.  ``use_cache=False``
        decodes a whole video and, as the reference's ``decode`` clears the cache before and after (vae.py:546, 568), ends a
        cached one."""
        if use_cache:
            assert latent.shape[0] == 1, "Batch size must be 1 when using cache"
            return self.model.decode_stream(latent[0], self.mean, self.std).float().clamp_(-1, 1).unsqueeze(0)
        self.model.clear_cache()
        return torch.stack([self.model.decode(u, self.mean, self.std).float().clamp_(-1, 1) for u in latent], dim=0)


class TAEHVWrapper(torch.nn.Module):
    """The tiny preview autoencoder (demo_utils/taehv.py, ``taew2_1.pth``) behind ``WanVAEWrapper``'s contract, on the HIP engines
    of mmpl_amd/taehv.py: ``decode_to_pixel`` (frames in [-1, 1]), ``model.clear_cache()``, ``model.decode_stream(...)`` and, when
    the weights hold the encoder half (``encoder.*`` keys), ``encode_to_latent`` / ``encode_stream`` on ``self.encoder``.  Without
    them ``self.encoder`` is None and the encode methods raise.

    The decoder engine, like this reference's ``decode_video``, returns 4 frames per latent frame; the wrapper drops the first 3
    frames of a VIDEO (where upstream put the trim), so frame counts equal the Wan VAE's -- ``1 + 4(F - 1)`` for a video's first
    call, ``4F`` after -- and the two decoders are interchangeable.  ``encode_to_latent`` mirrors that on the way in."""

    TRIM = 3

    def __init__(self, geometry: Optional[Geometry] = None, device="cuda:0", state_dict: Optional[dict] = None,
                 pretrained_path: Optional[str] = None):
        super().__init__()
        from .taehv import TaehvEncoderEngine, TaehvEngine
        self.geometry = geometry or Geometry.named("480p")
        self.model = TaehvEngine(self.geometry.lat_h, self.geometry.lat_w, device)
        self.encoder = None                                          # TaehvEncoderEngine once encoder weights are loaded
        self.mean, self.std = None, None                             # both halves work in the normalised latent space
        state_dict = _state_dict_or_disk(state_dict, pretrained_path or f"{local_wan_path}/taew2_1.pth")
        if state_dict is not None:
            self.model.load_state_dict(state_dict)
            if any(k.startswith("encoder.") for k in state_dict):
                self.encoder = TaehvEncoderEngine(self.geometry.lat_h, self.geometry.lat_w, device)
                self.encoder.load_state_dict(state_dict)

    def to(self, *args, **kwargs):
        return self

    def _need_encoder(self):
        if self.encoder is None:
            raise RuntimeError("TAEHVWrapper: no encoder weights (the state dict / checkpoint has no 'encoder.*' tensors); "
                               "only the decode methods are available")
        return self.encoder

    def encode_stream(self, px: torch.Tensor) -> torch.Tensor:
        """The encoder engine's ``encode_stream``: the NEXT T frames (float [T, 3, H, W] in [0, 1] or uint8 [T, H, W, 3], T a
        multiple of 4) of the streamed video -> bf16 [T / 4, 16, h, w]; ``self.encoder.clear_cache()`` starts a new video."""
        return self._need_encoder().encode_stream(px)

    @staticmethod
    def latent_frames(T: int) -> int:
        """Latent frames ``encode_to_latent`` returns for T pixel frames; ValueError for a count it does not take."""
        if T >= 4 and T % 4 == 0:
            return T // 4
        if T >= 1 and T % 4 == 1:
            return (T - 1) // 4 + 1
        raise ValueError(f"{T} frames: encode_to_latent takes 4k frames (k latents) or the Wan VAE's 1 + 4k (k + 1 latents)")

    def encode_to_latent(self, pixel: torch.Tensor) -> torch.Tensor:
        """pixel [1, 3, T, H, W] in [-1, 1] -> latent [1, F, 16, h, w] float32, a whole video from zero memories
        (``WanVAEWrapper.encode_to_latent``'s signature).  T = 4k gives k latents, the tiny encoder's own grid.  T = 1 + 4k, the
        Wan VAE's grid, gives k + 1 latents: the first frame is repeated three times in front -- the mirror of ``TRIM`` on the decode
        side.  That front padding is this wrapper's choice and has no counterpart in the reference, whose ``encode_video`` takes
        multiples of 4 only.  Any other T raises ValueError."""
        if pixel.dim() != 5 or pixel.shape[0] != 1 or pixel.shape[1] != 3:
            raise ValueError(f"pixel {tuple(pixel.shape)}: expected [1, 3, T, H, W]")
        T = pixel.shape[2]
        self.latent_frames(T)
        enc = self._need_encoder()
        px = (pixel[0].permute(1, 0, 2, 3).float() + 1) * 0.5                # [T, 3, H, W] in [0, 1]
        if T % 4 == 1:
            px = torch.cat([px[:1].expand(self.TRIM, -1, -1, -1), px], 0)
        z = enc.encode(px)
        enc.clear_cache()
        return z.float().unsqueeze(0)

    def decode_stream(self, latent: torch.Tensor, out_format: str = "float") -> torch.Tensor:
        """The engine's ``decode_stream`` ([F, 16, h, w] -> frames in the network's [0, 1] scale, "float" unclamped) minus the
        video's first 3 frames."""
        first = self.model.latents_done == 0                         # since ``model.clear_cache()``
        px = self.model.decode_stream(latent, out_format=out_format)
        return px[self.TRIM:] if first else px

    def decode_to_pixel(self, latent: torch.Tensor, use_cache: bool = False) -> torch.Tensor:
        """latent [1, F, 16, h, w] -> pixel [1, T, 3, 8h, 8w] float32 in [-1, 1] (``x * 2 - 1``, clamped).  ``use_cache=True``
        continues the video of the earlier cached calls; ``use_cache=False`` decodes a whole video and ends a cached one."""
        assert latent.shape[0] == 1, "Batch size must be 1"
        if not use_cache:
            self.model.clear_cache()
        px = self.decode_stream(latent[0])
        if not use_cache:
            self.model.clear_cache()
        return (px * 2 - 1).clamp_(-1, 1).unsqueeze(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# Few-step (Self-Forcing / CausVid) generator: CausalWanModel behind WanDiffusionWrapper (utils/wan_wrapper.py:116-300)
# ---------------------------------------------------------------------------------------------------------------------------------

def causal_slots(start_frame: int, n_frames: int, n_slots: int, window_frames: int, local_end: int = 0, global_end: int = 0):
    """KV slots of one CausalWanSelfAttention forward (wan/modules/causal_model.py:196-224), in frames of S tokens.

    The block's frames are written at ``local_end - n_frames .. local_end - 1`` with
    ``local_end = local_end_index + (start_frame + n_frames) - global_end_index`` (the cache's bookkeeping before the call), and
    the attention sees ``[max(0, local_end - window_frames), local_end)``.  Returns (write_slots, visible_slots, local_end).
    Where the reference would index past its cache (an IndexError / shape mismatch there) this raises ValueError."""
    if n_frames < 1 or start_frame < 0:
        raise ValueError(f"causal cache: bad block (start frame {start_frame}, {n_frames} frames)")
    le = local_end + start_frame + n_frames - global_end
    ls = le - n_frames
    if ls < 0 or le > n_slots:
        raise ValueError(f"causal cache overflow: frames {start_frame}..{start_frame + n_frames - 1} map to slots {ls}..{le - 1}, "
                         f"the cache holds {n_slots} frame slots (allocate it with new_kv_cache(n_slots) >= {le})")
    return list(range(ls, le)), list(range(max(0, le - window_frames), le)), le


ROPE_POSITIONS = 1024     # temporal positions the engine's RoPE tables hold (QkNormArgs cos_tab / sin_tab)


def rolling_slots(start_frame: int, n_frames: int, window_frames: int, sink_frames: int = 0):
    """KV slots of a block under the rolling window: the cache has ``window_frames`` slots, its first ``sink_frames`` are never
    overwritten once written, the rest is a ring.  Frame f < window lives in slot f (as ``causal_slots`` puts it); frame
    f >= window in slot ``sink + (f - sink) % (window - sink)``, i.e. over the oldest frame that is not a sink frame.  The block
    attends to slots ``0 .. min(end, window) - 1`` IN SLOT ORDER (contiguous pages for the attention launcher): the sink frames
    plus the most recent ``window - sink`` frames, its own included.  Returns (write_slots, visible_slots); the write slots of a
    block may wrap (window 8, sink 2: frames 6, 7, 8 -> slots 6, 7, 2).  RoPE stays on the absolute frame id, hence the table limit.

    ValueError: a sink outside ``0 <= sink < window``, a block of more than ``window - sink`` frames (it would overwrite its own
    frames), a block whose last frame id exceeds the RoPE tables' last position."""
    W, s = int(window_frames), int(sink_frames)
    if s < 0 or s >= W:
        raise ValueError(f"rolling KV window: sink_size {s} must satisfy 0 <= sink_size < window ({W} frames)")
    if n_frames < 1 or start_frame < 0:
        raise ValueError(f"rolling KV window: bad block (start frame {start_frame}, {n_frames} frames)")
    R = W - s
    if n_frames > R:
        raise ValueError(f"rolling KV window: a block of {n_frames} frames does not fit the {R} rolling slots "
                         f"(window {W} - sink_size {s})")
    end = start_frame + n_frames
    if end - 1 > ROPE_POSITIONS - 1:
        raise ValueError(f"rolling KV window: frame id {end - 1} is past the RoPE tables' last position ({ROPE_POSITIONS - 1})")
    write = [f if f < W else s + (f - s) % R for f in range(start_frame, end)]
    return write, list(range(min(end, W)))


class _CausalModelHandle(_ModelHandle):
    """`generator.model` of the causal wrapper: the reference's CausalWanModel attributes the pipeline reads or sets."""

    def __init__(self, engine: DitEngine, local_attn_size: int, sink_size: int):
        super().__init__(engine)
        self.local_attn_size = local_attn_size
        self.sink_size = sink_size


class WanDiffusionWrapper(_GeneratorBase):
    """utils/wan_wrapper.py:116-300 with ``is_causal=True`` (CausalWanModel, the Self-Forcing / CausVid generator) on the HIP DiT.

    For inference CausalWanModel differs from CausalFPSWanModel in two places only, both host-side here:
      * RoPE: contiguous frame ids ``current_start / S + i`` (causal_rope_apply, causal_model.py:27-57);
      * cache indexing: the block is written at its own frames and attends to the last ``window`` frames up to its end
        (causal_model.py:196-224; window = 21 frames when local_attn_size == -1, the reference's 32760 tokens at 480p).
    ``forward`` returns (flow_pred, pred_x0); pred_x0 is ``_convert_flow_pred_to_x0`` on the device (mmpl_fewstep_update).

    ``is_causal=False`` is the reference's other branch: WanModel, the base (bidirectional) Wan2.1-T2V weights.  ``model`` is then a
    plain handle, ``uniform_timestep`` is True and ``forward(noisy, conditional_dict, timestep)`` -- no caches -- is ONE whole-clip
    forward at ``timestep[:, 0]`` (DitEngine.forward_full: frame i at position i, every frame sees every frame, no KV cache);
    ``seq_len`` becomes the call's token count.  The pipelines' graphs use ``flow_full`` / ``fewstep_update``.

    ``is_causal=False`` also serves the Wan-I2V model type (``model_type`` 'i2v' in the config: the released Wan2.1-I2V-14B-480P /
    -720P weights, sampled over the whole clip as ``WanI2V.generate`` does): ``forward`` then takes ``clip_fea`` and ``y`` from
    ``conditional_dict`` (as ``WanFPSWrapper`` does), ``flow_full`` takes the frame-major ``y`` next to x, and ``set_image``
    rebuilds the per-layer image K / V IN PLACE -- one pair per wrapper, whose addresses a captured step graph holds."""

    def __init__(self, model_name="Wan2.1-T2V-14B", timestep_shift=8.0, is_causal=False, local_attn_size=-1, sink_size=0,
                 *, model_config: Optional[dict] = None, geometry: Optional[Geometry] = None, device="cuda:0", max_frames: int = 7):
        super().__init__(model_name, timestep_shift, is_causal, model_config, geometry, device, max_frames)
        self.is_causal = bool(is_causal)
        if self.model_type != "t2v" and self.is_causal:
            raise ValueError("WanDiffusionWrapper: the few-step causal generator is a t2v model (the i2v model type is bidirectional: "
                             "is_causal=False)")
        self.local_attn_size = int(local_attn_size)
        # is_causal=False: WanModel, the whole clip in one forward (DitEngine.forward_full); nothing of the causal cache applies
        self.model = _CausalModelHandle(self.engine, self.local_attn_size, sink_size) if self.is_causal else _ModelHandle(self.engine)
        self._ctx: List[tuple] = []               # is_causal=False: (`_source` of prompt_embeds, CrossKV) of the last two prompts
        self._img_kv = None                   # i2v: the wrapper's one (img_k, img_v) pair, refreshed in place by set_image
        self._sig64 = self.scheduler.sigmas.double()
        self._ts64 = self.scheduler.timesteps.double()

    @property
    def window_frames(self) -> int:
        """max_attention_size in frames: 32760 tokens = 21 frames (local_attn_size == -1) or local_attn_size (causal_model.py:76)."""
        return self.geometry.frames_per_chunk if self.local_attn_size == -1 else self.local_attn_size

    def new_kv_cache(self, n_slots: Optional[int] = None, batch: int = 1) -> KVCache:
        """The reference's kv_cache1 (causal_inference.py:278-297): local_attn_size frames, or 32760 tokens = 21 frames, per sample."""
        return KVCache(self.engine, self.window_frames if n_slots is None else n_slots, batch)

    # -- host scalars of the reference's timestep -> sigma lookups ------------------------------------------------------------
    def sigma_x0(self, timestep) -> float:
        """sigma_t of _convert_flow_pred_to_x0 (wan_wrapper.py:190-197): argmin over the fp64 timesteps, fp64 sigma."""
        t = torch.as_tensor(timestep).reshape(1).double()
        return float(self._sig64[torch.argmin((self._ts64.unsqueeze(0) - t.unsqueeze(1)).abs(), dim=1)].item())

    def sigma_add_noise(self, timestep) -> float:
        """sigma of FlowMatchScheduler.add_noise (scheduler.py:170-175) for a timestep tensor of the caller's dtype."""
        s = self.scheduler
        t = torch.as_tensor(timestep).reshape(1)
        return float(s.sigmas[torch.argmin((s.timesteps.unsqueeze(0) - t.unsqueeze(1)).abs(), dim=1)].item())

    # -- device pieces (capturable) ------------------------------------------------------------------------------------------
    def slots(self, kv_cache: KVCache, start_frame: int, n_frames: int, rolling: bool = False, batch: int = 1):
        """(write_slots, visible_slots, local_end) of a forward at `start_frame` against `kv_cache`'s current bookkeeping.
        ``rolling``: the rolling window with ``model.sink_size`` sink frames (``rolling_slots``) over a cache of exactly
        ``window_frames`` slots; local_end is then ``min(start + n, window)``, what ``set_cache_ends`` records.
        ``batch`` > 1 (a ``KVCache(..., batch=G)``; every sample is at the same frame): sample g's slots are sample 0's plus
        ``g * kv_cache.n_slots`` -- write_slots sample-major for all ``G * n_frames`` frames, visible_slots one list per sample."""
        G = getattr(kv_cache, "batch", 1)
        if batch != G:
            raise ValueError(f"slots: batch {batch} against a KV cache for {G} samples")
        n_slots = kv_cache.k_all.shape[1] // self.engine.S // G          # frame slots of ONE sample
        if rolling:
            if n_slots != self.window_frames:
                raise ValueError(f"rolling KV window: the cache holds {n_slots} frame slots, the window is {self.window_frames}")
            write, vis = rolling_slots(start_frame, n_frames, self.window_frames, int(self.model.sink_size))
            le = min(start_frame + n_frames, self.window_frames)
        else:
            write, vis, le = causal_slots(start_frame, n_frames, n_slots, self.window_frames, int(kv_cache[0]["local_end_index"][0]),
                                          int(kv_cache[0]["global_end_index"][0]))
        if batch == 1:
            return write, vis, le
        return [w + g * n_slots for g in range(batch) for w in write], [[v + g * n_slots for v in vis] for g in range(batch)], le

    @staticmethod
    def set_cache_ends(kv_cache: KVCache, global_end_frame: int, local_end_frame: int) -> None:
        """global_end_index / local_end_index after a forward (causal_model.py:225-226), in tokens, on every layer's dict."""
        S = kv_cache.engine.S
        for blk in kv_cache:
            blk["global_end_index"].fill_(global_end_frame * S)
            blk["local_end_index"].fill_(local_end_frame * S)

    def flow(self, x: torch.Tensor, t: torch.Tensor, start_frame: int, write_slots, visible_slots, kv_cache: KVCache,
             crossattn_cache: CrossAttnCache, out: Optional[torch.Tensor] = None,
             frame_base: Optional[torch.Tensor] = None, cache_mode: int = 0, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One CausalWanModel._forward_inference on explicit slots: x [F, 16, h, w] bf16, t [F] float32 on the device.  Stateless
        attention; the text cross-attention runs over all text_len rows (no prompt-dependent host value enters the launch).
        ``frame_base`` (int32 device scalar): `start_frame` is then relative to its value at execution time (DitEngine.forward).
        A ``KVCache(..., batch=G)``: x [G*F, 16, h, w] and t [G*F] sample-major, slots as ``slots(..., batch=G)`` gives them, every
        sample at `start_frame` (DitEngine.forward_groups).  `cache_mode` / `residual`: step caching (DitEngine.forward); a batched
        cache has no cached form."""
        G = getattr(kv_cache, "batch", 1)
        if G > 1:
            if cache_mode:
                raise ValueError("WanDiffusionWrapper.flow: step caching is not available to a batched (grouped) forward")
            frames = [start_frame + i for _ in range(G) for i in range(x.shape[0] // G)]
            return self.engine.forward_groups(x, t, G, frames, write_slots, visible_slots, kv_cache.k_all, kv_cache.v_all,
                                              crossattn_cache.pairs(), out=out, frame_base=frame_base)
        frames = [start_frame + i for i in range(x.shape[0])]
        return self.engine.forward(x, t, frames, write_slots, visible_slots, kv_cache.k_all, kv_cache.v_all, crossattn_cache.k_all,
                                   crossattn_cache.v_all, out=out, frame_base=frame_base, cache_mode=cache_mode, residual=residual)

    @staticmethod
    def fewstep_update(flow: torch.Tensor, x: torch.Tensor, noise: Optional[torch.Tensor], x0_out: torch.Tensor, sigma_t: float,
                       sigma_next: float = 0.0) -> None:
        """x0_out = _convert_flow_pred_to_x0(flow, x); if noise is given, x = add_noise(x0_out, noise, sigma_next) (mmpl_fewstep_update)."""
        n = x.numel()
        for t in (flow, x, x0_out) + ((noise,) if noise is not None else ()):
            assert t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == n and t.is_cuda, (t.dtype, tuple(t.shape))
        _lib.check(_lib.load().mmpl_fewstep_update(_lib.ptr(flow), _lib.ptr(x), _lib.ptr(noise), _lib.ptr(x0_out), n,
                                                   float(sigma_t), float(sigma_next), _lib.stream_ptr()), "mmpl_fewstep_update")

    # -- is_causal=False: WanModel.forward over the whole clip (wan/modules/model.py, utils/wan_wrapper.py:277-281) ------------------
    def flow_full(self, x: torch.Tensor, t: torch.Tensor, crossattn_cache: CrossAttnCache, out: Optional[torch.Tensor] = None,
                  share_out: Optional[torch.Tensor] = None, share_in: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, cache_mode: int = 0,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One whole-clip forward: x [F, 16, h, w] bf16, t ONE float32 on the device (uniform_timestep).  Stateless attention; the
        text cross-attention runs over all text_len rows (no prompt-dependent host value enters the launch: a captured graph
        serves every later prompt).  share_out / share_in / workspace as in DitEngine.forward_full.  i2v model type: `y`
        [F, 20, h, w] bf16 (frame-major) is required and `set_image` must have run; the image K / V it fills keep their address, so
        a captured graph serves every later image too.  `cache_mode` / `residual`: step caching (DitEngine.forward_full)."""
        return self.engine.forward_full(x, t, crossattn_cache.k_all, crossattn_cache.v_all, out=out, share_out=share_out,
                                        share_in=share_in, workspace=workspace, y=y, cache_mode=cache_mode, residual=residual)

    def set_image(self, clip_fea: torch.Tensor) -> None:
        """i2v model type: (re)build the per-layer image K / V of `clip_fea` ([257, 1280] or [1, 257, 1280]) into the wrapper's one
        static pair -- allocated and attached to the engine on first use, written in place afterwards -- unless they were built from
        this very tensor and it was not written since."""
        if self.model_type != "i2v":
            raise ValueError("WanDiffusionWrapper.set_image: the generator is a t2v model")
        if _built_from(self._clip_src, clip_fea):
            return
        fea = _unbatched(clip_fea)
        if self._img_kv is not None and self._img_kv[0].shape[1] != fea.shape[0]:
            raise ValueError(f"WanDiffusionWrapper.set_image: {fea.shape[0]} image tokens, the attached K / V hold {self._img_kv[0].shape[1]}")
        first = self._img_kv is None
        self._img_kv = self.engine.precompute_image_context(fea, out=self._img_kv)
        if first:
            self.engine.set_image_kv(*self._img_kv)
        self._clip_src = _source(clip_fea)

    def frame_major_y(self, y) -> torch.Tensor:
        """The conditioning video as the reference passes it ([20, F, h, w], a list of one such, or [1, 20, F, h, w]) -> [F, 20, h, w]
        bf16 on the engine's device, the layout `flow_full` reads."""
        yy = _conditioning_video(y, self.engine, "WanDiffusionWrapper")
        return yy.to(device=self.engine.device, dtype=torch.bfloat16).permute(1, 0, 2, 3).contiguous()

    def _context_kv(self, prompt_embeds: torch.Tensor):
        """Per-layer text K / V of `prompt_embeds`, kept for the last two prompts (the cond and the uncond one of a CFG loop) as
        long as the tensor is the same object and was not written since."""
        for src, kv in self._ctx:
            if _built_from(src, prompt_embeds):
                return kv
        kv = self.engine.precompute_context(_unbatched(prompt_embeds))
        self._ctx = self._ctx[-1:] + [(_source(prompt_embeds), kv)]
        return kv

    def _forward_full(self, noisy_image_or_video: torch.Tensor, conditional_dict: dict, timestep: torch.Tensor):
        assert noisy_image_or_video.shape[0] == 1, "batch size 1 (as every reference entry point)"
        clip_fea = y = None
        if self.model_type == "i2v":                                        # model.py:672-673: clip_fea and y are required
            clip_fea, y = conditional_dict.get("clip_fea"), conditional_dict.get("y")
            if clip_fea is None or y is None:
                raise ValueError("WanDiffusionWrapper: an i2v model needs clip_fea and y in conditional_dict (model.py:672-673)")
        x = noisy_image_or_video[0].to(device=self.engine.device, dtype=torch.bfloat16).contiguous()
        nF = x.shape[0]
        self.seq_len = nF * self.engine.S                                  # the call's token count: nothing is padded
        ts = timestep.reshape(noisy_image_or_video.shape[0], -1)[:, 0]      # input_timestep = timestep[:, 0] (:236-237)
        ys = None
        if self.model_type == "i2v":
            ys = self.frame_major_y(y)
            if ys.shape[0] != nF:
                raise ValueError(f"WanDiffusionWrapper: y holds {ys.shape[0]} frames, the latents {nF}")
            self.set_image(clip_fea)
        kv = self._context_kv(conditional_dict["prompt_embeds"])
        flow = self.engine.forward_full(x, ts.to(device=x.device, dtype=torch.float32), kv[0], kv[1], cross_rows=kv.rows, y=ys)
        x0 = torch.empty_like(x)
        self.fewstep_update(flow, x, None, x0, self.sigma_x0(ts.cpu()[0]))
        return flow.unsqueeze(0), x0.unsqueeze(0)

    # -- the reference's call shape ------------------------------------------------------------------------------------------
    def forward(self, noisy_image_or_video: torch.Tensor, conditional_dict: dict, timestep: torch.Tensor,
                kv_cache: Optional[KVCache] = None, crossattn_cache: Optional[CrossAttnCache] = None,
                current_start: Optional[int] = None, classify_mode: Optional[bool] = False,
                concat_time_embeddings: Optional[bool] = False, clean_x=None, aug_t=None, cache_start: Optional[int] = None):
        """noisy_image_or_video [1, F, 16, h, w]; timestep [1, F]; current_start in tokens.  -> (flow_pred, pred_x0), both
        [1, F, 16, h, w] bf16.  Reads the timestep on the host (one sync when it lives on the device): the pipeline's graphs use
        `flow` / `fewstep_update` with host scalars instead.  is_causal=False: no caches (a kv_cache is a ValueError), the whole
        clip at timestep[:, 0]; is_causal=True: the caches are required."""
        if self.is_causal and (kv_cache is None or crossattn_cache is None):
            raise ValueError("WanDiffusionWrapper: only the KV-cached inference forward is implemented (kv_cache / crossattn_cache)")
        if classify_mode or clean_x is not None:
            raise ValueError("WanDiffusionWrapper: training-only forward modes (classify_mode / clean_x) are not implemented")
        if not self.is_causal:
            if kv_cache is not None or crossattn_cache is not None:
                raise ValueError("WanDiffusionWrapper(is_causal=False): the bidirectional forward runs the whole clip and takes no "
                                 "kv_cache / crossattn_cache")
            return self._forward_full(noisy_image_or_video, conditional_dict, timestep)
        assert noisy_image_or_video.shape[0] == 1, "batch size 1 (as every reference entry point)"
        S = self.engine.S
        cs = int(current_start or 0)
        if cs % S:
            raise ValueError(f"current_start {cs} is not a multiple of the frame length {S}")
        if not crossattn_cache.is_init:                                   # model.py:175-180
            crossattn_cache.fill(conditional_dict["prompt_embeds"])
        x = noisy_image_or_video[0].to(torch.bfloat16).contiguous()
        nF = x.shape[0]
        ts = timestep.reshape(-1)
        assert ts.numel() == nF, (tuple(timestep.shape), nF)
        write, vis, le = self.slots(kv_cache, cs // S, nF)
        flow = self.flow(x, ts.to(device=x.device, dtype=torch.float32), cs // S, write, vis, kv_cache, crossattn_cache)
        self.set_cache_ends(kv_cache, cs // S + nF, le)
        x0 = torch.empty_like(x)
        sig = [self.sigma_x0(t) for t in ts.cpu()]                       # per-frame sigma (uniform_timestep = False)
        if all(s == sig[0] for s in sig):
            self.fewstep_update(flow, x, None, x0, sig[0])
        else:
            for i in range(nF):
                self.fewstep_update(flow[i], x[i], None, x0[i], sig[i])
        return flow.unsqueeze(0), x0.unsqueeze(0)
