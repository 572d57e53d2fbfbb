"""Host-side handles of the HIP TAEHV preview autoencoder (libmmpl_hip.so: mmpl_taehv_*), the engines behind ``TAEHVWrapper``.

The "Tiny AutoEncoder" of the reference's demo (demo_utils/taehv.py, checkpoint ``taew2_1.pth`` for Wan 2.1).  ``TaehvEngine`` is
the decoder half: 35 plain 2-D convolutions, causal in time with one frame of memory per MemBlock.  It takes the reference's
state dict as it is (``decoder.N...`` keys; encoder keys are ignored), repacks the conv weights once into the kernels'
fragment-major layout and keeps them on the GPU.  ``TaehvEncoderEngine`` (below) is the encoder half, built the same way.  Latents are the pipeline's normalised latents (no mean / std); the output is the network's, nominally
[0, 1], and UNTRIMMED like this reference's ``decode_video``: 4 frames per latent frame (``TAEHVWrapper`` drops the first 3).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _lib
from .vae import VaeEngine

# nn.Sequential indices of the decoder's TGrow layers -> rows the model keeps (channels * stride)
TGROW_ROWS = {"decoder.7.conv.weight": 256 * 1, "decoder.13.conv.weight": 128 * 2, "decoder.19.conv.weight": 64 * 2}


def patch_tgrow_layers(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A checkpoint trained with a larger temporal stride has more TGrow output rows than the model: the model keeps the LAST
    ``channels * stride`` of them (the last time steps), as the reference's loader does."""
    out = dict(sd)
    for key, rows in TGROW_ROWS.items():
        if key in out and out[key].shape[0] > rows:
            out[key] = out[key][-rows:]
    return out


class _TaehvHalf:
    """What the two engines share: the library handle behind the symbol prefix ``_SYM`` (<_SYM>_create / _destroy /
    _num_weights / _weight_name / _bind_weights / _reset / _workspace_bytes), the repacked weights and the lazy workspace."""
    _SYM = ""

    def __init__(self, lat_h: int, lat_w: int, device="cuda:0"):
        self.lat_h, self.lat_w = lat_h, lat_w
        self.device = torch.device(device)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._fn("create")(lat_h, lat_w, C.byref(h)), f"{self._SYM}_create")
        self._h = h
        self._weights: List[torch.Tensor] = []
        self._ws: Optional[torch.Tensor] = None

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._SYM}_{name}")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def weight_names(cls) -> List[str]:
        lib = _lib.load()
        name = getattr(lib, f"{cls._SYM}_weight_name")
        return [name(i).decode() for i in range(getattr(lib, f"{cls._SYM}_num_weights")())]

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        names = self.weight_names()
        missing = [n for n in names if n not in sd]
        if missing:
            raise KeyError(f"TAEHV state dict lacks {missing[:3]}{' ...' if len(missing) > 3 else ''}")
        ws = [self._repack(n, sd[n]).contiguous().to(self.device) for n in names]
        _lib.bind_weights(self._fn("bind_weights"), self._h, ws, f"{self._SYM}_bind_weights")
        self._weights = ws

    def clear_cache(self) -> None:
        """Ends the streamed video: the next streamed call starts from zero memories."""
        _lib.check(self._fn("reset")(self._h), f"{self._SYM}_reset")

    def _workspace(self) -> torch.Tensor:
        if self._ws is None:
            self._ws = torch.empty(self._fn("workspace_bytes")(self._h), dtype=torch.uint8, device=self.device)
        return self._ws


class TaehvEngine(_TaehvHalf):
    _SYM = "mmpl_taehv"

    def __init__(self, lat_h: int, lat_w: int, device="cuda:0"):
        super().__init__(lat_h, lat_w, device)
        self.latents_done = 0                                        # latent frames decoded since clear_cache()

    @staticmethod
    def _repack(name: str, t: torch.Tensor) -> torch.Tensor:
        t = t.to(torch.bfloat16)
        if name.endswith(".bias"):
            t = t.reshape(-1)
            return torch.cat([t, t.new_zeros(-t.numel() % 4)])
        cout, cin = t.shape[0], t.shape[1]
        t = t.permute(0, 2, 3, 1).reshape(cout, -1, cin)                 # [Cout, taps, Cin]
        cin_pad = (cin + 31) // 32 * 32
        if cin_pad != cin:
            t = torch.cat([t, t.new_zeros(cout, t.shape[1], cin_pad - cin)], dim=2)
        return VaeEngine._frag_pack(t.reshape(cout, -1), cin_pad)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        super().load_state_dict(patch_tgrow_layers(sd))

    def clear_cache(self) -> None:
        """Ends the streamed video: the next ``decode_stream`` call starts from zero memories."""
        super().clear_cache()
        self.latents_done = 0

    def decode_stream(self, latent: torch.Tensor, mean=None, std=None, out_format: str = "float") -> torch.Tensor:
        """latent [F, 16, h, w] = the NEXT F latent frames of the streamed video -> 4F frames on the current stream.
        "float": float32 [4F, 3, 8h, 8w], the network's output (nominally [0, 1], unclamped); "uint8": [4F, 8h, 8w, 3] =
        ``(x.clamp(0, 1) * 255)`` truncated.  ``mean`` / ``std`` are accepted for call compatibility with ``VaeEngine`` and
        ignored: this decoder reads the normalised latent."""
        if out_format not in ("float", "uint8"):
            raise ValueError(f"out_format {out_format!r}: 'float' or 'uint8'")
        z = latent.to(device=self.device, dtype=torch.bfloat16).contiguous()
        F = z.shape[0]
        assert F >= 1 and z.shape[1:] == (16, self.lat_h, self.lat_w)
        ws = self._workspace()
        H, W = 8 * self.lat_h, 8 * self.lat_w
        if out_format == "uint8":
            out = torch.empty(4 * F, H, W, 3, dtype=torch.uint8, device=self.device)
        else:
            out = torch.empty(4 * F, 3, H, W, dtype=torch.float32, device=self.device)
        n_out = C.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_taehv_decode(self._h, _lib.ptr(z), F, _lib.ptr(out), int(out_format == "uint8"), C.byref(n_out),
                                                   _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "mmpl_taehv_decode")
        self.latents_done += F
        return out[:n_out.value]

    def decode(self, latent: torch.Tensor, out_format: str = "float") -> torch.Tensor:
        """One-shot: a whole video [F, 16, h, w] from zero memories -> 4F frames (see ``decode_stream``)."""
        if out_format not in ("float", "uint8"):
            raise ValueError(f"out_format {out_format!r}: 'float' or 'uint8'")
        self.clear_cache()
        return self.decode_stream(latent, out_format=out_format)


class TaehvEncoderEngine(_TaehvHalf):
    """The ENCODER half (``TAEHV.encode_video``; libmmpl_hip.so: mmpl_taehv_enc_* / mmpl_taehv_encode): pixels in [0, 1] -> the
    pipeline's normalised latents, 4 pixel frames per latent frame, causal in time with one frame of memory per MemBlock.  Takes
    the reference's state dict as it is (``encoder.N...`` keys; decoder keys are ignored)."""
    _SYM = "mmpl_taehv_enc"

    def __init__(self, lat_h: int, lat_w: int, device="cuda:0"):
        super().__init__(lat_h, lat_w, device)
        self.frames_done = 0                                         # pixel frames encoded since clear_cache()

    @staticmethod
    def _repack(name: str, t: torch.Tensor) -> torch.Tensor:
        if name == "encoder.0.weight":
            # the input layer's packed K: [64, 3, 3, 3] -> [64, 32], column (3 ky + kx) * 3 + c, columns 27 .. 31 zero: one chunk
            t = t.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(t.shape[0], 27)
            return VaeEngine._frag_pack(torch.cat([t, t.new_zeros(t.shape[0], 5)], dim=1), 32)
        return TaehvEngine._repack(name, t)

    def clear_cache(self) -> None:
        """Ends the streamed video: the next ``encode_stream`` call starts from zero memories."""
        super().clear_cache()
        self.frames_done = 0

    def _check_px(self, px: torch.Tensor) -> bool:
        """-> whether ``px`` is the uint8 format; ValueError before the device is touched."""
        H, W = 8 * self.lat_h, 8 * self.lat_w
        u8 = px.dtype == torch.uint8
        want = (H, W, 3) if u8 else (3, H, W)
        if px.dim() != 4 or tuple(px.shape[1:]) != want or not (u8 or px.dtype.is_floating_point):
            raise ValueError(f"pixels {tuple(px.shape)} {px.dtype}: float [T, 3, {H}, {W}] in [0, 1] or uint8 [T, {H}, {W}, 3]")
        if px.shape[0] < 4 or px.shape[0] % 4:
            raise ValueError(f"{px.shape[0]} frames: the encoder takes a multiple of 4 (4 pixel frames per latent frame)")
        return u8

    def encode_stream(self, px: torch.Tensor) -> torch.Tensor:
        """px = the NEXT T frames of the streamed video, float [T, 3, 8h, 8w] in [0, 1] or uint8 [T, 8h, 8w, 3], T a multiple of 4
        -> bf16 [T / 4, 16, h, w], the pipeline's normalised latents, on the current stream."""
        u8 = self._check_px(px)
        px = px.to(device=self.device, dtype=torch.uint8 if u8 else torch.float32).contiguous()
        T = px.shape[0]
        ws = self._workspace()
        z = torch.empty(T // 4, 16, self.lat_h, self.lat_w, dtype=torch.bfloat16, device=self.device)
        n_out = C.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_taehv_encode(self._h, _lib.ptr(px), int(u8), T, _lib.ptr(z), C.byref(n_out), _lib.ptr(ws),
                                                   ws.numel(), _lib.stream_ptr()), "mmpl_taehv_encode")
        self.frames_done += T
        return z[:n_out.value]

    def encode(self, px: torch.Tensor) -> torch.Tensor:
        """One-shot: a whole video from zero memories (see ``encode_stream``)."""
        self._check_px(px)
        self.clear_cache()
        return self.encode_stream(px)
