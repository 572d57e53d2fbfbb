"""Host-side handle of the HIP Wan 3D-VAE (libmmpl_hip.so: mmpl_vae_*), the engine behind ``WanVAEWrapper``.

Takes the reference's ``Wan2.1_VAE.pth`` state_dict as is (MMPL_t2v/wan/modules/vae.py:612-636), repacks the conv
weights once into the implicit-GEMM operand layout ([Cout, taps * Cin], Cin contiguous) and keeps them on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib


class VaeEngine:
    def __init__(self, lat_h: int, lat_w: int, device="cuda:0"):
        self.lat_h, self.lat_w = lat_h, lat_w
        self.device = torch.device(device)
        self._lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_vae_create(lat_h, lat_w, C.byref(h)), "mmpl_vae_create")
        self._h = h
        self._weights: List[torch.Tensor] = []
        self._ws: Dict[int, torch.Tensor] = {}
        # the streamed video (decode_stream): its own handle and its own workspace, which decode / encode never touch
        self._stream = None
        self._stream_ws: Optional[torch.Tensor] = None

    def __del__(self):
        try:
            if getattr(self, "_stream", None):
                self._lib.mmpl_vae_stream_destroy(self._stream)
                self._stream = None
            if getattr(self, "_h", None):
                self._lib.mmpl_vae_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def clear_cache(self):
        """WanVAE_.clear_cache (vae.py:602-609): ends the streamed video, the next ``decode_stream`` call decodes a first frame.
        The one-shot ``decode`` / ``encode`` start from a cleared cache of their own on every call and do not need it."""
        if self._stream is not None:
            _lib.check(self._lib.mmpl_vae_stream_reset(self._stream), "mmpl_vae_stream_reset")

    def decode_stream(self, latent: torch.Tensor, mean, std, out_format: str = "float") -> torch.Tensor:
        """WanVAE_.cached_decode (vae.py:571-593): latent [F, 16, h, w] = the NEXT F latent frames of the streamed video ->
        1 + 4(F-1) pixel frames if they are the video's first (after ``clear_cache()``), else 4F, on the current stream.
        out_format "float": float32 [T, 3, 8h, 8w] in [-1, 1], bit-identical to the same frames of a one-shot ``decode``;
        "uint8": [T, 8h, 8w, 3], the video writer's layout."""
        if out_format not in ("float", "uint8"):
            raise ValueError(f"out_format {out_format!r}: 'float' or 'uint8'")
        z = latent.to(device=self.device, dtype=torch.bfloat16).contiguous()
        F = z.shape[0]
        assert F >= 1 and z.shape[1:] == (16, self.lat_h, self.lat_w)
        if self._stream is None:
            h = C.c_void_p()
            _lib.check(self._lib.mmpl_vae_stream_create(self._h, C.byref(h)), "mmpl_vae_stream_create")
            self._stream = h
        if self._stream_ws is None:
            self._stream_ws = torch.empty(self._lib.mmpl_vae_workspace_bytes(self._h, 0), dtype=torch.uint8, device=self.device)
        ws = self._stream_ws
        H, W = 8 * self.lat_h, 8 * self.lat_w
        # room for the most this call can produce; the library reports what it wrote (a video's first latent yields 1 frame, not 4)
        if out_format == "uint8":
            out = torch.empty(4 * F, H, W, 3, dtype=torch.uint8, device=self.device)
        else:
            out = torch.empty(4 * F, 3, H, W, dtype=torch.float32, device=self.device)
        m, inv = self._scales(mean, std)
        n_out = C.c_int(0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_vae_stream_decode(self._stream, _lib.ptr(z), F, m, inv, _lib.ptr(out), int(out_format == "uint8"),
                                                        C.byref(n_out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "mmpl_vae_stream_decode")
        return out[:n_out.value]

    @staticmethod
    def _repack(name: str, t: torch.Tensor) -> torch.Tensor:
        t = t.to(torch.bfloat16)
        if name.endswith(".gamma"):
            return t.reshape(-1)
        if name.endswith(".bias"):
            if name == "decoder.head.2.bias":
                t = torch.cat([t, t.new_zeros(1)])
            return t.reshape(-1)
        if name in ("conv1.weight", "conv2.weight"):
            return t.reshape(t.shape[0], t.shape[1])
        if t.dim() == 5:
            t = t.permute(0, 2, 3, 4, 1)
        elif t.dim() == 4:
            t = t.permute(0, 2, 3, 1)
        cout, cin = t.shape[0], t.shape[-1]
        t = t.reshape(cout, -1, cin)
        if cin % 32:
            pad = 32 - cin % 32
            t = torch.cat([t, t.new_zeros(cout, t.shape[1], pad)], dim=2)
        t = t.reshape(cout, -1)
        if name == "decoder.head.2.weight":
            t = torch.cat([t, t.new_zeros(1, t.shape[1])])
        return t

    @staticmethod
    def _frag_pack(w2d: torch.Tensor, cin_pad: int) -> torch.Tensor:
        """[N, ntaps * Cin] (tap-major, Cin a multiple of 32) -> the fragment-major packing conv_halo_kernel loads: for every
        (32-channel chunk, tap, 16-row group) the 64 lanes' 16 bytes back to back, lane = 16 * (8-channel k chunk) + row."""
        n, k = w2d.shape
        ntaps, nchunk = k // cin_pad, cin_pad // 32
        npad = (n + 15) // 16 * 16
        if npad != n:
            w2d = torch.cat([w2d, w2d.new_zeros(npad - n, k)])
        return w2d.view(npad // 16, 16, ntaps, nchunk, 4, 8).permute(3, 2, 0, 4, 1, 5).contiguous().view(-1)

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        n = self._lib.mmpl_vae_num_weights()
        ws = []
        for i in range(n):
            name = self._lib.mmpl_vae_weight_name(i).decode()
            if name.endswith(".weight.frag"):
                base = name[:-len(".frag")]
                w2d = self._repack(base, sd[base])
                cin = sd[base].shape[1]
                ws.append(self._frag_pack(w2d, (cin + 31) // 32 * 32).to(self.device))
                continue
            ws.append(self._repack(name, sd[name]).contiguous().to(self.device))
        _lib.bind_weights(self._lib.mmpl_vae_bind_weights, self._h, ws, "mmpl_vae_bind_weights")
        self._weights = ws

    def _workspace(self, mode: int) -> torch.Tensor:
        if mode not in self._ws:
            nbytes = self._lib.mmpl_vae_workspace_bytes(self._h, mode)
            other = self._ws.get(1 - mode)
            if other is not None and other.numel() >= nbytes:
                self._ws[mode] = other
            else:
                self._ws[mode] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws[mode]

    @staticmethod
    def _scales(mean: Sequence[float], std: Sequence[float]):
        m = torch.tensor(mean, dtype=torch.float32).to(torch.bfloat16)
        inv = 1.0 / torch.tensor(std, dtype=torch.float32).to(torch.bfloat16)          # bf16 arithmetic like the wrapper
        return (C.c_float * 16)(*m.float().tolist()), (C.c_float * 16)(*inv.float().tolist())

    def decode(self, latent: torch.Tensor, mean, std) -> torch.Tensor:
        """latent [F, 16, h, w] -> float32 [1 + 4(F-1), 3, 8h, 8w] in [-1, 1]."""
        z = latent.to(device=self.device, dtype=torch.bfloat16).contiguous()
        F = z.shape[0]
        assert z.shape[1:] == (16, self.lat_h, self.lat_w)
        out = torch.empty(1 + 4 * (F - 1), 3, 8 * self.lat_h, 8 * self.lat_w, dtype=torch.float32, device=self.device)
        ws = self._workspace(0)
        m, inv = self._scales(mean, std)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_vae_decode(self._h, _lib.ptr(z), F, m, inv, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "mmpl_vae_decode")
        return out

    def encode(self, pixel: torch.Tensor, mean, std) -> torch.Tensor:
        """pixel [3, T = 1 + 4k, 8h, 8w] in [-1, 1] -> float32 [1 + k, 16, h, w] (normalised mu)."""
        x = pixel.to(device=self.device, dtype=torch.bfloat16).contiguous()
        T = x.shape[1]
        assert x.shape[0] == 3 and x.shape[2:] == (8 * self.lat_h, 8 * self.lat_w) and (T - 1) % 4 == 0
        out = torch.empty(1 + (T - 1) // 4, 16, self.lat_h, self.lat_w, dtype=torch.float32, device=self.device)
        ws = self._workspace(1)
        m, inv = self._scales(mean, std)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.mmpl_vae_encode(self._h, _lib.ptr(x), T, m, inv, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "mmpl_vae_encode")
        return out
