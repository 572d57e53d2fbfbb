"""The Wan 3D causal VAE (mmpl_vae_decode, mmpl_vae_encode, mmpl_vae_stream_decode) as ORDERED LISTS OF LAUNCHES, written from the model
-- the reference's wan/modules/vae.py: CausalConv3d :17-36, RMS_norm :39-54, Resample :66-160, ResidualBlock :186-220,
AttentionBlock :223-262, Encoder3d :265-366, Decoder3d :369-472, WanVAE_.encode / decode :517-569, restated in oracle/vae_ref.py -- on
the launch contracts of include/mmpl_hip.h, not from csrc/vae.hip.

`VaeChain(sd, lat_h, lat_w, ops)` takes the REFERENCE state dict (the keys of mmpl_amd.synthetic.vae_state_dict) and packs it itself
(pack_conv, pack_frag below, written from the header's description of the operands: channels-last weights with Cin padded to 32, the
fragment-major packing of conv_halo_kernel, the decoder head padded 3 -> 4, conv2 folded into z_prep and conv1 into mu_out); it never
calls VaeEngine._repack / _frag_pack, which are under test.

The temporal cache.  The model keeps, per CausalConv3d, "the last two input frames" (vae.py:207-216), zeros before the video starts.
The chain keeps exactly that: two padded frames per conv, EACH IN A BUFFER OF ITS OWN, and hands the halo kernel the list
[cached frame, cached frame, new frames ...]; a conv on the plain kernel (which addresses frames linearly) gets those frames copied
into a fresh volume.  There is no ring, no slot arithmetic and no shift here: where vae.hip's ring base or slot copy goes wrong, the
two disagree.

Every launch goes through a small `ops` backend:

  VaeHipOps  each op is exactly ONE call of the matching single-launch C entry (mmpl_vae_conv, mmpl_vae_norm, mmpl_vae_upsample,
             mmpl_vae_softmax, mmpl_vae_transpose, mmpl_vae_zprep, mmpl_vae_mu_out, mmpl_vae_px_in, mmpl_vae_px_out,
             mmpl_vae_px_out_u8, mmpl_gemm_ex; `copy` is a device-to-device copy of one frame).  Every intermediate is a buffer of its
             own with a tail of the 0x7FA5 canary, filled with that NaN pattern too unless the model pads it with zeros.
  VaeRefOps  each op as its documented contract in plain torch on the CPU, float64 or float32; round=True rounds to bf16 where the
             kernels do (through the per-launch references of tests/vae_kernel_ref.py: vae_conv_ref, rms_norm_ref, softmax_ref),
             round=False never rounds.

tests/test_vae_chain_host.py shows on the CPU that the chain is the model (VaeRefOps against the oracle, both in float64);
tests/test_vae_chain_gpu.py demands that the library's decode / encode / stream equal the VaeHipOps chain in every bit.

WIRING holds the decisions of the model a composition can get wrong; a test hands in an altered copy to build a mutant of the chain.
FUSE holds the one choice of the PRODUCT that changes bits (see there).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from tests import vae_kernel_ref as R

BF = torch.bfloat16
CANARY = 0x7FA5                       # the NaN pattern of the exact tests
TAIL = 128                            # canary elements (int16) behind every VaeHipOps buffer
EPI_BIAS, EPI_RES, EPI_F32 = 0, 4, 5  # mmpl_gemm_ex's `epi`
K_HALO6, K_HALO1 = 3, 4               # mmpl_vae_conv's kernel_out: conv_halo_kernel<6> / <1>
DIM, ZD = 96, 16
DIM_MULT = (1, 2, 4, 4)
T_DOWN = (False, True, True)          # temperal_downsample (vae.py:617-624)
# the latent statistics of Wan2.1 (mmpl_amd/wan_wrapper.py), which every VAE test of the suite uses
MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508, 0.4134, -0.0715, 0.5517, -0.3632, -0.1922,
        -0.9497, 0.2503, -0.2921]
STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743, 3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253,
       2.8251, 1.9160]

# The model's wiring (the numbers are lines of wan/modules/vae.py).
WIRING = dict(
    cache_frames=2,                                         # :14 CACHE_T: a CausalConv3d's cache is its last TWO input frames
    first_frame="rep",                                      # :103-113 the video's first latent frame skips the upsampler's time_conv ('Rep')
    enc_down_order=("resample", "time_conv"),               # :138-159 downsample3d: the strided Conv2d first, then the time_conv
    norm2_gamma=lambda pre, cin, cout: pre + "residual.3.gamma",   # :192-197 the second norm of a ResidualBlock has its own gamma
    shortcut_src="input",                                   # :203 h = self.shortcut(x): the 1x1x1 conv of a widening block reads the block INPUT
    attn_scale=lambda c: float(np.float32(1.0) / np.sqrt(np.float32(c))),   # :255 scaled_dot_product_attention: 1 / sqrt(C)
    down_pad=(0, 0),                                        # :87 ZeroPad2d((0, 1, 0, 1)): the zero row / column is at the bottom / right
    dec_head_gamma="decoder.head.0.gamma",                  # :418 the head has its own RMS_norm
    enc_head_gamma="encoder.head.0.gamma",                  # :313
)

# The product's one choice that changes bits: where the RMS_norm + SiLU in front of a cached 3x3x3 conv runs in the PRODUCING conv's
# epilogue (mmpl_vae_conv's ngamma: same rounding points, another order of the fp32 sum of squares) instead of as a norm pass.
# The launcher allows it for a stride-1 3x3(x3) conv on conv_halo_kernel<6> with 96 output channels and at most 8 output frames,
# whose consumer takes frame pointers (a halo conv); of the edges of the network that qualify, these are the ones that use it.
# MMPL_VAE_NO_FUSE_NORM=1 (fuse=False here) turns all of them off.
FUSE = dict(
    res_inner=True,               # residual.2 -> residual.6 inside one ResidualBlock, decoder and encoder
    dec_block_to_block=True,      # a decoder block's residual.6 -> the next block's residual.2 in the same stage
    dec_up_to_block=True,         # an upsampler's Conv2d -> the first block of the next stage
    dec_last_to_head=True,        # the last block's residual.6 -> decoder.head.2
    enc_conv1_to_block=False,     # encoder.conv1 -> the first block: qualifies, runs the norm pass
    enc_block_to_block=False,     # an encoder block's residual.6 -> the next block's residual.2: qualifies, runs the norm pass
)


def latent_scales(mean: Sequence[float], std: Sequence[float]):
    """wan_wrapper.py:74-113: mean and 1 / std in bf16 arithmetic -> two lists of 16 floats."""
    m = torch.tensor(mean, dtype=torch.float32).to(BF)
    inv = 1.0 / torch.tensor(std, dtype=torch.float32).to(BF)
    return m.float().tolist(), inv.float().tolist()


def takes_halo(N: int, k, s, frag: bool) -> bool:
    """include/mmpl_hip.h, mmpl_vae_conv: with Wfrag, a 3x3(x3 | x1) stride-1 conv out of a source padded by one pixel with
    N % 96 == 0 or N <= 16 takes conv_halo_kernel (every stride-1 3x3 conv of the chain reads such a source)."""
    return bool(frag) and k[1] == 3 and k[2] == 3 and k[0] in (1, 3) and tuple(s) == (1, 1, 1) and (N % 96 == 0 or N <= 16)


# ====================================================================================================== packing
def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[N, Cin, (kt,) kh, kw] -> [N, ntaps * Cin32]: tap-major, Cin contiguous and padded with zeros to a multiple of 32."""
    n, cin = w.shape[:2]
    t = w.reshape(n, cin, -1).permute(0, 2, 1)
    if cin % 32:
        t = F.pad(t, (0, 32 - cin % 32))
    return t.reshape(n, -1).contiguous()


def pack_frag(w2d: torch.Tensor, cin: int) -> torch.Tensor:
    """The header's "<conv>.weight.frag": [Cin / 32][ntaps][ceil(N / 16)][64 lanes][8], lane = 16 * (k chunk of 8) + (row within the
    16), rows zero-padded to a multiple of 16 -- as a gather by that index formula."""
    n, k = w2d.shape
    ntaps, nchunk, nj = k // cin, cin // 32, (n + 15) // 16
    i = torch.arange(nchunk * ntaps * nj * 512)
    e, lane, g, tap, ch = i % 8, i // 8 % 64, i // 512 % nj, i // (512 * nj) % ntaps, i // (512 * nj * ntaps)
    wp = F.pad(w2d, (0, 0, 0, nj * 16 - n))
    return wp[16 * g + lane % 16, tap * cin + 32 * ch + 8 * (lane // 16) + e].contiguous()


class _Conv:
    def __init__(self, name, W, Wfrag, bias, N, Cin, k):
        self.name, self.W, self.Wfrag, self.bias, self.N, self.Cin, self.k = name, W, Wfrag, bias, N, Cin, k


# ====================================================================================================== backends
class VaeRefOps:
    """Every op as its documented contract (include/mmpl_hip.h), in plain torch on the CPU.  Activations are channels-last."""

    def __init__(self, dtype=torch.float64, round: bool = False):
        assert not round or dtype == torch.float64, "the bf16 roundings of tests/vae_kernel_ref.py are done in float64"
        self.dtype, self.round = dtype, round

    def _r(self, x):
        return R.rbf(x) if self.round else x

    def new(self, shape, zero=False, kind="bf16"):
        if kind == "u8":
            return torch.full(tuple(shape), 0xA5, dtype=torch.uint8)
        return torch.zeros(tuple(shape), dtype=self.dtype) if zero else torch.full(tuple(shape), float("nan"), dtype=self.dtype)

    def param(self, t):
        return t.detach().to("cpu").to(self.dtype).contiguous()

    def tensor(self, t):
        return self.param(t)

    def finish(self):
        pass

    def canaries_intact(self) -> bool:
        return True

    def _norm(self, x, gamma, silu):
        if gamma is None:
            return x
        if self.round:
            return R.rms_norm_ref(x, gamma, silu)[0]
        y = x / torch.sqrt((x * x).sum(-1, keepdim=True)).clamp_min(1e-12) * math.sqrt(x.shape[-1]) * gamma
        return y / (1.0 + torch.exp(-y)) if silu else y

    def conv(self, cv, out, k, s, To, Ho, Wo, frames=None, src=None, res=None, ngamma=None, nframes=None, halo=False):
        vol = torch.stack(list(frames)) if frames is not None else src
        Tp = (To - 1) * s[0] + k[0]
        xp = vol[:Tp].permute(3, 0, 1, 2).unsqueeze(0)
        w = cv.W.view(cv.N, k[0], k[1], k[2], cv.Cin).permute(0, 4, 1, 2, 3)
        r = None if res is None else res.reshape(To, Ho, Wo, -1)[..., :cv.N].permute(3, 0, 1, 2).unsqueeze(0)
        if self.round:
            y, _ = R.vae_conv_ref(xp, w, cv.bias, tuple(s), r)
        else:
            y = F.conv3d(xp, w, None, stride=tuple(s)) + cv.bias.view(1, -1, 1, 1, 1)
            y = y if r is None else y + r
        assert tuple(y.shape[2:]) == (To, Ho, Wo), (cv.name, tuple(y.shape), (To, Ho, Wo))
        ycl = y[0].permute(1, 2, 3, 0)
        if out is not None:
            out.copy_(ycl)
        if ngamma is not None:
            n = self._norm(ycl, ngamma, True)
            for t in range(To):
                nframes[t][1:-1, 1:-1, :] = n[t]

    def norm(self, dst, x, gamma, silu, dt0=0, dy0=0, dx0=0):
        T, H, W, C_ = x.shape
        dst[dt0:dt0 + T, dy0:dy0 + H, dx0:dx0 + W, :C_] = self._norm(x, gamma, silu)

    def upsample(self, dst, src, lds, C_, H, W, To, interleave):
        Ts = To // 2 if interleave else To
        v = src.reshape(Ts, H, W, lds)
        v = v[..., :2 * C_].reshape(Ts, H, W, 2, C_).permute(0, 3, 1, 2, 4).reshape(To, H, W, C_) if interleave else v[..., :C_]
        dst[:, 1:-1, 1:-1, :] = v.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

    def softmax(self, p, sc, cols):
        p[:, :cols] = self._r(R.softmax_ref(sc[:, :cols]).to(self.dtype) if self.round else torch.softmax(sc[:, :cols], dim=-1))
        p[:, cols:] = 0

    def transpose(self, vt, v, rows):
        vt[:, :rows] = v[:rows].t()
        vt[:, rows:] = 0

    def zprep(self, dst, z, mean, inv, w2, b2):
        m, i = torch.tensor(mean, dtype=self.dtype), torch.tensor(inv, dtype=self.dtype)
        v = z.permute(0, 2, 3, 1)
        zz = self._r(self._r(v / i) + m)
        dst[:, 1:-1, 1:-1, :16] = self._r(zz @ w2.t() + b2)

    def mu_out(self, out, f_out, enc, w1, b1, mean, inv, F_, h, w):
        m, i = torch.tensor(mean, dtype=self.dtype), torch.tensor(inv, dtype=self.dtype)
        mu = self._r(enc.reshape(F_, h, w, 32) @ w1[:16].t() + b1[:16])
        out[f_out:f_out + F_] = self._r(self._r(mu - m) * i).permute(0, 3, 1, 2)

    def gemm(self, name, out, A, W, bias, M, N, K, epi=EPI_BIAS, res=None, alpha=1.0):
        acc = A[:M, :K] @ W[:N, :K].t()
        if epi == EPI_F32:
            out[:M, :N] = (alpha * acc).to(torch.float32).to(self.dtype) if self.round else alpha * acc
            return
        y = self._r(acc + (0 if bias is None else bias))
        out[:M, :N] = self._r(res[:M, :N] + y) if epi == EPI_RES else y

    def px_in(self, dst, px, Ttot, t):
        dst[0, 1:-1, 1:-1, :3] = px[:, t].permute(1, 2, 0)

    def px_out(self, out, src, t_out):
        T = src.shape[0]
        out[t_out:t_out + T] = src[..., :3].clamp(-1.0, 1.0).permute(0, 3, 1, 2)

    def px_out_u8(self, out, src, t_out):
        T = src.shape[0]
        v = (src[..., :3].clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1)
        out[t_out:t_out + T] = (v * 255.0).clamp(0, 255).to(torch.uint8)

    def copy(self, dst, src):
        dst.copy_(src)


class VaeHipOps:
    """Every op is one call of the matching single-launch entry of libmmpl_hip.so on the current stream of `device`."""

    def __init__(self, lib, device="cuda:0"):
        from mmpl_amd import _lib
        self.lib, self._lib, self.device = lib, _lib, torch.device(device)
        self.buffers: List[torch.Tensor] = []
        self.payload: List[int] = []
        self.kernels: Dict[str, int] = {}                  # conv name -> kernel_out of its last launch
        self.launches = 0

    # ---- buffers
    def new(self, shape, zero=False, kind="bf16"):
        dtype, size = {"bf16": (BF, 2), "f32": (torch.float32, 4), "u8": (torch.uint8, 1)}[kind]
        nbytes = math.prod(shape) * size
        assert nbytes % 2 == 0
        b = torch.full((nbytes // 2 + TAIL,), CANARY, dtype=torch.int16, device=self.device)
        self.buffers.append(b)
        self.payload.append(nbytes // 2)
        if zero:
            b[:nbytes // 2] = 0
        return b[:nbytes // 2].view(dtype).view(tuple(shape))

    def param(self, t):
        return t.detach().to(device=self.device, dtype=BF).contiguous()

    def tensor(self, t):
        return t.detach().to(self.device).contiguous()

    def finish(self):
        torch.cuda.synchronize(self.device)

    def canaries_intact(self) -> bool:
        torch.cuda.synchronize(self.device)
        return all(bool((b[n:] == CANARY).all()) for b, n in zip(self.buffers, self.payload))

    # ---- helpers
    def _p(self, t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _ptrs(self, ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, rc, what):
        self.launches += 1
        self._lib.check(rc, what)

    @staticmethod
    def _f16(v):
        return (C.c_float * 16)(*v)

    # ---- ops
    def conv(self, cv, out, k, s, To, Ho, Wo, frames=None, src=None, res=None, ngamma=None, nframes=None, halo=False):
        first = frames[0] if frames is not None else src[0]
        Hp, Wp, Cin = first.shape
        assert Cin == cv.Cin and (frames is None or all(f.is_contiguous() for f in frames))
        kernel = C.c_int(-1)
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_conv(
                self._p(src), None if frames is None else self._ptrs(frames), 0 if frames is None else len(frames), Cin, Hp, Wp, *s, *k,
                self._p(cv.W), self._p(cv.Wfrag), self._p(cv.bias), To, Ho, Wo, cv.N, self._p(out), Ho, Wo, cv.N, 0, 0, 0, self._p(res),
                0 if res is None else cv.N, self._p(ngamma), math.sqrt(cv.N), None if nframes is None else self._ptrs(nframes),
                C.byref(kernel), self._stream()), "conv " + cv.name)
        assert (kernel.value in (K_HALO6, K_HALO1)) == halo, f"{cv.name}: the launcher took kernel {kernel.value}"
        self.kernels[cv.name] = kernel.value

    def norm(self, dst, x, gamma, silu, dt0=0, dy0=0, dx0=0):
        T, H, W, C_ = x.shape
        _, Hd, Wd, ldd = dst.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_norm(self._p(x), T, H, W, C_, self._p(gamma), math.sqrt(C_), int(silu), self._p(dst), Hd, Wd, ldd,
                                              dt0, dy0, dx0, self._stream()), "norm")

    def upsample(self, dst, src, lds, C_, H, W, To, interleave):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_upsample(self._p(src), lds, C_, H, W, To, interleave, self._p(dst), 2 * H + 2, 2 * W + 2,
                                                  self._stream()), "upsample")

    def softmax(self, p, sc, cols):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_softmax(self._p(sc), sc.stride(0), self._p(p), p.stride(0), p.shape[0], cols, self._stream()), "softmax")

    def transpose(self, vt, v, rows):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_transpose(self._p(v), v.stride(0), self._p(vt), vt.stride(0), rows, vt.shape[0], self._stream()),
                       "transpose")

    def zprep(self, dst, z, mean, inv, w2, b2):
        F_, _, h, w = z.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_zprep(self._p(z), F_, h, w, self._f16(mean), self._f16(inv), self._p(w2), self._p(b2), self._p(dst), 0,
                                               self._stream()), "zprep")

    def mu_out(self, out, f_out, enc, w1, b1, mean, inv, F_, h, w):
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_mu_out(self._p(enc), self._p(w1), self._p(b1), self._f16(mean), self._f16(inv), self._p(out), F_, f_out,
                                                h, w, self._stream()), "mu_out")

    def gemm(self, name, out, A, W, bias, M, N, K, epi=EPI_BIAS, res=None, alpha=1.0):
        plan = (C.c_int * 6)(*([-1] * 6))
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_gemm_ex(self._p(A), A.stride(0), self._p(W), W.stride(0), self._p(bias), self._p(out), out.stride(0), M, N, K,
                                             epi, self._p(res), 0 if res is None else res.stride(0), None, 0, 1, alpha, 1, 0, 0, 0, None, 0, 0, 0,
                                             None, 0, None, plan, self._stream()), "gemm " + name)

    def px_in(self, dst, px, Ttot, t):
        _, Hp, Wp, _ = dst.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_px_in(self._p(px), self._p(dst), Ttot, t, 1, Hp - 2, Wp - 2, 0, self._stream()), "px_in")

    def px_out(self, out, src, t_out):
        T, H, W, _ = src.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_px_out(self._p(src), self._p(out), T, H, W, t_out, self._stream()), "px_out")

    def px_out_u8(self, out, src, t_out):
        T, H, W, _ = src.shape
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_vae_px_out_u8(self._p(src), self._p(out), T, H, W, t_out, self._stream()), "px_out_u8")

    def copy(self, dst, src):
        assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
        dst.copy_(src)


# ====================================================================================================== the chain
class _State:
    """What a video carries from one latent frame / pixel chunk to the next: every cached conv's last input frames, the frames a
    producer's epilogue has already normalised for its consumer, and how many frames / chunks went through."""

    def __init__(self):
        self.cache: Dict[str, list] = {}
        self.pending: Dict[str, tuple] = {}
        self.n = 0


class VaeChain:
    def __init__(self, sd, lat_h: int, lat_w: int, ops, wiring: Optional[dict] = None, fuse=None):
        self.sd, self.h, self.w, self.ops = sd, lat_h, lat_w, ops
        self.wr = dict(WIRING)
        self.wr.update(wiring or {})
        self.fuse = {k: False for k in FUSE} if fuse is False else dict(FUSE, **(fuse or {}))
        self._cv: Dict[str, _Conv] = {}
        self._par: Dict[str, torch.Tensor] = {}

    # ---- parameters, packed here
    def cv(self, name: str, frag: bool) -> _Conv:
        if name not in self._cv:
            w, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
            if w.dim() == 4:                                  # a Resample's Conv2d is a (1, 3, 3) filter
                w = w.unsqueeze(2)
            if name == "decoder.head.2":                      # three output channels, stored as four
                w, b = torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))]), torch.cat([b, b.new_zeros(1)])
            W2 = pack_conv(w)
            k = tuple(w.shape[2:])
            cin = W2.shape[1] // math.prod(k)
            self._cv[name] = _Conv(name, self.ops.param(W2), self.ops.param(pack_frag(W2, cin)) if frag else None,
                                   self.ops.param(b.reshape(-1)), w.shape[0], cin, k)
        assert (self._cv[name].Wfrag is not None) == frag
        return self._cv[name]

    def par(self, key: str, shape=None) -> torch.Tensor:
        """gamma [C], or the weight of a 1x1 conv as a matrix."""
        if key not in self._par:
            t = self.sd[key]
            self._par[key] = self.ops.param(t.reshape(-1) if shape is None else t.reshape(shape))
        return self._par[key]

    # ---- pieces
    def _frame(self, H, W, C_, pad=1):
        return self.ops.new((H + 2 * pad, W + 2 * pad, C_), zero=True)

    def _keep(self, frames):
        """The cache after a conv saw `frames` (its cache followed by its new input): the last two of them."""
        n = self.wr["cache_frames"]
        return list(frames[-n:])

    def _history(self, st, name, make, want=2):
        """The `want` frames in front of a conv's new input: its cache, zeros where the video has not reached that far back."""
        have = st.cache.get(name, [])[-want:]
        return [make() for _ in range(want - len(have))] + list(have)

    def _fuse(self, st, edge, N, halo, T, H, W):
        """-> (gamma, frames) for the producing conv's epilogue, or (None, None): the norm pass will run."""
        if edge is None:
            return None, None
        kind, cname, gname, cN = edge
        if not (self.fuse[kind] and halo and N == 96 and T <= 8 and takes_halo(cN, (3, 3, 3), (1, 1, 1), True)):
            return None, None
        frames = [self._frame(H, W, N) for _ in range(T)]
        st.pending[cname] = (frames, gname)
        return self.par(gname), frames

    def _cconv(self, st, name, x, gname, T, H, W, Cin, N, res=None, edge=None, keep_out=True, new_frames=None):
        """CausalConv3d(3, padding 1) behind RMS_norm + SiLU (gname) or on frames prepared by the caller (new_frames, already padded):
        the conv reads [the last two input frames | the T new ones] (vae.py:28-36, 207-216).  -> plain [T, H, W, N], or None when only
        the fused consumer reads the result."""
        ops = self.ops
        cv = self.cv(name, frag=True)
        halo = takes_halo(N, (3, 3, 3), (1, 1, 1), True)
        if name in st.pending:
            new, g_applied = st.pending.pop(name)
            assert g_applied == gname and len(new) == T, (name, g_applied, gname)
        elif new_frames is not None:
            new = list(new_frames)
        else:
            new = []
            for t in range(T):
                f = self._frame(H, W, Cin)
                ops.norm(f.unsqueeze(0), x[t:t + 1], self.par(gname), True, 0, 1, 1)
                new.append(f)
        frames = self._history(st, name, lambda: self._frame(H, W, Cin)) + new
        ng, nfr = self._fuse(st, edge, N, halo, T, H, W)
        out = ops.new((T, H, W, N)) if (keep_out or ng is None) else None
        if halo:
            ops.conv(cv, out, (3, 3, 3), (1, 1, 1), T, H, W, frames=frames, res=res, ngamma=ng, nframes=nfr, halo=True)
        else:
            vol = ops.new((T + 2, H + 2, W + 2, Cin))
            for j, f in enumerate(frames):
                ops.copy(vol[j], f)
            ops.conv(cv, out, (3, 3, 3), (1, 1, 1), T, H, W, src=vol, res=res, halo=False)
        st.cache[name] = self._keep(frames)
        return out

    def _res_block(self, st, pre, x, T, H, W, cin, cout, out_edge=None):
        """ResidualBlock (vae.py:186-220): shortcut(x) + conv(silu(norm(conv(silu(norm(x))))))."""
        ops = self.ops
        g0, g3 = pre + "residual.0.gamma", self.wr["norm2_gamma"](pre, cin, cout)
        h = x
        if cin != cout:
            src = x
            if self.wr["shortcut_src"] != "input":
                src = ops.new((T, H, W, cin))
                ops.norm(src, x, self.par(g0), True)
            h = ops.new((T, H, W, cout))
            ops.conv(self.cv(pre + "shortcut", frag=False), h, (1, 1, 1), (1, 1, 1), T, H, W, src=src, halo=False)
        a = self._cconv(st, pre + "residual.2", x, g0, T, H, W, cin, cout, edge=("res_inner", pre + "residual.6", g3, cout), keep_out=False)
        return self._cconv(st, pre + "residual.6", a, g3, T, H, W, cout, cout, res=h, edge=out_edge)

    def _attn(self, pre, x, T, H, W, C_):
        """AttentionBlock (vae.py:223-262): per frame, one head of dim C over the H * W tokens; x + proj(softmax(q k^T / sqrt(C)) v).
        Launch contracts: the P . V GEMM needs K % 64 == 0, so P and V^T are padded with zeros to HWp columns (the softmax and the
        transpose write those zeros); a GEMM stores N % 4 == 0 columns, so the scores are computed against HW4 = HW rounded up to 4
        keys, the extra ones being zero rows of qkv whose scores the softmax never reads."""
        ops = self.ops
        HW, HWp, HW4 = H * W, (H * W + 63) // 64 * 64, (H * W + 3) // 4 * 4
        wq, bq = self.par(pre + "to_qkv.weight", (3 * C_, C_)), self.par(pre + "to_qkv.bias")
        wp, bp = self.par(pre + "proj.weight", (C_, C_)), self.par(pre + "proj.bias")
        out = ops.new((T, H, W, C_))
        for t in range(T):
            xn = ops.new((1, H, W, C_))
            ops.norm(xn, x[t:t + 1], self.par(pre + "norm.gamma"), False)
            qkv = ops.new((HW4, 3 * C_), zero=True)
            ops.gemm("to_qkv", qkv, xn.view(HW, C_), wq, bq, HW, 3 * C_, C_)
            sc = ops.new((HW, HWp), kind="f32")
            ops.gemm("scores", sc, qkv[:, :C_], qkv[:, C_:2 * C_], None, HW, HW4, C_, epi=EPI_F32, alpha=self.wr["attn_scale"](C_))
            p = ops.new((HW, HWp))
            ops.softmax(p, sc, HW)
            vt = ops.new((C_, HWp))
            ops.transpose(vt, qkv[:, 2 * C_:], HW)
            o = ops.new((HW, C_))
            ops.gemm("pv", o, p, vt, None, HW, C_, HWp)
            ops.gemm("proj", out[t].view(HW, C_), o, wp, bp, HW, C_, C_, epi=EPI_RES, res=x[t].view(HW, C_))
        return out

    def _own(self, frame):
        f = self.ops.new(tuple(frame.shape))
        self.ops.copy(f, frame)
        return f

    def _up(self, st, pre, x, T, H, W, C_, temporal, first, edge):
        """Resample upsample2d / upsample3d (vae.py:101-141): [time_conv C -> 2C, the halves becoming frames 2t, 2t + 1], nearest x2,
        Conv2d(C, C / 2, 3, padding 1).  The video's first latent frame skips the time_conv and is NOT cached ('Rep')."""
        ops = self.ops
        src, lds, To, inter = x, C_, T, 0
        if temporal and not (first and self.wr["first_frame"] == "rep"):
            name = pre + "time_conv"
            new = [self._own(x[t]) for t in range(T)]
            frames = self._history(st, name, lambda: ops.new((H, W, C_), zero=True)) + new
            vol = ops.new((T + 2, H, W, C_))
            for j, f in enumerate(frames):
                ops.copy(vol[j], f)
            y = ops.new((T, H, W, 2 * C_))
            ops.conv(self.cv(name, frag=False), y, (3, 1, 1), (1, 1, 1), T, H, W, src=vol, halo=False)
            st.cache[name] = self._keep(frames)
            src, lds = y, 2 * C_
            if not first:
                To, inter = 2 * T, 1
        up = ops.new((To, 2 * H + 2, 2 * W + 2, C_), zero=True)
        ops.upsample(up, src, lds, C_, H, W, To, inter)
        T, H, W = To, 2 * H, 2 * W
        cv = self.cv(pre + "resample.1", frag=True)
        halo = takes_halo(C_ // 2, (1, 3, 3), (1, 1, 1), True)
        ng, nfr = self._fuse(st, edge, C_ // 2, halo, T, H, W)
        y = ops.new((T, H, W, C_ // 2))
        ops.conv(cv, y, (1, 3, 3), (1, 1, 1), T, H, W, src=up, ngamma=ng, nframes=nfr, halo=halo)
        return y, T, H, W

    def _down(self, st, pre, x, T, H, W, C_, temporal, first):
        """Resample downsample2d / downsample3d (vae.py:138-160): ZeroPad2d((0, 1, 0, 1)) + Conv2d(C, C, 3, stride 2), then the
        time_conv (3, 1, 1) of stride 2 over [the last frame of the chunk before | x]; the first chunk only fills that cache."""
        ops = self.ops
        for step in self.wr["enc_down_order"]:
            if step == "resample":
                dy, dx = self.wr["down_pad"]
                pd = ops.new((T, H + 1, W + 1, C_), zero=True)
                ops.norm(pd, x, None, False, 0, dy, dx)
                y = ops.new((T, H // 2, W // 2, C_))
                ops.conv(self.cv(pre + "resample.1", frag=False), y, (1, 3, 3), (1, 2, 2), T, H // 2, W // 2, src=pd, halo=False)
                x, H, W = y, H // 2, W // 2
            elif temporal:
                name = pre + "time_conv"
                if first:
                    st.cache[name] = [self._own(x[T - 1])]
                    continue
                vol = ops.new((T + 1, H, W, C_))
                ops.copy(vol[0], st.cache[name][-1])
                for t in range(T):
                    ops.copy(vol[t + 1], x[t])
                To = (T + 1 - 3) // 2 + 1
                y = ops.new((To, H, W, C_))
                ops.conv(self.cv(name, frag=False), y, (3, 1, 1), (2, 1, 1), To, H, W, src=vol, halo=False)
                st.cache[name] = [self._own(x[T - 1])]
                x, T = y, To
        return x, T, H, W

    # ---- one latent frame / one pixel chunk
    def _decoder_frame(self, st, z1, mean, inv, out, out_format, t_out):
        """Decoder3d.forward on one latent frame (vae.py:423-472) behind the de-normalisation and conv2 (:548-554).  -> frames written."""
        ops, h, w = self.ops, self.h, self.w
        first = st.n == 0
        zf = ops.new((1, h + 2, w + 2, 32), zero=True)
        ops.zprep(zf, z1, mean, inv, self.par("conv2.weight", (16, 16)), self.par("conv2.bias"))
        x = self._cconv(st, "decoder.conv1", None, None, 1, h, w, 32, 384, new_frames=[zf[0]])
        x = self._res_block(st, "decoder.middle.0.", x, 1, h, w, 384, 384)
        x = self._attn("decoder.middle.1.", x, 1, h, w, 384)
        x = self._res_block(st, "decoder.middle.2.", x, 1, h, w, 384, 384)
        dims = [DIM * u for u in (DIM_MULT[-1],) + DIM_MULT[::-1]]            # 384 384 384 192 96
        t_up = T_DOWN[::-1]
        T, H, W, j = 1, h, w, 0
        for i in range(4):
            cin, cout = dims[i], dims[i + 1]
            if i >= 1:
                cin //= 2                                                      # the upsampler in front halved the channels
            for r in range(3):
                nxt = f"decoder.upsamples.{j + 1}."
                edge = None
                if r < 2:
                    edge = ("dec_block_to_block", nxt + "residual.2", nxt + "residual.0.gamma", cout)
                elif i == 3:
                    edge = ("dec_last_to_head", "decoder.head.2", self.wr["dec_head_gamma"], 4)
                x = self._res_block(st, f"decoder.upsamples.{j}.", x, T, H, W, cin, cout, edge)
                cin = cout
                j += 1
            if i != 3:
                nxt = f"decoder.upsamples.{j + 1}."
                edge = ("dec_up_to_block", nxt + "residual.2", nxt + "residual.0.gamma", dims[i + 2])
                x, T, H, W = self._up(st, f"decoder.upsamples.{j}.", x, T, H, W, cout, t_up[i], first, edge)
                j += 1
        y = self._cconv(st, "decoder.head.2", x, self.wr["dec_head_gamma"], T, H, W, DIM, 4)
        (ops.px_out_u8 if out_format == "uint8" else ops.px_out)(out, y, t_out)
        st.n += 1
        return T

    def _encoder_chunk(self, st, px, Ttot, t0, T, mean, inv, out, f_out):
        """Encoder3d.forward on one chunk of pixel frames (vae.py:318-366), then conv1's mu half and the normalisation (:536-541)."""
        ops = self.ops
        first = st.n == 0
        H, W = 8 * self.h, 8 * self.w
        new = []
        for t in range(T):
            f = ops.new((1, H + 2, W + 2, 32), zero=True)
            ops.px_in(f, px, Ttot, t0 + t)
            new.append(f[0])
        edge = ("enc_conv1_to_block", "encoder.downsamples.0.residual.2", "encoder.downsamples.0.residual.0.gamma", DIM)
        x = self._cconv(st, "encoder.conv1", None, None, T, H, W, 32, DIM, new_frames=new, edge=edge)
        dims = [DIM * u for u in (1,) + DIM_MULT]                             # 96 96 192 384 384
        j = 0
        for i in range(4):
            cin, cout = dims[i], dims[i + 1]
            for r in range(2):
                nxt = f"encoder.downsamples.{j + 1}."
                edge = ("enc_block_to_block", nxt + "residual.2", nxt + "residual.0.gamma", cout) if r == 0 else None
                x = self._res_block(st, f"encoder.downsamples.{j}.", x, T, H, W, cin, cout, edge)
                cin = cout
                j += 1
            if i != 3:
                x, T, H, W = self._down(st, f"encoder.downsamples.{j}.", x, T, H, W, cout, T_DOWN[i], first)
                j += 1
        x = self._res_block(st, "encoder.middle.0.", x, T, H, W, 384, 384)
        x = self._attn("encoder.middle.1.", x, T, H, W, 384)
        x = self._res_block(st, "encoder.middle.2.", x, T, H, W, 384, 384)
        y = self._cconv(st, "encoder.head.2", x, self.wr["enc_head_gamma"], T, H, W, 384, 32)
        ops.mu_out(out, f_out, y.view(T * H * W, 32), self.par("conv1.weight", (32, 32)), self.par("conv1.bias"), mean, inv, T, H, W)
        st.n += 1

    # ---- the products
    def _decode_into(self, st, z, mean, inv, out_format):
        ops = self.ops
        z = ops.tensor(z) if isinstance(ops, VaeRefOps) else ops.tensor(z.to(BF))
        F_ = z.shape[0]
        n = 4 * F_ - (3 if st.n == 0 else 0)
        H, W = 8 * self.h, 8 * self.w
        out = ops.new((n, H, W, 3), kind="u8") if out_format == "uint8" else ops.new((n, 3, H, W), kind="f32")
        t_out = 0
        for i in range(F_):
            t_out += self._decoder_frame(st, z[i:i + 1], mean, inv, out, out_format, t_out)
        assert t_out == n
        ops.finish()
        return out

    def decode(self, z, mean, inv, out_format="float"):
        """WanVAE_.decode + the wrapper's clamp: z [F, 16, h, w] -> [1 + 4 (F - 1), 3, 8h, 8w] in [-1, 1] (or uint8 [T, 8h, 8w, 3])."""
        return self._decode_into(_State(), z, mean, inv, out_format)

    def encode(self, px, mean, inv):
        """WanVAE_.encode: px [3, 1 + 4k, 8h, 8w] -> normalised mu [1 + k, 16, h, w]: the first frame alone, then chunks of four."""
        ops = self.ops
        px = ops.tensor(px) if isinstance(ops, VaeRefOps) else ops.tensor(px.to(BF))
        Ttot = px.shape[1]
        assert (Ttot - 1) % 4 == 0
        n = 1 + (Ttot - 1) // 4
        out = ops.new((n, 16, self.h, self.w), kind="f32")
        st = _State()
        for i in range(n):
            self._encoder_chunk(st, px, Ttot, 0 if i == 0 else 1 + 4 * (i - 1), 1 if i == 0 else 4, mean, inv, out, i)
        ops.finish()
        return out

    def stream(self):
        return VaeChainStream(self)


class VaeChainStream:
    """WanVAE_.cached_decode (vae.py:571-593): the caches live from one call to the next; clear_cache starts a new video."""

    def __init__(self, chain: VaeChain):
        self.chain, self.st = chain, _State()

    def clear_cache(self):
        self.st = _State()

    def decode(self, z, mean, inv, out_format="float"):
        return self.chain._decode_into(self.st, z, mean, inv, out_format)
