"""The TAEHV preview autoencoder (mmpl_taehv_decode, mmpl_taehv_encode) as ORDERED LISTS OF LAUNCHES, written from the model -- the
layer list of the reference's demo_utils/taehv.py (TAEHV.decode_video / encode_video, restated in tests/taehv_ref.py and
tests/taehv_enc_ref.py) -- on the launch contracts of include/mmpl_hip.h, not from csrc/taehv.hip, taehv_enc.hip or taehv_host.h.

`TaehvChain(sd, lat_h, lat_w, ops)` takes the REFERENCE state dict (the keys of mmpl_amd.synthetic.taehv_state_dict /
taehv_encoder_state_dict) and packs it itself, from the header's description of the operands: fragment-major
[K / 32][ntaps][Nw / 16][64][8] (vae_chain.pack_frag), K order [x, past], Cin padded to 32, the head 3 of 16 with the bias padded to 4,
the input layer's k = (3 ky + kx) * 3 + c, the last channels * stride rows of a TGrow weight.  It never calls TaehvEngine._repack,
TaehvEncoderEngine._repack, VaeEngine._frag_pack or patch_tgrow_layers, which are under test.

Memory as the model has it.  A MemBlock has ONE frame of memory in a buffer of its own, zeros before the video starts.  For a call
of T frames the chain builds `past` = [memory, x_0 .. x_{T-2}] as a fresh volume of T frames (device copies), hands x and past to
the conv as two separate runs, and sets the new memory by copying x_{T-1} itself (keep = NULL).  There is no overlapping run, no
memory slot, no group of 3 and no fixed layout: a call's frames go through every layer in ONE launch whatever their number, the
full-resolution encoder level and the 8x decoder level included.

Level changes as the model orders them.  Decoder: an explicit nearest x2 up-sampled zero-bordered buffer, then TGrow's 1x1 conv AT
THE HIGH RESOLUTION -- one launch per channel block k with that block's rows of the weight, written to the frames S t + k -- then
the 3x3 conv with up = 0.  Encoder: TPool reads the frame pair (2t, 2t + 1), copied into two runs of their own, as src0 / src1, then
the stride-2 conv.  The product runs TGrow at the low resolution as one launch with a channel -> frame split and folds the
up-sampling into the 3x3 conv's addressing; a 1x1 conv is per pixel and per output channel, and the 3x3 conv stages the same values
in the same order, so both must give the same bits.

Every launch goes through a small `ops` backend:

  TaehvHipOps  each op is exactly ONE call of mmpl_taehv_conv, mmpl_taehv_prep, mmpl_taehv_conv_in, mmpl_taehv_conv_s2,
               mmpl_taehv_z_out or mmpl_taehv_px_out; `copy`, `upsample` and `fill` are device-side data movement.  Every intermediate
               is a buffer of its own: the zero border is written here, the interior is pre-filled with the 0x7FA5 NaN pattern, a
               128-element canary tail follows it.
  TaehvRefOps  each op as its documented contract in plain torch on the CPU, float64 or float32; round=True rounds to bf16 where
               the kernels do, round=False never rounds.

tests/test_taehv_chain_host.py shows on the CPU that the chain is the model; tests/test_taehv_chain_gpu.py demands that the
library's decode / encode / streaming equal the TaehvHipOps chain in every bit.

WIRING holds the decisions of the model a composition can get wrong; a test hands in an altered copy to build a mutant of the chain.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from tests.vae_chain import CANARY, TAIL, pack_conv, pack_frag

BF = torch.bfloat16
DEC_CH = (256, 128, 64, 64)           # decoder channels at 1x / 2x / 4x / 8x
GROW = (1, 2, 2)                      # TGrow stride leaving decoder level l
POOL = (2, 2, 1)                      # TPool stride entering encoder level l
ENC_C = 64

# The model's wiring.  Every value is one a test alters to build a mutant (tests/test_taehv_chain_host.py MUTANTS).
WIRING = dict(
    cat_order=("x", "past"),                        # MemBlock: conv(cat([x, past], 1)): x is the FIRST half of the K axis
    past_offset=1,                                  # past_t = the block's input ONE frame earlier
    memory_from=-1,                                 # the memory after a call is the call's LAST frame
    initial_memory=0.0,                             # before the video starts the memory is zeros
    tgrow_block=lambda S, j: j,                     # TGrow: frame S t + j is channel block j of the 1x1 conv's output for frame t
    tgrow_rows="last",                              # a TGrow weight with more rows than channels * stride keeps its LAST rows
    tpool_pair=lambda t: (2 * t, 2 * t + 1),        # TPool(2): output frame t pools the input frames 2t and 2t + 1 ...
    tpool_order=(0, 1),                             # ... frame 2t on the FIRST half of the 1x1 conv's K axis
    relu_after_in=True,                             # ReLU after decoder.1 and after encoder.0
    relu_after_level=lambda half, lvl: half == "decoder" and lvl == 2,   # no ReLU after a level-change conv, except in front of the decoder head
    level_bias=lambda key: None,                    # TGrow, TPool and the level-change convs have no bias
    clamp=("decoder",),                             # Clamp tanh(z / 3) * 3 on the decoder's input only
)


def rbf(x: torch.Tensor) -> torch.Tensor:
    """-> the nearest bf16 value (ties to even; inf and NaN kept), in x's dtype."""
    return x.to(torch.float32).to(BF).to(x.dtype) if x.dtype == torch.float32 else _rbf64(x)


def _rbf64(x):
    m, e = torch.frexp(x)
    r = torch.ldexp(torch.round(m * 256.0) / 256.0, e)
    return torch.where(torch.isfinite(x), r, x)


class _Conv:
    """One convolution's operands.  W: [N, ntaps * Cin] tap-major with Cin contiguous (what TaehvRefOps reads); Wfrag: its
    fragment-major packing (what the kernels read); N: channels stored per pixel; Nw: rows of the packed matrix."""

    def __init__(self, name, W, Wfrag, bias, N, Nw, Cin, ntaps):
        self.name, self.W, self.Wfrag, self.bias, self.N, self.Nw, self.Cin, self.ntaps = name, W, Wfrag, bias, N, Nw, Cin, ntaps


# ====================================================================================================== backends
class TaehvRefOps:
    """Every op as its documented contract (include/mmpl_hip.h), in plain torch on the CPU.  Frames are channels-last and padded."""

    def __init__(self, dtype=torch.float64, round: bool = False):
        self.dtype, self.round = dtype, round

    def _r(self, x):
        return rbf(x) if self.round else x

    def frames(self, T, H, W, C_, zero=False):
        v = torch.zeros((T, H + 2, W + 2, C_), dtype=self.dtype)
        if not zero:
            v[:, 1:-1, 1:-1, :] = float("nan")
        return v

    def out(self, shape, kind):
        if kind == "u8":
            return torch.full(tuple(shape), 0xA5, dtype=torch.uint8)
        return torch.full(tuple(shape), float("nan"), dtype=self.dtype)

    def param(self, t):
        return t.detach().to("cpu").to(self.dtype).contiguous()

    def latents(self, z):
        return self._r(z.detach().to("cpu").to(self.dtype))

    def pixels(self, px):
        return px.detach().to("cpu").contiguous() if px.dtype == torch.uint8 else px.detach().to("cpu").to(self.dtype).contiguous()

    def finish(self):
        pass

    def canaries_intact(self) -> bool:
        return True

    def _epilogue(self, y, cv, relu, skip=None):
        """[T, N, Ho, Wo] accumulators -> relu?(acc + bias? + skip?) rounded once, channels-last"""
        if cv.bias is not None:
            y = y + cv.bias.view(1, -1, 1, 1)
        if skip is not None:
            y = y + skip[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)
        if relu:
            y = y.clamp_min(0.0)
        return self._r(y).permute(0, 2, 3, 1)

    def conv(self, cv, dst, src0, src1=None, relu=False, skip=None):
        x = src0 if src1 is None else torch.cat([src0, src1], dim=-1)
        assert x.shape[-1] == cv.Cin, (cv.name, x.shape, cv.Cin)
        x = x.permute(0, 3, 1, 2)
        if cv.ntaps == 9:
            w = cv.W.view(cv.N, 3, 3, cv.Cin).permute(0, 3, 1, 2)
        else:
            w, x = cv.W.view(cv.N, cv.Cin, 1, 1), x[:, :, 1:-1, 1:-1]
        dst[:, 1:-1, 1:-1, :cv.N] = self._epilogue(F.conv2d(x, w), cv, relu, skip)

    def conv_s2(self, cv, dst, src, relu=False):
        w = cv.W.view(cv.N, 3, 3, cv.Cin).permute(0, 3, 1, 2)
        dst[:, 1:-1, 1:-1, :] = self._epilogue(F.conv2d(src.permute(0, 3, 1, 2), w, stride=2), cv, relu)

    def conv_in(self, cv, dst, px, relu=True):
        if px.dtype == torch.uint8:
            x = (px.to(torch.float32) / 255.0 if self.round else px.to(self.dtype) / 255.0).to(self.dtype).permute(0, 3, 1, 2)
        else:
            x = px
        w = cv.W[:, :27].view(cv.N, 3, 3, 3).permute(0, 3, 1, 2)              # column k = (3 ky + kx) * 3 + c
        dst[:, 1:-1, 1:-1, :] = self._epilogue(F.conv2d(self._r(x), w, padding=1), cv, relu)

    def prep(self, dst, z, clamp=True):
        """z [16, h, w] -> channels [0, 16) of the interior of dst [h + 2, w + 2, 32]"""
        v = torch.tanh(z / 3.0) * 3.0 if clamp else z
        dst[1:-1, 1:-1, :16] = self._r(v).permute(1, 2, 0)

    def px_out(self, out, src, fmt, t_out):
        T = src.shape[0]
        v = src[:, 1:-1, 1:-1, :3]
        if fmt == 0:
            out[t_out:t_out + T] = v.permute(0, 3, 1, 2)
        else:
            out[t_out:t_out + T] = (v.to(torch.float32).clamp(0, 1) * 255.0).to(torch.uint8)

    def z_out(self, out, src, f_out):
        T = src.shape[0]
        out[f_out:f_out + T] = src[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)

    def upsample(self, dst, src):
        dst[:, 1:-1, 1:-1, :] = src[:, 1:-1, 1:-1, :].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

    def copy(self, dst, src):
        dst.copy_(src)

    def fill(self, frame, value):
        frame[1:-1, 1:-1, :] = value


class TaehvHipOps:
    """Every op is one call of the matching single-launch entry of libmmpl_hip.so on the current stream of `device`."""

    def __init__(self, lib, device="cuda:0"):
        from mmpl_amd import _lib
        self.lib, self._lib, self.device = lib, _lib, torch.device(device)
        self.buffers, self.payload = [], []
        self.launches = 0

    # ---- buffers
    def _new(self, n16):
        b = torch.full((n16 + TAIL,), CANARY, dtype=torch.int16, device=self.device)
        self.buffers.append(b)
        self.payload.append(n16)
        return b[:n16]

    def frames(self, T, H, W, C_, zero=False):
        v = self._new(T * (H + 2) * (W + 2) * C_).view(BF).view(T, H + 2, W + 2, C_)
        if zero:
            v.zero_()
        else:                                               # the zero border; the interior keeps the NaN pattern
            v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 0, 0, 0, 0
        return v

    def out(self, shape, kind):
        dtype, size = {"bf16": (BF, 2), "f32": (torch.float32, 4), "u8": (torch.uint8, 1)}[kind]
        nbytes = math.prod(shape) * size
        assert nbytes % 2 == 0
        return self._new(nbytes // 2).view(dtype).view(tuple(shape))

    def param(self, t):
        return t.detach().to(device=self.device, dtype=BF).contiguous()

    def latents(self, z):
        return z.detach().to(device=self.device, dtype=BF).contiguous()

    def pixels(self, px):
        return px.detach().to(device=self.device, dtype=torch.uint8 if px.dtype == torch.uint8 else torch.float32).contiguous()

    def finish(self):
        torch.cuda.synchronize(self.device)

    def canaries_intact(self) -> bool:
        torch.cuda.synchronize(self.device)
        return all(bool((b[n:] == CANARY).all()) for b, n in zip(self.buffers, self.payload))

    # ---- helpers
    def _p(self, t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, rc, what):
        self.launches += 1
        self._lib.check(rc, what)

    @staticmethod
    def _run(v):
        """A run of frames: every frame contiguous -> its frame stride in elements."""
        assert v.dim() == 4 and v[0].is_contiguous()
        return v.stride(0) if v.shape[0] > 1 else v[0].numel()

    # ---- ops
    def conv(self, cv, dst, src0, src1=None, relu=False, skip=None):
        T, Hp, Wp, C0 = src0.shape
        C1 = 0 if src1 is None else src1.shape[3]
        assert C0 + C1 == cv.Cin and dst.shape[:3] == (T, Hp, Wp) and (src1 is None or src1.shape[:3] == (T, Hp, Wp))
        assert skip is None or tuple(skip.shape) == (T, Hp, Wp, cv.Nw)
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_conv(
                self._p(src0), self._p(src1), self._run(src0), 0 if src1 is None else self._run(src1), C0, C1, 0, cv.ntaps,
                self._p(cv.Wfrag), self._p(cv.bias), cv.Nw, cv.N, T, Hp - 2, Wp - 2, self._p(dst), self._run(dst), dst.shape[3],
                cv.Nw, int(relu), self._p(skip), 0 if skip is None else self._run(skip), None, self._stream()), "conv " + cv.name)

    def conv_s2(self, cv, dst, src, relu=False):
        assert cv.bias is None, "taehv_conv_s2_kernel has no bias"
        T, Hp, Wp, Cin = src.shape
        Ho, Wo = dst.shape[1] - 2, dst.shape[2] - 2
        assert Cin == cv.Cin and (Hp, Wp) == (2 * Ho + 2, 2 * Wo + 2) and dst.shape[0] == T and dst.shape[3] == cv.Nw
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_conv_s2(self._p(src), self._run(src), Cin, self._p(cv.Wfrag), cv.Nw, T, Ho, Wo, self._p(dst),
                                                   self._run(dst), int(relu), self._stream()), "conv_s2 " + cv.name)

    def conv_in(self, cv, dst, px, relu=True):
        assert relu, "taehv_conv_in_kernel always applies the ReLU"
        u8 = px.dtype == torch.uint8
        T, H, W = (px.shape[0], px.shape[1], px.shape[2]) if u8 else (px.shape[0], px.shape[2], px.shape[3])
        assert tuple(dst.shape) == (T, H + 2, W + 2, 64) and px.is_contiguous()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_conv_in(self._p(px), int(u8), self._p(cv.Wfrag), self._p(cv.bias), T, H, W, self._p(dst),
                                                   self._run(dst), self._stream()), "conv_in")

    def prep(self, dst, z, clamp=True):
        assert clamp, "taehv_prep_kernel always applies the Clamp"
        _, h, w = z.shape
        assert tuple(dst.shape) == (h + 2, w + 2, 32) and dst.is_contiguous() and z.is_contiguous()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_prep(self._p(z), self._p(dst), h, w, self._stream()), "prep")

    def px_out(self, out, src, fmt, t_out):
        T, Hp, Wp, c4 = src.shape
        assert c4 == 4 and src.is_contiguous()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_px_out(self._p(src), self._p(out), fmt, T, Hp - 2, Wp - 2, t_out, self._stream()), "px_out")

    def z_out(self, out, src, f_out):
        T, hp, wp, c16 = src.shape
        assert c16 == 16 and src.is_contiguous()
        with torch.cuda.device(self.device):
            self._call(self.lib.mmpl_taehv_z_out(self._p(src), self._p(out), T, hp - 2, wp - 2, f_out, self._stream()), "z_out")

    def upsample(self, dst, src):
        dst[:, 1:-1, 1:-1, :] = src[:, 1:-1, 1:-1, :].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

    def copy(self, dst, src):
        assert dst.shape == src.shape
        dst.copy_(src)

    def fill(self, frame, value):
        frame[1:-1, 1:-1, :] = value


# ====================================================================================================== the chain
class TaehvChain:
    """decode(z [T, 16, h, w], fmt) -> 4T frames (fmt 0: float [4T, 3, 8h, 8w]; 1: uint8 [4T, 8h, 8w, 3]); encode(px [T, 3, 8h, 8w]
    float in [0, 1] or uint8 [T, 8h, 8w, 3], T % 4 == 0) -> [T / 4, 16, h, w].  Both CONTINUE the current video, each half with
    memories of its own; reset() starts a new one."""

    def __init__(self, sd, lat_h: int, lat_w: int, ops, wiring: Optional[dict] = None):
        self.sd, self.h, self.w, self.ops = sd, lat_h, lat_w, ops
        self.wr = dict(WIRING)
        self.wr.update(wiring or {})
        self._cv: Dict[str, _Conv] = {}
        self.mem: Dict[tuple, torch.Tensor] = {}

    def reset(self):
        self.mem = {}

    # ---- parameters, packed here
    def _make(self, name, w, bias, ntaps):
        """w [N, Cin, k, k] (k * k == ntaps), bias [N] or None -> _Conv: Cin padded to 32, rows padded to 16 in the fragments only"""
        W2 = pack_conv(w)
        cin = W2.shape[1] // ntaps
        n = w.shape[0]
        ops = self.ops
        return _Conv(name, ops.param(W2), ops.param(pack_frag(W2, cin)), None if bias is None else ops.param(bias.reshape(-1)), n,
                     (n + 15) // 16 * 16, cin, ntaps)

    def cv(self, name: str, ntaps=9, bias=True) -> _Conv:
        """A 3x3 or 1x1 conv of the state dict under its own key.  bias=False: the layer has none (WIRING level_bias may add one)."""
        if name not in self._cv:
            w = self.sd[name + ".weight"]
            bkey = name + ".bias" if bias else self.wr["level_bias"](name)
            b = None if bkey is None else self.sd[bkey]
            if name == "decoder.22":                          # three output channels, stored as four; the bias padded to 4
                w, b = torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))]), torch.cat([b, b.new_zeros(1)])
            self._cv[name] = self._make(name, w, b, ntaps)
        return self._cv[name]

    def cv_in(self) -> _Conv:
        """encoder.0: the packed matrix [64, 32], column k = (3 ky + kx) * 3 + c, columns 27 .. 31 zero, ONE chunk with ntaps = 1"""
        if "encoder.0" not in self._cv:
            w = self.sd["encoder.0.weight"]
            W2 = F.pad(w.permute(0, 2, 3, 1).reshape(w.shape[0], 27), (0, 5))
            ops = self.ops
            self._cv["encoder.0"] = _Conv("encoder.0", ops.param(W2), ops.param(pack_frag(W2, 32)), ops.param(self.sd["encoder.0.bias"]),
                                          w.shape[0], w.shape[0], 32, 1)
        return self._cv["encoder.0"]

    def cv_tgrow(self, name: str, C_: int, S: int, j: int) -> _Conv:
        """The rows of TGrow's 1x1 conv (the kept channels * stride rows of it) that make frame S t + j"""
        key = f"{name}#{j}"
        if key not in self._cv:
            w = self.sd[name + ".weight"]
            rows = C_ * S
            w = w[-rows:] if self.wr["tgrow_rows"] == "last" else w[:rows]
            k = self.wr["tgrow_block"](S, j)
            bkey = self.wr["level_bias"](name)
            self._cv[key] = self._make(key, w[k * C_:(k + 1) * C_], None if bkey is None else self.sd[bkey], 1)
        return self._cv[key]

    # ---- pieces
    def _memblock(self, half, i, x):
        """MemBlock (taehv.py): ReLU(conv(ReLU(conv(ReLU(conv(cat([x, past], 1)))))) + x), past = the input one frame earlier."""
        ops, wr = self.ops, self.wr
        T, Hp, Wp, C_ = x.shape
        H, W = Hp - 2, Wp - 2
        mem = self.mem.get((half, i))
        if mem is None:
            mem = ops.frames(1, H, W, C_, zero=True)
            if wr["initial_memory"] != 0.0:
                ops.fill(mem[0], wr["initial_memory"])
        past = ops.frames(T, H, W, C_)
        for t in range(T):
            s = t - wr["past_offset"]
            ops.copy(past[t], x[s] if s >= 0 else mem[0])
        new_mem = ops.frames(1, H, W, C_)
        ops.copy(new_mem[0], x[wr["memory_from"]])
        self.mem[(half, i)] = new_mem
        s0, s1 = (x, past) if wr["cat_order"] == ("x", "past") else (past, x)
        pre = f"{half}.{i}.conv."
        t1 = ops.frames(T, H, W, C_)
        ops.conv(self.cv(pre + "0"), t1, s0, s1, relu=True)
        t2 = ops.frames(T, H, W, C_)
        ops.conv(self.cv(pre + "2"), t2, t1, relu=True)
        y = ops.frames(T, H, W, C_)
        ops.conv(self.cv(pre + "4"), y, t2, relu=True, skip=x)
        return y

    # ---- the products
    def decode(self, z, fmt: int = 0):
        ops, wr, h, w = self.ops, self.wr, self.h, self.w
        z = ops.latents(z)
        T = z.shape[0]
        assert T >= 1 and tuple(z.shape[1:]) == (16, h, w)
        zin = ops.frames(T, h, w, 32, zero=True)              # Cin 16 padded to 32 with zeros
        for t in range(T):
            ops.prep(zin[t], z[t], clamp="decoder" in wr["clamp"])
        H, W = h, w
        x = ops.frames(T, H, W, DEC_CH[0])
        ops.conv(self.cv("decoder.1"), x, zin, relu=wr["relu_after_in"])
        i = 3
        for lvl in range(3):
            C_, S, Cn = DEC_CH[lvl], GROW[lvl], DEC_CH[lvl + 1]
            for _ in range(3):
                x = self._memblock("decoder", i, x)
                i += 1
            up = ops.frames(T, 2 * H, 2 * W, C_)              # decoder.{i}: Upsample(scale_factor=2), nearest
            ops.upsample(up, x)
            H, W = 2 * H, 2 * W
            grown = ops.frames(T * S, H, W, C_)               # decoder.{i + 1}: TGrow
            for j in range(S):
                ops.conv(self.cv_tgrow(f"decoder.{i + 1}.conv", C_, S, j), grown[j::S], up)
            T *= S
            x = ops.frames(T, H, W, Cn)                       # decoder.{i + 2}: conv C -> Cn, no bias
            ops.conv(self.cv(f"decoder.{i + 2}", bias=False), x, grown, relu=wr["relu_after_level"]("decoder", lvl))
            i += 3
        head = ops.frames(T, H, W, 4)
        ops.conv(self.cv("decoder.22"), head, x)
        out = ops.out((T, H, W, 3), "u8") if fmt == 1 else ops.out((T, 3, H, W), "f32")
        ops.px_out(out, head, fmt, 0)
        ops.finish()
        return out

    def encode(self, px):
        ops, wr = self.ops, self.wr
        px = ops.pixels(px)
        u8 = px.dtype == torch.uint8
        T = px.shape[0]
        H, W = 8 * self.h, 8 * self.w
        assert T >= 4 and T % 4 == 0 and tuple(px.shape[1:]) == ((H, W, 3) if u8 else (3, H, W))
        if "encoder" in wr["clamp"]:
            px = torch.tanh(px / 3.0) * 3.0
        x = ops.frames(T, H, W, ENC_C)
        ops.conv_in(self.cv_in(), x, px, relu=wr["relu_after_in"])
        i = 2
        for lvl, S in enumerate(POOL):
            name = f"encoder.{i}.conv"                        # TPool(S)
            if S == 2:
                T //= 2
                runs = [ops.frames(T, H, W, ENC_C), ops.frames(T, H, W, ENC_C)]
                for t in range(T):
                    pair = wr["tpool_pair"](t)
                    for r in range(2):
                        ops.copy(runs[r][t], x[pair[r]])
                s0, s1 = runs[wr["tpool_order"][0]], runs[wr["tpool_order"][1]]
            else:
                s0, s1 = x, None
            pooled = ops.frames(T, H, W, ENC_C)
            ops.conv(self.cv(name, ntaps=1, bias=False), pooled, s0, s1)
            H, W = H // 2, W // 2
            x = ops.frames(T, H, W, ENC_C)                    # encoder.{i + 1}: conv stride 2, no bias
            ops.conv_s2(self.cv(f"encoder.{i + 1}", bias=False), x, pooled, relu=wr["relu_after_level"]("encoder", lvl))
            i += 2
            for _ in range(3):
                x = self._memblock("encoder", i, x)
                i += 1
        head = ops.frames(T, H, W, 16)
        ops.conv(self.cv("encoder.17"), head, x)
        out = ops.out((T, 16, H, W), "bf16")
        ops.z_out(out, head, 0)
        ops.finish()
        return out
