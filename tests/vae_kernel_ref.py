"""Float64 references, layout builders and the case tables of the per-launch VAE / TAEHV kernel tests
(tests/test_vae_kernels_gpu.py, tests/test_taehv_kernels_gpu.py; self-test: tests/test_vae_kernel_ref.py).  CPU only.

Activations start as plain NCDHW float64 tensors and weights as plain [N, Cin, (kt,) kh, kw] tensors; the kernels' operands are
made from them by the builders below and by the PRODUCT's packers (VaeEngine._repack / _frag_pack, TaehvEngine._repack), so
the packers are under test with the kernels.  The convolution itself is torch.nn.functional.conv3d / conv2d in float64 over an
explicitly zero-padded input.  bf16 round-to-nearest-even is applied exactly where the kernel comments say:

  VAE conv    bf16(acc + bias); with a residual bf16(that + res); on the fused path the norm chain of norm_act_pad_kernel follows
  RMS norm    d = max(bf16(||x||), 1e-12); bf16(x / d); bf16(* sqrt(C)); bf16(* gamma); [bf16(silu)]
  TAEHV conv  bf16(relu(acc + bias + skip)), nothing rounded in between

Exact regime: integer-valued operands with sum|a||w| + |bias| + |res| < 2^24 for every output element (assert_exact_regime), so
every fp32 product and partial sum is exact in any order and the kernel must match bit for bit.
Near-tie rule (the transcendental / division passes): an element of the reference is AMBIGUOUS where a value it was rounded from
lies within a relative 2^-18 of a bf16 rounding midpoint (2^-20 for a pixel's norm); only there may the kernel differ, by one
bf16 ulp.  2^-18 is about 8x the documented error of __expf / __fdividef / tanhf and of the fp32 rounding in front of the bf16 one;
where the kernel's value is a single correctly rounded fp32 operation (the norm's quotient and its * sqrt(C)) the window is 2^-23.
A single fp32 add or multiply of two bf16 values (z_prep's + mean, mu_out's - mean and * inv_std) is narrower still: a value
exactly ON a midpoint is representable in fp32, the operation delivers it exactly and round-to-nearest-even decides it the same way
in the kernel and here, so only the open window 0 < distance <= 2^-23 is ambiguous there (near_tie(..., exact_ok=True)).
The ambiguous set must stay under 1 % of the elements in every case: tests/test_vae_kernel_ref.py asserts it from these references.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from mmpl_amd.taehv import TaehvEngine
from mmpl_amd.vae import VaeEngine

F64 = torch.float64
EXACT_LIMIT = float(2 ** 24)
SENTINEL = -24576.0              # -3 * 2^13: exact in bf16
TIE_REL, TIE_REL_NORM = 2.0 ** -18, 2.0 ** -20
TIE_REL_FP32 = 2.0 ** -23        # in front of the bf16 rounding stands ONE correctly rounded fp32 operation (2^-24), factor 2 to spare
K_IGEMM3, K_IGEMM4, K_HALO6, K_HALO1 = 1, 2, 3, 4      # mmpl_vae_conv's kernel_out


# ------------------------------------------------------------------------------------------------ bf16 arithmetic in float64
def rbf(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 value (ties to even), as float64."""
    m, e = torch.frexp(x.to(F64))
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def near_tie(x: torch.Tensor, rel: float = TIE_REL, mag: Optional[torch.Tensor] = None, exact_ok: bool = False) -> torch.Tensor:
    """True where x lies within rel * |x| (or rel * mag) of a bf16 rounding midpoint.  exact_ok: a value exactly on a midpoint is NOT
    ambiguous (x is the float64 result of one fp32 operation that delivers a midpoint exactly; ties-to-even then decides it)."""
    x = x.to(F64)
    m, e = torch.frexp(x.abs())
    t = m * 256.0                                        # in [128, 256): the midpoints are the half-integers
    dist = torch.ldexp(((t - torch.floor(t)) - 0.5).abs() / 256.0, e)      # every step exact in float64: 0 iff x is a midpoint
    near = dist <= rel * (x.abs() if mag is None else mag)
    return near & (dist > 0) if exact_ok else near


def bf16_exact(x: torch.Tensor) -> torch.Tensor:
    """float64 values that ARE bf16 values -> a bf16 tensor (asserts nothing is lost)."""
    b = x.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(b.to(F64), x.to(F64)), "value not representable in bf16"
    return b


def bf16_line(t: torch.Tensor) -> torch.Tensor:
    """bf16 tensor -> its bit patterns on a monotone integer line (one step = one ulp; -0 and +0 coincide)."""
    i = t.contiguous().view(torch.int16).to(torch.int32) & 0xffff
    return torch.where(i >= 0x8000, -(i & 0x7fff), i)


def check_near_tie(got: torch.Tensor, ref: torch.Tensor, amb: torch.Tensor, what: str = "") -> None:
    """The near-tie rule: got == ref bit for bit outside amb, within one ulp inside."""
    d = (bf16_line(got) - bf16_line(ref)).abs()
    bad = (d > 0) & ~amb
    assert not bad.any(), f"{what}: {int(bad.sum())} of {d.numel()} unambiguous elements differ (max {int(d[~amb].max())} ulp)"
    assert int(d.max()) <= 1, f"{what}: an ambiguous element differs by {int(d.max())} ulp"


def _rng(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, shape, lim: int) -> torch.Tensor:
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def _gauss_bf16(g, shape, std: float = 1.0) -> torch.Tensor:
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------------------------------------ layouts
def to_cl(x: torch.Tensor) -> torch.Tensor:
    """NCDHW float64 [1, C, T, H, W] -> channels-last bf16 [T, H, W, C]."""
    return bf16_exact(x[0].permute(1, 2, 3, 0).contiguous())


def from_cl(v: torch.Tensor) -> torch.Tensor:
    """channels-last [T, H, W, C] -> NCDHW float64 [1, C, T, H, W]."""
    return v.to(F64).permute(3, 0, 1, 2).unsqueeze(0).contiguous()


def embed(v: torch.Tensor, Td: int, Hd: int, Wd: int, ldd: int, dt0: int = 0, dy0: int = 0, dx0: int = 0,
          fill: float = SENTINEL) -> torch.Tensor:
    """channels-last [T, H, W, C] -> a volume [Td, Hd, Wd, ldd] of `fill` holding v at (dt0, dy0, dx0), channels [0, C)."""
    T, H, W, C = v.shape
    out = torch.full((Td, Hd, Wd, ldd), fill, dtype=torch.bfloat16)
    out[dt0:dt0 + T, dy0:dy0 + H, dx0:dx0 + W, :C] = v
    return out


def extract(vol: torch.Tensor, T: int, H: int, W: int, C: int, dt0: int = 0, dy0: int = 0, dx0: int = 0) -> torch.Tensor:
    return vol[dt0:dt0 + T, dy0:dy0 + H, dx0:dx0 + W, :C].contiguous()


def outside_is(vol: torch.Tensor, T: int, H: int, W: int, C: int, dt0: int = 0, dy0: int = 0, dx0: int = 0,
               fill: float = SENTINEL) -> bool:
    """Does everything of vol outside the block [dt0.., dy0.., dx0.., 0..C) still hold `fill`?"""
    own = torch.zeros(vol.shape, dtype=torch.bool)
    own[dt0:dt0 + T, dy0:dy0 + H, dx0:dx0 + W, :C] = True
    return bool((vol[~own].to(F64) == fill).all())


def ring_slots(Tp: int, base: int, n: int):
    """Slot of logical frame j of a ring of Tp frame slots that stands at `base` (vae.hip cached_conv3)."""
    return [(base + j) % Tp for j in range(n)]


def to_ring(frames: torch.Tensor, Tp: int, base: int, fill: float = SENTINEL) -> torch.Tensor:
    """[n, ...] logical frames -> [Tp, ...] slots, frame j in slot (base + j) % Tp, the other slots = fill."""
    out = torch.full((Tp,) + tuple(frames.shape[1:]), fill, dtype=frames.dtype)
    for j, s in enumerate(ring_slots(Tp, base, frames.shape[0])):
        out[s] = frames[j]
    return out


def from_ring(ring: torch.Tensor, base: int, n: int) -> torch.Tensor:
    return torch.stack([ring[s] for s in ring_slots(ring.shape[0], base, n)])


def to_plain(x: torch.Tensor, ld: Optional[int] = None, fill: float = SENTINEL) -> torch.Tensor:
    """NCDHW [1, C, T, H, W] -> plain bf16 [T * H * W, ld] (columns past C = fill)."""
    v = to_cl(x)
    C = v.shape[-1]
    v = v.reshape(-1, C)
    if ld is None or ld == C:
        return v
    out = torch.full((v.shape[0], ld), fill, dtype=torch.bfloat16)
    out[:, :C] = v
    return out


# ------------------------------------------------------------------------------------------------ references
def assert_exact_regime(xp: torch.Tensor, w: torch.Tensor, bias=None, extra=None, stride=1) -> float:
    """xp: the zero-padded input, w the weights (conv3d / conv2d by rank).  Asserts integer operands and
    max(sum|a||w| + |bias| + |extra|) < 2^24; returns that maximum."""
    for t in (xp, w, bias, extra):
        if t is not None:
            assert torch.equal(t, torch.round(t)), "exact regime: operands must be integers"
    conv = F.conv3d if w.dim() == 5 else F.conv2d
    s = conv(xp.abs(), w.abs(), None, stride=stride)
    if bias is not None:
        s = s + bias.abs().view((1, -1) + (1,) * (s.dim() - 2))
    if extra is not None:
        s = s + extra.abs()
    m = float(s.max())
    assert m < EXACT_LIMIT, f"exact regime violated: {m} >= 2^24"
    return m


def vae_conv_ref(xp, w, bias, stride=(1, 1, 1), res=None):
    """xp [1, Cin, Tp, Hp, Wp] (already padded), w [N, Cin, kt, kh, kw], bias [N], res [1, N, To, Ho, Wo] or None ->
    (bf16(acc + bias) [then bf16(+ res)], acc), NCDHW float64."""
    acc = F.conv3d(xp, w, None, stride=stride)
    y = rbf(acc + bias.view(1, -1, 1, 1, 1))
    if res is not None:
        y = rbf(y + res)
    return y, acc


def rms_norm_ref(x: torch.Tensor, gamma: Optional[torch.Tensor], silu: bool):
    """norm_act_pad_kernel on x [..., C] (bf16 values in float64).  Returns (reference, ambiguous mask)."""
    if gamma is None:
        return x.clone(), torch.zeros_like(x, dtype=torch.bool)
    C = x.shape[-1]
    scale = float(torch.sqrt(torch.tensor(float(C), dtype=torch.float32)))          # the kernel's fp32 sqrtf(C)
    nrm = torch.sqrt((x * x).sum(-1, keepdim=True))
    amb = near_tie(nrm, TIE_REL_NORM).expand_as(x).clone()
    d = rbf(nrm).clamp_min(1e-12)
    # x / d and * sqrt(C): the kernel forms the correctly rounded fp32 quotient (its own comment) and one fp32 product, so these two
    # are ambiguous only within 2^-23 of a midpoint -- narrower than the general 2^-18, which the SiLU (__expf, __fdividef) needs
    for step in (lambda v: v / d, lambda v: v * scale):
        v = step(x)
        amb |= near_tie(v, TIE_REL_FP32)
        x = rbf(v)
    x = rbf(x * gamma)                                   # a product of two bf16 values is exact in fp32: no ambiguity
    if silu:
        v = x / (1.0 + torch.exp(-x))
        amb |= near_tie(v)
        x = rbf(v)
    return x, amb


def softmax_ref(s: torch.Tensor) -> torch.Tensor:
    return torch.softmax(s.to(F64), dim=-1)


def zprep_ref(z, mean, inv_std, w2, b2):
    """z [F, 16, h, w], mean / inv_std [16], w2 [16, 16], b2 [16] (float64) -> ([F, h, w, 16], ambiguous).  A near tie in the
    rounding of one latent channel makes the whole pixel ambiguous (every output reads every channel): the quotient z / inv_std within
    the general 2^-18, the sum + mean -- one fp32 add of two bf16 values -- only in the open 2^-23 window (an exact midpoint is decided
    by ties-to-even).  The 16-term fp32 dot product must be exact for the inputs (asserted): every term a multiple of 2^-10, the sum
    of magnitudes below 2^13, so the last rounding is unambiguous."""
    v = z.permute(0, 2, 3, 1)
    q = v / inv_std
    amb = near_tie(q).any(-1, keepdim=True)
    q = rbf(q)
    amb = amb | near_tie(q + mean, TIE_REL_FP32, exact_ok=True).any(-1, keepdim=True)
    zz = rbf(q + mean)
    acc = zz @ w2.t() + b2
    mag = zz.abs() @ w2.abs().t() + b2.abs()
    assert torch.equal(zz * 1024, torch.round(zz * 1024)) and torch.equal(w2, torch.round(w2)) and torch.equal(b2, torch.round(b2))
    assert float(mag.max()) < 2 ** 13, "z_prep: the dot product must be exact in fp32"
    return rbf(acc), amb.expand_as(acc).clone()


def mu_out_ref(enc, w1, b1, mean, inv_std):
    """enc [F, h, w, 32], w1 [32, 32], b1 [32] -> ([F, 16, h, w] bf16-valued float64, ambiguous).  Integer enc / w1 / b1 in the
    exact regime (asserted): the dot product is exact, the two scalings behind it are single fp32 operations on bf16 values -- ambiguous
    only in the open 2^-23 window, an exact midpoint is decided by ties-to-even."""
    for t in (enc, w1, b1):
        assert torch.equal(t, torch.round(t))
    assert float((enc.abs() @ w1[:16].abs().t() + b1[:16].abs()).max()) < EXACT_LIMIT
    mu = rbf(enc @ w1[:16].t() + b1[:16])
    d = mu - mean
    amb = near_tie(d, TIE_REL_FP32, exact_ok=True)
    d = rbf(d)
    amb |= near_tie(d * inv_std, TIE_REL_FP32, exact_ok=True)
    return rbf(d * inv_std).permute(0, 3, 1, 2).contiguous(), amb.permute(0, 3, 1, 2).contiguous()


def px_in_ref(px: torch.Tensor, t0: int, T: int) -> torch.Tensor:
    """px_in_kernel: px [3, Ttot, H, W] -> channels-last [T, H, W, 3], frames t0 .. t0 + T - 1, a copy."""
    return px[:, t0:t0 + T].permute(1, 2, 3, 0).contiguous()


def px_out_ref(src: torch.Tensor) -> torch.Tensor:
    """px_out_kernel: src bf16 [T, H, W, 4] -> float32 [T, 3, H, W], clamp(-1, 1) of the bf16 value; channel 3 is dropped."""
    return src[..., :3].to(torch.float32).clamp(-1.0, 1.0).permute(0, 3, 1, 2).contiguous()


def px_out_u8_ref(src: torch.Tensor) -> torch.Tensor:
    """px_out_u8_kernel: src bf16 [T, H, W, 4] -> uint8 [T, H, W, 3]: PyTorch's own float32 evaluation, on the CPU, of what the
    pipeline and the CLI do to a decoded frame (the expression the kernel's comment cites).  NaN inputs have no defined uint8 here:
    the caller masks them (nan_bf16)."""
    x = src[..., :3].to(torch.float32)
    v = (x.clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1)
    return (v * 255.0).clamp(0, 255).to(torch.uint8)


def all_bf16_patterns(mult: int = 1, add: int = 0) -> torch.Tensor:
    """All 65 536 bf16 bit patterns as a bf16 tensor, pattern (i * mult + add) mod 2^16 at index i (mult odd: a permutation)."""
    assert mult % 2 == 1
    i = (torch.arange(65536, dtype=torch.int64) * mult + add) & 0xffff
    return torch.where(i >= 0x8000, i - 0x10000, i).to(torch.int16).view(torch.bfloat16)


def taehv_prep_ref(z):
    """z [16, h, w] -> ([h, w, 16], ambiguous)."""
    v = torch.tanh(z / 3.0) * 3.0
    v = v.permute(1, 2, 0)
    return rbf(v), near_tie(v)


def taehv_conv_ref(x0, x1, w, bias, skip, relu: bool, up: bool):
    """x0 [T, C0, Hs, Ws], x1 [T, C1, Hs, Ws] or None (the frames each output frame reads), w [Nw, C0 + C1, k, k], bias [Nw] or None,
    skip [T, Nw, Ho, Wo] or None -> (bf16(relu(acc + bias + skip)) [T, Nw, Ho, Wo], padded input)."""
    x = x0 if x1 is None else torch.cat([x0, x1], dim=1)
    if up:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)              # nearest x2
    if w.shape[-1] == 3:
        x = F.pad(x, (1, 1, 1, 1))
    y = F.conv2d(x, w, None)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if skip is not None:
        y = y + skip
    if relu:
        y = y.clamp_min(0.0)
    return rbf(y), x


def accum_bound(xp, w, stride=1) -> torch.Tensor:
    """K * 2^-24 * (|A| * |W|): the standard worst-case bound of an fp32 accumulation of K = ntaps * Cin products."""
    conv = F.conv3d if w.dim() == 5 else F.conv2d
    K = w[0].numel()
    return K * 2.0 ** -24 * conv(xp.abs(), w.abs(), None, stride=stride)


# ------------------------------------------------------------------------------------------------ VAE conv cases
@dataclass(frozen=True)
class ConvCase:
    name: str
    kernel: int                       # the kernel vae_launch_conv must pick
    Cin: int
    N: int
    k: Tuple[int, int, int]
    s: Tuple[int, int, int]
    To: int
    Ho: int
    Wo: int
    regime: str = "act8"              # act8: activations +-255, weights -2..2 | w8: the roles swapped | small | gauss
    ring: Optional[Tuple[int, int]] = None     # (Tp, base): the source frames live in ring slots
    frag: bool = True                 # hand the kernel the fragment-packed weights
    res: bool = False
    fuse: Optional[Tuple[int, int, bool]] = None   # (Tp, base, dst given) of the consumer's ring: the fused norm epilogue
    cin_live: Optional[int] = None    # input channels that carry data (3 / 16 of 32)
    head: bool = False                # decoder.head.2: 3 output channels padded to 4 by _repack
    offset: bool = False              # write into an offset window of a larger, wider destination
    zero_front: bool = False          # the kt - 1 leading frames are the causal zero padding (a video's first chunk)


S1, S2 = (1, 1, 1), (1, 2, 2)
CONV_CASES = [
    # conv_halo_kernel<6>
    ConvCase("halo6_lin_96", K_HALO6, 96, 96, (3, 3, 3), S1, 2, 6, 10, zero_front=True),
    ConvCase("halo6_ring_192", K_HALO6, 192, 192, (3, 3, 3), S1, 4, 9, 33, "w8", ring=(6, 4)),
    ConvCase("halo6_ring_384", K_HALO6, 384, 384, (3, 3, 3), S1, 4, 6, 10, ring=(6, 4), res=True),
    ConvCase("halo6_k1_384_192", K_HALO6, 384, 192, (1, 3, 3), S1, 2, 9, 33, offset=True),
    ConvCase("halo6_k1_192_96", K_HALO6, 192, 96, (1, 3, 3), S1, 1, 16, 64, "w8"),
    ConvCase("halo6_c32_96", K_HALO6, 32, 96, (3, 3, 3), S1, 1, 9, 33, cin_live=3),
    ConvCase("halo6_c32_384", K_HALO6, 32, 384, (3, 3, 3), S1, 1, 6, 10, "w8", cin_live=16, zero_front=True),
    # conv_halo_kernel<1>: the decoder head
    ConvCase("halo1_head", K_HALO1, 96, 4, (3, 3, 3), S1, 4, 9, 33, ring=(6, 4), head=True),
    ConvCase("halo1_head_w8", K_HALO1, 96, 4, (3, 3, 3), S1, 4, 6, 10, "w8", ring=(6, 4), head=True, offset=True),
    # the fused RMS_norm + SiLU epilogue
    ConvCase("fuse_ring_dst_T4", K_HALO6, 96, 96, (3, 3, 3), S1, 4, 9, 33, "small", ring=(6, 4), fuse=(6, 3, True)),
    ConvCase("fuse_ring_res_nodst_T1", K_HALO6, 96, 96, (3, 3, 3), S1, 1, 6, 10, "small", ring=(6, 5), res=True, fuse=(3, 2, False)),
    ConvCase("fuse_ring_res_dst_T4", K_HALO6, 96, 96, (3, 3, 3), S1, 4, 6, 10, "small", ring=(6, 4), res=True, fuse=(6, 3, True)),
    ConvCase("fuse_ring_nodst_T1", K_HALO6, 96, 96, (3, 3, 3), S1, 1, 8, 32, "small", ring=(3, 2), fuse=(3, 0, False)),
    ConvCase("fuse_k1_192_96", K_HALO6, 192, 96, (1, 3, 3), S1, 2, 9, 33, "small", fuse=(4, 1, True)),
    # conv_igemm_kernel<3>
    ConvCase("ig3_down_96", K_IGEMM3, 96, 96, (1, 3, 3), S2, 2, 5, 17, frag=False),
    ConvCase("ig3_down_192", K_IGEMM3, 192, 192, (1, 3, 3), S2, 1, 5, 17, "w8", frag=False),
    ConvCase("ig3_short_96_192", K_IGEMM3, 96, 192, (1, 1, 1), S1, 1, 9, 33, frag=False, offset=True),
    ConvCase("ig3_k333_res_nofrag", K_IGEMM3, 96, 96, (3, 3, 3), S1, 2, 6, 10, "w8", frag=False, res=True),
    # (the encoder's 192 -> 192 time_conv: N = 192 is a multiple of 96 and not of 128, so the launcher takes the 96-wide tile)
    ConvCase("ig3_time_down_192", K_IGEMM3, 192, 192, (3, 1, 1), (2, 1, 1), 2, 6, 10, frag=False),      # T = 4 new + 1 cached -> To = 2
    # conv_igemm_kernel<4>
    ConvCase("ig4_down_384", K_IGEMM4, 384, 384, (1, 3, 3), S2, 1, 5, 17, frag=False),
    ConvCase("ig4_time_384_768", K_IGEMM4, 384, 768, (3, 1, 1), S1, 2, 6, 10, "w8", frag=False),
    ConvCase("ig4_time_down_384", K_IGEMM4, 384, 384, (3, 1, 1), (2, 1, 1), 2, 6, 10, frag=False),      # T = 4 new + 1 cached -> To = 2
    ConvCase("ig4_short_192_384_M256", K_IGEMM4, 192, 384, (1, 1, 1), S1, 1, 8, 32, frag=False),
    ConvCase("ig4_enc_head_384_32", K_IGEMM4, 384, 32, (3, 3, 3), S1, 1, 6, 10, "w8"),
    # ordinary data: one per kernel
    ConvCase("gauss_halo6", K_HALO6, 96, 96, (3, 3, 3), S1, 2, 9, 33, "gauss", ring=(4, 3)),
    ConvCase("gauss_halo1", K_HALO1, 96, 4, (3, 3, 3), S1, 2, 6, 10, "gauss", ring=(4, 3), head=True),
    ConvCase("gauss_ig3", K_IGEMM3, 96, 96, (1, 3, 3), S2, 1, 5, 17, "gauss", frag=False),
    ConvCase("gauss_ig4", K_IGEMM4, 192, 384, (1, 1, 1), S1, 1, 9, 33, "gauss", frag=False),
    # ordinary data at K = 27 * 384 = 10368, one per kernel (see GAUSS_DEEP_MARGIN)
    ConvCase("gaussdeep_halo6", K_HALO6, 384, 384, (3, 3, 3), S1, 2, 6, 10, "gauss", ring=(4, 3)),
    ConvCase("gaussdeep_halo1", K_HALO1, 384, 4, (3, 3, 3), S1, 2, 9, 33, "gauss", ring=(4, 3), head=True),
    ConvCase("gaussdeep_ig3", K_IGEMM3, 384, 96, (3, 3, 3), S1, 2, 6, 10, "gauss", frag=False),
    ConvCase("gaussdeep_ig4", K_IGEMM4, 384, 32, (3, 3, 3), S1, 1, 9, 33, "gauss"),       # the encoder head's shape
]

# The Gaussian-data bound |y - y64| <= 2^-9 |y64| + K 2^-24 (|A| * |W|) allows 2^-9 |y| for the final bf16 rounding, but round to
# nearest with 8 significant bits costs up to 2^-8 |y| (at the bottom of a binade): the bound can hold for a correctly rounded
# result only where the accumulation term covers the other 2^-9 |y|.  That term grows like K^1.5 against |y| for random-sign data,
# so the bound is asserted on the "gaussdeep_" cases (K = 10368 for the VAE, 4608 for TAEHV), chosen so that bf16(y64) ITSELF uses at
# most this share of the bound on every element -- a condition on the float64 reference alone, checked on the CPU
# (tests/test_vae_kernel_ref.py).  The rest is room for the kernel's fp32 accumulation, whose real error (~ sqrt(K) 2^-24 |a||w|)
# is far below the worst-case term.  The small "gauss_" cases are held to the sharper 2^-8 |y| form of the bound instead.
GAUSS_DEEP_MARGIN = 0.75


def is_deep(c) -> bool:
    return c.name.startswith("gaussdeep_")


def _operands(g, regime, xshape, wshape, nbias, rshape):
    if regime == "gauss":
        return _gauss_bf16(g, xshape), _gauss_bf16(g, wshape, 0.05), _gauss_bf16(g, (nbias,), 0.5), \
            (_gauss_bf16(g, rshape) if rshape else None)
    ax, aw = {"act8": (255, 2), "w8": (2, 255), "small": (7, 1)}[regime]
    lim = 16 if regime == "small" else 255
    return _ints(g, xshape, ax), _ints(g, wshape, aw), _ints(g, (nbias,), lim), (_ints(g, rshape, lim) if rshape else None)


@lru_cache(maxsize=None)
def build_conv(c: ConvCase) -> dict:
    """Everything of a VAE conv case, on the CPU: the plain tensors, the reference and the kernel's operands."""
    g = _rng(c.name)
    kt, kh, kw = c.k
    st, sy, sx = c.s
    Tp, Hp, Wp = (c.To - 1) * st + kt, (c.Ho - 1) * sy + kh, (c.Wo - 1) * sx + kw
    # the zero padding the product applies: one pixel all round for a stride-1 3x3, ZeroPad2d((0, 1, 0, 1)) for the stride-2 one
    pad = (1, 1, 1, 1) if (kh == 3 and sy == 1) else ((0, 1, 0, 1) if kh == 3 else (0, 0, 0, 0))
    Hi, Wi = Hp - pad[2] - pad[3], Wp - pad[0] - pad[1]
    live = c.cin_live or c.Cin
    nw = 3 if c.head else c.N
    x, w, bias, res = _operands(g, c.regime, (1, live, Tp, Hi, Wi), (nw, live) + c.k, nw,
                                (1, c.N, c.To, c.Ho, c.Wo) if c.res else None)
    if c.zero_front:
        x[:, :, :kt - 1] = 0.0
    xp = F.pad(x, pad)                                              # explicit zero padding
    w_ref, bias_ref = w, bias
    if c.head:                                                      # the padded fourth channel computes 0
        w_ref = torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))])
        bias_ref = torch.cat([bias, bias.new_zeros(1)])
    y, acc = vae_conv_ref(xp, w_ref, bias_ref, c.s, res)
    out = dict(case=c, x=x, xp=xp, w=w_ref, bias=bias_ref, res=res, y=y, acc=acc, Tp=Tp, Hp=Hp, Wp=Wp)
    if c.regime != "gauss":
        out["exact_max"] = assert_exact_regime(xp, w_ref, bias_ref, res, c.s)
    # ---- the kernel's operands: channels padded to Cin with zeros as the product does, weights through the product's packers
    xk = xp if live == c.Cin else torch.cat([xp, xp.new_zeros(1, c.Cin - live, Tp, Hp, Wp)], dim=1)
    out["vol"] = to_cl(xk)                                          # [Tp, Hp, Wp, Cin]
    wname = "decoder.head.2" if c.head else "layer"
    wt = w[:, :, 0] if (kt == 1 and kh == 3) else w                 # the resamplers are Conv2d: [N, Cin, 3, 3]
    W2d = VaeEngine._repack(wname + ".weight", bf16_exact(wt)).contiguous()
    out["W2d"] = W2d
    out["Wfrag"] = VaeEngine._frag_pack(W2d, c.Cin).contiguous() if c.frag else None
    out["bias_k"] = VaeEngine._repack(wname + ".bias", bf16_exact(bias)).contiguous()
    assert W2d.shape == (c.N, kt * kh * kw * c.Cin) and out["bias_k"].numel() == c.N
    if c.res:
        out["ldres"] = c.N + 8
        out["res_k"] = to_plain(res, c.N + 8)
    if c.fuse:
        gamma = _gauss_bf16(g, (c.N,)) + 1.0
        gamma = rbf(torch.where(gamma.abs() < 0.125, torch.ones_like(gamma), gamma))
        out["gamma"] = gamma
        ycl = y[0].permute(1, 2, 3, 0)                              # [To, Ho, Wo, N]
        sq = (ycl * ycl).sum(-1)
        assert float(sq.max()) < EXACT_LIMIT and torch.equal(ycl, torch.round(ycl)), "fused case: the sum of squares must be exact"
        out["norm"], out["norm_amb"] = rms_norm_ref(ycl, gamma, True)
    return out


# ------------------------------------------------------------------------------------------------ TAEHV conv cases
@dataclass(frozen=True)
class TaehvCase:
    name: str
    C0: int
    C1: int
    Nw: int
    ntaps: int
    T: int
    Ho: int
    Wo: int
    regime: str = "act8"
    up: bool = False
    bias: bool = True
    relu: bool = True
    skip: bool = False                # + skip, keep = the skip of the last frame
    Nsplit: Optional[int] = None      # TGrow: output channels -> frames
    head: bool = False                # 3 output channels: Nw = 16, N = ldd = 4
    cin_live: Optional[int] = None
    ldd_extra: int = 0


TAEHV_CASES = [
    TaehvCase("first_32_256", 32, 0, 256, 9, 2, 9, 13, cin_live=16),
    TaehvCase("mem1_64", 64, 64, 64, 9, 2, 6, 10, "w8"),
    TaehvCase("mem1_256", 256, 256, 256, 9, 3, 9, 33),
    TaehvCase("mem3_64_skip_keep", 64, 0, 64, 9, 3, 9, 13, skip=True),
    TaehvCase("mem3_256_skip_keep", 256, 0, 256, 9, 3, 6, 10, "w8", skip=True, ldd_extra=8),
    TaehvCase("tgrow_64_x2", 64, 0, 128, 1, 2, 9, 13, "w8", bias=False, relu=False, Nsplit=64, ldd_extra=8),
    TaehvCase("tgrow_256_x1", 256, 0, 256, 1, 2, 6, 10, bias=False, relu=False, Nsplit=256),
    TaehvCase("up_256_128", 256, 0, 128, 9, 2, 18, 26, up=True, bias=False, relu=False),
    TaehvCase("up_64_64_relu", 64, 0, 64, 9, 1, 16, 64, "w8", up=True, bias=False),
    TaehvCase("head_64_3", 64, 0, 16, 9, 2, 9, 33, relu=False, head=True),
    TaehvCase("head_64_3_w8", 64, 0, 16, 9, 1, 6, 10, "w8", relu=False, head=True),
    TaehvCase("gauss_mem1_64", 64, 64, 64, 9, 2, 9, 13, "gauss"),
    TaehvCase("gauss_head", 64, 0, 16, 9, 1, 9, 13, "gauss", relu=False, head=True),
    TaehvCase("gaussdeep_mem1_256", 256, 256, 256, 9, 2, 9, 13, "gauss"),
    TaehvCase("gaussdeep_head_512", 256, 256, 16, 9, 2, 9, 13, "gauss", relu=False, head=True),
]


def pad_frames(x: torch.Tensor, fill_border: float = 0.0) -> torch.Tensor:
    """[T, C, H, W] float64 -> TAEHV frames, channels-last bf16 [T, H + 2, W + 2, C] with a one-pixel border."""
    v = bf16_exact(x.permute(0, 2, 3, 1).contiguous())
    T, H, W, C = v.shape
    out = torch.full((T, H + 2, W + 2, C), fill_border, dtype=torch.bfloat16)
    out[:, 1:-1, 1:-1] = v
    return out


def unpad_frames(v: torch.Tensor) -> torch.Tensor:
    return v[:, 1:-1, 1:-1].to(F64).permute(0, 3, 1, 2).contiguous()


@lru_cache(maxsize=None)
def build_taehv(c: TaehvCase) -> dict:
    g = _rng(c.name)
    Hs, Ws = (c.Ho // 2, c.Wo // 2) if c.up else (c.Ho, c.Wo)
    k = 3 if c.ntaps == 9 else 1
    live = c.cin_live or c.C0
    nw = 3 if c.head else c.Nw
    gauss = c.regime == "gauss"
    ax, aw = {"act8": (255, 2), "w8": (2, 255), "gauss": (0, 0)}[c.regime]
    rnd = (lambda shape, lim, std=1.0: _gauss_bf16(g, shape, std)) if gauss else (lambda shape, lim, std=1.0: _ints(g, shape, lim))
    # a MemBlock's run of frames [memory, x_0 .. x_{T-1}]: src0 = x_f, src1 = the frame before it
    run = rnd((c.T + 1, live, Hs, Ws), ax)
    x0 = run[1:]
    x1 = run[:-1] if c.C1 else None
    w = rnd((nw, live + c.C1, k, k), aw, 0.05)
    bias = rnd((nw,), 255, 0.5) if c.bias else None
    skip = rnd((c.T, c.Nw, c.Ho, c.Wo), 255) if c.skip else None
    y, xin = taehv_conv_ref(x0, x1, w, bias, skip, c.relu, c.up)
    out = dict(case=c, run=run, w=w, bias=bias, skip=skip, y=y, xin=xin, Hs=Hs, Ws=Ws)
    if not gauss:
        out["exact_max"] = assert_exact_regime(xin, w, bias, skip[:, :nw] if skip is not None else None)
    runk = run if live == c.C0 else torch.cat([run, run.new_zeros(c.T + 1, c.C0 - live, Hs, Ws)], dim=1)
    out["run_k"] = pad_frames(runk)                                 # [T + 1, Hs + 2, Ws + 2, C0]
    wk = w if live == c.C0 else torch.cat([w, w.new_zeros(nw, c.C0 - live, k, k)], dim=1)
    out["Wfrag"] = TaehvEngine._repack("layer.weight", bf16_exact(wk)).contiguous()
    assert out["Wfrag"].numel() == (c.C0 + c.C1) // 32 * c.ntaps * c.Nw * 32
    out["bias_k"] = TaehvEngine._repack("layer.bias", bf16_exact(bias)).contiguous() if c.bias else None
    if c.skip:
        out["skip_k"] = pad_frames(skip)
    out["N"] = 4 if c.head else c.Nw
    out["Nsplit"] = c.Nsplit or c.Nw
    out["ldd"] = (4 if c.head else out["Nsplit"]) + c.ldd_extra
    return out


# ------------------------------------------------------------------------------------------------ the passes
NORM_CASES = [(C, npix, mode) for C in (96, 192, 384) for npix in (1, 33, 297) for mode in ("copy", "norm", "silu")]


@lru_cache(maxsize=None)
def build_norm(C: int, npix: int, mode: str) -> dict:
    """Integer activations of +-255 (full mantissas, an exact fp32 sum of squares), a generic bf16 gamma."""
    H, W = {1: (1, 1), 33: (1, 33), 297: (9, 33)}[npix]
    g = _rng(f"norm{C}_{npix}_{mode}_0")
    x = _ints(g, (npix, C), 255)
    assert float((x * x).sum(-1).max()) < EXACT_LIMIT, "the fp32 sum of squares must be exact"
    gamma = None
    if mode != "copy":
        gamma = _gauss_bf16(g, (C,)) + 1.0
        gamma = rbf(torch.where(gamma.abs() < 0.125, torch.ones_like(gamma), gamma))
    ref, amb = rms_norm_ref(x, gamma, mode == "silu")
    return dict(x=x, gamma=gamma, ref=ref, amb=amb, H=H, W=W)


def latent_scales(seed: str, structured: bool):
    """mean / inv_std [16] as the product hands them over: bf16-valued floats.  structured: only channels 0 and 1 are arbitrary, the
    others are small integers and powers of two, all different, which keeps z_prep's own roundings exact there (zprep_ref)."""
    g = _rng(seed)
    sign = torch.where(torch.rand(16, generator=g) < 0.5, -1.0, 1.0).to(F64)
    mean = rbf(sign * (40.0 + torch.rand(16, generator=g).to(F64)))
    inv = rbf(1.0 / (0.5 + torch.rand(16, generator=g).to(F64)))
    if structured:
        mean[2:] = _ints(g, (14,), 16)
        inv[2:] = 2.0 ** -(torch.arange(14) % 4).to(F64)
    return mean, inv


@lru_cache(maxsize=None)
def build_zprep() -> dict:
    """z_prep_kernel's case: 2 frames of 5 x 7 latents, integers of +-15; w2 in -2..2, b2 in +-16."""
    F_, h, w = 2, 5, 7
    g = _rng("zprep")
    z = _ints(g, (F_, 16, h, w), 15)
    w2, b2 = _ints(g, (16, 16), 2), _ints(g, (16,), 16)
    mean, inv = latent_scales("zprep_scales", True)
    ref, amb = zprep_ref(z, mean, inv, w2, b2)
    return dict(F=F_, h=h, w=w, z=z, w2=w2, b2=b2, mean=mean, inv=inv, ref=ref, amb=amb)


@lru_cache(maxsize=None)
def build_mu_out() -> dict:
    """mu_out_kernel's case: 2 frames of 5 x 7 encoder pixels, integers of +-255; w1 in -2..2, b1 in +-255; arbitrary scales."""
    F_, h, w = 2, 5, 7
    g = _rng("mu")
    enc = _ints(g, (F_, h, w, 32), 255)
    w1, b1 = _ints(g, (32, 32), 2), _ints(g, (32,), 255)
    mean, inv = latent_scales("mu_scales", False)
    ref, amb = mu_out_ref(enc, w1, b1, mean, inv)
    return dict(F=F_, h=h, w=w, enc=enc, w1=w1, b1=b1, mean=mean, inv=inv, ref=ref, amb=amb)


TAEHV_PREP_CASES = [(9, 13), (6, 10)]


@lru_cache(maxsize=None)
def build_taehv_prep(h: int, w: int) -> dict:
    """taehv_prep_kernel's case: Gaussian bf16 latents of std 2, so tanh(z / 3) runs from its linear part into saturation."""
    z = _gauss_bf16(_rng(f"prep{h}"), (16, h, w), 2.0)
    ref, amb = taehv_prep_ref(z)
    return dict(z=z, ref=ref, amb=amb)


def softmax_scores(rows: int, cols: int, name: str) -> torch.Tensor:
    """fp32 scores spread over [-30, 30]: every probability is >= e^-60 / cols > 2^-100."""
    return (torch.rand((rows, cols), generator=_rng(name)) * 60.0 - 30.0).to(torch.float32)
