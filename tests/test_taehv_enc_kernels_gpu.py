"""The TAEHV encoder's own kernels one launch at a time, bit-exact against float64 (taehv_enc_kernels.hip through
mmpl_taehv_conv_in / mmpl_taehv_conv_s2 / mmpl_taehv_z_out), and TPool through the existing mmpl_taehv_conv.

Inputs and weights are small integers (conv_in: bf16(u / 255), multiples of 2^-15 below 1, against integer weights), so every fp32
accumulation is exact whatever its order and the expected output is the float64 convolution rounded to bf16 once.  Destination
buffers start as a sentinel: borders, and frames the launch does not address, must still hold it.  Source frames sit between guard
frames of a poison value, and the bottom row / right column of a stride-2 source's border -- which no valid output reads -- hold
poison too: a tap that strays shows up in the result."""
import pytest
import torch
import torch.nn.functional as F

from mmpl_amd import _lib
from mmpl_amd.taehv import TaehvEncoderEngine, TaehvEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, POISON = -77.0, 5.0


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _padded(x, border=0.0):
    """[T, C, H, W] float64 -> channels-last bf16 frames [T, H + 2, W + 2, C] with `border` around"""
    T, C, H, W = x.shape
    out = torch.full((T, H + 2, W + 2, C), border, dtype=torch.float64)
    out[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return out.to(torch.bfloat16)


def _check_dst(dst, expect, first):
    """dst [n, H + 2, W + 2, C] from the device; frames first .. first + T - 1 hold `expect` [T, C, H, W] (float64, exact before the
    one rounding) in their interiors, and everything else the sentinel"""
    T = expect.shape[0]
    want = torch.full(dst.shape, SENTINEL, dtype=torch.bfloat16)
    want[first:first + T, 1:-1, 1:-1] = expect.permute(0, 2, 3, 1).to(torch.bfloat16)
    bad = dst.cpu().view(torch.int16) != want.view(torch.int16)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ (first at {bad.nonzero()[0].tolist()})"


def _s2_weight(C):
    """[64, C, 3, 3]: output channel n < 9 * C / 32 singles out tap n // (C / 32) of channel 32 * (n % (C / 32)) + 5 -- the output IS
    that input pixel, so every tap and every 32-channel chunk is told apart; the other rows are random integers in [-1, 1]"""
    w = _ints((64, C, 3, 3), -1, 1, 11)
    nch = C // 32
    for n in range(9 * nch):
        tap, chunk = divmod(n, nch)
        w[n] = 0
        w[n, 32 * chunk + 5, tap // 3, tap % 3] = 1
    return w


@pytest.mark.parametrize("relu", [0, 1], ids=["plain", "relu"])
@pytest.mark.parametrize("Ho,Wo", [(9, 35), (1, 1)], ids=["9x35", "1x1"])
def test_conv_s2(lib, Ho, Wo, relu):
    T, C, Hi, Wi = 2, 64, 2 * Ho, 2 * Wo
    x = _ints((T, C, Hi, Wi), -2, 2, 3)
    w = _s2_weight(C)
    y = F.conv2d(x, w, None, stride=2, padding=1)
    assert float(y.abs().max()) < 2 ** 24 and tuple(y.shape) == (T, 64, Ho, Wo)
    if relu:
        y = y.clamp_min(0)
    src = torch.full((T + 2, Hi + 2, Wi + 2, C), POISON, dtype=torch.bfloat16)
    src[1:-1] = _padded(x)
    src[1:-1, -1, :] = POISON                          # the bottom row and the right column of the border are never read
    src[1:-1, :, -1] = POISON
    src = src.to(DEV)
    Wfrag = TaehvEngine._repack("w.weight", w).to(DEV)
    dst = torch.full((T + 2, Ho + 2, Wo + 2, 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
    fs, fsd = src[0].numel(), dst[0].numel()
    _lib.check(lib.mmpl_taehv_conv_s2(src.data_ptr() + 2 * fs, fs, C, _lib.ptr(Wfrag), 64, T, Ho, Wo, dst.data_ptr() + 2 * fsd, fsd,
                                      relu, _lib.stream_ptr()), "mmpl_taehv_conv_s2")
    torch.cuda.synchronize()
    _check_dst(dst, y, 1)


def _pixels_u8(T, H, W):
    g = torch.Generator().manual_seed(21)
    u = torch.randint(0, 256, (T, H, W, 3), generator=g, dtype=torch.uint8)
    u.view(-1)[:5] = torch.tensor([0, 1, 127, 128, 255], dtype=torch.uint8)
    u[-1, -1, -1] = torch.tensor([255, 128, 1], dtype=torch.uint8)
    return u


def _in_weight():
    """[64, 3, 3, 3]: output channel n < 27 singles out product k = n = (3 ky + kx) * 3 + c; the rest random integers in [-2, 2]"""
    w = _ints((64, 3, 3, 3), -2, 2, 13)
    for n in range(27):
        tap, c = divmod(n, 3)
        w[n] = 0
        w[n, c, tap // 3, tap % 3] = 1
    return w


_conv_in_out = {}


def _run_conv_in(lib, H, W, fmt):
    """-> (dst frames from the device, expected [T, 64, H, W] float64), one launch per (size, format)"""
    if (H, W, fmt) not in _conv_in_out:
        T = 2
        u = _pixels_u8(T, H, W)
        xf = (u.float() / 255).permute(0, 3, 1, 2).contiguous()                 # float32 [T, 3, H, W], the kernel's format 0
        w, b = _in_weight(), _ints((64,), -3, 3, 14)
        b[:27] = 0                                                               # the selected products come out as they are
        y = F.conv2d(xf.to(torch.bfloat16).double(), w, b, padding=1).clamp_min(0)
        Wfrag = TaehvEncoderEngine._repack("encoder.0.weight", w).to(DEV)
        bias = b.to(torch.bfloat16).to(DEV)
        dst = torch.full((T + 2, H + 2, W + 2, 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
        px = (u if fmt else xf).to(DEV)
        fsd = dst[0].numel()
        _lib.check(lib.mmpl_taehv_conv_in(_lib.ptr(px), fmt, _lib.ptr(Wfrag), _lib.ptr(bias), T, H, W, dst.data_ptr() + 2 * fsd, fsd,
                                          _lib.stream_ptr()), "mmpl_taehv_conv_in")
        torch.cuda.synchronize()
        _conv_in_out[(H, W, fmt)] = (dst.cpu(), y, u)
    return _conv_in_out[(H, W, fmt)]


@pytest.mark.parametrize("fmt", [0, 1], ids=["float", "uint8"])
@pytest.mark.parametrize("H,W", [(10, 34), (8, 8)], ids=["10x34", "8x8"])
def test_conv_in(lib, H, W, fmt):
    dst, y, u = _run_conv_in(lib, H, W, fmt)
    assert {0, 1, 127, 128, 255} <= set(u.view(-1).tolist())
    _check_dst(dst, y, 1)
    # channel n < 27 is the bf16 pixel under tap (ky, kx) of colour c, zero where the conv's padding lies
    got = dst[1:3, 1:-1, 1:-1].float()
    px = F.pad((u.float() / 255).to(torch.bfloat16).float(), (0, 0, 1, 1, 1, 1))             # [T, H + 2, W + 2, 3]
    for n in range(27):
        tap, c = divmod(n, 3)
        assert torch.equal(got[..., n], px[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, c]), (n, tap, c)


@pytest.mark.parametrize("H,W", [(10, 34), (8, 8)], ids=["10x34", "8x8"])
def test_conv_in_uint8_equals_float(lib, H, W):
    a, b = _run_conv_in(lib, H, W, 0)[0], _run_conv_in(lib, H, W, 1)[0]
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_z_out(lib):
    T, h, w, f_out = 2, 5, 7, 1
    g = torch.Generator().manual_seed(5)
    z = torch.randn(T, 16, h, w, generator=g).to(torch.bfloat16)
    src = torch.full((T, h + 2, w + 2, 16), POISON, dtype=torch.bfloat16)
    src[:, 1:-1, 1:-1] = z.permute(0, 2, 3, 1)
    out = torch.full((T + 2, 16, h, w), SENTINEL, dtype=torch.bfloat16, device=DEV)
    src = src.to(DEV)
    _lib.check(lib.mmpl_taehv_z_out(_lib.ptr(src), _lib.ptr(out), T, h, w, f_out, _lib.stream_ptr()), "mmpl_taehv_z_out")
    torch.cuda.synchronize()
    want = torch.full((T + 2, 16, h, w), SENTINEL, dtype=torch.bfloat16)
    want[f_out:f_out + T] = z
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_tpool_pairs_frames(lib):
    """TPool(2) as the encoder launches it on the existing conv entry: ntaps 1, src0 = the even frames, src1 = the odd ones, both
    with a stride of two frames.  Output channel n < 64 copies channel n of frame 2t, channel 64 + n ... of frame 2t + 1 is told
    apart by the weight's second half."""
    T, C, H, W = 2, 64, 6, 10
    x = _ints((2 * T, C, H, W), -2, 2, 7)
    w = _ints((64, 2 * C, 1, 1), -1, 1, 8)
    for n in range(32):                                   # rows 0 .. 31: even frame's channel n; rows 32 .. 63: odd frame's channel n
        w[n] = 0
        w[n, n] = 1
        w[32 + n] = 0
        w[32 + n, C + n] = 1
    y = F.conv2d(x.reshape(T, 2 * C, H, W), w)
    assert torch.equal(y[:, :32], x[0::2, :32]) and torch.equal(y[:, 32:], x[1::2, :32])
    src = torch.full((2 * T + 2, H + 2, W + 2, C), POISON, dtype=torch.bfloat16)
    src[1:-1] = _padded(x)
    src = src.to(DEV)
    Wfrag = TaehvEngine._repack("w.weight", w).to(DEV)
    dst = torch.full((T + 2, H + 2, W + 2, 64), SENTINEL, dtype=torch.bfloat16, device=DEV)
    fs, fsd = src[0].numel(), dst[0].numel()
    _lib.check(lib.mmpl_taehv_conv(src.data_ptr() + 2 * fs, src.data_ptr() + 4 * fs, 2 * fs, 2 * fs, C, C, 0, 1, _lib.ptr(Wfrag), None,
                                   64, 64, T, H, W, dst.data_ptr() + 2 * fsd, fsd, 64, 64, 0, None, 0, None, _lib.stream_ptr()),
               "mmpl_taehv_conv")
    torch.cuda.synchronize()
    _check_dst(dst, y, 1)
