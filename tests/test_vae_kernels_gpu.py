"""The Wan VAE kernels one launch at a time against float64 (vae_kernels.hip through the mmpl_vae_* kernel-level entry points).

Every convolution case runs ONE launch on operands made from plain tensors by the product's own packers and compares it with
torch conv3d in float64 (tests/vae_kernel_ref.py).  In the exact regime (integer operands, every partial sum below 2^24) the
result must be bit-identical; everything a launch does not own -- borders, channels [N, ldd), frames and slots it was not given,
pixels outside its window -- must still hold the sentinel it was filled with.  Each case asserts the kernel the launcher reported.
The division / exponential passes follow the near-tie rule, the softmax and the Gaussian cases derived bounds (see the reference
module's docstring and the tests below).  The pixel passes (px_in, px_out, px_out_u8) are pure data movement and clamping and must
match exactly, px_out_u8 on every bf16 bit pattern.  Whole-network accuracy stays in tests/test_vae_gpu.py; the compositions are held
to a chain of these launches in tests/test_vae_chain_gpu.py."""
import ctypes as C
import math

import pytest
import torch

import vae_kernel_ref as R
from mmpl_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sentinel(*shape):
    return torch.full(shape, R.SENTINEL, dtype=torch.bfloat16, device=DEV)


def run_conv(lib, c: R.ConvCase):
    """One mmpl_vae_conv launch of case c.  Returns (kernel, dst volume, window, consumer ring) on the CPU."""
    b = R.build_conv(c)
    kt, kh, kw = c.k
    W, bias = b["W2d"].to(DEV), b["bias_k"].to(DEV)
    Wfrag = b["Wfrag"].to(DEV) if c.frag else None
    src, frames, n_frames = None, None, 0
    if c.ring:
        Tp, base = c.ring
        ring = R.to_ring(b["vol"], Tp, base).to(DEV)               # logical frame j in slot (base + j) % Tp
        frames, n_frames = _ptrs([ring[s] for s in R.ring_slots(Tp, base, b["Tp"])]), b["Tp"]
    else:
        src = b["vol"].to(DEV)
    # destination: plain [To, Ho, Wo, N], or an offset window of a larger and wider volume
    win = (c.To + 2, c.Ho + 2, c.Wo + 3, c.N + 8, 1, 1, 2) if c.offset else (c.To, c.Ho, c.Wo, c.N, 0, 0, 0)
    Td, Hd, Wd, ldd, dt0, dy0, dx0 = win
    dst = None
    if not c.fuse or c.fuse[2]:
        dst = _sentinel(Td, Hd, Wd, ldd)
    res = b["res_k"].to(DEV) if c.res else None
    gamma, nring, nframes = None, None, None
    if c.fuse:
        nTp, nbase, _ = c.fuse
        gamma = R.bf16_exact(b["gamma"]).to(DEV)
        nring = _sentinel(nTp, c.Ho + 2, c.Wo + 2, c.N)
        nframes = _ptrs([nring[s] for s in R.ring_slots(nTp, nbase + 2, c.To)])     # resolve_fuse: slot (base + t + 2) % Tp
    kernel = C.c_int(-1)
    rc = lib.mmpl_vae_conv(_lib.ptr(src), frames, n_frames, c.Cin, b["Hp"], b["Wp"], *c.s, kt, kh, kw, _lib.ptr(W), _lib.ptr(Wfrag),
                           _lib.ptr(bias), c.To, c.Ho, c.Wo, c.N, _lib.ptr(dst), Hd, Wd, ldd, dt0, dy0, dx0, _lib.ptr(res),
                           b.get("ldres", 0), _lib.ptr(gamma), math.sqrt(c.N), nframes, C.byref(kernel), _lib.stream_ptr())
    _lib.check(rc, "mmpl_vae_conv")
    torch.cuda.synchronize()
    return kernel.value, (dst.cpu() if dst is not None else None), win, (nring.cpu() if nring is not None else None)


EXACT = [c for c in R.CONV_CASES if c.regime != "gauss"]
GAUSS = [c for c in R.CONV_CASES if c.regime == "gauss"]


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_conv_exact(lib, c):
    """Exact regime: bit-identical to float64 conv3d with bf16(acc + bias) [bf16(+ res)]; the fused norm output by the near-tie rule."""
    b = R.build_conv(c)
    kernel, dst, win, nring = run_conv(lib, c)
    assert kernel == c.kernel, f"the launcher took kernel {kernel}, the case is written for {c.kernel}"
    ref = R.to_cl(b["y"])
    if dst is not None:
        Td, Hd, Wd, ldd, dt0, dy0, dx0 = win
        got = R.extract(dst, c.To, c.Ho, c.Wo, c.N, dt0, dy0, dx0)
        nbad = int((R.bf16_line(got) != R.bf16_line(ref)).sum())
        print(f"{c.name}: max sum|a||w| {b['exact_max']:.0f}, {nbad} of {got.numel()} elements differ")
        assert nbad == 0, f"{nbad} of {got.numel()} elements differ from the float64 reference"
        assert R.outside_is(dst, c.To, c.Ho, c.Wo, c.N, dt0, dy0, dx0), "the launch wrote outside its window"
    if c.fuse:
        nTp, nbase, _ = c.fuse
        slots = R.ring_slots(nTp, nbase + 2, c.To)
        frac = float(b["norm_amb"].double().mean())
        print(f"{c.name}: ambiguous {frac:.4%}")
        for t, s in enumerate(slots):
            R.check_near_tie(nring[s, 1:-1, 1:-1], R.bf16_exact(b["norm"][t]), b["norm_amb"][t], f"{c.name} frame {t}")
            assert R.outside_is(nring[s:s + 1], 1, c.Ho, c.Wo, c.N, 0, 1, 1), "the epilogue wrote a border pixel"
        for s in set(range(nTp)) - set(slots):
            assert bool((nring[s].double() == R.SENTINEL).all()), f"slot {s} was not addressed but written"


_gauss_cache = {}


def _gauss_errors(lib, c):
    """One launch of a Gaussian case -> (|y - y64|, |y64|, K 2^-24 (|A| * |W|), the same error of the correctly rounded bf16(y64),
    sentinel rule held), shared by the two tests below."""
    if c.name not in _gauss_cache:
        b = R.build_conv(c)
        kernel, dst, win, _ = run_conv(lib, c)
        assert kernel == c.kernel
        y64 = (b["acc"] + b["bias"].view(1, -1, 1, 1, 1))[0].permute(1, 2, 3, 0)
        acc_bound = R.accum_bound(b["xp"], b["w"], c.s)[0].permute(1, 2, 3, 0)
        got = R.extract(dst, c.To, c.Ho, c.Wo, c.N, *win[4:]).double()
        _gauss_cache[c.name] = ((got - y64).abs(), y64.abs(), acc_bound, (R.rbf(y64) - y64).abs(),
                                R.outside_is(dst, c.To, c.Ho, c.Wo, c.N, *win[4:]))
    return _gauss_cache[c.name]


@pytest.mark.parametrize("c", [c for c in GAUSS if R.is_deep(c)], ids=lambda c: c.name)
def test_conv_gaussian(lib, c):
    """Ordinary data: |y - y64| <= 2^-9 |y64| + K 2^-24 (|A| * |W|) per element, K = ntaps * Cin = 10368.

    2^-9 |y| is half of what a bf16 rounding can cost (8 significant bits: up to 2^-8 |y|), so this bound can hold only where the
    accumulation term covers the rest; the cases are chosen for that from the float64 reference alone (vae_kernel_ref.GAUSS_DEEP_MARGIN:
    bf16(y64) itself stays under 0.75 of the bound on every element).  On the small Gaussian cases the correctly rounded result breaks
    it (worst error / bound 1.17 - 1.93, kernel and bf16(y64) alike); those are held to the 2^-8 form below.

    This bound is NOT tight: at K = 10368 it is dominated by the worst-case accumulation term, which is what leaves room for the
    rounding, so it catches only gross accumulation errors.  The bit-identical exact-regime cases carry the real weight."""
    err, mag, acc_bound, err_rounded, clean = _gauss_errors(lib, c)
    bound = (2.0 ** -9 * mag + acc_bound).clamp_min(1e-300)
    worst = float((err / bound).max())
    print(f"{c.name}: worst error / bound = {worst:.3f}; of the correctly rounded bf16(y64): {float((err_rounded / bound).max()):.3f}")
    assert clean
    assert worst <= 1.0


@pytest.mark.parametrize("c", GAUSS, ids=lambda c: c.name)
def test_conv_gaussian_unit_roundoff(lib, c):
    """|y - y64| <= 2^-8 |y64| + K 2^-24 (|A| * |W|): the unit roundoff of bf16 (8 significant bits, round to nearest) for the one final
    rounding, plus the standard worst-case bound of an fp32 accumulation of K = ntaps * Cin products (bias included in y64)."""
    err, mag, acc_bound, _, clean = _gauss_errors(lib, c)
    worst = float((err / (2.0 ** -8 * mag + acc_bound).clamp_min(1e-300)).max())
    print(f"{c.name}: worst error / bound = {worst:.3f}")
    assert clean and worst <= 1.0


def test_every_conv_kernel_has_an_exact_case():
    assert {c.kernel for c in EXACT} == {R.K_IGEMM3, R.K_IGEMM4, R.K_HALO6, R.K_HALO1}


# ------------------------------------------------------------------------------------------------ passes
@pytest.mark.parametrize("C_,npix,mode", R.NORM_CASES)
def test_norm_act_pad(lib, C_, npix, mode):
    """norm_act_pad_kernel into an offset window of a padded, wider destination: copy bit-identical, norm / norm + SiLU by the
    near-tie rule; C = 96 / 192 / 384 are the 16- / 32- / 64-lane groups."""
    b = R.build_norm(C_, npix, mode)
    H, W = b["H"], b["W"]
    x = R.bf16_exact(b["x"]).to(DEV)
    gamma = R.bf16_exact(b["gamma"]).to(DEV) if b["gamma"] is not None else None
    Td, Hd, Wd, ldd, dt0, dy0, dx0 = 3, H + 2, W + 3, C_ + 8, 1, 1, 2
    dst = _sentinel(Td, Hd, Wd, ldd)
    _lib.check(lib.mmpl_vae_norm(_lib.ptr(x), 1, H, W, C_, _lib.ptr(gamma), math.sqrt(C_), int(mode == "silu"), _lib.ptr(dst), Hd, Wd,
                                 ldd, dt0, dy0, dx0, _lib.stream_ptr()), "mmpl_vae_norm")
    torch.cuda.synchronize()
    dst = dst.cpu()
    got = R.extract(dst, 1, H, W, C_, dt0, dy0, dx0).reshape(npix, C_)
    print(f"norm C={C_} npix={npix} {mode}: ambiguous {float(b['amb'].double().mean()):.4%}")
    R.check_near_tie(got, R.bf16_exact(b["ref"]), b["amb"], f"norm C={C_} npix={npix} {mode}")
    assert R.outside_is(dst, 1, H, W, C_, dt0, dy0, dx0)


@pytest.mark.parametrize("C_,interleave", [(192, 0), (192, 1), (384, 0), (384, 1)])
def test_upsample_pad(lib, C_, interleave):
    """Pure data movement: nearest x2 (with the time_conv de-interleave) bit-identical, border untouched."""
    H, W, To = 3, 5, 2
    Ts, lds = (To // 2, 2 * C_) if interleave else (To, C_)
    src = R._ints(R._rng(f"up{C_}_{interleave}"), (Ts, H, W, lds), 255)
    dst = _sentinel(To, 2 * H + 2, 2 * W + 2, C_)
    s = R.bf16_exact(src).to(DEV)
    _lib.check(lib.mmpl_vae_upsample(_lib.ptr(s), lds, C_, H, W, To, interleave, _lib.ptr(dst), 2 * H + 2, 2 * W + 2, _lib.stream_ptr()),
               "mmpl_vae_upsample")
    torch.cuda.synchronize()
    dst = dst.cpu()
    frames = src.reshape(Ts, H, W, 2, C_).permute(0, 3, 1, 2, 4).reshape(To, H, W, C_) if interleave else src
    ref = frames.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(R.extract(dst, To, 2 * H, 2 * W, C_, 0, 1, 1).double(), ref)
    assert R.outside_is(dst, To, 2 * H, 2 * W, C_, 0, 1, 1)


@pytest.mark.parametrize("rows,ldt", [(60, 64), (96, 128)])
def test_transpose(lib, rows, ldt):
    """v [rows, C] at row stride 3C (the V third of a qkv buffer) -> vt [C, ldt], bit-identical, the tail [rows, ldt) zero."""
    C_ = 96
    qkv = R._ints(R._rng(f"tr{rows}"), (rows, 3 * C_), 255)
    q = R.bf16_exact(qkv).to(DEV)
    vt = _sentinel(C_ + 1, ldt)                                    # one row more than the kernel owns
    _lib.check(lib.mmpl_vae_transpose(C.c_void_p(q.data_ptr() + 2 * C_ * 2), 3 * C_, _lib.ptr(vt), ldt, rows, C_, _lib.stream_ptr()),
               "mmpl_vae_transpose")
    torch.cuda.synchronize()
    vt = vt.cpu().double()
    assert torch.equal(vt[:C_, :rows], qkv[:, 2 * C_:].t())
    assert bool((vt[:C_, rows:] == 0).all()) and bool((vt[C_] == R.SENTINEL).all())


@pytest.mark.parametrize("cols", [1, 63, 65, 96, 300])
def test_softmax_rows(lib, cols):
    """|p - p64| <= 2^-8 p64 per element (2^-9 of the final bf16 rounding; an fp32 sum over <= 300 terms plus __expf stay under
    2^-13); scores spread over [-30, 30] keep every probability above 2^-100.  The tail [cols, ldp) must be exactly zero."""
    rows, ld = 5, cols + 3
    ldp = (cols + 63) // 64 * 64
    sc = torch.full((rows, ld), float("nan"), dtype=torch.float32)
    sc[:, :cols] = R.softmax_scores(rows, cols, f"sm{cols}")
    p = _sentinel(rows + 1, ldp)
    s = sc.to(DEV)
    _lib.check(lib.mmpl_vae_softmax(_lib.ptr(s), ld, _lib.ptr(p), ldp, rows, cols, _lib.stream_ptr()), "mmpl_vae_softmax")
    torch.cuda.synchronize()
    p = p.cpu().double()
    p64 = R.softmax_ref(sc[:, :cols])
    assert float(p64.min()) >= 2.0 ** -100
    worst = float(((p[:rows, :cols] - p64).abs() / p64).max())
    print(f"softmax cols={cols}: worst relative error {worst:.3e} (bound {2.0 ** -8:.3e})")
    assert worst <= 2.0 ** -8
    assert bool((p[:rows, cols:] == 0).all()) and bool((p[rows] == R.SENTINEL).all())


def _f16(v):
    return (C.c_float * 16)(*v.tolist())


def test_z_prep(lib):
    """z_prep_kernel (de-normalisation + conv2 1x1x1) into frame dt0 of a padded 32-channel volume: near-tie rule; border, channels
    16..31 and the other frames untouched."""
    b = R.build_zprep()
    F_, h, w = b["F"], b["h"], b["w"]
    print(f"z_prep: ambiguous {float(b['amb'].double().mean()):.4%}")
    dst = _sentinel(F_ + 3, h + 2, w + 2, 32)
    zd, w2d, b2d = R.bf16_exact(b["z"]).to(DEV), R.bf16_exact(b["w2"]).to(DEV), R.bf16_exact(b["b2"]).to(DEV)
    _lib.check(lib.mmpl_vae_zprep(_lib.ptr(zd), F_, h, w, _f16(b["mean"]), _f16(b["inv"]), _lib.ptr(w2d), _lib.ptr(b2d), _lib.ptr(dst), 2,
                                  _lib.stream_ptr()), "mmpl_vae_zprep")
    torch.cuda.synchronize()
    dst = dst.cpu()
    R.check_near_tie(R.extract(dst, F_, h, w, 16, 2, 1, 1), R.bf16_exact(b["ref"]), b["amb"], "z_prep")
    assert R.outside_is(dst, F_, h, w, 16, 2, 1, 1)


def test_mu_out(lib):
    """mu_out_kernel (conv1 1x1x1, first 16 rows, then the normalisation) into frames f_out.. of a float32 latent: near-tie rule."""
    b = R.build_mu_out()
    F_, h, w, f_out = b["F"], b["h"], b["w"], 1
    print(f"mu_out: ambiguous {float(b['amb'].double().mean()):.4%}")
    out = torch.full((F_ + 2, 16, h, w), R.SENTINEL, dtype=torch.float32, device=DEV)
    ed, w1d, b1d = R.bf16_exact(b["enc"]).to(DEV), R.bf16_exact(b["w1"]).to(DEV), R.bf16_exact(b["b1"]).to(DEV)
    _lib.check(lib.mmpl_vae_mu_out(_lib.ptr(ed), _lib.ptr(w1d), _lib.ptr(b1d), _f16(b["mean"]), _f16(b["inv"]), _lib.ptr(out), F_, f_out, h, w,
                                   _lib.stream_ptr()), "mmpl_vae_mu_out")
    torch.cuda.synchronize()
    out = out.cpu()
    got = out[f_out:f_out + F_]
    assert torch.equal(got.to(torch.bfloat16).float(), got), "mu_out stores bf16-rounded values"
    R.check_near_tie(got.to(torch.bfloat16), R.bf16_exact(b["ref"]), b["amb"], "mu_out")
    assert bool((out[:f_out] == R.SENTINEL).all()) and bool((out[f_out + F_:] == R.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ pixel in / out
CANARY_TAIL = 256                  # elements behind every buffer of the pixel cases that no launch may touch


def _tailed(shape, dtype, fill):
    """A buffer of `shape` filled with `fill` with CANARY_TAIL more elements of it behind: (view of the buffer, the whole)."""
    n = math.prod(shape)
    whole = torch.full((n + CANARY_TAIL,), fill, dtype=dtype, device=DEV)
    return whole[:n].view(shape), whole


def _tail_intact(whole, fill):
    return bool((whole[-CANARY_TAIL:].cpu().double() == fill).all())


@pytest.mark.parametrize("H,W", [(16, 24), (8, 8)])
@pytest.mark.parametrize("dt0", [0, 2])
@pytest.mark.parametrize("t0,T", [(0, 1), (1, 4)])
def test_px_in(lib, t0, T, dt0, H, W):
    """px_in_kernel: frames t0 .. t0 + T - 1 of px [3, 5, H, W] -> channels 0..2 of the interior of frames dt0.. of a padded
    32-channel volume, an exact copy; the border, channels 3..31 and the frames in front of dt0 keep the prefill."""
    Ttot = 5
    px = R._ints(R._rng(f"pxin{H}"), (3, Ttot, H, W), 255)
    pxd, px_whole = _tailed((3, Ttot, H, W), torch.bfloat16, R.SENTINEL)
    pxd.copy_(R.bf16_exact(px))
    dst, whole = _tailed((dt0 + T, H + 2, W + 2, 32), torch.bfloat16, R.SENTINEL)
    _lib.check(lib.mmpl_vae_px_in(_lib.ptr(pxd), _lib.ptr(dst), Ttot, t0, T, H, W, dt0, _lib.stream_ptr()), "mmpl_vae_px_in")
    torch.cuda.synchronize()
    vol = dst.cpu()
    assert torch.equal(R.extract(vol, T, H, W, 3, dt0, 1, 1).double(), R.px_in_ref(px, t0, T))
    assert R.outside_is(vol, T, H, W, 3, dt0, 1, 1), "px_in wrote more than three channels of the interior of its frames"
    assert _tail_intact(whole, R.SENTINEL) and _tail_intact(px_whole, R.SENTINEL)


def _px_out_src(name, T, H, W):
    """[T, H, W, 4] bf16: Gaussian values of std 1.5 (a third of them outside [-1, 1]) with, in front, +-1, their bf16 neighbours on
    both sides, +-0, and values far outside; channel 3 holds 0.5, which no other element holds."""
    src = R._gauss_bf16(R._rng(name), (T, H, W, 4), 1.5).to(torch.float32)
    src[src == 0.5] = 0.25
    edge = [1.0, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8, -1.0, -1.0 - 2.0 ** -7, -1.0 + 2.0 ** -8, 0.0, -0.0, 100.0, -100.0, 2.0 ** 127, -2.0 ** 127,
            float("inf"), float("-inf"), 2.0 ** -126, -2.0 ** -133]
    flat = src[..., :3].reshape(-1)
    flat[:len(edge)] = torch.tensor(edge)
    flat[-len(edge):] = torch.tensor(edge)
    src[..., :3] = flat.view(T, H, W, 3)
    src[..., 3] = 0.5
    out = src.to(torch.bfloat16)
    assert torch.equal(out.to(torch.float32), src)
    return out


@pytest.mark.parametrize("t_out", [0, 1])
@pytest.mark.parametrize("T", [1, 4])
def test_px_out(lib, T, t_out):
    """px_out_kernel: float32 [t_out + T, 3, H, W] = clamp(-1, 1) of the bf16 value, bit for bit (the sign of zero included); the
    fourth channel never appears, the frames in front of t_out and the tail keep the prefill."""
    H, W = 16, 24
    src = _px_out_src(f"pxout{T}", T, H, W)
    srcd, src_whole = _tailed((T, H, W, 4), torch.bfloat16, R.SENTINEL)
    srcd.copy_(src)
    out, whole = _tailed((t_out + T, 3, H, W), torch.float32, R.SENTINEL)
    _lib.check(lib.mmpl_vae_px_out(_lib.ptr(srcd), _lib.ptr(out), T, H, W, t_out, _lib.stream_ptr()), "mmpl_vae_px_out")
    torch.cuda.synchronize()
    got = out.cpu()
    ref = R.px_out_ref(src)
    assert torch.equal(got[t_out:].view(torch.int32), ref.view(torch.int32))
    assert not bool((got == 0.5).any()), "the padding channel reached the output"
    assert bool((got[:t_out] == R.SENTINEL).all()) and _tail_intact(whole, R.SENTINEL) and _tail_intact(src_whole, R.SENTINEL)


def test_px_out_u8_every_bf16(lib):
    """px_out_u8_kernel over all 65 536 bf16 bit patterns in every channel (three different orders), one launch of 4 frames of
    64 x 256: bit-equal to PyTorch's float32 (x.clamp(-1, 1) * 0.5 + 0.5).clamp(0, 1) -> (v * 255.0).clamp(0, 255).to(uint8) on the CPU.
    NaN patterns are excluded from that comparison (torch's clamp propagates a NaN, whose uint8 is undefined) and pinned instead:
    the kernel's fmaxf(-1, NaN) returns -1, so every NaN, quiet or signalling, of either sign, becomes byte 0."""
    T, H, W = 4, 64, 256
    src = torch.empty(T * H * W, 4, dtype=torch.bfloat16)
    src[:, 0] = R.all_bf16_patterns()
    src[:, 1] = R.all_bf16_patterns(40503, 1)
    src[:, 2] = R.all_bf16_patterns(-1 & 0xffff, 0)
    src[:, 3] = 0.5
    src = src.view(T, H, W, 4)
    srcd, src_whole = _tailed((T, H, W, 4), torch.bfloat16, R.SENTINEL)
    srcd.copy_(src)
    out, whole = _tailed((T, H, W, 3), torch.uint8, 0xA5)
    _lib.check(lib.mmpl_vae_px_out_u8(_lib.ptr(srcd), _lib.ptr(out), T, H, W, 0, _lib.stream_ptr()), "mmpl_vae_px_out_u8")
    torch.cuda.synchronize()
    got = out.cpu()
    nan = torch.isnan(src[..., :3].float())
    assert int(nan.sum()) == 3 * 2 * 127                           # exponent 0xff, mantissa != 0, both signs
    ref = R.px_out_u8_ref(src)
    nbad = int(((got != ref) & ~nan).sum())
    print(f"px_out_u8: {nbad} of {int((~nan).sum())} non-NaN elements differ; NaN inputs give bytes {sorted(set(got[nan].tolist()))}")
    assert nbad == 0
    assert bool((got[nan] == 0).all()), "a NaN input must give byte 0"
    assert set(got[~nan].tolist()) == set(range(256))              # the inputs reach every byte value
    assert _tail_intact(whole, 0xA5) and _tail_intact(src_whole, R.SENTINEL)


def test_px_out_u8_byte_order(lib):
    """[T, H, W, 3] uint8 at frame t_out = 1, RGB within a pixel and pixels in row-major order: independent values per channel, so a
    swapped byte or pixel inside a lane's group of 4 shows; frame 0 and the tail keep the prefill."""
    T, H, W, t_out = 2, 16, 24, 1
    src = (torch.rand((T, H, W, 4), generator=R._rng("pxu8")) * 2.5 - 1.25).to(torch.bfloat16)
    srcd, _ = _tailed((T, H, W, 4), torch.bfloat16, R.SENTINEL)
    srcd.copy_(src)
    out, whole = _tailed((t_out + T, H, W, 3), torch.uint8, 0xA5)
    _lib.check(lib.mmpl_vae_px_out_u8(_lib.ptr(srcd), _lib.ptr(out), T, H, W, t_out, _lib.stream_ptr()), "mmpl_vae_px_out_u8")
    torch.cuda.synchronize()
    got = out.cpu()
    ref = R.px_out_u8_ref(src)
    assert len(set(ref.reshape(-1).tolist())) > 200
    assert torch.equal(got[t_out:], ref)
    assert bool((got[:t_out] == 0xA5).all()) and _tail_intact(whole, 0xA5)
