"""Argument checks of the kernel-level VAE / TAEHV / GEMM / attention / norm / RoPE / elementwise / umT5 and CLIP glue entry points (include/mmpl_hip.h): every rejection happens before the first HIP
call, so this file needs no GPU and no real buffer -- the pointers below are made-up, aligned addresses that nothing dereferences.
Each call is wrong in exactly one way and is matched against the message of the check that must catch it."""
import ctypes as C

import pytest

from mmpl_amd import _lib

P = 0x100000                       # a made-up 16-byte aligned "device pointer"
VP = C.c_void_p


def _err(rc):
    assert rc != 0
    return _lib.load().mmpl_last_error().decode()


def _conv(**kw):
    """mmpl_vae_conv on a valid 96 -> 96 3x3x3 halo call (To = 2, 6 x 10), with overrides."""
    a = dict(src=P, frames=None, n_frames=0, Cin=96, Hp=8, Wp=12, st=1, sy=1, sx=1, kt=3, kh=3, kw=3, W=P, Wfrag=P, bias=P, To=2, Ho=6,
             Wo=10, N=96, dst=P, Hd=6, Wd=10, ldd=96, dt0=0, dy0=0, dx0=0, res=None, ldres=0, ngamma=None, nscale=1.0, nframes=None)
    a.update(kw)
    k = C.c_int(-1)
    rc = _lib.load().mmpl_vae_conv(*a.values(), C.byref(k), None)
    return _err(rc), k.value


def _frames(n, bad=None):
    return (VP * n)(*[0 if i == bad else P + 0x1000 * i for i in range(n)])


CONV_REJECTS = [
    (dict(W=None), "null argument"), (dict(bias=None), "null argument"), (dict(src=None), "null argument"),
    (dict(dst=None), "null destination"),
    (dict(To=0), "non-positive size"), (dict(Ho=-1), "non-positive size"), (dict(Cin=0), "non-positive size"), (dict(N=0), "non-positive size"),
    (dict(kt=4), "out of range"), (dict(sy=0), "out of range"),
    (dict(Cin=48), "Cin % 32"), (dict(N=98), "N % 4"),
    (dict(Hp=7), "leave the padded source frame"), (dict(Wp=11), "leave the padded source frame"), (dict(sx=2), "leave the padded source frame"),
    (dict(To=2, Ho=1 << 16, Wo=1 << 14, Hp=(1 << 16) + 2, Wp=(1 << 14) + 2, Hd=1 << 16, Wd=1 << 14), "too many output pixels"),
    (dict(src=P + 8), "misaligned"), (dict(bias=P + 2), "misaligned"), (dict(dst=P + 4), "misaligned"),
    (dict(Hd=5), "leaves the destination frame"), (dict(dx0=1), "leaves the destination frame"), (dict(dt0=-1), "leaves the destination frame"),
    (dict(ldd=92), "ldd < N"), (dict(ldd=98), "ldd % 4"),
    (dict(res=P, ldres=64), "ldres < N"),
    (dict(frames=_frames(9), n_frames=9, To=7), "more than 8 ring frames"),
    (dict(frames=_frames(3), n_frames=3), "To + kt - 1 frames"),
    (dict(frames=_frames(4, bad=2), n_frames=4), "null or misaligned ring frame"),
    (dict(frames=_frames(4), n_frames=4, Wfrag=None), "invalid argument"),          # the launcher's own: ring slots need conv_halo_kernel
    (dict(ngamma=P, nframes=_frames(2), N=192, ldd=192), "N == 96 only"),
    (dict(ngamma=P, nframes=_frames(2), Wfrag=None), "N == 96 only"),               # conv_igemm_kernel has no fused epilogue
    (dict(ngamma=P, nframes=None), "norm frames"),
    (dict(ngamma=P, nframes=_frames(2, bad=1), dst=None), "null or misaligned norm frame"),
    (dict(ngamma=P, nframes=_frames(8), frames=None, To=9, Hd=6), "norm frames"),
]


@pytest.mark.parametrize("kw,msg", CONV_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(CONV_REJECTS)])
def test_vae_conv_rejects(kw, msg):
    text, kernel = _conv(**kw)
    assert text.startswith("mmpl_vae_conv:") and msg in text, text
    assert kernel == 0                                             # nothing was chosen, nothing was launched


def test_vae_pass_entry_points_reject():
    lib = _lib.load()
    e = lambda rc: _err(rc)
    assert "null argument" in e(lib.mmpl_vae_norm(None, 1, 3, 3, 96, None, 1.0, 0, P, 3, 3, 96, 0, 0, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_norm(P, 0, 3, 3, 96, None, 1.0, 0, P, 3, 3, 96, 0, 0, 0, None))
    assert "C % 8" in e(lib.mmpl_vae_norm(P, 1, 3, 3, 100, None, 1.0, 0, P, 3, 3, 104, 0, 0, 0, None))
    assert "C % 8" in e(lib.mmpl_vae_norm(P, 1, 3, 3, 1032, None, 1.0, 0, P, 3, 3, 1032, 0, 0, 0, None))
    assert "ldd < C" in e(lib.mmpl_vae_norm(P, 1, 3, 3, 96, None, 1.0, 0, P, 3, 3, 88, 0, 0, 0, None))
    assert "leaves the destination" in e(lib.mmpl_vae_norm(P, 1, 3, 3, 96, None, 1.0, 0, P, 4, 4, 96, 0, 2, 0, None))
    assert "misaligned" in e(lib.mmpl_vae_norm(P, 1, 3, 3, 96, P + 8, 1.0, 0, P, 3, 3, 96, 0, 0, 0, None))
    assert "too many pixels" in e(lib.mmpl_vae_norm(P, 2, 1 << 16, 1 << 14, 96, None, 1.0, 0, P, 1 << 16, 1 << 14, 96, 0, 0, 0, None))
    assert "too many pixels" in e(lib.mmpl_vae_norm(P, 1 << 30, 1 << 30, 1 << 30, 96, None, 1.0, 0, P, 1 << 30, 1 << 30, 96, 0, 0, 0, None))
    assert "null argument" in e(lib.mmpl_vae_upsample(P, 192, 192, 3, 5, 2, 0, None, 8, 12, None))
    assert "non-positive" in e(lib.mmpl_vae_upsample(P, 192, 192, 3, 0, 2, 0, P, 8, 2, None))
    assert "lds too small" in e(lib.mmpl_vae_upsample(P, 192, 192, 3, 5, 2, 1, P, 8, 12, None))
    assert "even To" in e(lib.mmpl_vae_upsample(P, 384, 192, 3, 5, 3, 1, P, 8, 12, None))
    assert "[2H + 2, 2W + 2]" in e(lib.mmpl_vae_upsample(P, 192, 192, 3, 5, 2, 0, P, 8, 11, None))
    assert "too many output pixels" in e(lib.mmpl_vae_upsample(P, 192, 192, 1 << 14, 1 << 14, 2, 0, P, (1 << 15) + 2, (1 << 15) + 2, None))
    assert "null argument" in e(lib.mmpl_vae_softmax(None, 64, P, 64, 4, 60, None))
    assert "non-positive" in e(lib.mmpl_vae_softmax(P, 64, P, 64, 0, 60, None))
    assert "ldp < cols" in e(lib.mmpl_vae_softmax(P, 64, P, 32, 4, 60, None))
    assert "null argument" in e(lib.mmpl_vae_transpose(P, 288, None, 64, 60, 96, None))
    assert "ldt < rows" in e(lib.mmpl_vae_transpose(P, 288, P, 32, 60, 96, None))
    assert "ld < C" in e(lib.mmpl_vae_transpose(P, 64, P, 64, 60, 96, None))
    f16 = (C.c_float * 16)()
    assert "null argument" in e(lib.mmpl_vae_zprep(P, 1, 4, 4, None, f16, P, P, P, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_zprep(P, 1, 4, 4, f16, f16, P, P, P, -1, None))
    assert "too many pixels" in e(lib.mmpl_vae_zprep(P, 2, 1 << 16, 1 << 14, f16, f16, P, P, P, 0, None))
    assert "null argument" in e(lib.mmpl_vae_mu_out(P, P, None, f16, f16, P, 1, 0, 4, 4, None))
    assert "non-positive" in e(lib.mmpl_vae_mu_out(P, P, P, f16, f16, P, 0, 0, 4, 4, None))
    assert "too many pixels" in e(lib.mmpl_vae_mu_out(P, P, P, f16, f16, P, 2, 0, 1 << 16, 1 << 14, None))
    # px_in(px, dst, Ttot, t0, T, H, W, dt0)
    assert "null argument" in e(lib.mmpl_vae_px_in(None, P, 5, 0, 1, 8, 8, 2, None))
    assert "null argument" in e(lib.mmpl_vae_px_in(P, None, 5, 0, 1, 8, 8, 2, None))
    assert "non-positive" in e(lib.mmpl_vae_px_in(P, P, 5, 0, 0, 8, 8, 2, None))
    assert "non-positive" in e(lib.mmpl_vae_px_in(P, P, 5, -1, 1, 8, 8, 2, None))
    assert "non-positive" in e(lib.mmpl_vae_px_in(P, P, 5, 0, 1, 8, 8, -1, None))
    assert "t0 + T > Ttot" in e(lib.mmpl_vae_px_in(P, P, 5, 2, 4, 8, 8, 2, None))
    assert "t0 + T > Ttot" in e(lib.mmpl_vae_px_in(P, P, 0x7fffffff, 0x7fffffff, 1, 8, 8, 2, None))
    assert "too many pixels" in e(lib.mmpl_vae_px_in(P, P, 5, 0, 2, 1 << 16, 1 << 14, 2, None))
    assert "misaligned" in e(lib.mmpl_vae_px_in(P + 1, P, 5, 0, 1, 8, 8, 2, None))
    # px_out(src, out, T, H, W, t_out)
    assert "null argument" in e(lib.mmpl_vae_px_out(None, P, 1, 8, 8, 0, None))
    assert "null argument" in e(lib.mmpl_vae_px_out(P, None, 1, 8, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_px_out(P, P, 1, 0, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_px_out(P, P, 1, 8, 8, -1, None))
    assert "too many pixels" in e(lib.mmpl_vae_px_out(P, P, 2, 1 << 16, 1 << 14, 0, None))
    assert "misaligned" in e(lib.mmpl_vae_px_out(P + 4, P, 1, 8, 8, 0, None))          # the [.., 4] bf16 source: 8 bytes per pixel
    assert "misaligned" in e(lib.mmpl_vae_px_out(P, P + 2, 1, 8, 8, 0, None))
    # px_out_u8(src, out, T, H, W, t_out)
    assert "null argument" in e(lib.mmpl_vae_px_out_u8(None, P, 1, 8, 8, 0, None))
    assert "null argument" in e(lib.mmpl_vae_px_out_u8(P, None, 1, 8, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_px_out_u8(P, P, 0, 8, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_vae_px_out_u8(P, P, 1, 8, 8, -1, None))
    assert "too many pixels" in e(lib.mmpl_vae_px_out_u8(P, P, 2, 1 << 16, 1 << 14, 0, None))
    assert "W % 8" in e(lib.mmpl_vae_px_out_u8(P, P, 1, 8, 12, 0, None))
    assert "W % 8" in e(lib.mmpl_vae_px_out_u8(P, P, 1, 3, 5, 0, None))
    assert "misaligned" in e(lib.mmpl_vae_px_out_u8(P + 8, P, 1, 8, 8, 0, None))       # two 16-byte loads per lane
    assert "misaligned" in e(lib.mmpl_vae_px_out_u8(P, P + 2, 1, 8, 8, 0, None))       # three dword stores per lane
    assert "null argument" in e(lib.mmpl_taehv_prep(None, P, 4, 4, None))
    assert "non-positive" in e(lib.mmpl_taehv_prep(P, P, 0, 4, None))
    assert "misaligned" in e(lib.mmpl_taehv_prep(P, P + 8, 4, 4, None))
    # taehv px_out(src, out, out_format, T, H, W, t_out)
    assert "null argument" in e(lib.mmpl_taehv_px_out(None, P, 0, 1, 8, 8, 0, None))
    assert "null argument" in e(lib.mmpl_taehv_px_out(P, None, 1, 1, 8, 8, 0, None))
    assert "unknown out_format" in e(lib.mmpl_taehv_px_out(P, P, 2, 1, 8, 8, 0, None))
    assert "unknown out_format" in e(lib.mmpl_taehv_px_out(P, P, -1, 1, 8, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_taehv_px_out(P, P, 0, 0, 8, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_taehv_px_out(P, P, 0, 1, 0, 8, 0, None))
    assert "non-positive" in e(lib.mmpl_taehv_px_out(P, P, 1, 1, 8, -3, 0, None))
    assert "non-positive" in e(lib.mmpl_taehv_px_out(P, P, 0, 1, 8, 8, -1, None))
    assert "too many pixels" in e(lib.mmpl_taehv_px_out(P, P, 0, 2, 1 << 16, 1 << 14, 0, None))
    assert "too many pixels" in e(lib.mmpl_taehv_px_out(P, P, 1, 1 << 30, 1 << 30, 1 << 30, 0, None))
    assert "misaligned" in e(lib.mmpl_taehv_px_out(P + 4, P, 0, 1, 8, 8, 0, None))      # the [.., 4] bf16 source: 8 bytes per pixel
    assert "misaligned" in e(lib.mmpl_taehv_px_out(P, P + 2, 0, 1, 8, 8, 0, None))      # float32 stores
    assert e(lib.mmpl_taehv_px_out(P, P + 2, 0, 1, 8, 8, 0, None)).startswith("mmpl_taehv_px_out:")


def _taehv(**kw):
    """mmpl_taehv_conv on a valid MemBlock first conv (64 + 64 -> 64, T = 2, 6 x 10), with overrides."""
    fs = 8 * 12 * 64
    a = dict(src0=P + 2 * fs, src1=P, fs0=fs, fs1=fs, C0=64, C1=64, up=0, ntaps=9, Wfrag=P, bias=P, Nw=64, N=64, T=2, Ho=6, Wo=10, dst=P,
             fsd=fs, ldd=64, Nsplit=64, relu=1, skip=None, fss=0, keep=None)
    a.update(kw)
    return _err(_lib.load().mmpl_taehv_conv(*a.values(), None))


TAEHV_REJECTS = [
    (dict(src0=None), "null argument"), (dict(Wfrag=None), "null argument"), (dict(dst=None), "null argument"), (dict(src1=None), "null argument"),
    (dict(T=0), "non-positive size"), (dict(Wo=0), "non-positive size"), (dict(C0=0), "non-positive size"), (dict(Nsplit=0), "non-positive size"),
    (dict(fs0=-8), "negative frame stride"), (dict(fs1=12), "multiple of the access width"),
    (dict(keep=P), "keep without skip"),
    (dict(ntaps=3), "invalid argument"), (dict(C0=48), "invalid argument"), (dict(Nw=72, N=72, ldd=72, Nsplit=72), "invalid argument"),
    (dict(Nw=128, N=128, Nsplit=96, ldd=128), "invalid argument"), (dict(N=66), "invalid argument"), (dict(N=128, ldd=128), "invalid argument"),
    (dict(up=1, Ho=7), "invalid argument"), (dict(skip=P, fss=8 * 12 * 64, N=32), "invalid argument"),
    (dict(Nw=128, N=64, Nsplit=64), "N == Nw"),
    (dict(ldd=32), "ldd smaller"),
    (dict(bias=P + 4), "misaligned"), (dict(src1=P + 8), "misaligned"),
]


@pytest.mark.parametrize("kw,msg", TAEHV_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(TAEHV_REJECTS)])
def test_taehv_conv_rejects(kw, msg):
    text = _taehv(**kw)
    assert text.startswith("mmpl_taehv_conv:") and msg in text, text


def _gemm(**kw):
    """mmpl_gemm_ex on a valid 1100 x 520 x 192 call (epi 0, no scratch), with overrides; epi 3 / 4 / 6 get their operands unless overridden."""
    a = dict(A=P, lda=192, W=P, ldw=192, bias=P, C=P, ldc=520, M=1100, N=520, K=192, epi=0, res=None, ldres=0, gate=None,
             gate_frame_stride=0, rows_per_frame=0, alpha=1.0, batch=1, sA=0, sW=0, sC=0, v_dst=None, n_v_dst=0, v_col0=0, v_ld=0,
             scratch=None, scratch_bytes=0, tile_counter=None)
    epi = kw.get("epi", 0)
    if epi in (3, 4):
        a.update(res=P, ldres=520)
    if epi == 3:
        a.update(gate=P, gate_frame_stride=520, rows_per_frame=200)
    if epi == 6:
        a.update(v_dst=_frames(6), n_v_dst=6, v_col0=256, v_ld=264, rows_per_frame=200)
    a.update(kw)
    plan = (C.c_int * 6)(*([-1] * 6))
    rc = _lib.load().mmpl_gemm_ex(*a.values(), plan, None)
    return _err(rc), list(plan)


BIG = 1 << 40
GEMM_REJECTS = [
    (dict(epi=7), "unknown epilogue"), (dict(epi=-1), "unknown epilogue"),
    (dict(A=None), "null argument"), (dict(W=None), "null argument"), (dict(C=None), "null argument"),
    (dict(epi=3, res=None), "missing epilogue operand"), (dict(epi=3, gate=None), "missing epilogue operand"),
    (dict(epi=4, res=None), "missing epilogue operand"), (dict(epi=6, v_dst=None), "missing epilogue operand"),
    (dict(M=0), "non-positive size"), (dict(N=0), "non-positive size"), (dict(K=0), "non-positive size"),
    (dict(K=96), "K % 64"), (dict(N=518), "N % 4"),
    (dict(lda=196), "lda % 8"), (dict(lda=184), "lda < K"), (dict(ldw=196), "ldw % 8"), (dict(ldw=128), "ldw < K"),
    (dict(batch=0), "batch < 1"), (dict(batch=65536), "batch > 65535"),
    (dict(ldc=522), "ldc % 4"), (dict(ldc=516), "ldc < N"),
    (dict(epi=5), "takes no bias"),
    (dict(epi=4, ldres=516), "ldres < N"), (dict(epi=4, ldres=522), "ldres % 4"),
    (dict(epi=3, rows_per_frame=0), "rows_per_frame < 1"), (dict(epi=6, rows_per_frame=0), "rows_per_frame < 1"),
    (dict(epi=3, gate_frame_stride=-520), "gate_frame_stride < 0"), (dict(epi=3, gate_frame_stride=522), "gate_frame_stride % 4"),
    (dict(epi=3, gate_frame_stride=516), "gate_frame_stride < N with more than one frame"),
    (dict(A=P + 8), "A not 16-byte"), (dict(W=P + 8), "W not 16-byte"), (dict(C=P + 4), "C not 8-byte"),
    (dict(epi=5, bias=None, C=P + 8), "fp32 C not 16-byte"),
    (dict(bias=P + 4), "bias not 8-byte"), (dict(epi=4, res=P + 4), "res not 8-byte"), (dict(epi=3, gate=P + 4), "gate not 8-byte"),
    (dict(epi=4, batch=2), "no residual and no pages"), (dict(epi=6, batch=2), "no residual and no pages"),
    (dict(batch=2, sA=-8), "negative batch stride"), (dict(batch=2, sW=-8), "negative batch stride"), (dict(batch=2, sC=-4), "negative batch stride"),
    (dict(batch=2, sA=4), "sA % 8"), (dict(batch=2, sW=4), "sW % 8"), (dict(batch=2, sC=6), "sC % 4"),
    (dict(epi=6, n_v_dst=0), "n_v_dst < 1"), (dict(epi=6, v_dst=_frames(9), n_v_dst=9), "more than 8 pages"),
    (dict(epi=6, v_dst=_frames(5), n_v_dst=5), "fewer than M rows"),
    (dict(epi=6, v_col0=258), "v_col0 % 4"), (dict(epi=6, v_col0=0), "v_col0 outside"), (dict(epi=6, v_col0=520), "v_col0 outside"),
    (dict(epi=6, v_ld=260), "v_ld < N - v_col0"), (dict(epi=6, v_ld=266), "v_ld % 4"),
    (dict(epi=6, v_dst=_frames(6, bad=3)), "null page"),
    (dict(epi=6, v_dst=(VP * 6)(*[P + 0x10000 * i + (4 if i == 2 else 0) for i in range(6)])), "page not 8-byte"),
    (dict(scratch=P, scratch_bytes=4096), "scratch smaller"), (dict(scratch=P + 128, scratch_bytes=BIG), "256-byte aligned"),
    (dict(tile_counter=P + 2), "tile_counter not 4-byte"),
]


@pytest.mark.parametrize("kw,msg", GEMM_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(GEMM_REJECTS)])
def test_gemm_ex_rejects(kw, msg):
    text, plan = _gemm(**kw)
    assert text.startswith("mmpl_gemm_ex:") and msg in text, text
    assert plan == [0] * 6                                         # no plan was made, nothing was launched


def _pages(n, bad=None, off=0):
    return (VP * max(n, 1))(*[0 if i == bad else P + 0x10000 * i + (off if i == 1 else 0) for i in range(max(n, 1))])


def _attn(**kw):
    """mmpl_attn_fwd_ex on a valid 2-head, 3-page w64 call (variant 3, no workspace), with overrides."""
    a = dict(q=P, ldq=256, o=P, ldo=256, k_pages=_pages(3), v_pages=_pages(3), page_group=None, ldk=256, ldv=256, n_pages=3, page_rows=72,
             Lq=300, num_heads=2, softmax_scale=0.6931472, workspace=None, workspace_bytes=0, variant=3, q_prescaled=0, cross=0,
             last_row_copies=0, history=None, stats_dev=None)
    a.update(kw)
    plan = (C.c_int * 8)(*([-1] * 8))
    rc = _lib.load().mmpl_attn_fwd_ex(*a.values(), plan, None)
    return _err(rc), list(plan)


ATTN_REJECTS = [
    (dict(q=None), "null argument"), (dict(o=None), "null argument"), (dict(k_pages=None), "null argument"), (dict(v_pages=None), "null argument"),
    (dict(n_pages=0), "n_pages < 1"), (dict(n_pages=25, k_pages=_pages(25), v_pages=_pages(25)), "more than 24 pages"),
    (dict(page_rows=0), "non-positive size"), (dict(Lq=0), "non-positive size"), (dict(num_heads=0), "non-positive size"),
    (dict(softmax_scale=0.0), "softmax_scale"), (dict(softmax_scale=float("nan")), "softmax_scale"), (dict(softmax_scale=float("inf")), "softmax_scale"),
    (dict(variant=2), "unknown kernel variant"), (dict(variant=5), "unknown kernel variant"), (dict(variant=-1), "unknown kernel variant"),
    (dict(ldq=260), "ldq % 8"), (dict(ldo=260), "ldo % 8"), (dict(ldk=260), "ldk % 8"), (dict(ldv=260), "ldv % 8"),
    (dict(ldq=128), "ldq < 128 * num_heads"), (dict(ldo=128), "ldo < 128 * num_heads"), (dict(ldk=128), "ldk < 128 * num_heads"),
    (dict(ldv=128), "ldv < 128 * num_heads"),
    (dict(q=P + 8), "q not 16-byte"), (dict(o=P + 8), "o not 16-byte"),
    (dict(last_row_copies=-1), "last_row_copies < 0"),
    (dict(workspace=P + 8, workspace_bytes=BIG), "workspace not 16-byte"), (dict(history=P + 1), "history not 2-byte"),
    (dict(stats_dev=P + 4), "stats not 8-byte"),
    (dict(k_pages=_pages(3, bad=1)), "null page"), (dict(v_pages=_pages(3, bad=2)), "null page"),
    (dict(k_pages=_pages(3, off=8)), "page not 16-byte"), (dict(v_pages=_pages(3, off=8)), "page not 16-byte"),
    (dict(variant=1, q_prescaled=1), "prescaled q"), (dict(variant=0, q_prescaled=1, cross=1), "prescaled q"),
    (dict(variant=3, last_row_copies=2, n_pages=1), "lock-step kernel only"), (dict(variant=4, last_row_copies=448, n_pages=1), "lock-step kernel only"),
    (dict(variant=1, last_row_copies=2), "more than one page"),
]


@pytest.mark.parametrize("kw,msg", ATTN_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(ATTN_REJECTS)])
def test_attn_fwd_ex_rejects(kw, msg):
    text, plan = _attn(**kw)
    assert text.startswith("mmpl_attn_fwd_ex:") and msg in text, text
    assert plan == [0] * 8                                         # no plan was made, nothing was launched


def test_attn_entries_keep_their_checks():
    """mmpl_attn_fwd_variant / _history reject as before."""
    lib = _lib.load()
    pg = _pages(3)
    assert "mmpl_attn_fwd: n_pages out of range" in _err(lib.mmpl_attn_fwd_variant(P, 256, P, 256, pg, pg, 256, 256, 0, 72, 300, 2, 0.5, None, 0, 0, 0, None))
    assert "mmpl_attn_fwd: unknown kernel variant" in _err(lib.mmpl_attn_fwd_variant(P, 256, P, 256, pg, pg, 256, 256, 3, 72, 300, 2, 0.5, None, 0, 2, 0, None))
    assert "mmpl_attn_fwd_history: stats must be 8-byte aligned" in _err(lib.mmpl_attn_fwd_history(P, 256, P, 256, pg, pg, 256, 256, 3, 72, 300, 2, 0.5, None, 0, None, P + 4, None))


def test_gemm_entries_keep_their_checks():
    """mmpl_gemm / _tickets / _scratch still reject the page epilogue (6) and report as before."""
    lib = _lib.load()
    assert "mmpl_gemm: unknown epilogue" in _err(lib.mmpl_gemm(P, 192, P, 192, P, P, 520, 1100, 520, 192, 6, None, 0, None, 0, 0, None))
    assert "mmpl_gemm: missing epilogue operand" in _err(lib.mmpl_gemm_tickets(P, 192, P, 192, P, P, 520, 1100, 520, 192, 4, None, 0, None, 0, 0, None, None))
    assert "mmpl_gemm_scratch: scratch missing" in _err(lib.mmpl_gemm_scratch(P, 192, P, 192, P, P, 520, 1100, 520, 192, 0, None, 0, None, 0, 0, None, 0, None))


def _ln(**kw):
    """mmpl_layernorm_ex on a valid 50 x 3072 modulation call (2 frames of 25 rows, the forward's 6 d layout), with overrides."""
    a = dict(x=P, ldx=3072, y=P, ldy=3072, rows=50, d=3072, eps=1e-6, scale=P + 2 * 3072, shift=P, mod_frame_stride=6 * 3072,
             rows_per_frame=25, w=None, b=None, pipeline=-1, groups_per_block=0)
    a.update(kw)
    plan = (C.c_int * 7)(*([-1] * 7))
    rc = _lib.load().mmpl_layernorm_ex(*a.values(), plan, None)
    return _err(rc), list(plan)


LN_REJECTS = [
    (dict(x=None), "null argument"), (dict(y=None), "null argument"),
    (dict(scale=None), "need (scale, shift) or (w, b)"), (dict(shift=None), "need (scale, shift) or (w, b)"), (dict(w=P), "w without b"),
    (dict(rows=0), "non-positive size"), (dict(rows=-4), "non-positive size"), (dict(d=0), "non-positive size"),
    (dict(d=3076, ldx=3080, ldy=3080), "d % 8"), (dict(d=5128, ldx=5128, ldy=5128), "d > 5120"),
    (dict(ldx=3076), "ldx % 8"), (dict(ldx=3064), "ldx < d"), (dict(ldy=3076), "ldy % 8"), (dict(ldy=3064), "ldy < d"),
    (dict(rows_per_frame=0), "rows_per_frame < 1"), (dict(mod_frame_stride=-8), "mod_frame_stride < 0"),
    (dict(mod_frame_stride=3076), "mod_frame_stride % 8"),
    (dict(x=P + 8), "x not 16-byte"), (dict(y=P + 8), "y not 16-byte"), (dict(scale=P + 8), "column vector not 16-byte"),
    (dict(shift=P + 4), "column vector not 16-byte"), (dict(w=P, b=P + 8), "column vector not 16-byte"),
    (dict(w=P + 2, b=P), "column vector not 16-byte"),
    (dict(pipeline=2), "pipeline outside"), (dict(pipeline=-2), "pipeline outside"),
    (dict(pipeline=1, d=2560, ldx=2560, ldy=2560), "from NIT 6"), (dict(pipeline=1, d=8, ldx=8, ldy=8), "from NIT 6"),
    (dict(groups_per_block=-1), "groups_per_block < 0"),
    (dict(groups_per_block=3), "one-row-per-wave kernel"), (dict(pipeline=0, groups_per_block=3), "one-row-per-wave kernel"),
]


@pytest.mark.parametrize("kw,msg", LN_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(LN_REJECTS)])
def test_layernorm_ex_rejects(kw, msg):
    text, plan = _ln(**kw)
    assert text.startswith("mmpl_layernorm_ex:") and msg in text, text
    assert plan == [0] * 7                                         # no plan was reported, nothing was launched


def _qk(**kw):
    """mmpl_qknorm_ex on a valid forward-form call (q, k in a [30, 3 d] matrix, 2 frames of a 3 x 5 grid, d = 1536), with overrides."""
    d = 1536
    a = dict(q=P, ldq=3 * d, k=P + 2 * d, ldk=3 * d, v=None, ldv=0, wq=P, wk=P, rows=30, d=d, eps=1e-6, q_scale=0.125, rope=1, cos_tab=P,
             sin_tab=P, n_frames=2, frame_ids=(C.c_int * 8)(), frame_base_dev=None, k_dst=_frames(2), v_dst=None, rows_per_frame=15,
             grid_w=5, groups_per_block=0)
    a.update(kw)
    plan = (C.c_int * 7)(*([-1] * 7))
    rc = _lib.load().mmpl_qknorm_ex(*a.values(), plan, None)
    return _err(rc), list(plan)


_V = dict(v=P + 4 * 1536, ldv=3 * 1536, v_dst=_frames(2))
QK_REJECTS = [
    (dict(q=None), "null argument"), (dict(wq=None), "null argument"),
    (dict(_V, k=None), "v without k"), (dict(wk=None), "k without wk or k_dst"), (dict(k_dst=None), "k without wk or k_dst"),
    (dict(_V, v_dst=None), "v without v_dst"),
    (dict(rows=0, n_frames=1, rows_per_frame=0), "non-positive size"), (dict(d=0), "non-positive size"),
    (dict(d=1544), "d % 128"), (dict(d=5248, ldq=3 * 5248, ldk=3 * 5248), "d > 5120"),
    (dict(ldq=4612), "ldq % 8"), (dict(ldq=1528), "ldq < d"), (dict(ldk=4612), "ldk % 8"), (dict(ldk=1528), "ldk < d"),
    (dict(_V, ldv=4612), "ldv % 8"), (dict(_V, ldv=1528), "ldv < d"),
    (dict(q=P + 8), "q not 16-byte"), (dict(k=P + 8), "k not 16-byte"), (dict(_V, v=P + 8), "v not 16-byte"),
    (dict(wq=P + 8), "gain not 16-byte"), (dict(wk=P + 4), "gain not 16-byte"),
    (dict(n_frames=0), "n_frames outside"), (dict(n_frames=9, rows=135), "n_frames outside"),
    (dict(cos_tab=None), "rope without tables"), (dict(sin_tab=None), "rope without tables"), (dict(frame_ids=None), "rope without tables"),
    (dict(cos_tab=P + 2), "not 4-byte aligned"), (dict(frame_base_dev=P + 2), "not 4-byte aligned"),
    (dict(rows_per_frame=0), "rows_per_frame < 1"),
    (dict(rows=31), "rows != n_frames * rows_per_frame"), (dict(rows_per_frame=16), "rows != n_frames * rows_per_frame"),
    (dict(grid_w=0), "grid_w < 1"), (dict(grid_w=1025), "grid_w > 1024"),
    (dict(rows=2050, rows_per_frame=1025, grid_w=1), "more than 1024 grid rows"),
    (dict(groups_per_block=-1), "groups_per_block < 0"),
    (dict(k_dst=_frames(2, bad=1)), "null page"), (dict(_V, v_dst=_frames(2, bad=0)), "null page"),
    (dict(k_dst=(VP * 2)(P, P + 0x1008)), "page not 16-byte"), (dict(_V, v_dst=(VP * 2)(P + 8, P + 0x1000)), "page not 16-byte"),
    (dict(rope=0, k_dst=_frames(1, bad=0)), "null page"),
]


@pytest.mark.parametrize("kw,msg", QK_REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(QK_REJECTS)])
def test_qknorm_ex_rejects(kw, msg):
    text, plan = _qk(**kw)
    assert text.startswith("mmpl_qknorm_ex:") and msg in text, text
    assert plan == [0] * 7                                         # no plan was reported, nothing was launched


def test_small_elementwise_entry_points_reject():
    lib = _lib.load()
    e = lambda rc: _err(rc)
    d = 256
    assert "mmpl_modulation: null argument" in e(lib.mmpl_modulation(None, 6 * d, P, 6 * d, 0, P, 2, 3, 6, d, None))
    assert "null argument" in e(lib.mmpl_modulation(P, 6 * d, None, 6 * d, 0, P, 2, 3, 6, d, None))
    assert "null argument" in e(lib.mmpl_modulation(P, 6 * d, P, 6 * d, 0, None, 2, 3, 6, d, None))
    assert "non-positive" in e(lib.mmpl_modulation(P, 6 * d, P, 6 * d, 0, P, 0, 3, 6, d, None))
    assert "non-positive" in e(lib.mmpl_modulation(P, 6 * d, P, 6 * d, 0, P, 2, 3, 6, 0, None))
    assert "negative stride" in e(lib.mmpl_modulation(P, -6 * d, P, 6 * d, 0, P, 2, 3, 6, d, None))
    assert "negative stride" in e(lib.mmpl_modulation(P, 6 * d, P, -d, 0, P, 2, 3, 6, d, None))
    assert "too many elements" in e(lib.mmpl_modulation(P, 6 * d, P, 6 * d, 0, P, 1 << 12, 1 << 12, 1 << 8, d, None))
    assert "misaligned" in e(lib.mmpl_modulation(P + 1, 6 * d, P, 6 * d, 0, P, 2, 3, 6, d, None))
    assert "mmpl_patchify: null argument" in e(lib.mmpl_patchify(None, P, 64, 3, 16, 6, 10, None))
    assert "non-positive" in e(lib.mmpl_patchify(P, P, 64, 0, 16, 6, 10, None))
    assert "odd h or w" in e(lib.mmpl_patchify(P, P, 64, 3, 16, 7, 10, None))
    assert "odd h or w" in e(lib.mmpl_patchify(P, P, 64, 3, 16, 6, 9, None))
    assert "lda < 4 C" in e(lib.mmpl_patchify(P, P, 63, 3, 16, 6, 10, None))
    assert "too many pixels" in e(lib.mmpl_patchify(P, P, 64, 2, 16, 1 << 16, 1 << 14, None))
    assert "misaligned" in e(lib.mmpl_patchify(P, P + 1, 64, 3, 16, 6, 10, None))
    assert "mmpl_unpatchify: null argument" in e(lib.mmpl_unpatchify(P, 64, None, 3, 16, 6, 10, None))
    assert "non-positive" in e(lib.mmpl_unpatchify(P, 64, P, 3, 0, 6, 10, None))
    assert "odd h or w" in e(lib.mmpl_unpatchify(P, 64, P, 3, 16, 6, 11, None))
    assert "ldy < 4 C" in e(lib.mmpl_unpatchify(P, 60, P, 3, 16, 6, 10, None))
    assert "too many pixels" in e(lib.mmpl_unpatchify(P, 64, P, 2, 16, 1 << 16, 1 << 14, None))
    assert "misaligned" in e(lib.mmpl_unpatchify(P + 1, 64, P, 3, 16, 6, 10, None))
    assert "mmpl_sinusoid: null argument" in e(lib.mmpl_sinusoid(None, P, 4, 256, None))
    assert "non-positive" in e(lib.mmpl_sinusoid(P, P, 0, 256, None))
    assert "non-positive" in e(lib.mmpl_sinusoid(P, P, 4, 0, None))
    assert "odd freq_dim" in e(lib.mmpl_sinusoid(P, P, 4, 255, None))
    assert "too many elements" in e(lib.mmpl_sinusoid(P, P, 1 << 24, 256, None))
    assert "misaligned" in e(lib.mmpl_sinusoid(P + 2, P, 4, 256, None))
    assert "mmpl_silu: null argument" in e(lib.mmpl_silu(P, None, 16, None))
    assert "non-positive" in e(lib.mmpl_silu(P, P, 0, None))
    assert "misaligned" in e(lib.mmpl_silu(P + 1, P, 16, None))
    assert "mmpl_rows_equal_last: null argument" in e(lib.mmpl_rows_equal_last(P, 4104, 5, 4096, None, None))
    assert "rows < 1" in e(lib.mmpl_rows_equal_last(P, 4104, 0, 4096, P, None))
    assert "non-positive" in e(lib.mmpl_rows_equal_last(P, 4104, 5, 0, P, None))
    assert "d % 8" in e(lib.mmpl_rows_equal_last(P, 4104, 5, 4092, P, None))
    assert "ld % 8" in e(lib.mmpl_rows_equal_last(P, 4100, 5, 4096, P, None))
    assert "ld < d" in e(lib.mmpl_rows_equal_last(P, 4088, 5, 4096, P, None))
    assert "misaligned" in e(lib.mmpl_rows_equal_last(P + 8, 4104, 5, 4096, P, None))
    assert "misaligned" in e(lib.mmpl_rows_equal_last(P, 4104, 5, 4096, P + 2, None))


def test_norm_entries_keep_their_checks():
    """mmpl_layernorm rejects as before."""
    assert "mmpl_layernorm: need (scale, shift) or (w, b)" in _err(_lib.load().mmpl_layernorm(P, 256, P, 256, 4, 256, 1e-6, None, None, 0, 1, None, None, None))


def test_glue_entry_points_reject():
    """mmpl_t5_gather / _softmax / _transpose / _gated / _zero_pad, mmpl_gelu_erf, mmpl_add: every check, one wrong thing per call."""
    lib = _lib.load()
    e = lambda rc: _err(rc)
    assert "mmpl_t5_gather: null argument" in e(lib.mmpl_t5_gather(None, P, P, 64, 128, None))
    assert "null argument" in e(lib.mmpl_t5_gather(P, None, P, 64, 128, None))
    assert "null argument" in e(lib.mmpl_t5_gather(P, P, None, 64, 128, None))
    assert "non-positive" in e(lib.mmpl_t5_gather(P, P, P, 0, 128, None))
    assert "non-positive" in e(lib.mmpl_t5_gather(P, P, P, 64, -8, None))
    assert "dim % 8" in e(lib.mmpl_t5_gather(P, P, P, 64, 132, None))
    assert "emb not 16-byte" in e(lib.mmpl_t5_gather(P, P + 8, P, 64, 128, None))
    assert "out not 16-byte" in e(lib.mmpl_t5_gather(P, P, P + 2, 64, 128, None))
    assert "ids not 4-byte" in e(lib.mmpl_t5_gather(P + 2, P, P, 64, 128, None))
    assert "mmpl_t5_softmax: null argument" in e(lib.mmpl_t5_softmax(None, P, P, P, P, 3, 64, None))
    assert "null argument" in e(lib.mmpl_t5_softmax(P, None, P, P, P, 3, 64, None))
    assert "null argument" in e(lib.mmpl_t5_softmax(P, P, None, P, P, 3, 64, None))
    assert "null argument" in e(lib.mmpl_t5_softmax(P, P, P, None, P, 3, 64, None))
    assert "null argument" in e(lib.mmpl_t5_softmax(P, P, P, P, None, 3, 64, None))
    assert "non-positive" in e(lib.mmpl_t5_softmax(P, P, P, P, P, 0, 64, None))
    assert "non-positive" in e(lib.mmpl_t5_softmax(P, P, P, P, P, 3, 0, None))
    assert "L % 64" in e(lib.mmpl_t5_softmax(P, P, P, P, P, 3, 96, None))
    assert "exceeds the grid" in e(lib.mmpl_t5_softmax(P, P, P, P, P, 1 << 16, 1 << 15, None))
    assert "not 4-byte" in e(lib.mmpl_t5_softmax(P + 2, P, P, P, P, 3, 64, None))
    assert "not 4-byte" in e(lib.mmpl_t5_softmax(P, P, P + 2, P, P, 3, 64, None))
    assert "not 4-byte" in e(lib.mmpl_t5_softmax(P, P, P, P + 1, P, 3, 64, None))
    assert "not 2-byte" in e(lib.mmpl_t5_softmax(P, P + 1, P, P, P, 3, 64, None))
    assert "not 2-byte" in e(lib.mmpl_t5_softmax(P, P, P, P, P + 1, 3, 64, None))
    assert "mmpl_t5_transpose: null argument" in e(lib.mmpl_t5_transpose(None, 192, P, 64, 64, 3, None))
    assert "null argument" in e(lib.mmpl_t5_transpose(P, 192, None, 64, 64, 3, None))
    assert "non-positive" in e(lib.mmpl_t5_transpose(P, 192, P, 0, 64, 3, None))
    assert "non-positive" in e(lib.mmpl_t5_transpose(P, 192, P, 64, 0, 3, None))
    assert "non-positive" in e(lib.mmpl_t5_transpose(P, 192, P, 64, 64, 0, None))
    assert "ld < H * c" in e(lib.mmpl_t5_transpose(P, 191, P, 64, 64, 3, None))
    assert "ld < H * c" in e(lib.mmpl_t5_transpose(P, 1 << 30, P, 64, 1 << 20, 1 << 12, None))
    assert "exceeds the grid" in e(lib.mmpl_t5_transpose(P, 1 << 30, P, 64, 64, 1 << 16, None))
    assert "exceeds the grid" in e(lib.mmpl_t5_transpose(P, 1 << 30, P, 64, 1 << 22, 2, None))
    assert "misaligned" in e(lib.mmpl_t5_transpose(P + 1, 192, P, 64, 64, 3, None))
    assert "misaligned" in e(lib.mmpl_t5_transpose(P, 192, P + 1, 64, 64, 3, None))
    assert "mmpl_t5_gated: null argument" in e(lib.mmpl_t5_gated(None, P, 16, None))
    assert "null argument" in e(lib.mmpl_t5_gated(P, None, 16, None))
    assert "non-positive" in e(lib.mmpl_t5_gated(P, P, 0, None))
    assert "misaligned" in e(lib.mmpl_t5_gated(P + 1, P, 16, None))
    assert "misaligned" in e(lib.mmpl_t5_gated(P, P + 1, 16, None))
    assert "mmpl_t5_zero_pad: null argument" in e(lib.mmpl_t5_zero_pad(None, P, 64, 128, None))
    assert "null argument" in e(lib.mmpl_t5_zero_pad(P, None, 64, 128, None))
    assert "non-positive" in e(lib.mmpl_t5_zero_pad(P, P, 0, 128, None))
    assert "non-positive" in e(lib.mmpl_t5_zero_pad(P, P, 64, 0, None))
    assert "out not 2-byte" in e(lib.mmpl_t5_zero_pad(P + 1, P, 64, 128, None))
    assert "mask not 4-byte" in e(lib.mmpl_t5_zero_pad(P, P + 2, 64, 128, None))
    assert "mmpl_gelu_erf: null argument" in e(lib.mmpl_gelu_erf(None, 16, None))
    assert "non-positive" in e(lib.mmpl_gelu_erf(P, 0, None))
    assert "misaligned" in e(lib.mmpl_gelu_erf(P + 1, 16, None))
    assert "mmpl_add: null argument" in e(lib.mmpl_add(None, P, 16, None))
    assert "null argument" in e(lib.mmpl_add(P, None, 16, None))
    assert "non-positive" in e(lib.mmpl_add(P, P, 0, None))
    assert "misaligned" in e(lib.mmpl_add(P + 1, P, 16, None))
    assert "misaligned" in e(lib.mmpl_add(P, P + 1, 16, None))


def test_unipc_entries_reject_null_tensors():
    """mmpl_cfg_unipc_step / _table: a null flow_cond, x, m0, m1 or last_sample is rejected before the launch (flow_uncond may be NULL)."""
    lib = _lib.load()
    st = _lib.MmplUniPCStep()
    for bad in (0, 2, 3, 4, 5):
        a = [P] * 6
        a[bad] = None
        assert "mmpl_cfg_unipc_step: null argument" in _err(lib.mmpl_cfg_unipc_step(*a, 16, C.byref(st), None))
        assert "mmpl_cfg_unipc_step_table: null argument" in _err(lib.mmpl_cfg_unipc_step_table(*a, 16, P, P, P, P, 1, 50, None))
    assert "null step" in _err(lib.mmpl_cfg_unipc_step(*[P] * 6, 16, None, None))
    assert "bad arguments" in _err(lib.mmpl_cfg_unipc_step_table(*[P] * 6, 16, None, P, P, P, 1, 50, None))
