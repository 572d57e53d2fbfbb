#!/usr/bin/env python3
"""Micro-benchmarks of the two MFMA kernels on the 14B/720p shapes (dev tool).
    python tools/bench_kernels.py attn|gemm|all|gemmref|attnref|elem|cross [--iters N]
    python tools/bench_kernels.py taehv [--iters N] [--out FILE]     # the TAEHV preview decoder against the Wan VAE's streamed decode
    python tools/bench_kernels.py taehvenc [--iters N] [--out FILE]  # the TAEHV encoder against the Wan VAE's encode"""
import ctypes as C
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmpl_amd import _lib  # noqa: E402

lib = _lib.load()
dev = "cuda:0"
BF = torch.bfloat16


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench_attn(iters):
    H, S, d = 40, 3600, 5120
    n_slots = 21
    kc = torch.randn(n_slots * S, d, device=dev).to(BF)
    vc = torch.randn(n_slots * S, d, device=dev).to(BF)
    for name, nq, npg in (("s0", 2, 2), ("s1", 7, 9), ("s2", 6, 13), ("s3", 6, 21), ("cross", 7, 0)):
        Lq = nq * S
        q = torch.randn(Lq, 3 * d, device=dev).to(BF)
        o = torch.empty(Lq, d, device=dev, dtype=BF)
        if npg == 0:
            pr, npg_ = 512, 1
        else:
            pr, npg_ = S, npg
        kp = (C.c_void_p * npg_)(*[kc[i * S:].data_ptr() for i in range(npg_)])
        vp = (C.c_void_p * npg_)(*[vc[i * S:].data_ptr() for i in range(npg_)])
        fn = lambda: _lib.check(lib.mmpl_attn_fwd(_lib.ptr(q), 3 * d, _lib.ptr(o), d, kp, vp, d, d, npg_, pr, Lq, H,
                                                  1 / math.sqrt(128), _lib.stream_ptr()))
        ms = timeit(fn, iters)
        fl = 4.0 * Lq * npg_ * pr * d
        print(f"attn {name}: Lq={Lq} Lkv={npg_ * pr}  {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TFLOP/s", flush=True)


def bench_attn_ref(iters):
    """yardstick only (never on the product path): PyTorch-ROCm's scaled_dot_product_attention (its flash / memory-efficient backends:
    AOTriton / CK as the wheel was built) on the self-attention shapes of the 14B / 720p stages, K / V gathered CONTIGUOUS (what the
    reference materialises per layer before calling flash-attn, causal_fps_model.py:219-227) -- the gather itself is not timed.
    Next to it: mmpl_attn_fwd on the same q / k / v values (paged, in place)."""
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel
    H, S, d = 40, 3600, 5120
    for name, nq, nkv in (("s0", 2, 2), ("s1", 7, 9), ("s2", 6, 13), ("s3", 6, 21)):
        Lq, Lkv = nq * S, nkv * S
        q = torch.randn(Lq, d, device=dev).to(BF)
        k = torch.randn(Lkv, d, device=dev).to(BF)
        v = torch.randn(Lkv, d, device=dev).to(BF)
        fl = 4.0 * Lq * Lkv * d
        o = torch.empty(Lq, d, device=dev, dtype=BF)
        kp = (C.c_void_p * nkv)(*[k[i * S:].data_ptr() for i in range(nkv)])
        vp = (C.c_void_p * nkv)(*[v[i * S:].data_ptr() for i in range(nkv)])
        ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
        fn = lambda: _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o), d, kp, vp, d, d, nkv, S, Lq, H, 1 / math.sqrt(128),
                                                          _lib.ptr(ws), ws.numel(), 3, 0, _lib.stream_ptr()))
        ms = min(timeit(fn, iters), timeit(fn, iters))
        print(f"attnref {name}: Lq={Lq} Lkv={Lkv}  mmpl attn_w64 (paged, raw q) {ms:8.3f} ms  {fl / ms / 1e9:8.1f} TFLOP/s", flush=True)
        # [B=1, H, L, 128] views of the token-major tensors (what flash-attn style kernels take) and head-major contiguous copies
        for layout in ("token-major views", "head-major contiguous"):
            q4, k4, v4 = (t.view(1, -1, H, 128).transpose(1, 2) for t in (q, k, v))
            if layout.startswith("head"):
                q4, k4, v4 = q4.contiguous(), k4.contiguous(), v4.contiguous()
            for be in (SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION):
                try:
                    with sdpa_kernel([be]):
                        f2 = lambda: F.scaled_dot_product_attention(q4, k4, v4)
                        ref = f2()
                        ms2 = min(timeit(f2, iters), timeit(f2, iters))
                    err = ((ref.transpose(1, 2).reshape(Lq, d).float() - o.float()).norm() / o.float().norm()).item()
                    print(f"attnref {name}: torch SDPA {be.name:22s} {layout:22s} {ms2:8.3f} ms  {fl / ms2 / 1e9:8.1f} TFLOP/s   (rel-L2 vs mmpl {err:.2e})", flush=True)
                    del ref
                except Exception as e:
                    print(f"attnref {name}: torch SDPA {be.name} {layout}: unavailable ({str(e).splitlines()[0][:120]})", flush=True)
            del q4, k4, v4
        del q, k, v, o


def bench_gemm(iters):
    m_big = int(os.environ.get("BENCH_M", "25200"))          # the stage's query rows: 25200 (s1), 21600 (s2, s3)
    shapes = (("qkv", m_big, 15360, 5120, 0), ("o", m_big, 5120, 5120, 3), ("ffn0", m_big, 13824, 5120, 1),
              ("ffn2", m_big, 5120, 13824, 3), ("qkv_s0", 7200, 15360, 5120, 0), ("sq8k", 8192, 8192, 8192, 0))
    if os.environ.get("BENCH_SHAPES"):                       # "name:M:N:K:epi,..." (e.g. the 1.3B / 480p block shapes)
        shapes = tuple((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])) for f in (x.split(":") for x in os.environ["BENCH_SHAPES"].split(",")))
    for name, M, N, K, epi in shapes:
        # BENCH_PAD_K / BENCH_PAD_N: extra elements in the leading dimension of the K-contiguous operands / of C and the residual
        # (dev: does the power-of-two-ish row stride camp on a few HBM channels?)
        pk, pn = int(os.environ.get("BENCH_PAD_K", "0")), int(os.environ.get("BENCH_PAD_N", "0"))
        A = torch.randn(M, K + pk, device=dev).to(BF)
        W = (torch.randn(N, K + pk, device=dev) / math.sqrt(K)).to(BF)
        b = torch.randn(N, device=dev).to(BF)
        Cc = torch.empty(M, N + pn, device=dev, dtype=BF)
        res = torch.randn(M, N + pn, device=dev).to(BF)
        gate = torch.randn(8, N, device=dev).to(BF)
        fn = lambda: _lib.check(lib.mmpl_gemm(_lib.ptr(A), K + pk, _lib.ptr(W), K + pk, _lib.ptr(b), _lib.ptr(Cc), N + pn, M, N, K, epi, _lib.ptr(res),
                                              N + pn, _lib.ptr(gate), N, 3600, _lib.stream_ptr()))
        ctr = torch.zeros(8, dtype=torch.int32, device=dev)
        fn_t = lambda: _lib.check(lib.mmpl_gemm_tickets(_lib.ptr(A), K + pk, _lib.ptr(W), K + pk, _lib.ptr(b), _lib.ptr(Cc), N + pn, M, N, K, epi, _lib.ptr(res),
                                                        N + pn, _lib.ptr(gate), N, 3600, _lib.ptr(ctr), _lib.stream_ptr()))
        nb = lib.mmpl_gemm_scratch_bytes()
        scratch = torch.zeros(nb, dtype=torch.uint8, device=dev)
        fn_s = lambda: _lib.check(lib.mmpl_gemm_scratch(_lib.ptr(A), K + pk, _lib.ptr(W), K + pk, _lib.ptr(b), _lib.ptr(Cc), N + pn, M, N, K, epi, _lib.ptr(res),
                                                        N + pn, _lib.ptr(gate), N, 3600, _lib.ptr(scratch), nb, _lib.stream_ptr()))
        ms, ms_t, ms_s = timeit(fn, iters), timeit(fn_t, iters), timeit(fn_s, iters)
        ms2, ms_t2, ms_s2 = timeit(fn, iters), timeit(fn_t, iters), timeit(fn_s, iters)
        ms, ms_t, ms_s = min(ms, ms2), min(ms_t, ms_t2), min(ms_s, ms_s2)
        print(f"gemm {name}: M={M} N={N} K={K} epi={epi}  {ms:8.3f} ms  {2.0 * M * N * K / ms / 1e9:8.1f} TFLOP/s   |  tile tickets {ms_t:8.3f} ms  "
              f"{2.0 * M * N * K / ms_t / 1e9:8.1f} TFLOP/s   |  + split-K tail {ms_s:8.3f} ms  {2.0 * M * N * K / ms_s / 1e9:8.1f} TFLOP/s", flush=True)


def bench_gemm_ref(iters):
    """yardstick only (never on the product path): the vendor library (torch.matmul -> hipBLASLt / rocBLAS) on the same shapes
    and the same random operands, plain C = A W^T without bias / epilogue"""
    shapes = (("qkv", 25200, 15360, 5120), ("o", 25200, 5120, 5120), ("ffn0", 25200, 13824, 5120), ("ffn2", 25200, 5120, 13824),
              ("qkv_s0", 7200, 15360, 5120), ("sq8k", 8192, 8192, 8192))
    if os.environ.get("BENCH_SHAPES"):
        shapes = tuple((f[0], int(f[1]), int(f[2]), int(f[3])) for f in (x.split(":") for x in os.environ["BENCH_SHAPES"].split(",")))
    for name, M, N, K in shapes:
        A = torch.randn(M, K, device=dev).to(BF)
        W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
        out = torch.empty(M, N, device=dev, dtype=BF)
        fn = lambda: torch.matmul(A, W.t(), out=out)
        ms = min(timeit(fn, iters), timeit(fn, iters))
        print(f"vendor gemm {name}: M={M} N={N} K={K}  {ms:8.3f} ms  {2.0 * M * N * K / ms / 1e9:8.1f} TFLOP/s", flush=True)


def gemm_phases(epi=3):
    """needs a -DMMPL_DEV_ABLATIONS -DGEMM6_TIMING=1 build (tools/r06_gpu.sh gemmphases): per-wave { prologue, k loop, epilogue } cycles written over the output"""
    M, N, K = (int(v) for v in os.environ.get("BENCH_PHASE_SHAPE", "25200:5120:5120").split(":"))
    A = torch.randn(M, K, device=dev).to(BF)
    W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
    b = torch.randn(N, device=dev).to(BF)
    Cc = torch.zeros(M, N, device=dev, dtype=BF)
    res = torch.randn(M, N, device=dev).to(BF)
    gate = torch.randn(8, N, device=dev).to(BF)
    for _ in range(2):
        _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(Cc), N, M, N, K, epi, _lib.ptr(res), N, _lib.ptr(gate), N,
                                 3600, _lib.stream_ptr()))
    torch.cuda.synchronize()
    nblk = ((M + 255) // 256) * (N // 256)
    t = Cc.view(-1).view(torch.float32)[: nblk * 16].view(-1, 4).double()
    t = t[t[:, 3] == K // 32]
    print(f"gemmphases {M}x{N}x{K} epi={epi}: waves {len(t)}  prologue {t[:, 0].mean().item():.0f}  loop {t[:, 1].mean().item():.0f} "
          f"({t[:, 1].mean().item() / (K // 32) / 32:.2f} per MFMA; p5 {t[:, 1].quantile(0.05).item():.0f} p50 {t[:, 1].quantile(0.5).item():.0f} "
          f"p95 {t[:, 1].quantile(0.95).item():.0f})  epilogue {t[:, 2].mean().item():.0f} (max {t[:, 2].max().item():.0f}) cycles", flush=True)


def bench_elem(iters):
    """the HBM-bound passes of a block at the stage shapes: LayerNorm + modulation (3 per block) and q/k RMS-norm + RoPE + K page write
    (1 per block; the cross-attention's q norm is the same kernel on q alone).  Prints time, algorithmic GB/s and a hash of the outputs."""
    import hashlib
    from mmpl_amd.dit import DitEngine

    def sha(*ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
        return h.hexdigest()[:12]

    for model, d, H, lat, S, frames_list in (("14B/720p", 5120, 40, (90, 160), 3600, (7, 6, 2)), ("14B/480p", 5120, 40, (60, 104), 1560, (7, 6, 2)),
                                             ("1.3B/480p", 1536, 12, (60, 104), 1560, (7, 6, 2))):
        eng = DitEngine(dict(dim=d, ffn_dim=256, num_heads=H, num_layers=1, text_dim=64), lat[0], lat[1], dev)
        for nF in frames_list:
            rows = nF * S
            torch.manual_seed(nF)
            x = (torch.randn(rows, d, device=dev) * 3 + 0.5).to(BF)
            e = (torch.randn(nF, 6, d, device=dev) * 0.3).to(BF)
            y = torch.empty_like(x)
            fn = lambda: _lib.check(lib.mmpl_layernorm(_lib.ptr(x), d, _lib.ptr(y), d, rows, d, 1e-6, _lib.ptr(e[:, 1]), _lib.ptr(e[:, 0]), 6 * d, S,
                                                       None, None, _lib.stream_ptr()))
            ms = min(timeit(fn, iters), timeit(fn, iters))
            gb = 2.0 * rows * d * 2 / 1e9
            h = sha(y)
            w = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
            b = (0.1 * torch.randn(d, device=dev)).to(BF)
            _lib.check(lib.mmpl_layernorm(_lib.ptr(x), d, _lib.ptr(y), d, rows, d, 1e-6, None, None, 0, S, _lib.ptr(w), _lib.ptr(b), _lib.stream_ptr()))
            print(f"elem {model} layernorm+mod rows={rows} d={d}  {ms * 1e3:8.1f} us  {gb / ms:6.2f} TB/s  sha {h} affine {sha(y)}", flush=True)
            qkv0 = torch.randn(rows, 3 * d, device=dev).to(BF)
            qkv = qkv0.clone()
            wq = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
            wk = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
            kc = torch.zeros(nF * S, d, device=dev, dtype=BF)
            kd = (C.c_void_p * nF)(*[kc[i * S:].data_ptr() for i in range(nF)])
            fi = (C.c_int * nF)(*range(3, 3 + nF))
            # v = NULL as in the forward (the QKV GEMM's epilogue writes the V pages)
            fq = lambda: _lib.check(lib.mmpl_qknorm_rope(eng._h, _lib.ptr(qkv), 3 * d, _lib.ptr(qkv[:, d:]), 3 * d, None, 3 * d, _lib.ptr(wq), _lib.ptr(wk),
                                                         nF, fi, kd, kd, _lib.stream_ptr()))
            fq()
            torch.cuda.synchronize()
            h = sha(qkv[:, :d], kc)
            ms = min(timeit(fq, iters), timeit(fq, iters))       # q is normalised in place again and again: same work, values irrelevant
            gb = 4.0 * rows * d * 2 / 1e9
            print(f"elem {model} qknorm+rope+kwrite rows={rows} d={d}  {ms * 1e3:8.1f} us  {gb / ms:6.2f} TB/s  sha {h}", flush=True)
            del qkv, qkv0, kc, x, y
    bench_solver_steps(iters)


def bench_solver_steps(iters):
    """the two fused CFG + solver updates side by side at the same n, alternating (3 rounds, the best of each): mmpl_cfg_unipc_step
    (6 reads + 4 writes per element at a second-order step with the corrector) and mmpl_cfg_dpmpp_step (4 reads + 3 writes at a
    second-order step).  n = the largest stage of 720p (7 frames x 16 x 90 x 160) and 2^26 elements (HBM-bound)."""
    from mmpl_amd.scheduler import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    u = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    u.set_timesteps(50, shift=5.0)
    su = [u.step_scalars(5.0) for _ in range(26)][25]
    d = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    retrieve_timesteps(d, sigmas=get_sampling_sigmas(50, 5.0))
    sd = [d.step_scalars(5.0) for _ in range(26)][25]
    assert su.use_corrector and su.corr_order == 2 and su.pred_order == 2 and sd.order == 2
    for n in (7 * 16 * 90 * 160, 1 << 26):
        torch.manual_seed(1)
        t = [torch.randn(n, device=dev).to(BF) for _ in range(6)]
        fu_ = lambda: _lib.check(lib.mmpl_cfg_unipc_step(*[_lib.ptr(b) for b in t], n, C.byref(su), _lib.stream_ptr()))
        fd_ = lambda: _lib.check(lib.mmpl_cfg_dpmpp_step(*[_lib.ptr(b) for b in t[:5]], n, C.byref(sd), _lib.stream_ptr()))
        best = {"unipc": float("inf"), "dpm++": float("inf")}
        for _ in range(3):
            best["unipc"] = min(best["unipc"], timeit(fu_, iters))
            best["dpm++"] = min(best["dpm++"], timeit(fd_, iters))
        for name, passes in (("unipc", 10), ("dpm++", 7)):
            ms = best[name]
            print(f"elem cfg+{name} step n={n}  {ms * 1e3:8.1f} us  {passes * n * 2 / 1e9 / ms:6.2f} TB/s", flush=True)
        del t


def bench_cross(iters):
    """text cross-attention alone (attn_fwd_kernel<1>): Lq query rows x 40 heads against `keys` context rows (valid tokens + the one
    collapsed padding row), q and o streams of Lq x 5120 bf16 each; time, algorithmic TB/s of q + o, a hash of the output"""
    import hashlib
    for H, d, Lq, keys in [(40, 5120, Lq, keys) for Lq in (25200, 21600, 7200) for keys in (128, 100, 65, 41, 13)] + \
                          [(12, 1536, Lq, keys) for Lq in (10920, 9360, 3120) for keys in (65, 41)]:
        if True:
            torch.manual_seed(keys)
            q = torch.randn(Lq, d, device=dev).to(BF)
            k = torch.randn(512, d, device=dev).to(BF)
            v = torch.randn(512, d, device=dev).to(BF)
            o = torch.empty_like(q)
            kp, vp = (C.c_void_p * 1)(k.data_ptr()), (C.c_void_p * 1)(v.data_ptr())
            fn = lambda: _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o), d, kp, vp, d, d, 1, keys, Lq, H, 1.0 / math.sqrt(128.0),
                                                              None, 0, 0, 1, _lib.stream_ptr()))
            ms = min(timeit(fn, iters), timeit(fn, iters))
            h = hashlib.sha256(o.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:12]
            print(f"cross H={H} Lq={Lq} keys={keys}  {ms * 1e3:8.1f} us  {2.0 * Lq * d * 2 / 1e9 / ms:6.2f} TB/s (q + o)  "
                  f"{4.0 * Lq * keys * d / ms / 1e9:7.1f} TFLOP/s  sha {h}", flush=True)


def taehv_macs_per_latent(h, w):
    """Multiply-accumulates of the TAEHV decoder per latent frame (= 4 pixel frames), from the layer shapes as the engine runs them
    (TGrow's 1x1 at the low resolution; the 3-channel head counted as 3 channels, not the 16 the tile computes)."""
    ch, grow = [256, 128, 64, 64], [1, 2, 2]
    macs, px, t = h * w * 9 * 16 * ch[0], h * w, 1
    for lvl in range(3):
        c = ch[lvl]
        macs += 3 * t * px * 9 * (2 * c * c + c * c + c * c)                 # 3 MemBlocks: conv 2C->C, C->C, C->C
        macs += t * px * c * c * grow[lvl]                                   # TGrow 1x1
        t, px = t * grow[lvl], px * 4
        macs += t * px * 9 * c * ch[lvl + 1]                                 # the up-sampling 3x3 conv
    return macs + t * px * 9 * ch[3] * 3                                     # head


def bench_taehv(iters, out_path=None):
    """Same process, alternating, warm, event-timed: the streamed decode of one 3-latent block (not the video's first) and the
    one-shot 21-latent decode, by mmpl_vae_stream_decode / mmpl_vae_decode and by the TAEHV engine, at 480p and 720p."""
    from mmpl_amd.synthetic import taehv_state_dict, vae_state_dict
    from mmpl_amd.taehv import TaehvEngine
    from mmpl_amd.vae import VaeEngine
    from mmpl_amd.wan_wrapper import WanVAEWrapper
    mean, std = WanVAEWrapper.mean, WanVAEWrapper.std
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_kernels.py taehv --iters {iters}: min of 3 windows of {iters} calls each, hipEvent-timed, alternating decoders")
    for name, (h, w) in (("480p", (60, 104)), ("720p", (90, 160))):
        vae, tiny = VaeEngine(h, w, dev), TaehvEngine(h, w, dev)
        vae.load_state_dict(vae_state_dict(seed=2))
        tiny.load_state_dict(taehv_state_dict(seed=4))
        g = torch.Generator(device=dev).manual_seed(3)
        z = torch.randn(21, 16, h, w, generator=g, device=dev).bfloat16()
        gmac = taehv_macs_per_latent(h, w) / 1e9
        say(f"{name} ({h} x {w} latents): TAEHV {gmac:.1f} GMAC = {2 * gmac / 1e3:.3f} TFLOP per latent frame")
        for fmt in ("uint8",):
            vae.clear_cache(); tiny.clear_cache()
            vae.decode_stream(z[:3], mean, std, out_format=fmt); tiny.decode_stream(z[:3], out_format=fmt)      # the videos' first blocks
            fv = lambda: vae.decode_stream(z[3:6], mean, std, out_format=fmt)
            ft = lambda: tiny.decode_stream(z[3:6], out_format=fmt)
            tv, tt = [], []
            for _ in range(3):
                tv.append(timeit(fv, iters)); tt.append(timeit(ft, iters))
            v, t = min(tv), min(tt)
            say(f"{name} streamed block of 3 latents ({fmt}, not the first): wan_vae {v:8.3f} ms   taehv {t:8.3f} ms   ratio {v / t:5.2f}x   "
                f"taehv {3 * 2 * gmac / t:6.1f} TFLOP/s   (windows: vae {' '.join(f'{x:.3f}' for x in tv)} | taehv {' '.join(f'{x:.3f}' for x in tt)})")
        fv = lambda: vae.decode(z, mean, std)
        ft = lambda: tiny.decode(z)
        n1 = max(1, iters // 4)
        tv, tt = [], []
        for _ in range(2):
            tv.append(timeit(fv, n1)); tt.append(timeit(ft, n1))
        v, t = min(tv), min(tt)
        say(f"{name} one-shot 21 latents (float): wan_vae {v:8.2f} ms ({1 + 4 * 20} frames)   taehv {t:8.2f} ms ({4 * 21} frames)   ratio {v / t:5.2f}x   "
            f"taehv {21 * 2 * gmac / t:6.1f} TFLOP/s")
        del vae, tiny
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def taehv_enc_macs_per_latent(h, w):
    """Multiply-accumulates of the TAEHV encoder per latent frame (= 4 pixel frames), from the layer shapes as the engine runs them
    (the input layer counted as its 27 real products, not the 32 the MFMA computes)."""
    c, hw = 64, h * w
    macs = 4 * 64 * hw * 27 * c                                              # input layer, 4 full-resolution frames
    t, px = 4, 64 * hw
    for stride in (2, 2, 1):
        t //= stride
        macs += t * px * stride * c * c                                      # TPool 1x1 at the incoming resolution
        px //= 4
        macs += t * px * 9 * c * c                                           # stride-2 3x3 conv
        macs += 3 * t * px * 9 * (2 * c * c + c * c + c * c)                 # 3 MemBlocks
    return macs + t * px * 9 * c * 16                                        # head


def bench_taehvenc(iters, out_path=None):
    """Same process, alternating, warm, event-timed: the tiny encoder on 12 pixel frames (a streamed group that is not the video's
    first) against WanVAEWrapper.encode_to_latent on 13 frames of the same size, at 480p and 720p; then the input layer alone
    against the same layer through the generic conv on a zero-padded 32-channel frame (whose staging is not even counted)."""
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import taehv_encoder_state_dict, vae_state_dict
    from mmpl_amd.taehv import TaehvEncoderEngine, TaehvEngine
    from mmpl_amd.wan_wrapper import WanVAEWrapper
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/bench_kernels.py taehvenc --iters {iters}: min of 3 windows of {iters} calls each, hipEvent-timed, alternating encoders")
    sd = taehv_encoder_state_dict(seed=5)
    for name, (h, w) in (("480p", (60, 104)), ("720p", (90, 160))):
        H, W = 8 * h, 8 * w
        wan = WanVAEWrapper(geometry=Geometry(h, w), device=dev, state_dict=vae_state_dict(seed=2))
        tiny = TaehvEncoderEngine(h, w, dev)
        tiny.load_state_dict(sd)
        g = torch.Generator(device=dev).manual_seed(3)
        u8 = torch.randint(0, 256, (24, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        video = (u8[:13].permute(3, 0, 1, 2).float() / 127.5 - 1).to(BF).unsqueeze(0).contiguous()        # [1, 3, 13, H, W] in [-1, 1]
        gmac = taehv_enc_macs_per_latent(h, w) / 1e9
        say(f"{name} ({h} x {w} latents): TAEHV encoder {gmac:.1f} GMAC = {2 * gmac / 1e3:.3f} TFLOP per latent frame")
        tiny.clear_cache()
        tiny.encode_stream(u8[:12])                                          # the video's first group
        fv = lambda: wan.encode_to_latent(video)
        ft = lambda: tiny.encode_stream(u8[12:24])
        tv, tt = [], []
        for _ in range(3):
            tv.append(timeit(fv, iters)); tt.append(timeit(ft, iters))
        v, t = min(tv), min(tt)
        say(f"{name} wan_vae encode_to_latent, 13 frames: {v:8.3f} ms = {v / 13:7.3f} ms / frame   taehv encode_stream, 12 frames (uint8, not "
            f"the first): {t:8.3f} ms = {t / 12:7.3f} ms / frame   ratio per frame {(v / 13) / (t / 12):5.2f}x   taehv {3 * 2 * gmac / t:6.1f} TFLOP/s"
            f"   (windows: vae {' '.join(f'{x:.3f}' for x in tv)} | taehv {' '.join(f'{x:.3f}' for x in tt)})")
        del wan, tiny
        torch.cuda.empty_cache()
        # the input layer alone, 4 frames: the packed-K kernel against taehv_conv_kernel on a [H + 2, W + 2, 32] frame
        w0, b0 = sd["encoder.0.weight"], sd["encoder.0.bias"].to(dev)
        wp = TaehvEncoderEngine._repack("encoder.0.weight", w0).to(dev)
        wg = TaehvEngine._repack("encoder.0.weight", w0).to(dev)             # Cin 3 zero-padded to 32, 9 taps
        dst = torch.zeros(4, H + 2, W + 2, 64, device=dev, dtype=BF)
        src = torch.zeros(4, H + 2, W + 2, 32, device=dev, dtype=BF)
        src[:, 1:-1, 1:-1, :3] = (u8[:4].float() / 255).to(BF)
        fsd, fs = dst[0].numel(), src[0].numel()
        fp = lambda: _lib.check(lib.mmpl_taehv_conv_in(_lib.ptr(u8), 1, _lib.ptr(wp), _lib.ptr(b0), 4, H, W, _lib.ptr(dst), fsd, _lib.stream_ptr()))
        fg = lambda: _lib.check(lib.mmpl_taehv_conv(_lib.ptr(src), None, fs, 0, 32, 0, 0, 9, _lib.ptr(wg), _lib.ptr(b0), 64, 64, 4, H, W,
                                                    _lib.ptr(dst), fsd, 64, 64, 1, None, 0, None, _lib.stream_ptr()))
        fg()
        a = dst.clone()
        fp()
        diff = float((a.float() - dst.float()).abs().max())                  # two summation orders of the same 27 products
        tp, tg = [], []
        for _ in range(3):
            tp.append(timeit(fp, iters)); tg.append(timeit(fg, iters))
        say(f"{name} input layer, 4 frames: packed-K conv_in {min(tp):7.3f} ms   generic 3x3 conv on a padded 32-channel frame {min(tg):7.3f} ms   "
            f"ratio {min(tg) / min(tp):5.2f}x   max |d| between them {diff:.3g}   ({4 * dst[0].numel() * 2 / 1e6 / min(tp):.0f} GB/s of output)")
        del dst, src, u8, video
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 5
    if what in ("attn", "all"):
        bench_attn(iters)
    if what == "gemmphases":
        gemm_phases(3)
        gemm_phases(0)
    if what in ("gemm", "all"):
        bench_gemm(iters)
    if what == "gemmref":
        bench_gemm_ref(iters)
    if what == "attnref":
        bench_attn_ref(iters)
    if what == "elem":
        bench_elem(iters)
    if what == "cross":
        bench_cross(iters)
    if what == "taehv":
        bench_taehv(iters, sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
    if what == "taehvenc":
        bench_taehvenc(iters, sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None)
