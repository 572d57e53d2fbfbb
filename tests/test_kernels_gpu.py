"""GPU parity of each HIP kernel behind the C ABI against the oracle / a plain fp32 restatement (-m gpu).

Tolerances (stated, bf16 path): a kernel output must sit within 2e-3 rel-L2 of the fp32 restatement of the same op
rounded at the same points (i.e. only accumulation-order differences remain), and elementwise kernels must be within
1 bf16 ulp of the oracle on >= 99.9 % of elements.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import bf16_ulp_frac, max_abs, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _sp():
    from mmpl_amd import _lib
    return _lib.stream_ptr()


# (3120, 192, 256): M >= 1024 and 128 <= N < 256 -> the 256x128 kernel (gemm_bf16_v2_kernel)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 384, 256), (1560 * 2, 768, 256), (7, 1536, 256), (777, 64, 512),
                                   (3120, 192, 256), (4096, 5120, 5120)])
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
def test_gemm(lib, M, N, K, epi):
    from mmpl_amd import _lib
    if M == 4096 and epi not in (0, 3):
        pytest.skip("large shape covered for two epilogues")
    torch.manual_seed(M + N + K + epi)
    dev = "cuda:0"
    A = torch.randn(M, K, device=dev).to(BF)
    W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
    b = (torch.randn(N, device=dev) * 0.1).to(BF)
    res = torch.randn(M, N, device=dev).to(BF)
    S = 97 if M > 97 else M
    nfr = (M + S - 1) // S
    gate = torch.randn(nfr, 3, N, device=dev).to(BF)     # per-frame vectors with a frame stride of 3*N
    Cc = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(Cc), N, M, N, K, epi, _lib.ptr(res), N,
                             _lib.ptr(gate[:, 1]), 3 * N, S, _sp()))
    torch.cuda.synchronize()
    y = (A.float() @ W.float().t() + b.float()).to(BF)
    if epi == 1:
        y = F.gelu(y.float(), approximate="tanh").to(BF)
    elif epi == 2:
        y = F.silu(y.float()).to(BF)
    elif epi == 3:
        fr = torch.arange(M, device=dev) // S
        y = (res.float() + (y.float() * gate[fr, 1].float()).to(BF).float()).to(BF)
    elif epi == 4:
        y = (res.float() + y.float()).to(BF)
    assert rel_l2(Cc, y) < 2e-3, (rel_l2(Cc, y), max_abs(Cc, y))
    assert bf16_ulp_frac(Cc, y, 2) < 2e-3


def test_cross_attention_on_w64_opt_in():
    """MMPL_CROSS_W64=1 (read once per process) puts the text / image cross-attention on the 64-rows-per-wave kernel too
    (q prescaled by the cross q-norm): the DiT forward and the i2v model-type goldens in a child process with it set."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMPL_CROSS_W64="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "tests/test_dit_forward_gpu.py", "tests/test_i2v_clip_gpu.py",
                        "-k", "golden or oracle_small"], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# (M, N, K, epi, split): 258 tiles = one full round + 2 (Wan 1.3B ffn2 at s1); 78 tiles, no full round at all (1.3B s0); 580 = 2 rounds
# + 68 (14B / 720p s0) with GELU and with the plain bias epilogue; NOT split: a short K (the partials' round trip costs more than it
# saves), a leftover of 28 tiles per XCD
@pytest.mark.parametrize("M,N,K,epi,split", [(10920, 1536, 8960, 3, True), (3120, 1536, 8960, 3, True), (7200, 5120, 5120, 1, True),
                                             (7200, 5120, 4096, 0, True), (10920, 1536, 1536, 3, False), (9360, 1536, 8960, 4, False)])
def test_gemm_split_k_tail(lib, M, N, K, epi, split):
    """mmpl_gemm_scratch: the leftover tiles of the partial last round run as 2-4 blocks each over a share of K, fp32 partials summed
    in part order by the last part to finish.  Against fp32 like test_gemm; against mmpl_gemm only the split tiles differ (fp32
    summation order), everything else bit-identical; two runs bit-identical (deterministic); scratch header left zero."""
    from mmpl_amd import _lib
    torch.manual_seed(M + N + K)
    dev = "cuda:0"
    A = torch.randn(M, K, device=dev).to(BF)
    W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
    b = (torch.randn(N, device=dev) * 0.1).to(BF)
    res = torch.randn(M, N, device=dev).to(BF)
    gate = torch.randn((M + 1559) // 1560, N, device=dev).to(BF)
    plain = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(plain), N, M, N, K, epi, _lib.ptr(res), N, _lib.ptr(gate), N, 1560, _sp()))
    nb = lib.mmpl_gemm_scratch_bytes()
    scratch = torch.zeros(nb, dtype=torch.uint8, device=dev)

    def run(a_mat, stream=None):
        out = torch.full((M, N), float("nan"), device=dev, dtype=BF)
        _lib.check(lib.mmpl_gemm_scratch(_lib.ptr(a_mat), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(out), N, M, N, K, epi, _lib.ptr(res), N,
                                         _lib.ptr(gate), N, 1560, _lib.ptr(scratch), nb, stream if stream is not None else _sp()))
        return out

    outs = []
    for _ in range(2):
        scratch[2048:] = 0xFF                                    # the partial area needs no initialisation (NaN patterns), and a stale
        out = run(A)                                             # partial of the PREVIOUS run must not be what the last part sums
        torch.cuda.synchronize()
        assert int(scratch[:2048].to(torch.int32).sum()) == 0
        outs.append(out)
    # steady state as a forward sees it: the same scratch, ANOTHER A in between (stale partials would now be wrong numbers, not NaN),
    # then A again -- bit-identical to the first runs
    A2 = (A.float() * 0.5 + 1.0).to(BF)
    o2 = run(A2)
    outs.append(run(A))
    plain2 = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A2), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(plain2), N, M, N, K, epi, _lib.ptr(res), N, _lib.ptr(gate), N, 1560, _sp()))
    torch.cuda.synchronize()
    assert rel_l2(o2, plain2) < 1e-3 and torch.equal(outs[2], outs[0])
    # ... and with a second queue keeping the CUs busy (the idle device is exactly the condition a dispatch-order probe runs under:
    # the exchange of the partials must not depend on where the parts land)
    side = torch.cuda.Stream()
    filler_a = torch.randn(4096, 4096, device=dev).to(BF)
    with torch.cuda.stream(side):
        for _ in range(6):
            filler_a = (filler_a @ filler_a).clamp_(-1, 1)
    busy = [run(A2), run(A)]
    torch.cuda.synchronize()
    assert torch.equal(busy[0], o2) and torch.equal(busy[1], outs[0])
    assert torch.equal(outs[0], outs[1])
    out = outs[0]
    assert torch.isfinite(out.float()).all()
    tiles_differ = (out != plain).reshape(-1)[: (M // 256) * 256 * N].reshape(M // 256, 256, N // 256, 256).any(dim=3).any(dim=1)
    if split:
        assert 0 < int(tiles_differ.sum()) <= 128
    else:
        assert torch.equal(out, plain)
    y = A.float() @ W.float().t() + b.float()
    y = y.to(BF).float()
    if epi == 1:
        y = torch.nn.functional.gelu(y, approximate="tanh")
    if epi == 3:
        fr = torch.arange(M, device=dev) // 1560
        y = res.float() + (y * gate.float()[fr]).to(BF).float()
    if epi == 4:
        y = res.float() + y
    assert rel_l2(out, y.to(BF)) < 2e-3 and rel_l2(out, plain) < 1e-3


# Wan 1.3B at 480p: qkv at s1 = 43 x 18 = 774 tiles (3 rounds + 6), o / cross-q / cross-o = 258 (1 round + 2), the same at s0 = 78 tiles
# (no full round at all), qkv at s2 = 37 x 18 = 666 (2 rounds + 154: NOT sub-tiled, the leftover is more than half a round)
@pytest.mark.parametrize("M,N,K,epi", [(10920, 4608, 1536, 0), (10920, 1536, 1536, 3), (10920, 1536, 1536, 4), (3120, 1536, 1536, 1),
                                       (9360, 4608, 1536, 2), (10920, 1536, 2048, 3)])
def test_gemm_subtile_tail(lib, M, N, K, epi):
    """Short-K GEMMs with tile tickets: the leftover tiles of the partial last round run as 128 x 128 quadrants in a second launch
    (gemm_tail128_kernel).  Same MFMAs in the same order per accumulator, same epilogue arithmetic: bit-identical to the one-launch
    mmpl_gemm; the ticket counters are zero again afterwards (two launches in a row)."""
    from mmpl_amd import _lib
    torch.manual_seed(M + N + K + epi)
    dev = "cuda:0"
    A = torch.randn(M, K, device=dev).to(BF)
    W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
    b = (torch.randn(N, device=dev) * 0.1).to(BF)
    res = torch.randn(M, N, device=dev).to(BF)
    gate = torch.randn((M + 1559) // 1560, N, device=dev).to(BF)
    ref = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(ref), N, M, N, K, epi, _lib.ptr(res), N, _lib.ptr(gate), N, 1560, _sp()))
    ctr = torch.zeros(8, dtype=torch.int32, device=dev)
    for _ in range(2):
        out = torch.full((M, N), float("nan"), device=dev, dtype=BF)
        _lib.check(lib.mmpl_gemm_tickets(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(out), N, M, N, K, epi, _lib.ptr(res), N,
                                         _lib.ptr(gate), N, 1560, _lib.ptr(ctr), _sp()))
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        assert int(ctr.abs().sum()) == 0
    y = A.float() @ W.float().t() + b.float()
    y = y.to(BF).float()
    if epi == 1:
        y = F.gelu(y, approximate="tanh").to(BF).float()
    elif epi == 2:
        y = F.silu(y).to(BF).float()
    elif epi == 3:
        fr = torch.arange(M, device=dev) // 1560
        y = res.float() + (y * gate.float()[fr]).to(BF).float()
    elif epi == 4:
        y = res.float() + y
    assert rel_l2(out, y.to(BF)) < 2e-3


@pytest.mark.parametrize("M,N,K,epi", [(25200, 5120, 1024, 3), (9000, 2560, 512, 0), (4096, 5120, 5120, 1), (3120, 768, 256, 4)])
def test_gemm_dynamic_tile_scheduling(lib, M, N, K, epi):
    """mmpl_gemm_tickets: the large-problem kernel launched once per CU, blocks drawing tiles from per-XCD tickets.  Same tiles,
    same arithmetic per tile -> bit-identical to mmpl_gemm; the counters are zero again afterwards (two launches in a row).
    The last shape has fewer tiles than CUs: falls back to one block per tile."""
    from mmpl_amd import _lib
    torch.manual_seed(M + N + K)
    dev = "cuda:0"
    A = torch.randn(M, K, device=dev).to(BF)
    W = (torch.randn(N, K, device=dev) / math.sqrt(K)).to(BF)
    b = (torch.randn(N, device=dev) * 0.1).to(BF)
    res = torch.randn(M, N, device=dev).to(BF)
    gate = torch.randn((M + 3599) // 3600, N, device=dev).to(BF)
    ref = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(ref), N, M, N, K, epi, _lib.ptr(res), N, _lib.ptr(gate), N, 3600, _sp()))
    ctr = torch.zeros(8, dtype=torch.int32, device=dev)
    for _ in range(2):
        out = torch.full((M, N), float("nan"), device=dev, dtype=BF)
        _lib.check(lib.mmpl_gemm_tickets(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(out), N, M, N, K, epi, _lib.ptr(res), N,
                                         _lib.ptr(gate), N, 3600, _lib.ptr(ctr), _sp()))
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        assert int(ctr.abs().sum()) == 0


def test_gemm_heavy_tailed(lib):
    """Wan-like activation statistics: a few channels of A carry values ~100x the rest (massive activations) and a few
    weight rows are large; same tolerance as test_gemm (the fp32 accumulation must not lose the small terms)."""
    from mmpl_amd import _lib
    torch.manual_seed(7)
    dev = "cuda:0"
    M, N, K = 3600, 5120, 5120
    A = torch.randn(M, K, device=dev)
    A[:, torch.randperm(K)[:6]] *= 100.0
    W = torch.randn(N, K, device=dev) / math.sqrt(K)
    W[torch.randperm(N)[:5]] *= 30.0
    A, W = A.to(BF), W.to(BF)
    b = (torch.randn(N, device=dev) * 0.1).to(BF)
    Cc = torch.empty(M, N, device=dev, dtype=BF)
    _lib.check(lib.mmpl_gemm(_lib.ptr(A), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(Cc), N, M, N, K, 0, None, N, None, 0, 1, _sp()))
    torch.cuda.synchronize()
    y = (A.float() @ W.float().t() + b.float()).to(BF)
    assert rel_l2(Cc, y) < 2e-3 and bf16_ulp_frac(Cc, y, 2) < 2e-3


def _attn_case(lib, Lq, H, S, n_pages, ld_mult=1, seed=0, variant=0, qk_gain=1.0, cross=0):
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(seed)
    dev = "cuda:0"
    d = H * 128
    q32 = torch.randn(Lq, ld_mult * d, device=dev) * qk_gain
    q = q32.to(BF)
    if variant == 4:
        # the producer folds softmax_scale * log2(e) into q before rounding it (what mmpl_dit_forward's qknorm kernel does);
        # the reference attends with the exactly un-scaled value of that bf16 tensor
        c = (1.0 / math.sqrt(128)) * 1.4426950408889634
        q = (q32 * c).to(BF)
        q32 = q.float() / c
    n_slots = n_pages + 2
    kc = (torch.randn(n_slots * S, d, device=dev) * qk_gain).to(BF)
    vc = torch.randn(n_slots * S, d, device=dev).to(BF)
    slots = torch.randperm(n_slots)[:n_pages].tolist()
    o = torch.zeros(Lq, d, device=dev, dtype=BF)
    kp = (C.c_void_p * n_pages)(*[kc[s * S:].data_ptr() for s in slots])
    vp = (C.c_void_p * n_pages)(*[vc[s * S:].data_ptr() for s in slots])
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), ld_mult * d, _lib.ptr(o), d, kp, vp, d, d, n_pages, S, Lq, H,
                                         1.0 / math.sqrt(128), None, 0, variant, cross, _sp()))
    torch.cuda.synchronize()
    idx = [j for s in slots for j in range(s * S, (s + 1) * S)]
    qq = (q32 if variant == 4 else q)[:, :d].reshape(1, Lq, H, 128).cpu()
    kk = kc[idx].reshape(1, -1, H, 128).cpu()
    vv = vc[idx].reshape(1, -1, H, 128).cpu()
    ref32 = W.sdpa_fp32(qq, kk, vv).reshape(Lq, d)
    ref16 = W.sdpa(qq, kk, vv).reshape(Lq, d)
    return o, ref32, ref16


# (the last row: KV streams of 1, 1 (ragged), 3, 4 and 24 (max pages, all ragged) tiles -- the prologue / ring-wrap / counted
# s_waitcnt branches of the DMA kernels).  variant: 0 = what a raw-q launch gets (the lock-step kernel), 1 = the lock-step kernel
# the text cross-attention uses, 3 = 64 query rows per wave prescaling a raw q itself, 4 = 64 rows per wave on
# a q prescaled by its producer (the DiT forward's self-attention launch).
@pytest.mark.parametrize("variant", [0, 1, 3, 4])
@pytest.mark.parametrize("Lq,H,S,n_pages", [(96, 2, 96, 1), (200, 2, 100, 3), (512, 1, 512, 1), (3120, 2, 1560, 2),
                                            (300, 8, 72, 21), (257, 3, 40, 5),
                                            (64, 1, 64, 1), (130, 2, 30, 1), (100, 1, 64, 3), (70, 2, 128, 2), (256, 1, 10, 24)])
def test_attention_paged(lib, Lq, H, S, n_pages, variant):
    o, ref32, ref16 = _attn_case(lib, Lq, H, S, n_pages, ld_mult=3 if H == 2 else 1, variant=variant)
    e_kernel, e_ref = rel_l2(o, ref32), rel_l2(ref16, ref32)
    # two-sided bf16 tolerance: kernel and the reference's own bf16 SDPA both within 1e-2 of fp32, and the kernel
    # not worse than 1.5x the reference's bf16 error
    assert e_kernel < 1e-2 and e_kernel < 1.5 * e_ref + 1e-3, (e_kernel, e_ref)


@pytest.mark.parametrize("Lq,H,S", [(5000, 40, 65), (5000, 40, 13), (256 * 70, 8, 128), (256 * 9 + 1, 3, 64), (100, 2, 41), (1560 * 7, 12, 65)])
def test_cross_attention_short_context(lib, Lq, H, S):
    """Text cross-attention over <= 2 KV tiles (attn_cross_kernel): a block keeps its head's K / V in LDS over a run of query
    blocks -- several per block at these sizes, a ragged last one -- with the next block's q in flight.  Against fp32, and
    bit-identical to the lock-step kernel on the same inputs (same tile routine, same order)."""
    o, ref32, ref16 = _attn_case(lib, Lq, H, S, 1, variant=0, cross=1, seed=S)
    e_kernel, e_ref = rel_l2(o, ref32), rel_l2(ref16, ref32)
    assert e_kernel < 1e-2 and e_kernel < 1.5 * e_ref + 1e-3, (e_kernel, e_ref)
    o_lock, _, _ = _attn_case(lib, Lq, H, S, 1, variant=0, cross=0, seed=S)
    assert torch.equal(o, o_lock)


@pytest.mark.parametrize("variant", [0, 1, 4])
def test_attention_large_qk_gain(lib, variant):
    """QK-norm gains x8 (Wan checkpoints carry large norm_q / norm_k weights): logits ~64x those of N(0,1) inputs, near
    one-hot softmax rows.  The 64-rows-per-wave kernel leaves its max-free fast path on such rows (|row max| > 2^6).
    (Variant 3 -- that kernel rounding a raw q a second time -- is 1.3e-2 off here: the reason the DiT forward prescales q
    where it is produced and raw-q launches take the lock-step kernel.)"""
    o, ref32, ref16 = _attn_case(lib, 700, 2, 328, 3, variant=variant, qk_gain=8.0, seed=5)
    e_kernel, e_ref = rel_l2(o, ref32), rel_l2(ref16, ref32)
    assert e_kernel < 1e-2 and e_kernel < 1.5 * e_ref + 1e-3, (e_kernel, e_ref)


@pytest.mark.parametrize("variant", [0, 1, 3, 4])
@pytest.mark.parametrize("spike", [4.0, 30.0])
def test_attention_spiked_scores(lib, variant, spike):
    """force online-softmax max jumps late in the KV stream (rescale path) -- rule 26 of the CDNA guide.  spike 30: the
    aligned key's score is ~340 (2^490 in the exp2 domain), far beyond every deferral bound of the 64-rows-per-wave kernel
    (first-tile range 2^6, tile-sum bounds 2^80 / 2^30), in the 4th tile, so that kernel must re-reference mid-stream."""
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(3)
    dev = "cuda:0"
    Lq, H, S = 128, 1, 320
    q = torch.randn(Lq, 128, device=dev).to(BF)
    k = torch.randn(S, 128, device=dev).to(BF)
    v = torch.randn(S, 128, device=dev).to(BF)
    k[300] = (q[5].float() * 4).to(BF)          # one key aligned with one query, in the last tile
    k[70] = (q[17].float() * 3).to(BF)
    k[200] = (q[40].float() * spike).to(BF)
    q_ref = q
    if variant == 4:
        c = (1.0 / math.sqrt(128)) * 1.4426950408889634
        q = (q.float() * c).to(BF)
        q_ref = q.float() / c
    o = torch.zeros(Lq, 128, device=dev, dtype=BF)
    kp = (C.c_void_p * 1)(k.data_ptr())
    vp = (C.c_void_p * 1)(v.data_ptr())
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), 128, _lib.ptr(o), 128, kp, vp, 128, 128, 1, S, Lq, H, 1.0 / math.sqrt(128),
                                         None, 0, variant, 0, _sp()))
    torch.cuda.synchronize()
    ref = W.sdpa_fp32(q_ref.cpu().view(1, Lq, 1, 128), k.cpu().view(1, S, 1, 128), v.cpu().view(1, S, 1, 128)).view(Lq, 128)
    # max: 2 bf16 ulps of the largest output (a one-hot row returns a V row, rounded once more by the kernel)
    assert max_abs(o, ref) < 2.0 ** -7 * ref.abs().max().item() + 1e-2 and rel_l2(o, ref) < 1e-2


@pytest.mark.parametrize("d,rows,S", [(256, 200, 50), (1536, 97, 97), (5120, 130, 65), (512, 8, 4),
                                      # many rows, several frames (all below MMPL_LN_PIPELINE_MIN_ROWS or NIT 6: layernorm_kernel; the pipelined
                                      # kernel is run one launch at a time by tests/test_rowpass_exact_gpu.py):
                                      (5120, 7224, 1204), (1536, 9 * 1204, 1204), (5120, 7 * 1001, 1001), (1024, 20000, 20000)])
def test_layernorm_modulate_and_affine(lib, d, rows, S):
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(d)
    dev = "cuda:0"
    nF = rows // S
    rows = nF * S
    x = (torch.randn(rows, d, device=dev) * 3 + 0.5).to(BF)
    e = (torch.randn(nF, 6, d, device=dev) * 0.3).to(BF)
    y = torch.empty_like(x)
    _lib.check(lib.mmpl_layernorm(_lib.ptr(x), d, _lib.ptr(y), d, rows, d, 1e-6, _lib.ptr(e[:, 1]), _lib.ptr(e[:, 0]), 6 * d, S,
                                  None, None, _sp()))
    torch.cuda.synchronize()
    xc, ec = x.cpu(), e.cpu()
    ref = (W.layer_norm(xc.unsqueeze(0), 1e-6).unflatten(1, (nF, S)) * (1 + ec[None, :, 1:2]) + ec[None, :, 0:1]).flatten(1, 2)[0]
    assert bf16_ulp_frac(y, ref, 1) < 1e-3, (bf16_ulp_frac(y, ref, 1), max_abs(y, ref))
    w = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
    b = (0.1 * torch.randn(d, device=dev)).to(BF)
    _lib.check(lib.mmpl_layernorm(_lib.ptr(x), d, _lib.ptr(y), d, rows, d, 1e-6, None, None, 0, S, _lib.ptr(w), _lib.ptr(b), _sp()))
    torch.cuda.synchronize()
    ref = W.layer_norm(xc, 1e-6, w.cpu(), b.cpu())
    assert bf16_ulp_frac(y, ref, 1) < 1e-3


@pytest.mark.parametrize("H,lat,frames", [(2, (8, 12), [3, 10]), (12, (6, 10), [0, 19, 20]), (40, (4, 8), [5]),
                                          # several row groups per block (qknorm_kernel's prefetch loop): 7224 rows of 5120 / 1536, and an odd row count
                                          (40, (56, 86), [0, 1, 2, 7, 19, 20]), (12, (56, 86), [3, 4, 5, 6, 7, 8, 9]), (4, (70, 86), [2, 3, 4, 5, 6])])
def test_qknorm_rope_kvwrite(lib, H, lat, frames):
    from mmpl_amd import _lib
    from mmpl_amd.dit import DitEngine
    from oracle import wan_dit_ref as W
    torch.manual_seed(H)
    dev = "cuda:0"
    d = H * 128
    eng = DitEngine(dict(dim=d, ffn_dim=256, num_heads=H, num_layers=1, text_dim=64), lat[0], lat[1], dev)
    gh, gw = lat[0] // 2, lat[1] // 2
    S, nF = gh * gw, len(frames)
    qkv = torch.randn(nF * S, 3 * d, device=dev).to(BF)
    wq = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
    wk = (1 + 0.1 * torch.randn(d, device=dev)).to(BF)
    kc = torch.zeros(25 * S, d, device=dev, dtype=BF)
    vc = torch.zeros(25 * S, d, device=dev, dtype=BF)
    slots = [W_ for W_ in range(3, 3 + nF)]
    orig = qkv.clone()
    kd = (C.c_void_p * nF)(*[kc[s * S:].data_ptr() for s in slots])
    vd = (C.c_void_p * nF)(*[vc[s * S:].data_ptr() for s in slots])
    fi = (C.c_int * nF)(*frames)
    _lib.check(lib.mmpl_qknorm_rope(eng._h, _lib.ptr(qkv), 3 * d, _lib.ptr(qkv[:, d:]), 3 * d, _lib.ptr(qkv[:, 2 * d:]), 3 * d,
                                    _lib.ptr(wq), _lib.ptr(wk), nF, fi, kd, vd, _sp()))
    torch.cuda.synchronize()
    oc = orig.cpu()
    freqs = W.rope_table(128)
    q_ref = W.fps_rope_apply(W.rms_norm(oc[:, :d].unsqueeze(0), wq.cpu(), 1e-6).view(1, -1, H, 128), frames, gh, gw, freqs)
    k_ref = W.fps_rope_apply(W.rms_norm(oc[:, d:2 * d].unsqueeze(0), wk.cpu(), 1e-6).view(1, -1, H, 128), frames, gh, gw, freqs)
    assert bf16_ulp_frac(qkv[:, :d], q_ref.reshape(-1, d), 1) < 1e-3
    for i, s in enumerate(slots):
        assert bf16_ulp_frac(kc[s * S:(s + 1) * S], k_ref.reshape(-1, d)[i * S:(i + 1) * S], 1) < 1e-3
        assert torch.equal(vc[s * S:(s + 1) * S].cpu(), oc[i * S:(i + 1) * S, 2 * d:])
    assert torch.equal(qkv[:, d:].cpu(), oc[:, d:])          # k, v inputs untouched
    assert kc[:3 * S].abs().sum().item() == 0 and kc[(3 + nF) * S:].abs().sum().item() == 0


@pytest.mark.parametrize("variant", [3])
def test_attention_split_kv_tail_round(lib, variant):
    """A query-block count that leaves a partial last round of one-block-per-CU (41 blocks per XCD on 32 CUs): with a
    workspace the 9 leftover blocks of every XCD run as 3 KV-range partials + merge.  Result vs fp32 and vs the unsplit
    launch (same tolerance class; accumulation order differs)."""
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(11)
    dev = "cuda:0"
    H, S, n_pages, Lq = 8, 640, 3, 256 * 41 - 57
    d = H * 128
    q = torch.randn(Lq, d, device=dev).to(BF)
    kc = torch.randn(n_pages * S, d, device=dev).to(BF)
    vc = torch.randn(n_pages * S, d, device=dev).to(BF)
    kp = (C.c_void_p * n_pages)(*[kc[i * S:].data_ptr() for i in range(n_pages)])
    vp = (C.c_void_p * n_pages)(*[vc[i * S:].data_ptr() for i in range(n_pages)])
    o_ws = torch.zeros(Lq, d, device=dev, dtype=BF)
    o_plain = torch.zeros_like(o_ws)
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o_ws), d, kp, vp, d, d, n_pages, S, Lq, H, 1.0 / math.sqrt(128),
                                         _lib.ptr(ws), ws.numel(), variant, 0, _sp()))
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o_plain), d, kp, vp, d, d, n_pages, S, Lq, H, 1.0 / math.sqrt(128),
                                         None, 0, variant, 0, _sp()))
    torch.cuda.synchronize()
    n_diff_rows = int((o_ws != o_plain).any(dim=1).sum())
    assert 0 < n_diff_rows <= 9 * 256              # only (some of) the tail blocks' rows went through the split path
    rows = torch.cat([torch.arange(0, 300), torch.arange(Lq - 2400, Lq)])          # head of the grid + the tail blocks
    ref32 = W.sdpa_fp32(q[rows].reshape(1, -1, H, 128).cpu(), kc.reshape(1, -1, H, 128).cpu(), vc.reshape(1, -1, H, 128).cpu()).reshape(-1, d)
    assert rel_l2(o_ws[rows], ref32) < 1e-2 and rel_l2(o_plain[rows], ref32) < 1e-2
    assert rel_l2(o_ws, o_plain) < 3e-3


# (H, query blocks, rows per page): 12 heads (Wan 1.3B: no multiple of the 8 XCDs -- 65 items per XCD, one tail item each in 4
# parts; the last XCD's chunk is short, so its tail item does not exist); 20 heads: 73 items per XCD, a tail of 9 in 3 parts each
@pytest.mark.parametrize("H,n_qb,S,max_tail_items", [(12, 43, 704, 8), (20, 29, 704, 8 * 9)])
def test_attention_split_kv_tail_any_shape(lib, H, n_qb, S, max_tail_items):
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(13)
    dev = "cuda:0"
    n_pages, Lq = 3, 256 * n_qb - 57
    d = H * 128
    c = (1.0 / math.sqrt(128)) * 1.4426950408889634
    q = (torch.randn(Lq, d, device=dev) * c).to(BF)                      # variant 4: q prescaled by its producer
    kc = torch.randn(n_pages * S, d, device=dev).to(BF)
    vc = torch.randn(n_pages * S, d, device=dev).to(BF)
    kp = (C.c_void_p * n_pages)(*[kc[i * S:].data_ptr() for i in range(n_pages)])
    vp = (C.c_void_p * n_pages)(*[vc[i * S:].data_ptr() for i in range(n_pages)])
    o_ws = torch.full((Lq, d), float("nan"), device=dev, dtype=BF)
    o_plain = torch.full((Lq, d), float("nan"), device=dev, dtype=BF)
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o_ws), d, kp, vp, d, d, n_pages, S, Lq, H, 1.0 / math.sqrt(128),
                                         _lib.ptr(ws), ws.numel(), 4, 0, _sp()))
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o_plain), d, kp, vp, d, d, n_pages, S, Lq, H, 1.0 / math.sqrt(128),
                                         None, 0, 4, 0, _sp()))
    torch.cuda.synchronize()
    assert torch.isfinite(o_ws.float()).all() and torch.isfinite(o_plain.float()).all()      # every (row, head) was written by both
    diff = (o_ws != o_plain).reshape(Lq, H, 128).any(dim=2)               # [row, head]: went through the split path
    n_items = int(diff.reshape(-1, H)[: (Lq // 256) * 256].reshape(-1, 256, H).any(dim=1).sum()) + int(diff[(Lq // 256) * 256:].any(dim=0).sum())
    assert 0 < n_items <= max_tail_items, n_items
    assert rel_l2(o_ws, o_plain) < 3e-3
    rows = torch.unique(torch.cat([torch.arange(0, 200), diff.any(dim=1).nonzero()[:, 0][::7].cpu(), torch.arange(Lq - 200, Lq)]))[:1500]
    ref32 = W.sdpa_fp32(q[rows].float().div(c).reshape(1, -1, H, 128).cpu(), kc.reshape(1, -1, H, 128).cpu(), vc.reshape(1, -1, H, 128).cpu()).reshape(-1, d)
    assert rel_l2(o_ws[rows], ref32) < 1e-2 and rel_l2(o_plain[rows], ref32) < 1e-2


@pytest.mark.parametrize("variant", [4])
def test_attention_split_kv_tail_round_spiked(lib, variant):
    """The tail round with scores no FAST pass can hold: a few keys are large multiples of a few queries, in the rows of the
    split tail blocks and in rows of the main round, in different KV ranges of the split.  The w64 kernel's blocks that see them
    redo their KV range in the GENERAL pass and write partials with their own references; the merge must still give the exact
    softmax (checker: fp32).  Variant 4 = w64 on a q its producer prescaled."""
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(12)
    dev = "cuda:0"
    H, S, n_pages, Lq = 8, 640, 3, 256 * 41 - 57
    d = H * 128
    q32 = torch.randn(Lq, d, device=dev)
    kc32 = torch.randn(n_pages * S, d, device=dev)
    vc = torch.randn(n_pages * S, d, device=dev).to(BF)
    hot_rows = [5, 300, Lq - 2000, Lq - 700, Lq - 3]                      # main-round rows and tail-block rows
    hot_keys = [17, 700, 1300, 1900, 650]                                  # spread over the three pages = over the split's KV ranges
    for r, kk in zip(hot_rows, hot_keys):
        for h in (0, 3, 7):
            kc32[kk, h * 128:(h + 1) * 128] = q32[r, h * 128:(h + 1) * 128] * 25.0
    c = (1.0 / math.sqrt(128)) * 1.4426950408889634
    q = (q32 * c).to(BF) if variant == 4 else q32.to(BF)
    q_ref = (q.float() / c) if variant == 4 else q.float()
    kc = kc32.to(BF)
    kp = (C.c_void_p * n_pages)(*[kc[i * S:].data_ptr() for i in range(n_pages)])
    vp = (C.c_void_p * n_pages)(*[vc[i * S:].data_ptr() for i in range(n_pages)])
    o = torch.full((Lq, d), float("nan"), device=dev, dtype=BF)
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), d, _lib.ptr(o), d, kp, vp, d, d, n_pages, S, Lq, H, 1.0 / math.sqrt(128),
                                         _lib.ptr(ws), ws.numel(), variant, 0, _sp()))
    torch.cuda.synchronize()
    assert torch.isfinite(o.float()).all()
    rows = torch.cat([torch.arange(0, 600), torch.arange(Lq - 2400, Lq)])
    ref32 = W.sdpa_fp32(q_ref[rows].reshape(1, -1, H, 128).cpu(), kc.float().reshape(1, -1, H, 128).cpu(), vc.float().reshape(1, -1, H, 128).cpu()).reshape(-1, d)
    assert rel_l2(o[rows], ref32) < 1e-2
    for r in hot_rows:                                                     # the spiked rows themselves: one-hot-like softmax, 2 bf16 ulps
        i = (rows == r).nonzero()[0, 0]
        assert max_abs(o[r], ref32[i]) < 2.0 ** -7 * ref32[i].abs().max().item() + 1e-3


@pytest.mark.parametrize("variant", [1, 4])
def test_attention_all_scores_very_negative(lib, variant):
    """Rows whose every score is far below zero (here ~ -90 in the exponent's log2 units): exp2 of them underflows a pass that
    takes 0 as the reference, so the w64 kernel's end-of-pass check (row sum < 2^-100) must send the block through the GENERAL
    pass; the answer is an ordinary softmax over the differences.  Checker: fp32."""
    from mmpl_amd import _lib
    from oracle import wan_dit_ref as W
    torch.manual_seed(21)
    dev = "cuda:0"
    Lq, S, H = 300, 200, 1
    u = torch.randn(128, device=dev)
    u = u / u.norm()
    q32 = torch.randn(Lq, 128, device=dev) * 0.3
    k32 = torch.randn(S, 128, device=dev) * 0.3
    q32[:40] += 26.0 * u                      # these rows: q.k / sqrt(128) ~ -26*26/11.3 ~ -60 (natural units) for every key
    k32 -= 26.0 * u
    q32[40:80] -= 26.0 * u                    # and these the opposite: every score ~ +60 -> overflow side of the same check
    v = torch.randn(S, 128, device=dev).to(BF)
    c = (1.0 / math.sqrt(128)) * 1.4426950408889634
    q = (q32 * c).to(BF) if variant == 4 else q32.to(BF)
    q_ref = (q.float() / c) if variant == 4 else q.float()
    k = k32.to(BF)
    kp = (C.c_void_p * 1)(k.data_ptr())
    vp = (C.c_void_p * 1)(v.data_ptr())
    o = torch.full((Lq, 128), float("nan"), device=dev, dtype=BF)
    _lib.check(lib.mmpl_attn_fwd_variant(_lib.ptr(q), 128, _lib.ptr(o), 128, kp, vp, 128, 128, 1, S, Lq, H, 1.0 / math.sqrt(128), None, 0,
                                         variant, 0, _sp()))
    torch.cuda.synchronize()
    ref = W.sdpa_fp32(q_ref.reshape(1, Lq, 1, 128).cpu(), k.float().reshape(1, S, 1, 128).cpu(), v.float().reshape(1, S, 1, 128).cpu()).reshape(Lq, 128)
    assert torch.isfinite(o.float()).all()
    for rows in (slice(0, 40), slice(40, 80), slice(80, Lq)):
        assert rel_l2(o[rows], ref[rows]) < 1e-2, (rows, rel_l2(o[rows], ref[rows]))
