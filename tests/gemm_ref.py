"""Exact-regime reference of the GEMM (csrc/gemm.hip) in the forms the DiT forward, T5, CLIP and the VAE launch it: the case table of
tests/test_gemm_forms_gpu.py, seeded input builders, the buffer geometry around every output (canaries, KV pages) and a float64
reference of every epilogue that rounds where gemm_epilogue / epi_stage / epi_finish round.  Importable without a GPU
(tests/test_gemm_ref.py proves, on the CPU, the conditions the bit-exact comparison rests on).

Why bit-exact is possible.  A and W are integers in [-2, 2], so every product and every partial sum of the accumulator is an integer
below 2^24: exact in fp32 whatever the order of summation -- MFMA order, k-tile order, split-K partials.  From an exact accumulator
the epilogues 0, 3, 4, 5, 6 are a chain of steps that are each exact or ONE round-to-nearest-even:
    pre = acc + bias          bias a multiple of 1/2: exact in fp32
    v   = bf16(pre)           RNE                                                  (epi 0 / 6 store v)
    t   = bf16(v * gate)      the product of two bf16 is exact in fp32; RNE         (epi 3)
    out = bf16(x + t)         x a multiple of 1/4 in [-32, 32], t a multiple of 1/16: exact in fp32; RNE at the pack   (epi 3 / 4)
    out = fp32(acc * alpha)   the float64 product of an integer < 2^24 and float64(float32(alpha)) is exact (48 bits); ONE RNE  (epi 5)
so the kernel's output is determined bit for bit.  GELU / SiLU (epi 1 / 2) are transcendental: their pre-activation v is exact and the
fp32 restatement of the activation is compared with tests/test_kernels_gpu.py::test_gemm's criteria.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Optional

import numpy as np
import torch

BF = torch.bfloat16
EPI_BIAS, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_RES, EPI_F32_SCALE, EPI_VPAGES = range(7)
EXACT_EPIS = (EPI_BIAS, EPI_GATE_RES, EPI_RES, EPI_F32_SCALE, EPI_VPAGES)
SMALL, V2, V6, V8 = 1, 2, 3, 4                       # plan[0]: GemmKernel (csrc/kernels.h)
NO_TAIL, SPLITK, TAIL128_8, TAIL128_4 = 0, 1, 2, 3   # plan[1]: GemmTail
A_MAX = W_MAX = 2                                    # |A|, |W| <= 2, integers
BIAS_MAX, GATE_MAX, RES_MAX = 8.0, 2.0, 32.0         # bias k/2, gate k/8, res k/4: all bf16-exact (at most 8 significant bits)
CANARY_BF16, CANARY_F32 = 0x7FA5, 0x7FA5A5A5         # NaN patterns no kernel produces
SLACK_ROWS = 2                                       # canary rows before and after every KV page, 3 behind C
ALPHA_T5 = float(np.float32(1.0 / math.sqrt(384.0)))


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    epi: int
    # expected path (what the issue's table names; at 32 CUs per XCD): kernel, tail, staged epilogue, split-K parts, main launch
    kernel: int
    tail: int = NO_TAIL
    staged: int = 0
    splitk_s: int = 1
    main: str = "tiles"            # "tiles": one block per tile; "percu": persistent, one block per CU; "none": main launch skipped
    # form
    rpf: int = 0                   # rows_per_frame (epi 3 and 6)
    inplace: bool = False          # res is C
    bias: bool = True
    alpha: float = 1.0
    lda: int = 0                   # 0 = K
    ldw: int = 0
    ldc_pad: int = 0               # ldc = N + ldc_pad (in-place: ldres too)
    c_off: int = 0                 # C (and an in-place res) starts this many elements into its buffer
    gate_stride: int = 0           # 0 = N; 3 * N: gate row f at gate + N + f * 3 N (the middle of three modulation vectors)
    batch: int = 1
    sA: int = 0
    sW: int = 0
    sC: int = 0
    ldc: int = 0                   # batched: the row stride of C (0 = N + ldc_pad)
    v_col0: int = 0                # epi 6
    v_ld: int = 0                  # 0 = N - v_col0
    v_page_off: int = 0            # epi 6: page 1 starts this many elements later (4: not 16-byte aligned -> direct epilogue)
    scratch: bool = False          # hand in the split-K scratch (tile tickets + counters + partials)
    tickets: bool = False          # hand in tile tickets only

    # ---- derived
    @property
    def LDA(self): return self.lda or self.K
    @property
    def LDW(self): return self.ldw or self.K
    @property
    def LDC(self): return self.ldc or (self.N + self.ldc_pad)
    @property
    def n_c(self): return self.v_col0 if self.epi == EPI_VPAGES else self.N      # columns of C that are written
    @property
    def n_frames(self): return (self.M + self.rpf - 1) // self.rpf if self.rpf else 1
    @property
    def GATE_STRIDE(self): return self.gate_stride or self.N
    @property
    def V_LD(self): return self.v_ld or (self.N - self.v_col0)
    @property
    def input_key(self): return (self.M, self.N, self.K, self.batch, self.LDA, self.LDW, self.sA, self.sW)


def _cases():
    c = []
    add = lambda name, M, N, K, epi, kernel, **kw: c.append(Case(f"{name}-{M}x{N}x{K}-epi{epi}", M, N, K, epi, kernel, **kw))
    # ---- small kernel: N % 8 == 4, one k-tile, rows_per_frame 97, null bias for epi 0, res is C for epi 3 / 4
    for epi in (0, 1, 2, 3, 4, 6):
        add("small", 200, 132, 64, epi, SMALL, rpf=97, inplace=epi in (3, 4), bias=epi != 0, ldc_pad=4 if epi == 1 else 0,
            v_col0=68 if epi == 6 else 0)
    # ---- batched, as T5 launches them: QK^T (fp32 out, heads side by side in one [L, 3 * dim_attn] qkv matrix) and PV (column blocks
    # of one [L, dim_attn] matrix)
    for L in (192, 200):
        for i, alpha in enumerate((0.125, ALPHA_T5)):
            add(f"t5qk-a{i}", L, L, 64, 5, SMALL, batch=3, lda=576, ldw=576, sA=64, sW=64, sC=L * L, alpha=alpha)
    add("t5pv", 192, 64, 192, 0, SMALL, batch=3, sA=192 * 192, sW=64 * 192, ldc=192, sC=64, bias=False)
    # ---- v2 (256 x 128 tiles: M >= 1024, 128 <= N < 256), in place
    for N in (192, 132):
        for epi in (0, 3, 4):
            add("v2", 1064, N, 128, epi, V2, rpf=200, inplace=epi != 0, ldc_pad=8 if (N == 192 and epi == 4) else 0)
    # ---- v6, one block per tile
    for epi in (0, 3):
        add("v6-min", 1024, 256, 128, epi, V6, staged=1, rpf=300, inplace=epi == 3)
    for epi in (0, 1, 2, 3, 4):
        add("v6-staged", 1100, 520, 192, epi, V6, staged=1, rpf=300, inplace=epi in (3, 4), ldc_pad=8 if epi in (0, 4) else 0)
    for rpf in (128, 130, 200):       # the staged gate pick holds two candidate frames per 128-row sub-tile: frames of >= 128 rows
        add(f"v6-staged-rpf{rpf}", 1100, 520, 192, 3, V6, staged=1, rpf=rpf, inplace=True, gate_stride=3 * 520)
    add("v6-direct-rpf97", 1100, 520, 192, 3, V6, rpf=97, inplace=True, gate_stride=3 * 520)
    for epi in (0, 3):
        add("v6-direct-n4", 1100, 516, 192, epi, V6, rpf=200, inplace=epi == 3, bias=epi != 0)
    for epi in (0, 4):
        add("v6-direct-coff", 1100, 520, 192, epi, V6, c_off=4, ldc_pad=4, inplace=epi == 4)
    for i, alpha in enumerate((0.125, ALPHA_T5)):   # the VAE mid-block form: fp32 out, strided operands
        add(f"v6-direct-f32-a{i}", 1100, 520, 192, 5, V6, alpha=alpha, lda=3 * 192, ldw=3 * 192)
    # ---- epi 6: the fused qkv projection, V third into per-frame pages (d = 256; 6 frames of 200 rows, the last one partial)
    add("vpages-staged", 1100, 768, 256, 6, V6, staged=1, rpf=200, v_col0=512)
    add("vpages-staged-vld", 1100, 768, 256, 6, V6, staged=1, rpf=200, v_col0=512, v_ld=264)
    add("vpages-direct-pageoff", 1100, 768, 256, 6, V6, rpf=200, v_col0=512, v_page_off=4)
    add("vpages-small", 600, 768, 256, 6, SMALL, rpf=97, v_col0=512)            # 7 frames of the 8 a launch may name
    # ---- v8 (N >= 8192), one block per tile
    for M, N in ((1024, 8192), (1030, 8200)):
        for epi in (0, 1, 3, 5):
            add("v8", M, N, 128, epi, V8, staged=int(epi != 5), rpf=200, inplace=epi == 3, alpha=ALPHA_T5 if epi == 5 else 1.0,
                ldc_pad=8 if (epi == 0 and N == 8200) else 0)
    # ---- tile tickets: 9 x 29 = 261 tiles, a persistent v6 main launch over the full rounds plus one leftover tile per XCD as quadrants
    add("tickets", 2304, 7424, 128, 3, V6, tail=TAIL128_8, staged=1, main="percu", rpf=300, inplace=True, tickets=True)
    # ---- 128 x 128 tail: 96 tiles = 12 per XCD, no full round (main launch skipped, register-staged body); 264 tiles = v8 round + 1 per XCD
    for epi in (3, 4, 0, 6):
        add("tail128-4", 2048, 3072, 128, epi, V6, tail=TAIL128_4, staged=1, main="none", rpf=300, inplace=epi in (3, 4), tickets=True,
            v_col0=2048 if epi == 6 else 0)
    for epi in (3, 4, 0):
        add("tail128-8", 2048, 8448, 128, epi, V8, tail=TAIL128_8, staged=1, main="percu", rpf=300, inplace=epi in (3, 4), tickets=True)
    # ---- split-K tail (K >= 4096, scratch): 16 tiles in 4 parts; 80 tiles in 3 uneven parts of 64 k-tiles; 128 tiles in 2 parts;
    # 65 k-tiles over 4 parts; 258 tiles = a full round + 1 per XCD
    for M, N, K, s, main in ((1024, 1024, 4096, 4, "none"), (2048, 2560, 4096, 3, "none"), (2048, 4096, 4096, 2, "none"),
                             (1024, 1024, 4160, 4, "none"), (10908, 1536, 4096, 4, "percu")):
        for epi in (3, 4, 0, 1):
            add("splitk", M, N, K, epi, V6, tail=SPLITK, staged=1, splitk_s=s, main=main, rpf=300, inplace=epi in (3, 4), scratch=True,
                ldc_pad=8 if (epi == 4 and M == 2048) else 0)
    add("splitk-vpages", 2048, 3072, 4096, 6, V6, tail=SPLITK, staged=1, splitk_s=2, main="none", rpf=300, v_col0=2048, scratch=True)  # 14B qkv form
    # ---- scratch given, short K: no split (the four tiles run as quadrants)
    add("scratch-shortk", 1024, 256, 128, 3, V6, tail=TAIL128_8, staged=1, main="none", rpf=300, inplace=True, scratch=True)
    return c


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------- launch plan
def plan_restated(c: Case, per: int = 32):
    """[kernel, tail, staged, main blocks, tail blocks, split-K parts] as the issue's tile arithmetic gives them for `per` CUs per XCD
    (an independent restatement: the GPU test compares it with what mmpl_gemm_ex reports from the launcher's own plan)."""
    M, N, K = c.M, c.N, c.K
    big = c.batch <= 1 and M >= 1024 and N >= 256 and K >= 128
    if not big:
        if c.batch <= 1 and M >= 1024 and N >= 128 and K >= 128:
            return [V2, 0, 0, -(-M // 256) * -(-N // 128), 0, 1]
        return [SMALL, 0, 0, -(-M // 128) * -(-N // 128) * c.batch, 0, 1]
    kernel = V8 if N >= 8192 else V6
    al8 = lambda v: v % 8 == 0
    staged = c.epi != EPI_F32_SCALE and al8(N) and al8(c.LDC) and al8(c.c_off)
    if c.epi == EPI_GATE_RES:
        staged = staged and al8(c.GATE_STRIDE) and c.rpf >= 128
    if c.epi == EPI_VPAGES:
        staged = staged and al8(c.v_col0) and al8(c.V_LD) and al8(c.v_page_off)
    tm, tn = -(-M // 256), -(-N // 256)
    tiles, group = tm * tn, (8 if (tm >= 96 and N < 8192 and K < 8192) else 4)
    counter = c.scratch or c.tickets
    if counter and c.epi != EPI_F32_SCALE:
        dealt = ((tm // group) >> 3) * group * tn
        left = tiles - 8 * dealt
        chunks = [dealt + left // 8 + (1 if x < left % 8 else 0) for x in range(8)]
        tb, main_tiles = max(ch % per for ch in chunks), sum(ch - ch % per for ch in chunks)
        main = min(main_tiles, 8 * per)
        if K // 64 >= 64:
            sp = min(4, per // tb) if tb else 1
            if c.scratch and sp >= 2 and 8 * tb * sp <= 256:
                return [kernel, SPLITK, int(staged), main, 8 * tb * sp, sp]
        elif tb > 0 and 2 * tb <= per:
            return [kernel, TAIL128_8 if 4 * tb <= per else TAIL128_4, int(staged), main, 32 * tb, 1]
    return [kernel, 0, int(staged), 8 * per if (counter and tiles > 8 * per) else tiles, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- geometry
def page_layout(c: Case):
    """epi 6: (element offset of every page in one flat buffer, rows of every page, buffer elements).  The pages lie at shuffled
    addresses with SLACK_ROWS canary rows before and after each."""
    rows = [min(c.rpf, c.M - f * c.rpf) for f in range(c.n_frames)]
    order = list(np.random.RandomState(c.M + c.N).permutation(c.n_frames))
    off, cur = [0] * c.n_frames, 0
    for f in order:
        cur += SLACK_ROWS * c.V_LD
        off[f] = cur + (c.v_page_off if f == 1 else 0)
        cur += rows[f] * c.V_LD + (8 if f == 1 and c.v_page_off else 0)
    return off, rows, cur + SLACK_ROWS * c.V_LD


def c_elems(c: Case):
    return c.c_off + (c.batch - 1) * c.sC + (c.M + 3) * c.LDC


def _strided(buf, shape, strides, offset=0):
    return torch.as_strided(buf, shape, strides, offset)


def c_view(c: Case, buf):
    """The [batch, M, n_c] window of C's buffer a launch may write."""
    return _strided(buf, (c.batch, c.M, c.n_c), (c.sC, c.LDC, 1), c.c_off)


def page_views(c: Case, vbuf):
    off, rows, _ = page_layout(c)
    return [_strided(vbuf, (rows[f], c.N - c.v_col0), (c.V_LD, 1), off[f]) for f in range(c.n_frames)]


def canary(n, dtype, device="cpu"):
    if dtype == torch.float32:
        return torch.full((n,), CANARY_F32, dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((n,), CANARY_BF16, dtype=torch.int16, device=device).view(BF)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _randint(g, n, lo, hi, step):
    return (torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32).float() * step).to(BF)


@functools.lru_cache(maxsize=2)
def operands(key):
    """A and W buffers of an input key (shared by every epilogue of a shape): integers in [-2, 2], also outside the windows a launch reads."""
    M, N, K, batch, lda, ldw, sA, sW = key
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + batch)
    a = _randint(g, (batch - 1) * sA + (M - 1) * lda + K, -A_MAX, A_MAX, 1.0)
    w = _randint(g, (batch - 1) * sW + (N - 1) * ldw + K, -W_MAX, W_MAX, 1.0)
    return a, w


def operand_views(c: Case, a, w):
    return _strided(a, (c.batch, c.M, c.K), (c.sA, c.LDA, 1)), _strided(w, (c.batch, c.N, c.K), (c.sW, c.LDW, 1))


def epilogue_inputs(c: Case):
    """bias [N] (k / 2), gate buffer (k / 8, |.| <= 2; row f at GATE_OFF + f * GATE_STRIDE), res [M, N] (k / 4, |.| <= 32)."""
    g = torch.Generator().manual_seed(7919 * c.M + 31 * c.N + c.epi)
    bias = _randint(g, c.N, -int(2 * BIAS_MAX), int(2 * BIAS_MAX), 0.5) if c.bias and c.epi != EPI_F32_SCALE else None
    gate = _randint(g, c.n_frames * c.GATE_STRIDE, -int(8 * GATE_MAX), int(8 * GATE_MAX), 0.125) if c.epi == EPI_GATE_RES else None
    res = _randint(g, c.M * c.N, -int(4 * RES_MAX), int(4 * RES_MAX), 0.25).view(c.M, c.N) if c.epi in (EPI_GATE_RES, EPI_RES) else None
    return bias, gate, res


def gate_off(c: Case):
    return c.N if c.gate_stride else 0


def gate_rows(c: Case, gate):
    """The gate vector of every row: frame = m / rows_per_frame."""
    frame = torch.arange(c.M, device=gate.device) // c.rpf
    return _strided(gate, (c.n_frames, c.N), (c.GATE_STRIDE, 1), gate_off(c))[frame]


# ---------------------------------------------------------------------------------------------------------------- reference
def accumulate(c: Case, a, w):
    """float64 [batch, M, N] accumulator (exact integers) on the operands' device."""
    av, wv = operand_views(c, a, w)
    return torch.matmul(av.double(), wv.double().transpose(1, 2))


def _held_fp32(x64, amb):
    """x64 is a value the kernel holds in an fp32 register: it must be representable (else the reference would be ambiguous)."""
    x32 = x64.float()
    amb[0] += int((x32.double() != x64).sum())
    return x32


GELU_C0, GELU_C1 = math.sqrt(2.0 / math.pi), 0.044715


def activation(epi: int, x):
    """The fp32 (or, for a float64 x, the float64) restatement of GELU(approximate='tanh') / SiLU, in the form that keeps its relative
    accuracy at every pre-activation: 0.5 x (1 + tanh u) == x / (1 + exp(-2 u)), u = sqrt(2 / pi) (x + 0.044715 x^3).

    The integer accumulator puts a good part of the pre-activations far below zero (sigma = 2 sqrt(K) >= 16), where the textbook form
    that F.gelu evaluates has no digits left in fp32: 1 + tanh u is a difference of two numbers next to 1, quantised to 2^-24, and
    exactly 0 from x = -5.5 on, while the true value is x * 1e-7 .. x * 1e-38 -- thousands of bf16 ulps from -0.0, at an absolute
    distance of 1e-6 and less.  tests/test_gemm_ref.py holds this form to 1 bf16 ulp of its float64 evaluation at every pre-activation
    a case can produce (values below 2^-120, where fp32's exp overflows, apart); F.gelu's fp32 result is tens to thousands of ulps off for -10 <= x <= -5.  (tests/test_kernels_gpu.py::test_gemm's
    pre-activations are ~N(0, 1) and never get there.)  F.silu already is x / (1 + exp(-x))."""
    if epi == EPI_SILU:
        return x / (1.0 + torch.exp(-x))
    u = GELU_C0 * (x + GELU_C1 * x * x * x)
    return x / (1.0 + torch.exp(-2.0 * u))


def epilogue(c: Case, acc, bias, gate, res):
    """acc float64 [batch, M, N] -> (out [batch, M, N] bf16 or fp32, pre-activation bf16 or None, number of ambiguous elements)."""
    amb = [0]
    _held_fp32(acc, amb)
    if c.epi == EPI_F32_SCALE:
        return (acc * float(np.float32(c.alpha))).float(), None, amb[0]                 # one RNE of the exact float64 product
    pre = acc if bias is None else acc + bias.double()
    v = _held_fp32(pre, amb).to(BF)                                                     # Linear output rounds to bf16
    if c.epi in (EPI_GELU, EPI_SILU):
        return activation(c.epi, v.float()).to(BF), v, amb[0]
    if c.epi in (EPI_BIAS, EPI_VPAGES):
        return v, v, amb[0]
    t = v
    if c.epi == EPI_GATE_RES:
        t = _held_fp32(v.double() * gate_rows(c, gate).double(), amb).to(BF)            # y * e rounds
    return _held_fp32(res.double() + t.double(), amb).to(BF), v, amb[0]                 # x + (.) rounds at the pack


@dataclasses.dataclass
class Expected:
    c_buf: torch.Tensor                 # C's whole buffer after the launch (canaries where nothing may be written)
    c_written: torch.Tensor             # bool, same length: the elements a launch writes
    v_buf: Optional[torch.Tensor]       # the pages' whole buffer after the launch
    v_written: Optional[torch.Tensor]
    ambiguous: int


def initial_buffers(c: Case, res, device):
    """C's buffer (canaries; the residual inside the window for an in-place case) and the pages' buffer before a launch."""
    cb = canary(c_elems(c), torch.float32 if c.epi == EPI_F32_SCALE else BF, device)
    if c.inplace:
        c_view(c, cb)[0].copy_(res)
    vb = canary(page_layout(c)[2], BF, device) if c.epi == EPI_VPAGES else None
    return cb, vb


def expected(c: Case, acc, bias, gate, res) -> Expected:
    out, _, amb = epilogue(c, acc, bias, gate, res)
    cb, vb = initial_buffers(c, res, out.device)
    cw = torch.zeros(cb.numel(), dtype=torch.bool, device=out.device)
    c_view(c, cb).copy_(out[:, :, :c.n_c])
    c_view(c, cw).fill_(True)
    vw = None
    if vb is not None:
        vw = torch.zeros(vb.numel(), dtype=torch.bool, device=out.device)
        for f, (pv, pw) in enumerate(zip(page_views(c, vb), page_views(c, vw))):
            pv.copy_(out[0, f * c.rpf: f * c.rpf + pv.shape[0], c.v_col0:])
            pw.fill_(True)
    return Expected(cb, cw, vb, vw, amb)


def exactness_bounds(c: Case):
    """The quantum q and the bound B of every fp32-held intermediate of case c, from the input RANGES alone: each is an integer multiple
    of q with |.| <= B, so it is exact in fp32 iff B / q < 2^24."""
    acc = c.K * A_MAX * W_MAX
    out = [("acc", 1.0, acc)]
    if c.epi == EPI_F32_SCALE:
        return out
    pre = acc + (BIAS_MAX if c.bias else 0)
    out.append(("acc + bias", 0.5, pre))
    v = pre * (1 + 2.0 ** -8)                                   # after RNE to bf16 (still a multiple of 1/2 or coarser)
    if c.epi == EPI_GATE_RES:
        out.append(("y * gate", 0.5 * 0.125, v * GATE_MAX))
        out.append(("x + t", 0.0625, RES_MAX + v * GATE_MAX * (1 + 2.0 ** -8)))
    if c.epi == EPI_RES:
        out.append(("x + y", 0.25, RES_MAX + v))
    return out
