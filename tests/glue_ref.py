"""Exact-input reference of the glue kernels of csrc/t5.hip (gather, softmax, transpose, gated GELU, zero-pad), of csrc/i2v.hip
(gelu_erf, add) and of the bf16 UniPC step (csrc/sampler.hip), one launch at a time through mmpl_t5_gather,
mmpl_t5_softmax, mmpl_t5_transpose, mmpl_t5_gated, mmpl_t5_zero_pad, mmpl_gelu_erf, mmpl_add and mmpl_cfg_unipc_step / _table: the
case tables of tests/test_glue_exact_gpu.py, seeded generators, the buffer geometry (canaries), references in numpy float64 /
float32, independent fp32 emulations with the value mutations the tests must catch, and the criteria.  numpy only: importable
without a GPU (tests/test_glue_ref.py proves, on the CPU, every condition the comparisons rest on).  The bf16 helpers, Expect and
cand are tests/rowpass_ref.py's.

u = 2^-24.  Canaries (0x7FA5, a NaN no kernel produces) stand behind every buffer and in every ld gap.  An element is AMBIGUOUS when
its candidates differ; at most AMBIGUITY_CAP = 1 % of a case, asserted from the reference alone.

Bit for bit, no allowance.
  gather      a copy of 16-byte chunks: rows of random 16-bit patterns (NaNs included), ids 0, vocab - 1, repeats, arbitrary.
  transpose   a copy: every source element distinct where the shape allows, else random patterns; the ragged 70 x 40 case runs the
              bounds branches of both tile loops; the production form reads the V third of a [L, 3 H c] matrix.
  zero-pad    rows under mask == 0 become +0, kept rows (arbitrary patterns, NaNs included) are untouched.
  add         ONE fp32 add of two bf16 values and one RNE: numpy float32 does exactly that.  The operands are finite and their sum is
              zero or at least 2^-126 in magnitude (`no_subnormal`: the project states no flush mode, so no bit-exact case may depend on one).
  UniPC       every operation of the bf16 UniPC solver is one IEEE fp32 operation between two bf16 roundings, so the kernel equals the
              emulation (tests/test_scheduler_host.py: emulate_kernel; restated here in numpy as `unipc_chain`, which also returns
              every intermediate for the subnormal check) in every bit of x, m0, m1 and last_sample, or it is wrong.

t5_gated_kernel.  x = g; p3 = bf16(x x x) (both products exact in fp32: 8-bit significands), u = bf16(x + bf16(0.044715f p3)),
z = bf16(0.79788456f u), th = bf16(tanhf(z)), gl = bf16(bf16(0.5 x) bf16(1 + th)), f = bf16(f gl): everything but tanhf is a single
fp32 operation on bf16 operands and is repeated in numpy float32.  tanhf has no installed bound; the project's allowance for it is
vae_kernel_ref.TIE_REL = 2^-18 relative, so th is one of bf16(tanh64(z) (1 -+ 2^-18)) and the rest of the chain runs on each.
Where g^3 overflows, z = +-inf and tanh is exactly +-1.  Of the 38 491 distinct finite z none is ambiguous.  The 512 inputs with
|g| < 2^-125 (0.5 g, 0.797 g or g itself below the smallest normal fp32) instead carry the absolute 2^-126 |f| around f g / 2:
whether such intermediates are flushed is not stated; they are 0.78 % of a case and the only ambiguous elements.  |f| lies in
[1, 16), so no product f gl is subnormal beside those.  (Below |g| = 2^-42 the cube underflows, but any value in
[0, 0.045 |g|^3] leaves u = g, flushed or not.)

gelu_erf_kernel, in place: t = fl(v c) with c = float32(1 / sqrt 2), e = erff(t), s = fl(1 + e), p = fl((0.5 v) s), bf16(p).  Against
y = 0.5 v erfc(-v / sqrt 2) in float64 (erfc: no cancellation at v < 0) the fp32 value lies within
    D = 0.5 |v| (K ulp32(erf t) + 2 u |t| erf'(t) + u |1 + erf t|) + u |y|
(K ulps of erff; the rounding of t and of c moved through erf'; the rounding of s; the rounding of p), so the element lies in
[bf16(y - D), bf16(y + D)].  K has no installed bound and is measured: ERF_MEASURED is the smallest K under which every element of
case A passed on an MI355X (tests/test_glue_exact_gpu.py prints it, on a grid of 2^(1/4) steps): 0.5 ulp, which is what a correctly
rounded erff needs (tests/test_glue_ref.py: 0.5 for the correctly rounded emulation, 1.4 - 1.7 with erff one ulp off); the allowance
ERF_K is 4 x that, capped at 8 ulp: 2 ulp.  As with rowpass_ref's rsqrtf this rests on the toolchain's erff staying as good as it was
measured; a ROCm whose erff is worse can fail case A with a correct kernel, and the answer then is a new measurement.
  case A  every finite normal bf16 v >= -8 (49 025 values), repeated until n passes the launcher's cap of 4096 x 256 elements, so
          that the stride loop makes a second trip and an element visited twice (gelu of gelu) shows.  17 repetitions, the figure
          first planned, give 833 425 < 1 048 576: GELU_A_REPS = 22.  With K = 8, the cap of the allowance, the reference alone
          leaves 289 of the 49 025 ambiguous (0.59 %), nearly all in v in [-8, -3], where 1 + erf t cancels; with K = 2, 265.
  case B  the subnormal bf16 inputs and +-0, with SiLU's absolute addend 2^-126.  Exempt from the cap: y = 0.5 v is an exact bf16
          tie for every odd multiple of 2^-133, so half the elements are ambiguous by construction, whatever the kernel does.
  case C  every finite v < -8 (15 999 values): 1 + erf t < 2^-50, a saturating erff returns exactly -1 and the element must be -0
          (0x8000) in bits: `GELU_C_BITS`, no interval.

t5_softmax_kernel.  val_j = bf16(bf16(sc_j) + bias_j) and d_j = val_j - max are single fp32 operations, repeated in bits (the
scores are fp32 values that are NOT bf16-representable, so the inner rounding shows).  x_j = exp(d_j) / sum_k exp(d_k) is formed in
float64; the kernel's fp32 value lies in x (1 -+ EPS), EPS = 2 E + 13 u: E covers __expf of the numerator and of the sum's terms;
the sum takes at most ceil(L / 256) - 1 + 6 + 3 <= 10 additions of positive terms (u each), the division is correctly rounded (u),
the product one more (u), one u to spare.  E is measured like ERF_MEASURED (EXP_MEASURED, on a grid of 2^(1/2) steps: at most 2.83 u
over the cases, 0 in the small ones; E = 4 x that = 11.3 u, EPS = 35.6 u, capped at 2^-16 = 256 u): valid keys keep d >= -60 (the
generator reaches -50), where the rounding of d log2(e) alone can be worth |d| log2(e) u.  The candidates are bf16(x (1 -+ EPS)).  Masked keys (bias
= finfo(bfloat16).min) must be +0 in bits.  Anchors, exact with eps 0: an all-masked row is bf16(1 / L) in bits (every val equals
the minimum, every exp is 1, L a power of two), a row of 64 equal valid keys is 2^-6.  The deep case reaches d = -120, where exp(d)
is below the smallest normal fp32 and the element carries the absolute addend 2^-126.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from tests.rowpass_ref import (AMBIGUITY_CAP, CANARY, F32, F64, U, Expect, bf2f, bf16_from_f32, bf16_from_f64, cand, order,  # noqa: F401
                               rbf, to_bf16)

TANH_REL = 2.0 ** -18                                # vae_kernel_ref.TIE_REL: the project's allowance for tanhf
ERF_MEASURED = 0.5                                   # ulps of erff: measured 2026-10-19 on an MI355X (gfx950, ROCm 7.2.0), case A; case B: 0
ERF_K = min(4.0 * ERF_MEASURED, 8.0)                 # 2 ulp
EXP_MEASURED = 2.0 ** -22.5                          # 2.83 u: measured 2026-10-19 on an MI355X (gfx950, ROCm 7.2.0): the largest of the cases
EXP_E = 4.0 * EXP_MEASURED                           # 11.3 u
SOFTMAX_EPS = min(2.0 * EXP_E + 13.0 * U, 2.0 ** -16)   # 35.6 u
ABS_FLOOR = 2.0 ** -126                              # the smallest normal fp32: the absolute addend where a result may be flushed
GELU_C_BITS = 0x8000                                 # case C: -0
GELU_A_REPS = 22                                     # 49 025 x 22 = 1 078 550 > 4096 x 256 (docstring)
GATED_REPS = 33                                      # 65 280 x 33 = 2 154 240 > 8192 x 256
KMIN = F32(-3.3895313892515355e38)                   # torch.finfo(torch.bfloat16).min, the bias of a masked key


def finite_bf16():
    b = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7F80) != 0x7F80]                 # 65 280


def random_bits(rng, shape):
    return rng.integers(0, 1 << 16, size=shape).astype(np.uint16)


def with_canary(a, tail=64):
    """flat copy of a (uint16) followed by `tail` canaries."""
    return np.concatenate([np.ascontiguousarray(a).reshape(-1), np.full(tail, CANARY, dtype=np.uint16)])


def no_subnormal(*arrays):
    """True if every fp32 value is zero, inf / nan or at least 2^-126 in magnitude."""
    for a in arrays:
        v = np.abs(np.asarray(a, dtype=F32))
        if ((v > 0) & (v < ABS_FLOOR)).any():
            return False
    return True


# ------------------------------------------------------------------ gather
@dataclasses.dataclass(frozen=True)
class GatherCase:
    name: str
    vocab: int
    dim: int
    L: int = 64


GATHER_CASES = [GatherCase("gather-d128", 97, 128), GatherCase("gather-d4096", 33, 4096)]


def gather_operands(c: GatherCase):
    rng = np.random.default_rng(4000 + c.dim)
    ids = rng.integers(0, c.vocab, c.L).astype(np.int32)
    ids[:6] = [0, c.vocab - 1, 0, c.vocab - 1, 5, 5]                     # both ends of the table, repeats
    ids[-1] = c.vocab - 1
    return dict(ids=ids, emb=random_bits(rng, (c.vocab, c.dim)))


def gather_ref(op):
    return op["emb"][op["ids"]]


# ------------------------------------------------------------------ transpose
@dataclasses.dataclass(frozen=True)
class TransposeCase:
    name: str
    L: int
    c: int
    H: int
    ld: int
    off: int = 0                   # the column of head 0 inside a row of ld elements


TRANSPOSE_CASES = [TransposeCase("transpose-64x64-h3", 64, 64, 3, 3 * 64),
                   TransposeCase("transpose-128x64-qkv", 128, 64, 2, 3 * 2 * 64, off=2 * 2 * 64),       # v = qkv + 2 H c, ld = 3 H c
                   TransposeCase("transpose-ragged-70x40", 70, 40, 2, 2 * 40 + 8)]


def transpose_operands(c: TransposeCase):
    rng = np.random.default_rng(4100 + c.L + c.c)
    n = c.L * c.ld
    v = (rng.permutation(n) if n <= 1 << 16 else rng.integers(0, 1 << 16, n)).astype(np.uint16).reshape(c.L, c.ld)
    return dict(v=v)


def transpose_ref(c: TransposeCase, op, head_offset=True):
    """vt [H][c][L]; head_offset False: the mutation that reads head 0 for every head."""
    out = np.empty((c.H, c.c, c.L), dtype=np.uint16)
    for h in range(c.H):
        col = c.off + (h * c.c if head_offset else 0)
        out[h] = op["v"][:, col:col + c.c].T
    return out


# ------------------------------------------------------------------ zero-pad
ZERO_PAD_MASKS = ("prefix", "holes", "ones", "zeros")
ZERO_PAD_L, ZERO_PAD_DIM = 64, 72


def zero_pad_operands(kind):
    rng = np.random.default_rng(4200 + ZERO_PAD_MASKS.index(kind))
    L = ZERO_PAD_L
    mask = {"prefix": (np.arange(L) < 37), "holes": rng.integers(0, 2, L) > 0, "ones": np.ones(L, bool), "zeros": np.zeros(L, bool)}[kind]
    mask = mask.astype(np.int32)
    if kind == "holes":
        mask[:4] = [7, 0, -1, 0]                                           # any non-zero int keeps the row
    return dict(mask=mask, out=random_bits(rng, (L, ZERO_PAD_DIM)))


def zero_pad_ref(op):
    out = op["out"].copy()
    out[op["mask"] == 0] = 0
    return out


# ------------------------------------------------------------------ add
ADD_SIZES = (1, 257, 4096 * 256 + 257)               # the last: the stride loop's second trip, a ragged one


def add_operands(n):
    """finite bf16 a, b over 40 binades; every 7th element b = -a (a sum of exactly zero)."""
    rng = np.random.default_rng(4300 + n % 1000)
    a = to_bf16(rng.normal(0, 1, n) * np.exp2(rng.integers(-20, 20, n)))
    b = to_bf16(rng.normal(0, 1, n) * np.exp2(rng.integers(-20, 20, n)))
    b[::7] = a[::7] ^ np.uint16(0x8000)
    return a, b


def add_ref(a, b, mutation=None):
    out = bf16_from_f32(bf2f(a) + bf2f(b))
    if mutation == "stride_start":                   # every thread of a block starts at the block's first element: that one takes b
        idx = np.arange(len(a))                      # again and again, the others never
        first = idx % 256 == 0
        out = np.where(first, bf16_from_f32(bf2f(out) + bf2f(b)), a)
    return out


# ------------------------------------------------------------------ t5_gated_kernel
GATED_SIZES = (1, 257, 65280 * GATED_REPS)
GATED_MUTATIONS = ("half_x_unrounded", "p3_unrounded")   # the first is value-neutral (0.5 x is exact in bf16; see gated_chain)


def gated_operands(n):
    """g: all finite bf16 patterns, repeated (or the first n of a shuffle); f: per element, |f| in [1, 16)."""
    rng = np.random.default_rng(4400 + n % 1000)
    fin = finite_bf16()
    g = np.tile(fin, GATED_REPS) if n == len(fin) * GATED_REPS else rng.permutation(fin)[:n]
    f = to_bf16(rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(0, 4, n)) * rng.choice([-1.0, 1.0], n))
    return f, g


def _tanh32(z, ulp=0):
    with np.errstate(over="ignore"):
        t = np.tanh(z.astype(F64)).astype(F32)
    return t if ulp == 0 else (t.view(np.int32) + ulp).view(F32)


def gated_front(g_bits, mutation=None):
    """g -> (x, z) in fp32: the chain up to tanhf's argument."""
    x = bf2f(g_bits)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p3 = x * x * x
        if mutation != "p3_unrounded":
            p3 = rbf(p3)
        u = rbf(x + rbf(F32(0.044715) * p3))
        z = rbf(F32(0.7978845608028654) * u)
    return x, z


def gated_back(x, th, f_bits, mutation=None):
    """th (fp32 holding a bf16 value) -> the element's bits: bf16(f bf16(bf16(0.5 x) bf16(1 + th)))."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        hx = F32(0.5) * x
        if mutation != "half_x_unrounded":
            hx = rbf(hx)
        gl = rbf(hx * rbf(F32(1.0) + th))
        return bf16_from_f32(bf2f(f_bits) * gl)


def gated_reference(f_bits, g_bits):
    """-> (Expect over [n], z fp32): two candidates of th, the chain on each; the 2^-126 addend where |g| < 2^-125 (docstring)."""
    x, z = gated_front(g_bits)
    with np.errstate(over="ignore"):
        t = np.tanh(z.astype(F64))
    lo, hi = cand(t, TANH_REL)
    a, b = gated_back(x, bf2f(lo), f_bits), gated_back(x, bf2f(hi), f_bits)
    tiny = np.abs(x) < 2.0 ** -125
    if tiny.any():
        fv = bf2f(f_bits[tiny]).astype(F64)
        y = fv * 0.5 * x[tiny].astype(F64)
        D = ABS_FLOOR * np.maximum(1.0, np.abs(fv))
        a, b = a.copy(), b.copy()
        a[tiny], b[tiny] = bf16_from_f64(y - D), bf16_from_f64(y + D)
    return Expect(np.stack([a]), np.stack([b])), z


def gated_emulate(f_bits, g_bits, ulp=0, mutation=None):
    x, z = gated_front(g_bits, mutation)
    return gated_back(x, rbf(_tanh32(z, ulp)), f_bits, mutation)


# ------------------------------------------------------------------ gelu_erf_kernel
def gelu_inputs(case):
    b = finite_bf16()
    v = bf2f(b)
    sub = (b & 0x7F80) == 0                                                # subnormals and +-0
    if case == "A":
        return np.tile(b[~sub & (v >= -8.0)], GELU_A_REPS)
    if case == "B":
        return b[sub]
    return b[v < -8.0]                                                     # C


_erf = np.vectorize(math.erf, otypes=[F64])
_erfc = np.vectorize(math.erfc, otypes=[F64])


def _ulp32(x):
    """the fp32 ulp at |x| (float64 array; x != 0)."""
    return np.exp2(np.floor(np.log2(np.abs(x))) - 23)


def _gelu_parts(ub):
    """distinct inputs -> (v, y, the K-free part of D, the factor of K), all float64."""
    v = bf2f(ub).astype(F64)
    t = v * F64(F32(0.70710678118654752440))
    y = 0.5 * v * _erfc(-t)
    e = _erf(t)
    ulp_e = np.where(e != 0, _ulp32(np.where(e != 0, e, 1.0)), 0.0)
    fixed = 0.5 * np.abs(v) * (2 * U * np.abs(t) * (2 / math.sqrt(math.pi)) * np.exp(-t * t) + U * np.abs(1 + e)) + U * np.abs(y)
    return v, y, fixed, 0.5 * np.abs(v) * ulp_e


def _gelu_expect(parts, K, abs_floor):
    v, y, fixed, per_k = parts
    D = fixed + K * per_k + (ABS_FLOOR * np.maximum(1.0, np.abs(v)) if abs_floor else 0.0)
    return bf16_from_f64(y - D), bf16_from_f64(y + D)


def gelu_ref(bits, K=None, abs_floor=False):
    """-> (Expect over [n], y float64).  Computed on the distinct inputs and scattered."""
    ub, inv = np.unique(bits, return_inverse=True)
    parts = _gelu_parts(ub)
    lo, hi = _gelu_expect(parts, ERF_K if K is None else K, abs_floor)
    return Expect(lo[inv][None], hi[inv][None]), parts[1][inv]


def gelu_emulate(bits, ulp=0, mutation=None):
    """fp32, erff correctly rounded (+ ulp).  mutation 'coarse_constant': 0.7071f for 0.70710677f."""
    v = bf2f(bits)
    c = F32(0.7071) if mutation == "coarse_constant" else F32(0.70710678118654752440)
    with np.errstate(under="ignore"):
        t = v * c
        e = _erf(t.astype(F64)).astype(F32)
        if ulp:
            e = np.clip((e.view(np.int32) + np.where(e == 0, 0, ulp).astype(np.int32)).view(F32), -1.0, 1.0).astype(F32)
        return bf16_from_f32((F32(0.5) * v) * (F32(1.0) + e))


def gelu_needed_K(got, bits, abs_floor=False, top=64.0):
    """Measurement: the smallest K (0, then 2^(1/4) steps from 1/16) under which every element passes."""
    ub, inv = np.unique(bits, return_inverse=True)
    parts = _gelu_parts(ub)
    K = 0.0
    while K <= top:
        lo, hi = _gelu_expect(parts, K, abs_floor)
        if not Expect(lo[inv][None], hi[inv][None]).outside(got).any():
            return K
        K = 1.0 / 16 if K == 0.0 else K * 2.0 ** 0.25
    return float("inf")


# ------------------------------------------------------------------ t5_softmax_kernel
NUM_BUCKETS = 32


@dataclasses.dataclass(frozen=True)
class SoftmaxCase:
    name: str
    H: int
    L: int
    n_valid: int = -1              # -1: L; mask = the first n_valid keys
    holes: bool = False            # a random mask instead
    table: str = "product"         # relative_position_buckets | "synthetic": r % 32
    kind: str = "random"           # scores: "random" | "equal" (one value, constant pos_emb) | "deep" (d down to -120)

    @property
    def valid(self): return self.L if self.n_valid < 0 else self.n_valid


def _softmax_cases():
    out = []
    add = lambda name, H, L, **kw: out.append(SoftmaxCase(f"softmax-{name}", H, L, **kw))
    for H in (1, 3):
        for L in (64, 256, 512):
            add(f"h{H}-l{L}", H, L)
    add("h3-l64-last-masked", 3, 64, n_valid=63), add("h1-l512-last-masked", 1, 512, n_valid=511)
    add("h3-l256-v37", 3, 256, n_valid=37), add("h1-l64-v37", 1, 64, n_valid=37)
    add("h3-l512-v1", 3, 512, n_valid=1), add("h1-l64-v1", 1, 64, n_valid=1)
    add("h3-l256-all-masked", 3, 256, n_valid=0), add("h1-l64-all-masked", 1, 64, n_valid=0), add("h1-l512-all-masked", 1, 512, n_valid=0)
    add("h3-l256-holes", 3, 256, holes=True)
    add("h3-l256-synthetic", 3, 256, table="synthetic")
    add("h1-l64-equal", 1, 64, kind="equal")
    add("h3-l256-deep", 3, 256, kind="deep")
    return out


SOFTMAX_CASES = _softmax_cases()
SOFTMAX_MUTATIONS = ("bias_i_minus_j", "pos_no_head", "score_unrounded", "mask_ignored", "inv_wave0")


def product_buckets(L, num_buckets=NUM_BUCKETS, max_dist=128):
    """mmpl_amd.t5.relative_position_buckets restated in numpy (tests/test_glue_ref.py compares the two): int32 [2 L - 1]."""
    rel = np.arange(-(L - 1), L)
    nb = num_buckets // 2
    out = (rel > 0).astype(np.int64) * nb
    rel = np.abs(rel)
    max_exact = nb // 2
    large = max_exact + (np.log(np.maximum(rel, 1).astype(F32) / F32(max_exact)) / F32(math.log(max_dist / max_exact)) * (nb - max_exact)).astype(np.int64)
    large = np.minimum(large, nb - 1)
    return (out + np.where(rel < max_exact, rel, large)).astype(np.int32)


def softmax_operands(c: SoftmaxCase, bucket=None):
    """-> dict: sc float32 [H, L, L], pos bf16 bits [32, H], bucket int32 [2 L - 1], mask int32 [L]."""
    rng = np.random.default_rng(4500 + 7 * c.H + c.L + len(c.name))
    H, L = c.H, c.L
    if bucket is None:
        bucket = product_buckets(L) if c.table == "product" else (np.arange(2 * L - 1) % NUM_BUCKETS).astype(np.int32)
    pos = to_bf16((np.arange(NUM_BUCKETS * H).reshape(NUM_BUCKETS, H) - 16.0 * H) / 32.0)       # distinct per (bucket, head), |.| <= 1.5
    mask = (np.arange(L) < c.valid).astype(np.int32)
    if c.holes:
        mask = (rng.integers(0, 3, L) > 0).astype(np.int32)
        mask[[0, L - 1]] = [0, 1]
    if c.kind == "equal":
        sc = np.full((H, L, L), 1.3, dtype=F32)
        pos = to_bf16(np.full((NUM_BUCKETS, H), 0.5))
    else:
        sc = np.clip(rng.normal(0.0, 6.0, (H, L, L)), -28.0, 28.0).astype(F32)                   # |bias| <= 1.5: val - max >= -60
        if c.kind == "deep":
            sc[:, ::2, 5] -= F32(90.0)                                                           # one key of every other row: d below -120
        rep = bf2f(bf16_from_f32(sc)) == sc
        sc[rep] = np.nextafter(sc[rep], F32(np.inf))                                             # no score is bf16-representable
    return dict(sc=sc, pos=pos, bucket=np.asarray(bucket, dtype=np.int32), mask=mask)


def softmax_vals(c: SoftmaxCase, op, mutation=None):
    """val fp32 [H, L, L] = bf16(bf16(sc) + bias): single fp32 operations."""
    H, L = c.H, c.L
    i, j = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    rel = (i - j if mutation == "bias_i_minus_j" else j - i) + L - 1
    b = op["bucket"][rel]                                                   # [L, L]
    h = np.zeros(H, dtype=np.int64) if mutation == "pos_no_head" else np.arange(H)
    bias = bf2f(op["pos"].reshape(-1)[b[None] * H + h[:, None, None]])      # [H, L, L]
    if mutation != "mask_ignored":
        bias = np.where(op["mask"][None, None, :] != 0, bias, KMIN)
    s = op["sc"] if mutation == "score_unrounded" else rbf(op["sc"])
    with np.errstate(over="ignore"):
        return rbf(s + bias)


def _softmax_expect(x, d, eps):
    lo, hi = cand(x, eps)
    deep = d.astype(F64) < math.log(ABS_FLOOR)                              # exp(d) below the smallest normal fp32
    if deep.any():
        lo[deep] = bf16_from_f64(np.maximum(x[deep] * (1 - eps) - ABS_FLOOR, 0.0))
        hi[deep] = bf16_from_f64(x[deep] * (1 + eps) + ABS_FLOOR)
    zero = x == 0                                                           # masked keys beside a valid one: +0, not -0
    lo[zero], hi[zero] = 0, 0
    return Expect(lo[None], hi[None])


def softmax_reference(c: SoftmaxCase, op, eps=None):
    """-> (Expect over [H, L, L], x float64, d fp32).  Masked keys of a row with a valid key: exactly +0."""
    val = softmax_vals(c, op)
    d = val - val.max(axis=-1, keepdims=True)                               # one fp32 subtraction
    e = np.exp(d.astype(F64))
    x = e / e.sum(axis=-1, keepdims=True)
    return _softmax_expect(x, d, SOFTMAX_EPS if eps is None else eps), x, d


def softmax_zero_bits(c: SoftmaxCase, op):
    """Where the output must be 0x0000 in bits: masked keys of rows that have a valid key."""
    m = op["mask"] != 0
    return np.broadcast_to(~m[None, None, :], (c.H, c.L, c.L)) & m.any()


def softmax_emulate(c: SoftmaxCase, op, mutation=None):
    """fp32 emulation in the kernel's order: per-thread strided sums, the butterfly of each wave, red[0] + red[1] + red[2] + red[3],
    a correctly rounded exp, one division, one product."""
    H, L = c.H, c.L
    val = softmax_vals(c, op, mutation)
    d = val - val.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(d.astype(F64)).astype(F32)                               # [H, L, L]
    ep = np.zeros((H, L, ((L + 255) // 256) * 256), dtype=F32)
    ep[..., :L] = e
    t = ep.reshape(H, L, -1, 256)
    part = t[:, :, 0]
    for k in range(1, t.shape[2]):
        part = part + t[:, :, k]                                            # thread partials [H, L, 256]
    w = part.reshape(H, L, 4, 64)
    n = 64
    while n > 1:
        n //= 2
        w = w[..., :n] + w[..., n:2 * n]
    red = w[..., 0]                                                         # [H, L, 4]
    total = red[..., 0] if mutation == "inv_wave0" else (red[..., 0] + red[..., 1]) + red[..., 2] + red[..., 3]
    inv = F32(1.0) / total
    return bf16_from_f32(e * inv[..., None])


def softmax_needed_E(got, x, d, top=2.0 ** -12):
    """Measurement: the smallest E (0, then 2^(1/2) steps from u / 4) under which every element passes with eps = 2 E + 13 u
    (x, d: softmax_reference's)."""
    E = 0.0
    while E <= top:
        if not _softmax_expect(x, d, 2 * E + 13 * U).outside(got).any():
            return E
        E = U / 4 if E == 0.0 else E * 2.0 ** 0.5
    return float("inf")


# ------------------------------------------------------------------ UniPC
UNIPC_STEPS = (0, 1, 2, 25, 49)                      # of the 50-step, shift-5 schedule at guidance 5
UNIPC_ORDERS = {0: (0, 1, 1), 1: (1, 1, 2), 2: (1, 2, 2), 25: (1, 2, 2), 49: (1, 2, 1)}   # (use_corrector, corr_order, pred_order)
UNIPC_SIZES = (1, 255, 8192 * 256 + 257)             # 2 097 409: a lone element-wise tail, a tail behind 31 vectors, 1025 blocks + a tail
UNIPC_MUTATIONS = ("diff_unrounded", "pred_m_swapped", "half_d1_unrounded")   # the last is value-neutral (0.5 d1 is exact in bf16)
UNIPC_FIELDS = ("guidance", "sigma_cur", "use_corrector", "corr_order", "c_c1", "c_c2", "c_c3", "c_inv_rk", "c_rho0", "c_rho_last",
                "pred_order", "p_c1", "p_c2", "p_c3", "p_inv_rk")


def unipc_operands(n, seed=0):
    """six bf16 tensors of N(0, 1): flow_cond, flow_uncond, x, m0, m1, last_sample."""
    rng = np.random.default_rng(4600 + seed + n % 1000)
    return [to_bf16(rng.normal(0, 1, n)) for _ in range(6)]


def unipc_chain(st, fc, fu, x, m0, m1, last, mutation=None):
    """the bf16 UniPC solver of csrc/sampler.hip in numpy float32 (st: any object with MmplUniPCStep's fields; fu None = fc is the combined flow).
    -> (x, m0, m1, last_sample as bf16 bits, the list of every fp32 intermediate)."""
    s = lambda k: F32(getattr(st, k))
    mids = []

    def r(v):
        mids.append(v)
        return rbf(v)

    flow, x, m0, m1, last = bf2f(fc), bf2f(x), bf2f(m0), bf2f(m1), bf2f(last)
    if fu is not None:
        f_u = bf2f(fu)
        diff = flow - f_u
        if mutation != "diff_unrounded":
            diff = r(diff)
        flow = r(f_u + r(s("guidance") * diff))
    m_conv = r(x - r(s("sigma_cur") * flow))
    if st.use_corrector:
        xt_ = r(r(s("c_c1") * last) - r(s("c_c2") * m0))
        acc = r(s("c_rho_last") * r(m_conv - m0))
        if st.corr_order == 2:
            acc = r(r(s("c_rho0") * r(r(m1 - m0) * s("c_inv_rk"))) + acc)
        x = r(xt_ - r(s("c_c3") * acc))
    m1, m0, last = m0, m_conv, x
    xt = r(r(s("p_c1") * x) - r(s("p_c2") * m0))
    if st.pred_order == 2:
        d1 = r(r((m0 - m1) if mutation == "pred_m_swapped" else (m1 - m0)) * s("p_inv_rk"))
        h = F32(0.5) * d1
        if mutation != "half_d1_unrounded":
            h = r(h)
        xt = r(xt - r(s("p_c3") * h))
    return [bf16_from_f32(v) for v in (xt, m0, m1, last)], mids
