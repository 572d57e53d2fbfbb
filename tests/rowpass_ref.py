"""Exact-input reference of the row passes and small kernels of csrc/elementwise.hip, one launch at a time through mmpl_layernorm_ex,
mmpl_qknorm_ex, mmpl_modulation, mmpl_patchify, mmpl_unpatchify, mmpl_sinusoid, mmpl_silu and mmpl_rows_equal_last: the case tables
of tests/test_rowpass_exact_gpu.py, a seeded generator, the buffer geometry (canaries), references in numpy float64 / float32, an
independent fp32 emulation with the value mutations the tests must catch, and the criterion.  numpy only: importable without a GPU
(tests/test_rowpass_ref.py proves, on the CPU, every condition the comparison rests on).

The construction, u = 2^-24.
LayerNorm.  A row holds small integers (exact in bf16) whose sum is a multiple of d / 8, so mean = sum / d = m / 8 has at most 3
fractional bits: sum (any order: |partial| <= sum |x| < 2^24), the fp32 quotient, every x - mean (a multiple of 1/8 below 2^8) and
every square (a multiple of 1/64) are exact, and so is the sum of squares in any order as long as 64 sum (x - mean)^2 < 2^24
(`ln_exact`; the amplitude `ln_amp(d)` is chosen for it: |x| <= 6, |mean| < 1 at d = 5120 gives 64 * 5120 * 49 = 1.61e7 < 2^24 = 1.68e7).
RMSNorm.  |x| <= 9: sum x^2 <= 81 * 5120 < 2^19, exact in any order.
What the kernel computes inexactly is r = rsqrtf(stat / d + eps) and t = fl32(v * r); the first ROUNDED quantity is bf16(t).  With
x the float64 value of v / sqrt(stat / d + eps) the kernel's t lies in x (1 -+ EPS), so bf16(t) is one of the two candidates
bf16_rne(x (1 -+ EPS)) (rounding is monotonic; bf16_rne rounds the float64 ONCE, `bf16_from_f64`).  Everything behind that rounding
is a single IEEE fp32 operation on bf16 operands or an exact one, and the reference repeats it bit for bit in numpy float32 on
each candidate:
    modulation   s1 = bf16(1 + scale) (one fp32 add), bf16(n * s1) (a product of two 8-bit significands: exact in fp32), + shift
                 (one fp32 add), pack (bf16_rne of an fp32);
    RMSNorm      bf16(bf16(t) * w) (exact product, one rounding), * q_scale (one fp32 product), pack;
    RoPE, exact  the table holds dyadic k / 16, |k| <= 16 (`exact_tables`: a hash of position and pair): re * cs and im * sn have 13-bit
                 significands and, the gains being within [0.5, 2) in magnitude, exponents so close that re cs - im sn is exact in
                 fp32 however it is contracted (`qk_exact` asserts it on all four candidate combinations of every pair);
    affine       nothing is rounded before the fma: y = fma(t, w, b) carries EPS |t w| from t and u |y| from its own rounding, so there
                 the criterion is the interval [bf16_rne(y - D), bf16_rne(y + D)], D = EPS |t w| + u |y|, of the float64 y.
    RoPE, real   (`real_tables`: float32(cos), float32(sin) of the model's frequencies) the four products / fmas of a pair round up to
                 three times: the float64 rotation of each candidate combination with D = 3 u (|re cs| + |im sn|) (+ 2^-50 relative for
                 the float64 arithmetic itself), then * q_scale in fp32 and the pack, both monotonic: an interval per combination.
A kernel element passes if it equals a candidate's result in bits or lies strictly inside a combination's interval; for x == 0 the
candidates are +0 and -0.  No element is excluded.  An element is AMBIGUOUS when its candidates' results differ; at most
AMBIGUITY_CAP = 1 % of a case (asserted from the reference alone in tests/test_rowpass_ref.py).

EPS.  Derivation: stat exact; the quotient stat / d and the sum with eps are one fp32 rounding each (u relative each, halved by the
square root: u together); rsqrtf at 1 ulp = 2 u; the product v * r one more u: 4 u.  The "1 ulp" of rsqrtf is the HIP math API's
accuracy table, which is NOT installed with this toolchain, so the number is measured instead, the way attn_ref.COPIES_MEASURED was:
RSQRT_MEASURED is the smallest eps under which every element of every norm case passed on an MI355X against the float64 reference
(tests/test_rowpass_exact_gpu.py prints it per case), the allowance EPS is 4 x that, capped at 2^-16.  Only a case with very many
distinct values of v * r can tell: the rows of the ordinary cases hold a few dozen distinct values each, none of them within 4 u of
a bf16 tie, and every one of their elements equals bf16_rne(x) (needed eps 0).  qk-rms-measure-d512 (4096 rows, |x| <= 100, some
7e5 distinct values) is the case the number comes from: 0.42 u (2^-25.25, on the measurement's grid of 2^(1/8) steps), so EPS = 1.68 u.
That is LESS than the derived 4 u, and less than an fp32 emulation needs whose rsqrt is moved by a whole ulp (2.6 u on that case;
0.77 u with a correctly rounded one; the affine LayerNorm cases, where every element tells, show the same): tests/test_rowpass_ref.py
therefore holds the correctly rounded emulation of every case to EPS, the criterion, and the +-1 ulp emulations to EPS_DERIVED.
So the criterion rests on an ASSUMPTION that nothing here measures for other toolchains: that rsqrtf stays as much better than its
documented 1 ulp as this ROCm's is on this device.  A ROCm version whose rsqrtf merely meets the documented bound can fail
qk-rms-measure-d512 and the affine cases with a correct kernel; the answer then is a new measurement (the tests print the needed
eps per case), not a kernel change.
silu_kernel (x * v_rcp_f32(1 + __expf(-x))) has no documented bound either: SILU_MEASURED likewise (1.19 u), SILU_EPS = 4 x, capped at 2^-12,
relative to y = x / (1 + exp(-x)) in float64, plus the absolute 2^-126 max(1, |x|): v_exp_f32 / v_rcp_f32 return zero for results
below the smallest normal fp32 (exp(-x) overflows to inf from x < -88.7, where y is still a normal bf16), and x times that is the
element.  All 65 280 finite bf16 values are the input.
Sinusoid: the device's double pow / cos / sin are within a few ulp of 2^-53 at |angle| <= 1000: the interval of the float64 value
-+ 2^-40, through the kernel's two monotonic roundings (float, then bf16).
Bit for bit, no allowance: the V copy (random 16-bit patterns, NaNs included), untouched inputs, every canary (0x7FA5), patchify
(with its zeroed columns), unpatchify, modulation (one fp32 add, one rounding), the rows_equal_last flags.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

U = 2.0 ** -24
AMBIGUITY_CAP = 0.01
CANARY = 0x7FA5                                      # a NaN pattern no kernel produces
EPS_DERIVED = 4.0 * U                                # the docstring's derivation on a 1-ulp rsqrtf
RSQRT_MEASURED = 2.0 ** -25.25                       # 0.42 u: measured on an MI355X (docstring), case qk-rms-measure-d512; 0 in every other case
EPS = min(4.0 * RSQRT_MEASURED, 2.0 ** -16)          # 1.68 u
SILU_MEASURED = 2.0 ** -23.25                        # 1.19 u: measured on an MI355X over all 65 280 inputs
SILU_EPS = min(4.0 * SILU_MEASURED, 2.0 ** -12)      # 2^-21.25
LN, LN_PIPELINED, QKNORM = 1, 2, 3                   # plan[0]: RowPassKernel (csrc/kernels.h)
Q_SCALE = float(np.float32(np.float32(1.0 / math.sqrt(128.0)) * np.float32(1.4426950408889634)))   # softmax_scale * log2(e), as api.hip forms it
PERIOD = 61                                          # launcher-geometry cases: row r of a frame holds the content of row r % 61
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ bf16 <-> float, in bits
def bf2f(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_from_f32(f):
    """bf16_rne of an fp32 array (finite), as v_cvt_pk_bf16_f32 / c10::BFloat16 round."""
    b = np.ascontiguousarray(f, dtype=F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def bf16_from_f64(x):
    """bf16_rne of a float64 array in ONE rounding: to fp32 by round-to-odd (exact, or truncated with the last bit set), then RNE."""
    x = np.asarray(x, dtype=F64)
    f = x.astype(F32)
    b = f.view(np.uint32).copy()
    inexact = f.astype(F64) != x
    over = inexact & (np.abs(f.astype(F64)) > np.abs(x))
    b[over] -= 1                                     # back to the truncation (never crosses zero: |f| > |x| > 0)
    b[inexact] |= 1
    return bf16_from_f32(b.view(F32))


def rbf(f):
    return bf2f(bf16_from_f32(f))


def order(bits):
    """bf16 bits -> an integer that orders like the value (+0 and -0 both 0)."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def to_bf16(x):
    """float array -> bf16 bits of the nearest value (operands: the values are then whatever the bits say)."""
    return bf16_from_f32(np.asarray(x, dtype=F32))


@dataclasses.dataclass
class Expect:
    """What a launch may write: K candidate pairs per element.  g passes if g == lo[k] or g == hi[k] in bits, or lies strictly between."""
    lo: np.ndarray                                   # [K, ...] uint16
    hi: np.ndarray

    def outside(self, g):
        g = np.asarray(g, dtype=np.uint16)
        go = order(g)
        ok = np.zeros(g.shape, dtype=bool)
        for lo, hi in zip(self.lo, self.hi):
            a, b = order(lo), order(hi)
            ok |= (g == lo) | (g == hi) | ((np.minimum(a, b) < go) & (go < np.maximum(a, b)))
        return ~ok

    def ambiguous(self):
        a = order(self.lo[:1])                           # (+0 against -0 is no ambiguity)
        return ((order(self.lo) != a) | (order(self.hi) != a)).any(axis=0)

    def take(self, idx):
        return Expect(self.lo[:, idx], self.hi[:, idx])


def cand(x64, eps=None):
    """The two candidates bf16_rne(x (1 -+ eps)) of a float64 array; +0 and -0 where x == 0."""
    eps = EPS if eps is None else eps
    lo, hi = bf16_from_f64(x64 * (1.0 - eps)), bf16_from_f64(x64 * (1.0 + eps))
    z = x64 == 0
    lo[z], hi[z] = 0x0000, 0x8000
    return lo, hi


def needed_eps(g, x64, chain, top=2.0 ** -10):
    """Measurement: the smallest eps (0, then a grid of 2^(1/8) steps from u / 16) under which every element g equals chain(candidate)."""
    e = 0.0
    while e <= top:
        lo, hi = cand(x64, e)
        if not Expect(np.stack([chain(lo), chain(hi)]), np.stack([chain(lo), chain(hi)])).outside(g).any():
            return e
        e = U / 16 if e == 0.0 else e * 2.0 ** 0.125
    return float("inf")


# ------------------------------------------------------------------ geometry: canaries behind every row, behind the last row, around pages
def padded(rows, d, ld, tail_rows=2):
    """A [rows + tail_rows, ld] buffer of canaries; the window is [:rows, :d]."""
    return np.full((rows + tail_rows, ld), CANARY, dtype=np.uint16)


def window_intact(buf, rows, d):
    m = np.ones(buf.shape, dtype=bool)
    m[:rows, :d] = False
    return bool((buf[m] == CANARY).all())


# ------------------------------------------------------------------ LayerNorm
@dataclasses.dataclass(frozen=True)
class LnCase:
    name: str
    rows: int
    d: int
    affine: bool = False
    eps: float = 1e-6
    rpf: int = 13                  # rows per frame (modulation form)
    layout: str = "b1"             # modulation buffer: "b1" [F, 6 d] scale +d shift +0, "b2" scale +4 d shift +3 d, "head" [F, 2 d] scale +d shift +0
    xpad: int = 0                  # ldx = d + xpad
    ypad: int = 0
    pipeline: int = -1
    gpb: int = 0
    period: int = 0                # > 0: row r of a frame holds the content of row r % period (launcher-geometry cases)
    seed: int = 0

    @property
    def nit_raw(self): return (self.d // 8 + 63) // 64
    @property
    def nit(self): return self.nit_raw if self.nit_raw <= 4 else (self.nit_raw + 1) & ~1
    @property
    def frames(self): return 1 if self.affine else (self.rows + self.rpf - 1) // self.rpf
    @property
    def mod_stride(self): return 0 if self.affine else (2 if self.layout == "head" else 6) * self.d
    @property
    def mod_offsets(self): return {"b1": (self.d, 0), "b2": (4 * self.d, 3 * self.d), "head": (self.d, 0)}[self.layout]   # (scale, shift)
    @property
    def content_rows(self): return min(self.period, self.rpf) if self.period else self.rows

    def plan(self, resident, min_rows=16384):
        """mmpl_ln_plan restated: [kernel, NIT, FULL, resident, groups_per_block, grid x, grid y]."""
        pipelined = self.nit_raw >= 6 and (self.rows >= min_rows if self.pipeline < 0 else self.pipeline == 1)
        ngroups = (self.rows + 3) // 4
        if not pipelined:
            return [LN, self.nit, 0, 0, 1, ngroups, 1]
        full = int(self.d == 512 * self.nit and self.rows % 4 == 0 and (self.affine or self.rpf % 4 == 0))   # NIT as INSTANTIATED: no dead iteration
        gpb = self.gpb or (ngroups + resident - 1) // resident
        return [LN_PIPELINED, self.nit, full, resident, gpb, (ngroups + gpb - 1) // gpb, 1]


def ln_amp(d):
    """Largest amplitude A (<= 9) with 64 d (A + 1)^2 < 2^24: rows drawn in [-A, A] have |mean| < 1."""
    return max(1, min(9, int(math.isqrt(((1 << 18) - 1) // d)) - 1))


def ln_rows(rng, n, d, special=True):
    """n integer rows whose sums are multiples of d / 8.  With special (n >= 8): row 5 constant, row 6 of variance 2 / d, row 7 of mean 24."""
    A, q = ln_amp(d), d // 8
    x = rng.integers(-A, A + 1, size=(n, d)).astype(np.int64)
    for r in range(n):
        s = int(x[r].sum()) % q
        if s == 0:
            continue
        up = q - s <= s                                 # bump a few elements by one, in the cheaper direction
        k = q - s if up else s
        idx = rng.permutation(np.nonzero(x[r] < A if up else x[r] > -A)[0])[:k]
        assert len(idx) == k
        x[r, idx] += 1 if up else -1
    if special and n >= 8:
        x[5] = 3                                         # variance 0: the output is exactly shift / b
        x[6] = -2                                        # variance 2 / d: eps decides the result
        x[6, 1] += 1
        x[6, d - 3] -= 1
        x[7] = x[0] + 24                                 # mean 24 + m / 8
    return x


def ln_operands(c: LnCase):
    """-> dict: x int64 [content_rows, d]; scale / shift or w / b as bf16 bits ([frames, d] / [d])."""
    rng = np.random.default_rng(1000 + c.seed + 7 * c.d + c.rows)
    x = ln_rows(rng, c.content_rows, c.d)
    if c.affine:
        return dict(x=x, w=to_bf16(rng.normal(1.0, 0.5, c.d)), b=to_bf16(rng.normal(0.0, 1.0, c.d)))
    return dict(x=x, scale=to_bf16(rng.normal(0.0, 0.5, (c.frames, c.d))), shift=to_bf16(rng.normal(0.0, 1.0, (c.frames, c.d))))


def ln_row_frame(c: LnCase):
    """-> (content index, frame) of every row."""
    r = np.arange(c.rows)
    if c.affine:
        return (r % c.period if c.period else r), np.zeros(c.rows, dtype=np.int64)
    f = r // c.rpf
    return ((r - f * c.rpf) % c.period if c.period else r), f


def ln_exact(x, d):
    """The exactness conditions of a set of LayerNorm rows (module docstring)."""
    s = x.sum(axis=1)
    assert (s % (d // 8) == 0).all()
    dl8 = 8 * x - (8 * s // d)[:, None]                  # 8 (x - mean): integers
    assert (8 * s % d == 0).all() and np.abs(x).max() <= 256 and np.abs(dl8).max() < 2 ** 11
    assert ((dl8 * dl8).sum(axis=1) < 2 ** 24).all() and np.abs(x).sum(axis=1).max() < 2 ** 24


def ln_mod_chain(c, n_bits, sc, sh):
    """bf16 candidate of the norm output -> the kernel's element, bit for bit: bf16(bf16(n * bf16(1 + scale)) + shift)."""
    s1 = rbf(F32(1.0) + bf2f(sc))
    return bf16_from_f32(rbf(bf2f(n_bits) * s1) + bf2f(sh))


def ln_reference(c: LnCase, op, eps=None):
    """-> (Expect over [rows, d], float64 norm value x [rows, d] (the first rounded quantity; affine: y))."""
    x = op["x"].astype(F64)
    mean = x.mean(axis=1, keepdims=True)
    dl = x - mean
    r = 1.0 / np.sqrt((dl * dl).sum(axis=1, keepdims=True) / c.d + F64(F32(c.eps)))
    t = dl * r                                           # [content_rows, d]
    ci, fr = ln_row_frame(c)
    if c.affine:
        w, b = bf2f(op["w"]).astype(F64), bf2f(op["b"]).astype(F64)
        y = t * w + b
        D = (EPS if eps is None else eps) * np.abs(t * w) + U * np.abs(y)
        lo, hi = bf16_from_f64(y - D), bf16_from_f64(y + D)
        return Expect(lo[None][:, ci], hi[None][:, ci]), y[ci]
    lo, hi = cand(t, eps)
    lo, hi = lo[ci], hi[ci]
    sc, sh = op["scale"][fr], op["shift"][fr]
    a, b = ln_mod_chain(c, lo, sc, sh), ln_mod_chain(c, hi, sc, sh)
    return Expect(np.stack([a, b]), np.stack([a, b])), t[ci]


# value mutations of csrc/elementwise.hip (the issue's list), as switches of the fp32 emulations below
LN_MUTATIONS = ("staged_always", "var_counts_dead", "mean_by_padded", "scale_not_rounded", "staged_never_updated", "fma_split")


def _perm_sum(rng, a):
    """fp32 sum of each row of a in a random order of the adds."""
    return np.add.reduce(a[:, rng.permutation(a.shape[1])].astype(F32), axis=1, dtype=F32)


def _rsqrt32(v, ulp):
    r = (1.0 / np.sqrt(v.astype(F64))).astype(F32)
    return (r.view(np.int32) + ulp).view(F32)


def ln_emulate(c: LnCase, op, plan, ulp=0, mutation=None, seed=0):
    """Independent fp32 emulation of layernorm_kernel / layernorm_pipelined_kernel as the plan runs them (block ranges, staging), the
    adds of each sum in a random order, rsqrtf `ulp` off the correctly rounded value.  -> bf16 bits [rows, d]."""
    rng = np.random.default_rng(seed)
    ci, fr = ln_row_frame(c)
    x = op["x"][ci].astype(F32)
    rows, d = x.shape
    kernel, nit, full, _, gpb, _, _ = plan
    pad = 512 * nit - d
    mean = _perm_sum(rng, x) / F32(512 * nit if mutation == "mean_by_padded" else d)
    dl = x - mean[:, None]
    sq = _perm_sum(rng, dl * dl)
    if mutation == "var_counts_dead" and kernel == LN_PIPELINED and not full:
        sq = sq + F32(pad) * mean * mean
    rstd = _rsqrt32(sq / F32(d) + F32(c.eps), ulp)
    t = dl * rstd[:, None]
    if c.affine:
        w, b = bf2f(op["w"]), bf2f(op["b"])
        if mutation == "fma_split":
            return bf16_from_f32(t * w + b)
        return bf16_from_f32((t.astype(F64) * w.astype(F64) + b.astype(F64)).astype(F32))   # (53 bits hold the 32-bit product + b: one rounding but for ties of 2^-29)
    used = fr.copy()
    if kernel == LN_PIPELINED:
        r = np.arange(rows)
        g = r // 4
        gframe = (4 * g) // c.rpf
        first = (4 * (g // gpb) * gpb) // c.rpf          # the frame the block staged first
        if mutation == "staged_always":
            used = gframe
        elif mutation == "staged_never_updated":
            used = np.where(full | (fr == first), first, fr)
    sc, sh = bf2f(op["scale"][used]), bf2f(op["shift"][used])
    s1 = F32(1.0) + sc
    if mutation != "scale_not_rounded":
        s1 = rbf(s1)
    return bf16_from_f32(rbf(rbf(t) * s1) + sh)


def _ln_cases():
    out = []
    add = lambda name, rows, d, **kw: out.append(LnCase(f"ln-{name}", rows, d, **kw))
    for d in (512, 1024, 1536, 2048, 3072, 4096, 5120):              # every instantiation of layernorm_kernel
        for rows in (1, 3, 50):
            add(f"d{d}-r{rows}-mod", rows, d)
            add(f"d{d}-r{rows}-aff", rows, d, affine=True)
    add("d8-mod", 50, 8), add("d8-aff", 50, 8, affine=True)
    add("clip-d1280-r257-aff", 257, 1280, affine=True, eps=1e-5)     # a partial last iteration
    for d in (5112, 2560, 3584, 4608):                               # one dead lane; the dispatch rounds NIT up (5 -> 6, 7 -> 8, 9 -> 10)
        add(f"d{d}-mod", 50, d), add(f"d{d}-aff", 50, d, affine=True)
    for d in (3072, 4096, 5120):                                     # layernorm_pipelined_kernel, FULL: the frame changes inside a block's range
        for rpf in (8, 20):
            add(f"pipe-full-d{d}-rpf{rpf}", 40, d, rpf=rpf, pipeline=1, gpb=3)
        add(f"pipe-full-d{d}-aff", 40, d, affine=True, pipeline=1, gpb=3)
    for d, rows, rpf in ((2688, 49, 13), (3584, 50, 15), (4608, 51, 13), (3072, 50, 15), (4096, 51, 13), (5120, 49, 15)):
        add(f"pipe-d{d}-r{rows}-rpf{rpf}", rows, d, rpf=rpf, pipeline=1, gpb=3)     # not FULL: groups straddle frames, ragged last block
    for d in (2688, 3584, 4608):                                     # FULL but for the width: rows % 4 == 0, rpf % 4 == 0, yet a dead / partial iteration
        add(f"pipe-round-d{d}-rpf8", 40, d, rpf=8, pipeline=1, gpb=3)
        add(f"pipe-round-d{d}-aff", 40, d, affine=True, pipeline=1, gpb=3)
    add("pipe-d2688-aff", 50, 2688, affine=True, pipeline=1, gpb=3), add("pipe-d4608-aff", 49, 4608, affine=True, pipeline=1, gpb=3)
    add("d1536-b2", 50, 1536, layout="b2"), add("d1536-head", 50, 1536, layout="head")
    add("pipe-full-d3072-b2", 40, 3072, rpf=8, layout="b2", pipeline=1, gpb=3)
    add("pipe-d2688-head", 50, 2688, rpf=13, layout="head", pipeline=1, gpb=3)
    add("d1536-ld-mod", 50, 1536, xpad=8, ypad=24), add("d1536-ld-aff", 50, 1536, affine=True, xpad=8, ypad=24)
    add("pipe-full-d3072-ld", 40, 3072, rpf=8, xpad=8, ypad=24, pipeline=1, gpb=3)
    add("pipe-d4608-ld-aff", 50, 4608, affine=True, xpad=8, ypad=24, pipeline=1, gpb=3)
    return out


LN_CASES = _ln_cases()
LN_GEOMETRY_D = (2568, 3080, 4104)                   # launcher-geometry cases: the smallest d of NIT 6 / 8 / 10 (rows >= 16384 there)


def ln_geometry_case(d, resident, min_rows=16384):
    rows = max(4 * (2 * resident + 1) + 1, min_rows + 1)
    return LnCase(f"ln-own-geometry-d{d}", rows, d, rpf=(rows + 5) // 6, period=PERIOD)


# ------------------------------------------------------------------ QK RMSNorm + RoPE + page write
@dataclasses.dataclass(frozen=True)
class QkCase:
    name: str
    d: int
    n_frames: int = 1
    rpf: int = 15
    grid_w: int = 5
    rope: bool = True
    has_k: bool = True
    has_v: bool = False
    fused: bool = True             # q | k | v are the thirds of one [rows, 3 d] matrix (else separate matrices of ld = d + ldpad)
    ldpad: int = 0
    q_scale: float = 0.0
    gpb: int = 0
    frame_ids: tuple = (131, 977, 500, 128, 640, 257, 801, 333)
    fbase: object = None           # None: NULL frame_base_dev; an int: the device int
    table: str = "exact"
    slots: tuple = (5, 1, 3, 7, 0, 6, 2, 4)   # page of local frame i inside the page buffer: neither ascending nor adjacent
    eps: float = 1e-6
    period: int = 0
    amp: int = 9                   # |x| <= amp
    seed: int = 0

    @property
    def rows(self): return self.n_frames * self.rpf
    @property
    def nit_raw(self): return (self.d // 8 + 63) // 64
    @property
    def nit(self): return self.nit_raw if self.nit_raw <= 4 else (self.nit_raw + 1) & ~1
    @property
    def ld(self): return 3 * self.d if self.fused else self.d + self.ldpad
    @property
    def positions(self): return [min(max(f + (self.fbase or 0), 0), 1023) for f in self.frame_ids[:self.n_frames]]
    @property
    def content_rows(self): return min(self.period, self.rpf) if self.period else self.rpf

    def plan(self, resident):
        """mmpl_qknorm_plan restated."""
        ngroups = (self.rows + 3) // 4
        full = int(self.d == 512 * self.nit and self.rows % 4 == 0)      # NIT as INSTANTIATED: d = 2560, 3584, 4608 are never FULL
        gpb = self.gpb or (ngroups + resident - 1) // resident
        return [QKNORM, self.nit, full, resident, gpb, (ngroups + gpb - 1) // gpb, 1 + int(self.has_k) + int(self.has_v)]


def _hash(a, b):
    h = (np.asarray(a, dtype=np.uint64) * np.uint64(2654435761) + np.asarray(b, dtype=np.uint64) * np.uint64(40503) + np.uint64(12345))
    h ^= h >> np.uint64(13)
    h = h * np.uint64(1274126177) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(16))


def exact_tables():
    """fp32 [1024][64] x 2 of dyadic k / 16, |k| <= 16, by a hash of (position, pair): no two positions, and no two pairs, look alike."""
    pos, p = np.meshgrid(np.arange(1024), np.arange(64), indexing="ij")
    cs = ((_hash(pos, p) % np.uint64(33)).astype(np.int64) - 16) / 16.0
    sn = ((_hash(pos + 4096, p + 64) % np.uint64(33)).astype(np.int64) - 16) / 16.0
    return cs.astype(F32), sn.astype(F32)


def real_tables():
    """float32(cos), float32(sin) of the model's angles: pair p of a 128-wide head belongs to the frame axis (p < 22, 44 of the 128
    dimensions), the grid row (p < 43, 42) or the grid column (42), each axis with theta 10000 over its own dimensions."""
    cs, sn = np.zeros((1024, 64)), np.zeros((1024, 64))
    pos = np.arange(1024, dtype=F64)[:, None]
    for p0, n in ((0, 22), (22, 21), (43, 21)):
        ang = pos / np.power(10000.0, np.arange(n, dtype=F64) / n)[None, :]
        cs[:, p0:p0 + n], sn[:, p0:p0 + n] = np.cos(ang), np.sin(ang)
    return cs.astype(F32), sn.astype(F32)


def qk_operands(c: QkCase):
    """-> dict: q, k int64 [n_frames, content_rows, d] (|x| <= 9), v uint16 [rows, d] of random bits, wq / wk bf16 bits in +-[0.5, 2)."""
    rng = np.random.default_rng(2000 + c.seed + 3 * c.d + c.rows)
    gain = lambda: to_bf16(rng.uniform(0.5, 1.99, c.d) * rng.choice([-1.0, 1.0], c.d))
    op = dict(q=rng.integers(-c.amp, c.amp + 1, size=(c.n_frames, c.content_rows, c.d)), wq=gain())
    if c.has_k:
        op.update(k=rng.integers(-c.amp, c.amp + 1, size=(c.n_frames, c.content_rows, c.d)), wk=gain())
    if c.has_v:
        op["v"] = rng.integers(0, 1 << 16, size=(c.rows, c.d)).astype(np.uint16)
    return op


def qk_row_index(c: QkCase):
    """-> (frame, token, content index) of every row."""
    r = np.arange(c.rows)
    f = r // c.rpf
    tok = r - f * c.rpf
    return f, tok, (tok % c.period if c.period else tok)


def qk_factors(c: QkCase, tables, swap_axes=False, split=(22, 43), positions=None):
    """cos / sin of every (row, column pair of a row of d): fp32 [rows, d / 2]."""
    cs_t, sn_t = tables
    f, tok, _ = qk_row_index(c)
    ft = np.asarray(c.positions if positions is None else positions)[f]
    gy, gx = tok // c.grid_w, tok % c.grid_w
    if swap_axes:
        gy, gx = gx, gy
    p = np.arange(c.d // 2) % 64
    pos = np.where(p[None, :] < split[0], ft[:, None], np.where(p[None, :] < split[1], gy[:, None], gx[:, None]))
    return cs_t[pos, p[None, :]], sn_t[pos, p[None, :]]


def _qk_norm_candidates(c, x, w_bits, eps=None):
    """x int64 [F, R, d] -> (lo, hi) bf16 bits of bf16(bf16(v rr) * w) on either candidate of bf16(v rr), and the float64 v rr."""
    x = x.astype(F64)
    t = x / np.sqrt((x * x).sum(axis=-1, keepdims=True) / c.d + F64(F32(c.eps)))
    lo, hi = cand(t, eps)
    w = bf2f(w_bits)
    return bf16_from_f32(bf2f(lo) * w), bf16_from_f32(bf2f(hi) * w), t


def qk_reference(c: QkCase, op, which, tables=None, eps=None):
    """which 'q' | 'k' -> Expect over [rows, d]: what q holds afterwards / what the K pages hold, row by row."""
    lo, hi, _ = _qk_norm_candidates(c, op[which], op["w" + which], eps)
    f, _, ci = qk_row_index(c)
    lo, hi = lo[f, ci], hi[f, ci]                           # [rows, d]
    qs = F32(c.q_scale) if (which == "q" and c.q_scale != 0.0) else F32(1.0)
    if not c.rope:
        a, b = bf16_from_f32(bf2f(lo) * qs), bf16_from_f32(bf2f(hi) * qs)
        return Expect(np.stack([a, b]), np.stack([a, b]))
    cs, sn = qk_factors(c, tables)
    los, his = [], []
    for re_b in (lo[:, 0::2], hi[:, 0::2]):
        for im_b in (lo[:, 1::2], hi[:, 1::2]):
            re, im = bf2f(re_b), bf2f(im_b)
            if c.table == "exact":                          # exact in fp32 (qk_exact): any contraction gives this
                o = np.empty(lo.shape, dtype=F32)
                o[:, 0::2], o[:, 1::2] = re * cs - im * sn, re * sn + im * cs
                v = bf16_from_f32(o * qs)
                los.append(v), his.append(v)
            else:
                re, im, c64, s64 = re.astype(F64), im.astype(F64), cs.astype(F64), sn.astype(F64)
                o, D = np.empty(lo.shape), np.empty(lo.shape)
                o[:, 0::2], o[:, 1::2] = re * c64 - im * s64, re * s64 + im * c64
                D[:, 0::2] = 3 * U * (np.abs(re * c64) + np.abs(im * s64))
                D[:, 1::2] = 3 * U * (np.abs(re * s64) + np.abs(im * c64))
                D = D + np.abs(o) * 2.0 ** -50
                los.append(bf16_from_f32((o - D).astype(F32) * qs)), his.append(bf16_from_f32((o + D).astype(F32) * qs))
    return Expect(np.stack(los), np.stack(his))


def qk_exact(c: QkCase, op, tables):
    """The exactness conditions of a QK case: sum x^2 < 2^24, and (exact table) every rotation exact in fp32 on all candidate combinations."""
    for which in ("q", "k") if c.has_k else ("q",):
        x = op[which]
        assert np.abs(x).max() <= 256 and ((x * x).sum(axis=-1) < 2 ** 24).all()
        if not c.rope or c.table != "exact":
            continue
        lo, hi, _ = _qk_norm_candidates(c, x, op["w" + which])
        f, _, ci = qk_row_index(c)
        cs, sn = (a.astype(F64) for a in qk_factors(c, tables))
        for re_b in (lo[f, ci][:, 0::2], hi[f, ci][:, 0::2]):
            for im_b in (lo[f, ci][:, 1::2], hi[f, ci][:, 1::2]):
                re, im = bf2f(re_b).astype(F64), bf2f(im_b).astype(F64)
                for o in (re * cs - im * sn, re * sn + im * cs):
                    assert (o.astype(F32).astype(F64) == o).all()


QK_MUTATIONS = ("split_moved", "axes_swapped", "rc_not_advanced", "clamp_3fe", "fbase_ignored", "k_scaled", "k_page_prev_frame", "v_src_off_by_one")


def qk_emulate(c: QkCase, op, plan, tables, ulp=0, mutation=None, seed=0):
    """Independent fp32 emulation of qknorm_kernel.  -> dict: q bf16 bits [rows, d]; k, v: [n_frames, rpf, d] page contents (CANARY where
    a mutation leaves a page row unwritten)."""
    rng = np.random.default_rng(seed)
    f, tok, ci = qk_row_index(c)
    gpb = plan[4]
    positions = None
    if mutation == "fbase_ignored":
        positions = [min(max(x, 0), 1023) for x in c.frame_ids[:c.n_frames]]
    if mutation == "clamp_3fe":
        positions = [min(p, 0x3FE) for p in c.positions]
    out = {}
    for which in ("q", "k") if c.has_k else ("q",):
        x = op[which][f, ci].astype(F32)
        rr = _rsqrt32(_perm_sum(rng, x * x) / F32(c.d) + F32(c.eps), ulp)
        o = rbf(rbf(x * rr[:, None]) * bf2f(op["w" + which]))
        if c.rope:
            cs, sn = qk_factors(c, tables, swap_axes=mutation == "axes_swapped", split=(23, 44) if mutation == "split_moved" else (22, 43),
                                positions=positions)
            if mutation == "rc_not_advanced":               # every row of a block's range is rotated as the block's first group was
                r = np.arange(c.rows)
                src = np.minimum(4 * ((r // 4) // gpb) * gpb + r % 4, c.rows - 1)
                cs, sn = cs[src], sn[src]
            re, im = o[:, 0::2].astype(F64), o[:, 1::2].astype(F64)
            rot = np.empty(o.shape, dtype=F32)
            rot[:, 0::2], rot[:, 1::2] = (re * cs - im * sn).astype(F32), (re * sn + im * cs).astype(F32)   # (one rounding per sum: the fused end of what the kernel may do)
            o = rot
        qs = F32(c.q_scale) if c.q_scale != 0.0 and (which == "q" or mutation == "k_scaled") else F32(1.0)
        bits = bf16_from_f32(o * qs)
        if which == "q":
            out["q"] = bits
        else:
            pages = np.full((c.n_frames, c.rpf, c.d), CANARY, dtype=np.uint16)
            pf = np.maximum(f - (tok == 0), 0) if mutation == "k_page_prev_frame" else f      # (the frame of row - 1)
            pages[pf, tok] = bits
            out["k"] = pages
    if c.has_v:
        src = np.arange(c.rows)
        if mutation == "v_src_off_by_one":
            src = np.minimum(src + 1, c.rows - 1)
        out["v"] = op["v"][src].reshape(c.n_frames, c.rpf, c.d)
    return out


def _qk_cases():
    out = []
    add = lambda name, d, **kw: out.append(QkCase(f"qk-{name}", d, **kw))
    for d in (1536, 5120):                                          # the forward's form: v NULL, q_scale, q | k inside [rows, 3 d], a block's range crosses frames
        for nf in (2, 3, 4):                                        # 30 and 45 rows are not FULL (rows % 4); 60 rows are
            add(f"fwd-d{d}-f{nf}", d, n_frames=nf, q_scale=Q_SCALE, gpb=3)
    for d in (2560, 3584, 4608):                                    # rows % 4 == 0 at a width whose NIT is rounded up: a dead iteration, never FULL
        add(f"fwd-round-d{d}-f4", d, n_frames=4, q_scale=Q_SCALE, gpb=3)
    add("v-d256", 256, n_frames=2, has_v=True, gpb=3)               # the public form with V (grid.y = 3), rows % 4 != 0
    add("v-d640", 640, n_frames=3, rpf=7, grid_w=3, has_v=True, fused=False, ldpad=8, gpb=2)      # a partial last iteration
    add("v-d2560", 2560, n_frames=2, has_v=True, fused=False, gpb=3)                             # a dead iteration
    for d, rpf, qs, pad in ((4096, 512, 0.0, 0), (4096, 512, Q_SCALE, 8), (1536, 257, 0.0, 8), (1536, 257, Q_SCALE, 0), (5120, 257, 0.0, 0),
                            (5120, 257, Q_SCALE, 8)):               # rope 0, k NULL: T5 (FULL), i2v / cross q-norm (257 rows)
        add(f"rms-d{d}-r{rpf}-{'qs' if qs else 'plain'}-ld{pad}", d, rpf=rpf, rope=False, has_k=False, fused=False, ldpad=pad, q_scale=qs)
    # the case EPS is measured on: 4096 rows of ~100 distinct magnitudes each, every row with another sum of squares (<= 512 * 10^4 < 2^24)
    # -- some 4e5 distinct values of v * rr, of which dozens lie within a few u of a bf16 tie; the other cases hold too few to tell
    add("rms-measure-d512", 512, rpf=4096, rope=False, has_k=False, fused=False, amp=100)
    add("pos-0-1023", 256, n_frames=2, frame_ids=(0, 1023), gpb=3)
    add("pos-base-up", 256, n_frames=2, frame_ids=(5, 1000), fbase=100, gpb=3)          # 1100 -> 1023
    add("pos-base-down", 256, n_frames=2, frame_ids=(5, 1000), fbase=-50, gpb=3)        # -45 -> 0
    add("pos-base-zero", 256, n_frames=2, frame_ids=(130, 1023), fbase=0, gpb=3)
    add("real-fwd-d1536-f4", 1536, n_frames=4, q_scale=Q_SCALE, gpb=3, table="real")
    add("real-v-d640", 640, n_frames=3, rpf=7, grid_w=3, has_v=True, fused=False, ldpad=8, gpb=2, table="real")
    add("real-fwd-d5120-f2", 5120, n_frames=2, q_scale=Q_SCALE, gpb=3, table="real")
    return out


QK_CASES = _qk_cases()
QK_GEOMETRY_D = (512, 1024, 1536, 2048, 3072, 4096, 5120)          # launcher-geometry cases: every FULL NIT


def qk_geometry_case(d, resident):
    return QkCase(f"qk-own-geometry-d{d}", d, n_frames=4, rpf=2 * resident + 1, grid_w=max(5, (2 * resident + 1) // 1000 + 1), fused=False,
                  q_scale=Q_SCALE, period=PERIOD, slots=(2, 0, 3, 1))


# ------------------------------------------------------------------ small kernels
def modulation_ref(mod, stride, e, e_stride, bcast, n_layers, n_frames, nmod, d, ignore_bcast=False):
    """bf16 bits in flat arrays -> emod bits [n_layers, n_frames, nmod * d]: one fp32 add, one rounding."""
    within = np.arange(nmod * d)
    ew = within % d if (bcast and not ignore_bcast) else within
    out = np.empty((n_layers, n_frames, nmod * d), dtype=np.uint16)
    for l in range(n_layers):
        for f in range(n_frames):
            out[l, f] = bf16_from_f32(bf2f(mod[l * stride + within]) + bf2f(e[f * e_stride + ew]))
    return out


def patchify_ref(x, lda, swap=False):
    """x bits [F, C, h, w] -> a [F * h/2 * w/2, lda]: column c * 4 + ph * 2 + pw, zero from column 4 C."""
    F, C, h, w = x.shape
    p = x.reshape(F, C, h // 2, 2, w // 2, 2)               # f c gy ph gx pw
    p = p.transpose(0, 2, 4, 1, 5, 3) if swap else p.transpose(0, 2, 4, 1, 3, 5)
    a = np.zeros((F * (h // 2) * (w // 2), lda), dtype=np.uint16)
    a[:, :4 * C] = p.reshape(-1, 4 * C)
    return a


def unpatchify_ref(y, F, C, h, w):
    """y bits [F * h/2 * w/2, ldy], column (ph * 2 + pw) * C + c -> out [F, C, h, w]."""
    p = y[:, :4 * C].reshape(F, h // 2, w // 2, 2, 2, C)     # f gy gx ph pw c
    return p.transpose(0, 5, 1, 3, 2, 4).reshape(F, C, h, w)


def sinusoid_ref(t, freq_dim):
    """t float32 [F] -> Expect over [F, freq_dim]."""
    half = freq_dim // 2
    ang = t.astype(F64)[:, None] * np.power(10000.0, -np.arange(half, dtype=F64) / half)[None, :]
    v = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)
    lo, hi = bf16_from_f32((v - 2.0 ** -40).astype(F32)), bf16_from_f32((v + 2.0 ** -40).astype(F32))
    return Expect(lo[None], hi[None])


def silu_inputs():
    b = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7F80) != 0x7F80]                         # every finite bf16 value: 65 280


def silu_ref(bits, eps=None):
    eps = SILU_EPS if eps is None else eps
    x = bf2f(bits).astype(F64)
    with np.errstate(over="ignore"):
        y = x / (1.0 + np.exp(-x))
    D = eps * np.abs(y) + 2.0 ** -126 * np.maximum(1.0, np.abs(x))
    return Expect(bf16_from_f64(y - D)[None], bf16_from_f64(y + D)[None]), y


def rows_equal_last_case(rng, d=4096, ld=4104):
    """-> (buffer bits [rows, ld], flags): rows equal to the last one, rows one bit off in chunk 0 / 64 / the last, junk in the gap."""
    last = rng.integers(0, 1 << 16, d).astype(np.uint16)
    spec = [None, (0, 3, 0), None, (64, 5, 9), (d // 8 - 1, 7, 15), None, (64, 0, 31 - 16), (0, 6, 1), None]   # (chunk, element, bit) | equal
    buf = rng.integers(0, 1 << 16, (len(spec), ld)).astype(np.uint16)
    flags = []
    for r, s in enumerate(spec):
        buf[r, :d] = last
        if s:
            buf[r, 8 * s[0] + s[1]] ^= np.uint16(1 << s[2])
        flags.append(0 if s else 1)
    return buf, np.asarray(flags, dtype=np.int32), spec


def rows_equal_last_ref(buf, d, words=4):
    """flags by comparing `words` of the four 32-bit words of every 16-byte chunk (4: the kernel; 3: the mutation)."""
    x = buf[:, :d].reshape(buf.shape[0], d // 8, 4, 2)[:, :, :words]
    return (x == x[-1:]).all(axis=(1, 2, 3)).astype(np.int32)
