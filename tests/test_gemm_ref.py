"""The conditions the bit-exact GEMM tests (tests/test_gemm_forms_gpu.py) rest on, proven on the CPU from the inputs alone:
tests/gemm_ref.py's cases keep the accumulator and every fp32-held intermediate exact, its reference agrees with a per-element
evaluation in exact rational arithmetic, its launch-plan restatement gives what the case table says, and its canary / page geometry
is consistent."""
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import gemm_ref as R

IDS = [c.name for c in R.CASES]


def test_case_table_covers_the_forms():
    assert len(set(IDS)) == len(IDS)
    by = lambda pred: [c for c in R.CASES if pred(c)]
    for kernel in (R.SMALL, R.V2, R.V6, R.V8):
        assert by(lambda c: c.kernel == kernel and c.LDC > c.N and c.batch == 1), kernel          # ldc > N at least once per kernel
        assert by(lambda c: c.kernel == kernel and c.inplace and c.epi == R.EPI_GATE_RES), kernel
    for tail in (R.SPLITK, R.TAIL128_8, R.TAIL128_4):
        assert by(lambda c: c.tail == tail and c.inplace), tail
    for tail in (R.SPLITK, R.TAIL128_4):
        assert by(lambda c: c.tail == tail and c.epi == R.EPI_VPAGES), tail
    assert by(lambda c: c.kernel == R.V6 and not c.staged and c.epi == R.EPI_F32_SCALE)
    assert {c.rpf for c in R.CASES if c.staged and c.epi == R.EPI_GATE_RES and c.gate_stride} == {128, 130, 200}
    assert all(c.inplace for c in R.CASES if c.epi in (R.EPI_GATE_RES, R.EPI_RES))                  # the form production launches


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_plan_table_matches_tile_arithmetic(c):
    """The path each case names (kernel, tail, epilogue form, parts, main launch) is what the tile arithmetic gives at 32 CUs per XCD."""
    kernel, tail, staged, main, tail_blocks, s = R.plan_restated(c, 32)
    assert (kernel, tail, staged, s) == (c.kernel, c.tail, c.staged, c.splitk_s)
    tiles = -(-c.M // 256) * -(-c.N // 256)
    if c.kernel in (R.V6, R.V8):
        assert {"none": main == 0, "percu": main == 256 and tiles > 256, "tiles": main == tiles and tail == 0}[c.main]
    assert (tail_blocks > 0) == (tail != 0)
    if tail == R.SPLITK:
        assert tail_blocks % (8 * s) == 0 and c.K // 64 >= s


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_ranges_keep_every_intermediate_exact(c):
    """From the input ranges alone: K max|a| max|w| < 2^24, and every value the kernel holds in fp32 is a multiple of a quantum q
    bounded by B with B / q < 2^24."""
    assert c.K * R.A_MAX * R.W_MAX < 2 ** 24
    for what, q, bound in R.exactness_bounds(c):
        assert bound / q < 2 ** 24, what
    a, w = R.operands(c.input_key)
    assert float(a.float().abs().max()) <= R.A_MAX and float(w.float().abs().max()) <= R.W_MAX
    assert torch.equal(a.float(), a.float().round()) and torch.equal(w.float(), w.float().round())
    bias, gate, res = R.epilogue_inputs(c)
    for t, q, mx in ((bias, 0.5, R.BIAS_MAX), (gate, 0.125, R.GATE_MAX), (res, 0.25, R.RES_MAX)):
        if t is not None:
            v = t.double() / q                                         # the bf16 tensor holds exactly k * q, |k * q| <= max
            assert torch.equal(v, v.round()) and float(t.float().abs().max()) <= mx


_acc = {}


def _accumulator(c):
    """float64 accumulator of a case's operands, kept for the next epilogue of the same shape (the cases of a shape are adjacent)."""
    if c.input_key not in _acc:
        _acc.clear()
        _acc[c.input_key] = R.accumulate(c, *R.operands(c.input_key))
    return _acc[c.input_key]


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_reference_leaves_no_ambiguous_element(c):
    """The float64 chain on the real inputs of every case: the accumulator is an integer below 2^24 and every fp32-held intermediate
    survives the round trip through float32 (counted by the reference itself)."""
    bias, gate, res = R.epilogue_inputs(c)
    acc = _accumulator(c)
    assert float(acc.abs().max()) < 2 ** 24 and torch.equal(acc, acc.round())
    e = R.expected(c, acc, bias, gate, res)
    assert e.ambiguous == 0
    assert int(e.c_written.sum()) == c.batch * c.M * c.n_c
    assert not bool((R.bits(e.c_buf)[e.c_written] == R.bits(R.canary(1, e.c_buf.dtype))[0]).any())      # the canary is no output value


def _rne_bf16(x: Fraction) -> Fraction:
    """Round-to-nearest-even of an exact rational to bf16 (8 significant bits; the test values are far from the exponent limits)."""
    if x == 0:
        return x
    e = 0
    ax = abs(x)
    while ax >= 256:
        ax /= 2; e += 1
    while ax < 128:
        ax *= 2; e -= 1
    n, r = divmod(ax, 1)
    n = int(n)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return (1 if x > 0 else -1) * Fraction(n) * Fraction(2) ** e


def _rne_f32(x: Fraction) -> Fraction:
    return Fraction(struct.unpack("f", struct.pack("f", float(x)))[0])      # float(Fraction) is correctly rounded to double; the
    # values here have at most 48 significant bits, so that step is exact and the pack is the single RNE to fp32


@pytest.mark.parametrize("epi", [0, 3, 4, 5, 6])
def test_reference_against_exact_rational_evaluation(epi):
    """A tiny case of every exact epilogue, element by element in Fractions: accumulate, add the bias, round to bf16 by the rule
    itself (not by torch), gate by frame = m / rows_per_frame, add the residual, round; pages and untouched columns included."""
    c = R.Case(f"tiny-epi{epi}", 11, 12, 64, epi, R.SMALL, rpf=4, inplace=epi in (3, 4), alpha=R.ALPHA_T5, v_col0=8 if epi == 6 else 0,
               gate_stride=36 if epi == 3 else 0, ldc_pad=4)
    a, w = R.operands(c.input_key)
    bias, gate, res = R.epilogue_inputs(c)
    e = R.expected(c, R.accumulate(c, a, w), bias, gate, res)
    assert e.ambiguous == 0
    fr = lambda t, *i: Fraction(float(t[i]))
    want_c = np.zeros((c.M, c.N), dtype=object)
    for m in range(c.M):
        for n in range(c.N):
            acc = sum(Fraction(int(a[m * c.K + k])) * Fraction(int(w[n * c.K + k])) for k in range(c.K))
            if epi == 5:
                want_c[m, n] = _rne_f32(acc * Fraction(float(np.float32(c.alpha))))
                continue
            v = _rne_bf16(acc + fr(bias, n))
            if epi == 3:
                v = _rne_bf16(v * fr(gate, c.N + (m // c.rpf) * c.GATE_STRIDE + n))
            if epi in (3, 4):
                v = _rne_bf16(fr(res, m, n) + v)
            want_c[m, n] = v
    got = R.c_view(c, e.c_buf)[0]
    for m in range(c.M):
        for n in range(c.n_c):
            assert Fraction(float(got[m, n])) == want_c[m, n], (m, n)
    buf2d = R.bits(e.c_buf).view(c.M + 3, c.LDC)
    canary = R.bits(R.canary(1, e.c_buf.dtype))[0]
    assert bool((buf2d[:, c.n_c:] == canary).all()) and bool((buf2d[c.M:] == canary).all())
    if epi == 6:
        off, rows, total = R.page_layout(c)
        assert rows == [4, 4, 3] and e.v_buf.numel() == total
        for f, page in enumerate(R.page_views(c, e.v_buf)):
            for r in range(rows[f]):
                for n in range(c.N - c.v_col0):
                    assert Fraction(float(page[r, n])) == want_c[f * c.rpf + r, c.v_col0 + n], (f, r, n)
        assert int(e.v_written.sum()) == c.M * (c.N - c.v_col0)
        assert bool((R.bits(e.v_buf)[~e.v_written] == canary).all())


@pytest.mark.parametrize("epi", [R.EPI_GELU, R.EPI_SILU])
def test_activation_reference_is_accurate_where_the_cases_evaluate_it(epi):
    """The reference's own error: the fp32 restatement of GELU / SiLU, rounded to bf16, is within 1 bf16 ulp of the same function in
    float64 at EVERY pre-activation a case can hand it -- the bf16 values among the multiples of 1/2 up to the largest |acc + bias| --
    wherever that value is at least 2^-120 in magnitude, and within 2^-120 of it below that -- so the 2-ulp criterion of the GPU test measures the kernel.  (The far negative tail is where this matters: there the value is
    x * 1e-7 and smaller, and a form that cancels, 0.5 x (1 + tanh u), returns -0.0 or a few quanta of 2^-24.)"""
    from tests.util import bf16_ulp_frac
    bound = max(B for c in R.CASES if c.epi == epi for _, _, B in R.exactness_bounds(c)[:2])
    x = (torch.arange(-2 * int(bound) - 2, 2 * int(bound) + 3, dtype=torch.float64) / 2).to(R.BF).unique()
    top = float(torch.tensor(bound).to(R.BF))                    # the pre-activation reaches the activation rounded to bf16
    assert x.numel() > 1000 and float(x.min()) == -top and float(x.max()) == top
    got = R.activation(epi, x.float())
    want = R.activation(epi, x.double())
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and bool(torch.isfinite(got).all())
    # ... down to the last binades of fp32: exp(-x) overflows fp32 from x = -88.7 on (SiLU; GELU's exp(-2u) from x = -10.3 on), and
    # every fp32 evaluation returns -0.0 for a value that is below 2^-120 in magnitude; there the claim is that absolute distance
    tiny = 2.0 ** -120
    ok = want.abs() >= tiny
    assert float(x[ok].min()) <= (-87 if epi == R.EPI_SILU else -9.5)            # the relative claim reaches that far
    assert bf16_ulp_frac(got[ok].to(R.BF), want[ok].to(R.BF), 1) == 0.0
    assert float((got[~ok].double() - want[~ok]).abs().max()) < tiny
    # and it is the function torch names, where that is evaluated without cancellation
    import torch.nn.functional as F
    pos = x[x >= -2].double()
    named = F.gelu(pos, approximate="tanh") if epi == R.EPI_GELU else F.silu(pos)
    assert float(((R.activation(epi, pos) - named).abs() / named.abs().clamp_min(1e-30)).max()) < 1e-12


VP = [c for c in R.CASES if c.epi == R.EPI_VPAGES]


@pytest.mark.parametrize("c", VP, ids=[c.name for c in VP])
def test_page_geometry(c):
    """Pages hold every row of their frame, do not overlap, keep SLACK_ROWS canary rows on both sides, sit at shuffled addresses, and
    only the deliberately offset page is not 16-byte aligned; the arguments pass mmpl_gemm_ex's own checks."""
    off, rows, total = R.page_layout(c)
    assert 1 <= c.n_frames <= 8 and c.n_frames * c.rpf >= c.M and sum(rows) == c.M and min(rows) >= 1
    assert c.v_col0 % 4 == 0 and 0 < c.v_col0 < c.N and c.V_LD >= c.N - c.v_col0 and c.V_LD % 4 == 0
    spans = sorted((off[f], off[f] + (rows[f] - 1) * c.V_LD + (c.N - c.v_col0)) for f in range(c.n_frames))
    assert spans[0][0] >= R.SLACK_ROWS * c.V_LD and total - spans[-1][1] >= R.SLACK_ROWS * c.V_LD
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert start - end >= R.SLACK_ROWS * c.V_LD
    assert off != sorted(off)
    assert [o % 8 for o in off] == [c.v_page_off if f == 1 else 0 for f in range(c.n_frames)]
    written = torch.zeros(total, dtype=torch.int32)
    for v in R.page_views(c, written):
        v += 1
    assert int(written.max()) == 1 and int(written.sum()) == c.M * (c.N - c.v_col0)


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_c_geometry(c):
    """C's window lies inside its buffer with three canary rows behind it, batched windows do not overlap, and the strides pass
    mmpl_gemm_ex's checks."""
    n = R.c_elems(c)
    hits = torch.zeros(n, dtype=torch.int32)
    R.c_view(c, hits).add_(1)
    assert int(hits.max()) == 1 and int(hits.sum()) == c.batch * c.M * c.n_c
    last = int(hits.nonzero().max())
    assert n - 1 - last >= 2 * c.LDC
    assert c.LDC % 4 == 0 and c.LDA % 8 == 0 and c.LDW % 8 == 0 and c.LDA >= c.K and c.LDW >= c.K and c.K % 64 == 0 and c.N % 4 == 0
    assert c.c_off % 4 == 0 and c.sA % 8 == 0 and c.sW % 8 == 0 and c.sC % 4 == 0
    assert c.batch == 1 or c.kernel == R.SMALL
