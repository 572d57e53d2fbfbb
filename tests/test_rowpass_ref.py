"""CPU proofs for tests/rowpass_ref.py: for every case of its tables the exactness conditions its docstring states, the ambiguity cap
from the reference alone, that an independent fp32 emulation (sums in a random order, rsqrtf one ulp either way) passes the
criterion (with rsqrtf a whole ulp off: at the derived 4 u, which the measured allowance undercuts), and that every value mutation of the emulation fails it somewhere."""
import numpy as np
import pytest

from tests import rowpass_ref as R

RESIDENT = 4                                         # a stand-in: the device's own count enters only the launcher-geometry cases
LN_ALL = R.LN_CASES + [R.ln_geometry_case(d, RESIDENT, min_rows=0) for d in R.LN_GEOMETRY_D]
QK_ALL = R.QK_CASES + [R.qk_geometry_case(d, RESIDENT) for d in R.QK_GEOMETRY_D]
TABLES = {"exact": R.exact_tables(), "real": R.real_tables()}


def test_bf16_rounding_helpers():
    f = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-40, 0.0], dtype=np.float32)
    assert R.bf16_from_f32(f).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x7F62, 0x0001, 0]      # ties to even
    # a float64 just above a bf16 tie that fp32 rounding would first pull onto the tie: one rounding, not two
    x = np.array([1.00390625 + 2.0 ** -30, 1.00390625 - 2.0 ** -30, -(1.01171875 - 2.0 ** -40)])
    assert R.bf16_from_f64(x).tolist() == [0x3F81, 0x3F80, 0xBF81]
    assert R.order(np.array([0x8000, 0, 0x3F80, 0xBF80], dtype=np.uint16)).tolist() == [0, 0, 0x3F80, -0x3F80]
    e = R.Expect(np.array([[0x3F80], [0x4000]], dtype=np.uint16), np.array([[0x3F82], [0x4000]], dtype=np.uint16))
    assert R.Expect.outside(e, np.array([0x3F81], dtype=np.uint16)).tolist() == [False]
    assert R.Expect.outside(e, np.array([0x3F83], dtype=np.uint16)).tolist() == [True]
    assert R.Expect.outside(e, np.array([0x4000], dtype=np.uint16)).tolist() == [False]
    assert R.Expect.outside(e, np.array([R.CANARY], dtype=np.uint16)).tolist() == [True]


def test_tables():
    cs, sn = TABLES["exact"]
    for t in (cs, sn):
        assert t.shape == (1024, 64) and (np.abs(t) <= 1).all() and (t * 16 == np.round(t * 16)).all()
    both = np.concatenate([cs, sn], axis=1)
    assert len(np.unique(both, axis=0)) == 1024                      # no two positions alike
    assert len(np.unique(both.reshape(1024, 2, 64).transpose(2, 0, 1).reshape(64, -1), axis=0)) == 64     # no two pairs alike
    rc, rs = TABLES["real"]
    assert np.allclose(rc * rc + rs * rs, 1.0, atol=1e-6) and rc[0].min() == 1.0 and rs[1, 0] == np.float32(np.sin(1.0))
    assert rc[3, 22] == np.float32(np.cos(3.0)) and rc[3, 43] == np.float32(np.cos(3.0)) and rc[5, 21] == np.float32(np.cos(5.0 / 10000 ** (21 / 22)))


@pytest.mark.parametrize("c", LN_ALL, ids=[c.name for c in LN_ALL])
def test_layernorm_case(c):
    op = R.ln_operands(c)
    R.ln_exact(op["x"], c.d)
    assert 64 * c.d * (R.ln_amp(c.d) + 1) ** 2 < 2 ** 24
    exp, _ = R.ln_reference(c, op)
    assert exp.ambiguous().mean() <= R.AMBIGUITY_CAP
    plan = c.plan(RESIDENT, min_rows=0 if c.period else 16384)
    assert plan[0] == (R.LN_PIPELINED if (c.pipeline == 1 or c.period) else R.LN)
    wide, _ = R.ln_reference(c, op, eps=R.EPS_DERIVED)
    for ulp in (-1, 0, 1):                                           # (rowpass_ref's docstring, "EPS": a whole ulp of rsqrt exceeds what was measured)
        g = R.ln_emulate(c, op, plan, ulp=ulp, seed=ulp + 5)
        e = exp if ulp == 0 else wide
        assert not e.outside(g).any(), (ulp, int(e.outside(g).sum()))
    if c.content_rows >= 8 and not c.affine:                                 # the constant row returns shift, bit for bit, in every candidate
        ci, fr = R.ln_row_frame(c)
        assert (exp.lo[:, 5] == exp.hi[:, 5]).all() and (R.order(exp.lo[0, 5]) == R.order(op["shift"][fr[5]])).all()


def test_layernorm_mutations_fail():
    failing = {m: [] for m in R.LN_MUTATIONS}
    for c in LN_ALL:
        op = R.ln_operands(c)
        exp, _ = R.ln_reference(c, op)
        plan = c.plan(RESIDENT, min_rows=0 if c.period else 16384)
        for m in R.LN_MUTATIONS:
            if exp.outside(R.ln_emulate(c, op, plan, mutation=m)).any():
                failing[m].append(c.name)
    print({m: len(v) for m, v in failing.items()})
    for m in R.LN_MUTATIONS:
        assert failing[m], m


@pytest.mark.parametrize("c", QK_ALL, ids=[c.name for c in QK_ALL])
def test_qknorm_case(c):
    op = R.qk_operands(c)
    tables = TABLES[c.table]
    R.qk_exact(c, op, tables)
    assert c.n_frames <= 8 and c.grid_w <= 1024 and (c.rpf - 1) // c.grid_w <= 1023
    if not c.period and c.rope:
        f, tok, _ = R.qk_row_index(c)
        assert min(c.frame_ids[:c.n_frames]) >= 0 and (tok // c.grid_w).max() < 128 and ((tok // c.grid_w) != (tok % c.grid_w)).mean() > 0.6
    plan = c.plan(RESIDENT)
    exps = {w: R.qk_reference(c, op, w, tables) for w in (("q", "k") if c.has_k else ("q",))}
    for w, e in exps.items():
        assert e.ambiguous().mean() <= R.AMBIGUITY_CAP, (w, e.ambiguous().mean())
    wide = {w: R.qk_reference(c, op, w, tables, eps=R.EPS_DERIVED) for w in exps}
    for ulp in (-1, 0, 1):                                           # (rowpass_ref's docstring, "EPS": a whole ulp of rsqrt exceeds what was measured)
        g = R.qk_emulate(c, op, plan, tables, ulp=ulp, seed=ulp + 9)
        exps = exps if ulp == 0 else wide
        assert not exps["q"].outside(g["q"]).any()
        if c.has_k:
            assert not exps["k"].outside(g["k"].reshape(c.rows, c.d)).any()


def test_qknorm_mutations_fail():
    failing = {m: [] for m in R.QK_MUTATIONS}
    for c in QK_ALL:
        op = R.qk_operands(c)
        tables = TABLES[c.table]
        plan = c.plan(RESIDENT)
        exps = {w: R.qk_reference(c, op, w, tables) for w in (("q", "k") if c.has_k else ("q",))}
        for m in R.QK_MUTATIONS:
            g = R.qk_emulate(c, op, plan, tables, mutation=m)
            bad = exps["q"].outside(g["q"]).any() or (c.has_k and exps["k"].outside(g["k"].reshape(c.rows, c.d)).any())
            if c.has_v:
                bad = bad or not np.array_equal(g["v"].reshape(c.rows, c.d), op["v"])
            if bad:
                failing[m].append(c.name)
    print({m: len(v) for m, v in failing.items()})
    for m in R.QK_MUTATIONS:
        assert failing[m], m


def test_small_kernel_references():
    rng = np.random.default_rng(3)
    x = np.arange(3 * 16 * 6 * 10, dtype=np.uint16).reshape(3, 16, 6, 10)
    a = R.patchify_ref(x, 64)
    assert a.shape == (3 * 3 * 5, 64) and a[7, 4 * 5 + 2 * 1 + 0] == x[0, 5, 2 * 1 + 1, 2 * 2 + 0]      # token 7 = (gy 1, gx 2)
    assert not np.array_equal(a, R.patchify_ref(x, 64, swap=True))
    y = rng.permutation(45 * 64).astype(np.uint16).reshape(45, 64)
    o = R.unpatchify_ref(y, 3, 16, 6, 10)
    assert o[1, 9, 3, 4] == y[(1 * 3 + 1) * 5 + 2, (1 * 2 + 0) * 16 + 9]
    d = 8
    mod, e = R.to_bf16(rng.normal(size=2 * d)), R.to_bf16(rng.normal(size=3 * d))
    head = R.modulation_ref(mod, 0, e, d, 1, 1, 3, 2, d)
    assert head[0, 2, d + 1] == R.bf16_from_f32(R.bf2f(mod[d + 1:d + 2]) + R.bf2f(e[2 * d + 1:2 * d + 2]))[0]
    assert not np.array_equal(head, R.modulation_ref(mod, 0, np.concatenate([e, e]), d, 1, 1, 3, 2, d, ignore_bcast=True))
    buf, flags, _ = R.rows_equal_last_case(rng)
    assert R.rows_equal_last_ref(buf, 4096).tolist() == flags.tolist() and flags[-1] == 1 and flags.sum() == 4
    assert R.rows_equal_last_ref(buf, 4096, words=3).tolist() != flags.tolist()
    exp, yv = R.silu_ref(R.silu_inputs())
    assert len(yv) == 65280 and not exp.outside(R.bf16_from_f64(yv)).any()
    s = R.sinusoid_ref(np.array([0.0, 0.5, 999.0, 1000.0], dtype=np.float32), 256)
    assert s.lo.shape == (1, 4, 256) and (s.lo[0, 0, :128] == 0x3F80).all() and s.ambiguous()[1:].mean() < 0.01   # (sin 0 = 0 +- 2^-40: row 0's sines lie strictly inside)
