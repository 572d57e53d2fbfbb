"""CPU proofs for tests/glue_ref.py: for every case of its tables the ambiguity cap from the reference alone, that no bit-exact case
has a subnormal intermediate (the project states no flush mode), that a correctly rounded fp32 emulation of each kernel passes its
criterion (the transcendental one ulp either way where an allowance covers it), and that every value mutation of the emulation is
rejected -- except the two that change no value at all (0.5 x of a bf16 x is exact), which are shown to be identities."""
import numpy as np
import pytest
import torch

from tests import glue_ref as G
from tests.test_scheduler_host import emulate_kernel

SM = {c.name: c for c in G.SOFTMAX_CASES}


def _step_scalars():
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    s = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    s.set_timesteps(50, shift=5.0)
    return [s.step_scalars(5.0) for _ in range(50)]


def test_copies_and_their_mutation():
    for c in G.GATHER_CASES:
        op = G.gather_operands(c)
        ids = op["ids"].tolist()
        assert 0 in ids and c.vocab - 1 in ids and len(set(ids)) < len(ids) and min(ids) >= 0 and max(ids) < c.vocab
        assert G.gather_ref(op).shape == (c.L, c.dim) and c.dim % 8 == 0
        assert np.isnan(G.bf2f(op["emb"])).any()                           # NaN patterns travel too
    for c in G.TRANSPOSE_CASES:
        op = G.transpose_operands(c)
        want = G.transpose_ref(c, op)
        assert c.ld >= c.off + c.H * c.c and want.shape == (c.H, c.c, c.L)
        assert want[c.H - 1, 3, 5] == op["v"][5, c.off + (c.H - 1) * c.c + 3]
        assert not np.array_equal(want, G.transpose_ref(c, op, head_offset=False))
    assert any(c.L % 32 and c.c % 32 for c in G.TRANSPOSE_CASES) and any(c.off for c in G.TRANSPOSE_CASES)
    for kind in G.ZERO_PAD_MASKS:
        op = G.zero_pad_operands(kind)
        want = G.zero_pad_ref(op)
        keep = op["mask"] != 0
        assert (want[~keep] == 0).all() and np.array_equal(want[keep], op["out"][keep])
        assert {"prefix": keep.sum() == 37, "holes": 0 < keep.sum() < 64 and not keep[1], "ones": keep.all(), "zeros": not keep.any()}[kind]


@pytest.mark.parametrize("n", G.ADD_SIZES)
def test_add(n):
    a, b = G.add_operands(n)
    s = G.bf2f(a) + G.bf2f(b)
    assert np.isfinite(s).all() and G.no_subnormal(G.bf2f(a), G.bf2f(b), s)
    want = G.add_ref(a, b)
    assert (s[::7] == 0).all() and (want != a).mean() > 0.5 or n == 1
    assert not np.array_equal(want, G.add_ref(a, b, "stride_start"))
    assert G.ADD_SIZES[-1] > 4096 * 256 and G.ADD_SIZES[-1] % 256


@pytest.mark.parametrize("n", G.GATED_SIZES)
def test_gated(n):
    f, g = G.gated_operands(n)
    exp, z = G.gated_reference(f, g)
    assert exp.ambiguous().mean() <= G.AMBIGUITY_CAP
    for ulp in (-1, 0, 1):
        assert not exp.outside(G.gated_emulate(f, g, ulp)).any(), ulp
    # 0.5 x is exact for every bf16 x whose half is a normal bf16, and where it is not, 1 + th == 1: dropping that rounding changes no bit
    assert np.array_equal(G.gated_emulate(f, g, mutation="half_x_unrounded"), G.gated_emulate(f, g))
    if n == G.GATED_SIZES[-1]:
        assert n > 8192 * 256 and len(np.unique(g)) == 65280
        tiny = np.abs(G.bf2f(g)) < 2.0 ** -125
        assert (exp.ambiguous() <= tiny).all() and tiny.sum() == 512 * G.GATED_REPS      # nothing is ambiguous beside the flush class
        assert len(np.unique(z[np.isfinite(z)])) == 38491
        assert exp.outside(G.gated_emulate(f, g, mutation="p3_unrounded")).any()
        assert np.isinf(z).any()                                                         # g^3 overflows: tanh is exactly +-1


def test_gelu_erf_cases():
    a, b, c = G.gelu_inputs("A"), G.gelu_inputs("B"), G.gelu_inputs("C")
    assert len(a) == 49025 * G.GELU_A_REPS > 4096 * 256 and len(b) == 256 and len(c) == 15999
    assert len(np.unique(np.concatenate([a, b, c]))) == 65280                # together: every finite bf16 value
    exp, y = G.gelu_ref(a)
    wide, _ = G.gelu_ref(np.unique(a), K=8.0)
    assert exp.ambiguous().mean() <= G.AMBIGUITY_CAP and wide.ambiguous().sum() == 289      # (at the cap of K too)
    for ulp in (-1, 0, 1):
        assert not exp.outside(G.gelu_emulate(a, ulp)).any(), ulp
        assert G.gelu_needed_K(G.gelu_emulate(np.unique(a), ulp), np.unique(a)) <= 2.0
    assert exp.outside(G.gelu_emulate(a, mutation="coarse_constant")).any()
    twice = G.gelu_emulate(G.gelu_emulate(a))                                # an element the stride loop visits twice
    assert exp.outside(twice).mean() > 0.3
    expb, yb = G.gelu_ref(b, abs_floor=True)
    assert not expb.outside(G.gelu_emulate(b)).any()
    odd = (b & 1) == 1                                                       # 0.5 v is a tie of the bf16 grid: why case B is exempt from the cap
    assert (G.bf16_from_f64(yb[odd] * (1 + 2.0 ** -40)) != G.bf16_from_f64(yb[odd] * (1 - 2.0 ** -40))).all()
    assert (G.gelu_emulate(c) == G.GELU_C_BITS).all()                        # a saturating erff: -0 in bits
    t = G.bf2f(c).astype(np.float64) * np.float64(np.float32(0.70710678118654752440))
    assert (G._erfc(-t) < 2.0 ** -50).all()


@pytest.mark.parametrize("c", G.SOFTMAX_CASES, ids=[c.name for c in G.SOFTMAX_CASES])
def test_softmax_case(c):
    op = G.softmax_operands(c)
    exp, x, d = G.softmax_reference(c, op)
    assert exp.ambiguous().mean() <= G.AMBIGUITY_CAP, exp.ambiguous().mean()
    got = G.softmax_emulate(c, op)
    assert not exp.outside(got).any()
    valid = op["mask"] != 0
    if c.kind != "equal":
        assert (G.bf2f(G.bf16_from_f32(op["sc"])) != op["sc"]).all()         # no score is bf16-representable
        assert len(np.unique(op["pos"])) == G.NUM_BUCKETS * c.H              # distinct per (bucket, head)
    if valid.any():
        assert d[..., valid].min() >= (-60.0 if c.kind != "deep" else -150.0)
        zero = G.softmax_zero_bits(c, op)
        assert (got[zero] == 0).all() and (exp.lo[0][zero] == 0).all() and (exp.hi[0][zero] == 0).all()
    if c.kind == "deep":
        assert d.min() <= -120.0
    if c.valid == 0 or c.kind == "equal":                                    # the anchors: exact with eps 0
        exact, _, _ = G.softmax_reference(c, op, eps=0.0)
        bits = int(G.bf16_from_f64(np.array([1.0 / c.L]))[0])
        assert bits == {64: 0x3C80, 256: 0x3B80, 512: 0x3B00}[c.L]
        assert (exact.lo == bits).all() and (exact.hi == bits).all() and (got == bits).all()


def test_softmax_tables_and_mutations():
    from mmpl_amd.t5 import relative_position_buckets
    for L in (64, 256, 512):
        assert np.array_equal(G.product_buckets(L), relative_position_buckets(L, G.NUM_BUCKETS).numpy())
    assert {c.H for c in G.SOFTMAX_CASES} == {1, 3} and {c.L for c in G.SOFTMAX_CASES} == {64, 256, 512}
    assert {c.valid for c in G.SOFTMAX_CASES if not c.holes} >= {0, 1, 37} and any(c.valid == c.L - 1 for c in G.SOFTMAX_CASES)
    failing = {m: [] for m in G.SOFTMAX_MUTATIONS}
    for c in G.SOFTMAX_CASES:
        op = G.softmax_operands(c)
        exp = G.softmax_reference(c, op)[0]
        for m in G.SOFTMAX_MUTATIONS:
            if exp.outside(G.softmax_emulate(c, op, m)).any():
                failing[m].append(c.name)
    print({m: len(v) for m, v in failing.items()})
    for m in G.SOFTMAX_MUTATIONS:
        assert failing[m], m
    assert all(SM[n].H == 3 for n in failing["pos_no_head"]) and all(SM[n].L >= 256 for n in failing["inv_wave0"])


def _torch_bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("n", G.UNIPC_SIZES)
def test_unipc_chain(n):
    """unipc_chain is tests/test_scheduler_host.py's emulate_kernel in bits, has no subnormal intermediate on these inputs, and its
    value mutations change bits (0.5 d1 is exact in bf16: leaving it unrounded is an identity)."""
    sts = _step_scalars()
    ops = G.unipc_operands(n)
    tens = [torch.from_numpy(o.view(np.int16).copy()).view(torch.bfloat16) for o in ops]
    assert G.UNIPC_SIZES[-1] > 8192 * 256
    for step in G.UNIPC_STEPS:
        st = sts[step]
        assert (st.use_corrector, st.corr_order, st.pred_order) == G.UNIPC_ORDERS[step]
        for with_u in (True, False):
            fu = ops[1] if with_u else None
            out, mids = G.unipc_chain(st, ops[0], fu, *ops[2:])
            assert G.no_subnormal(*mids), (step, with_u)
            want = emulate_kernel(st, tens[0], tens[1] if with_u else tens[0], *tens[2:])   # (fc == fu: the combine is the identity)
            for o, w in zip(out, want):
                assert np.array_equal(o, _torch_bits(w)), (step, with_u)
            if n != 255:                                                     # (the mutations: once, at the middle size)
                continue
            neutral, _ = G.unipc_chain(st, ops[0], fu, *ops[2:], mutation="half_d1_unrounded")
            assert all(np.array_equal(a, b) for a, b in zip(neutral, out))
            if with_u:
                m, _ = G.unipc_chain(st, ops[0], fu, *ops[2:], mutation="diff_unrounded")
                assert not np.array_equal(m[0], out[0]) and not np.array_equal(m[1], out[1])
            if st.pred_order == 2:
                m, _ = G.unipc_chain(st, ops[0], fu, *ops[2:], mutation="pred_m_swapped")
                assert not np.array_equal(m[0], out[0]) and np.array_equal(m[1], out[1])
