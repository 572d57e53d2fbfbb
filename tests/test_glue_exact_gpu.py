"""The glue kernels of csrc/t5.hip and csrc/i2v.hip and the bf16 UniPC step of csrc/sampler.hip one launch at a time on exact inputs
(-m gpu): t5_gather_kernel, t5_softmax_kernel, t5_transpose_kernel, t5_gated_kernel, t5_zero_pad_kernel, gelu_erf_kernel and
add_kernel through their entry points (the launchers mmpl_t5_encode, mmpl_i2v_* and mmpl_clip_visual call), the UniPC step and its
table form through mmpl_cfg_unipc_step / _table.

Every case of tests/glue_ref.py's tables makes one launch and asserts
  - ZERO elements outside their candidates (glue_ref's docstring derives them; tests/test_glue_ref.py proves on the CPU that the
    inputs leave nothing else to tolerate) and at most 1 % ambiguous ones; the copies, the add and the UniPC step bit for bit;
  - every canary (behind each buffer, in every ld gap) and every input intact, bit for bit.
The gelu and softmax tests print the K / E their elements needed: what glue_ref.ERF_MEASURED / EXP_MEASURED record.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_ref as G
from tests.test_rowpass_exact_gpu import _check, _ptr, _stream, dev, host
from tests.test_scheduler_host import emulate_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 64


def _report(name, exp, g, extra="", cap=True):
    bad = exp.outside(g)
    amb = float(exp.ambiguous().mean())
    print(f"{name}: {int(bad.sum())} of {bad.size} elements outside their candidates, {amb:.5%} ambiguous{extra}")
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].tolist(), g[bad][:8].tolist(), exp.lo[:, bad][:, :8].tolist())
    if cap:
        assert amb <= G.AMBIGUITY_CAP


def _tail_intact(got, n):
    return bool((got.reshape(-1)[n:] == G.CANARY).all()) and got.size == n + TAIL


# ------------------------------------------------------------------ copies
@pytest.mark.parametrize("c", G.GATHER_CASES, ids=[c.name for c in G.GATHER_CASES])
def test_gather_bit_for_bit(lib, c):
    op = G.gather_operands(c)
    idd, ed, od = dev(op["ids"]), dev(G.with_canary(op["emb"])), dev(np.full(c.L * c.dim + TAIL, G.CANARY, dtype=np.uint16))
    _check(lib, lib.mmpl_t5_gather(_ptr(idd), _ptr(ed), _ptr(od), c.L, c.dim, _stream()), c.name)
    torch.cuda.synchronize()
    got = host(od)
    assert np.array_equal(got[:c.L * c.dim].reshape(c.L, c.dim), G.gather_ref(op)) and _tail_intact(got, c.L * c.dim)
    assert np.array_equal(host(ed), G.with_canary(op["emb"])) and np.array_equal(host(idd), op["ids"])


@pytest.mark.parametrize("c", G.TRANSPOSE_CASES, ids=[c.name for c in G.TRANSPOSE_CASES])
def test_transpose_bit_for_bit(lib, c):
    op = G.transpose_operands(c)
    n = c.H * c.c * c.L
    vd, td = dev(op["v"]), dev(np.full(n + TAIL, G.CANARY, dtype=np.uint16))
    _check(lib, lib.mmpl_t5_transpose(_ptr(vd, 2 * c.off), c.ld, _ptr(td), c.L, c.c, c.H, _stream()), c.name)
    torch.cuda.synchronize()
    got = host(td)
    assert np.array_equal(got[:n].reshape(c.H, c.c, c.L), G.transpose_ref(c, op)) and _tail_intact(got, n)
    assert np.array_equal(host(vd), op["v"])


@pytest.mark.parametrize("kind", G.ZERO_PAD_MASKS)
def test_zero_pad_bit_for_bit(lib, kind):
    op = G.zero_pad_operands(kind)
    L, dim = op["out"].shape
    md, od = dev(op["mask"]), dev(G.with_canary(op["out"]))
    _check(lib, lib.mmpl_t5_zero_pad(_ptr(od), _ptr(md), L, dim, _stream()), kind)
    torch.cuda.synchronize()
    got = host(od)
    assert np.array_equal(got[:L * dim].reshape(L, dim), G.zero_pad_ref(op)) and _tail_intact(got, L * dim)
    assert np.array_equal(host(md), op["mask"])


@pytest.mark.parametrize("n", G.ADD_SIZES)
def test_add_bit_for_bit(lib, n):
    a, b = G.add_operands(n)
    ad, bd = dev(G.with_canary(a)), dev(G.with_canary(b))
    _check(lib, lib.mmpl_add(_ptr(ad), _ptr(bd), n, _stream()), f"add {n}")
    torch.cuda.synchronize()
    got = host(ad)
    bad = got[:n] != G.add_ref(a, b)
    print(f"add n={n}: {int(bad.sum())} elements differ from one fp32 add and one rounding")
    assert not bad.any(), np.argwhere(bad)[:8].tolist()
    assert _tail_intact(got, n) and np.array_equal(host(bd), G.with_canary(b))


# ------------------------------------------------------------------ gated GELU, GELU(erf)
@pytest.mark.parametrize("n", G.GATED_SIZES)
def test_gated_every_finite_bf16(lib, n):
    f, g = G.gated_operands(n)
    exp, _ = G.gated_reference(f, g)
    fd, gd = dev(G.with_canary(f)), dev(G.with_canary(g))
    _check(lib, lib.mmpl_t5_gated(_ptr(fd), _ptr(gd), n, _stream()), f"gated {n}")
    torch.cuda.synchronize()
    got = host(fd)
    _report(f"gated n={n}", exp, got[:n])
    assert _tail_intact(got, n) and np.array_equal(host(gd), G.with_canary(g))


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_gelu_erf_in_place(lib, case):
    x = G.gelu_inputs(case)
    n = len(x)
    xd = dev(G.with_canary(x))
    _check(lib, lib.mmpl_gelu_erf(_ptr(xd), n, _stream()), f"gelu_erf {case}")
    torch.cuda.synchronize()
    got = host(xd)
    assert _tail_intact(got, n)
    if case == "C":                                                        # a saturating erff: -0 in bits
        bad = got[:n] != G.GELU_C_BITS
        print(f"gelu_erf C: {int(bad.sum())} of {n} elements are not -0")
        assert not bad.any(), ([hex(v) for v in x[bad][:8]], [hex(v) for v in got[:n][bad][:8]])
        return
    exp, y = G.gelu_ref(x, abs_floor=case == "B")
    m = n // G.GELU_A_REPS if case == "A" else n                            # (measured on the first repetition; the criterion below holds all)
    need = G.gelu_needed_K(got[:m], x[:m], abs_floor=case == "B")
    _report(f"gelu_erf {case}", exp, got[:n], f", needed K {need:.3f} ulp of {G.ERF_K:.2f}", cap=case == "A")


# ------------------------------------------------------------------ softmax
@pytest.mark.parametrize("c", G.SOFTMAX_CASES, ids=[c.name for c in G.SOFTMAX_CASES])
def test_softmax_exact(lib, c):
    from mmpl_amd.t5 import relative_position_buckets
    bucket = relative_position_buckets(c.L, G.NUM_BUCKETS).numpy() if c.table == "product" else None
    op = G.softmax_operands(c, bucket)
    exp, x, d = G.softmax_reference(c, op)
    n = c.H * c.L * c.L
    sc = np.concatenate([op["sc"].reshape(-1), np.full(TAIL, np.nan, dtype=np.float32)])
    bk = np.concatenate([op["bucket"], np.zeros(TAIL, dtype=np.int32)])
    sd, pd, bd, md = dev(sc), dev(G.with_canary(op["pos"])), dev(bk), dev(op["mask"])
    od = dev(np.full(n + TAIL, G.CANARY, dtype=np.uint16))
    _check(lib, lib.mmpl_t5_softmax(_ptr(sd), _ptr(pd), _ptr(bd), _ptr(md), _ptr(od), c.H, c.L, _stream()), c.name)
    torch.cuda.synchronize()
    got = host(od)
    g = got[:n].reshape(c.H, c.L, c.L)
    need = G.softmax_needed_E(g, x, d)
    _report(c.name, exp, g, f", needed E {need / G.U:.2f} u (eps {(2 * need + 13 * G.U) / G.U:.2f} u of {G.SOFTMAX_EPS / G.U:.2f} u), "
            f"d >= {float(d[..., op['mask'] != 0].min()) if (op['mask'] != 0).any() else 0.0:.1f}")
    zero = G.softmax_zero_bits(c, op)
    assert (g[zero] == 0).all()                                            # masked keys: +0 in bits
    if c.valid == 0 or c.kind == "equal":                                  # the anchors
        assert (g == int(G.bf16_from_f64(np.array([1.0 / c.L]))[0])).all()
    assert _tail_intact(got, n)
    assert np.array_equal(host(sd).view(np.uint32), sc.view(np.uint32)) and np.array_equal(host(pd), G.with_canary(op["pos"]))
    assert np.array_equal(host(bd), bk) and np.array_equal(host(md), op["mask"])


# ------------------------------------------------------------------ UniPC
_scalars = []


def _step_scalars():
    if not _scalars:
        from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
        s = FlowUniPCMultistepScheduler(1000, 2, 1.0)
        s.set_timesteps(50, shift=5.0)
        _scalars.extend(s.step_scalars(5.0) for _ in range(50))
    return _scalars


def _bf(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def _unipc_compare(name, n, st, ops, with_u, bufs):
    tens = [_bf(o) for o in ops]
    want = emulate_kernel(st, tens[0], tens[1] if with_u else tens[0], *tens[2:])          # (fc == fu: the combine is the identity)
    torch.cuda.synchronize()
    differ = {}
    for what, t, w in zip(("x", "m0", "m1", "last_sample"), bufs[2:], want):
        got = host(t)
        differ[what] = int((got[:n] != w.view(torch.int16).numpy().view(np.uint16)).sum())
        assert _tail_intact(got, n)
    print(f"{name}: elements of {n} that differ from the emulation: {differ}")
    assert not any(differ.values()), differ
    for t, src in zip(bufs[:2], ops[:2]):
        assert np.array_equal(host(t), G.with_canary(src))


def _unipc_steps(lib, n, with_u, steps):
    ops = G.unipc_operands(n)
    for step in steps:
        st = _step_scalars()[step]
        assert (st.use_corrector, st.corr_order, st.pred_order) == G.UNIPC_ORDERS[step]
        bufs = [dev(G.with_canary(o)) for o in ops]
        _check(lib, lib.mmpl_cfg_unipc_step(_ptr(bufs[0]), _ptr(bufs[1]) if with_u else None, *[_ptr(b) for b in bufs[2:]], n,
                                            C.byref(st), _stream()), f"unipc step {step}")
        _unipc_compare(f"unipc n={n} step {step} {'cfg' if with_u else 'combined'}", n, st, ops, with_u, bufs)


@pytest.mark.parametrize("with_u", [True, False], ids=["cfg", "combined"])
@pytest.mark.parametrize("n", G.UNIPC_SIZES)
def test_unipc_equals_emulation(lib, n, with_u):
    _unipc_steps(lib, n, with_u, G.UNIPC_STEPS)


@pytest.mark.parametrize("with_u", [True, False], ids=["cfg", "combined"])
@pytest.mark.parametrize("n", [7, 8, 9])
def test_unipc_around_the_vector_width(lib, n, with_u):
    """One lane's 8 elements: an element-wise tail alone, exactly one 16-byte access, one access and a tail of one; at step 2 (corrector
    and predictor of order 2) and step 0 (no corrector, order 1)."""
    _unipc_steps(lib, n, with_u, (2, 0))


def test_unipc_unaligned_operands_take_the_element_wise_path(lib):
    """every pointer 2 bytes past a 16-byte boundary: the same bits, the element in front of each buffer and the canaries intact."""
    n, st = 255, _step_scalars()[25]
    ops = G.unipc_operands(n, seed=2)
    bufs = [dev(np.concatenate([np.full(1, G.CANARY, dtype=np.uint16), G.with_canary(o)])) for o in ops]
    _check(lib, lib.mmpl_cfg_unipc_step(*[_ptr(b, 2) for b in bufs], n, C.byref(st), _stream()), "unipc unaligned")
    torch.cuda.synchronize()
    want = emulate_kernel(st, *[_bf(o) for o in ops])
    for b, w in zip(bufs[2:], want):
        g = host(b)
        assert g[0] == G.CANARY and np.array_equal(g[1:n + 1], w.view(torch.int16).numpy().view(np.uint16))
        assert bool((g[n + 1:] == G.CANARY).all()) and g.size == n + 1 + TAIL
    for b, src in zip(bufs[:2], ops[:2]):                 # the flows are read only
        assert np.array_equal(host(b)[1:], G.with_canary(src))


def test_unipc_table_equals_emulation(lib):
    """The device-table form at step 2 (corrector and predictor of order 2): the same bits, the counter advanced, the next timestep written."""
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    n, step = 255, 2
    s = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    s.set_timesteps(50, shift=5.0)
    s.build_step_table(5.0, DEV)
    s._counter.fill_(step)
    ops = G.unipc_operands(n, seed=1)
    bufs = [dev(G.with_canary(o)) for o in ops]
    t = torch.full([3], -1.0, dtype=torch.float32, device=DEV)
    _check(lib, lib.mmpl_cfg_unipc_step_table(*[_ptr(b) for b in bufs], n, _ptr(s._table), _ptr(s._counter), _ptr(t), _ptr(s._t_table), 3,
                                              s._table_n, _stream()), "unipc table")
    _unipc_compare("unipc table step 2", n, _step_scalars()[step], ops, True, bufs)
    assert int(s._counter.item()) == step + 1 and t.tolist() == [float(s.timesteps[step + 1])] * 3
