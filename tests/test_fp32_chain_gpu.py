"""The float32 latent chain's kernels on the device (-m gpu): csrc/sampler.hip through mmpl_cfg_unipc_step_f32 /
mmpl_cfg_dpmpp_step_f32 and their _table forms, one launch each, against tests/fp32_chain_ref.py BIT FOR BIT (the restatement is
one IEEE fp32 operation per kernel operation; tests/test_fp32_chain_host.py ties it to the REAL reference's schedulers).

  single steps   n in {1, 3, 255, 256, 257, 4099, 18432}, every pointer 16-byte aligned (the vector path) and every pointer one
                 element further (4-byte / 2-byte aligned only: the element-wise path); the steps that take every branch -- UniPC
                 step 0 (no corrector, predictor order 1), 1 (corrector 1, predictor 2), 25 (2 / 2), 49 (predictor order 1),
                 DPM-Solver++ step 0 (order 1), 1 and 25 (order 2), 49 (the final one) --, with and without flow_uncond, with and
                 without x_bf16; normal-range random float32 operands (|v| in [2^-20, 2^20]); x, m0, m1, last_sample equal the
                 restatement in every bit, x_bf16 == x.to(bfloat16), the flows and the sentinels around every buffer are intact;
  table form     the 6-step trajectories of tests/golden/fp32_chain.pt replayed by six launches of ONE captured graph give the
                 REAL reference's x at every step in every bit (the table carries the fixture's record of the scalars: the
                 last bits of the host's torch.log / expm1 / linalg.solve depend on its CPU); a seventh replay changes nothing;
                 reset_step_table rewinds;
  rejects        bad arguments return an error and launch nothing.
"""
import ctypes as C

import pytest
import torch

from tests import fp32_chain_ref as R
from tests.dpmpp_ref import STRIDE_PERIOD, STRIDE_SIZE
from tests.test_fp32_chain_host import FX, f32_scheduler, recorded_rows
from tests.test_rowpass_exact_gpu import _check, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
PAD = 8                                               # elements in front of and behind every operand (8 floats / 8 bf16: 16-byte multiples)
SENT_F, SENT_B = -7777.25, -3.0e38                    # the sentinels (float32 / bf16 buffers)
UNIPC_STEPS = {0: (0, 1, 1), 1: (1, 1, 2), 25: (1, 2, 2), 49: (1, 2, 1)}     # step -> (use_corrector, corr_order, pred_order)
DPMPP_STEPS = {0: 1, 1: 2, 25: 2, 49: 1}                                      # step -> order

_rows = {}


def _scalars(solver):
    if solver not in _rows:
        s = f32_scheduler(solver, 50, 5.0)
        _rows[solver] = [s.step_scalars(5.0) for _ in range(50)]
    return _rows[solver]


def _padded(values, off, sentinel):
    """values (host tensor) on the device inside a sentinel-filled buffer, `off` elements past a 16-byte boundary -> (buffer, view)."""
    n = values.numel()
    buf = torch.full([n + 2 * PAD + 1], sentinel, dtype=values.dtype, device=DEV)
    view = buf[PAD + off:PAD + off + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == (off * values.element_size()) % 16
    return buf, view


def _intact(buf, off, n, sentinel):
    s = torch.tensor(sentinel, dtype=buf.dtype)
    return bool((buf[:PAD + off].cpu() == s).all()) and bool((buf[PAD + off + n:].cpu() == s).all())


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == F32 else t.view(torch.int16) if t.dtype == BF else t


def _launch_and_compare(lib, solver, step, n, off, with_u, with_shadow):
    st = _scalars(solver)[step]
    fc, fu, x, m0, m1, last = R.operands(n, seed=step)
    if solver == "unipc":
        want = R.unipc_f32(st, fc, fu if with_u else None, x, m0, m1, last)
        names, ins = ("x", "m0", "m1", "last"), (x, m0, m1, last)
    else:
        want = R.dpmpp_f32(st, fc, fu if with_u else None, x, m0, m1)
        names, ins = ("x", "m0", "m1"), (x, m0, m1)
    flows = [_padded(v, off, SENT_B) for v in (fc, fu)]
    state = [_padded(v, off, SENT_F) for v in ins]
    shadow = _padded(torch.full([n], SENT_B, dtype=BF), off, SENT_B)
    args = [_ptr(flows[0][1]), _ptr(flows[1][1]) if with_u else None] + [_ptr(v) for _, v in state] + [_ptr(shadow[1]) if with_shadow else None]
    fn = lib.mmpl_cfg_unipc_step_f32 if solver == "unipc" else lib.mmpl_cfg_dpmpp_step_f32
    _check(lib, fn(*args, n, C.byref(st), _stream()), f"{solver} f32 step {step}")
    torch.cuda.synchronize()
    tag = f"{solver} step {step} n={n} off={off} {'cfg' if with_u else 'combined'} {'shadow' if with_shadow else 'no shadow'}"
    differ = {k: int((_bits(v) != _bits(w)).sum()) for k, (_, v), w in zip(names, state, want)}
    assert not any(differ.values()), (tag, differ)
    for (buf, _), _v in zip(state, ins):
        assert _intact(buf, off, n, SENT_F), tag
    for (buf, v), src in zip(flows, (fc, fu)):                            # the flows are read only
        assert _intact(buf, off, n, SENT_B) and torch.equal(_bits(v), _bits(src)), tag
    assert _intact(shadow[0], off, n, SENT_B), tag
    if with_shadow:
        assert torch.equal(_bits(shadow[1]), _bits(want[0].to(BF))), tag   # == bf16(x_new), round to nearest even
        assert torch.equal(_bits(shadow[1]), _bits(state[0][1].to(BF))), tag
    else:
        assert bool((shadow[1].cpu() == torch.tensor(SENT_B, dtype=BF)).all()), tag
    return differ


def test_the_chosen_steps_take_every_branch():
    for step, (uc, co, po) in UNIPC_STEPS.items():
        st = _scalars("unipc")[step]
        assert (st.use_corrector, st.corr_order if uc else 1, st.pred_order) == (uc, co, po), step
    for step, order in DPMPP_STEPS.items():
        assert _scalars("dpm++")[step].order == order, step
    assert _scalars("dpm++")[1].inv_r0 == 0.0 and _scalars("dpm++")[25].inv_r0 != 0.0


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", R.SIZES)
def test_unipc_f32_single_steps_equal_the_restatement(lib, n, off):
    for step in UNIPC_STEPS:
        for with_u in (True, False):
            for with_shadow in (True, False):
                _launch_and_compare(lib, "unipc", step, n, off, with_u, with_shadow)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", R.SIZES)
def test_dpmpp_f32_single_steps_equal_the_restatement(lib, n, off):
    for step in DPMPP_STEPS:
        for with_u in (True, False):
            for with_shadow in (True, False):
                _launch_and_compare(lib, "dpm++", step, n, off, with_u, with_shadow)


def test_dpmpp_f32_strides_past_the_block_cap(lib):
    """n = dpmpp_ref.STRIDE_SIZE, step 25 of 50: the first lanes go round the grid-stride loop a second time, the last of them into
    the ragged tail.  Every element against the restatement, evaluated on one period of the tiled operands."""
    n, st = STRIDE_SIZE, _scalars("dpm++")[25]
    ops = R.operands(STRIDE_PERIOD, seed=25)[:5]
    want = R.dpmpp_f32(st, *ops)
    tile = lambda v: v.repeat(-(-n // STRIDE_PERIOD))[:n]
    flows = [_padded(tile(v), 0, SENT_B) for v in ops[:2]]
    state = [_padded(tile(v), 0, SENT_F) for v in ops[2:]]
    shadow = _padded(torch.full([n], SENT_B, dtype=BF), 0, SENT_B)
    _check(lib, lib.mmpl_cfg_dpmpp_step_f32(*[_ptr(v) for _, v in flows + state + [shadow]], n, C.byref(st), _stream()), "dpm++ f32 past the block cap")
    torch.cuda.synchronize()
    for what, (buf, v), w in zip(("x", "m0", "m1"), state, want):
        assert torch.equal(_bits(v), _bits(tile(w))) and _intact(buf, 0, n, SENT_F), what
    assert torch.equal(_bits(shadow[1]), _bits(tile(want[0].to(BF)))) and _intact(shadow[0], 0, n, SENT_B)
    for (buf, v), src in zip(flows, ops[:2]):                              # the flows are read only
        assert torch.equal(_bits(v), _bits(tile(src))) and _intact(buf, 0, n, SENT_B)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("solver", ["unipc", "dpm++"])
def test_a_negative_counter_is_a_no_op_in_every_table_form(lib, solver, dtype):
    """counter = -1: x, the solver state, the shadow, the counter and `timestep` keep every bit.  table_dev is row 1 of a table whose
    every row holds the valid coefficients of step 25, so a kernel without the guard applies row 0 and changes the tensors: it does
    not read out of bounds."""
    from mmpl_amd.pipeline._common import make_sample_scheduler
    n = 255
    fc, fu, *state = R.operands(n, seed=4)
    state = [v.to(dtype).to(DEV) for v in state[:4 if solver == "unipc" else 3]]          # x, m0, m1 (, last_sample)
    s, _ = make_sample_scheduler(solver, 1000, 50, 5.0, "cpu")
    s._ensure_state(torch.zeros(1, dtype=dtype))                                          # the rows' struct is the storage type's
    row = bytes([s.step_scalars(5.0) for _ in range(26)][25])
    table = torch.frombuffer(bytearray(row * 3), dtype=torch.uint8).to(DEV)
    counter = torch.full([1], -1, dtype=torch.int32, device=DEV)
    t, t_table = torch.full([3], -1.0, dtype=F32, device=DEV), torch.full([2], 500.0, dtype=F32, device=DEV)
    shadow = [torch.full([n], SENT_B, dtype=BF, device=DEV)] if dtype == F32 else []
    fc, fu = fc.to(DEV), fu.to(DEV)
    keep = [v.clone() for v in (*state, *shadow, counter, t)]
    fn = getattr(lib, f"mmpl_cfg_{s._stem}_step{'_f32' if dtype == F32 else ''}_table")
    _check(lib, fn(*[_ptr(v) for v in (fc, fu, *state, *shadow)], n, _ptr(table, len(row)), _ptr(counter), _ptr(t), _ptr(t_table), 3, 2,
                   _stream()), f"{solver} {dtype} counter -1")
    torch.cuda.synchronize()
    assert int(counter.item()) == -1
    for a, b in zip((*state, *shadow, counter, t), keep):
        assert torch.equal(_bits(a), _bits(b))


def test_a_contracted_or_reciprocal_kernel_would_show(lib):
    """The operands have teeth: on them the restatement differs from itself with 1 / rk multiplied (UniPC 2 / 2 step) -- what the
    kernel is held against is not insensitive to the last bit."""
    st = _scalars("unipc")[25]
    ops = R.operands(4099, seed=25)
    a = R.unipc_f32(st, *ops)
    b = R.unipc_f32(st, *ops, mutation="inv_rk")
    assert int((_bits(a[0]) != _bits(b[0])).sum()) > 0


@pytest.mark.parametrize("solver", ["unipc", "dpm++"])
def test_table_form_replays_the_reference_trajectory_from_one_graph(solver):
    e = FX["sched"][solver]["s6"]
    n, steps = e["x0"].numel(), e["steps"]
    s = f32_scheduler(solver, steps, e["shift"])
    x = e["x0"].to(DEV).clone()
    shadow = torch.full([n], SENT_B, dtype=BF, device=DEV)
    fc, fu = torch.empty(n, dtype=BF, device=DEV), torch.empty(n, dtype=BF, device=DEV)
    t = torch.full([3], -1.0, dtype=F32, device=DEV)
    s._ensure_state(x)
    s.build_step_table(e["guidance"], DEV)
    assert s.step_index == 0 and s._table_dtype == F32
    # the table's rows as the machine that made the fixture computed them (the last bits of torch.log / expm1 / linalg.solve depend
    # on the host CPU; tests/test_fp32_chain_host.py holds this host's own scalars to them)
    rows = recorded_rows(solver, e)
    packed = torch.frombuffer(bytearray(b"".join(bytes(r) for r in rows)), dtype=torch.uint8)
    assert packed.numel() == s._table.numel()
    s._table.copy_(packed)

    def start():
        x.copy_(e["x0"])
        shadow.fill_(SENT_B)
        s.reset_step_table(t)

    start()
    fc.copy_(e["flow_cond"][0]), fu.copy_(e["flow_uncond"][0])
    s.step_cfg_table(fc, fu, x, t, sample_bf16=shadow)                     # eager once (loads the kernels outside the capture)
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(e["x"][0]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s.step_cfg_table(fc, fu, x, t, sample_bf16=shadow)
    for _ in range(2):                                                     # the second pass: reset_step_table rewinds
        start()
        assert t.tolist() == [float(e["timesteps"][0])] * 3
        for i in range(steps):
            fc.copy_(e["flow_cond"][i]), fu.copy_(e["flow_uncond"][i])
            g.replay()
            torch.cuda.synchronize()
            differ = int((_bits(x) != _bits(e["x"][i])).sum())
            assert differ == 0, (solver, i, differ)
            assert torch.equal(_bits(shadow), _bits(e["x"][i].to(BF)))
            assert int(s._counter.item()) == i + 1
            assert t.tolist() == [float(e["timesteps"][min(i + 1, steps - 1)])] * 3
        keep = [v.clone() for v in (x, shadow, t, *s._state)]
        g.replay()                                                         # a seventh replay changes nothing, x_bf16 included
        torch.cuda.synchronize()
        assert int(s._counter.item()) == steps
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((x, shadow, t, *s._state), keep))


def test_bad_arguments_launch_nothing(lib):
    n = 64
    st_u, st_d = _scalars("unipc")[25], _scalars("dpm++")[25]
    fc, fu, x, m0, m1, last = [v.to(DEV) for v in R.operands(n, seed=3)]
    shadow = torch.full([n], SENT_B, dtype=BF, device=DEV)
    s = f32_scheduler("unipc", 6, 8.0)
    s._ensure_state(x.clone())
    s.build_step_table(5.0, DEV)
    d = f32_scheduler("dpm++", 6, 8.0)
    d._ensure_state(x.clone())
    d.build_step_table(5.0, DEV)
    t = torch.full([1], -1.0, dtype=F32, device=DEV)
    keep = [v.clone() for v in (x, m0, m1, last, shadow, t, s._counter, d._counter)]
    P, S = _ptr, _stream()
    tab_u = (P(s._table), P(s._counter), P(t), P(s._t_table))
    tab_d = (P(d._table), P(d._counter), P(t), P(d._t_table))
    bad = [
        lib.mmpl_cfg_unipc_step_f32(None, P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, C.byref(st_u), S),
        lib.mmpl_cfg_unipc_step_f32(P(fc), P(fu), None, P(m0), P(m1), P(last), P(shadow), n, C.byref(st_u), S),
        lib.mmpl_cfg_unipc_step_f32(P(fc), P(fu), P(x), P(m0), P(m1), None, P(shadow), n, C.byref(st_u), S),
        lib.mmpl_cfg_unipc_step_f32(P(fc), P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, None, S),
        lib.mmpl_cfg_unipc_step_f32(P(fc), P(fu), P(x, 2), P(m0), P(m1), P(last), P(shadow), n, C.byref(st_u), S),     # float32 at 2 bytes
        lib.mmpl_cfg_unipc_step_f32(P(fc), P(fu), P(x), P(m0), P(m1, 1), P(last), P(shadow), n, C.byref(st_u), S),
        lib.mmpl_cfg_dpmpp_step_f32(P(fc), P(fu), P(x), None, P(m1), P(shadow), n, C.byref(st_d), S),
        lib.mmpl_cfg_dpmpp_step_f32(P(fc), P(fu), P(x), P(m0, 2), P(m1), P(shadow), n, C.byref(st_d), S),
        lib.mmpl_cfg_dpmpp_step_f32(P(fc), P(fu), P(x), P(m0), P(m1), P(shadow), n, None, S),
        lib.mmpl_cfg_unipc_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, *tab_u, 1, 0, S),          # n_steps < 1
        lib.mmpl_cfg_unipc_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, *tab_u, -1, 6, S),         # n_timestep < 0
        lib.mmpl_cfg_unipc_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, None, *tab_u[1:], 1, 6, S),
        lib.mmpl_cfg_unipc_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(last), P(shadow), n, tab_u[0], None, *tab_u[2:], 1, 6, S),
        lib.mmpl_cfg_unipc_step_f32_table(P(fc), P(fu), P(x, 2), P(m0), P(m1), P(last), P(shadow), n, *tab_u, 1, 6, S),
        lib.mmpl_cfg_dpmpp_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(shadow), n, *tab_d, 1, 0, S),
        lib.mmpl_cfg_dpmpp_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(shadow), n, *tab_d, -1, 6, S),
        lib.mmpl_cfg_dpmpp_step_f32_table(P(fc), None, None, P(m0), P(m1), P(shadow), n, *tab_d, 1, 6, S),
        lib.mmpl_cfg_dpmpp_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(shadow), n, *tab_d[:3], None, 1, 6, S),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert b"mmpl_cfg_dpmpp_step_f32_table" in lib.mmpl_last_error()
    for a, b in zip((x, m0, m1, last, shadow, t, s._counter, d._counter), keep):
        assert torch.equal(_bits(a), _bits(b))
    # n_timestep == 0 is allowed: the step is applied, no timestep is written
    _check(lib, lib.mmpl_cfg_dpmpp_step_f32_table(P(fc), P(fu), P(x), P(m0), P(m1), P(shadow), n, *tab_d, 0, 6, S), "n_timestep 0")
    torch.cuda.synchronize()
    assert int(d._counter.item()) == 1 and float(t[0]) == -1.0 and not torch.equal(x, keep[0])
