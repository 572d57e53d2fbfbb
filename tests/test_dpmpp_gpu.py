"""The fused CFG + DPM-Solver++ step (csrc/sampler.hip through mmpl_cfg_dpmpp_step / _table) and the pipeline with
sample_solver='dpm++' on the device (-m gpu).

  single steps   one launch per case on the operands of tests/dpmpp_ref.py: x, m0 and m1 equal `dpmpp_chain` in every bit (the chain is
                 one IEEE fp32 operation between bf16 roundings on both sides; tests/test_dpmpp_host.py ties it to the REAL reference's
                 trajectory), no mutant of dpmpp_ref.bites' table does (sizes above one element), the canaries behind every buffer and the two flows are intact;
  table form     equals the host-scalar form over all 50 steps, stops at the end of the table, rewinds;
  trajectory     the toy trajectory of tests/golden/dpmpp_sched.pt, free running from its first sample on the flows the reference was
                 fed: every sample equals the reference's (under the scalar semantics of its native platform) in every bit;
  pipeline       the T2V first chunk, tiny model, 10 steps per stage, against tests/golden/chunk_t2v_tiny_dpmpp.pt (the REAL reference's
                 stage loop with its DPM-Solver++ scheduler) at 60x104 -- the one latent size the reference model runs at (its
                 frame_seqlen 1560 is a literal) --, bound 2 x the fixture's own K/V-order noise as in tests/test_trajectory_gpu.py;
                 the three launch modes give the same bits (T2V and I2V, 16x24); the default solver's chunk is the same before and
                 after a 'dpm++' chunk in one process.
Measured on an MI355X: latents 6.16e-3, hand-off 6.20e-3 against the bound 1.23e-2.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dpmpp_ref as D
from tests import glue_ref as G
from tests.test_rowpass_exact_gpu import _check, _ptr, _stream, dev, host
from tests.util import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
TAIL = 64


def _scheduler(steps=50, shift=5.0):
    from mmpl_amd.scheduler import FlowDPMSolverMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    retrieve_timesteps(s, device=DEV, sigmas=get_sampling_sigmas(steps, shift))
    return s


_rows = {}


def _step_scalars(steps):
    if steps not in _rows:
        s = _scheduler(steps)
        _rows[steps] = [s.step_scalars(5.0) for _ in range(steps)]
    return _rows[steps]


def _compare(name, n, st, ops, with_u, bufs):
    fu = ops[1] if with_u else None
    want, _ = D.dpmpp_chain(st, ops[0], fu, *ops[2:])
    torch.cuda.synchronize()
    got = [host(t) for t in bufs[2:]]
    differ = {}
    for what, g, w in zip(("x", "m0", "m1"), got, want):
        differ[what] = int((g[:n] != w).sum())
        assert bool((g[n:] == G.CANARY).all()) and g.size == n + TAIL, what
    print(f"{name}: elements of {n} that differ from the emulation: {differ}")
    assert not any(differ.values()), differ
    for t, src in zip(bufs[:2], ops[:2]):                 # the flows are read only
        assert np.array_equal(host(t), G.with_canary(src))
    if n not in D.MUTANT_SIZES:
        return
    k = min(n, D.MUTANT_SLICE)
    head = [o[:k] for o in ops]
    for mut in D.MUTATIONS:
        m, _ = D.dpmpp_chain(st, head[0], head[1] if with_u else None, *head[2:], mutation=mut)
        bites = sum(D.differs(m, [w[:k] for w in want]))
        if D.bites(mut, st):                              # the table both tests share: this mutant has teeth here, and the kernel is not it
            assert bites and sum(D.differs(m, [g[:k] for g in got])), (name, mut)
        elif bites:
            assert sum(D.differs(m, [g[:k] for g in got])), (name, mut)


@pytest.mark.parametrize("with_u", [True, False], ids=["cfg", "combined"])
@pytest.mark.parametrize("n", D.SIZES)
def test_single_steps_equal_the_emulation(lib, n, with_u):
    ops = D.operands(n)
    for steps, picks in ((50, D.STEPS_50), (10, D.STEPS_10)):
        for step in picks:
            st = _step_scalars(steps)[step]
            assert st.order == D.ORDERS[(steps, step)]
            bufs = [dev(G.with_canary(o)) for o in ops]
            _check(lib, lib.mmpl_cfg_dpmpp_step(_ptr(bufs[0]), _ptr(bufs[1]) if with_u else None, *[_ptr(b) for b in bufs[2:]], n,
                                                C.byref(st), _stream()), f"dpm++ step {step} of {steps}")
            _compare(f"dpm++ n={n} step {step}/{steps} {'cfg' if with_u else 'combined'}", n, st, ops, with_u, bufs)


def test_unaligned_operands_take_the_element_wise_path(lib):
    """every pointer 2 bytes past a 16-byte boundary: the same bits, the element in front of each buffer and the canaries intact."""
    n, st = 255, _step_scalars(50)[25]
    ops = D.operands(n, seed=2)
    bufs = [dev(np.concatenate([np.full(1, G.CANARY, dtype=np.uint16), G.with_canary(o)])) for o in ops]
    _check(lib, lib.mmpl_cfg_dpmpp_step(*[_ptr(b, 2) for b in bufs], n, C.byref(st), _stream()), "dpm++ unaligned")
    torch.cuda.synchronize()
    want, _ = D.dpmpp_chain(st, *ops)
    for b, w in zip(bufs[2:], want):
        g = host(b)
        assert g[0] == G.CANARY and np.array_equal(g[1:n + 1], w) and bool((g[n + 1:] == G.CANARY).all())


def test_the_grid_stride_loop_past_the_block_cap(lib):
    """n = dpmpp_ref.STRIDE_SIZE, step 25 of 50: the first lanes go round the loop a second time, the last of them into the ragged tail.
    Every element against the emulation, evaluated on one period of the tiled operands."""
    n, st = D.STRIDE_SIZE, _step_scalars(50)[25]
    ops = D.operands(D.STRIDE_PERIOD, seed=3)
    want, _ = D.dpmpp_chain(st, *ops)
    bufs = [dev(G.with_canary(np.resize(o, n))) for o in ops]
    _check(lib, lib.mmpl_cfg_dpmpp_step(*[_ptr(b) for b in bufs], n, C.byref(st), _stream()), "dpm++ past the block cap")
    torch.cuda.synchronize()
    for what, b, w in zip(("x", "m0", "m1"), bufs[2:], want):
        g = host(b)
        assert np.array_equal(g[:n], np.resize(w, n)), what
        assert bool((g[n:] == G.CANARY).all()) and g.size == n + TAIL, what
    for b, src in zip(bufs[:2], ops[:2]):                 # the flows are read only
        assert np.array_equal(host(b), G.with_canary(np.resize(src, n)))


def test_table_step_at_one_entry_equals_the_emulation(lib):
    """The device-table form at step 2: the same bits, the counter advanced, the next timestep written."""
    n, step = 255, 2
    s = _scheduler(50)
    s.build_step_table(5.0, DEV)
    s._counter.fill_(step)
    ops = D.operands(n)                                  # the operands dpmpp_ref.bites is proven on
    bufs = [dev(G.with_canary(o)) for o in ops]
    t = torch.full([3], -1.0, dtype=torch.float32, device=DEV)
    _check(lib, lib.mmpl_cfg_dpmpp_step_table(*[_ptr(b) for b in bufs], n, _ptr(s._table), _ptr(s._counter), _ptr(t), _ptr(s._t_table), 3,
                                              s._table_n, _stream()), "dpm++ table")
    _compare("dpm++ table step 2", n, _step_scalars(50)[step], ops, True, bufs)
    assert int(s._counter.item()) == step + 1 and t.tolist() == [float(s.timesteps[step + 1])] * 3


def test_device_table_step_equals_host_scalar_step():
    """mmpl_cfg_dpmpp_step_table (scalars, step counter and next timestep on the device: the form captured in the per-denoise-step
    hipGraph) is bit-identical to mmpl_cfg_dpmpp_step over all 50 steps and leaves the right timestep; a 51st launch changes nothing;
    reset_step_table rewinds."""
    torch.manual_seed(0)
    x0 = torch.randn(3, 16, 8, 12, device=DEV).bfloat16()
    flows = [(torch.randn_like(x0), torch.randn_like(x0)) for _ in range(50)]
    a, b = _scheduler(50), _scheduler(50)
    xa, xb = x0.clone(), x0.clone()
    t = torch.full([3], float(b.timesteps[0]), dtype=torch.float32, device=DEV)
    b.build_step_table(5.0, DEV)
    assert b.step_index == 0 and b._table.numel() == 50 * 24
    for i, (fc, fu) in enumerate(flows):
        a.step_cfg(fc, fu, 5.0, xa)
        assert float(t[0]) == float(b.timesteps[i])              # the forwards of replay i would read this
        b.step_cfg_table(fc, fu, xb, t)
        assert torch.equal(xa, xb) and torch.equal(a._state[0], b._state[0]) and torch.equal(a._state[1], b._state[1]), i
    assert int(b._counter.item()) == 50 and len(a._state) == 2 and torch.isfinite(xa.float()).all()
    keep, keep_m, keep_t = xb.clone(), [m.clone() for m in b._state], t.clone()
    b.step_cfg_table(flows[0][0], flows[0][1], xb, t)
    assert torch.equal(xb, keep) and int(b._counter.item()) == 50 and torch.equal(t, keep_t)
    assert all(torch.equal(m, k) for m, k in zip(b._state, keep_m))
    b.reset_step_table(t)
    xb = x0.clone()
    assert int(b._counter.item()) == 0 and float(t[0]) == float(b.timesteps[0]) == 1000.0
    for fc, fu in flows:
        b.step_cfg_table(fc, fu, xb, t)
    assert torch.equal(xa, xb)


@pytest.mark.parametrize("steps", [50, 10])
def test_toy_trajectory_follows_the_reference_bit_for_bit(steps):
    """Free running from the fixture's first sample through `step` in the reference's call shape, fed the flows the reference was fed."""
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(f"{GOLDEN}/dpmpp_sched.pt")
    e, toy = fx[f"s{steps}"], fx["toy"]
    s = _scheduler(steps, e["shift"])
    assert torch.equal(s.timesteps.cpu(), e["timesteps"]) and torch.equal(s.sigmas, e["sigmas"])
    x = philox_normal(toy["shape"], toy["x_seed"], BF).cuda()
    for i, t in enumerate(s.timesteps):
        x = s.step(e["flow_gpu"][i].cuda(), t, x, return_dict=False)[0]
        assert torch.equal(x.cpu().view(torch.int16), e["traj_gpu"][i].view(torch.int16)), i
    assert not torch.equal(x.cpu(), e["traj_cpu"][-1])           # the CPU-semantics run ends elsewhere: the fixture tells them apart


# ------------------------------------------------------------------ pipeline
def _chunk(pipe, noise, renoise, initial=None):
    got = {}
    pipe.handoff_sink = lambda t: got.__setitem__("h", t.clone())
    if renoise is not None:
        pipe.renoise_override = {k: v.cuda() for k, v in renoise.items()}
    _, lat = pipe.inference(noise.cuda(), ["a cat"], initial_latent=None if initial is None else initial.cuda(), return_latents=True, decode=False)
    torch.cuda.synchronize()
    return lat.cpu(), got["h"].cpu()


def test_t2v_chunk_vs_reference_fixture():
    from mmpl_amd.scheduler import FlowDPMSolverMultistepScheduler
    from tests.test_pipeline_gpu import _setup
    from tests.test_trajectory_gpu import _inputs
    fx = torch.load(f"{GOLDEN}/chunk_t2v_tiny_dpmpp.pt")
    m, nf = fx["meta"], fx["noise_floor"]
    assert "REAL reference" in fx["produced_by"] and m["sample_solver"] == "dpm++" and m["steps"] == 10 and m["guidance"] == 5.0
    lat_hw = tuple(m["lat"])
    pipe, *_ = _setup("t2v", steps=m["steps"], lat=lat_hw, cfg_name=m["cfg"], weight_seed=m["weight_seed"], ctx_seeds=m["ctx_seeds"],
                      n_valid=m["n_valid"])
    pipe.sample_solver = "dpm++"
    assert pipe.use_graphs and pipe.step_graphs
    assert type(pipe._initialize_sample_scheduler(torch.zeros(1, device=DEV))) is FlowDPMSolverMultistepScheduler
    noise, renoise = _inputs(lat_hw, m["noise_seed"], m["renoise_seed_base"])
    lat, hand = _chunk(pipe, noise, renoise)
    (so, sw), (ho, hw) = m["out_stride"], m["handoff_stride"]
    e, eh = rel_l2(lat[..., ::so, ::sw], fx["out_strided"]), rel_l2(hand[..., ::ho, ::hw], fx["handoff_strided"])
    print(f"dpm++, 88 forwards (10 steps x CFG 5 x 4 stages + refresh) at {lat_hw[0]}x{lat_hw[1]}: HIP vs the reference under GPU scalar semantics: "
          f"latents {e:.3e} hand-off {eh:.3e} (bound 2 x the reference's K/V-order noise = {2 * nf['order_out']:.3e} / {2 * nf['order_handoff']:.3e})")
    assert torch.isfinite(lat.float()).all() and int(pipe.timesteps[0]) == 1000 and len(pipe.timesteps) == 10
    assert e <= 2 * nf["order_out"] and eh <= 2 * nf["order_handoff"]
    # the per-step hipGraph with the device table against per-forward graphs with host scalars: the same bits at this size too
    pipe.step_graphs = False
    lat2, hand2 = _chunk(pipe, noise, renoise)
    assert torch.equal(lat2, lat) and torch.equal(hand2, hand)


@pytest.mark.parametrize("mode", ["t2v", "i2v"])
def test_launch_modes_give_identical_bits(mode):
    """one hipGraph per denoise step (device table) == one hipGraph per forward + host scalars == eager launches."""
    from mmpl_amd.synthetic import philox_normal
    from tests.test_pipeline_gpu import LAT, _setup
    from tests.test_trajectory_gpu import _inputs
    pipe, *_ = _setup(mode, steps=10)
    pipe.sample_solver = "dpm++"
    noise, renoise = _inputs(LAT, 23 if mode == "t2v" else 24)
    renoise = renoise if mode == "t2v" else None
    initial = None if mode == "t2v" else philox_normal([1, 1, 16, *LAT], 56)
    lat, hand = _chunk(pipe, noise, renoise, initial)
    assert torch.isfinite(lat.float()).all() and lat.float().std() > 0.1
    pipe.step_graphs = False
    lat_f, hand_f = _chunk(pipe, noise, renoise, initial)
    pipe.use_graphs = False
    lat_e, hand_e = _chunk(pipe, noise, renoise, initial)
    assert torch.equal(lat_f, lat) and torch.equal(hand_f, hand)
    assert torch.equal(lat_e, lat) and torch.equal(hand_e, hand)


def test_default_solver_is_untouched_by_a_dpmpp_chunk():
    """The default solver's chunk before and after a 'dpm++' chunk on the same pipeline, and on a pipeline that never saw the
    attribute: the same bits; the 'dpm++' chunk is another trajectory."""
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    from tests.test_pipeline_gpu import LAT, _setup
    from tests.test_trajectory_gpu import _inputs
    noise, renoise = _inputs(LAT, 23)
    pipe, *_ = _setup("t2v", steps=10)
    assert pipe.sample_solver == "unipc" and type(pipe._initialize_sample_scheduler(torch.zeros(1, device=DEV))) is FlowUniPCMultistepScheduler
    before = _chunk(pipe, noise, renoise)
    pipe.sample_solver = "dpm++"
    other = _chunk(pipe, noise, renoise)
    pipe.sample_solver = "unipc"
    after = _chunk(pipe, noise, renoise)
    fresh = _chunk(_setup("t2v", steps=10)[0], noise, renoise)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(before[0], fresh[0]) and torch.equal(before[1], fresh[1])
    assert not torch.equal(other[0], before[0])
