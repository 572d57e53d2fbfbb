"""Fused CFG + FlowUniPC HIP step vs the oracle scheduler and the reference's golden trajectory (-m gpu)."""
import pytest
import torch

from tests.util import GOLDEN, bf16_ulp_frac, max_abs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def test_unipc_trajectory_matches_reference_golden():
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    from mmpl_amd.synthetic import philox_normal
    fx = torch.load(f"{GOLDEN}/sched.pt")
    s = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    s.set_timesteps(50, shift=5.0)
    assert torch.equal(s.timesteps, fx["timesteps"]) and torch.equal(s.sigmas, fx["sigmas"])
    x = philox_normal([1, 3, 4, 6, 8], 5, BF).cuda()
    target = philox_normal([1, 3, 4, 6, 8], 6, BF).cuda()
    worst = 0.0
    for i, t in enumerate(s.timesteps):
        v = ((x - target) * (1.0 + 0.1 * torch.sin(x.float() * 3 + i).to(BF))).contiguous()
        x = s.step(v, t, x, return_dict=False)[0]
        ref = fx["traj_bf16"][i]
        # the driving field is evaluated on our own x, so compare loosely along the way and tightly in ulps per step below
        worst = max(worst, max_abs(x, ref))
    # the golden run is the reference on CPU, whose `scalar * tensor` products round the scalar to bf16 (see
    # oracle/unipc_ref.py); the HIP step keeps fp32 scalars like PyTorch's GPU kernels -> loose bound here, the
    # bit-level check is test_unipc_single_steps_bit_level
    assert worst < 0.15, worst


def test_unipc_single_steps_bit_level():
    """Feed the reference trajectory's own states: each fused step must land within 1 bf16 ulp of the oracle step, and must equal
    the bit-level emulation of the kernel's chain (tests/test_scheduler_host.py: emulate_kernel) fed the same states, in every bit
    of x, m0, m1 and last_sample: every operation of the chain is one IEEE fp32 operation between two bf16 roundings."""
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    from mmpl_amd.synthetic import philox_normal
    from oracle.unipc_ref import FlowUniPCRef
    from tests.test_scheduler_host import emulate_kernel
    shape = [1, 7, 16, 12, 20]
    o = FlowUniPCRef(1000, 2, 1.0, gpu_scalar_semantics=True)   # the HIP step follows PyTorch's GPU scalar rule
    o.set_timesteps(50, shift=5.0)
    s = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    s.set_timesteps(50, shift=5.0)
    s2 = FlowUniPCMultistepScheduler(1000, 2, 1.0)              # the same scalars, step by step, for the emulation
    s2.set_timesteps(50, shift=5.0)
    x = philox_normal(shape, 1, BF)
    xg = x.clone().cuda()
    bad = 0.0
    for i in range(50):
        fc, fu = philox_normal(shape, 100 + i, BF), philox_normal(shape, 200 + i, BF)
        flow = fu + 5.0 * (fc - fu)
        before = [xg.cpu()] + ([t.cpu() for t in s._state] if s._state is not None else [torch.zeros_like(x)] * 3)
        x = o.step(flow, x)
        xg = s.step_cfg(fc.cuda(), fu.cuda(), 5.0, xg)
        want = emulate_kernel(s2.step_scalars(5.0), fc, fu, *before)
        for name, got, w in zip(("x", "m0", "m1", "last_sample"), [xg] + list(s._state), want):
            assert torch.equal(got.cpu().view(torch.int16), w.view(torch.int16)), (i, name)
        bad = max(bad, bf16_ulp_frac(xg, x, 1))
        xg = x.clone().cuda()                     # re-sync so errors do not compound across steps
        s._state[0].copy_(o.model_outputs[-1])
        if o.model_outputs[-2] is not None:
            s._state[1].copy_(o.model_outputs[-2])
        s._state[2].copy_(o.last_sample)
    assert bad < 2e-3, bad


def test_device_table_step_equals_host_scalar_step():
    """mmpl_cfg_unipc_step_table (scalars, step counter and next timestep on the device: the form captured in the
    per-denoise-step hipGraph) is bit-identical to mmpl_cfg_unipc_step over all 50 steps, and leaves the right timestep."""
    from mmpl_amd.scheduler import FlowUniPCMultistepScheduler
    torch.manual_seed(0)
    dev = "cuda:0"
    x0 = torch.randn(3, 16, 8, 12, device=dev).bfloat16()
    flows = [(torch.randn_like(x0), torch.randn_like(x0)) for _ in range(50)]
    a = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    a.set_timesteps(50, shift=5.0)
    b = FlowUniPCMultistepScheduler(1000, 2, 1.0)
    b.set_timesteps(50, shift=5.0)
    xa, xb = x0.clone(), x0.clone()
    t = torch.full([3], float(b.timesteps[0]), dtype=torch.float32, device=dev)
    b.build_step_table(5.0, dev)
    for i, (fc, fu) in enumerate(flows):
        a.step_cfg(fc, fu, 5.0, xa)
        assert float(t[0]) == float(b.timesteps[i])              # the forwards of replay i would read this
        b.step_cfg_table(fc, fu, xb, t)
        assert torch.equal(xa, xb), i
    assert int(b._counter.item()) == 50
    # a replay beyond the uploaded table is a no-op (no out-of-bounds coefficients, counter stays clamped) ...
    keep = xb.clone()
    b.step_cfg_table(flows[0][0], flows[0][1], xb, t)
    assert torch.equal(xb, keep) and int(b._counter.item()) == 50
    # ... and a rewind replays the same trajectory bit-identically
    b.reset_step_table(t)
    xb = x0.clone()
    assert int(b._counter.item()) == 0 and float(t[0]) == float(b.timesteps[0])
    for fc, fu in flows:
        b.step_cfg_table(fc, fu, xb, t)
    assert torch.equal(xa, xb)
