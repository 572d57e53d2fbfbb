"""Host side of the exact tests of the float32 latent chain (csrc/sampler.hip through mmpl_cfg_unipc_step_f32 /
mmpl_cfg_dpmpp_step_f32 and their _table forms): the two kernels restated per element in torch float32 operations, one torch
operation per IEEE operation of the kernel, in the kernel's order (the formulas at the entries in include/mmpl_hip.h), and the
operands the GPU test launches on.

torch's float32 element-wise add / sub / mul / div on the CPU are single IEEE operations (nothing is fused in eager mode), the
kernel is compiled with contract(off) and plain operators, and bf16 rounding is round-to-nearest-even on both sides: for finite,
normal values the kernel equals the restatement in every bit.  tests/test_fp32_chain_host.py ties the restatement, driven by the
float32 scalars of mmpl_amd/scheduler.py, to the REAL reference's schedulers (tests/golden/fp32_chain.pt, bit for bit on every
step).
"""
import torch

F32 = torch.float32
BF = torch.bfloat16
SIZES = (1, 3, 255, 256, 257, 4099, 18432)           # 18432 = one 3-frame clip of the tiny geometry (3 x 16 x 16 x 24)


def _s(v):
    return torch.tensor(float(v), dtype=F32)


def cfg_flow(fc, fu, guidance):
    """f = fu + g * (fc - fu) on the widened bf16 flows (fc when fu is None)."""
    fc = fc.to(F32)
    if fu is None:
        return fc
    fu = fu.to(F32)
    return fu + _s(guidance) * (fc - fu)


def unipc_f32(st, fc, fu, x, m0, m1, last, mutation=None):
    """the float32 UniPC solver of csrc/sampler.hip (st: any object with MmplUniPCStepF32's fields; the state BEFORE the step).
    -> (x, m0, m1, last) after the step, float32.  `mutation` = a plausible wrong kernel: 'inv_rk' multiplies by 1 / rk where the
    reference divides (the bf16 kernel's struct), 'bf16_rho' rounds the rhos to bf16 (`rhos_c.to(x.dtype)` of a bf16 sample)."""
    div = (lambda a, rk: a * (_s(1.0) / _s(rk))) if mutation == "inv_rk" else (lambda a, rk: a / _s(rk))
    rho = (lambda v: _s(v).to(BF).to(F32)) if mutation == "bf16_rho" else _s
    f = cfg_flow(fc, fu, st.guidance)
    mc = x - _s(st.sigma_cur) * f
    if st.use_corrector:
        xt_ = _s(st.c_c1) * last - _s(st.c_c2) * m0
        d1t = mc - m0
        corr = torch.zeros_like(x)
        if st.corr_order == 2:
            corr = rho(st.c_rho0) * div(m1 - m0, st.c_rk)
        acc = corr + rho(st.c_rho_last) * d1t
        x = xt_ - _s(st.c_c3) * acc
    m1, m0, last = m0, mc, x
    xt_ = _s(st.p_c1) * x - _s(st.p_c2) * m0
    pr = torch.zeros_like(x)
    if st.pred_order == 2:
        pr = _s(0.5) * div(m1 - m0, st.p_rk)
    return xt_ - _s(st.p_c3) * pr, m0, m1, last


def dpmpp_f32(st, fc, fu, x, m0, m1):
    """the float32 DPM-Solver++ solver of csrc/sampler.hip (st: MmplDpmppStep's fields; m1's values are not read: the rotation overwrites it).
    -> (x, m0, m1) after the step, float32."""
    f = cfg_flow(fc, fu, st.guidance)
    mc = x - _s(st.sigma_cur) * f
    m1, m0 = m0, mc
    acc = _s(st.c1) * x - _s(st.c2) * m0
    if st.order == 2:
        d1 = _s(st.inv_r0) * (m0 - m1)
        acc = acc - (_s(0.5) * _s(st.c2)) * d1
    return acc, m0, m1


def normal_range(n, seed):
    """n float32 values of either sign with |v| in [2^-20, 2^20] and full mantissas, so that a contracted FMA, a reciprocal multiply
    or a reordered sum shows in the last bit."""
    g = torch.Generator().manual_seed(seed)
    mant = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    expo = torch.randint(-20, 20, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (sign * mant * torch.exp2(expo)).to(F32)


def operands(n, seed=0):
    """flow_cond, flow_uncond (bf16), x, m0, m1, last (float32), all normal-range."""
    base = 9100 + 10 * seed + n % 1000
    flows = [normal_range(n, base + i).to(BF) for i in range(2)]
    return flows + [normal_range(n, base + 2 + i) for i in range(4)]
