"""Host side of the exact tests of the bf16 DPM-Solver++ step (csrc/sampler.hip, through mmpl_cfg_dpmpp_step / _table): the
kernel's chain restated in numpy float32 and the operands the GPU test launches on.

Every operation of the chain is ONE IEEE fp32 operation (numpy float32 arithmetic is IEEE, the kernel is compiled with
contract(off) and uses no approximate instruction) and bf16 rounding is round-to-nearest-even on both sides, so for finite,
normal inputs the kernel equals `dpmpp_chain` in every bit of x, m0 and m1: there is nothing to tolerate.
tests/test_dpmpp_host.py ties `dpmpp_chain` to the REAL reference (tests/golden/dpmpp_sched.pt: its trajectory under the scalar
semantics of its native platform, bit for bit on every step) and shows that each named mutation -- a plausible wrong kernel --
changes at least one output element on these operands; the GPU test asserts that the kernel equals the chain and none of the mutants.

    scalar_rounded   the scalars sigma_cur, c2, inv_r0 and 0.5 c2 rounded to bf16 before their products: PyTorch's CPU semantics
    d1_unrounded     (m0 - m1) not rounded to bf16 before the product with inv_r0
    m_swapped        D1 from (m1 - m0)
"""
import numpy as np

from tests.rowpass_ref import F32, bf2f, bf16_from_f32, rbf, to_bf16

STEPS_50 = (0, 1, 2, 25, 49)                         # of the 50-step, shift-5 schedule at guidance 5
STEPS_10 = (8, 9)                                    # of the 10-step, shift-5 schedule
ORDERS = {(50, 0): 1, (50, 1): 2, (50, 2): 2, (50, 25): 2, (50, 49): 1, (10, 8): 2, (10, 9): 1}
SIZES = (1, 255, 8192 * 256 + 257)                   # 2 097 409: a lone element-wise tail, a tail behind 31 vectors, 1025 blocks + a tail
STRIDE_SIZE = 8192 * 256 * 8 + 2051                  # the grid is capped at 8192 blocks x 256 lanes x 8 elements: 2051 elements into the loop's second round
STRIDE_PERIOD = 1_000_003                            # the chain is element-wise: at STRIDE_SIZE the operands are this many values, tiled (a prime: no stride
                                                     # of the kernel is a multiple of it, so an element taken from the wrong place shows)
MUTATIONS = ("scalar_rounded", "d1_unrounded", "m_swapped")
FIELDS = ("guidance", "sigma_cur", "order", "c1", "c2", "inv_r0")
MUTANT_SLICE = 4096                                  # the chain is element-wise: the mutants are evaluated on the first elements only
MUTANT_SIZES = SIZES[1:]                             # one element cannot show every rounding: the mutants are held at the other sizes


def bites(mutation, st):
    """True: the mutant must change an output element among the first min(n, MUTANT_SLICE) operands of every size in MUTANT_SIZES
    (tests/test_dpmpp_host.py proves it does, the GPU test then asserts the kernel differs from it); False: it cannot; None: it may
    (scalar_rounded at step 0: sigma_cur = 1 is exact in bf16 and c2's rounding moves a term 250 times smaller than the sample)."""
    if mutation == "scalar_rounded":
        return True if st.sigma_cur != 1.0 else None
    return st.order == 2 and st.inv_r0 != 0.0        # step 1's D1 is +-0 whatever the difference is


def operands(n, seed=0):
    """five bf16 tensors of N(0, 1): flow_cond, flow_uncond, x, m0, m1."""
    rng = np.random.default_rng(7300 + seed + n % 1000)
    return [to_bf16(rng.normal(0, 1, n)) for _ in range(5)]


def dpmpp_chain(st, fc, fu, x, m0, m1, mutation=None):
    """the bf16 DPM-Solver++ solver of csrc/sampler.hip in numpy float32 (st: any object with MmplDpmppStep's fields; fu None = fc is the combined flow;
    m0, m1: the history BEFORE the step; m1's values are not read: the rotation overwrites it).
    -> ([x, m0, m1] after the step as bf16 bits, the list of every fp32 intermediate that is rounded)."""
    q = (lambda v: rbf(F32(v))) if mutation == "scalar_rounded" else F32
    mids = []

    def r(v):
        mids.append(v)
        return rbf(v)

    f, x, m0_old = bf2f(fc), bf2f(x), bf2f(m0)
    if fu is not None:
        u = bf2f(fu)
        f = r(u + r(F32(st.guidance) * r(f - u)))
    m0 = r(x - r(q(st.sigma_cur) * f))
    m1 = m0_old
    acc = F32(st.c1) * x - r(q(st.c2) * m0)
    if st.order == 2:
        diff = (m1 - m0) if mutation == "m_swapped" else (m0 - m1)
        if mutation != "d1_unrounded":
            diff = r(diff)
        d1 = r(q(st.inv_r0) * diff)
        acc = acc - r(q(F32(0.5) * F32(st.c2)) * d1)
    mids.append(acc)
    return [bf16_from_f32(v) for v in (acc, m0, m1)], mids


def differs(a, b):
    """number of elements in which two lists of bf16 bit arrays differ, per array."""
    return [int((np.asarray(p) != np.asarray(q)).sum()) for p, q in zip(a, b)]
