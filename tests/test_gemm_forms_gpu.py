"""The GEMM (csrc/gemm.hip) one launch at a time, in the forms the DiT forward, T5, CLIP and the VAE launch it, bit for bit (-m gpu).

Every case of tests/gemm_ref.py's table calls mmpl_gemm_ex and asserts
  - the plan the launcher took (kernel, tail, epilogue form, block counts, split-K parts), as mmpl_gemm_ex reports it from
    mmpl_gemm_plan, against the path the case names AND against the tile arithmetic restated in gemm_ref.plan_restated for the CUs
    per XCD this device has (read from the plan's own persistent block count where there is one, else from the device properties);
  - for the epilogues 0, 3, 4, 5, 6: C's whole buffer ([M + 3, ldc] and more, pre-filled with a NaN pattern, the residual inside the
    window where res is C) and the pages' whole buffer equal to the float64 reference's IN EVERY BIT -- zero mismatches, canaries
    included; the inputs keep the accumulator and every intermediate exact (tests/test_gemm_ref.py), so there is nothing to tolerate;
  - for GELU / SiLU: tests/test_kernels_gpu.py::test_gemm's criteria against the fp32 activation of the exact pre-activation
    (gemm_ref.activation: the form that does not cancel in the far negative tail these inputs reach), and the canaries bit for bit;
  - the scratch header (tile tickets, split-K counters) zero after each of two runs on the same scratch, whose partial area is filled
    with 0xFF before each.
"""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as R
from tests.util import bf16_ulp_frac, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scratch(lib):
    nb = lib.mmpl_gemm_scratch_bytes()
    return torch.zeros(nb, dtype=torch.uint8, device=DEV), nb


_acc_cache = {}


def _operands_and_acc(c):
    """Device operands and their float64 accumulator, computed once per shape and shared by its epilogues."""
    if c.input_key not in _acc_cache:
        _acc_cache.clear()
        a, w = (t.to(DEV) for t in R.operands(c.input_key))
        _acc_cache[c.input_key] = (a, w, R.accumulate(c, a, w))
    return _acc_cache[c.input_key]


def _mismatches(got, want):
    return int((R.bits(got) != R.bits(want)).sum())


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_gemm_form(lib, scratch, c):
    from mmpl_amd import _lib
    a, w, acc = _operands_and_acc(c)
    bias, gate, res = (None if t is None else t.to(DEV) for t in R.epilogue_inputs(c))
    want = R.expected(c, acc, bias, gate, res)
    assert want.ambiguous == 0
    sbuf, sbytes = scratch
    tickets = torch.zeros(8, dtype=torch.int32, device=DEV) if c.tickets else None
    esz = 4 if c.epi == R.EPI_F32_SCALE else 2
    per_dev = torch.cuda.get_device_properties(0).multi_processor_count // 8

    for run in range(2):
        cb, vb = R.initial_buffers(c, res, DEV)
        c_ptr = cb.data_ptr() + esz * c.c_off
        if c.epi in (R.EPI_GATE_RES, R.EPI_RES):
            res_ptr, ldres = (c_ptr, c.LDC) if c.inplace else (res.data_ptr(), c.N)
        else:
            res_ptr, ldres = 0, 0
        gate_ptr = gate.data_ptr() + 2 * R.gate_off(c) if gate is not None else 0
        pages, n_pages = None, 0
        if vb is not None:
            off, _, _ = R.page_layout(c)
            n_pages = c.n_frames
            pages = (C.c_void_p * n_pages)(*[vb.data_ptr() + 2 * o for o in off])
        if c.scratch:
            sbuf[2048:] = 0xFF
        plan = (C.c_int * 6)(*([-1] * 6))
        _lib.check(lib.mmpl_gemm_ex(_lib.ptr(a), c.LDA, _lib.ptr(w), c.LDW, _lib.ptr(bias), C.c_void_p(c_ptr), c.LDC, c.M, c.N, c.K, c.epi,
                                    C.c_void_p(res_ptr), ldres, C.c_void_p(gate_ptr), c.GATE_STRIDE if gate is not None else 0, c.rpf,
                                    c.alpha, c.batch, c.sA, c.sW, c.sC, pages, n_pages, c.v_col0, c.V_LD if vb is not None else 0,
                                    _lib.ptr(sbuf) if c.scratch else None, sbytes if c.scratch else 0, _lib.ptr(tickets), plan,
                                    _lib.stream_ptr()), c.name)
        torch.cuda.synchronize()
        plan = list(plan)
        print(f"{c.name} run {run}: plan {plan}")

        # ---- the path: what the case names, and the restated tile arithmetic at this device's CUs per XCD
        per = plan[3] // 8 if c.main == "percu" else per_dev
        assert per == per_dev and (c.main != "percu" or plan[3] == 8 * per_dev), (plan, per_dev)
        assert plan[:3] == [c.kernel, c.tail, c.staged] and plan[5] == c.splitk_s, (plan, "the shape no longer reaches the path it is here for")
        assert {"none": plan[3] == 0, "percu": plan[3] == 8 * per, "tiles": plan[3] > 0 and plan[4] == 0}[c.main], plan
        assert plan == R.plan_restated(c, per), (plan, R.plan_restated(c, per))

        # ---- tickets and counters are left zero
        if c.scratch:
            assert int(sbuf[:2048].to(torch.int32).sum()) == 0
        if tickets is not None:
            assert int(tickets.abs().sum()) == 0

        # ---- the output
        if c.epi in R.EXACT_EPIS:
            bad = _mismatches(cb, want.c_buf)
            print(f"{c.name} run {run}: {bad} mismatching elements of C's buffer")
            assert bad == 0, (bad, int((R.bits(cb) != R.bits(want.c_buf))[~want.c_written].sum()), "of them outside the window")
        else:
            got, ref = R.c_view(c, cb), R.c_view(c, want.c_buf)
            r, u = rel_l2(got, ref), bf16_ulp_frac(got, ref, 2)
            print(f"{c.name} run {run}: rel_l2 {r:.3e}, fraction beyond 2 bf16 ulp {u:.3e}")
            assert r < 2e-3 and u < 2e-3, (r, u)
            assert _mismatches(cb[~want.c_written], want.c_buf[~want.c_written]) == 0
        if vb is not None:
            bad = _mismatches(vb, want.v_buf)
            print(f"{c.name} run {run}: {bad} mismatching elements of the pages' buffer")
            assert bad == 0, (bad, int((R.bits(vb) != R.bits(want.v_buf))[~want.v_written].sum()), "of them outside the pages")
