"""The attention kernels one launch at a time on exact inputs (-m gpu): attn_w64_kernel (FAST and GENERAL passes, history, split-KV
tail and merge, merged pages), attn_fwd_kernel, attn_cross_kernel<1 | 2> and attn_merge_kernel through mmpl_attn_fwd_ex.

Every case of tests/attn_ref.py's table makes one launch and asserts
  - the plan the launcher took (kernel, pages after the merge, KV tiles, blocks, split parts, the cross kernel's block shape), as
    mmpl_attn_fwd_ex reports it from mmpl_attn_plan, against the path the case names AND against attn_ref.plan_restated at this
    device's CUs per XCD; for attn_w64_kernel the counters (blocks redone by the GENERAL pass, blocks whose FAST pass held on
    remembered references) the case names -- where it names none, what attn_ref.predict_redone derives from the scores: zero, except
    for the parts of a split tail block in which a probe row's target is missing;
  - ZERO elements outside their candidates bf16_rne(x (1 -+ eps)) of the float64 reference x (attn_ref's docstring derives eps;
    tests/test_attn_ref.py proves on the CPU that the inputs leave nothing else to tolerate);
  - o's whole buffer ([Lq + 3, ldo], pre-filled with a NaN pattern) untouched outside the window, bit for bit, and the K / V / q
    buffers (pages cut from one allocation with non-finite canary rows behind each) unchanged;
  - the same on a second launch (with a history: the second launch of the sequence).
"""
import ctypes as C

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WRONG_PATH = "the shape no longer reaches the path it is here for"


def _per():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8


def _ws_bytes():
    from mmpl_amd import _lib
    return _lib.load().mmpl_attn_workspace_bytes()


_ref_cache = {}


def _setup(c):
    """Device buffers and the float64 reference of a case, computed once and left unchanged (shared by the launches of the case and by
    the cases that share its operands and plan)."""
    key = (c.operand_key, c.copies, c.layout, c.split_groups, c.workspace, c.w64, c.kpad, c.ldq_mult, c.cdiv)
    if key not in _ref_cache:
        _ref_cache.clear()
        q, K, V, _ = R.case_operands(c)
        qd, Kd, Vd = q.to(DEV), K.to(DEV), V.to(DEV)
        x, A = R.reference(c, qd, Kd, Vd, plan=R.plan_restated(c, _per(), _ws_bytes()), per=_per())
        kb, vb = R.kv_buffers(c, Kd, Vd, DEV)
        redone = R.predict_redone(c, qd, Kd, R.plan_restated(c, _per(), _ws_bytes()), _per()) if c.w64 and not c.stats else 0
        _ref_cache[key] = (R.q_buffer(c, qd, DEV), kb, vb, x, A, redone)
    return _ref_cache[key]


def _launch(lib, c, qb, kb, vb, ws, hist, stats):
    from mmpl_amd import _lib
    lay = R.layout(c)
    kp = (C.c_void_p * c.n_pages)(*[kb[r0:].data_ptr() for r0 in lay.page_row0])
    vp = (C.c_void_p * c.n_pages)(*[vb[r0:].data_ptr() for r0 in lay.page_row0])
    groups = (C.c_ubyte * c.n_pages)(*lay.groups)
    o = R.o_buffer(c, DEV)
    plan = (C.c_int * 8)(*([-1] * 8))
    if stats is not None:
        stats.zero_()
    _lib.check(lib.mmpl_attn_fwd_ex(_lib.ptr(qb), c.ldq, _lib.ptr(o), c.ldo, kp, vp, groups, c.ldk, c.ldk, c.n_pages, c.page_rows, c.Lq,
                                    c.H, c.scale, _lib.ptr(ws), 0 if ws is None else ws.numel(), c.variant, 0, c.cross, c.copies,
                                    _lib.ptr(hist), _lib.ptr(stats), plan, _lib.stream_ptr()), c.name)
    torch.cuda.synchronize()
    return o, list(plan), None if stats is None else [int(v) for v in stats.cpu()]


def _run_case(lib, c):
    qb, kb, vb, x, A, predicted = _setup(c)
    snap = [R.bits(t).clone() for t in (qb, kb, vb)]
    per = _per()
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=DEV).fill_(0xFF) if c.workspace else None
    hist = torch.zeros(lib.mmpl_attn_history_bytes(c.Lq, c.H), dtype=torch.uint8, device=DEV) if c.history else None
    stats = torch.zeros(5, dtype=torch.int64, device=DEV) if c.w64 else None
    want_plan = R.plan_restated(c, per, lib.mmpl_attn_workspace_bytes())
    outs = []
    for run in range(2):
        o, plan, st = _launch(lib, c, qb, kb, vb, ws, hist, stats)
        print(f"{c.name} run {run}: plan {plan} stats {st}")
        assert plan[0] == c.kernel and plan[1] == (c.pages_walked or c.n_pages) and (plan[5] > 1) == c.split, (plan, WRONG_PATH)
        assert plan == want_plan, (plan, want_plan, WRONG_PATH)
        if st is not None:
            redone, held = c.stats[run] if c.stats else (predicted, 0)
            assert st[1] == redone and st[4] == held and st[3] == 0, (st, WRONG_PATH)
            assert st[0] == c.n_qb * c.H + (plan[5] - 1) * _tail_blocks(c, per, plan), st
        win = o[:c.Lq, :c.d]
        delta = R.eps(c, plan[5]) * A
        bad = R.outside(win, x, delta)
        amb = float(R.ambiguous(x, delta).double().mean())
        n_bad = int(bad.sum())
        need = R.needed_eps(win, x, A) if (c.copies > 1 or n_bad) else None
        print(f"{c.name} run {run}: {n_bad} of {bad.numel()} elements outside their candidates, {amb:.4%} ambiguous, eps {R.eps(c, plan[5]) / R.U:.1f} u"
              + (f", needed {need / R.U:.1f} u" if need is not None else ""))
        assert n_bad == 0, (n_bad, bad.nonzero()[:8].tolist(), win[bad][:8].tolist(), x[bad][:8].tolist())
        assert amb <= R.AMBIGUITY_CAP
        # ---- nothing outside the window was written, nothing that was read changed
        mask = torch.ones_like(o, dtype=torch.bool)
        mask[:c.Lq, :c.d] = False
        assert int((R.bits(o)[mask] != R.CANARY_BF16).sum()) == 0
        for t, s0 in zip((qb, kb, vb), snap):
            assert torch.equal(R.bits(t), s0)
        outs.append(o)
    return outs


def _tail_blocks(c, per, plan):
    return len(R.tail_items(c, per, plan[4])) if plan[5] > 1 else 0


@pytest.mark.parametrize("c", R.CASES, ids=[c.name for c in R.CASES])
def test_attn_exact(lib, c):
    _run_case(lib, c)


@pytest.mark.parametrize("variant", [3, 4])
def test_merged_pages_equal_unmerged_bit_for_bit(lib, variant):
    """4 + 5 pages of two allocations: merged into two long pages (other tile boundaries, other order) the kernel returns the bits it
    returns for the same keys presented as nine pages -- the exact inputs leave the summation order nothing to change."""
    by_name = {c.name: c for c in R.CASES}
    merged = _run_case(lib, by_name[f"kv-4+5x40-groups-v{variant}"])[0]
    apart = _run_case(lib, by_name[f"kv-4+5x40-unmerged-v{variant}"])[0]
    assert torch.equal(R.bits(merged), R.bits(apart))
