"""The grouped launch of attn_w64_kernel (mmpl_attn_fwd_groups_ex): n_groups self-attentions of equal shape in ONE launch, each
group's query rows seeing its own pages only -- what a batched few-step forward needs of the self-attention.

One grouped call on poisoned buffers against G calls of mmpl_attn_fwd_ex (variant 0, q_prescaled) on the same memory, bit for bit:
block for block the grouped launch does what the single launches do (same pages after each group's own merge, same tiles, same
order), so with no split-KV tail on either side nothing is left to tolerate.  Every group of a call has its own page list -- one page,
three back-to-back pages that merge into one, two pages that do not touch -- cut from one cache allocation whose other slots, like
the rows of o outside the groups and its columns >= 128 H, hold a canary that must survive.  The shape whose grouped plan splits its tail
round is judged on tests/attn_ref.py's exact inputs against its float64 result by its own criterion.  The rejections that need no
device (made-up pointers, as tests/test_kernel_entry_errors.py) carry no gpu mark.
"""
import ctypes as C
import dataclasses
import math

import pytest
import torch

from tests import attn_ref as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLOTS_PER_GROUP = 5
LISTS = ((0,), (1, 2, 3), (0, 2), (4,), (2, 3, 4))      # slots of a group's own 5: one page; three that merge; two apart; ...


def _lists(G):
    """per group: the cache slots it attends to (global indices)"""
    return [[g * SLOTS_PER_GROUP + i for i in LISTS[g % len(LISTS)]] for g in range(G)]


def _pages(cache, lists, S):
    flat = [s for l in lists for s in l]
    return (C.c_void_p * len(flat))(*[cache[s * S:].data_ptr() for s in flat]), (C.c_int * len(lists))(*[len(l) for l in lists])


def _merged(l):
    return 1 + sum(1 for a, b in zip(sorted(l), sorted(l)[1:]) if b != a + 1)


class Shape:
    def __init__(self, G, rows, H, lists=None, seed=0):
        self.G, self.rows, self.H = G, rows, H
        self.S = 96 if rows < 1560 else 520                         # both end in a ragged 64-row tile
        self.d = 128 * H
        self.ldq, self.ldo, self.ldk = 3 * self.d, self.d + 8, self.d
        self.lists = lists or _lists(G)
        self.scale = 1.0 / math.sqrt(128.0)
        g = torch.Generator(device=DEV).manual_seed(1000 * G + rows + H + seed)
        n_slots = G * SLOTS_PER_GROUP
        self.q = R.canary((G * rows + 3) * self.ldq, DEV).view(-1, self.ldq)
        self.q[:G * rows, :self.d] = (torch.randn(G * rows, self.d, generator=g, device=DEV) * (self.scale * 1.4426950408889634)).to(BF)
        self.k = torch.randn(n_slots * self.S, self.d, generator=g, device=DEV).to(BF)
        self.v = torch.randn(n_slots * self.S, self.d, generator=g, device=DEV).to(BF)
        used = {s for l in self.lists for s in l}
        for s in range(n_slots):                                    # slots no group attends to: read by nobody
            if s not in used:
                self.k[s * self.S:(s + 1) * self.S] = R.K_CANARY
                R.bits(self.v)[s * self.S:(s + 1) * self.S] = R.CANARY_BF16

    def o_buffer(self):
        return R.canary((self.G * self.rows + 3) * self.ldo, DEV).view(-1, self.ldo)

    def grouped(self, lib, ws=None, hist=None, stats=None, variant=0):
        from mmpl_amd import _lib
        o = self.o_buffer()
        kp, n_each = _pages(self.k, self.lists, self.S)
        vp, _ = _pages(self.v, self.lists, self.S)
        plan = (C.c_int * 10)(*([-1] * 10))
        _lib.check(lib.mmpl_attn_fwd_groups_ex(_lib.ptr(self.q), self.ldq, _lib.ptr(o), self.ldo, kp, vp, None, n_each, self.G, self.rows,
                                               self.ldk, self.ldk, self.S, self.H, self.scale, _lib.ptr(ws), 0 if ws is None else ws.numel(),
                                               variant, 1, _lib.ptr(hist), _lib.ptr(stats), plan, _lib.stream_ptr()), "grouped")
        torch.cuda.synchronize()
        return o, list(plan)

    def one_by_one(self, lib, ws=None):
        """G launches of mmpl_attn_fwd_ex into one poisoned o, each on its group's rows"""
        from mmpl_amd import _lib
        o = self.o_buffer()
        plans = []
        for g, l in enumerate(self.lists):
            kp, _ = _pages(self.k, [l], self.S)
            vp, _ = _pages(self.v, [l], self.S)
            plan = (C.c_int * 8)(*([-1] * 8))
            _lib.check(lib.mmpl_attn_fwd_ex(_lib.ptr(self.q[g * self.rows:]), self.ldq, _lib.ptr(o[g * self.rows:]), self.ldo, kp, vp, None,
                                            self.ldk, self.ldk, len(l), self.S, self.rows, self.H, self.scale, _lib.ptr(ws),
                                            0 if ws is None else ws.numel(), 0, 1, 0, 0, None, None, plan, _lib.stream_ptr()), f"group {g}")
            plans.append(list(plan))
        torch.cuda.synchronize()
        return o, plans


def _assert_same(sh, o, want):
    assert torch.equal(R.bits(o), R.bits(want)), [int((R.bits(o[g * sh.rows:(g + 1) * sh.rows]) != R.bits(want[g * sh.rows:(g + 1) * sh.rows])).sum())
                                                  for g in range(sh.G)]
    mask = torch.ones_like(o, dtype=torch.bool)
    mask[:sh.G * sh.rows, :sh.d] = False
    assert int((R.bits(o)[mask] != R.CANARY_BF16).sum()) == 0                   # rows outside every group, columns >= 128 H
    assert not bool(torch.isnan(o[:sh.G * sh.rows, :sh.d].float()).any())       # ... and every row of every group was written


@gpu
@pytest.mark.parametrize("H", [1, 3, 8, 12])
@pytest.mark.parametrize("rows", [96, 288, 512, 1560])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_grouped_equals_one_launch_per_group(lib, G, rows, H):
    sh = Shape(G, rows, H)
    snap = [R.bits(t).clone() for t in (sh.q, sh.k, sh.v)]
    stats = torch.zeros(5, dtype=torch.int64, device=DEV)
    o, plan = sh.grouped(lib, stats=stats)
    want, plans = sh.one_by_one(lib)
    n_qb = -(-rows // 256)
    print(f"G {G} rows {rows} H {H}: grouped plan {plan}, single plans {plans}")
    assert plan[0] == R.W64 and plan[8] == 1 and plan[9] == G * H * n_qb, plan
    assert plan[1] == sum(_merged(l) for l in sh.lists) and plan[5] == 1 and plan[4] == 0, plan
    assert plan[2] == max(p[2] for p in plans)
    assert all(p[0] == R.W64 and p[5] == 1 and p[1] == _merged(l) for p, l in zip(plans, sh.lists)), plans
    assert int(stats[0]) == G * H * n_qb                                        # one block per (group, head, query block)
    _assert_same(sh, o, want)
    for t, s0 in zip((sh.q, sh.k, sh.v), snap):
        assert torch.equal(R.bits(t), s0)


@gpu
def test_history_takes_one_launch_per_group(lib):
    sh = Shape(3, 288, 3)
    hist = torch.zeros(3 * lib.mmpl_attn_history_bytes(sh.rows, sh.H), dtype=torch.uint8, device=DEV)
    o, plan = sh.grouped(lib, hist=hist)
    want, plans = sh.one_by_one(lib)
    assert plan[8] == 0 and plan[:8] == plans[0], (plan, plans)
    _assert_same(sh, o, want)                        # an all-zero history is the stateless kernel, bit for bit


@gpu
def test_25_merged_pages_take_one_launch_per_group(lib):
    lists = [[g * SLOTS_PER_GROUP + i for i in (0, 2, 4)] for g in range(8)]
    lists[7] = lists[7] + [1]            # (groups may share slots: group 7 also reads one of group 0's five) -- 8 x 3 + 1 pages, no two adjacent
    sh = Shape(8, 96, 3, lists=lists)
    o, plan = sh.grouped(lib)
    want, _ = sh.one_by_one(lib)
    assert plan[8] == 0 and plan[9] == 8 * 3, plan
    _assert_same(sh, o, want)
    lists24 = lists[:7] + [lists[7][:3]]                             # one page fewer: 24 still go as one launch
    sh = Shape(8, 96, 3, lists=lists24)
    o, plan = sh.grouped(lib)
    assert plan[8] == 1 and plan[1] == 24, plan
    _assert_same(sh, o, sh.one_by_one(lib)[0])


@gpu
def test_lockstep_variant_takes_one_launch_per_group(lib):
    """the lock-step kernel (what MMPL_ATTN_V1 makes of every self-attention) has no grouped form: raw q, variant 1"""
    from mmpl_amd import _lib
    sh = Shape(2, 288, 3)
    o = sh.o_buffer()
    kp, n_each = _pages(sh.k, sh.lists, sh.S)
    vp, _ = _pages(sh.v, sh.lists, sh.S)
    plan = (C.c_int * 10)(*([-1] * 10))
    _lib.check(lib.mmpl_attn_fwd_groups_ex(_lib.ptr(sh.q), sh.ldq, _lib.ptr(o), sh.ldo, kp, vp, None, n_each, sh.G, sh.rows, sh.ldk, sh.ldk,
                                           sh.S, sh.H, sh.scale, None, 0, 1, 0, None, None, plan, _lib.stream_ptr()), "lock-step")
    want = sh.o_buffer()
    for g, l in enumerate(sh.lists):
        kp1, _ = _pages(sh.k, [l], sh.S)
        vp1, _ = _pages(sh.v, [l], sh.S)
        _lib.check(lib.mmpl_attn_fwd_ex(_lib.ptr(sh.q[g * sh.rows:]), sh.ldq, _lib.ptr(want[g * sh.rows:]), sh.ldo, kp1, vp1, None, sh.ldk,
                                        sh.ldk, len(l), sh.S, sh.rows, sh.H, sh.scale, None, 0, 1, 0, 0, 0, None, None, None,
                                        _lib.stream_ptr()), f"group {g}")
    torch.cuda.synchronize()
    assert list(plan)[0] == R.LOCKSTEP and list(plan)[8] == 0, list(plan)
    _assert_same(sh, o, want)


@gpu
def test_grouped_split_tail_on_exact_inputs(lib):
    """2 groups x 8 heads x 21 query blocks: 42 work items per XCD, whose last round of 10 (at 32 CUs per XCD) runs in 3 KV parts and is
    merged by attn_merge_groups_kernel.  Inputs, float64 reference and criterion are tests/attn_ref.py's; the two groups take the
    operands of the variant-4 and the variant-3 case of one shape (c = 1: a raw q is the prescaled one)."""
    from mmpl_amd import _lib
    G, per = 2, torch.cuda.get_device_properties(0).multi_processor_count // 8
    cs = [R.Case(f"grouped-split-g{g}", v, 3, 520, Lq=256 * 20 + 1, H=8, workspace=True) for g, v in enumerate((4, 3))]
    c = cs[0]
    ops = []
    for cg in cs:
        q, K, V, _ = R.case_operands(cg)
        ops.append((q.to(DEV), K.to(DEV), V.to(DEV)))
    qb = R.canary((G * c.Lq + 3) * c.ldq, DEV).view(-1, c.ldq)
    for g in range(G):
        qb[g * c.Lq:(g + 1) * c.Lq, :c.d] = ops[g][0]
    kvb = [R.kv_buffers(cg, K, V, DEV) for cg, (_, K, V) in zip(cs, ops)]
    lay = R.layout(c)
    kp = (C.c_void_p * (G * c.n_pages))(*[kvb[g][0][r0:].data_ptr() for g in range(G) for r0 in lay.page_row0])
    vp = (C.c_void_p * (G * c.n_pages))(*[kvb[g][1][r0:].data_ptr() for g in range(G) for r0 in lay.page_row0])
    n_each = (C.c_int * G)(*([c.n_pages] * G))
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=DEV).fill_(0xFF)
    o = R.canary((G * c.Lq + 3) * c.ldo, DEV).view(-1, c.ldo)
    plan = (C.c_int * 10)(*([-1] * 10))
    _lib.check(lib.mmpl_attn_fwd_groups_ex(_lib.ptr(qb), c.ldq, _lib.ptr(o), c.ldo, kp, vp, None, n_each, G, c.Lq, c.ldk, c.ldk, c.page_rows,
                                           c.H, c.scale, _lib.ptr(ws), ws.numel(), 4, 0, None, None, plan, _lib.stream_ptr()), "split")
    torch.cuda.synchronize()
    plan = list(plan)
    cv = dataclasses.replace(c, H=G * c.H)                       # the virtual heads' case: its plan and tail items are the grouped launch's
    want_plan = R.plan_restated(cv, per, ws.numel())
    print(f"grouped split: plan {plan}, restated {want_plan}")
    assert plan[:8] == want_plan[:1] + [G * want_plan[1]] + want_plan[2:], (plan, want_plan)
    assert plan[8] == 1 and plan[9] == G * c.H * c.n_qb
    if per == 32:
        assert plan[5] == 3 and plan[4] == 10, (plan, "the shape no longer reaches the path it is here for")
    sp = plan[5]
    tails = {}
    for hv, qblk in (R.tail_items(cv, per, plan[4]) if sp > 1 else []):
        tails.setdefault(hv, []).append(qblk)
    parts = R.split_parts(c, sp) if sp > 1 else None
    n_split = 0
    for g in range(G):
        q, K, V = ops[g]
        w = R.key_weights(cs[g], DEV)
        x = torch.empty(c.Lq, c.d, dtype=torch.float64, device=DEV)
        A = torch.empty_like(x)
        split_rows = torch.zeros(c.Lq, dtype=torch.bool, device=DEV)
        for h in range(c.H):                                     # (R.reference's loop, with the grouped launch's tail items)
            s = R.scores(cs[g], q, K, h)
            Vh = V[:, h * R.HD:(h + 1) * R.HD]
            xh, Ah = R.softmax_ref(cs[g], s, Vh, w)
            for qblk in tails.get(g * c.H + h, []):
                r = slice(qblk * R.QB, min((qblk + 1) * R.QB, c.Lq))
                _, Ah[r] = R.softmax_ref(cs[g], s[r], Vh, w, parts)
                split_rows[r] = True
            x[:, h * R.HD:(h + 1) * R.HD], A[:, h * R.HD:(h + 1) * R.HD] = xh, Ah
        win = o[g * c.Lq:(g + 1) * c.Lq, :c.d]
        delta = R.eps(c, sp) * A                                 # the criterion of tests/test_attn_exact_gpu.py for a case that splits
        bad = R.outside(win, x, delta)
        amb = float(R.ambiguous(x, delta).double().mean())
        print(f"group {g}: {int(bad.sum())} of {bad.numel()} elements outside their candidates, {amb:.4%} ambiguous, "
              f"{int(split_rows.sum())} rows in split blocks")
        assert int(bad.sum()) == 0, (g, bad.nonzero()[:8].tolist())
        assert amb <= R.AMBIGUITY_CAP
        n_split += int(split_rows.sum())
    assert (n_split > 0) == (sp > 1)            # (at 32 CUs per XCD: query blocks 11 .. 20 of every head of group 1)
    mask = torch.ones_like(o, dtype=torch.bool)
    mask[:G * c.Lq, :c.d] = False
    assert int((R.bits(o)[mask] != R.CANARY_BF16).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- rejections (no GPU)
P = 0x100000                       # a made-up 16-byte aligned "device pointer" that nothing dereferences


def _call(**kw):
    from mmpl_amd import _lib
    pages = (C.c_void_p * 4)(*[P + 0x10000 * i for i in range(4)])
    a = dict(q=P, ldq=256, o=P, ldo=256, k_pages=pages, v_pages=pages, page_group=None, group_n_pages=(C.c_int * 2)(3, 1), n_groups=2,
             group_rows=300, ldk=256, ldv=256, page_rows=72, num_heads=2, softmax_scale=0.6931472, workspace=None, workspace_bytes=0,
             variant=4, q_prescaled=0, history=None, stats_dev=None)
    a.update(kw)
    plan = (C.c_int * 10)(*([-1] * 10))
    rc = _lib.load().mmpl_attn_fwd_groups_ex(*a.values(), plan, None)
    assert rc != 0
    return _lib.load().mmpl_last_error().decode(), list(plan)


REJECTS = [
    (dict(n_groups=0), "n_groups < 1"), (dict(n_groups=9), "more than 8 groups"), (dict(group_rows=0), "non-positive size"),
    (dict(q=P + 8), "q not 16-byte"), (dict(o=P + 8), "o not 16-byte"), (dict(ldq=260), "ldq % 8"), (dict(ldo=128), "ldo < 128 * num_heads"),
    (dict(k_pages=(C.c_void_p * 4)(P, P + 8, P, P)), "page not 16-byte"), (dict(v_pages=(C.c_void_p * 4)(P, P, 0, P)), "null page"),
    (dict(group_n_pages=(C.c_int * 2)(3, 0)), "a group with n_pages < 1"), (dict(group_n_pages=(C.c_int * 2)(25, 1)), "a group with more than 24 pages"),
    (dict(group_n_pages=None), "null argument"), (dict(history=P + 1), "history not 2-byte"), (dict(variant=1, q_prescaled=1), "prescaled q"),
]


@pytest.mark.parametrize("kw,msg", REJECTS, ids=[f"{i}-{m[:18]}" for i, (_, m) in enumerate(REJECTS)])
def test_rejects_launch_nothing(kw, msg):
    text, plan = _call(**kw)
    assert text.startswith("mmpl_attn_fwd_groups_ex:") and msg in text, text
    assert plan == [0] * 10                                        # no plan was made, nothing was launched
