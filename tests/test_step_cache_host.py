"""Step caching (TeaCache), host side (no GPU): StepCachePolicy.schedule against an independent restatement of its rule, the five new
C entries in the header and the library, and the CLI's flags and refusals."""
import os
import random
import re
import types

import numpy as np
import pytest

from mmpl_amd.step_cache import StepCachePolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mmpl_dit_forward_at_cached", "mmpl_dit_forward_full_cached", "mmpl_dit_step_cache_bytes", "mmpl_dit_time_embed",
               "mmpl_rel_l1_rows")


def restated(rel, thresh, coefficients, ret_steps, cutoff):
    """The rule as the design states it, written on numpy.poly1d and a running state machine of its own."""
    n = len(rel)
    cutoff = n - 1 if cutoff is None else cutoff
    P = np.poly1d(list(coefficients))
    forced = [i < ret_steps or i >= cutoff for i in range(n)]
    out, acc = [None] * n, 0.0
    for i in range(n):
        if not forced[i]:
            acc += float(P(rel[i]))
        out[i] = forced[i] or not acc < thresh
        acc = 0.0 if out[i] else acc
    return out


def test_schedule_equals_the_restated_rule_on_random_sequences():
    rng = random.Random(1234)
    skipped = 0
    for case in range(300):
        n = rng.randint(1, 60)
        rel = [0.0] + [rng.uniform(0.0, 0.3) for _ in range(n - 1)]
        coeff = [(1.0, 0.0), (2.0, -0.1, 0.01), (0.5, 1.5, 0.0, 0.02), (3.0,)][case % 4]
        ret = rng.randint(1, 6)
        cutoff = [None, n, rng.randint(0, n)][case % 3]
        thresh = rng.choice([0.0, 0.05, 0.2, 0.7])
        p = StepCachePolicy(thresh, coefficients=coeff, ret_steps=ret, cutoff=cutoff)
        got = p.schedule(rel)
        assert got == restated(rel, thresh, coeff, ret, cutoff), (case, rel, coeff, ret, cutoff, thresh)
        assert len(got) == n and all(isinstance(c, bool) for c in got)
        skipped += got.count(False)
    assert skipped > 500                                    # (the cases do skip)


def test_thresh_zero_computes_every_step():
    rel = [0.0] + [0.01 * (i % 7) for i in range(49)]
    assert StepCachePolicy(0.0).schedule(rel) == [True] * 50
    assert StepCachePolicy(0.0, ret_steps=5, cutoff=50, indicator="e0").schedule(rel) == [True] * 50


@pytest.mark.parametrize("ret_steps,cutoff", [(1, None), (5, 50), (3, 40), (1, 0)])
def test_huge_thresh_computes_exactly_the_forced_steps(ret_steps, cutoff):
    n = 50
    got = StepCachePolicy(1e30, ret_steps=ret_steps, cutoff=cutoff).schedule([0.0] + [0.1] * (n - 1))
    c = n - 1 if cutoff is None else cutoff
    assert got == [i < ret_steps or i >= c for i in range(n)]
    assert sum(got) == len(set(range(min(ret_steps, n))) | set(range(c, n)))


def test_coefficients_are_highest_power_first():
    """P(r) = 2 r + 10 (numpy.poly1d([2, 10])): every step adds more than 10, so thresh 10 computes every step; read in the other
    order (10 r + 2) four steps of r = 0.01 would be skipped at a time."""
    rel = [0.0] + [0.01] * 20
    p = StepCachePolicy(10.0, coefficients=(2.0, 10.0), cutoff=21)
    assert p.rescale(0.01) == pytest.approx(10.02) and float(np.poly1d([2.0, 10.0])(0.01)) == pytest.approx(10.02)
    assert p.schedule(rel) == [True] * 21
    flipped = StepCachePolicy(10.0, coefficients=(10.0, 2.0), cutoff=21).schedule(rel)
    assert flipped[:7] == [True, False, False, False, False, True, False]
    assert StepCachePolicy(1.0).coefficients == (1.0, 0.0) and StepCachePolicy(1.0).rescale(0.37) == 0.37      # the default: identity


def test_bad_arguments_raise():
    with pytest.raises(ValueError, match="ret_steps"):
        StepCachePolicy(0.1, ret_steps=0)
    with pytest.raises(ValueError, match="indicator"):
        StepCachePolicy(0.1, indicator="x")
    with pytest.raises(ValueError, match="thresh"):
        StepCachePolicy(-0.1)
    assert StepCachePolicy(0.1).key() != StepCachePolicy(0.2).key() and StepCachePolicy(0.1).key() == StepCachePolicy(0.1).key()


def test_header_declares_and_library_exports_the_new_entries():
    from mmpl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmpl_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_ENTRIES + ("mmpl_dit_time_embed_workspace_bytes",):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/mmpl_hip.h"
        assert name in _lib.SYMBOLS and hasattr(lib, name), f"{name} is not exported by libmmpl_hip.so"
    at = re.search(r"\bmmpl_dit_forward_at\s*\(([^)]*)\)", src).group(1).count(",") + 1
    full = re.search(r"\bmmpl_dit_forward_full\s*\(([^)]*)\)", src).group(1).count(",") + 1
    assert len(lib.mmpl_dit_forward_at_cached.argtypes) == at + 2          # ..., int cache_mode, void* residual
    assert len(lib.mmpl_dit_forward_full_cached.argtypes) == full + 3      # ..., const void* y_in, int cache_mode, void* residual
    assert len(lib.mmpl_dit_time_embed.argtypes) == 8 and len(lib.mmpl_rel_l1_rows.argtypes) == 6


# ---------------------------------------------------------------------------------------------------------------- CLI
def _cli_args(**kw):
    a = dict(num_samples=1, bidirectional=False, stream=False, extend=None, extend_context=None, num_frame_per_block=1, preview_vae=None,
             rolling=False, sample_solver="unipc", fp32_latents=False, duration=1, i2v=False, i2v_model=False, num_output_frames=21,
             cfg_split=False, sampling_steps=50, teacache_thresh=None, teacache_coefficients=None, teacache_ret_steps=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def test_cli_refusals_each_fire():
    from mmpl_amd import cli
    on = dict(teacache_thresh=0.1)
    assert cli.step_cache_refusal(_cli_args(**on), 1, False) is None and cli.first_refusal(_cli_args(**on), 1, False) is None
    assert cli.first_refusal(_cli_args(bidirectional=True, **on), 1, False) is None
    assert "50-step samplers" in cli.step_cache_refusal(_cli_args(**on), 1, True)
    assert "50-step samplers" in cli.first_refusal(_cli_args(bidirectional=True, **on), 1, True)
    assert "--num_samples" in cli.step_cache_refusal(_cli_args(num_samples=2, **on), 1, True)
    assert "--num_samples" in cli.first_refusal(_cli_args(num_samples=2, num_frame_per_block=3, **on), 1, True)
    assert "single-process" in cli.step_cache_refusal(_cli_args(**on), 2, False)
    assert "single-process" in cli.step_cache_refusal(_cli_args(cfg_split=True, **on), 1, False)
    assert "single-process" in cli.first_refusal(_cli_args(**on), 4, False)
    assert "at least 0" in cli.step_cache_refusal(_cli_args(teacache_thresh=-1.0), 1, False)
    assert "highest power first" in cli.step_cache_refusal(_cli_args(teacache_coefficients="1,x", **on), 1, False)
    assert "only with --teacache_thresh" in cli.step_cache_refusal(_cli_args(teacache_coefficients="1,0"), 1, False)
    assert "only with --teacache_thresh" in cli.step_cache_refusal(_cli_args(teacache_ret_steps=True), 1, False)


def test_cli_policy_from_flags():
    from mmpl_amd import cli
    assert cli.step_cache_policy(_cli_args()) is None
    p = cli.step_cache_policy(_cli_args(teacache_thresh=0.2))
    assert (p.thresh, p.coefficients, p.ret_steps, p.cutoff, p.indicator) == (0.2, (1.0, 0.0), 1, None, "e")
    p = cli.step_cache_policy(_cli_args(teacache_thresh=0.2, teacache_coefficients="2,-0.5,0.25", teacache_ret_steps=True, sampling_steps=40))
    assert (p.thresh, p.coefficients, p.ret_steps, p.cutoff, p.indicator) == (0.2, (2.0, -0.5, 0.25), 5, 40, "e0")


def test_command_line_without_the_flags_resolves_as_before():
    """A namespace that does not even know the new flags (every earlier caller's) is refused, or not, exactly as before: the new check
    is the last of first_refusal's list and says nothing."""
    from mmpl_amd import cli
    old = dict(num_samples=2, bidirectional=False, stream=False, extend=None, extend_context=None, num_frame_per_block=3, preview_vae=None,
               rolling=False, sample_solver="unipc", fp32_latents=False, duration=1, i2v=False, i2v_model=False, num_output_frames=21)
    ns = lambda **kw: types.SimpleNamespace(**dict(old, **kw))
    assert cli.step_cache_refusal(ns(), 1, True) is None and cli.step_cache_refusal(ns(), 8, False) is None
    assert cli.step_cache_policy(ns()) is None
    assert cli.first_refusal(ns(), 1, True) is None
    assert cli.first_refusal(ns(), 1, False) == cli.samples_refusal(ns(), False) and "few-step config" in cli.first_refusal(ns(), 1, False)
    assert cli.first_refusal(ns(stream=True), 1, True) == cli.samples_refusal(ns(stream=True), True)
    # with the flag, an earlier refusal still comes first
    assert cli.first_refusal(ns(teacache_thresh=0.1), 1, False) == cli.samples_refusal(ns(), False)
