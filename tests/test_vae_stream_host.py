"""Streaming VAE decode, host side (no GPU): the argument checks of mmpl_vae_stream_* run before the first HIP call, the
reference fixture's frame-count facts (tests/golden/make_golden_vae_stream.py), and the CLI's --stream parsing / refusal."""
import ctypes as C
import os
import types

import pytest
import torch

from mmpl_amd import _lib, cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _err(rc):
    assert rc != 0
    return _lib.load().mmpl_last_error().decode()


@pytest.fixture
def vae():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mmpl_vae_create(8, 12, C.byref(h)) == 0
    yield lib, h
    lib.mmpl_vae_destroy(h)


def _bind_placeholders(lib, h):
    """mmpl_vae_bind_weights only asks for non-null pointers; nothing may dereference these before the checks are through."""
    n = lib.mmpl_vae_num_weights()
    arr = (C.c_void_p * n)(*[0x10000 + 256 * i for i in range(n)])
    assert lib.mmpl_vae_bind_weights(h, arr, n) == 0


def test_stream_entry_points_reject_bad_arguments(vae):
    lib, h = vae
    s = C.c_void_p()
    assert "null argument" in _err(lib.mmpl_vae_stream_create(None, C.byref(s)))
    assert "null argument" in _err(lib.mmpl_vae_stream_create(h, None))
    assert "null argument" in _err(lib.mmpl_vae_stream_reset(None))
    assert "null argument" in _err(lib.mmpl_vae_stream_decode(None, None, 1, None, None, None, 0, None, None, 0, None))
    lib.mmpl_vae_stream_destroy(None)                                       # like free(NULL)
    assert lib.mmpl_vae_stream_create(h, C.byref(s)) == 0 and s.value
    try:
        sc = (C.c_float * 16)()
        need = lib.mmpl_vae_workspace_bytes(h, 0)
        assert need > 0
        z, out, ws = C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000)
        n = C.c_int(-1)
        assert "weights not bound" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, out, 0, C.byref(n), ws, need, None))
        _bind_placeholders(lib, h)
        assert "n_frames < 1" in _err(lib.mmpl_vae_stream_decode(s, z, 0, sc, sc, out, 0, C.byref(n), ws, need, None))
        assert "unknown out_format" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, out, 2, C.byref(n), ws, need, None))
        assert "unknown out_format" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, out, -1, C.byref(n), ws, need, None))
        assert "workspace too small" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, out, 0, C.byref(n), ws, need - 1, None))
        assert "workspace too small" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, out, 1, C.byref(n), None, need, None))
        assert "null argument" in _err(lib.mmpl_vae_stream_decode(s, None, 1, sc, sc, out, 0, C.byref(n), ws, need, None))
        assert "null argument" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, None, 0, C.byref(n), ws, need, None))
        assert "4-byte aligned" in _err(lib.mmpl_vae_stream_decode(s, z, 1, sc, sc, C.c_void_p(0x30001), 1, C.byref(n), ws, need, None))
        assert n.value == -1                                                # a refused call reports nothing
        assert lib.mmpl_vae_stream_reset(s) == 0
    finally:
        lib.mmpl_vae_stream_destroy(s)


def test_stream_workspace_is_the_decoders(vae):
    """The stream's layout is the one-shot decoder's: the same size whether or not weights are bound; it grows with the geometry."""
    lib, h = vae
    a = lib.mmpl_vae_workspace_bytes(h, 0)
    _bind_placeholders(lib, h)
    assert lib.mmpl_vae_workspace_bytes(h, 0) == a
    h2 = C.c_void_p()
    assert lib.mmpl_vae_create(16, 24, C.byref(h2)) == 0
    assert lib.mmpl_vae_workspace_bytes(h2, 0) > a
    lib.mmpl_vae_destroy(h2)


def test_fixture_frame_count_facts():
    fx = torch.load(os.path.join(GOLDEN, "vae_stream_tiny.pt"))
    assert fx["splits"] == [[1, 3, 3], [3, 3, 1], [1] * 7, [2, 5]]
    assert fx["counts"] == [[1, 12, 12], [9, 12, 4], [1, 4, 4, 4, 4, 4, 4], [5, 20]]
    assert all(fx["equal"]) and fx["max_abs"] == [0.0] * 4               # the reference: every split == one-shot, bit for bit
    assert fx["stale_count"] == 4                                          # without clear_cache a lone latent is no first frame
    assert tuple(fx["dec_out"].shape) == (1, 3, 25, 64, 96) and fx["dec_out"].dtype == torch.bfloat16
    for split, counts in zip(fx["splits"], fx["counts"]):
        assert sum(split) == 7 and sum(counts) == 25
        assert counts == [1 + 4 * (n - 1) if i == 0 else 4 * n for i, n in enumerate(split)]


def test_engine_rejects_unknown_out_format():
    from mmpl_amd.vae import VaeEngine
    eng = VaeEngine.__new__(VaeEngine)                                     # no device: the check comes first
    with pytest.raises(ValueError, match="out_format"):
        eng.decode_stream(torch.zeros(1, 16, 8, 12), [0.0] * 16, [1.0] * 16, out_format="rgb")


def test_cli_stream_refused_without_fewstep_config(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--model", "tiny", "--duration", "1", "--stream"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--stream" in err and "denoising_step_list" in err


def test_cli_stream_refusal_text_and_parsing(tmp_path, capsys):
    few = types.SimpleNamespace(stream=True)
    assert cli.stream_refusal(few, fewstep=True) is None
    assert cli.stream_refusal(types.SimpleNamespace(stream=False), fewstep=False) is None
    assert cli.stream_refusal(types.SimpleNamespace(), fewstep=False) is None
    why = cli.stream_refusal(few, fewstep=False)
    assert why.startswith("--stream") and "few-step" in why
    # a few-step config with --stream passes the stream check and meets the existing few-step refusals
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n")
    with pytest.raises(SystemExit):
        cli.main(["--config_path", str(cfg), "--synthetic", "--model", "tiny", "--stream", "--duration", "2"])
    assert "--duration 2" in capsys.readouterr().err


def test_inference_stream_rejects_unknown_output():
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.pipeline import CausalInferencePipeline
    from mmpl_amd.scheduler import FlowMatchScheduler

    class _Gen:
        def __init__(self):
            self.geometry = Geometry.named("480p")
            self.scheduler = FlowMatchScheduler(shift=5.0, sigma_min=0.0, extra_one_step=True)
            self.scheduler.set_timesteps(1000, training=True)
            self.engine = types.SimpleNamespace(L=30, max_frames=7)
            self.model = types.SimpleNamespace(local_attn_size=-1, num_frame_per_block=1)

        def get_scheduler(self):
            return self.scheduler

    a = types.SimpleNamespace(denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                              independent_first_frame=False, context_noise=0)
    p = CausalInferencePipeline(a, "cpu", generator=_Gen(), text_encoder=object(), vae=object())
    with pytest.raises(ValueError, match="output"):
        next(p.inference_stream(torch.zeros(1, 3, 16, 60, 104), ["p"], output="rgb"))
