"""TAEHV preview decoder, host side (no GPU): the restatement tests/taehv_ref.py against the real reference's output
(tests/golden/taehv_tiny.pt, tests/golden/make_golden_taehv.py), the fixture's own conditions, the argument checks of mmpl_taehv_*
that run before the first HIP call, the weight names, and the CLI / pipeline refusals."""
import ctypes as C
import os
import types

import pytest
import torch

import taehv_ref
from mmpl_amd import _lib, cli
from mmpl_amd.synthetic import philox_normal, taehv_layout, taehv_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEMBLOCKS = [3, 4, 5, 9, 10, 11, 15, 16, 17]
# The reference's own two evaluation orders (parallel=True / False) differ by ~3e-7 relative in fp32 (6e-7 on this fixture, stored
# as parallel_rel_l2), its bf16 evaluation by 6e-3: 1e-5 sits well clear of both.
RESTATEMENT_TOL = 1e-5


@pytest.fixture(scope="module")
def fx():
    return torch.load(os.path.join(GOLDEN, "taehv_tiny.pt"))


@pytest.fixture(scope="module")
def video(fx):
    m = fx["meta"]
    return taehv_state_dict(seed=m["weight_seed"]), philox_normal(m["z_shape"], m["z_seed"])


def test_restatement_reproduces_the_reference(fx, video):
    sd, z = video
    torch.set_grad_enabled(False)
    out = taehv_ref.decode_video(sd, z.float())
    assert tuple(out.shape) == tuple(fx["exact"].shape) == (12, 3, 64, 96)
    d = taehv_ref.rel_l2(out, fx["exact"])
    print(f"restatement vs reference: rel L2 {d:.3e} (the reference's two orders: {fx['parallel_rel_l2']:.3e})")
    assert d <= RESTATEMENT_TOL
    assert fx["parallel_rel_l2"] < RESTATEMENT_TOL < fx["ref_bf16_rel_l2"]


def test_restatement_streams_and_is_causal(fx, video):
    """Frame counts (4 per latent, untrimmed) and the prefix property for the restatement's streamed mode.  The reference against
    itself: exactly 0 for 2 of 3 latents, round-off for 1 of 3 (another convolution algorithm at batch 1) -- recorded, not asserted
    as bit-equality; the restatement is held to the same 1e-5."""
    sd, z = video
    torch.set_grad_enabled(False)
    assert [p["frames"] for p in fx["prefix"]] == [4, 8] and [p["latents"] for p in fx["prefix"]] == [1, 2]
    assert all(p["max_abs"] < 1e-4 for p in fx["prefix"])
    for split in ([1, 1, 1], [2, 1], [1, 2]):
        m = taehv_ref.TaehvRef(sd)
        parts, f0 = [], 0
        for n in split:
            parts.append(m.decode(z[f0:f0 + n].float()))
            assert parts[-1].shape[0] == 4 * n
            f0 += n
        assert taehv_ref.rel_l2(torch.cat(parts), fx["exact"]) <= RESTATEMENT_TOL, split
    for n in (1, 2):
        p = taehv_ref.decode_video(sd, z[:n].float())
        assert p.shape[0] == 4 * n
        assert taehv_ref.rel_l2(p, fx["exact"][:4 * n]) <= RESTATEMENT_TOL


def test_restatement_patch_tgrow_case(fx, video):
    sd, _ = video
    torch.set_grad_enabled(False)
    tg = fx["tgrow"]
    g = torch.Generator().manual_seed(tg["extra_seed"])
    extra = (torch.randn(256, 256, 1, 1, generator=g) * (1.0 / 16)).to(torch.bfloat16)
    big = dict(sd)
    big["decoder.7.conv.weight"] = torch.cat([extra, sd["decoder.7.conv.weight"]], 0)     # 2 * 256 rows: the LAST 256 are kept
    z = philox_normal(tg["z_shape"], tg["z_seed"])
    out = taehv_ref.decode_video(big, z.float())
    assert tuple(out.shape) == tuple(tg["out"].shape)
    assert taehv_ref.rel_l2(out, tg["out"]) <= RESTATEMENT_TOL
    from mmpl_amd.taehv import patch_tgrow_layers
    kept = patch_tgrow_layers(big)["decoder.7.conv.weight"]
    assert torch.equal(kept, sd["decoder.7.conv.weight"]) and big["decoder.7.conv.weight"].shape[0] == 512


def test_fixture_conditions(fx, video):
    """Neither the clamp nor the uint8 conversion can hide an error, and every MemBlock's memory matters."""
    sd, z = video
    torch.set_grad_enabled(False)
    x = fx["exact"]
    inside = float(((x > 0) & (x < 1)).float().mean())
    beyond = float(((x < -1) | (x > 2)).float().mean())
    print(f"inside (0, 1): {inside:.3f}; beyond [-1, 2]: {beyond:.4f}; ref_bf16_rel_l2 {fx['ref_bf16_rel_l2']:.3e}")
    assert inside >= 0.5 and beyond < 0.05
    assert 1e-3 < fx["ref_bf16_rel_l2"] < 2e-2                            # one bf16 rounding per layer over 35 layers, not more
    bf = torch.load(os.path.join(GOLDEN, "taehv_tiny_bf16.pt"))["ref_bf16"]
    assert bf.dtype == torch.bfloat16 and abs(taehv_ref.rel_l2(bf.float(), x) - fx["ref_bf16_rel_l2"]) < 1e-9
    assert len(fx["mem_effect"]) == 9 and min(fx["mem_effect"]) > 2 * fx["ref_bf16_rel_l2"]
    for i, recorded in zip(MEMBLOCKS, fx["mem_effect"]):
        cut = dict(sd)
        w = sd[f"decoder.{i}.conv.0.weight"].clone()
        w[:, w.shape[1] // 2:] = 0
        cut[f"decoder.{i}.conv.0.weight"] = w
        d = taehv_ref.rel_l2(taehv_ref.decode_video(cut, z.float()), x)
        assert d > 2 * fx["ref_bf16_rel_l2"] and abs(d - recorded) < 1e-3, (i, d, recorded)


def test_synthetic_layout_is_the_decoder():
    keys = [k for k, _, _ in taehv_layout()]
    assert len(keys) == 64 and all(k.startswith("decoder.") for k in keys)
    n = 0
    for _, shape, _ in taehv_layout():
        e = 1
        for s in shape:
            e *= s
        n += e
    assert n == 9844611                                                     # the reference decoder's parameter count
    sd = taehv_state_dict(seed=1)
    assert list(sd) == keys and all(v.dtype == torch.bfloat16 for v in sd.values())
    assert all(torch.equal(a, b) for a, b in zip(sd.values(), taehv_state_dict(seed=1).values()))


def _err(rc):
    assert rc != 0
    return _lib.load().mmpl_last_error().decode()


def test_weight_names_are_the_decoder_keys():
    lib = _lib.load()
    n = lib.mmpl_taehv_num_weights()
    names = [lib.mmpl_taehv_weight_name(i).decode() for i in range(n)]
    assert lib.mmpl_taehv_weight_name(n) is None and lib.mmpl_taehv_weight_name(-1) is None
    assert names == [k for k, _, _ in taehv_layout()]
    assert not any(k.startswith("encoder.") for k in names)


def test_entry_points_reject_bad_arguments():
    lib = _lib.load()
    h = C.c_void_p()
    assert "bad arguments" in _err(lib.mmpl_taehv_create(8, 12, None))
    assert "bad arguments" in _err(lib.mmpl_taehv_create(0, 12, C.byref(h)))
    assert "null argument" in _err(lib.mmpl_taehv_reset(None))
    assert "null argument" in _err(lib.mmpl_taehv_decode(None, None, 1, None, 0, None, None, 0, None))
    assert lib.mmpl_taehv_workspace_bytes(None) == 0
    lib.mmpl_taehv_destroy(None)                                            # like free(NULL)
    assert lib.mmpl_taehv_create(8, 12, C.byref(h)) == 0 and h.value
    try:
        need = lib.mmpl_taehv_workspace_bytes(h)
        assert need > 0
        z, out, ws = C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000)
        n = C.c_int(-1)
        assert "weights not bound" in _err(lib.mmpl_taehv_decode(h, z, 1, out, 0, C.byref(n), ws, need, None))
        nw = lib.mmpl_taehv_num_weights()
        assert "wrong pointer count" in _err(lib.mmpl_taehv_bind_weights(h, (C.c_void_p * 3)(1, 2, 3), 3))
        assert "null weight pointer" in _err(lib.mmpl_taehv_bind_weights(h, (C.c_void_p * nw)(*([0x1000] * (nw - 1) + [0])), nw))
        assert "weights not bound" in _err(lib.mmpl_taehv_decode(h, z, 1, out, 0, C.byref(n), ws, need, None))
        arr = (C.c_void_p * nw)(*[0x10000 + 256 * i for i in range(nw)])   # nothing may dereference these before the checks are through
        assert lib.mmpl_taehv_bind_weights(h, arr, nw) == 0
        assert lib.mmpl_taehv_workspace_bytes(h) == need
        assert "n_frames < 1" in _err(lib.mmpl_taehv_decode(h, z, 0, out, 0, C.byref(n), ws, need, None))
        assert "unknown out_format" in _err(lib.mmpl_taehv_decode(h, z, 1, out, 2, C.byref(n), ws, need, None))
        assert "unknown out_format" in _err(lib.mmpl_taehv_decode(h, z, 1, out, -1, C.byref(n), ws, need, None))
        assert "workspace too small" in _err(lib.mmpl_taehv_decode(h, z, 1, out, 0, C.byref(n), ws, need - 1, None))
        assert "workspace too small" in _err(lib.mmpl_taehv_decode(h, z, 1, out, 1, C.byref(n), None, need, None))
        assert "null argument" in _err(lib.mmpl_taehv_decode(h, None, 1, out, 0, C.byref(n), ws, need, None))
        assert "null argument" in _err(lib.mmpl_taehv_decode(h, z, 1, None, 0, C.byref(n), ws, need, None))
        assert n.value == -1                                                # a refused call reports nothing
        assert lib.mmpl_taehv_reset(h) == 0
        h2 = C.c_void_p()
        assert lib.mmpl_taehv_create(9, 13, C.byref(h2)) == 0
        assert lib.mmpl_taehv_workspace_bytes(h2) > need                    # grows with the geometry
        lib.mmpl_taehv_destroy(h2)
    finally:
        lib.mmpl_taehv_destroy(h)


def test_engine_rejects_unknown_out_format():
    from mmpl_amd.taehv import TaehvEngine
    eng = TaehvEngine.__new__(TaehvEngine)                                  # no device: the check comes first
    with pytest.raises(ValueError, match="out_format"):
        eng.decode_stream(torch.zeros(1, 16, 8, 12), out_format="rgb")
    with pytest.raises(ValueError, match="out_format"):
        eng.decode(torch.zeros(1, 16, 8, 12), out_format="rgb")


def test_engine_packing_layout():
    """The fragment-major packing the header documents: element (n, tap, c) of a conv weight at
    ((((c / 32) * taps + tap) * (Cout_pad / 16) + n / 16) * 4 + (c % 32) / 8) * 16 + n % 16) * 8 + c % 8."""
    from mmpl_amd.taehv import TaehvEngine
    w = torch.arange(3 * 64 * 9, dtype=torch.float32).reshape(3, 64, 3, 3) % 251            # exact in bf16
    p = TaehvEngine._repack("decoder.22.weight", w)
    assert p.numel() == 2 * 9 * 1 * 64 * 8
    for n, tap, c in [(0, 0, 0), (2, 4, 37), (1, 8, 63), (2, 5, 8)]:
        at = ((((c // 32) * 9 + tap) * 1 + n // 16) * 4 + (c % 32) // 8) * 16 + n % 16
        assert float(p[at * 8 + c % 8]) == float(w[n, c, tap // 3, tap % 3])
    w16 = torch.ones(256, 16, 3, 3)
    assert TaehvEngine._repack("decoder.1.weight", w16).numel() == 9 * 256 * 32 and float(TaehvEngine._repack("decoder.1.weight", w16).sum()) == 256 * 16 * 9
    assert TaehvEngine._repack("decoder.22.bias", torch.ones(3)).tolist() == [1, 1, 1, 0]


def test_read_taehv_checkpoint(tmp_path):
    from mmpl_amd.checkpoints import read_taehv
    sd = taehv_state_dict(seed=2)
    blob = dict(sd)
    blob["encoder.0.weight"] = torch.zeros(64, 3, 3, 3)
    torch.save(blob, tmp_path / "taew2_1.pth")
    got = read_taehv(str(tmp_path / "taew2_1.pth"))
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    torch.save({"encoder.0.weight": torch.zeros(1)}, tmp_path / "enc.pth")
    with pytest.raises(ValueError, match="decoder"):
        read_taehv(str(tmp_path / "enc.pth"))


def test_cli_preview_vae_refused_without_stream(tmp_path, capsys):
    assert cli.preview_refusal(types.SimpleNamespace(preview_vae=None, stream=False)) is None
    assert cli.preview_refusal(types.SimpleNamespace()) is None
    assert cli.preview_refusal(types.SimpleNamespace(preview_vae="", stream=True)) is None
    why = cli.preview_refusal(types.SimpleNamespace(preview_vae="", stream=False))
    assert why.startswith("--preview_vae") and "--stream" in why
    cfg = tmp_path / "self_forcing_dmd.yaml"
    cfg.write_text("denoising_step_list: [1000, 750, 500, 250]\nwarp_denoising_step: true\nnum_frame_per_block: 3\n")
    for extra in (["--preview_vae"], ["--preview_vae", "some/taew2_1.pth"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["--config_path", str(cfg), "--synthetic", "--model", "tiny", "--duration", "1"] + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--preview_vae" in err and "--stream" in err
    with pytest.raises(SystemExit) as e:                                     # the 50-step pipeline: same refusal
        cli.main(["--synthetic", "--model", "tiny", "--duration", "1", "--preview_vae"])
    assert e.value.code == 2 and "--preview_vae" in capsys.readouterr().err


def _host_pipeline(preview_vae=None):
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
    return CausalInferencePipeline(a, "cpu", generator=_Gen(), text_encoder=object(), vae=object(), preview_vae=preview_vae)


def test_inference_stream_decoder_argument():
    p = _host_pipeline()
    assert p.preview_vae is None
    noise = torch.zeros(1, 3, 16, 60, 104)
    with pytest.raises(ValueError, match="preview"):
        next(p.inference_stream(noise, ["p"], decoder="preview"))
    with pytest.raises(ValueError, match="decoder"):
        next(p.inference_stream(noise, ["p"], decoder="tiny"))
    with pytest.raises(ValueError, match="decoder"):
        next(_host_pipeline(preview_vae=object()).inference_stream(noise, ["p"], decoder="tiny"))
