"""Workspace sizes the C ABI reports, against the values recorded before the host layer's carvers were merged into one
(tests/golden/workspace_bytes.json).  Callers allocate exactly these sizes and the engines carve them at fixed offsets, so a carver
that rounds or orders its arithmetic differently shows here as another number.

The host cases cover the entries that make no HIP call and need no GPU.  mmpl_dit_create allocates its RoPE tables on the device, so
the DiT's three size functions are one gpu-marked case; its five numbers were recorded on an MI355X."""
import ctypes as C
import json
import os

import pytest

from mmpl_amd import _lib
from tests.util import GOLDEN

CODEC_SHAPES = [(1, 1), (3, 5), (60, 104)]
VAE_SHAPES = [(2, 2), (3, 5), (60, 104)]
T5_SHAPES = {   # the tiny config of tests/test_t5_gpu.py, and umT5-xxl
    "tiny": dict(vocab=1000, dim=256, dim_attn=256, dim_ffn=512, num_heads=4, num_layers=2, num_buckets=32, text_len=64, eps=1e-6),
    "umt5-xxl": dict(vocab=256384, dim=4096, dim_attn=4096, dim_ffn=10240, num_heads=64, num_layers=24, num_buckets=32, text_len=512,
                     eps=1e-6),
}


def _want():
    return json.load(open(os.path.join(GOLDEN, "workspace_bytes.json")))


def _with_handle(create, destroy, size):
    h = C.c_void_p()
    assert create(C.byref(h)) == 0 and h.value
    try:
        return size(h)
    finally:
        destroy(h)


def host_sizes():
    lib = _lib.load()
    out = {}
    for lh, lw in CODEC_SHAPES:
        out[f"taehv {lh}x{lw}"] = _with_handle(lambda p: lib.mmpl_taehv_create(lh, lw, p), lib.mmpl_taehv_destroy,
                                               lib.mmpl_taehv_workspace_bytes)
        out[f"taehv_enc {lh}x{lw}"] = _with_handle(lambda p: lib.mmpl_taehv_enc_create(lh, lw, p), lib.mmpl_taehv_enc_destroy,
                                                   lib.mmpl_taehv_enc_workspace_bytes)
    for lh, lw in VAE_SHAPES:
        for mode in (0, 1):
            out[f"vae {lh}x{lw} mode {mode}"] = _with_handle(lambda p: lib.mmpl_vae_create(lh, lw, p), lib.mmpl_vae_destroy,
                                                             lambda h: lib.mmpl_vae_workspace_bytes(h, mode))
    for name, cfg in T5_SHAPES.items():
        c = _lib.MmplT5Config(**cfg)
        out[f"t5 {name}"] = _with_handle(lambda p: lib.mmpl_t5_create(C.byref(c), p), lib.mmpl_t5_destroy, lib.mmpl_t5_workspace_bytes)
    for d in (1536, 5120):
        out[f"i2v_img_proj 257x1280 -> {d}"] = lib.mmpl_i2v_img_proj_workspace_bytes(257, 1280, d)
    out["i2v_cross_attn 1560x1536"] = lib.mmpl_i2v_cross_attn_workspace_bytes(1560, 1536)
    out["clip_visual 257x1280 mlp 5120 heads 16"] = lib.mmpl_clip_visual_workspace_bytes(257, 1280, 5120, 16)
    out["gemm_scratch"] = lib.mmpl_gemm_scratch_bytes()
    return out


def dit_sizes():
    """The tiny config and geometry of tests/test_dit_forward_gpu.py."""
    from mmpl_amd.dit import DitEngine
    from mmpl_amd.synthetic import WAN_CONFIGS
    eng = DitEngine(WAN_CONFIGS["tiny"], 16, 24, "cuda:0")
    lib = eng._lib
    out = {f"workspace n_frames {n}": lib.mmpl_dit_workspace_bytes(eng._h, n) for n in (1, 3)}
    out.update({f"full_workspace n_frames {n}": lib.mmpl_dit_full_workspace_bytes(eng._h, n) for n in (1, 5)})
    out["context_workspace"] = lib.mmpl_dit_context_workspace_bytes(eng._h)
    return out


def test_host_workspace_bytes_are_the_recorded_ones():
    got, want = host_sizes(), _want()["host"]
    assert sorted(got) == sorted(want)
    assert all(v > 0 for v in got.values())
    assert got == want


@pytest.mark.gpu
def test_dit_workspace_bytes_are_the_recorded_ones():
    got, want = dit_sizes(), _want()["dit"]
    assert len(want) == 5 and all(v > 0 for v in got.values())
    assert got == want
