"""The C-ABI library loads on a CPU-only box and exports every symbol include/mmpl_hip.h declares (no compute)."""
import ctypes
import os
import re

from mmpl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "mmpl_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmpl_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mmpl_hip.h but not exported by libmmpl_hip.so"
    assert sorted(_lib.SYMBOLS) == names, (sorted(set(names) ^ set(_lib.SYMBOLS)))


def test_version_and_error_strings():
    lib = _lib.load()
    assert b"gfx950" in lib.mmpl_version()
    assert isinstance(lib.mmpl_last_error(), bytes)


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.MmplDitConfig) == 13 * 4
    assert ctypes.sizeof(_lib.MmplUniPCStep) == 15 * 4
    assert ctypes.sizeof(_lib.MmplT5Config) == 9 * 4
    i, f = ctypes.c_int, ctypes.c_float
    assert _lib.MmplDitConfig._fields_ == [
        ("dim", i), ("ffn_dim", i), ("num_heads", i), ("num_layers", i), ("text_dim", i), ("freq_dim", i), ("in_dim", i),
        ("out_dim", i), ("text_len", i), ("eps", f), ("lat_h", i), ("lat_w", i), ("max_frames", i)]
    assert _lib.MmplUniPCStep._fields_ == [
        ("guidance", f), ("sigma_cur", f), ("use_corrector", i), ("corr_order", i), ("c_c1", f), ("c_c2", f), ("c_c3", f),
        ("c_inv_rk", f), ("c_rho0", f), ("c_rho_last", f), ("pred_order", i), ("p_c1", f), ("p_c2", f), ("p_c3", f), ("p_inv_rk", f)]
    assert _lib.MmplT5Config._fields_ == [
        ("vocab", i), ("dim", i), ("dim_attn", i), ("dim_ffn", i), ("num_heads", i), ("num_layers", i), ("num_buckets", i),
        ("text_len", i), ("eps", f)]
    t5 = _lib.MmplT5Config(vocab=7, text_len=512, eps=0.5)                 # constructible by keyword, as the engines do
    assert (t5.vocab, t5.dim, t5.text_len, t5.eps) == (7, 0, 512, 0.5)


def test_signatures_follow_header():
    """Every bound function has as many argtypes as its declaration has parameters (counted by this test's own regex), and a
    hand-written table pins the exact restype / argtypes of one function of each kind under the loader's rule."""
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmpl_hip.h")).read(), flags=re.S)
    decls = dict(re.findall(r"\b(mmpl_[a-z0-9_]+)\s*\(([^)]*)\)", src))
    assert sorted(decls) == _declared()
    for name, params in decls.items():
        n = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(getattr(lib, name).argtypes) == n, (name, n, getattr(lib, name).argtypes)
    vp, ci, cf, cd, sz, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t, ctypes.c_longlong
    P = ctypes.POINTER
    fwd = [vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, sz]
    table = {
        "mmpl_dit_workspace_bytes": (sz, [vp, ci]),
        "mmpl_dit_rope_tables": (ci, [vp, vp, vp, vp]),
        "mmpl_dit_destroy": (None, [vp]),
        "mmpl_dit_weight_name": (ctypes.c_char_p, [ci, ci]),
        "mmpl_last_error": (ctypes.c_char_p, []),
        "mmpl_gemm_scratch_bytes": (sz, []),
        "mmpl_fewstep_update": (ci, [vp, vp, vp, vp, sz, cd, cf, vp]),
        "mmpl_taehv_conv": (ci, [vp, vp, ll, ll, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, ci, vp, ll, ci, ci, ci, vp, ll, vp, vp]),
        "mmpl_cfg_unipc_step": (ci, [vp, vp, vp, vp, vp, vp, sz, P(_lib.MmplUniPCStep), vp]),
        "mmpl_cfg_unipc_step_table": (ci, [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, ci, ci, vp]),   # table_dev: a device pointer
        "mmpl_t5_create": (ci, [P(_lib.MmplT5Config), vp]),
        "mmpl_dit_create": (ci, [P(_lib.MmplDitConfig), vp]),
        "mmpl_vae_stream_create": (ci, [vp, vp]),
        "mmpl_profile_read": (ci, [ci, vp, vp, vp]),
        "mmpl_probe_mfma_tflops": (ci, [ci, cd, vp]),
        "mmpl_dit_forward": (ci, fwd + [vp]),
        "mmpl_dit_forward_at": (ci, fwd + [vp, vp]),
        "mmpl_attn_fwd": (ci, [vp, ci, vp, ci, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]),
        "mmpl_layernorm_ex": (ci, [vp, ci, vp, ci, ci, ci, cf, vp, vp, ci, ci, vp, vp, ci, ci, vp, vp]),
        "mmpl_qknorm_ex": (ci, [vp, ci, vp, ci, vp, ci, vp, vp, ci, ci, cf, cf, ci, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp, vp]),
        "mmpl_modulation": (ci, [vp, ll, vp, ci, ci, vp, ci, ci, ci, ci, vp]),
        "mmpl_silu": (ci, [vp, vp, sz, vp]),
        "mmpl_rows_equal_last": (ci, [vp, ci, ci, ci, vp, vp]),
        "mmpl_t5_gather": (ci, [vp, vp, vp, ci, ci, vp]),
        "mmpl_t5_softmax": (ci, [vp, vp, vp, vp, vp, ci, ci, vp]),
        "mmpl_t5_transpose": (ci, [vp, ci, vp, ci, ci, ci, vp]),
        "mmpl_t5_gated": (ci, [vp, vp, sz, vp]),
        "mmpl_t5_zero_pad": (ci, [vp, vp, ci, ci, vp]),
        "mmpl_gelu_erf": (ci, [vp, sz, vp]),
        "mmpl_add": (ci, [vp, vp, sz, vp]),
    }
    assert len(table["mmpl_dit_forward_at"][1]) == 22
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)


def test_weight_slot_names():
    lib = _lib.load()
    cfg = _lib.MmplDitConfig(dim=256, ffn_dim=512, num_heads=2, num_layers=2, text_dim=64, freq_dim=256, in_dim=16, out_dim=16,
                             text_len=512, eps=1e-6, lat_h=16, lat_w=24, max_frames=7)
    assert lib.mmpl_dit_num_weights(ctypes.byref(cfg)) == 16 + 2 * 22
    assert lib.mmpl_dit_weight_name(0, 0) == b"patch_embedding.weight"
    assert lib.mmpl_dit_weight_name(21, 1) == b"ffn.2.bias"
    assert lib.mmpl_dit_weight_name(22, 1) is None


def test_weight_slot_walk_order():
    """DitEngine binds what the library's slot names say, in the library's order: the walk load_state_dict uses (no handle, no
    device) names the slots and fetches the state-dict keys in exactly the order written out here."""
    import torch
    from mmpl_amd import dit
    lib = _lib.load()
    global_keys = ["patch_embedding.weight", "patch_embedding.bias", "text_embedding.0.weight", "text_embedding.0.bias",
                   "text_embedding.2.weight", "text_embedding.2.bias", "time_embedding.0.weight", "time_embedding.0.bias",
                   "time_embedding.2.weight", "time_embedding.2.bias", "time_projection.1.weight", "time_projection.1.bias",
                   "head.modulation", "head.head.weight", "head.head.bias"]
    layer_keys = ["self_attn.norm_q.weight", "self_attn.norm_k.weight", "self_attn.o.weight", "self_attn.o.bias",
                  "norm3.weight", "norm3.bias", "cross_attn.q.weight", "cross_attn.q.bias", "cross_attn.norm_q.weight",
                  "cross_attn.k.weight", "cross_attn.k.bias", "cross_attn.norm_k.weight", "cross_attn.v.weight",
                  "cross_attn.v.bias", "cross_attn.o.weight", "cross_attn.o.bias", "ffn.0.weight", "ffn.0.bias",
                  "ffn.2.weight", "ffn.2.bias"]
    assert dit.weight_slot_names(lib, 0) + dit.weight_slot_names(lib, 1) == \
        global_keys + ["pack:blocks.*.modulation[L,6,dim]"] + \
        ["pack:self_attn.{q,k,v}.weight[3dim,dim]", "pack:self_attn.{q,k,v}.bias[3dim]"] + layer_keys

    # the tiny config's geometry (dim 256, 2 layers, in_dim 16): every fetched key, in order, and the shapes of what is bound
    L, dim, in_dim = 2, 256, 16
    shapes = {"patch_embedding.weight": (dim, in_dim, 1, 2, 2), "modulation": (1, 6, dim), "self_attn.q.weight": (dim, dim),
              "self_attn.k.weight": (dim, dim), "self_attn.v.weight": (dim, dim)}
    fetched = []

    def g(key):
        fetched.append(key)
        return torch.full(shapes.get(key.split(".", 2)[2] if key.startswith("blocks.") else key, (dim,)), float(len(fetched)))

    w = dit.slot_tensors(lib, g, L, dim, in_dim)
    qkv = [f"self_attn.{x}.{part}" for part in ("weight", "bias") for x in "qkv"]
    assert fetched == global_keys + [f"blocks.{i}.modulation" for i in range(L)] + \
        [f"blocks.{i}.{k}" for i in range(L) for k in qkv + layer_keys]
    assert len(w) == 16 + L * 22 and all(t.is_contiguous() for t in w)
    assert w[0].shape == (dim, 64) and bool((w[0][:, :4 * in_dim] == 1).all()) and bool((w[0][:, 4 * in_dim:] == 0).all())
    assert w[15].shape == (L, 6, dim) and w[16].shape == (3 * dim, dim) and w[17].shape == (3 * dim,)
    # a tensor's fill value is its position in the fetch order: q | k | v of layer 0 follow the 15 globals and the L modulations
    assert [float(w[16][r * dim, 0]) for r in range(3)] == [15.0 + L + 1, 15.0 + L + 2, 15.0 + L + 3]
    assert float(w[18][0]) == 15.0 + L + 7                                                  # layer 0's self_attn.norm_q.weight


def test_no_oracle_import_in_product():
    """the product path must never route through the oracle (or any CPU fallback)."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "mmpl_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
