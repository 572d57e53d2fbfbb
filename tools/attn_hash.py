#!/usr/bin/env python3
"""sha256 of the attention kernels' outputs on fixed seeded inputs at a few shapes -- to tell whether two builds of the library compute
the same BITS.  One line per shape; run it once per library and compare the lines.

    python tools/attn_hash.py [path/to/libmmpl_hip.so]        (default: the tree's mmpl_amd/lib/libmmpl_hip.so)

Every launch goes through mmpl_attn_fwd_ex / mmpl_attn_fwd_groups_ex (stateless), and its plan is printed next to the hash: the 64-rows-per-wave
kernel on a prescaled q (with and without a split tail), the lock-step kernel, the cross kernels with and without a weighted last row,
and a grouped launch whose tail round is split."""
import ctypes as C
import hashlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (bound by hand, not through mmpl_amd._lib: an older library lacks symbols that module binds)
lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "mmpl_amd", "lib", "libmmpl_hip.so"))
vp, ci, cf, sz, pp, pi = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
lib.mmpl_attn_fwd_ex.argtypes = [vp, ci, vp, ci, pp, pp, vp, ci, ci, ci, ci, ci, ci, cf, vp, sz, ci, ci, ci, ci, vp, vp, pi, vp]
lib.mmpl_attn_fwd_groups_ex.argtypes = [vp, ci, vp, ci, pp, pp, vp, pi, ci, ci, ci, ci, ci, ci, cf, vp, sz, ci, ci, vp, vp, pi, vp]
lib.mmpl_attn_workspace_bytes.restype = sz
lib.mmpl_last_error.restype = C.c_char_p
dev = "cuda:0"
SCALE = 1.0 / math.sqrt(128)
W64, LOCKSTEP = 4, 1        # variants: 4 = the 64-rows-per-wave kernel on a prescaled q, 1 = the lock-step / cross kernels on a raw q

# name: (variant, cross, last_row_copies, groups, Lq per group, H, rows per page, pages per group, gain)
SHAPES = {
    "small": (W64, 0, 0, 1, 700, 2, 328, 3, 1.0), "one_block": (W64, 0, 0, 1, 192, 2, 96, 2, 1.0), "s1_1p3B": (W64, 0, 0, 1, 10920, 12, 1560, 9, 1.0),
    "heavy": (W64, 0, 0, 1, 2600, 8, 640, 3, 6.0), "split_tail": (W64, 0, 0, 1, 256 * 41 - 57, 8, 640, 3, 1.0),
    "lockstep_h2": (LOCKSTEP, 0, 0, 1, 700, 2, 328, 3, 1.0), "lockstep_h3": (LOCKSTEP, 0, 0, 1, 700, 3, 328, 3, 1.0),
    "lockstep_cross_257": (LOCKSTEP, 1, 0, 1, 513, 16, 257, 1, 1.0),
    "cross_40": (LOCKSTEP, 1, 0, 1, 7 * 256 - 100, 40, 40, 1, 1.0), "cross_40_copies": (LOCKSTEP, 1, 448, 1, 7 * 256 - 100, 40, 40, 1, 1.0),
    "cross_100": (LOCKSTEP, 1, 0, 1, 7 * 256 - 100, 40, 100, 1, 1.0), "cross_100_copies": (LOCKSTEP, 1, 448, 1, 7 * 256 - 100, 40, 100, 1, 1.0),
    "grouped_split_tail": (W64, 0, 0, 2, 256 * 20 + 1, 8, 520, 3, 1.0),
}
for name, (variant, cross, copies, G, Lq, H, S, n_pages, gain) in SHAPES.items():
    torch.manual_seed(7)
    d = H * 128
    qmul = SCALE * 1.4426950408889634 if variant == W64 else 1.0
    q = (torch.randn(G * Lq, d, device=dev) * gain * qmul).to(torch.bfloat16)
    kc = (torch.randn(G * n_pages * S, d, device=dev) * gain).to(torch.bfloat16)
    vc = torch.randn(G * n_pages * S, d, device=dev).to(torch.bfloat16)
    o = torch.zeros(G * Lq, d, device=dev, dtype=torch.bfloat16)
    kp = (C.c_void_p * (G * n_pages))(*[kc[i * S:].data_ptr() for i in range(G * n_pages)])
    vpp = (C.c_void_p * (G * n_pages))(*[vc[i * S:].data_ptr() for i in range(G * n_pages)])
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
    plan = (C.c_int * 10)()
    stream = torch.cuda.current_stream().cuda_stream
    if G == 1:
        rc = lib.mmpl_attn_fwd_ex(q.data_ptr(), d, o.data_ptr(), d, kp, vpp, None, d, d, n_pages, S, Lq, H, SCALE, ws.data_ptr(), ws.numel(), variant, 0,
                                  cross, copies, None, None, plan, stream)
    else:
        n_each = (C.c_int * G)(*([n_pages] * G))
        rc = lib.mmpl_attn_fwd_groups_ex(q.data_ptr(), d, o.data_ptr(), d, kp, vpp, None, n_each, G, Lq, d, d, S, H, SCALE, ws.data_ptr(), ws.numel(),
                                         variant, 0, None, None, plan, stream)
    assert rc == 0, lib.mmpl_last_error()
    torch.cuda.synchronize()
    print("attnhash", name, hashlib.sha256(o.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16], "plan", list(plan), flush=True)
