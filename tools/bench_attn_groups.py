"""The grouped self-attention launch (mmpl_attn_fwd_groups_ex: G samples in one launch of attn_w64_kernel's body) against the G
launches of mmpl_attn_fwd_ex it replaces, on the shapes of a batched few-step block: G samples x F frames of S tokens, each sample
attending to its own window of `--window` cache slots.  Device events around `--reps` back-to-back calls after a warm-up of each.
Prints one JSON line per shape.

    python tools/bench_attn_groups.py --model 1.3B --resolution 480p
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="1.3B", choices=["1.3B", "14B"])
    ap.add_argument("--resolution", default="480p", choices=["480p", "720p"])
    ap.add_argument("--window", type=int, default=21)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", type=str, default="2x3,4x1,8x1", help="G x F, comma separated")
    args = ap.parse_args()
    from mmpl_amd import _lib
    from mmpl_amd.geometry import Geometry
    from mmpl_amd.synthetic import WAN_CONFIGS
    lib = _lib.load()
    dev = "cuda:0"
    cfg, S = WAN_CONFIGS[args.model], Geometry.named(args.resolution).frame_seqlen
    H, d, W = cfg["num_heads"], cfg["dim"], args.window
    scale = 1.0 / math.sqrt(128.0)
    ws = torch.empty(lib.mmpl_attn_workspace_bytes(), dtype=torch.uint8, device=dev)
    for shape in args.shapes.split(","):
        G, F = (int(v) for v in shape.split("x"))
        rows = F * S
        q = (torch.randn(G * rows, 3 * d, device=dev) * scale * 1.4426950408889634).to(torch.bfloat16)
        o = torch.empty(G * rows, d, dtype=torch.bfloat16, device=dev)
        k = torch.randn(G * W * S, d, device=dev).to(torch.bfloat16)
        v = torch.randn(G * W * S, d, device=dev).to(torch.bfloat16)
        pages = lambda t, gs: (C.c_void_p * (len(gs) * W))(*[t[(g * W + i) * S:].data_ptr() for g in gs for i in range(W)])
        each = (C.c_int * G)(*([W] * G))
        plan_g, plan_1 = (C.c_int * 10)(), (C.c_int * 8)()

        def grouped():
            _lib.check(lib.mmpl_attn_fwd_groups_ex(_lib.ptr(q), 3 * d, _lib.ptr(o), d, pages(k, range(G)), pages(v, range(G)), None, each, G, rows,
                                                   d, d, S, H, scale, _lib.ptr(ws), ws.numel(), 0, 1, None, None, plan_g, _lib.stream_ptr()), "grouped")

        def one_by_one():
            for g in range(G):
                _lib.check(lib.mmpl_attn_fwd_ex(_lib.ptr(q[g * rows:]), 3 * d, _lib.ptr(o[g * rows:]), d, pages(k, [g]), pages(v, [g]), None, d, d,
                                                W, S, rows, H, scale, _lib.ptr(ws), ws.numel(), 0, 1, 0, 0, None, None, plan_1, _lib.stream_ptr()),
                           "single")

        ms = {}
        for name, fn in (("grouped", grouped), ("one_by_one", one_by_one), ("grouped_again", grouped), ("one_by_one_again", one_by_one)):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            b.synchronize()
            ms[name] = a.elapsed_time(b) / args.reps
        flop = 4.0 * G * rows * W * S * d
        print(json.dumps(dict(metric="attn_groups_vs_single_launches", model=args.model, resolution=args.resolution, G=G, F=F, rows_per_group=rows,
                              keys_per_group=W * S, heads=H, plan_grouped=list(plan_g), plan_single=list(plan_1),
                              ms={n: round(t, 4) for n, t in ms.items()}, speedup=ms["one_by_one"] / ms["grouped"],
                              tflops_grouped=flop / ms["grouped"] / 1e9, tflops_one_by_one=flop / ms["one_by_one"] / 1e9)))


if __name__ == "__main__":
    main()
