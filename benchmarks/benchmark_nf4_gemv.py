#!/usr/bin/env python3
"""NF4 decode GEMV: the one-wave kernel (gemv_nf4_kernel) against the
workgroup-split kernel (gemv_nf4_wg_kernel), and one graphed block decode step.
Both kernels return the same bits for the same split count, so every row
compares speed alone.

  gemv   llama-70b projections at --batches (default 1 and 4), over the split
         counts _FastWeight tunes among: the old kernel, and the new kernel at
         the smallest of 4, 8, 16 waves that holds the split's reduce groups
         (and the next larger), nt off and on. us and packed TB/s (weight +
         absmax bytes); the call includes the split-K reduce, as in decode.
  tune   what _FastWeight picks for each shape (split count from its
         back-to-back loop, kernel and load policy from cold caches), and the
         time of that pick against the old kernel at the same split count.
  block  one llama-70b NF4 block decode step, hipGraph-replayed, on the tuned
         configuration and on the old kernel at the same split counts.

Method (that of benchmark_mxfp4.py): the paths alternate inside one loop, one
device-event pair per call, median over --iters calls after --warmup. The
operands rotate through --rotate-mb of weight copies (more than L2 plus the
256 MiB cache) and every call takes the next copy, so no call finds its weight
resident. Needs a GPU."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = {  # [in, out] of the fused projections
    "llama70b.qkv": (8192, 10240),
    "llama70b.o": (8192, 8192),
    "llama70b.gate_up": (8192, 57344),
    "llama70b.down": (28672, 8192),
}
BATCHES = (1, 4)
OLD_SPLITS = (0, 32, 64, 96, 128, 160, 192, 256, 320, 384)
WG_WAVES = (4, 8, 16)


def _median(samples):
    s = sorted(samples)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3  # us


def bench_gemv(hip, name, in_dim, out_dim, batches, iters, warmup, rotate_mb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    p, a = hip.nf4_quantize(w)
    del w
    nbytes = p.numel() + a.numel() * 2
    n = max(2, -(-(rotate_mb << 20) // nbytes))
    copies = [(p.clone(), a.clone(), a.t().contiguous()) for _ in range(n)]
    ws = torch.empty(64 * max(batches) * out_dim, device="cuda")
    rows = []
    for B in batches:
        x = torch.randn(B, in_dim, device="cuda", generator=g)
        paths = {}
        for s in OLD_SPLITS:
            if s * 32 <= in_dim:
                paths[f"old/{s}"] = (0, s, False)
        for s in OLD_SPLITS:
            if s == 0 or s * 32 > in_dim:
                continue
            fits = [wv for wv in WG_WAVES if s <= 16 * wv and not (wv == 16 and B == 4)]
            for wv in fits[:2]:  # the smallest wave count that holds a group, and the next
                paths[f"wg{wv}/{s}"] = (wv, s, False)
                paths[f"wg{wv}/{s}/nt"] = (wv, s, True)

        def call(cfg, i):
            c = copies[i]
            return hip.gemv_nf4(c[0], c[1], x, ws, None, 0, cfg[1], None, c[2], cfg[0], cfg[2])

        times = {k: [] for k in paths}
        i = 0  # every call takes the next copy: a copy returns after n other weights went by
        for it in range(warmup + iters):
            for k, cfg in paths.items():
                i += 1
                t = _timed(lambda: call(cfg, i % n))
                if it >= warmup:
                    times[k].append(t)
        med = {k: _median(v) for k, v in times.items()}
        best_old = min((k for k in med if k.startswith("old/")), key=med.get)
        best_wg = min((k for k in med if k.startswith("wg")), key=med.get)
        rows.append(dict(shape=name, in_dim=in_dim, out_dim=out_dim, B=B, us=med, best_old=best_old, best_wg=best_wg,
                         old_tbs=nbytes / med[best_old] / 1e6, wg_tbs=nbytes / med[best_wg] / 1e6))
        print(f"gemv {name:17s} B={B}  " + "  ".join(f"{k} {v:.1f}" for k, v in med.items()), flush=True)
        print(f"gemv {name:17s} B={B}  best {best_old} {med[best_old]:.1f} us {rows[-1]['old_tbs']:.2f} TB/s | "
              f"best {best_wg} {med[best_wg]:.1f} us {rows[-1]['wg_tbs']:.2f} TB/s | "
              f"wg/old time {med[best_wg] / med[best_old]:.3f}", flush=True)
    return rows


def bench_tune(hip, name, in_dim, out_dim, iters, warmup, rotate_mb, seed):
    """_FastWeight's pick for one shape, then that pick against the old kernel
    at the same split count, rotated and alternated as in bench_gemv."""
    from petals_amd.ops import fused_decode as fd

    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    fd._split_autotune_cache.pop(("nf4", in_dim, out_dim), None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fw = fd._FastWeight(w, hip, "nf4")
    torch.cuda.synchronize()
    tune_s = time.perf_counter() - t0
    del w
    picked = (fw.wg_waves, fw.splits, fw.nt)
    old = (0, fw.splits, False)
    nbytes = fw.packed.numel() + fw.absmax.numel() * 2
    n = max(2, -(-(rotate_mb << 20) // nbytes))
    copies = [(fw.packed.clone(), fw.absmax.clone(), fw.absmax_t.clone()) for _ in range(n)]
    x = torch.randn(1, in_dim, device="cuda", generator=g)
    ws = torch.empty(64 * out_dim, device="cuda")
    times = {"picked": [], "old_best": []}
    i = 0
    for it in range(warmup + iters):
        for k, cfg in (("picked", picked), ("old_best", old)):
            i += 1
            c = copies[i % n]
            t = _timed(lambda: hip.gemv_nf4(c[0], c[1], x, ws, None, 0, cfg[1], None, c[2], cfg[0], cfg[2]))
            if it >= warmup:
                times[k].append(t)
    med = {k: _median(v) for k, v in times.items()}
    print(f"tune {name:17s} B=1  picked (waves, splits, nt)={picked} {med['picked']:.1f} us "
          f"{nbytes / med['picked'] / 1e6:.2f} TB/s | old kernel, same splits {med['old_best']:.1f} us "
          f"{nbytes / med['old_best'] / 1e6:.2f} TB/s | autotune (quantize included) {tune_s:.2f} s", flush=True)
    return dict(shape=name, picked=picked, us=med, autotune_s=tune_s)


def bench_block(model, iters, warmup):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode as fd
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config(model)
    runs, tuned = {}, {}
    for label in ("tuned", "old"):
        if label == "old":  # same shapes and split counts, forced onto the one-wave kernel
            for key, val in list(fd._split_autotune_cache.items()):
                if key[0] == "nf4":
                    fd._split_autotune_cache[key] = (0, val[1], False)
        blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
        init_random_block_(blk, cfg, 0)
        blk = blk.eval().optimize_for_inference(quant="nf4")
        fp = blk._fast
        tuned[label] = {n: (w.wg_waves, w.splits, w.nt) for n, w in
                        (("qkv", fp.wqkv_t), ("o", fp.wo_t), ("gate_up", fp.wgateup_t), ("down", fp.wdown_t))}
        print(f"block {model} nf4 {label}: (waves, splits, nt) {tuned[label]}", flush=True)
        ks, vs = blk.kv_cache_shape(1, 64)
        k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros_like(k)
        h = torch.randn(1, 1, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5
        ctx = DecodeContext(torch.device("cuda"))
        ctx.set_position(8)
        with torch.no_grad():
            graph = GraphedCallable(lambda blk=blk, h=h, k=k, v=v, ctx=ctx: blk(h, kv_cache=(k, v), ctx=ctx), [])
        runs[label] = graph.replay
    # a 512 MiB read pass between replays: in decode 79 other blocks go by between two visits
    flush = torch.zeros(128 << 20, dtype=torch.int32, device="cuda")
    times = {k: [] for k in runs}
    for it in range(warmup + iters):
        for k, fn in runs.items():
            flush.sum()
            t = _timed(fn)
            if it >= warmup:
                times[k].append(t)
    med = {k: _median(v) for k, v in times.items()}
    print(f"block {model} B=1 graphed decode step, weights not cache-resident: "
          + "  ".join(f"{k} {v:.1f} us" for k, v in med.items()), flush=True)
    return dict(model=model, B=1, us=med, tuned=tuned)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--only", nargs="+", default=["gemv", "tune", "block"], choices=["gemv", "tune", "block"])
    parser.add_argument("--batches", type=int, nargs="+", default=list(BATCHES), choices=[1, 2, 3, 4])
    parser.add_argument("--iters", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    parser.add_argument("--rotate-mb", type=int, default=768,
                        help="bytes of weight copies each path rotates through (L2 + the 256 MiB cache and more)")
    parser.add_argument("--block", metavar="MODEL", default="llama-2-70b")
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args()

    if not torch.cuda.is_available():
        sys.exit("benchmark_nf4_gemv needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    if hip is None:
        sys.exit(f"HIP extension failed to load: {ops._hip_import_error!r}")
    print(f"device: {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} "
          f"rotate={args.rotate_mb} MB (median of per-call device-event times)", flush=True)
    result = {"benchmark": "nf4_gemv"}
    if "gemv" in args.only:
        result["gemv"] = []
        for name in args.shapes:
            result["gemv"] += bench_gemv(hip, name, *SHAPES[name], args.batches, args.iters, args.warmup, args.rotate_mb, args.seed)
            torch.cuda.empty_cache()
    if "tune" in args.only:
        result["tune"] = []
        for name in args.shapes:
            result["tune"].append(bench_tune(hip, name, *SHAPES[name], args.iters, args.warmup, args.rotate_mb, args.seed))
            torch.cuda.empty_cache()
    if "block" in args.only:
        result["block"] = bench_block(args.block, args.iters, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
