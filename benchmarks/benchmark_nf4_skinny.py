#!/usr/bin/env python3
"""Wide decode: gemm_nf4_skinny (9..32 rows, ops/csrc/nf4_skinny.hip) against
what those rows cost without it.

  gemm   llama-70b projections at rows 9/16/24/32: gemm_nf4_skinny at its
         default split count and over a sweep of overrides, against
           (a) gemm_nf4, the fused prefill GEMM;
           (b) nf4_dequantize + torch.matmul;
           (c) torch.matmul on a resident bf16 copy;
           (d) ceil(rows / 8) calls of gemv_nf4 (decode_step_auto's sub-batching).
  block  one llama-70b NF4 block step at B = 12/16/32, kv 512 and 4096: the
         wide decode_step against forward() with the dequant LRU warm and with
         it emptied before every call.

Method (benchmark_mxfp4.py's): the paths alternate inside one loop, one
device-event pair per call, median over --iters calls after --warmup, the
whole measurement --repeats times (min..max of the medians is the spread).
Weights rotate through --rotate-mb of copies (well past L2 plus the 256 MB
cache) and every call takes the next copy. Needs a GPU."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from benchmark_mxfp4 import SHAPES, _copies, _median, _timed

ROWS = (9, 16, 24, 32)
SPLITS = (2, 4, 8, 16, 32)  # overrides swept next to the default (0)


def bench_gemm(hip, name, in_dim, out_dim, iters, warmup, repeats, rotate_mb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    p, a = hip.nf4_quantize(w)
    del w
    nbytes = p.numel() + a.numel() * 2
    n = _copies(nbytes, rotate_mb)
    nf_w = [(p.clone(), a.clone(), a.t().contiguous()) for _ in range(n)]
    nd = _copies(in_dim * out_dim * 2, rotate_mb)
    dense = [hip.nf4_dequantize(p, a) for _ in range(nd)]
    ws = torch.empty(64 * 8 * out_dim, device="cuda")
    out = []
    for rows in ROWS:
        x = torch.randn(rows, in_dim, device="cuda", generator=g)
        xb = x.to(torch.bfloat16)
        paths = {"skinny/0": lambda i: hip.gemm_nf4_skinny(nf_w[i][0], nf_w[i][1], x, ws, None, 0, 0, None, nf_w[i][2])}
        for s in SPLITS:
            if s * rows <= 512:
                paths[f"skinny/{s}"] = lambda i, s=s: hip.gemm_nf4_skinny(
                    nf_w[i][0], nf_w[i][1], x, ws, None, 0, s, None, nf_w[i][2])
        paths["a.gemm_nf4"] = lambda i: hip.gemm_nf4(nf_w[i][0], nf_w[i][1], xb, None)
        paths["b.dequant+matmul"] = lambda i: torch.matmul(xb, hip.nf4_dequantize(nf_w[i][0], nf_w[i][1]))
        paths["c.resident"] = lambda i: torch.matmul(xb, dense[i % nd])
        paths["d.gemv_x"] = lambda i: [
            hip.gemv_nf4(nf_w[i][0], nf_w[i][1], x[r : r + 8], ws, None, 0, 0, None, nf_w[i][2])
            for r in range(0, rows, 8)]
        meds = {k: [] for k in paths}
        call = 0
        for _ in range(repeats):
            times = {k: [] for k in paths}
            for it in range(warmup + iters):
                for k, fn in paths.items():
                    call += 1
                    t = _timed(lambda: fn(call % n))
                    if it >= warmup:
                        times[k].append(t)
            for k, v in times.items():
                meds[k].append(_median(v))
        us = {k: _median(v) for k, v in meds.items()}
        spread = {k: (min(v), max(v)) for k, v in meds.items()}
        default = int(hip.gemm_nf4_skinny_splits(in_dim, out_dim, rows, 0))
        out.append(dict(shape=name, rows=rows, default_splits=default, us=us, spread=spread,
                        skinny_tbs=nbytes / us["skinny/0"] / 1e6))
        print(f"gemm {name:17s} rows={rows:2d} S={default:2d} {nbytes / us['skinny/0'] / 1e6:.2f} TB/s  "
              + "  ".join(f"{k} {us[k]:7.1f} [{spread[k][0]:.1f}..{spread[k][1]:.1f}]" for k in paths), flush=True)
    return out


def bench_block(model, iters, warmup, repeats, quant="nf4"):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    cfg = load_model_config(model)
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    blk = blk.eval().optimize_for_inference(quant=quant)
    fast = blk._fast

    def empty_lru():
        fused_decode._dequant_cache = None
        fused_decode._dequant_cache_bytes = 0

    out = []
    for kv in (512, 4096):
        for B in (12, 16, 32):
            ks, vs = blk.kv_cache_shape(B, kv + 64)
            k = torch.randn(ks, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(vs, device="cuda", dtype=torch.bfloat16)
            h = torch.randn(B, 1, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5
            os.environ["PETALS_AMD_WIDE_DECODE"] = "on"
            runs = {
                "wide": lambda: fast.decode_step(h, k, v, kv),
                "forward/lru-warm": lambda: fast.forward(h, (k, v), kv),
                "forward/lru-empty": lambda: (empty_lru(), fast.forward(h, (k, v), kv)),
            }
            meds = {name: [] for name in runs}
            with torch.inference_mode():
                for _ in range(repeats):
                    times = {name: [] for name in runs}
                    for it in range(warmup + iters):
                        for name, fn in runs.items():
                            if name == "forward/lru-warm":
                                fn()  # untimed: refills the LRU the previous path emptied
                            t = _timed(fn)
                            if it >= warmup:
                                times[name].append(t)
                    for name, ts in times.items():
                        meds[name].append(_median(ts))
            us = {name: _median(m) for name, m in meds.items()}
            spread = {name: (min(m), max(m)) for name, m in meds.items()}
            out.append(dict(model=model, B=B, kv=kv, us=us, spread=spread))
            print(f"block {model} {quant} B={B:2d} kv={kv:4d}  "
                  + "  ".join(f"{name} {us[name]:8.1f} [{spread[name][0]:.1f}..{spread[name][1]:.1f}] us" for name in runs),
                  flush=True)
    empty_lru()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["gemm", "block"], default=None)
    ap.add_argument("--model", default="llama-2-70b")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_nf4_skinny needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
    result = {}
    if args.only in (None, "gemm"):
        result["gemm"] = [r for name, (i, o) in SHAPES.items()
                          for r in bench_gemm(hip, name, i, o, args.iters, args.warmup, args.repeats,
                                              args.rotate_mb, args.seed)]
    if args.only in (None, "block"):
        result["block"] = bench_block(args.model, args.iters, args.warmup, args.repeats)
    print(json.dumps({"benchmark": "nf4_skinny", **result}))


if __name__ == "__main__":
    main()
