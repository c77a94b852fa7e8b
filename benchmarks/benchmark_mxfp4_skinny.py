#!/usr/bin/env python3
"""Wide decode for MXFP4 weights: gemm_mxfp4_skinny (9..32 rows,
ops/csrc/mxfp4_skinny.hip) against what those rows cost without it.

  gemm   llama-70b projections at rows 9/16/24/32: gemm_mxfp4_skinny at its
         default split count and over a sweep of overrides, against
           (a) gemm_mxfp4, the fused prefill GEMM;
           (b) mxfp4_dequantize + torch.matmul;
           (c) ceil(rows / 8) calls of gemv_mxfp4 (decode_step_auto's sub-batching);
         and gemm_nf4_skinny on the same shape as a yardstick.
  block  one llama-70b MXFP4 block step at B = 12/16/32, kv 512 and 4096: the
         wide decode_step against forward() with the dequant LRU warm and with
         it emptied before every call (benchmark_nf4_skinny.bench_block).

Method (benchmark_nf4_skinny.py's): the paths alternate inside one loop, one
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
from benchmark_nf4_skinny import ROWS, bench_block

SPLITS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48)  # overrides swept next to the default (0)
BASELINES = ("a.gemm_mxfp4", "b.dequant+matmul", "c.gemv_x")


def bench_gemm(hip, name, in_dim, out_dim, iters, warmup, repeats, rotate_mb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    p, s = hip.mxfp4_quantize(w)
    nfp, nfa = hip.nf4_quantize(w)
    del w
    nbytes = p.numel() + s.numel()
    n = _copies(nbytes, rotate_mb)
    mx_w = [(p.clone(), s.clone()) for _ in range(n)]
    nf_w = [(nfp.clone(), nfa.clone(), nfa.t().contiguous()) for _ in range(n)]
    ws = torch.empty(64 * 8 * out_dim, device="cuda")
    tiles = -(-out_dim // 256)
    out = []
    for rows in ROWS:
        x = torch.randn(rows, in_dim, device="cuda", generator=g)
        xb = x.to(torch.bfloat16)
        paths = {"skinny/0": lambda i: hip.gemm_mxfp4_skinny(mx_w[i][0], mx_w[i][1], x, ws, None, 0, 0, None)}
        for sp in SPLITS:
            if sp * rows <= 512:
                paths[f"skinny/{sp}"] = lambda i, sp=sp: hip.gemm_mxfp4_skinny(
                    mx_w[i][0], mx_w[i][1], x, ws, None, 0, sp, None)
        paths["a.gemm_mxfp4"] = lambda i: hip.gemm_mxfp4(mx_w[i][0], mx_w[i][1], xb, None)
        paths["b.dequant+matmul"] = lambda i: torch.matmul(xb, hip.mxfp4_dequantize(mx_w[i][0], mx_w[i][1]))
        paths["c.gemv_x"] = lambda i: [
            hip.gemv_mxfp4(mx_w[i][0], mx_w[i][1], x[r : r + 8], ws, None, 0, 0, None) for r in range(0, rows, 8)]
        paths["nf4_skinny"] = lambda i: hip.gemm_nf4_skinny(nf_w[i][0], nf_w[i][1], x, ws, None, 0, 0, None, nf_w[i][2])
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
        default = int(hip.gemm_mxfp4_skinny_splits(in_dim, out_dim, rows, 0))
        best = min((k for k in paths if k.startswith("skinny/") and k != "skinny/0"), key=us.get)
        # routed only where the slowest repeat of the kernel beats the fastest repeat of every baseline
        wins = all(spread["skinny/0"][1] < spread[b][0] for b in BASELINES)
        out.append(dict(shape=name, rows=rows, tiles=tiles, default_splits=default, best_override=best, wins=wins,
                        us=us, spread=spread, skinny_tbs=nbytes / us["skinny/0"] / 1e6))
        print(f"gemm {name:17s} rows={rows:2d} tiles={tiles:3d} S={default:2d} {nbytes / us['skinny/0'] / 1e6:.2f} TB/s "
              f"best={best} wins={wins}  "
              + "  ".join(f"{k} {us[k]:7.1f} [{spread[k][0]:.1f}..{spread[k][1]:.1f}]" for k in paths), flush=True)
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
        sys.exit("benchmark_mxfp4_skinny needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
    result = {}
    if args.only in (None, "gemm"):
        result["gemm"] = [r for name, (i, o) in SHAPES.items()
                          for r in bench_gemm(hip, name, i, o, args.iters, args.warmup, args.repeats,
                                              args.rotate_mb, args.seed)]
    if args.only in (None, "block"):
        result["block"] = bench_block(args.model, args.iters, args.warmup, args.repeats, quant="mxfp4")
    print(json.dumps({"benchmark": "mxfp4_skinny", **result}))


if __name__ == "__main__":
    main()
