#!/usr/bin/env python3
"""Mixtral wide decode: gemm_nf4_moe_skinny (17..64 virtual rows grouped by
expert, ops/csrc/moe_skinny.hip) against what those rows cost without it.

  op     the 8x7B / 8x22B expert stacks at R = 18/32/48/64 virtual rows with a
         router-like sel (distinct top-2 experts per token): the new op at its
         default split count and over a sweep of overrides, against
           (a) sort_pairs_by_expert + moe_gemm, what these rows run today;
           (b) ceil(R / 16) calls of gemv_nf4_moe on 16-row slices.
  block  one mixtral-8x7b NF4 block step at B = 12/16/32, kv 512 and 4096, and
         (B, T) = (4, 4): the wide decode_step / decode_multi against forward()
         with the dequant LRU warm and with it emptied before every call.

Method (benchmark_nf4_skinny.py's): the paths alternate inside one loop, one
device-event pair per call, median over --iters calls after --warmup, the
whole measurement --repeats times (min..max of the medians is the spread).
The expert stacks rotate through --rotate-mb of copies (well past L2 plus the
256 MB cache) and every call takes the next copy. Needs a GPU."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from benchmark_mxfp4 import _copies, _median, _timed

EXPERTS, TOP_K = 8, 2
SHAPES = {  # name -> (in, out, k_per_tok, epilogue)
    "8x7b.gate_up": (4096, 28672, TOP_K, 3),
    "8x7b.down": (14336, 4096, 1, 0),
    "8x22b.gate_up": (6144, 32768, TOP_K, 3),
    "8x22b.down": (16384, 6144, 1, 0),
}
ROWS = (18, 32, 48, 64)
SPLITS = (1, 2, 4, 8)  # overrides swept next to the default (0)


def _alternate(paths, n, iters, warmup, repeats):
    """{name: (median us, min, max of the repeats' medians)}; every call takes the next weight copy."""
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
    return {k: (_median(v), min(v), max(v)) for k, v in meds.items()}


def bench_op(hip, name, iters, warmup, repeats, rotate_mb, seed, splits=SPLITS):
    from petals_amd.ops.fused_moe import sort_pairs_by_expert

    in_dim, out_dim, k, epi = SHAPES[name]
    g = torch.Generator(device="cuda").manual_seed(seed)
    pa = [hip.nf4_quantize((torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16))
          for _ in range(EXPERTS)]
    p, a = torch.stack([q for q, _ in pa]), torch.stack([q for _, q in pa])
    del pa
    nbytes = p.numel() + a.numel() * 2
    n = _copies(nbytes, rotate_mb)
    w = [(p.clone(), a.clone(), a.transpose(1, 2).contiguous()) for _ in range(n)]
    ws = torch.empty(64 * 8 * out_dim, device="cuda")
    out = []
    for rows in ROWS:
        tokens = rows // TOP_K
        selected = torch.stack([torch.randperm(EXPERTS, device="cuda", generator=g)[:TOP_K] for _ in range(tokens)])
        sel = selected.to(torch.int32).reshape(-1).contiguous()
        x = torch.randn(rows // k, in_dim, device="cuda", generator=g)
        xb = x.to(torch.bfloat16)
        active = int(torch.unique(sel).numel())

        def skinny(i, s=0):
            return hip.gemm_nf4_moe_skinny(w[i][0], w[i][1], x, sel, k, ws, epi, s, w[i][2])

        def grouped(i):  # today's path: host-free sort, padded 32-row tiles, then the epilogue's swiglu
            sp, te = sort_pairs_by_expert(selected, EXPERTS)
            c = hip.moe_gemm(None, w[i][0], w[i][1], xb, sp, te, k, rows)
            return hip.swiglu(c[:, : out_dim // 2].contiguous(), c[:, out_dim // 2 :].contiguous()) if epi == 3 else c

        def gemv_slices(i):
            return [hip.gemv_nf4_moe(w[i][0], w[i][1], x[r // k : (r + 16) // k], sel[r : r + 16], k, ws, epi)
                    for r in range(0, rows, 16)]

        paths = {"skinny/0": skinny}
        for s in splits:
            if s * rows <= 512:
                paths[f"skinny/{s}"] = lambda i, s=s: skinny(i, s)
        paths["a.sort+moe_gemm"] = grouped
        paths["b.gemv_moe_x"] = gemv_slices
        res = _alternate(paths, n, iters, warmup, repeats)
        default = int(hip.gemm_nf4_moe_skinny_splits(in_dim, out_dim, rows, EXPERTS, 0))
        tbs = nbytes * active / EXPERTS / res["skinny/0"][0] / 1e6
        out.append(dict(shape=name, rows=rows, active=active, default_splits=default, us=res, skinny_tbs=tbs))
        print(f"op {name:14s} R={rows:2d} active={active} S={default:2d} {tbs:.2f} TB/s  "
              + "  ".join(f"{n_} {m:7.1f} [{lo:.1f}..{hi:.1f}]" for n_, (m, lo, hi) in res.items()), flush=True)
    return out


def bench_block(model, iters, warmup, repeats):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    cfg = load_model_config(model)
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    fast = blk.eval().optimize_for_inference(quant="nf4")._fast
    os.environ["PETALS_AMD_WIDE_DECODE"] = "on"

    def empty_lru():
        fused_decode._dequant_cache = None
        fused_decode._dequant_cache_bytes = 0

    out = []
    for kv in (512, 4096):
        for B, T in ((12, 1), (16, 1), (32, 1), (4, 4)):
            ks, vs = blk.kv_cache_shape(B, kv + 64)
            k = torch.randn(ks, device="cuda", dtype=torch.bfloat16)
            v = torch.randn(vs, device="cuda", dtype=torch.bfloat16)
            h = torch.randn(B, T, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5
            wide = (lambda: fast.decode_step(h, k, v, kv)) if T == 1 else (lambda: fast.decode_multi(h, k, v, kv))
            runs = {
                "wide": lambda i: wide(),
                "forward/lru-warm": lambda i: fast.forward(h, (k, v), kv),
                "forward/lru-empty": lambda i: (empty_lru(), fast.forward(h, (k, v), kv)),
            }
            with torch.inference_mode():
                res = _alternate(runs, 1, iters, warmup, repeats)
            out.append(dict(model=model, B=B, T=T, kv=kv, us=res))
            print(f"block {model} nf4 B={B:2d} T={T} kv={kv:4d}  "
                  + "  ".join(f"{n_} {m:8.1f} [{lo:.1f}..{hi:.1f}] us" for n_, (m, lo, hi) in res.items()), flush=True)
    empty_lru()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["op", "block"], default=None)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--splits", type=int, nargs="*", default=list(SPLITS), help="split overrides to sweep")
    ap.add_argument("--model", default="mixtral-8x7b")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rotate-mb", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_moe_skinny needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
    result = {}
    if args.only in (None, "op"):
        result["op"] = [r for name in args.shapes
                        for r in bench_op(hip, name, args.iters, args.warmup, args.repeats, args.rotate_mb, args.seed,
                                           args.splits)]
    if args.only in (None, "block"):
        result["block"] = bench_block(args.model, args.iters, args.warmup, args.repeats)
    print(json.dumps({"benchmark": "moe_skinny", **result}))


if __name__ == "__main__":
    main()
