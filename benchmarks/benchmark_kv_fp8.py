#!/usr/bin/env python3
"""FP8 (OCP E4M3) KV cache against the bf16 cache.

  decode  llama-70b decode attention (B = 1, KV = 8, GQ = 8, HD = 128) at
          kv = 4k / 32k / 131k: attn_decode_fused on a bf16 cache and on an
          fp8 cache holding the same values. us and GB/s (K + V bytes of the
          format over kv_len rows).
  block   one llama-70b block decode step, hipGraph-replayed, at kv position 8
          and 32k, on a bf16 and on an fp8 cache.
  error   CPU, float64: worst-row nerr of attention over round-tripped K/V
          against attention over the unquantized K/V, on the "sharp" decode
          table of tests/test_attention_numerics.py.

Method: the two formats alternate inside one loop, one device-event pair per
call, median over --iters calls after --warmup. The decode caches rotate
through --rotate-mb of copies per format (more than L2 plus the 256 MB cache)
and every call takes the next copy, so no call finds its cache resident.
Needs a GPU except for `--only error`."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

KV_LENS = (4096, 32768, 131072)
KVH, GQ, HD = 8, 8, 128


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


def bench_decode(hip, kv_len, iters, warmup, rotate_mb, seed):
    from petals_amd.ops import kv_fp8

    g = torch.Generator(device="cuda").manual_seed(seed)
    shape = (1, KVH, kv_len, HD)
    fp8_bytes = 2 * KVH * kv_len * HD  # K + V, one byte per element
    n = max(2, -(-(rotate_mb << 20) // fp8_bytes))
    k16 = kv_fp8.roundtrip(torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16))
    v16 = kv_fp8.roundtrip(torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16))
    caches = {
        "bf16": [(k16.clone(), v16.clone()) for _ in range(n)],
        "fp8": [(kv_fp8.quantize(k16), kv_fp8.quantize(v16)) for _ in range(n)],
    }
    q = torch.randn(1, KVH * GQ * HD, device="cuda", generator=g)
    kv_len_t = torch.tensor([kv_len], dtype=torch.int32, device="cuda")
    empty = torch.empty(0, device="cuda")
    scale = HD**-0.5

    def run(fmt, i):
        k, v = caches[fmt][i]
        return hip.attn_decode_fused(q, k, v, kv_len_t, GQ, 0, empty, empty, scale, None)

    same = torch.equal(run("bf16", 0), run("fp8", 0))
    times = {fmt: [] for fmt in caches}
    call = 0
    for it in range(warmup + iters):
        for fmt in caches:
            call += 1
            t = _timed(lambda: run(fmt, call % n))
            if it >= warmup:
                times[fmt].append(t)
    med = {fmt: _median(v) for fmt, v in times.items()}
    gbs = {"bf16": 2 * fp8_bytes / med["bf16"] / 1e3, "fp8": fp8_bytes / med["fp8"] / 1e3}
    print(f"decode kv={kv_len:6d} copies={n:3d}  bf16 {med['bf16']:7.1f} us {gbs['bf16']:7.1f} GB/s | "
          f"fp8 {med['fp8']:7.1f} us {gbs['fp8']:7.1f} GB/s | fp8/bf16 time {med['fp8'] / med['bf16']:.2f} | "
          f"outputs bit-identical: {same}", flush=True)
    return dict(kv_len=kv_len, copies=n, us=med, gbs=gbs, bit_identical=same)


def bench_block(model, positions, iters, warmup):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config(model)
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    blk = blk.eval().optimize_for_inference()
    lmax = max(positions) + 64
    ks, vs = blk.kv_cache_shape(1, lmax)
    g = torch.Generator(device="cuda").manual_seed(1)
    h = (torch.randn(1, 1, cfg.hidden_size, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    runs = {}
    for fmt, dt in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
        k = torch.randn(ks, device="cuda", generator=g).to(dt)
        v = torch.randn(vs, device="cuda", generator=g).to(dt)
        ctx = DecodeContext(torch.device("cuda"))
        ctx.set_position(positions[0])
        with torch.no_grad():
            graph = GraphedCallable(lambda k=k, v=v, ctx=ctx: blk(h, kv_cache=(k, v), ctx=ctx), [])
        runs[fmt] = (graph, ctx)
    rows = []
    for pos in positions:
        times = {fmt: [] for fmt in runs}
        for it in range(warmup + iters):
            for fmt, (graph, ctx) in runs.items():
                ctx.set_position(pos)
                t = _timed(graph.replay)
                if it >= warmup:
                    times[fmt].append(t)
        med = {fmt: _median(v) for fmt, v in times.items()}
        rows.append(dict(model=model, position=pos, us=med))
        print(f"block {model} graph, kv position {pos:6d}  bf16 {med['bf16']:7.1f} us | fp8 {med['fp8']:7.1f} us | "
              f"fp8/bf16 time {med['fp8'] / med['bf16']:.3f}", flush=True)
    return rows


def quantization_error():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_attention_numerics import DECODE_CASES, decode_inputs, nerr, ref_attention_f64

    from petals_amd.ops import kv_fp8

    worst, where = 0.0, None
    for case in DECODE_CASES:
        inp = decode_inputs(case, "sharp")
        out = ref_attention_f64(inp.q, kv_fp8.roundtrip(inp.k), kv_fp8.roundtrip(inp.v), inp.kv_len, inp.scale,
                                slopes=inp.slopes)
        e = nerr(out, inp.ref)
        print(f"error {case.id:48s} nerr(quantized K/V, unquantized) = {e:.4f}", flush=True)
        if e > worst:
            worst, where = e, case.id
    print(f"error worst-row nerr {worst:.3f} at {where}", flush=True)
    return dict(worst=worst, where=where)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["decode", "block", "error"], default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=768)
    ap.add_argument("--model", default="llama-2-70b")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    result = {}
    if args.only in (None, "error"):
        result["error"] = quantization_error()
    if args.only != "error":
        from petals_amd import ops

        hip = ops._load_hip_ops()
        assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
        print(f"device {torch.cuda.get_device_name(0)}", flush=True)
        if args.only in (None, "decode"):
            result["decode"] = [bench_decode(hip, n, args.iters, args.warmup, args.rotate_mb, args.seed) for n in KV_LENS]
        if args.only in (None, "block"):
            result["block"] = bench_block(args.model, (8, 32768), args.iters, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
