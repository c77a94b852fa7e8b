#!/usr/bin/env python3
"""Prefill projection GEMMs on quantized weights: fused dequant-in-LDS MFMA
GEMM (ops/csrc/gemm_quant.hip) against the two torch paths it can replace.

Per shape, quant mode and row count M, three paths are timed on the GPU:
  (a) resident   torch.matmul on a resident bf16 weight  (dequant-LRU hit)
  (b) dequant+mm dequantize, then torch.matmul           (dequant-LRU miss:
                 what a span larger than the LRU runs for every weight)
  (c) fused      gemm_nf4 / gemm_int8 on the packed weight

Method: random operands, every path warmed at every shape, the three paths
alternated inside one loop, one device-event pair per call, median over
--iters calls. TF/s counts 2*M*in*out only. Needs a GPU; there is no CPU
fallback."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# [in, out] of the fused projections
SHAPES = {
    "llama70b.qkv": (8192, 10240),
    "llama70b.o": (8192, 8192),
    "llama70b.gate_up": (8192, 57344),
    "llama70b.down": (28672, 8192),
    "falcon7b.qkv": (4544, 4672),
}
INT8_SHAPES = ("llama70b.qkv", "llama70b.gate_up")
ROWS = (16, 128, 256, 512, 2048)  # 256 and 512 bracket the dense/fused crossover


def _median_ms(samples):
    s = sorted(samples)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def bench_one(hip, name, quant, in_dim, out_dim, rows, iters, warmup, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    if quant == "nf4":
        packed, absmax = hip.nf4_quantize(w)

        def dequant():
            return hip.nf4_dequantize(packed, absmax)

        def fused(x):
            return hip.gemm_nf4(packed, absmax, x)
    else:
        wf = w.float()
        scale = wf.abs().amax(dim=0).clamp_min(1e-8) / 127.0
        q8 = torch.round(wf / scale).clamp(-127, 127).to(torch.int8).contiguous()
        scale8 = scale.to(torch.bfloat16).contiguous()
        del wf, scale

        def dequant():  # _FastWeight.dense() for int8
            return (q8.to(torch.float32) * scale8.float()).to(torch.bfloat16)

        def fused(x):
            return hip.gemm_int8(q8, scale8, x)
    del w
    resident = dequant()

    paths = {
        "resident": lambda x: torch.matmul(x, resident),
        "dequant+mm": lambda x: torch.matmul(x, dequant()),
        "fused": fused,
    }
    results = []
    for m in rows:
        x = torch.randn(m, in_dim, device="cuda", generator=g).to(torch.bfloat16)
        ref = paths["resident"](x).float()
        got = paths["fused"](x).float()
        max_diff = (got - ref).abs().max().item()
        ref_scale = ref.abs().max().item()
        times = {k: [] for k in paths}
        for it in range(warmup + iters):
            for k, fn in paths.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn(x)
                t1.record()
                t1.synchronize()
                if it >= warmup:
                    times[k].append(t0.elapsed_time(t1))
        med = {k: _median_ms(v) for k, v in times.items()}
        flops = 2.0 * m * in_dim * out_dim
        row = dict(
            shape=name, quant=quant, in_dim=in_dim, out_dim=out_dim, M=m,
            resident_ms=med["resident"], dequant_mm_ms=med["dequant+mm"], fused_ms=med["fused"],
            fused_tflops=flops / med["fused"] / 1e9,
            fused_over_dequant_mm=med["fused"] / med["dequant+mm"],
            fused_over_resident=med["fused"] / med["resident"],
            max_abs_diff_vs_resident=max_diff, ref_abs_max=ref_scale,
        )
        results.append(row)
        print(
            f"{name:18s} {quant:4s} M={m:5d}  (a) resident {med['resident']:8.3f} ms  "
            f"(b) dequant+mm {med['dequant+mm']:8.3f} ms  (c) fused {med['fused']:8.3f} ms "
            f"[{row['fused_tflops']:6.1f} TF/s]  c/b {row['fused_over_dequant_mm']:5.2f}  "
            f"c/a {row['fused_over_resident']:5.2f}  maxdiff {max_diff:.3g} (|ref| max {ref_scale:.3g})",
            flush=True,
        )
    return results


def bench_block(model, seq_lens, iters, warmup):
    """One NF4 block of `model`, prefill with a KV cache, per mode: dense with
    the dequant LRU hitting, dense with the LRU disabled (every matmul
    dequantizes: the state of a span larger than the LRU), and fused."""
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    cfg = load_model_config(model)
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    blk = blk.eval().optimize_for_inference(quant="nf4")
    modes = {
        "dense, LRU hit": dict(PETALS_AMD_PREFILL_GEMM="dense", PETALS_AMD_DEQUANT_CACHE_MB="16384"),
        "dense, LRU miss": dict(PETALS_AMD_PREFILL_GEMM="dense", PETALS_AMD_DEQUANT_CACHE_MB="0"),
        "fused": dict(PETALS_AMD_PREFILL_GEMM="fused", PETALS_AMD_DEQUANT_CACHE_MB="16384"),
    }
    saved = {k: os.environ.get(k) for k in ("PETALS_AMD_PREFILL_GEMM", "PETALS_AMD_DEQUANT_CACHE_MB")}
    results = []
    try:
        for S in seq_lens:
            ks, vs = blk.kv_cache_shape(1, S + 64)
            k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
            v = torch.zeros_like(k)
            x = torch.randn(1, S, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5
            times = {m: [] for m in modes}
            for it in range(warmup + iters):
                for m, env in modes.items():
                    os.environ.update(env)
                    if m != "dense, LRU hit":  # leave no cached copy behind for the next mode
                        fused_decode._dequant_cache = None
                        fused_decode._dequant_cache_bytes = 0
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.inference_mode():
                        if m == "dense, LRU hit":
                            blk(x, kv_cache=(k, v), prefix_length=0)  # fill the LRU outside the timing
                        t0.record()
                        blk(x, kv_cache=(k, v), prefix_length=0)
                        t1.record()
                    t1.synchronize()
                    if it >= warmup:
                        times[m].append(t0.elapsed_time(t1))
            med = {m: _median_ms(t) for m, t in times.items()}
            results.append(dict(model=model, S=S, **{m: med[m] for m in modes}))
            print(f"{model} NF4 block prefill S={S:5d}: " +
                  "  ".join(f"{m} {med[m]:8.3f} ms" for m in modes), flush=True)
    finally:
        for key, val in saved.items():
            if val is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = val
        fused_decode._dequant_cache = None
        fused_decode._dequant_cache_bytes = 0
    return results


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--iters", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--rows", type=int, nargs="+", default=list(ROWS))
    parser.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--block", metavar="MODEL", default=None,
                        help="also time one NF4 block of MODEL (e.g. llama-2-70b) per prefill mode")
    parser.add_argument("--block-seq", type=int, nargs="+", default=[16, 128, 256, 2048])
    args = parser.parse_args()

    if not torch.cuda.is_available():
        sys.exit("benchmark_prefill_gemm needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    if hip is None:
        sys.exit(f"HIP extension failed to load: {ops._hip_import_error!r}")
    print(f"device: {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} "
          f"(median of per-call device-event times)", flush=True)

    results = []
    for name in args.shapes:
        in_dim, out_dim = SHAPES[name]
        for quant in ("nf4", "int8"):
            if quant == "int8" and name not in INT8_SHAPES:
                continue
            results += bench_one(hip, name, quant, in_dim, out_dim, args.rows, args.iters, args.warmup, args.seed)
            torch.cuda.empty_cache()
    block_results = bench_block(args.block, args.block_seq, max(args.iters // 3, 3), 2) if args.block else []
    print(json.dumps({"benchmark": "prefill_gemm", "results": results, "block": block_results}))


if __name__ == "__main__":
    main()
