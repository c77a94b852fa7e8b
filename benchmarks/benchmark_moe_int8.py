#!/usr/bin/env python3
"""int8 Mixtral experts: device-routed kernels (ops/csrc/moe.hip
gemv_int8_moe, int8 moe_gemm) against the host-routed per-expert path.

Three parts, each at the Mixtral 8x7B and 8x22B shapes:
  sweep    gemv_int8_moe at explicit split counts derived from a range of
           workgroup targets (the sweep that fixes the kernel's default)
  decode   one block, one decode step at batch 1/4/8: host-routed eager
           (PETALS_AMD_MOE_INT8=host), device-routed eager, device-routed
           replayed from a captured graph
  prefill  one block's MLP at T = 16/128/1024: grouped int8 GEMM against the
           per-expert dense loop with the dequant LRU hitting and missing

Method: random operands, every path warmed, the paths alternated inside one
loop, one device-event pair per call, median over --iters calls. The sweep
rotates the selected experts per call so no expert stays cache-resident.
Needs a GPU; there is no CPU fallback."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

MODELS = ("mixtral-8x7b", "mixtral-8x22b")
TARGETS = (256, 512, 768, 1024, 1536, 2048, 3072, 4096)
EPI_PLAIN, EPI_SWIGLU = 0, 3


def _median_ms(samples):
    s = sorted(samples)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def _timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def _alternate(paths, iters, warmup):
    times = {k: [] for k in paths}
    for it in range(warmup + iters):
        for k, fn in paths.items():
            ms = _timed(lambda: fn(it))
            if it >= warmup:
                times[k].append(ms)
    return {k: _median_ms(v) for k, v in times.items()}


def sweep(hip, model, iters, warmup):
    from petals_amd.models.config_base import load_model_config

    cfg = load_model_config(model)
    H, I, E, K = cfg.hidden_size, cfg.intermediate_size, cfg.num_local_experts, cfg.num_experts_per_tok
    results = []
    for name, in_dim, out_dim, epi in (("gate_up", H, 2 * I, EPI_SWIGLU), ("down", I, H, EPI_PLAIN)):
        q8 = torch.randint(-127, 128, (E, in_dim, out_dim), device="cuda", dtype=torch.int8)
        s8 = (torch.rand(E, out_dim, device="cuda") * 1e-3 + 1e-4).to(torch.bfloat16)
        out_waves = -(-out_dim // 512)
        max_splits = -(-in_dim // 128)
        for B in (1, 4, 8):
            rows = B * K
            k_per_tok = K if name == "gate_up" else 1
            x = torch.randn(rows // k_per_tok, in_dim, device="cuda")
            ws = torch.empty(max_splits * rows * out_dim, device="cuda")
            sels = [
                torch.tensor([(2 * it + r) % E for r in range(rows)], dtype=torch.int32, device="cuda")
                for it in range(E)
            ]
            splits = {t: max(1, min(max_splits, -(-t // (out_waves * rows)))) for t in TARGETS}
            paths = {
                t: (lambda it, s=s: hip.gemv_int8_moe(q8, s8, x, sels[it % E], k_per_tok, ws, epi, s))
                for t, s in splits.items()
            }
            med = _alternate(paths, iters, warmup)
            default = hip.gemv_int8_moe_splits(in_dim, out_dim, rows)
            gb = rows * in_dim * out_dim / 1e9  # weight bytes read (distinct experts per row)
            print(f"{model} {name:7s} [{in_dim}x{out_dim}] rows={rows:2d} (default splits {default}): " +
                  "  ".join(f"T{t}/S{splits[t]} {med[t] * 1e3:6.1f}us" for t in TARGETS) +
                  f"   best {gb / (min(med.values()) * 1e-3):6.0f} GB/s", flush=True)
            results.append(dict(model=model, weight=name, in_dim=in_dim, out_dim=out_dim, rows=rows,
                                default_splits=default,
                                us={str(t): med[t] * 1e3 for t in TARGETS},
                                splits={str(t): splits[t] for t in TARGETS}))
        del q8, s8
        torch.cuda.empty_cache()
    return results


def _make_block(cfg, mode):
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    saved = os.environ.get("PETALS_AMD_MOE_INT8")
    os.environ["PETALS_AMD_MOE_INT8"] = mode
    try:
        blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
        init_random_block_(blk, cfg, 0)
        return blk.eval().optimize_for_inference(quant="int8")
    finally:
        if saved is None:
            os.environ.pop("PETALS_AMD_MOE_INT8", None)
        else:
            os.environ["PETALS_AMD_MOE_INT8"] = saved


def block_bench(model, iters, warmup, prefill_rows):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config(model)
    H = cfg.hidden_size
    blk_host, blk_dev = _make_block(cfg, "host"), _make_block(cfg, "device")
    assert blk_dev._fast.graph_safe and not blk_host._fast.graph_safe
    decode, prefill = [], []

    with torch.inference_mode():
        for B in (1, 4, 8):
            ks, vs = blk_dev.kv_cache_shape(B, 256)
            caches = [(torch.zeros(ks, device="cuda", dtype=torch.bfloat16),
                       torch.zeros(vs, device="cuda", dtype=torch.bfloat16)) for _ in range(3)]
            xs = [torch.randn(B, 1, H, device="cuda", dtype=torch.bfloat16) * 0.5 for _ in range(8)]
            ctx = DecodeContext(torch.device("cuda"))
            ctx.set_position(128)
            h_in = torch.empty_like(xs[0])
            graph = GraphedCallable(lambda: blk_dev(h_in, kv_cache=caches[2], ctx=ctx), [])

            def graphed(it):
                h_in.copy_(xs[it % 8])
                graph.replay()

            paths = {
                "host eager": lambda it: blk_host(xs[it % 8], kv_cache=caches[0], prefix_length=128),
                "device eager": lambda it: blk_dev(xs[it % 8], kv_cache=caches[1], prefix_length=128),
                "device graph": graphed,
            }
            med = _alternate(paths, iters, warmup)
            decode.append(dict(model=model, batch=B, **{k: med[k] for k in paths}))
            print(f"{model} int8 block decode B={B}: " +
                  "  ".join(f"{k} {med[k] * 1e3:7.1f} us" for k in paths), flush=True)

        env_keys = ("PETALS_AMD_DEQUANT_CACHE_MB",)
        saved = {k: os.environ.get(k) for k in env_keys}
        try:
            for T in prefill_rows:
                x = torch.randn(1, T, H, device="cuda", dtype=torch.bfloat16) * 0.5

                def dense(it, budget, prefill_lru):
                    os.environ["PETALS_AMD_DEQUANT_CACHE_MB"] = budget
                    if not prefill_lru:  # leave no cached copy behind
                        fused_decode._dequant_cache = None
                        fused_decode._dequant_cache_bytes = 0
                    return blk_host._fast._mlp_dense(x, None, False)

                os.environ["PETALS_AMD_DEQUANT_CACHE_MB"] = "16384"
                blk_host._fast._mlp_dense(x, None, False)  # fill the LRU outside the timing
                ref = blk_host._fast._mlp_dense(x, None, False).float()
                got = blk_dev._fast._mlp_dense(x, None, False).float()
                diff = (got - ref).abs().max().item()
                # "hit" runs right after a fill; "miss" clears the LRU and disables it
                times = {"grouped": [], "dense, LRU hit": [], "dense, LRU miss": []}
                for it in range(warmup + iters):
                    os.environ["PETALS_AMD_DEQUANT_CACHE_MB"] = "16384"
                    blk_host._fast._mlp_dense(x, None, False)
                    ms = {
                        "dense, LRU hit": _timed(lambda: dense(it, "16384", True)),
                        "grouped": _timed(lambda: blk_dev._fast._mlp_dense(x, None, False)),
                        "dense, LRU miss": _timed(lambda: dense(it, "0", False)),
                    }
                    if it >= warmup:
                        for k, v in ms.items():
                            times[k].append(v)
                med = {k: _median_ms(v) for k, v in times.items()}
                prefill.append(dict(model=model, T=T, max_abs_diff=diff, ref_abs_max=ref.abs().max().item(), **med))
                print(f"{model} int8 block MLP prefill T={T:5d}: " +
                      "  ".join(f"{k} {med[k]:8.3f} ms" for k in med) +
                      f"  maxdiff {diff:.3g} (|ref| max {ref.abs().max().item():.3g})", flush=True)
        finally:
            for key, val in saved.items():
                if val is None:
                    os.environ.pop(key, None)
                else:
                    os.environ[key] = val
            fused_decode._dequant_cache = None
            fused_decode._dequant_cache_bytes = 0
    del blk_host, blk_dev
    torch.cuda.empty_cache()
    return decode, prefill


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--iters", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    parser.add_argument("--parts", nargs="+", default=["sweep", "block"], choices=["sweep", "block"])
    parser.add_argument("--prefill-rows", type=int, nargs="+", default=[16, 128, 1024])
    args = parser.parse_args()

    if not torch.cuda.is_available():
        sys.exit("benchmark_moe_int8 needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    if hip is None:
        sys.exit(f"HIP extension failed to load: {ops._hip_import_error!r}")
    print(f"device: {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} "
          f"(median of per-call device-event times)", flush=True)

    out = dict(benchmark="moe_int8", sweep=[], decode=[], prefill=[])
    for model in args.models:
        if "sweep" in args.parts:
            out["sweep"] += sweep(hip, model, args.iters, args.warmup)
        if "block" in args.parts:
            d, p = block_bench(model, args.iters, args.warmup, args.prefill_rows)
            out["decode"] += d
            out["prefill"] += p
    print(json.dumps(out))


if __name__ == "__main__":
    main()
