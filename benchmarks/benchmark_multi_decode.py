#!/usr/bin/env python3
"""A step of T = 2 / 4 / 8 new tokens against a long KV cache (a speculative
verify step): the prefill path every such step takes by default against the
multi-token decode chain (PETALS_AMD_MULTI_DECODE=on), B = 1.

  attn   attention alone at the llama-70b shape (KV 8, GQ 8, HD 128), kv = 512 /
         4096 / 32768: attn_prefill_fused on [1, 64, T, 128] against
         attn_decode_multi.
  block  one llama-70b NF4 block step: LlamaFastPath.forward with the dequant
         LRU warm (`fwd_hit`) and emptied before every call (`fwd_miss`),
         decode_multi (`multi`), and T successive decode_steps (`T x step`, the
         no-speculation yardstick).

Method: the paths alternate inside one loop, one device-event pair per call,
median over --iters calls after --warmup, and each cell is measured --repeats
times (all medians are printed). Caches rotate through --rotate-mb of copies
and the block paths through two blocks' weights, and every call takes the next
copy, so no call finds its cache or weights resident. Needs a GPU."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

TOKENS = (2, 4, 8)
KV_LENS = (512, 4096, 32768)
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


def _alternate(paths, iters, warmup, repeats):
    """paths: name -> fn(call_index). Returns name -> [median us per repeat]."""
    out = {name: [] for name in paths}
    call = 0
    for _ in range(repeats):
        times = {name: [] for name in paths}
        for it in range(warmup + iters):
            for name, fn in paths.items():
                call += 1
                t = _timed(lambda: fn(call))
                if it >= warmup:
                    times[name].append(t)
        for name, v in times.items():
            out[name].append(round(_median(v), 1))
    return out


def _row(tag, t_n, kv_len, med, base):
    cells = " | ".join(f"{name} {'/'.join(f'{u:.1f}' for u in us)} us" for name, us in med.items())
    ratios = " ".join(f"{name}/{base} {_median(us) / _median(med[base]):.2f}" for name, us in med.items() if name != base)
    print(f"{tag} T={t_n} kv={kv_len:6d}  {cells} | {ratios}", flush=True)
    return dict(tokens=t_n, kv_len=kv_len, us=med)


def bench_attn(hip, t_n, kv_len, args):
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    n = max(2, -(-(args.rotate_mb << 20) // (2 * KVH * kv_len * HD * 2)))
    k = torch.randn(n, 1, KVH, kv_len, HD, device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn(n, 1, KVH, kv_len, HD, device="cuda", generator=g).to(torch.bfloat16)
    q = torch.randn(t_n, KVH * GQ * HD, device="cuda", generator=g)  # token-major f32, the decode chain's q
    q_pre = q.view(1, t_n, KVH * GQ, HD).transpose(1, 2).to(torch.bfloat16).contiguous()  # [1, qh, T, hd]
    pos = torch.tensor([kv_len - t_n], dtype=torch.int32, device="cuda")
    empty = torch.empty(0, device="cuda")
    scale = HD**-0.5
    paths = {
        "prefill": lambda i: hip.attn_prefill_fused(q_pre, k[i % n], v[i % n], kv_len, kv_len - t_n, scale, True),
        "multi": lambda i: hip.attn_decode_multi(q, k[i % n], v[i % n], pos, t_n, GQ, 0, empty, empty, scale),
    }
    a = paths["prefill"](0).float().transpose(1, 2).reshape(t_n, -1)
    diff = (a - paths["multi"](0)).abs().max().item()
    row = _row("attn ", t_n, kv_len, _alternate(paths, args.iters, args.warmup, args.repeats), "prefill")
    print(f"      max |prefill - multi| = {diff:.4f} (bf16 output vs f32)", flush=True)
    return row


def bench_block(blocks, t_n, kv_len, args):
    from petals_amd.ops import fused_decode

    fasts = [b._fast for b in blocks]
    cfg = blocks[0].config
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    ks, _ = blocks[0].kv_cache_shape(1, kv_len)
    n = max(2, -(-(args.rotate_mb << 20) // (2 * ks[1] * kv_len * ks[3] * 2)))
    k = torch.randn((n,) + tuple(ks), device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn((n,) + tuple(ks), device="cuda", generator=g).to(torch.bfloat16)
    h = (torch.randn(1, t_n, cfg.hidden_size, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    pre = kv_len - t_n

    def forward(i):
        return fasts[i % 2].forward(h, (k[i % n], v[i % n]), pre)

    def forward_miss(i):
        if fused_decode._dequant_cache:
            fused_decode._dequant_cache.clear()
            fused_decode._dequant_cache_bytes = 0
        return forward(i)

    def steps(i):
        for t in range(t_n):
            out = fasts[i % 2].decode_step(h[:, t : t + 1], k[i % n], v[i % n], pre + t)
        return out

    paths = {
        "fwd_hit": forward,
        "multi": lambda i: fasts[i % 2].decode_multi(h, k[i % n], v[i % n], pre),
        f"{t_n}xstep": steps,
    }
    with torch.inference_mode():
        diff = (forward(0).float() - paths["multi"](0).float()).abs().max().item()
        med = _alternate(paths, args.iters, args.warmup, args.repeats)
        # the miss path empties the LRU, so it is timed apart from the hit path
        med.update(_alternate({"fwd_miss": forward_miss}, args.iters, args.warmup, args.repeats))
    row = _row("block", t_n, kv_len, med, "fwd_hit")
    print(f"      max |forward - decode_multi| = {diff:.4f}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["attn", "block"], default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rotate-mb", type=int, default=768)
    ap.add_argument("--model", default="llama-2-70b")
    ap.add_argument("--quant", default="nf4")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_multi_decode needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    result = {}
    if args.only in (None, "attn"):
        result["attn"] = [bench_attn(hip, t, n, args) for t in TOKENS for n in KV_LENS]
    if args.only in (None, "block"):
        from petals_amd.models.config_base import load_model_config
        from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

        cfg = load_model_config(args.model)
        blocks = []
        for i in range(2):
            blk = build_empty_block(cfg, i, "cuda:0", torch.bfloat16)
            init_random_block_(blk, cfg, i)
            blocks.append(blk.eval().optimize_for_inference(quant=args.quant))
        result["block"] = [bench_block(blocks, t, n, args) for t in TOKENS for n in KV_LENS]
    print(json.dumps({"benchmark": "multi_decode", **result}))


if __name__ == "__main__":
    main()
