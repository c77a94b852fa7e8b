#!/usr/bin/env python3
"""Training attention: PETALS_AMD_TRAIN_ATTN=fused against the torch composition.

  attn    forward + backward of causal GQA attention (B = 1, HD = 128) at the
          llama-70b (QH 64, KVH 8) and Mixtral (QH 32, KVH 8) geometries,
          S = 128 / 512 / 1024: `ops.attention` under autograd in both modes.
          Median device time and torch.cuda.max_memory_allocated above the
          inputs, per mode.
  split   attn_train_bwd alone with the q heads of a kv head summed in
          registers (gq_splits 1) against the kernel's own split policy (0).
  block   one TransformerBackend.backward of a llama-70b bf16 block at
          S = 1024 in both modes.

Method: the contenders alternate inside one loop, one device-event pair per
call, median over --iters calls after --warmup. Needs a GPU."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

GEOMETRIES = {"llama-70b": (64, 8), "mixtral": (32, 8)}
SEQS = (128, 512, 1024)
HD = 128


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


def _alternate(fns, iters, warmup):
    """{name: median us}; the contenders take turns inside one loop."""
    samples = {name: [] for name in fns}
    for i in range(warmup + iters):
        for name, fn in fns.items():
            t = _timed(fn)
            if i >= warmup:
                samples[name].append(t)
    return {name: _median(v) for name, v in samples.items()}


def _peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def _inputs(qh, kvh, s, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda h: torch.randn(1, h, s, HD, device="cuda", generator=g).to(torch.bfloat16)
    return mk(qh), mk(kvh), mk(kvh), mk(qh)


def bench_attn(name, s, iters, warmup, seed):
    from petals_amd import ops

    qh, kvh = GEOMETRIES[name]
    q, k, v, do = _inputs(qh, kvh, s, seed)

    def step(mode):
        os.environ["PETALS_AMD_TRAIN_ATTN"] = mode
        ql, kl, vl = (t.detach().requires_grad_() for t in (q, k, v))
        ops.attention(ql, kl, vl, causal=True).backward(do)
        return ql.grad, kl.grad, vl.grad

    gt, gf = step("torch"), step("fused")
    rel = max(((a.float() - b.float()).abs().max() / b.float().abs().max()).item() for a, b in zip(gf, gt))
    us = _alternate({m: (lambda m=m: step(m)) for m in ("torch", "fused")}, iters, warmup)
    mib = {m: _peak_mib(lambda m=m: step(m)) for m in ("torch", "fused")}
    return {"geometry": name, "s": s, "torch_us": us["torch"], "fused_us": us["fused"],
            "torch_peak_mib": mib["torch"], "fused_peak_mib": mib["fused"], "grad_rel_to_max": rel}


def bench_split(hip, name, s, iters, warmup, seed):
    qh, kvh = GEOMETRIES[name]
    q, k, v, do = _inputs(qh, kvh, s, seed)
    scale = HD**-0.5
    out, lse2 = hip.attn_train_fwd(q, k, v, scale)
    us = _alternate({f"gq_splits_{n}": (lambda n=n: hip.attn_train_bwd(q, k, v, out, lse2, do, scale, n))
                     for n in (1, 0)}, iters, warmup)
    return {"geometry": name, "s": s, "bwd_registers_us": us["gq_splits_1"], "bwd_auto_us": us["gq_splits_0"]}


def bench_block(s, iters, warmup, seed):
    from types import SimpleNamespace

    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.backend import TransformerBackend
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    cfg = load_model_config("llama-2-70b")
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    blk = blk.eval().optimize_for_inference()
    backend = SimpleNamespace(block=blk)  # backward() touches nothing else of the backend
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (0.5 * torch.randn(1, s, cfg.hidden_size, device="cuda", generator=g)).to(torch.bfloat16)
    dy = torch.randn(1, s, cfg.hidden_size, device="cuda", generator=g).to(torch.bfloat16)

    def step(mode):
        os.environ["PETALS_AMD_TRAIN_ATTN"] = mode
        return TransformerBackend.backward(backend, x, dy)[0]

    gt, gf = step("torch").float(), step("fused").float()
    rel = ((gf - gt).abs().max() / gt.abs().max()).item()
    us = _alternate({m: (lambda m=m: step(m)) for m in ("torch", "fused")}, iters, warmup)
    mib = {m: _peak_mib(lambda m=m: step(m)) for m in ("torch", "fused")}
    return {"block": "llama-2-70b", "s": s, "torch_us": us["torch"], "fused_us": us["fused"],
            "torch_peak_mib": mib["torch"], "fused_peak_mib": mib["fused"], "grad_rel_to_max": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", choices=["attn", "split", "block"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_attn_backward needs a GPU")
    from petals_amd import ops

    hip = ops._load_hip_ops()
    assert hip is not None, ops._hip_import_error
    saved = os.environ.get("PETALS_AMD_TRAIN_ATTN")
    res = {"benchmark": "attn_backward", "attn": [], "split": [], "block": []}
    for name in GEOMETRIES:
        for s in SEQS:
            if args.only in (None, "attn"):
                res["attn"].append(bench_attn(name, s, args.iters, args.warmup, args.seed))
                print(res["attn"][-1], flush=True)
            if args.only in (None, "split"):
                res["split"].append(bench_split(hip, name, s, args.iters, args.warmup, args.seed))
                print(res["split"][-1], flush=True)
    if args.only in (None, "block"):
        res["block"].append(bench_block(1024, args.iters, args.warmup, args.seed))
        print(res["block"][-1], flush=True)
    if saved is None:
        os.environ.pop("PETALS_AMD_TRAIN_ATTN", None)
    else:
        os.environ["PETALS_AMD_TRAIN_ATTN"] = saved
    print(json.dumps(res))


if __name__ == "__main__":
    main()
