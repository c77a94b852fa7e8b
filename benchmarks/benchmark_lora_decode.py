#!/usr/bin/env python3
"""One llama-70b NF4 block decode step under a LoRA adapter: the torch deltas
around each GEMV (PETALS_AMD_LORA_DECODE=torch, the default) against the fused
shrink + expand-in-the-reduce kernels (`fused`), with the adapter-free step as
the yardstick.

  step   decode_step at B = 1 / 4, kv = 512 / 4096, eager and as a captured
         graph; adapters of rank 16 on all seven projections (`all7`) and on q
         and v only (`qv`).
  multi  a T = 4 step at B = 1: decode_multi without an adapter and with `all7`
         fused, and LlamaFastPath.forward under the adapter (what such a step
         takes without the fused kernels).

Method (benchmark_multi_decode.py's): the paths alternate inside one loop, one
device-event pair per call, median over --iters calls after --warmup, each cell
measured --repeats times (all medians are printed). Calls go round two blocks'
weights (2 x ~0.4 GB of NF4, past the 256 MiB Infinity Cache), each block with
its own KV cache. Needs a GPU."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from benchmark_multi_decode import _alternate, _median

BATCHES = (1, 4)
KV_LENS = (512, 4096)
RANK = 16
ADAPTERS = {"all7": ("q", "k", "v", "o", "gate", "up", "down"), "qv": ("q", "v")}


def make_adapter(block, name, keys, g):
    from petals_amd.utils.peft import BlockAdapter, add_adapter_to_block

    cfg = block.config
    hd = cfg.head_dim
    qd, kd, hid, inter = cfg.num_attention_heads * hd, cfg.n_kv_heads * hd, cfg.hidden_size, cfg.intermediate_size
    shapes = dict(q=(hid, qd), k=(hid, kd), v=(hid, kd), o=(qd, hid), gate=(hid, inter), up=(hid, inter),
                  down=(inter, hid))
    proj = {}
    for key in keys:
        n_in, n_out = shapes[key]
        proj[key] = (torch.randn(RANK, n_in, generator=g) * 0.02, torch.randn(n_out, RANK, generator=g) * 0.02, 2.0)
    ad = BlockAdapter(name, proj)
    add_adapter_to_block(block, ad)
    return ad


def _with_mode(mode, fn):
    def run(i):
        os.environ["PETALS_AMD_LORA_DECODE"] = mode
        return fn(i)

    return run


def _row(tag, med):
    base = _median(med["none"])
    cells = " | ".join(f"{name} {'/'.join(f'{u:.1f}' for u in us)}" for name, us in med.items())
    ratios = " ".join(
        f"{name}/none {_median(us) / base:.2f}" for name, us in med.items() if name != "none"
    )
    verdict = []
    for ad in ADAPTERS:
        t, f = med.get(f"torch_{ad}"), med.get(f"fused_{ad}")
        if t and f:  # a win: every fused repeat under every torch repeat
            verdict.append(f"{ad}: fused {'wins' if max(f) < min(t) else 'DOES NOT WIN'} ({_median(t) / _median(f):.2f}x)")
    print(f"{tag}  us: {cells} | {ratios} | {'; '.join(verdict)}", flush=True)


def bench_step(blocks, adapters, batch, kv_len, graphed, args):
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.utils.graphs import GraphedCallable

    fasts = [b._fast for b in blocks]
    cfg = blocks[0].config
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    ks, _ = blocks[0].kv_cache_shape(batch, kv_len)
    caches = [(torch.randn(ks, device="cuda", generator=g).to(torch.bfloat16),
               torch.randn(ks, device="cuda", generator=g).to(torch.bfloat16)) for _ in fasts]
    h = (torch.randn(batch, 1, cfg.hidden_size, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    pre = kv_len - 1
    variants = {"none": ("torch", None)}
    for ad in ADAPTERS:
        variants[f"torch_{ad}"] = ("torch", ad)
        variants[f"fused_{ad}"] = ("fused", ad)

    paths = {}
    for name, (mode, ad) in variants.items():
        if graphed:
            graphs = []
            for j, fast in enumerate(fasts):
                ctx = DecodeContext(torch.device("cuda:0"))
                ctx.set_position(pre)
                os.environ["PETALS_AMD_LORA_DECODE"] = mode
                adapter = adapters[j][ad] if ad else None
                graphs.append(GraphedCallable(
                    lambda fast=fast, j=j, ctx=ctx, adapter=adapter: fast.decode_step(
                        h, caches[j][0], caches[j][1], ctx=ctx, adapter=adapter), []))
            paths[name] = lambda i, graphs=graphs: graphs[i % 2].replay()
        else:
            paths[name] = _with_mode(mode, lambda i, ad=ad: fasts[i % 2].decode_step(
                h, caches[i % 2][0], caches[i % 2][1], pre, adapter=adapters[i % 2][ad] if ad else None))
    with torch.inference_mode():
        outs = {name: fn(0).float().clone() for name, fn in paths.items()}
        med = _alternate(paths, args.iters, args.warmup, args.repeats)
    diffs = " ".join(f"{ad} {(outs[f'fused_{ad}'] - outs[f'torch_{ad}']).abs().max().item():.4f}" for ad in ADAPTERS)
    _row(f"step  {'graph' if graphed else 'eager'} B={batch} kv={kv_len:5d}", med)
    print(f"      max |fused - torch| (bf16 outputs): {diffs}", flush=True)
    return dict(batch=batch, kv_len=kv_len, graphed=graphed, us=med)


def bench_multi(blocks, adapters, kv_len, args, t_n=4):
    fasts = [b._fast for b in blocks]
    cfg = blocks[0].config
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    ks, _ = blocks[0].kv_cache_shape(1, kv_len)
    caches = [(torch.randn(ks, device="cuda", generator=g).to(torch.bfloat16),
               torch.randn(ks, device="cuda", generator=g).to(torch.bfloat16)) for _ in fasts]
    h = (torch.randn(1, t_n, cfg.hidden_size, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    pre = kv_len - t_n
    paths = {
        "none": _with_mode("torch", lambda i: fasts[i % 2].decode_multi(h, *caches[i % 2], pre)),
        "fused_all7": _with_mode("fused", lambda i: fasts[i % 2].decode_multi(
            h, *caches[i % 2], pre, adapter=adapters[i % 2]["all7"])),
        "forward_all7": _with_mode("torch", lambda i: fasts[i % 2].forward(
            h, caches[i % 2], pre, adapter=adapters[i % 2]["all7"])),
    }
    with torch.inference_mode():
        diff = (paths["fused_all7"](0).float() - paths["forward_all7"](0).float()).abs().max().item()
        med = _alternate(paths, args.iters, args.warmup, args.repeats)
    _row(f"multi eager B=1 T={t_n} kv={kv_len:5d}", med)
    print(f"      max |decode_multi fused - forward| under the adapter = {diff:.4f}", flush=True)
    return dict(tokens=t_n, kv_len=kv_len, us=med)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="llama-2-70b")
    ap.add_argument("--quant", default="nf4")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_lora_decode needs a GPU")
    from petals_amd import ops
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    hip = ops._load_hip_ops()
    assert hip is not None, f"HIP extension must load: {ops._hip_import_error!r}"
    print(f"device {torch.cuda.get_device_name(0)}", flush=True)
    cfg = load_model_config(args.model)
    blocks, adapters = [], []
    g = torch.Generator().manual_seed(args.seed)
    for i in range(2):
        blk = build_empty_block(cfg, i, "cuda:0", torch.bfloat16)
        init_random_block_(blk, cfg, i)
        blocks.append(blk.eval().optimize_for_inference(quant=args.quant))
        adapters.append({name: make_adapter(blocks[i], name, keys, g) for name, keys in ADAPTERS.items()})
    before = os.environ.get("PETALS_AMD_LORA_DECODE")
    try:
        steps = [bench_step(blocks, adapters, b, n, graphed, args)
                 for graphed in (False, True) for b in BATCHES for n in KV_LENS]
        multi = [bench_multi(blocks, adapters, n, args) for n in KV_LENS]
    finally:
        if before is None:
            os.environ.pop("PETALS_AMD_LORA_DECODE", None)
        else:
            os.environ["PETALS_AMD_LORA_DECODE"] = before
    print(json.dumps({"benchmark": "lora_decode", "step": steps, "multi": multi}))


if __name__ == "__main__":
    main()
