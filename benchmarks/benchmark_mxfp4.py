#!/usr/bin/env python3
"""MXFP4 weights against NF4 (and int8): decode GEMV, one block decode step,
prefill GEMM, and the quantization error of both 4-bit formats.

  gemv   llama-70b projections, batch 1/4/8: gemv_mxfp4 over a sweep of split
         counts (the default target is marked) against the unchanged gemv_nf4,
         in one process. us and packed TB/s (weight + scale bytes) for both.
  block  one llama-70b block decode step, eager and hipGraph-replayed, for
         nf4, mxfp4 and int8.
  gemm   prefill rows M: resident rocBLAS, mxfp4_dequantize + rocBLAS, fused
         gemm_mxfp4. FUSED_GEMM_MAX_ROWS["mxfp4"] is the largest M at which
         fused beats dequantize + rocBLAS on every shape.
  error  relative RMS of round-tripped N(0, 0.02^2) weights, on the CPU.

Method: the paths under comparison alternate inside one loop, one
device-event pair per call, median over --iters calls. The GEMV and GEMM
operands rotate through --rotate-mb of weight copies (more than L2 plus the
256 MB cache) and every call takes the next copy, so no call finds its weight
resident. Needs a GPU except for
`--only error`."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

SHAPES = {  # [in, out] of the fused projections
    "llama70b.qkv": (8192, 10240),
    "llama70b.o": (8192, 8192),
    "llama70b.gate_up": (8192, 57344),
    "llama70b.down": (28672, 8192),
}
BATCHES = (1, 4, 8)
SPLITS = (0, 4, 8, 16, 24, 32, 48, 64)  # 0 = the op's default target
ROWS = (16, 128, 256, 512, 2048)


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


def _copies(packed_bytes, rotate_mb):
    return max(2, -(-(rotate_mb << 20) // packed_bytes))


def bench_gemv(hip, name, in_dim, out_dim, iters, warmup, rotate_mb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    mxp, mxs = hip.mxfp4_quantize(w)
    nfp, nfa = hip.nf4_quantize(w)
    del w
    mx_bytes = mxp.numel() + mxs.numel()
    nf_bytes = nfp.numel() + nfa.numel() * 2
    n = _copies(min(mx_bytes, nf_bytes), rotate_mb)
    mx_w = [(mxp.clone(), mxs.clone()) for _ in range(n)]
    nf_w = [(nfp.clone(), nfa.clone(), nfa.t().contiguous()) for _ in range(n)]
    ws = torch.empty(64 * 8 * out_dim, device="cuda")
    rows = []
    for B in BATCHES:
        x = torch.randn(B, in_dim, device="cuda", generator=g)
        paths = {}
        for s in SPLITS:
            if s * 32 > in_dim:
                continue
            paths[f"mxfp4/{s}"] = lambda i, s=s: hip.gemv_mxfp4(mx_w[i][0], mx_w[i][1], x, ws, None, 0, s, None)
        # the NF4 comparator at its own default and at the splits its autotune picks among
        for s in (0, 64, 128, 256):
            paths[f"nf4/{s}"] = lambda i, s=s: hip.gemv_nf4(
                nf_w[i][0], nf_w[i][1], x, ws, None, 0, s, None, nf_w[i][2], None, 0.0, None)
        times = {k: [] for k in paths}
        call = 0  # every call takes the next copy: a copy returns after n other weights went by
        for it in range(warmup + iters):
            for k, fn in paths.items():
                call += 1
                t = _timed(lambda: fn(call % n))
                if it >= warmup:
                    times[k].append(t)
        med = {k: _median(v) for k, v in times.items()}
        best_mx = min((k for k in med if k.startswith("mxfp4/")), key=med.get)
        best_nf = min((k for k in med if k.startswith("nf4/")), key=med.get)
        row = dict(shape=name, in_dim=in_dim, out_dim=out_dim, B=B, us=med,
                   default_splits=int(hip.gemv_mxfp4_splits(in_dim, out_dim, B, 0)),
                   best_mxfp4=best_mx, best_nf4=best_nf,
                   mxfp4_tbs=mx_bytes / med[best_mx] / 1e6, nf4_tbs=nf_bytes / med[best_nf] / 1e6,
                   mxfp4_default_tbs=mx_bytes / med["mxfp4/0"] / 1e6)
        rows.append(row)
        print(f"gemv {name:17s} B={B}  " + "  ".join(f"{k} {v:7.1f}" for k, v in med.items()), flush=True)
        print(f"gemv {name:17s} B={B}  best {best_mx} {med[best_mx]:7.1f} us {row['mxfp4_tbs']:.2f} TB/s | "
              f"default ({row['default_splits']} splits) {med['mxfp4/0']:7.1f} us {row['mxfp4_default_tbs']:.2f} TB/s | "
              f"best {best_nf} {med[best_nf]:7.1f} us {row['nf4_tbs']:.2f} TB/s | "
              f"mxfp4/nf4 time {med[best_mx] / med[best_nf]:.2f}", flush=True)
    return rows


def bench_block(model, iters, warmup):
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config(model)
    rows = []
    blocks = {}
    for quant in ("nf4", "mxfp4", "int8"):
        blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
        init_random_block_(blk, cfg, 0)
        blocks[quant] = blk.eval().optimize_for_inference(quant=quant)
        fp = blocks[quant]._fast
        print(f"block {model} {quant}: tuned splits qkv={fp.wqkv_t.splits} o={fp.wo_t.splits} "
              f"gate_up={fp.wgateup_t.splits} down={fp.wdown_t.splits}", flush=True)
    for B in BATCHES:
        runs = {}
        for quant, blk in blocks.items():
            ks, vs = blk.kv_cache_shape(B, 64)
            k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
            v = torch.zeros_like(k)
            h = torch.randn(B, 1, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5
            ctx = DecodeContext(torch.device("cuda"))
            ctx.set_position(8)
            with torch.no_grad():
                graph = GraphedCallable(lambda blk=blk, h=h, k=k, v=v, ctx=ctx: blk(h, kv_cache=(k, v), ctx=ctx), [])
            runs[f"{quant}/eager"] = lambda blk=blk, h=h, k=k, v=v: blk(h, kv_cache=(k, v), prefix_length=8)
            runs[f"{quant}/graph"] = graph.replay
        times = {k: [] for k in runs}
        with torch.no_grad():
            for it in range(warmup + iters):
                for k, fn in runs.items():
                    t = _timed(fn)
                    if it >= warmup:
                        times[k].append(t)
        med = {k: _median(v) for k, v in times.items()}
        rows.append(dict(model=model, B=B, us=med))
        print(f"block {model} B={B}  " + "  ".join(f"{k} {v:7.1f} us" for k, v in med.items()), flush=True)
    return rows


def bench_gemm(hip, name, in_dim, out_dim, rows_m, iters, warmup, rotate_mb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(in_dim, out_dim, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    p, s = hip.mxfp4_quantize(w)
    del w
    n = _copies(p.numel() + s.numel(), rotate_mb)
    packed = [(p.clone(), s.clone()) for _ in range(n)]
    n_res = max(2, min(n, -(-(rotate_mb << 20) // (in_dim * out_dim * 2))))
    resident = [hip.mxfp4_dequantize(p, s) for _ in range(n_res)]
    paths = {
        "resident": lambda x, i: torch.matmul(x, resident[i % n_res]),
        "dequant+mm": lambda x, i: torch.matmul(x, hip.mxfp4_dequantize(*packed[i])),
        "fused": lambda x, i: hip.gemm_mxfp4(packed[i][0], packed[i][1], x, None),
    }
    out = []
    for m in rows_m:
        x = torch.randn(m, in_dim, device="cuda", generator=g).to(torch.bfloat16)
        diff = (paths["fused"](x, 0).float() - paths["resident"](x, 0).float()).abs().max().item()
        times = {k: [] for k in paths}
        call = 0  # every call takes the next copy, so no path finds the previous path's weight cached
        for it in range(warmup + iters):
            for k, fn in paths.items():
                call += 1
                t = _timed(lambda: fn(x, call % n))
                if it >= warmup:
                    times[k].append(t)
        med = {k: _median(v) for k, v in times.items()}
        out.append(dict(shape=name, M=m, us=med, max_abs_diff=diff))
        print(f"gemm {name:17s} M={m:5d}  resident {med['resident']:9.1f} us  dequant+mm {med['dequant+mm']:9.1f} us  "
              f"fused {med['fused']:9.1f} us [{2.0 * m * in_dim * out_dim / med['fused'] / 1e6:6.1f} TF/s]  "
              f"fused/dequant+mm {med['fused'] / med['dequant+mm']:5.2f}  maxdiff {diff:.3g}", flush=True)
    return out


def quant_error(seed):
    from petals_amd.ops import mxfp4, nf4

    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(2048, 2048, generator=g) * 0.02).to(torch.bfloat16)
    ref = w.double()
    out = {}
    for name, mod in (("mxfp4", mxfp4), ("nf4", nf4)):
        back = mod.dequantize(*mod.quantize(w)).double()
        out[name] = ((back - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"error: relative RMS of round-tripped N(0, 0.02^2) bf16 weights [2048, 2048]: "
          f"mxfp4 {out['mxfp4']:.4f}  nf4 {out['nf4']:.4f}", flush=True)
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--only", nargs="+", default=["gemv", "block", "gemm", "error"],
                        choices=["gemv", "block", "gemm", "error"])
    parser.add_argument("--iters", type=int, default=30)
    parser.add_argument("--warmup", type=int, default=5)
    parser.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    parser.add_argument("--rows", type=int, nargs="+", default=list(ROWS))
    parser.add_argument("--rotate-mb", type=int, default=768,
                        help="bytes of weight copies each path rotates through (L2 + the 256 MB cache and more)")
    parser.add_argument("--block", metavar="MODEL", default="llama-2-70b")
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args()

    result = {"benchmark": "mxfp4"}
    if "error" in args.only:
        result["error"] = quant_error(args.seed)
    if set(args.only) - {"error"}:
        if not torch.cuda.is_available():
            sys.exit("benchmark_mxfp4 needs a GPU for gemv / block / gemm")
        from petals_amd import ops

        hip = ops._load_hip_ops()
        if hip is None:
            sys.exit(f"HIP extension failed to load: {ops._hip_import_error!r}")
        print(f"device: {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} "
              f"rotate={args.rotate_mb} MB (median of per-call device-event times)", flush=True)
        if "gemv" in args.only:
            result["gemv"] = []
            for name in args.shapes:
                result["gemv"] += bench_gemv(hip, name, *SHAPES[name], args.iters, args.warmup, args.rotate_mb, args.seed)
                torch.cuda.empty_cache()
        if "block" in args.only:
            result["block"] = bench_block(args.block, args.iters, args.warmup)
            torch.cuda.empty_cache()
        if "gemm" in args.only:
            result["gemm"] = []
            for name in args.shapes:
                result["gemm"] += bench_gemm(hip, name, *SHAPES[name], args.rows, args.iters, args.warmup,
                                             args.rotate_mb, args.seed)
                torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
