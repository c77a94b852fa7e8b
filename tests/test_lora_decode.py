"""Fused LoRA decode (PETALS_AMD_LORA_DECODE=fused): lora_shrink and lora_reduce
(ops/csrc/lora.hip) against float64, and the Llama decode chain that uses them.

Bounds. A chain of m fp32 additions of products is within m * 2^-23 * sum |terms|
of the exact sum; the shrink has m = in, the reduce m = n + S + r_p + 2 (base
splits, t splits, rank rows, the scale and the final add). The epilogue forms
are tests/test_gemv_numerics.py's. Both tests print the measured share of the
bound (recorded in docs/KERNELS.md, "LoRA decode").

The block reference is the CPU fp32 block holding the weights the kernels read
(the bf16 or dequantized NF4 values) and the same adapter.
"""

import functools
import types

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
EPI_RAW, EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU = -1, 0, 2, 3
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# one short chunk, a ragged wave step, several chunks with a ragged tail; the
# last case has chunks of two 512-k steps (in > 32 * 512)
SHRINK = [(i, r, b) for i in (64, 520, 2056) for r in (1, 20, 192) for b in (1, 3, 8)] + [(16904, 20, 3)]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,R,rows", SHRINK)
def test_shrink_against_float64(hip, in_dim, R, rows):
    g = _gen(in_dim + R + rows)
    x = torch.randn(rows, in_dim, generator=g)
    a = (torch.randn(R, in_dim, generator=g) * 0.05).to(torch.bfloat16)
    x[:, -1] = 2.5  # the last input column carries weight
    t1, t2 = (hip.lora_shrink(x.cuda(), a.cuda()) for _ in range(2))
    assert t1.shape[1:] == (rows, R) and 1 <= t1.shape[0] <= 32
    assert torch.equal(t1.view(torch.int32), t2.view(torch.int32))
    ref = x.double() @ a.double().T
    bound = in_dim * EPS * (x.double().abs() @ a.double().abs().T)
    err = (t1.double().sum(0).cpu() - ref).abs()
    print(f"shrink in={in_dim} R={R} rows={rows} S={t1.shape[0]}: share of bound {(err / bound).max():.4f}")
    assert (err <= bound).all(), (err / bound).max()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("splits", [1, 5, 16, 37])
@pytest.mark.parametrize("epilogue", [EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU])
def test_reduce_zero_b_is_base_reduce(hip, epilogue, splits, rows):
    in_dim, out = 16 * 16 * 37, 384 if epilogue == EPI_SWIGLU else 192  # every split count divides in / 16
    g = _gen(splits)
    w = (torch.randn(in_dim, out, generator=g) * 0.05).to(torch.bfloat16).cuda()
    x = torch.randn(rows, in_dim, generator=g).cuda()
    res = torch.randn(rows, out, generator=g).to(torch.bfloat16).cuda() if epilogue == EPI_RESIDUAL else None
    ws = torch.empty(0, device="cuda")
    want = hip.gemv_bf16(w, x, ws, res, epilogue, splits)
    parts = hip.gemv_bf16(w, x, ws, None, EPI_RAW, splits)
    assert parts.shape[0] == splits
    t_part = torch.randn(3, rows, 4, generator=g).cuda()
    bt = torch.zeros(4 * out, dtype=torch.bfloat16, device="cuda")
    got = hip.lora_reduce(parts, t_part, bt, [0, out, 0, 4, 0], [2.0], res, None, epilogue)
    assert got.dtype == want.dtype and torch.equal(got, want)


# name -> (epilogue, member widths, ranks (None = absent), scales)
REDUCE = {
    "qkv": (EPI_PLAIN, (128, 64, 64), (4, None, 16), (2.0, 1.0, 0.5)),
    "gateup": (EPI_SWIGLU, (96, 96), (8, 3), (2.0, -0.75)),
    "single": (EPI_RESIDUAL, (192,), (64,), (1.5,)),
}


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n", [1, 16, 37])
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("case", list(REDUCE))
def test_reduce_against_float64(hip, case, rows, n):
    epilogue, widths, ranks, scales = REDUCE[case]
    out, S, R = sum(widths), 3, sum(r or 0 for r in ranks)
    g = _gen(n + rows)
    parts = torch.randn(n, rows, out, generator=g)
    t_part = torch.randn(S, rows, R, generator=g)
    res = torch.randn(rows, out, generator=g).to(torch.bfloat16)
    ref = parts.double().sum(0)
    mag = parts.double().abs().sum(0)
    terms = torch.full((out,), float(n + S + 2), dtype=torch.float64)
    segments, seg_scales, bts, c0, t_off, bt_off = [], [], [], 0, 0, 0
    for width, rank, scale in zip(widths, ranks, scales):
        if rank is not None:
            b_t = (torch.randn(rank, width, generator=g) * 0.05).to(torch.bfloat16)
            t = t_part[:, :, t_off : t_off + rank].double()
            ref[:, c0 : c0 + width] += scale * (t.sum(0) @ b_t.double())
            mag[:, c0 : c0 + width] += abs(scale) * (t.abs().sum(0) @ b_t.double().abs())
            terms[c0 : c0 + width] += rank
            segments += [c0, c0 + width, t_off, rank, bt_off]
            seg_scales.append(scale)
            bts.append(b_t.reshape(-1))
            t_off, bt_off = t_off + rank, bt_off + rank * width
        c0 += width
    bnd = terms * EPS * mag
    if epilogue == EPI_RESIDUAL:
        ref = ref + res.double()
        bnd = bnd + 2.0 ** -8 * ref.abs()
    elif epilogue == EPI_SWIGLU:
        half = out // 2
        (gt, up), (bg, bu) = ref.split(half, 1), bnd.split(half, 1)
        silu = gt / (1.0 + torch.exp(-gt))
        ref = silu * up
        bnd = 1.1 * bg * up.abs() + silu.abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * ref.abs()
    bt = torch.cat(bts).cuda()
    args = (parts.cuda(), t_part.cuda())
    tail = (res.cuda() if epilogue == EPI_RESIDUAL else None, None, epilogue)
    got = hip.lora_reduce(*args, bt, segments, seg_scales, *tail)
    err = (got.double().cpu() - ref).abs()
    print(f"reduce {case} rows={rows} n={n}: share of bound {(err / bnd).max():.4f}")
    assert (err <= bnd).all(), (err / bnd).max()
    if None in ranks:  # the absent member's columns: the base reduce's bits (zero B, test above)
        base = hip.lora_reduce(*args, torch.zeros_like(bt), segments, seg_scales, *tail)
        lo = sum(widths[: ranks.index(None)])
        hi = lo + widths[ranks.index(None)]
        assert torch.equal(got[:, lo:hi], base[:, lo:hi])
        assert not torch.equal(got[:, :lo], base[:, :lo])


@functools.lru_cache(maxsize=None)
def _blocks(quant):
    """(cpu fp32 block, fused gpu block), both carrying adapter `t` on all seven
    projections (ranks 4 and 8, values ~0.03, scale 2); the gpu block also
    carries `zero`, the same adapter with every B = 0."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_
    from petals_amd.utils.peft import BlockAdapter, add_adapter_to_block

    cfg = load_model_config("test-llama-hd128")
    cpu = get_model_block(cfg, 0)
    init_random_block_(cpu, cfg, 0)
    cpu = cpu.float().eval()
    gpu = get_model_block(cfg, 0)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant=quant)
    fast = gpu._fast
    lins = dict(q=cpu.self_attn.q_proj, k=cpu.self_attn.k_proj, v=cpu.self_attn.v_proj, o=cpu.self_attn.o_proj,
                gate=cpu.mlp.gate_proj, up=cpu.mlp.up_proj, down=cpu.mlp.down_proj)
    for w, keys in ((fast.wqkv_t, "qkv"), (fast.wo_t, "o"), (fast.wgateup_t, ("gate", "up")), (fast.wdown_t, ("down",))):
        wt, c0 = w.dense().float().cpu().t(), 0  # [out, in], the values the kernels read
        for key in keys:
            n_out = lins[key].out_features
            lins[key].weight.data = wt[c0 : c0 + n_out].contiguous()
            c0 += n_out
    g = _gen(17)
    proj = {}
    for i, (key, lin) in enumerate(lins.items()):
        r = (4, 8)[i % 2]
        proj[key] = ((torch.randn(r, lin.in_features, generator=g) * 0.03).to(torch.bfloat16).float(),
                     (torch.randn(lin.out_features, r, generator=g) * 0.03).to(torch.bfloat16).float(), 2.0)
    for blk in (cpu, gpu):
        add_adapter_to_block(blk, BlockAdapter("t", {k: (a.clone(), b.clone(), s) for k, (a, b, s) in proj.items()}))
    add_adapter_to_block(gpu, BlockAdapter("zero", {k: (a.clone(), torch.zeros_like(b), s) for k, (a, b, s) in proj.items()}))
    return cpu, gpu


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("quant", ["none", "nf4"])
def test_block_fused_decode(hip, monkeypatch, quant, B):
    """Prefill 5 under the adapter (torch deltas), then decode steps in `fused`
    mode: against the CPU block, zero-B against no adapter, graph replay."""
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.utils.peft import using_adapter

    cpu, gpu = _blocks(quant)
    entered = []
    real = gpu._fast._lora_group
    monkeypatch.setattr(gpu._fast, "_lora_group", lambda *a: entered.append(a[0]) or real(*a), raising=False)
    pre, steps, lmax = 5, 3, 16
    x = torch.randn(B, pre + steps, 512, generator=_gen(B)) * 0.5
    xg = x.cuda().bfloat16()
    ks, vs = cpu.kv_cache_shape(B, lmax)
    kc, vc = torch.zeros(ks), torch.zeros(vs)
    kg, vg = (torch.zeros(ks, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    with torch.inference_mode(), using_adapter("t"):
        monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "torch")
        cpu(x[:, :pre], kv_cache=(kc, vc), prefix_length=0)
        gpu(xg[:, :pre], kv_cache=(kg, vg), prefix_length=0)
        assert not entered
        monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "fused")
        kz, vz, kn, vn, kr, vr = (t.clone() for t in (kg, vg, kg, vg, kg, vg))
        ref = torch.cat([cpu(x[:, t : t + 1], kv_cache=(kc, vc), prefix_length=t) for t in range(pre, pre + steps)], 1)
        out = torch.cat([gpu(xg[:, t : t + 1], kv_cache=(kg, vg), prefix_length=t) for t in range(pre, pre + steps)], 1)
        assert entered == ["qkv", "o", "gateup", "down"] * steps
        assert torch.allclose(out.float().cpu(), ref, atol=0.05, rtol=0.05), (out.float().cpu() - ref).abs().max()

        # one capture, replayed over the same steps on a copy of the prefix cache
        ctx, h_in = DecodeContext(torch.device("cuda:0")), torch.empty_like(xg[:, :1])
        ctx.set_position(pre)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = gpu(h_in, kv_cache=(kr, vr), ctx=ctx)
        for i, t in enumerate(range(pre, pre + steps)):
            ctx.set_position(t)
            h_in.copy_(xg[:, t : t + 1])
            graph.replay()
            assert torch.equal(y, out[:, i : i + 1])
        assert torch.equal(kr, kg) and torch.equal(vr, vg)

    with torch.inference_mode():
        with using_adapter("zero"):
            y_zero = gpu(xg[:, pre : pre + 1], kv_cache=(kz, vz), prefix_length=pre)
        y_none = gpu(xg[:, pre : pre + 1], kv_cache=(kn, vn), prefix_length=pre)
    assert torch.equal(y_zero, y_none) and torch.equal(kz, kn) and torch.equal(vz, vn)
    assert kz[:, :, pre].abs().sum() > 0


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("B,T", [(1, 4), (2, 3)])
@pytest.mark.parametrize("quant", ["none", "nf4"])
def test_block_multi_step_with_adapter(hip, monkeypatch, quant, B, T):
    """forward(S=T) under the adapter with both modes on takes decode_multi and
    agrees with T fused decode_steps (tests/test_multi_decode.py's tolerance)."""
    from petals_amd.utils.peft import using_adapter

    _, gpu = _blocks(quant)
    entered = []
    real = gpu._fast.decode_multi
    monkeypatch.setattr(gpu._fast, "decode_multi", lambda *a, **kw: entered.append(kw.get("adapter")) or real(*a, **kw),
                        raising=False)
    pre, lmax = 5, 16
    x = (torch.randn(B, pre + T, 512, generator=_gen(B + T)) * 0.5).to(torch.bfloat16).cuda()
    ks, vs = gpu.kv_cache_shape(B, lmax)
    k1, v1 = (torch.zeros(ks, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "fused")
    monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "off")
    with torch.inference_mode(), using_adapter("t"):
        gpu(x[:, :pre], kv_cache=(k1, v1), prefix_length=0)
        k2, v2 = k1.clone(), v1.clone()
        y_steps = torch.cat([gpu(x[:, t : t + 1], kv_cache=(k1, v1), prefix_length=t) for t in range(pre, pre + T)], 1)
        monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "on")
        y_multi = gpu(x[:, pre:], kv_cache=(k2, v2), prefix_length=pre)
    assert len(entered) == 1 and entered[0] is not None
    assert torch.allclose(y_multi.float(), y_steps.float(), atol=2e-2, rtol=2e-2), (y_multi.float() - y_steps.float()).abs().max()
    assert torch.allclose(k2.float(), k1.float(), atol=2e-2, rtol=2e-2) and torch.allclose(v2.float(), v1.float(), atol=2e-2, rtol=2e-2)


def test_mode_switch_and_public_knobs(monkeypatch):
    import inspect

    from petals_amd.cli.run_server import build_parser
    from petals_amd.ops.fused_decode import lora_decode_mode, set_lora_decode_mode
    from petals_amd.server.server import Server

    monkeypatch.delenv("PETALS_AMD_LORA_DECODE", raising=False)
    assert lora_decode_mode() == "torch"
    monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "auto")
    with pytest.raises(ValueError, match="expected one of"):
        lora_decode_mode()
    with pytest.raises(ValueError, match="expected one of"):
        set_lora_decode_mode("auto")
    assert inspect.signature(Server.__init__).parameters["lora_decode"].default == "torch"
    with pytest.raises(ValueError, match="expected one of"):
        Server("test-llama", device="cpu", num_blocks=1, lora_decode="auto")
    monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "torch")
    Server("test-llama", device="cpu", num_blocks=1, lora_decode="fused")
    assert lora_decode_mode() == "fused"
    p = build_parser()
    assert p.parse_args(["test-llama"]).lora_decode == "torch"
    assert p.parse_args(["test-llama", "--lora_decode", "fused"]).lora_decode == "fused"


@pytest.mark.parametrize("ranks,rows,tp,want", [
    ({"q": 64, "k": 64, "v": 64, "down": 1}, 8, 1, True),
    ({"q": 65}, 1, 1, False),
    ({"gate": 257}, 1, 1, False),
    ({"q": 8}, 9, 1, False),
    ({"q": 8}, 1, 2, False),
])
def test_lora_fused_eligible(monkeypatch, ranks, rows, tp, want):
    from petals_amd.ops.lora import lora_fused_eligible
    from petals_amd.utils.peft import BlockAdapter

    fast = types.SimpleNamespace(tp_world=tp, device=torch.device("cpu"))
    ad = BlockAdapter("t", {k: (torch.zeros(r, 64, dtype=torch.bfloat16), torch.zeros(32, r, dtype=torch.bfloat16), 1.0)
                            for k, r in ranks.items()})
    monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "fused")
    assert lora_fused_eligible(fast, ad, rows) is want
    monkeypatch.setenv("PETALS_AMD_LORA_DECODE", "torch")
    assert lora_fused_eligible(fast, ad, rows) is False
