"""Mixtral wide decode: gemm_nf4_moe_skinny, the expert-grouped NF4 skinny-M MFMA
kernel (ops/csrc/moe_skinny.hip), and the Mixtral block routing built on it.

Reference: float64 x64 @ W64[e] with W64[e] = ops/nf4.py::dequantize of the packed
bytes the kernel reads. Every op runs twice on a NaN workspace of exactly
64 * 8 * out floats: bit-identical, partials in the workspace.

  1. one-hot rows, bit for bit: pins row -> expert, row -> token (r / k_per_tok),
     column, k and the pass / slot mapping (an odd R has no k_per_tok = 2 form);
  2. random data: |out - ref| <= (in * 2^-23 + [x off the bf16 grid] * 2^-9) * (|x| @ |W|),
     the SwiGLU propagation of tests/test_nf4_skinny.py;
  3. host checks; 4. block level against the fp32 CPU block over the dequantized
  weights, forward() patched to raise; 5. the eligibility truth table (CPU).
"""

import functools
from types import SimpleNamespace

import pytest
import torch

from petals_amd.ops import nf4

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
EPI_RAW, EPI_PLAIN, EPI_SWIGLU = -1, 0, 3
E = 4
SHAPES = [(64, 64), (160, 192), (1024, 2048)]  # one chunk; ragged chunks, out % 128 != 0; several tiles and waves
SEL = {  # name -> (k_per_tok, expert of every virtual row)
    "router18": (1, [(r * 3 + r // 4) % E for r in range(18)]),
    "router18k2": (2, [e for t in range(9) for e in (t % E, (t + 1 + t // E) % E)]),  # distinct experts per token
    "one64": (1, [2] * 64),  # four passes, three idle experts
    "one64k2": (2, [2] * 64),
    "edge33": (1, [1] * 16 + [3] * 17),  # exactly one full pass; one row into the second
    "single": (1, [3]),
    "r17": (1, [0] * 17),
}


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


@functools.lru_cache(maxsize=None)
def _weights(in_dim, out_dim):
    g = torch.Generator().manual_seed(in_dim * 7919 + out_dim)
    pa = [nf4.quantize(torch.randn(in_dim, out_dim, generator=g) * 0.05) for _ in range(E)]
    packed, absmax = torch.stack([p for p, _ in pa]), torch.stack([a for _, a in pa])
    w64 = torch.stack([nf4.dequantize(p, a).double() for p, a in pa])
    x = torch.randn(64, in_dim, generator=g)
    return (packed.cuda(), absmax.cuda(), absmax.transpose(1, 2).contiguous().cuda()), w64, x


def _twice(hip, dev, x, sel, k, out_dim, epi, splits, amt=True):
    """Two calls on a NaN-filled workspace of exactly 64 * 8 * out floats."""
    outs = []
    for _ in range(2):
        ws = torch.full((64 * 8 * out_dim,), float("nan"), device="cuda")
        outs.append(hip.gemm_nf4_moe_skinny(dev[0], dev[1], x, sel, k, ws, epi, splits, dev[2] if amt else None))
        assert not bool(torch.isnan(ws[0])), "the partials must land in the caller's workspace"
    assert torch.equal(outs[0], outs[1])
    return outs[0].cpu()


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("pattern", list(SEL))
def test_one_hot_rows_bit_for_bit(hip, pattern, in_dim, out_dim, splits):
    dev, w64, _ = _weights(in_dim, out_dim)
    k, sel = SEL[pattern]
    sel = torch.tensor(sel, dtype=torch.int32)
    rows, tokens = len(sel), len(sel) // k
    # every k-step edge is a candidate (chunks and wave shares are whole steps): k = 0 first, in - 1 last
    edges = sorted({c for e in range(0, in_dim + 1, 32) for c in (e - 1, e) if 0 <= c < in_dim})
    pick = torch.linspace(0, len(edges) - 1, tokens).round().long().tolist() if tokens <= len(edges) else range(tokens)
    pos = torch.tensor([edges[i % len(edges)] for i in pick])
    assert pos[0] == 0 and (tokens == 1 or in_dim - 1 in pos)
    val = torch.tensor([1.0 if t % 2 == 0 else -2.0 for t in range(tokens)])
    x = torch.zeros(tokens, in_dim)
    x[torch.arange(tokens), pos] = val
    tok = torch.arange(rows) // k  # the pairs of a token share x and differ in expert alone
    want = (val.double()[tok, None] * w64[sel.long(), pos[tok]]).float()
    assert hip.gemm_nf4_moe_skinny_splits(in_dim, out_dim, rows, E, splits) * rows <= 512
    out = _twice(hip, dev, x.cuda(), sel.cuda(), k, out_dim, EPI_PLAIN, splits, amt=splits % 2 == 0)
    assert torch.equal(out, want), (out != want).nonzero()[:4]


def _silu(t):
    return t / (1.0 + torch.exp(-t))


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("x_on_bf16_grid", [True, False])
@pytest.mark.parametrize("rows,in_dim,out_dim", [(18, 160, 192), (33, 1024, 2048), (64, 1024, 2048)])
def test_random_vs_float64(hip, rows, in_dim, out_dim, x_on_bf16_grid):
    dev, w64, x = _weights(in_dim, out_dim)
    k = 2 if rows % 2 == 0 else 1
    g = torch.Generator().manual_seed(rows)
    sel = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(rows // k)]).reshape(-1).to(torch.int32)
    x = x[: rows // k].to(torch.bfloat16).float() if x_on_bf16_grid else x[: rows // k]
    xr = x.double()[torch.arange(rows) // k]  # [R, in]
    ref, mag = torch.zeros(rows, out_dim, dtype=torch.float64), torch.zeros(rows, out_dim, dtype=torch.float64)
    for e in range(E):
        ref[sel == e], mag[sel == e] = xr[sel == e] @ w64[e], xr[sel == e].abs() @ w64[e].abs()
    bnd = (in_dim * 2.0 ** -23 + (0.0 if x_on_bf16_grid else 2.0 ** -9)) * mag
    half = out_dim // 2
    gt, up, bg, bu = ref[:, :half], ref[:, half:], bnd[:, :half], bnd[:, half:]
    ref_sw = _silu(gt) * up
    cases = {
        "plain": (EPI_PLAIN, ref, bnd),
        "swiglu": (EPI_SWIGLU, ref_sw,
                   1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * ref_sw.abs()),
    }
    worst = {}
    for splits in (0, 3):
        for amt in (True, False):
            for name, (epi, want, bound) in cases.items():
                out = _twice(hip, dev, x.cuda(), sel.cuda(), k, out_dim, epi, splits, amt=amt).double()
                assert out.shape == want.shape and torch.isfinite(out).all()
                err = (out - want).abs()
                worst[name] = max(worst.get(name, 0.0), (err / bound.clamp_min(1e-300)).max().item())
                assert (err <= bound).all(), f"splits={splits} amt={amt} {name}: err/bound {worst[name]:.3f}"
    print(f"gemm_nf4_moe_skinny {rows}x{in_dim}x{out_dim} grid={x_on_bf16_grid} worst err/bound: "
          + "  ".join(f"{n} {v:.4f}" for n, v in worst.items()))


@requires_gpu
@pytest.mark.gpu
def test_host_checks(hip):
    (packed, absmax, _), _, x = _weights(64, 64)
    ws = torch.empty(64 * 8 * 64, device="cuda")
    sel = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    xg = x.cuda()
    bad = [
        (packed, absmax, xg[:0], sel(0), 1, EPI_PLAIN),   # R = 0
        (packed, absmax, xg[:64], sel(65), 1, EPI_PLAIN),  # R = 65 (also tokens * k != R)
        (packed, absmax, xg[:9].to(torch.bfloat16), sel(9), 1, EPI_PLAIN),
        (packed[:, :48].contiguous(), absmax[:, :48].contiguous(), xg[:9, :48].contiguous(), sel(9), 1, EPI_PLAIN),
        (packed[:, :, :16].contiguous(), absmax, xg[:9], sel(9), 1, EPI_PLAIN),  # out = 32
        (packed, absmax, xg[:9], sel(17), 2, EPI_PLAIN),  # 9 tokens * 2 != 17
        (packed, absmax, xg[:9], sel(9), 1, EPI_RAW),
    ]
    for p, a, xx, s, k, epi in bad:
        with pytest.raises(RuntimeError, match="gemm_nf4_moe_skinny"):
            hip.gemm_nf4_moe_skinny(p, a, xx, s, k, ws, epi, 0)
    with pytest.raises(RuntimeError, match="1..64 virtual rows"):
        hip.gemm_nf4_moe_skinny_splits(64, 64, 65, E, 0)


# -------------------------------------------------------------------- block

# x seeds per (B, T): on the CPU reference every token of the step keeps its 2nd
# and 3rd router logit at least ROUTER_MARGIN * max |logit| apart, so bf16 inputs
# (about 2^-8 of a logit) cannot flip the top-k choice
BLOCK_SEEDS = {(12, 1): 180, (32, 1): 96, (4, 4): 194, (2, 3): 245}
ROUTER_MARGIN = 0.05


@functools.lru_cache(maxsize=None)
def _block_pair():
    """NF4 GPU block and an fp32 CPU block holding the weights it dequantizes, expert stacks included."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config("test-mixtral-hd64")
    blk_cpu = get_model_block(cfg, 0)
    init_random_block_(blk_cpu, cfg, 0)
    blk_cpu = blk_cpu.float().eval()
    blk_gpu = get_model_block(cfg, 0)
    blk_gpu.load_state_dict(blk_cpu.state_dict())
    blk_gpu = blk_gpu.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="nf4")
    fast = blk_gpu._fast
    deq = lambda p, a: nf4.dequantize(p.cpu(), a.cpu()).float().t()  # noqa: E731  [out, in]
    qkv = deq(fast.wqkv_t.packed, fast.wqkv_t.absmax)
    qd, kd = fast.qh * fast.hd, fast.kh * fast.hd
    attn, moe = blk_cpu.self_attn, blk_cpu.block_sparse_moe
    pairs = [(attn.q_proj, qkv[:qd]), (attn.k_proj, qkv[qd : qd + kd]), (attn.v_proj, qkv[qd + kd :]),
             (attn.o_proj, deq(fast.wo_t.packed, fast.wo_t.absmax)), (moe.gate, fast.w_router_t.t().float().cpu())]
    for e, expert in enumerate(moe.experts):
        gu = deq(fast.stacked_gu.packed_all[e], fast.stacked_gu.absmax_all[e])
        down = deq(fast.stacked_down.packed_all[e], fast.stacked_down.absmax_all[e])
        pairs += [(expert.w1, gu[: gu.shape[0] // 2]), (expert.w3, gu[gu.shape[0] // 2 :]), (expert.w2, down)]
    with torch.no_grad():
        for lin, w in pairs:
            lin.weight.copy_(w)
    return cfg, blk_cpu, blk_gpu


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("b,t", list(BLOCK_SEEDS))
def test_block_wide_step_matches_cpu(hip, monkeypatch, b, t):
    """Prefill 5, poison the cache past the step, then one step of b * t rows
    through MixtralBlock.forward with the mode(s) on and forward() patched to
    raise; with the modes unset the same step takes forward() as before.
    (2, 3) keeps wide mode off: 6 rows, 12 pairs, the gemv_nf4_moe route."""
    cfg, blk_cpu, blk_gpu = _block_pair()
    fast = blk_gpu._fast
    pre, lmax = 5, 32
    x = torch.randn(b, pre + t, cfg.hidden_size, generator=torch.Generator().manual_seed(BLOCK_SEEDS[b, t])) * 0.5
    ks, vs = blk_cpu.kv_cache_shape(b, lmax)
    kc, vc = torch.zeros(ks), torch.zeros(vs)
    kg = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
    vg = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
    monkeypatch.delenv("PETALS_AMD_WIDE_DECODE", raising=False)
    monkeypatch.delenv("PETALS_AMD_MULTI_DECODE", raising=False)
    xg = x.cuda().bfloat16()
    logits = []
    with torch.inference_mode():
        blk_cpu(x[:, :pre], kv_cache=(kc, vc), prefix_length=0)
        hook = blk_cpu.block_sparse_moe.gate.register_forward_hook(lambda m, i, o: logits.append(o))
        ref = blk_cpu(x[:, pre:], kv_cache=(kc, vc), prefix_length=pre)
        hook.remove()
        top = logits[0].sort(dim=-1, descending=True).values
        assert ((top[:, 1] - top[:, 2]) >= ROUTER_MARGIN * logits[0].abs().amax(dim=-1)).all(), "pick another seed"
        blk_gpu(xg[:, :pre], kv_cache=(kg, vg), prefix_length=0)
        vg[:, :, pre:] = 1.0e4  # the step overwrites its own rows; the rest must never be read
        k0, v0 = kg.clone(), vg.clone()
        entered, real = [], fast.forward
        monkeypatch.setattr(fast, "forward", lambda *a, **kw: entered.append(1) or real(*a, **kw), raising=False)
        blk_gpu(xg[:, pre:], kv_cache=(k0, v0), prefix_length=pre)
        assert entered, "modes unset: the step takes forward() as before"

        def refuse(*a, **kw):
            raise AssertionError("the step took the prefill path")

        monkeypatch.setattr(fast, "forward", refuse, raising=False)
        if b * t > 8:
            monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "on")
        if t > 1:
            monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "on")
        out = blk_gpu(xg[:, pre:], kv_cache=(kg, vg), prefix_length=pre).float().cpu()
    assert torch.allclose(out, ref, atol=2e-2, rtol=2e-2), (out - ref).abs().max()
    assert torch.equal(vg[:, :, pre + t :], torch.full_like(vg[:, :, pre + t :], 1.0e4))


def test_eligibility_truth_table(monkeypatch):
    from petals_amd.ops.fused_moe import MixtralFastPath

    def stub(quant="nf4", top_k=2, in_dim=256, out_dim=1024):
        fast = MixtralFastPath.__new__(MixtralFastPath)
        st = SimpleNamespace(skinny_ok=quant == "nf4" and in_dim % 32 == 0 and out_dim % 64 == 0)
        fast.__dict__.update(quant=quant, top_k=top_k, tp_world=1, gq=2, stacked_gu=st, stacked_down=st)
        return fast

    monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "off")
    assert not stub().wide_decode_eligible(12)
    assert stub().multi_decode_eligible(2, 3) and stub("int8").multi_decode_eligible(2, 4)  # <= 16 pairs: any format
    assert not stub().multi_decode_eligible(4, 4) and not stub(top_k=4).multi_decode_eligible(2, 3)
    monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "on")
    assert stub().wide_decode_eligible(9) and stub().wide_decode_eligible(32) and stub().multi_decode_eligible(4, 4)
    assert not stub().wide_decode_eligible(8) and not stub().wide_decode_eligible(33)
    assert not stub("int8").wide_decode_eligible(12) and not stub("int8").multi_decode_eligible(4, 4)
    assert not stub(top_k=4).wide_decode_eligible(17) and stub(top_k=4).wide_decode_eligible(16)  # rows * top_k <= 64
    assert not stub(out_dim=96).wide_decode_eligible(12) and not stub(in_dim=48).wide_decode_eligible(12)
    assert not stub().wide_decode_eligible(12, adapter=object())
