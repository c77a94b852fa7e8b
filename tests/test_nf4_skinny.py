"""Wide decode (PETALS_AMD_WIDE_DECODE=on): gemm_nf4_skinny, the NF4 skinny-M MFMA
kernel for 9..32 rows (ops/csrc/nf4_skinny.hip), and the Llama block routing.

Reference: float64 x64 @ W64 with W64 = ops/nf4.py::dequantize of the packed
bytes the kernel reads.

  1. one-hot rows, bit for bit: pins the row, column, k and interleave mapping;
  2. random data: |out - ref| <= in * 2^-23 * (|x| @ |W|) on the fp32 epilogues
     (x on the bf16 grid, so the kernel's one x rounding is exact; unrounded
     fp32 x adds 2^-9 * (|x| @ |W|)), + 2^-8 |ref| on residual-bf16, the SwiGLU
     propagation of tests/test_nf4_gemv_wg.py; twice on a NaN workspace of
     64 * 8 * out floats, bit-identical;
  3. host checks; 4. block level against the fp32 CPU block over the
  dequantized weights, forward() patched to raise; 5. mode validation (CPU).
"""

import functools

import pytest
import torch

from petals_amd.ops import nf4

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
EPI_RAW, EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU = -1, 0, 2, 3
SHAPES = [(64, 64), (160, 192), (1024, 2048)]  # one chunk; ragged chunks, out % 128 != 0; several tiles and waves


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


@functools.lru_cache(maxsize=None)
def _weights(in_dim, out_dim):
    g = torch.Generator().manual_seed(in_dim * 7919 + out_dim)
    packed, absmax = nf4.quantize(torch.randn(in_dim, out_dim, generator=g) * 0.05)
    w64 = nf4.dequantize(packed, absmax).double()
    x = torch.randn(32, in_dim, generator=g)
    res = torch.randn(32, out_dim, generator=g).to(torch.bfloat16)
    dev = (packed.cuda(), absmax.cuda(), absmax.t().contiguous().cuda())
    return dev, w64, x, res


def _twice(hip, dev, x, out_dim, epi, splits, residual=None, amt=True):
    """Two calls on a NaN-filled workspace of exactly 64 * 8 * out floats."""
    outs = []
    for _ in range(2):
        ws = torch.full((64 * 8 * out_dim,), float("nan"), device="cuda")
        outs.append(hip.gemm_nf4_skinny(dev[0], dev[1], x, ws, residual, epi, splits, None, dev[2] if amt else None))
        assert not bool(torch.isnan(ws[0])), "the partials must land in the caller's workspace"
    assert torch.equal(outs[0], outs[1])
    return outs[0].cpu()


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("rows", [9, 16, 17, 32])
def test_one_hot_rows_bit_for_bit(hip, rows, in_dim, out_dim, splits):
    dev, w64, _, _ = _weights(in_dim, out_dim)
    # every k-step edge is a candidate (chunks and wave shares are whole steps): first and last k included
    edges = sorted({k for e in range(0, in_dim + 1, 32) for k in (e - 1, e) if 0 <= k < in_dim})
    if len(edges) > rows:
        edges = [edges[i] for i in torch.linspace(0, len(edges) - 1, rows).round().long().tolist()]
    pos = (edges + [k for k in range(in_dim) if k not in edges])[:rows]
    assert len(set(pos)) == rows and 0 in pos and in_dim - 1 in pos
    val = torch.tensor([1.0 if b % 2 == 0 else -2.0 for b in range(rows)])
    x = torch.zeros(rows, in_dim)
    x[torch.arange(rows), pos] = val
    want = (val.double()[:, None] * w64[pos]).float()
    n = hip.gemm_nf4_skinny_splits(in_dim, out_dim, rows, splits)
    assert n * rows <= 512 and (splits == 0 or n <= splits)
    out = _twice(hip, dev, x.cuda(), out_dim, EPI_PLAIN, splits, amt=False)
    assert torch.equal(out, want), (out != want).nonzero()[:4]
    raw = _twice(hip, dev, x.cuda(), out_dim, EPI_RAW, splits)
    assert raw.shape == (n, rows, out_dim)
    assert torch.equal(raw.sum(0), want), (raw.sum(0) != want).nonzero()[:4]


def _silu(t):
    return t / (1.0 + torch.exp(-t))


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("x_on_bf16_grid", [True, False])
@pytest.mark.parametrize("rows,in_dim,out_dim", [(9, 160, 192), (17, 1024, 2048), (32, 1024, 2048)])
def test_random_vs_float64(hip, rows, in_dim, out_dim, x_on_bf16_grid):
    dev, w64, x, res = _weights(in_dim, out_dim)
    x = x[:rows].to(torch.bfloat16).float() if x_on_bf16_grid else x[:rows]
    res = res[:rows]
    ref = x.double() @ w64
    mag = x.double().abs() @ w64.abs()
    bnd = (in_dim * 2.0 ** -23 + (0.0 if x_on_bf16_grid else 2.0 ** -9)) * mag
    half = out_dim // 2
    gt, up, bg, bu = ref[:, :half], ref[:, half:], bnd[:, :half], bnd[:, half:]
    ref_sw, ref_res = _silu(gt) * up, ref + res.double()
    cases = {
        "plain": (EPI_PLAIN, None, ref, bnd),
        "raw": (EPI_RAW, None, ref, bnd),
        "residual": (EPI_RESIDUAL, res.cuda(), ref_res, bnd + 2.0 ** -8 * ref_res.abs()),
        "swiglu": (EPI_SWIGLU, None, ref_sw,
                   1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * ref_sw.abs()),
    }
    worst = {}
    for splits in (0, 3):
        for name, (epi, r, want, bound) in cases.items():
            out = _twice(hip, dev, x.cuda(), out_dim, epi, splits, r, amt=splits == 0).double()
            out = out.sum(0) if epi == EPI_RAW else out
            assert out.shape == want.shape and torch.isfinite(out).all()
            err = (out - want).abs()
            worst[name] = max(worst.get(name, 0.0), (err / bound.clamp_min(1e-300)).max().item())
            assert (err <= bound).all(), f"splits={splits} {name}: err/bound {worst[name]:.3f}"
    print(f"gemm_nf4_skinny {rows}x{in_dim}x{out_dim} grid={x_on_bf16_grid} worst err/bound: "
          + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@requires_gpu
@pytest.mark.gpu
def test_host_checks(hip):
    dev, _, x, _ = _weights(64, 64)
    ws = torch.empty(64 * 8 * 64, device="cuda")
    for bad in (x[:8].cuda(), torch.randn(33, 64, device="cuda"), x[:9].cuda().to(torch.bfloat16)):
        with pytest.raises(RuntimeError):
            hip.gemm_nf4_skinny(dev[0], dev[1], bad, ws, None, EPI_PLAIN, 0)
    with pytest.raises(RuntimeError, match="in % 32"):
        hip.gemm_nf4_skinny(dev[0][:48], dev[1][:48], x[:9, :48].contiguous().cuda(), ws, None, EPI_PLAIN, 0)
    with pytest.raises(RuntimeError, match="9..32 rows"):
        hip.gemm_nf4_skinny_splits(64, 64, 8, 0)


# -------------------------------------------------------------------- block


def _block_pair(preset):
    """NF4 GPU block and an fp32 CPU block holding the weights it dequantizes."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk_cpu = get_model_block(cfg, 0)
    init_random_block_(blk_cpu, cfg, 0)
    blk_cpu = blk_cpu.float().eval()
    blk_gpu = get_model_block(cfg, 0)
    blk_gpu.load_state_dict(blk_cpu.state_dict())
    blk_gpu = blk_gpu.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="nf4")
    fast = blk_gpu._fast
    assert (fast is not None) == (preset == "test-llama-hd128")  # head_dim 16 has no fused path
    if fast is not None:
        deq = lambda w: nf4.dequantize(w.packed.cpu(), w.absmax.cpu()).float().t()  # noqa: E731  [out, in]
        qkv, gu = deq(fast.wqkv_t), deq(fast.wgateup_t)
        qd, kd, inter = fast.qh * fast.hd, fast.kh * fast.hd, gu.shape[0] // 2
        attn, mlp = blk_cpu.self_attn, blk_cpu.mlp
        with torch.no_grad():
            for lin, w in ((attn.q_proj, qkv[:qd]), (attn.k_proj, qkv[qd : qd + kd]), (attn.v_proj, qkv[qd + kd :]),
                           (attn.o_proj, deq(fast.wo_t)), (mlp.gate_proj, gu[:inter]), (mlp.up_proj, gu[inter:]),
                           (mlp.down_proj, deq(fast.wdown_t))):
                lin.weight.copy_(w)
    return cfg, blk_cpu, blk_gpu


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(12, 1), (3, 4)])
@pytest.mark.parametrize("preset", ["test-llama-hd128", "test-llama"])
def test_block_wide_step_matches_cpu(hip, monkeypatch, preset, b, t):
    """Prefill 5, poison the cache past the step, then one step of b * t = 12
    rows through LlamaBlock.forward with the mode(s) on and forward() patched
    to raise; with the mode unset the same step takes forward() as before."""
    cfg, blk_cpu, blk_gpu = _block_pair(preset)
    fast = blk_gpu._fast
    pre, lmax = 5, 32
    x = torch.randn(b, pre + t, cfg.hidden_size, generator=torch.Generator().manual_seed(11 * b + t)) * 0.5
    ks, vs = blk_cpu.kv_cache_shape(b, lmax)
    kc, vc = torch.zeros(ks), torch.zeros(vs)
    kg = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
    vg = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
    monkeypatch.delenv("PETALS_AMD_WIDE_DECODE", raising=False)
    monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "on" if t > 1 else "off")
    xg = x.cuda().bfloat16()
    with torch.inference_mode():
        blk_cpu(x[:, :pre], kv_cache=(kc, vc), prefix_length=0)
        ref = blk_cpu(x[:, pre:], kv_cache=(kc, vc), prefix_length=pre)
        blk_gpu(xg[:, :pre], kv_cache=(kg, vg), prefix_length=0)
        vg[:, :, pre:] = 1.0e4  # the step overwrites its own rows; the rest must never be read
        k0, v0 = kg.clone(), vg.clone()
        if fast is not None:
            entered, real = [], fast.forward
            monkeypatch.setattr(fast, "forward", lambda *a, **kw: entered.append(1) or real(*a, **kw), raising=False)
            blk_gpu(xg[:, pre:], kv_cache=(k0, v0), prefix_length=pre)
            assert entered, "mode unset: a 12-row step takes forward() as before"

            def refuse(*a, **kw):
                raise AssertionError("the wide step took the prefill path")

            monkeypatch.setattr(fast, "forward", refuse, raising=False)
        monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "on")
        out = blk_gpu(xg[:, pre:], kv_cache=(kg, vg), prefix_length=pre).float().cpu()
    assert torch.allclose(out, ref, atol=2e-2, rtol=2e-2), (out - ref).abs().max()
    assert torch.equal(vg[:, :, pre + t :], torch.full_like(vg[:, :, pre + t :], 1.0e4))


def test_mode_switch_and_public_knobs(monkeypatch):
    import inspect

    from petals_amd.cli.run_server import build_parser
    from petals_amd.ops.fused_decode import set_wide_decode_mode, wide_decode_mode
    from petals_amd.server.server import Server

    monkeypatch.delenv("PETALS_AMD_WIDE_DECODE", raising=False)
    assert wide_decode_mode() == "off"
    monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "auto")
    with pytest.raises(ValueError, match="expected one of"):
        wide_decode_mode()
    with pytest.raises(ValueError, match="expected one of"):
        set_wide_decode_mode("auto")
    assert inspect.signature(Server.__init__).parameters["wide_decode"].default == "off"
    with pytest.raises(ValueError, match="expected one of"):
        Server("test-llama", device="cpu", num_blocks=1, wide_decode="auto")
    monkeypatch.setenv("PETALS_AMD_WIDE_DECODE", "off")
    Server("test-llama", device="cpu", num_blocks=1, wide_decode="on")
    assert wide_decode_mode() == "on"
    p = build_parser()
    assert p.parse_args(["test-llama"]).wide_decode == "off"
    assert p.parse_args(["test-llama", "--wide_decode", "on"]).wide_decode == "on"
