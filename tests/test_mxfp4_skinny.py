"""Wide decode for MXFP4 weights: gemm_mxfp4_skinny, the skinny-M MFMA kernel
for 9..32 rows (ops/csrc/mxfp4_skinny.hip), and the Llama block routing.

Reference: float64 x64 @ W64, W64 = ops/mxfp4.py::dequantize of the bytes the
kernel reads. One-hot rows are exact; random data stays within
in * 2^-23 * (|x| @ |W|) on the fp32 epilogues (W and the products are exact, x
on the bf16 grid; unrounded fp32 x adds 2^-9 * (|x| @ |W|)), + 2^-8 |ref| on
residual-bf16, the SwiGLU propagation of tests/test_nf4_skinny.py. Every call
runs twice on a NaN workspace of 64 * 8 * out floats, bit-identical.
"""

import functools

import pytest
import torch

from petals_amd.ops import mxfp4

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
EPI_RAW, EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU = -1, 0, 2, 3
SHAPES = [(64, 64), (160, 192), (1024, 2048)]  # one chunk; ragged chunks, out % 256 != 0; several tiles and waves


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


@functools.lru_cache(maxsize=None)
def _weights(in_dim, out_dim):
    g = torch.Generator().manual_seed(in_dim * 7919 + out_dim)
    packed, scales = mxfp4.quantize(torch.randn(in_dim, out_dim, generator=g) * 0.05)
    w64 = mxfp4.dequantize(packed, scales, torch.float64)
    x = torch.randn(32, in_dim, generator=g)
    res = torch.randn(32, out_dim, generator=g).to(torch.bfloat16)
    return (packed.cuda(), scales.cuda()), w64, x, res


def _twice(hip, dev, x, out_dim, epi, splits, residual=None):
    """Two calls on a NaN-filled workspace of exactly 64 * 8 * out floats."""
    outs = []
    for _ in range(2):
        ws = torch.full((64 * 8 * out_dim,), float("nan"), device="cuda")
        outs.append(hip.gemm_mxfp4_skinny(dev[0], dev[1], x, ws, residual, epi, splits, None))
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
    n = hip.gemm_mxfp4_skinny_splits(in_dim, out_dim, rows, splits)
    assert n * rows <= 512 and (splits == 0 or n <= splits)
    # both sides of every 32-step edge (chunks and wave shares are whole steps), first and last k
    # included, `rows` of them per call: neighbours are an odd and an even k, which pins the nibble order
    edges = sorted({k for e in range(0, in_dim + 1, 32) for k in (e - 1, e) if 0 <= k < in_dim})
    assert edges[0] == 0 and edges[-1] == in_dim - 1
    val = torch.tensor([1.0 if b % 2 == 0 else -2.0 for b in range(rows)])
    for first in range(0, len(edges), rows):
        pos = edges[first : first + rows]
        pos = (pos + [k for k in range(in_dim) if k not in pos])[:rows]
        x = torch.zeros(rows, in_dim)
        x[torch.arange(rows), pos] = val
        want = (val.double()[:, None] * w64[pos]).float()
        out = _twice(hip, dev, x.cuda(), out_dim, EPI_PLAIN, splits)
        assert torch.equal(out, want), (first, (out != want).nonzero()[:4])
        raw = _twice(hip, dev, x.cuda(), out_dim, EPI_RAW, splits)
        assert raw.shape == (n, rows, out_dim)
        assert torch.equal(raw.sum(0), want), (first, (raw.sum(0) != want).nonzero()[:4])


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
            out = _twice(hip, dev, x.cuda(), out_dim, epi, splits, r).double()
            out = out.sum(0) if epi == EPI_RAW else out
            assert out.shape == want.shape and torch.isfinite(out).all()
            err = (out - want).abs()
            worst[name] = max(worst.get(name, 0.0), (err / bound.clamp_min(1e-300)).max().item())
            assert (err <= bound).all(), f"splits={splits} {name}: err/bound {worst[name]:.3f}"
    print(f"gemm_mxfp4_skinny {rows}x{in_dim}x{out_dim} grid={x_on_bf16_grid} worst err/bound: "
          + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@requires_gpu
@pytest.mark.gpu
def test_host_checks(hip):
    (packed, scales), _, x, _ = _weights(64, 64)
    ws = torch.empty(64 * 8 * 64, device="cuda")
    for bad in (x[:8].cuda(), torch.randn(33, 64, device="cuda"), x[:9].cuda().to(torch.bfloat16)):
        with pytest.raises(RuntimeError):
            hip.gemm_mxfp4_skinny(packed, scales, bad, ws, None, EPI_PLAIN, 0)
    with pytest.raises(RuntimeError, match="in % 32"):
        hip.gemm_mxfp4_skinny(packed[:24], scales[:1], x[:9, :48].contiguous().cuda(), ws, None, EPI_PLAIN, 0)
    p72, s72 = (t.cuda() for t in mxfp4.quantize(torch.randn(64, 72) * 0.05))
    with pytest.raises(RuntimeError, match="out % 16"):
        hip.gemm_mxfp4_skinny(p72, s72, x[:9].cuda(), ws, None, EPI_PLAIN, 0)
    with pytest.raises(RuntimeError, match="scales"):
        hip.gemm_mxfp4_skinny(packed, scales[:1], x[:9].cuda(), ws, None, EPI_PLAIN, 0)
    with pytest.raises(RuntimeError, match="9..32 rows"):
        hip.gemm_mxfp4_skinny_splits(64, 64, 8, 0)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(12, 1), (3, 4)])
def test_block_wide_step_matches_cpu(hip, monkeypatch, b, t):
    """Prefill 5, poison V past the step, then one step of b * t = 12 rows through
    LlamaBlock.forward: with the mode unset it takes forward() as before; with
    the mode(s) on and forward() patched to raise it runs the decode chain."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config("test-llama-hd128")
    blk_cpu = get_model_block(cfg, 0)
    init_random_block_(blk_cpu, cfg, 0)
    blk_cpu = blk_cpu.float().eval()
    blk_gpu = get_model_block(cfg, 0)
    blk_gpu.load_state_dict(blk_cpu.state_dict())
    blk_gpu = blk_gpu.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="mxfp4")
    fast = blk_gpu._fast
    assert fast is not None and fast.quant == "mxfp4"
    deq = lambda w: mxfp4.dequantize(w.mx_packed.cpu(), w.mx_scales.cpu()).float().t()  # noqa: E731  [out, in]
    qkv, gu = deq(fast.wqkv_t), deq(fast.wgateup_t)
    qd, kd, inter = fast.qh * fast.hd, fast.kh * fast.hd, gu.shape[0] // 2
    attn, mlp = blk_cpu.self_attn, blk_cpu.mlp
    with torch.no_grad():  # the CPU block holds the weights the GPU block dequantizes
        for lin, w in ((attn.q_proj, qkv[:qd]), (attn.k_proj, qkv[qd : qd + kd]), (attn.v_proj, qkv[qd + kd :]),
                       (attn.o_proj, deq(fast.wo_t)), (mlp.gate_proj, gu[:inter]), (mlp.up_proj, gu[inter:]),
                       (mlp.down_proj, deq(fast.wdown_t))):
            lin.weight.copy_(w)

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
