"""Multi-token decode step (PETALS_AMD_MULTI_DECODE=on): T = 2..8 new tokens per
sequence against the KV cache on the decode kernel chain.

  1. attn_decode_multi against float64 causal attention, with a needle on each
     token's own key (`diag`: a mask one key early drops it) or on the first key
     it must not see (`forbid`: a mask one key late lets it in);
  2. the T-token cache writers against float64;
  3. LlamaBlock.forward(S=4) under mode `on` against four decode_steps;
  4. a served speculative generate() against plain greedy generate().

Tolerance of (1): the kernel has the decode kernel's rounding points, so the
bound is TOL_DECODE. `test_emulated_error_within_quarter_tol` recomputes, on the
CPU, the error of the float64 emulation of those rounding points on exactly the
inputs below (worst 0.0092, the fp8 rows included) and holds it under
TOL_DECODE / 4.
"""

import functools
import math

import pytest
import torch

from petals_amd.ops import kv_fp8
from test_attention_numerics import (
    TOL_DECODE,
    _gen,
    _ordered_bits,
    _sharp_kv,
    _unit,
    emulated_attention_f64,
    mfma_auto_splits,
    nerr,
    ref_attention_f64,
)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

# (B, KV, GQ, T, kv_len, lmax, HD): one and several row groups (two passes at
# two groups per pass), padded and full groups, tile edges 32/33, 64, 97, a
# cache of only the new tokens, idle waves, 1..many auto splits, B > 1
CASES = [
    (1, 2, 8, 2, 33, 64, 128),
    (1, 2, 8, 4, 64, 128, 128),
    (1, 1, 8, 8, 97, 256, 128),
    (2, 2, 4, 3, 40, 64, 64),
    (1, 2, 1, 8, 32, 64, 64),
    (1, 1, 16, 2, 700, 1024, 128),
    (1, 2, 6, 5, 129, 2048, 128),
    (1, 1, 8, 8, 8, 64, 128),
    (1, 2, 8, 4, 1300, 4096, 64),
]
# (case, n_splits (0 = the host's policy), fp8 cache)
RUNS = [(c, 0, False) for c in CASES]
RUNS += [(CASES[2], 1, False), (CASES[2], 5, False), (CASES[6], 1, False), (CASES[6], 5, False)]
RUNS += [(CASES[1], 0, True), (CASES[6], 0, True)]
ATTN_PARAMS = [
    pytest.param(c, ns, fp8, pat, id="-".join(map(str, c)) + f"-s{ns}" + ("-fp8" if fp8 else "") + f"-{pat}")
    for c, ns, fp8 in RUNS
    for pat in ("diag", "forbid")
]


@functools.lru_cache(maxsize=None)
def attn_inputs(case, pattern, fp8):
    """q [B, H, T, D] f32, k / v [B, KV, lmax, D] bf16 (on the E4M3 grid for
    fp8) with V = 1e4 past kv_len, and the float64 reference."""
    b, kvh, gq, t_n, kv_len, lmax, hd = case
    g = _gen(f"multi-{case}-{pattern}")
    k, v = _sharp_kv(g, b, kvh, lmax, hd)
    q = torch.randn(b, kvh * gq, t_n, hd, generator=g)
    qhat = _unit(q)
    for bi in range(b):
        for kh in range(kvh):
            for t in range(t_n - (pattern == "forbid")):  # the last token's forbidden key is the V poison
                key = kv_len - t_n + t + (pattern == "forbid")
                k[bi, kh, key] = (16.0 * qhat[bi, kh * gq + (t + bi) % gq, t]).to(torch.bfloat16)
    v[:, :, kv_len:] = 1.0e4
    if fp8:
        k, v = kv_fp8.roundtrip(k), kv_fp8.roundtrip(v)
    scale = 1.0 / math.sqrt(hd)
    args = (q, k, v, kv_len, scale, True, kv_len - t_n)
    return q, k, v, scale, ref_attention_f64(*args), emulated_attention_f64(*args)


def test_emulated_error_within_quarter_tol():
    worst = 0.0
    for p in ATTN_PARAMS:
        case, _, fp8, pattern = p.values
        *_, ref, emulated = attn_inputs(case, pattern, fp8)
        e = nerr(emulated, ref)
        print(f"multi emulated {p.id}: nerr={e:.5f}")
        worst = max(worst, e)
    assert worst <= TOL_DECODE / 4, worst


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case,n_splits,fp8,pattern", ATTN_PARAMS)
def test_attn_decode_multi_numerics(hip, case, n_splits, fp8, pattern):
    """Against float64 with 1e4- and NaN-poisoned cache tails and NaN-filled
    workspaces; every call twice, bit-identical."""
    b, kvh, gq, t_n, kv_len, lmax, hd = case
    q, k, v, scale, ref, _ = attn_inputs(case, pattern, fp8)
    ns = n_splits or mfma_auto_splits(b, kvh, lmax)
    q_dev = q.permute(0, 2, 1, 3).reshape(b * t_n, kvh * gq * hd).contiguous().cuda()  # row b*T + t
    pos = torch.tensor([kv_len - t_n], dtype=torch.int32, device="cuda")
    to_cache = (lambda x: kv_fp8.quantize(x).cuda()) if fp8 else (lambda x: x.cuda())
    k_dev = to_cache(k)
    v_nan = v.clone()
    v_nan[:, :, kv_len:] = float("nan")
    for vv in (v, v_nan):
        v_dev = to_cache(vv)
        outs = []
        for _ in range(2):
            part_o = torch.full((b * kvh * ns * t_n * gq * hd + 4099,), float("nan"), device="cuda")
            part_ml = torch.full((b * kvh * ns * t_n * gq * 2 + 131,), float("nan"), device="cuda")
            out = hip.attn_decode_multi(q_dev, k_dev, v_dev, pos, t_n, gq, n_splits, part_o, part_ml, scale)
            outs.append(out.cpu().view(b, t_n, kvh * gq, hd).permute(0, 2, 1, 3))
        assert torch.equal(outs[0].contiguous().view(torch.int32), outs[1].contiguous().view(torch.int32))
        e = nerr(outs[0], ref)
        print(f"multi {case} splits={ns} fp8={fp8} {pattern}: nerr={e:.5f} tol={TOL_DECODE}")
        assert e <= TOL_DECODE, e


@pytest.mark.gpu
@requires_gpu
def test_attn_decode_multi_refuses_unsupported(hip):
    k = torch.zeros(1, 1, 64, 64, device="cuda", dtype=torch.bfloat16)
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    empty = torch.empty(0, device="cuda")
    with pytest.raises(RuntimeError, match="gq"):  # falcon's multi-group geometry
        hip.attn_decode_multi(torch.zeros(2, 29 * 64, device="cuda"), k, k, pos, 2, 29, 0, empty, empty, 1.0)
    with pytest.raises(RuntimeError, match="tokens"):
        hip.attn_decode_multi(torch.zeros(9, 64, device="cuda"), k, k, pos, 9, 1, 0, empty, empty, 1.0)
    with pytest.raises(RuntimeError):  # 3 rows are no multiple of 2 tokens
        hip.attn_decode_multi(torch.zeros(3, 64, device="cuda"), k, k, pos, 2, 1, 0, empty, empty, 1.0)


# ------------------------------------------------------------------ writers


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("pos", [0, 2040])
@pytest.mark.parametrize("b,t_n", [(2, 2), (1, 8)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kernel", ["qkv_rope_reduce_multi", "rope_cache_write_multi"])
def test_multi_cache_writers(hip, kernel, hd, b, t_n, pos):
    """Row r -> cache batch r // T, position pos + r % T, with that position's
    rope row: q to 1e-5 relative, written rows within 1 bf16 ulp, every other
    byte of both caches (a spare batch row included) untouched."""
    from petals_amd.ops import reference

    qh, kh, lmax, half = 8, 2, 2048, hd // 2
    g = _gen(f"multi-writer-{kernel}-{hd}-{b}-{t_n}-{pos}")
    cos, sin = reference.build_rope_cache(hd, lmax)
    src = torch.randn(3, b * t_n, (qh + 2 * kh) * hd, generator=g)
    if kernel == "rope_cache_write_multi":
        src = src[0].contiguous()
    k0, v0 = _sharp_kv(g, b + 1, kh, lmax, hd)

    heads = (src.to(torch.float64).sum(0) if src.dim() == 3 else src.to(torch.float64)).view(b, t_n, qh + 2 * kh, hd)
    at = pos + torch.arange(t_n)
    c = cos[at, :half].to(torch.float64)[None, :, None, :]
    s = sin[at, :half].to(torch.float64)[None, :, None, :]
    x1, x2 = heads[:, :, : qh + kh, :half], heads[:, :, : qh + kh, half:]
    qk = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    q_ref, k_ref, v_ref = qk[:, :, :qh], qk[:, :, qh:], heads[:, :, qh + kh :]

    k_cache, v_cache = k0.cuda(), v0.cuda()
    pos_t = torch.tensor([pos], dtype=torch.int32, device="cuda")
    src_dev = src.cuda()
    if kernel == "qkv_rope_reduce_multi":
        q = hip.qkv_rope_reduce_multi(src_dev, cos.cuda(), sin.cuda(), pos_t, k_cache, v_cache, qh, kh, t_n)
    else:
        hip.rope_cache_write_multi(src_dev, cos.cuda(), sin.cuda(), pos_t, k_cache, v_cache, qh, kh, t_n)
        q = src_dev[:, : qh * hd]
    q_got = q.cpu().to(torch.float64).view(b, t_n, qh, hd)
    q_err = ((q_got - q_ref).abs().amax(-1) / q_ref.abs().amax(-1)).max().item()
    assert q_err <= 1e-5, q_err
    for got, before, ref in ((k_cache.cpu(), k0, k_ref), (v_cache.cpu(), v0, v_ref)):
        want = ref.transpose(1, 2).to(torch.float32).to(torch.bfloat16)  # [b, kh, T, hd]
        d = (_ordered_bits(got[:b, :, pos : pos + t_n]) - _ordered_bits(want)).abs()
        assert d.max().item() <= 1, d.max()
        rest = got.clone()
        rest[:b, :, pos : pos + t_n] = before[:b, :, pos : pos + t_n]
        assert torch.equal(rest.view(torch.int16), before.view(torch.int16))


# -------------------------------------------------------------------- block


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("quant", ["none", "nf4"])
@pytest.mark.parametrize("preset", ["test-llama-hd128", "test-llama"])
def test_block_multi_step_matches_decode_steps(hip, monkeypatch, preset, quant):
    """Prefill 5, then forward(S=4) under mode `on` against four decode_steps
    on a clone of the cache. `test-llama` (head_dim 16) has no fused path: the
    mode must leave it where it was."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    blk = blk.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant=quant)
    fast = blk._fast
    assert (fast is not None) == (preset == "test-llama-hd128")
    entered = []
    if fast is not None:
        real = fast.decode_multi
        monkeypatch.setattr(fast, "decode_multi", lambda *a, **kw: entered.append(1) or real(*a, **kw), raising=False)

    b, pre, s_n, lmax = 2, 5, 4, 16
    x = (torch.randn(b, pre + s_n, cfg.hidden_size, generator=_gen(f"multi-block-{preset}")) * 0.5).to(torch.bfloat16).cuda()
    ks, vs = blk.kv_cache_shape(b, lmax)
    caches = {name: (torch.zeros(ks, device="cuda", dtype=torch.bfloat16), torch.zeros(vs, device="cuda", dtype=torch.bfloat16))
              for name in ("multi", "steps", "off")}
    with torch.inference_mode():
        monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "off")
        blk(x[:, :pre], kv_cache=caches["steps"], prefix_length=0)
        for name in ("multi", "off"):
            for dst, src in zip(caches[name], caches["steps"]):
                dst.copy_(src)
        y_off = blk(x[:, pre:], kv_cache=caches["off"], prefix_length=pre)
        assert not entered, "mode off entered decode_multi"
        y_steps = torch.cat(
            [blk(x[:, t : t + 1], kv_cache=caches["steps"], prefix_length=t) for t in range(pre, pre + s_n)], 1
        )
        monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "on")
        y_on = blk(x[:, pre:], kv_cache=caches["multi"], prefix_length=pre)
    assert len(entered) == (fast is not None)
    assert torch.allclose(y_on.float(), y_steps.float(), atol=2e-2, rtol=2e-2), (y_on.float() - y_steps.float()).abs().max()
    assert torch.allclose(y_off.float(), y_steps.float(), atol=2e-2, rtol=2e-2)
    for got, want in zip(caches["multi"], caches["steps"]):
        got, want = got.cpu(), want.cpu()
        d = (_ordered_bits(got[:, :, pre : pre + s_n]) - _ordered_bits(want[:, :, pre : pre + s_n])).abs()
        assert d.max().item() <= 1, d.max()
        assert want[:, :, pre : pre + s_n].abs().sum() > 0
        rest = got.clone()
        rest[:, :, pre : pre + s_n] = want[:, :, pre : pre + s_n]
        assert torch.equal(rest.view(torch.int16), want.view(torch.int16))


def test_mode_switch_and_public_knobs(monkeypatch):
    import inspect

    from petals_amd.cli.run_server import build_parser
    from petals_amd.ops.fused_decode import multi_decode_mode, set_multi_decode_mode
    from petals_amd.server.server import Server

    monkeypatch.delenv("PETALS_AMD_MULTI_DECODE", raising=False)
    assert multi_decode_mode() == "off"
    monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "auto")
    with pytest.raises(ValueError, match="expected one of"):
        multi_decode_mode()
    with pytest.raises(ValueError, match="expected one of"):
        set_multi_decode_mode("auto")
    assert inspect.signature(Server.__init__).parameters["multi_decode"].default == "off"
    with pytest.raises(ValueError, match="expected one of"):
        Server("test-llama", device="cpu", num_blocks=1, multi_decode="auto")
    monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "off")
    Server("test-llama", device="cpu", num_blocks=1, multi_decode="on")
    assert multi_decode_mode() == "on"
    p = build_parser()
    assert p.parse_args(["test-llama"]).multi_decode == "off"
    assert p.parse_args(["test-llama", "--multi_decode", "on"]).multi_decode == "on"


# ------------------------------------------------------------------- served


@pytest.mark.gpu
@requires_gpu
def test_served_speculative_generate_matches_greedy(monkeypatch):
    """A server with multi_decode="on": speculative generate() with a draft
    that is always wrong verifies 4 tokens per step through decode_multi,
    rejects, rolls the position back, and returns greedy generate()'s tokens."""
    from petals_amd.dht.node import DHT
    from petals_amd.models.llama.speculative_model import DistributedLlamaForSpeculativeGeneration
    from petals_amd.ops.fused_decode import LlamaFastPath
    from petals_amd.server.server import Server
    from petals_amd.utils.auto_config import AutoDistributedModelForCausalLM

    monkeypatch.setenv("PETALS_AMD_MULTI_DECODE", "off")  # restored afterwards; the server turns it on
    steps = []
    real = LlamaFastPath.decode_multi
    monkeypatch.setattr(LlamaFastPath, "decode_multi", lambda self, h, *a, **kw: steps.append(h.shape[1]) or real(self, h, *a, **kw))

    class WrongDraft:
        def __call__(self, input_ids):
            logits = torch.zeros(1, input_ids.shape[1], 128)
            logits[0, -1, (int(input_ids[0, -1]) + 1 + input_ids.shape[1]) % 128] = 1.0
            return type("Out", (), {"logits": logits})

    preset, prefix = "test-llama-hd128", "gpu-multi-decode"
    boot = DHT(host="127.0.0.1")
    server = Server(
        preset, initial_peers=[boot.listen_addr], host="127.0.0.1", device="cuda", torch_dtype="bfloat16",
        block_indices="0:4", dht_prefix=prefix, throughput=1.0, multi_decode="on",
    ).start()
    try:
        model = AutoDistributedModelForCausalLM.from_pretrained(
            preset, initial_peers=[boot.listen_addr], dht_prefix=prefix, show_route=False, max_retries=1,
        )
        ids = torch.randint(0, 128, (1, 5), generator=_gen("multi-served"))
        greedy = model.generate(ids, max_new_tokens=6, do_sample=False)
        spec = DistributedLlamaForSpeculativeGeneration(model, WrongDraft()).generate(
            ids, max_new_tokens=6, speculative_tokens=4
        )
        assert 4 in steps, steps  # the verify steps (the 5-token prefill takes the chain too)
        assert torch.equal(spec, greedy), (spec, greedy)
        model.transformer.h.sequence_manager.shutdown()
    finally:
        server.shutdown()
        boot.shutdown()
