"""Training attention (`attn_train_fwd` / `attn_train_bwd`, `ops.FusedCausalAttention`)
against float64 attention with float64 autograd gradients on the CPU.

Metric: per (batch, head, row) max_d|g - ref| / max(max_d|ref|, 2^-4 max|ref| of
that (batch, head)); NaN counts as inf. The floor is a condition: row 0 of dQ is
zero in the reference (one visible key, p = 1, dS = 0).

Tolerances follow tests/test_attention_numerics.py: `emulate` is the same maths
in float64 with only the kernels' documented rounding points (q*scale*log2e,
P, dS and the outputs to bf16; D from the bf16 `out`), and TOL_* is 4x its worst
error over CASES, measured on the CPU, never from a kernel's output:

  case (hd, qh, kvh, s)   out     dq      dk      dv
  (64, 1, 1, 1)           0.00000 0.00000 0.00000 0.00000
  (128, 1, 1, 17)         0.00431 0.09743 0.01398 0.00620
  (64, 4, 2, 63)          0.00838 0.05677 0.00915 0.00830
  (128, 4, 2, 64)         0.01050 0.11628 0.02486 0.00735
  (64, 4, 2, 65)          0.00960 0.04375 0.02778 0.00777
  (128, 8, 1, 130)        0.00911 0.06647 0.00671 0.00949
  (64, 8, 1, 200)         0.01133 0.04667 0.00804 0.00949
  (128, 8, 1, 200)        0.01079 0.04866 0.00725 0.00766

dq and dk are the loose ones: dS = p (dP - D) cancels where a row's softmax is
nearly one-hot (sharp K, few visible keys), and D comes from the bf16 `out`.
"""

import functools
import math

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

LOG2E = 1.4426950408889634
B = 2
# (hd, qh, kvh, s): every s, hd and head geometry once; s = 200 with gq 8 for both hd
CASES = [
    (64, 1, 1, 1), (128, 1, 1, 17), (64, 4, 2, 63), (128, 4, 2, 64),
    (64, 4, 2, 65), (128, 8, 1, 130), (64, 8, 1, 200), (128, 8, 1, 200),
]
TOL = {"out": 0.0454, "dq": 0.466, "dk": 0.112, "dv": 0.0380}  # 4 x worst emulated, rounded up


def _bf16(x64):
    return x64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def reference(q, k, v, do, scale):
    """float64 attention on the bf16 input values, gradients by float64 autograd."""
    q, k, v = (t.to(torch.float64).requires_grad_() for t in (q, k, v))
    rep = q.shape[1] // k.shape[1]
    s = q.shape[2]
    logits = torch.einsum("bhsd,bhld->bhsl", q, k.repeat_interleave(rep, dim=1)) * scale
    logits = logits.masked_fill(torch.ones(s, s, dtype=torch.bool).triu(1), float("-inf"))
    out = torch.einsum("bhsl,bhld->bhsd", torch.softmax(logits, -1), v.repeat_interleave(rep, dim=1))
    out.backward(do.to(torch.float64))
    return {"out": out.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def emulate(q, k, v, do, scale):
    """The kernels' maths in float64 with their rounding points only."""
    b, qh, s, hd = q.shape
    kvh = k.shape[1]
    rep = qh // kvh
    qs = (q.to(torch.float32) * (torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)))
    qs = qs.to(torch.bfloat16).to(torch.float64)
    q64, do64 = q.to(torch.float64), do.to(torch.float64)
    k64 = k.to(torch.float64).repeat_interleave(rep, dim=1)
    v64 = v.to(torch.float64).repeat_interleave(rep, dim=1)
    dead = torch.ones(s, s, dtype=torch.bool).triu(1)
    s2 = torch.einsum("bhsd,bhld->bhsl", qs, k64).masked_fill(dead, float("-inf"))
    m = s2.amax(-1, keepdim=True)
    pu = torch.exp2(s2 - m)
    l = pu.sum(-1, keepdim=True)
    out = _bf16(torch.einsum("bhsl,bhld->bhsd", _bf16(pu), v64) / l)
    lse2 = (m + torch.log2(l)).to(torch.float32).to(torch.float64)
    p = torch.exp2(s2 - lse2)
    delta = (do64 * out).sum(-1, keepdim=True)
    ds = _bf16(p * (torch.einsum("bhsd,bhld->bhsl", do64, v64) - delta))
    dv = torch.einsum("bhsl,bhsd->bhld", _bf16(p), do64).view(b, kvh, rep, s, hd).sum(2)
    dk = scale * torch.einsum("bhsl,bhsd->bhld", ds, q64).view(b, kvh, rep, s, hd).sum(2)
    dq = scale * torch.einsum("bhsl,bhld->bhsd", ds, k64)
    return {"out": out, "dq": _bf16(dq), "dk": _bf16(dk), "dv": _bf16(dv)}


def row_err(got, ref, cancel):
    """`cancel` stands in where the metric's denominator is 0, which is a whole
    (batch, head) of zeros in the reference: dq and dk at s = 1, where
    dS = p (dP - D) cancels exactly. It is the size of the two cancelling terms,
    scale |dP| max(|q|, |k|), against which fp32 sums leave a residue."""
    ref = ref.to(torch.float64)
    diff = torch.nan_to_num((got.to(torch.float64) - ref).abs(), nan=float("inf"), posinf=float("inf"))
    row_max = ref.abs().amax(-1)
    denom = torch.maximum(row_max, row_max.amax(-1, keepdim=True) / 16)
    return (diff.amax(-1) / torch.where(denom == 0, cancel, denom)).max().item()


@functools.lru_cache(maxsize=None)
def problem(hd, qh, kvh, s, do_row=None):
    """Sharp inputs (K ~ 2 N(0,1)) rounded to bf16, and their float64 reference.
    `do_row`: dO is zero outside that q row."""
    g = torch.Generator().manual_seed(1000 * hd + 100 * qh + 10 * kvh + s)
    q = torch.randn(B, qh, s, hd, generator=g).to(torch.bfloat16)
    k = (2.0 * torch.randn(B, kvh, s, hd, generator=g)).to(torch.bfloat16)
    v = torch.randn(B, kvh, s, hd, generator=g).to(torch.bfloat16)
    do = torch.randn(B, qh, s, hd, generator=g).to(torch.bfloat16)
    if do_row is not None:
        keep = torch.zeros(s, 1, dtype=torch.bool)
        keep[do_row] = True
        do = do * keep
    scale = 1.0 / math.sqrt(hd)
    dp = torch.einsum("bhsd,bhld->bhsl", do.double(), v.double().repeat_interleave(qh // kvh, dim=1))
    cancel = scale * dp.abs().max() * max(q.double().abs().max(), k.double().abs().max())
    return (q, k, v, do, scale), reference(q, k, v, do, scale), cancel


@pytest.mark.parametrize("case", CASES, ids=str)
def test_emulated_error_within_quarter_tol(case):
    args, ref, cancel = problem(*case)
    emu = emulate(*args)
    errs = {name: row_err(emu[name], ref[name], cancel) for name in TOL}
    print(case, " ".join(f"{n}={e:.5f}" for n, e in errs.items()))
    for name, e in errs.items():
        assert e <= TOL[name] / 4, (name, e)


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


def _guarded(x):
    """The leading B entries of a B + 1 allocation whose last entry is NaN."""
    full = torch.cat([x, torch.full_like(x[:1], float("nan"))]).cuda()
    return full[: x.shape[0]]


def _run(hip, args, gq_splits):
    q, k, v, do, scale = args
    q, k, v, do = (_guarded(t) for t in (q, k, v, do))
    out, lse2 = hip.attn_train_fwd(q, k, v, scale)
    dq, dk, dv = hip.attn_train_bwd(q, k, v, out, lse2, do, scale, gq_splits)
    return {"out": out.cpu(), "dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_attn_train_numerics(hip, case):
    """out, dq, dk, dv against float64, with the GQA sum in registers
    (gq_splits 1), split in two, and under the kernel's own split policy (0);
    every variant twice with identical bits."""
    args, ref, cancel = problem(*case)
    gq = case[1] // case[2]
    for gq_splits in sorted({1, 2 if gq % 2 == 0 else 1, 0}):
        got, again = _run(hip, args, gq_splits), _run(hip, args, gq_splits)
        for name in TOL:
            e = row_err(got[name], ref[name], cancel)
            print(f"{case} gq_splits={gq_splits} {name}: err={e:.5f} tol={TOL[name]}")
            assert e <= TOL[name], (name, gq_splits, e)
            assert torch.equal(got[name].view(torch.int16), again[name].view(torch.int16)), (name, gq_splits)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("i", [0, 63, 64, 129])
def test_single_row_dout_gives_exact_zeros(hip, i):
    """dO nonzero in q row i only (s = 130): every other dq row, and every
    dk / dv row of a key > i, is exactly 0.0; the live dv rows hold p[i][j] dO[i]."""
    args, ref, cancel = problem(128, 4, 2, 130, do_row=i)
    for gq_splits in (1, 0):
        got = _run(hip, args, gq_splits)
        other = torch.arange(130) != i
        assert (got["dq"][:, :, other] == 0).all()
        assert (got["dk"][:, :, i + 1 :] == 0).all() and (got["dv"][:, :, i + 1 :] == 0).all()
        for name in ("dq", "dk", "dv"):
            assert row_err(got[name], ref[name], cancel) <= TOL[name], name


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("preset", ["test-llama-hd128", "test-mixtral-hd64"])
def test_block_training_fused_matches_torch(hip, monkeypatch, preset):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    blk = blk.to("cuda", torch.bfloat16).eval().optimize_for_inference("none")
    assert blk._fast is not None
    attn_outs = []
    real = fused_decode._train_attention
    monkeypatch.setattr(fused_decode, "_train_attention", lambda *a: attn_outs.append(real(*a)) or attn_outs[-1])

    torch.manual_seed(5)
    x0 = (torch.randn(2, 70, cfg.hidden_size) * 0.5).cuda().bfloat16()
    dy = torch.randn(2, 70, cfg.hidden_size).cuda().bfloat16()
    res = {}
    for mode in (None, "fused"):
        if mode is None:
            monkeypatch.delenv("PETALS_AMD_TRAIN_ATTN", raising=False)
        else:
            monkeypatch.setenv("PETALS_AMD_TRAIN_ATTN", mode)
        x = x0.clone().requires_grad_()
        y = blk(x)
        y.backward(dy)
        res[mode] = (y.detach().float().cpu(), x.grad.float().cpu())
        is_fused = type(attn_outs[-1].grad_fn).__name__ == "FusedCausalAttentionBackward"
        assert is_fused == (mode == "fused")
    for a, b_ in zip(res["fused"], res[None]):
        assert torch.isfinite(a).all()
        assert (a - b_).abs().max() <= 2e-2 * b_.abs().max(), ((a - b_).abs().max(), b_.abs().max())


def test_train_attn_plumbing(monkeypatch):
    import inspect

    from petals_amd import ops
    from petals_amd.cli import run_server as rs
    from petals_amd.server.server import Server

    monkeypatch.delenv("PETALS_AMD_TRAIN_ATTN", raising=False)
    assert ops.train_attn_mode() == "torch"
    assert inspect.signature(Server.__init__).parameters["train_attn"].default == "torch"
    monkeypatch.setenv("PETALS_AMD_TRAIN_ATTN", "fused")
    assert ops.train_attn_mode() == "fused"  # read at call time
    monkeypatch.setenv("PETALS_AMD_TRAIN_ATTN", "flash")
    with pytest.raises(ValueError, match="expected one of"):
        ops.train_attn_mode()
    monkeypatch.setenv("PETALS_AMD_TRAIN_ATTN", "torch")
    with pytest.raises(ValueError, match="expected one of"):
        ops.set_train_attn_mode("flash")
    with pytest.raises(ValueError, match="expected one of"):
        Server("test-llama", device="cpu", num_blocks=1, train_attn="flash")
    assert ops.train_attn_mode() == "torch"
    Server("test-llama", device="cpu", num_blocks=1, train_attn="fused")
    assert ops.train_attn_mode() == "fused"

    # CLI: parsed, validated, handed to Server
    monkeypatch.setenv("PETALS_AMD_TRAIN_ATTN", "torch")
    captured = {}

    class _Stop(Exception):
        pass

    def fake_server(*a, **kw):
        captured.update(kw)
        raise _Stop

    monkeypatch.setattr(rs, "Server", fake_server, raising=False)
    monkeypatch.setattr("petals_amd.server.server.Server", fake_server)
    with pytest.raises(_Stop):
        rs.main(["test-llama", "--train_attn", "fused"])
    assert captured["train_attn"] == "fused" and ops.train_attn_mode() == "fused"
    with pytest.raises(SystemExit):
        rs.main(["test-llama", "--train_attn", "flash"])

    # CPU tensors in fused mode silently take the torch path
    q = torch.randn(1, 2, 5, 64, dtype=torch.bfloat16, requires_grad=True)
    k, v = torch.randn(2, 1, 2, 5, 64, dtype=torch.bfloat16)
    out = ops.attention(q, k, v, causal=True)
    assert "FusedCausalAttention" not in type(out.grad_fn).__name__
    assert torch.equal(out, ops.reference.attention(q, k, v, causal=True))
