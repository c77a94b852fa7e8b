"""Fused NF4/int8 dequant MFMA GEMM for prefill projections
(ops/csrc/gemm_quant.hip, _FastWeight.matmul, PETALS_AMD_PREFILL_GEMM).

GPU tests: an exact index-mapping test (one-hot rows select weight rows, bit
for bit), a random-data test against float64 with a derived per-element bound,
and block-level dense-vs-fused prefills. CPU tests: the mode helper, the
eligibility function, the fallbacks of _FastWeight.matmul, and a self-check
that the float64 bound rejects three corrupted references.

Shapes are the smallest that can still go wrong for the kernel's 128x128 C
tile and 64-wide k step."""

import functools

import pytest
import torch

from petals_amd.ops import nf4 as nf4_ref

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

TILE = 128  # C tile rows and columns of gemm_quant.hip
# 1 and 5; one below / at / above a row-tile edge; one M spanning 3 row tiles
M_CASES = (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 44)
OUT_CASES = (64, TILE + 64, 3 * TILE)  # half tile; tile + ragged half; multi-tile
# single k-step; odd k-steps (buffer parity); 8 steps = two even split-K slices
# (these small grids split as soon as in >= 512); 9 steps = slices of 4, 4 and 1
IN_CASES = (64, 192, 512, 576)
M_MAX = max(M_CASES)


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared fixtures


def _int8_quantize(w_bf16: torch.Tensor):
    """_FastWeight's weight-only int8: per-out-column symmetric absmax."""
    w = w_bf16.float()
    scale = w.abs().amax(dim=0).clamp_min(1e-8) / 127.0
    q8 = torch.round(w / scale).clamp(-127, 127).to(torch.int8).contiguous()
    return q8, scale.to(torch.bfloat16).contiguous()


@functools.lru_cache(maxsize=None)
def _weights(in_dim: int, out_dim: int):
    """Random W (scale ~0.05) whose every (row, 64-column block) is multiplied
    by a random power of two in [2^-3, 2^3], so a wrong absmax index cannot
    hide; quantized on the CPU in both formats. Built once per shape."""
    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    w = torch.randn(in_dim, out_dim, generator=g) * 0.05
    pw = torch.randint(-3, 4, (in_dim, out_dim // 64), generator=g).float()
    w = (w * torch.exp2(pw).repeat_interleave(64, dim=1)).to(torch.bfloat16)
    packed, absmax = nf4_ref.quantize(w)
    q8, scale8 = _int8_quantize(w)
    bias = (torch.randn(out_dim, generator=g) * 0.5).to(torch.bfloat16)
    return dict(
        packed=packed, absmax=absmax, q8=q8, scale8=scale8, bias=bias,
        deq_nf4=nf4_ref.dequantize(packed, absmax),  # bf16, the CPU reference dequantizer
        deq_int8=q8.double() * scale8.double(),  # exact: the scale meets the fp32 accumulator
    )


@functools.lru_cache(maxsize=None)
def _x_random(in_dim: int):
    g = torch.Generator().manual_seed(77 + in_dim)
    return torch.randn(M_MAX, in_dim, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _x_onehot(in_dim: int):
    """One 1.0 per row at column perm(m): a random permutation, repeated when
    there are more rows than columns."""
    g = torch.Generator().manual_seed(5 + in_dim)
    perm = torch.cat([torch.randperm(in_dim, generator=g) for _ in range(-(-M_MAX // in_dim))])[:M_MAX]
    x = torch.zeros(M_MAX, in_dim, dtype=torch.bfloat16)
    x[torch.arange(M_MAX), perm] = 1.0
    return x, perm


def _run(hip, quant, w, x_gpu, bias_gpu=None):
    if quant == "nf4":
        return hip.gemm_nf4(w["packed"].cuda(), w["absmax"].cuda(), x_gpu, bias_gpu)
    return hip.gemm_int8(w["q8"].cuda(), w["scale8"].cuda(), x_gpu, bias_gpu)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def _bound(ref: torch.Tensor, x: torch.Tensor, wdeq: torch.Tensor) -> torch.Tensor:
    """Per-element bound on |out - ref|, derived and not measured: 2^-8 |ref|
    for the one bf16 rounding of the result (twice 2^-9; bf16 keeps 8
    significant bits, so a half ulp reaches 2^-8 |ref| at the bottom of a
    binade and measured ratios sit just under 1), plus twice the worst-case
    fp32 summation error over `in` terms (2 * in * 2^-24 * sum |x||w|)."""
    in_dim = x.shape[1]
    return 2.0 ** -8 * ref.abs() + in_dim * 2.0 ** -23 * (x.double().abs() @ wdeq.double().abs())


# ------------------------------------------------------------------ GPU: exact


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim", IN_CASES)
@pytest.mark.parametrize("out_dim", OUT_CASES)
@pytest.mark.parametrize("quant", ["nf4", "int8"])
def test_gemm_quant_index_mapping_exact(hip, quant, out_dim, in_dim):
    """Row m of the output is row perm(m) of the dequantized weight, bit for
    bit: nibble order, swizzle, absmax indexing, k-tile order and the row/col
    mapping, with no tolerance at all."""
    w = _weights(in_dim, out_dim)
    x, perm = _x_onehot(in_dim)
    if quant == "nf4":
        rows = w["deq_nf4"]
    else:  # one fp32 product of the stored bf16 scale, rounded once
        rows = (w["q8"].float() * w["scale8"].float()).to(torch.bfloat16)
    assert (rows.float().abs() >= 2.0 ** -126).logical_or(rows == 0).all(), "nothing subnormal"
    for m in M_CASES:
        out = _run(hip, quant, w, x[:m].cuda())
        assert out.shape == (m, out_dim) and out.dtype == torch.bfloat16
        again = _run(hip, quant, w, x[:m].cuda())
        out, again = out.cpu(), again.cpu()
        assert torch.equal(_bits(out), _bits(again)), f"M={m}: two runs differ"
        want = rows[perm[:m]]
        bad = (_bits(out) != _bits(want)).nonzero()
        assert bad.numel() == 0, f"M={m}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


# ------------------------------------------------------ GPU: random vs float64


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("in_dim", IN_CASES)
@pytest.mark.parametrize("out_dim", OUT_CASES)
@pytest.mark.parametrize("quant", ["nf4", "int8"])
def test_gemm_quant_random_vs_float64(hip, quant, out_dim, in_dim, with_bias):
    w = _weights(in_dim, out_dim)
    x = _x_random(in_dim)
    wdeq = w["deq_nf4"] if quant == "nf4" else w["deq_int8"]
    ref_all = x.double() @ wdeq.double()
    if with_bias:
        ref_all = ref_all + w["bias"].double()
    bound_all = _bound(ref_all, x, wdeq)
    bias_gpu = w["bias"].cuda() if with_bias else None
    for m in M_CASES:
        out = _run(hip, quant, w, x[:m].cuda(), bias_gpu)
        again = _run(hip, quant, w, x[:m].cuda(), bias_gpu)
        out, again = out.cpu(), again.cpu()
        assert torch.equal(_bits(out), _bits(again)), f"M={m}: two runs differ"
        err = (out.double() - ref_all[:m]).abs()
        ratio = (err / bound_all[:m].clamp_min(1e-300)).max().item()
        print(f"{quant} in={in_dim} out={out_dim} M={m} bias={with_bias}: max err/bound = {ratio:.3f}")
        assert (err <= bound_all[:m]).all(), f"M={m}: max err/bound = {ratio:.3f}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("quant", ["nf4", "int8"])
def test_fastweight_matmul_batched_input(hip, quant, monkeypatch):
    """[B, S, in] through _FastWeight.matmul in fused mode: leading dims are
    flattened and restored, the bias lands in the epilogue."""
    in_dim, out_dim = 192, TILE + 64
    w = _weights(in_dim, out_dim)
    fw = _stub_weight(quant, w, hip, device="cuda")
    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "fused")
    B, S = 3, 47  # 141 rows: two row tiles, the second ragged
    x = _x_random(in_dim)[: B * S].reshape(B, S, in_dim)
    wdeq = w["deq_nf4"] if quant == "nf4" else w["deq_int8"]
    ref = x.double() @ wdeq.double() + w["bias"].double()
    out = fw.matmul(x.cuda(), w["bias"].cuda())
    assert out.shape == (B, S, out_dim) and out.dtype == torch.bfloat16
    assert torch.equal(_bits(out.cpu()), _bits(fw.matmul(x.cuda(), w["bias"].cuda()).cpu()))
    err = (out.cpu().double() - ref).abs().reshape(B * S, out_dim)
    assert (err <= _bound(ref.reshape(B * S, out_dim), x.reshape(B * S, in_dim), wdeq)).all()
    from petals_amd.ops import fused_decode

    assert id(fw) not in (fused_decode._dequant_cache or {}), "fused mode must not dequantize"


@requires_gpu
@pytest.mark.gpu
def test_gemm_quant_rejects_bad_operands(hip):
    w = _weights(64, 64)
    x = _x_random(64)[:4].cuda()
    with pytest.raises(RuntimeError):  # fp32 x
        hip.gemm_nf4(w["packed"].cuda(), w["absmax"].cuda(), x.float(), None)
    with pytest.raises(RuntimeError):  # non-contiguous x
        hip.gemm_nf4(w["packed"].cuda(), w["absmax"].cuda(), _x_random(64)[:, :64].cuda().t(), None)
    with pytest.raises(RuntimeError):  # in % 64 != 0
        hip.gemm_int8(w["q8"][:32].contiguous().cuda(), w["scale8"].cuda(), x[:, :32].contiguous(), None)
    with pytest.raises(RuntimeError):  # bias of the wrong length
        hip.gemm_int8(w["q8"].cuda(), w["scale8"].cuda(), x, w["bias"][:32].contiguous().cuda())


# ------------------------------------------------------------ GPU: block level


def _prefill_both_modes(monkeypatch, preset, quant):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    blk = blk.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant=quant)
    assert blk._fast is not None and blk._fast.quant == quant

    torch.manual_seed(11)
    B, S1, S2 = 2, 37, 9
    x = (torch.randn(B, S1 + S2, cfg.hidden_size) * 0.5).cuda().bfloat16()
    ks, vs = blk.kv_cache_shape(B, 64)
    results = {}
    for mode in ("dense", "fused"):
        monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", mode)
        fused_decode._dequant_cache = None  # a fresh process-wide cache
        fused_decode._dequant_cache_bytes = 0
        k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
        with torch.inference_mode():
            y1 = blk(x[:, :S1], kv_cache=(k, v), prefix_length=0)
            y2 = blk(x[:, S1:], kv_cache=(k, v), prefix_length=S1)  # a second chunk on the cache
        results[mode] = (torch.cat([y1, y2], 1).float().cpu(), k.float().cpu(), v.float().cpu(),
                         fused_decode._dequant_cache_bytes)
    fused_decode._dequant_cache = None
    fused_decode._dequant_cache_bytes = 0
    return results, S1 + S2


def _assert_modes_agree(results, written):
    yd, kd, vd, bytes_dense = results["dense"]
    yf, kf, vf, bytes_fused = results["fused"]
    assert bytes_dense > 0, "dense mode dequantizes through the LRU"
    assert bytes_fused == 0, "fused mode must leave the dequant LRU empty"
    assert torch.isfinite(yf).all()
    assert torch.allclose(yf, yd, atol=2e-2, rtol=2e-2), (yf - yd).abs().max()
    assert kd[:, :, :written].abs().sum() > 0
    assert torch.allclose(kf[:, :, :written], kd[:, :, :written], atol=2e-2, rtol=2e-2)
    assert torch.allclose(vf[:, :, :written], vd[:, :, :written], atol=2e-2, rtol=2e-2)
    assert kf[:, :, written:].abs().sum() == 0 and vf[:, :, written:].abs().sum() == 0


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("preset,quant", [
    ("test-llama-hd128", "nf4"), ("test-bloom-hd64", "nf4"), ("test-llama-hd128", "int8"),
])
def test_block_prefill_fused_matches_dense(hip, monkeypatch, preset, quant):
    results, written = _prefill_both_modes(monkeypatch, preset, quant)
    _assert_modes_agree(results, written)


# ------------------------------------------------------------------------ CPU


class _StubHip:
    """Stands in for the extension: the fused ops must not be reached."""

    def gemm_nf4(self, *a, **k):
        raise AssertionError("fused gemm_nf4 must not be called here")

    gemm_int8 = gemm_nf4

    def nf4_dequantize(self, packed, absmax):
        return nf4_ref.dequantize(packed.cpu(), absmax.cpu()).to(packed.device)


def _stub_weight(quant, w, hip, device="cpu"):
    """A _FastWeight around already-quantized tensors (skips the load-time
    GPU quantizer and gemv autotune)."""
    from petals_amd.ops.fused_decode import _FastWeight

    fw = _FastWeight.__new__(_FastWeight)
    fw.hip, fw.quant = hip, quant
    fw.t = fw.packed = fw.absmax = fw.absmax_t = fw.q8 = fw.scale8 = None
    if quant == "nf4":
        fw.packed, fw.absmax = w["packed"].to(device), w["absmax"].to(device)
        fw.in_dim, fw.out_dim = fw.packed.shape[0], fw.packed.shape[1] * 2
    else:
        fw.q8, fw.scale8 = w["q8"].to(device), w["scale8"].to(device)
        fw.in_dim, fw.out_dim = fw.q8.shape
    fw.splits = 0
    return fw


def test_prefill_gemm_mode_parsing(monkeypatch):
    from petals_amd.ops.fused_decode import prefill_gemm_mode, set_prefill_gemm_mode

    monkeypatch.delenv("PETALS_AMD_PREFILL_GEMM", raising=False)
    assert prefill_gemm_mode() == "dense"
    for mode in ("dense", "fused"):
        monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", mode)
        assert prefill_gemm_mode() == mode  # read at call time
    for bad in ("", "Fused", "1", "rocblas"):
        monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", bad)
        with pytest.raises(ValueError):
            prefill_gemm_mode()
    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "dense")
    set_prefill_gemm_mode("fused")
    assert prefill_gemm_mode() == "fused"
    with pytest.raises(ValueError):
        set_prefill_gemm_mode("auto")
    assert prefill_gemm_mode() == "fused"


def test_fused_gemm_eligibility():
    from petals_amd.ops.fused_decode import fused_gemm_eligible

    from petals_amd.ops.fused_decode import FUSED_GEMM_MAX_ROWS

    assert fused_gemm_eligible("nf4", 1, 64, 64)
    assert fused_gemm_eligible("int8", 128, 8192, 57344)
    for quant, max_rows in FUSED_GEMM_MAX_ROWS.items():  # the measured crossover in rows
        assert fused_gemm_eligible(quant, max_rows, 4544, 4672)  # falcon-7b qkv: out = 73 * 64
        assert not fused_gemm_eligible(quant, max_rows + 1, 4544, 4672)
    assert not fused_gemm_eligible("nf4", 2048, 8192, 57344)
    assert not fused_gemm_eligible("nf4", 16, 96, 128)  # in % 64 != 0
    assert not fused_gemm_eligible("int8", 16, 4544 + 32, 4672)
    assert not fused_gemm_eligible("int8", 16, 128, 96)  # out % 64 != 0
    assert not fused_gemm_eligible("none", 16, 128, 128)  # bf16 weights stay on rocBLAS
    assert not fused_gemm_eligible("nf4", 0, 128, 128)


def test_server_and_cli_prefill_gemm_knob(monkeypatch):
    import inspect

    import petals_amd.cli.run_server as rs
    from petals_amd.ops.fused_decode import prefill_gemm_mode
    from petals_amd.server.server import Server

    assert inspect.signature(Server.__init__).parameters["prefill_gemm"].default == "dense"
    with pytest.raises(ValueError):
        Server("test-llama", device="cpu", num_blocks=1, prefill_gemm="auto")

    captured = {}

    class FakeServer:
        listen_addr = ("0.0.0.0", 0)
        peer_id = "fake"

        def __init__(self, model, **kwargs):
            captured.update(kwargs)

        def start(self):
            return self

        def is_healthy(self):
            return False

        def shutdown(self):
            pass

    monkeypatch.setattr("petals_amd.server.server.Server", FakeServer)
    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "dense")
    rs.main(["test-llama"])
    assert captured["prefill_gemm"] == "dense" and prefill_gemm_mode() == "dense"
    rs.main(["test-llama", "--prefill_gemm", "fused"])
    assert captured["prefill_gemm"] == "fused" and prefill_gemm_mode() == "fused"
    with pytest.raises(SystemExit):
        rs.main(["test-llama", "--prefill_gemm", "auto"])


@pytest.mark.parametrize("quant", ["nf4", "int8"])
def test_fastweight_matmul_falls_back_to_dense(monkeypatch, quant):
    """dense mode, and fused mode while autograd records, both run
    torch.matmul on dense() (+ bias); the stub raises if a fused op is hit."""
    from petals_amd.ops import fused_decode

    w = _weights(64, 64)
    fw = _stub_weight(quant, w, _StubHip())
    monkeypatch.setattr(fused_decode, "_dequant_cache", None)
    monkeypatch.setattr(fused_decode, "_dequant_cache_bytes", 0)
    x = _x_random(64)[:6].reshape(2, 3, 64)
    want = torch.matmul(x, fw.dense())

    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "dense")
    assert torch.equal(fw.matmul(x), want)
    assert torch.equal(fw.matmul(x, w["bias"]), want + w["bias"])

    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "fused")
    xg = x.clone().requires_grad_(True)
    out = fw.matmul(xg, w["bias"])
    assert out.requires_grad and torch.equal(out.detach(), want + w["bias"])
    out.float().sum().backward()
    assert xg.grad is not None and xg.grad.shape == x.shape

    monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", "bogus")
    with pytest.raises(ValueError):
        fw.matmul(x)


def test_float64_bound_rejects_corrupted_references():
    """The bound of the random-data test is tight enough to matter: each of
    three corrupted NF4 references (one 64-wide k-step dropped, one absmax
    block shifted by one, nibbles swapped) violates it by at least 2x on at
    least one case, while the bf16-rounded true product stays inside it."""
    worst = {"k-step dropped": 0.0, "absmax block shifted": 0.0, "nibbles swapped": 0.0}
    for in_dim in IN_CASES:
        for out_dim in OUT_CASES:
            w = _weights(in_dim, out_dim)
            x = _x_random(in_dim)[:TILE + 1]
            wdeq = w["deq_nf4"]
            ref = x.double() @ wdeq.double()
            bound = _bound(ref, x, wdeq).clamp_min(1e-300)
            honest = ref.to(torch.bfloat16).double()
            assert ((honest - ref).abs() <= bound).all()

            k0 = 64 * ((in_dim // 64) // 2)
            xd = x.clone()
            xd[:, k0 : k0 + 64] = 0
            shifted = w["absmax"].clone()
            j = (out_dim // 64) // 2
            shifted[:, j] = w["absmax"][:, (j + 1) % (out_dim // 64)]  # no-op at out = 64: one block
            swapped = (w["packed"] >> 4) | ((w["packed"] & 0xF) << 4)
            mutants = {
                "k-step dropped": xd.double() @ wdeq.double(),
                "absmax block shifted": x.double() @ nf4_ref.dequantize(w["packed"], shifted).double(),
                "nibbles swapped": x.double() @ nf4_ref.dequantize(swapped, w["absmax"]).double(),
            }
            for name, mut in mutants.items():
                out = mut.to(torch.bfloat16).double()
                worst[name] = max(worst[name], ((out - ref).abs() / bound).max().item())
    for name, ratio in worst.items():
        assert ratio >= 2.0, f"mutant '{name}' stays within {ratio:.2f}x of the bound"
