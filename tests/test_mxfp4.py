"""MXFP4 weights (ops/mxfp4.py, ops/csrc/mxfp4.hip, the MXFP4 mode of
ops/csrc/gemm_quant.hip, _FastWeight quant="mxfp4").

CPU tests pin the format: the reference quantizer's ties, saturation and
scale choice, the checkpoint-layout import, the plumbing, and a self-check
that the float64 bounds used on the GPU reject three corrupted references.

GPU tests: the quantize/dequantize kernels bit for bit against the reference;
one-hot inputs through the GEMV and the GEMM, which reproduce weight rows bit
for bit (nibble order, scale indexing, split-K chunking, lane liveness);
random data against float64 with bounds that come from the arithmetic:

* GEMV, fp32 accumulation of `in` terms over S splits:
  `|out - ref| <= in * 2^-23 * (|x| @ |W|)` (the (n + S) u bound, doubled);
* GEMM, the same accumulation then one bf16 rounding:
  `2^-8 |ref| + in * 2^-23 * (|X| @ |W|)` (test_prefill_gemm._bound).

MXFP4 values times power-of-two scales are exact in bf16 and fp32, so the
dequantized weight carries no error of its own.

Four values of the format overflow bf16: at s = 254 the magnitudes 2, 3, 4
and 6 (2^128 and up) exceed its range, so the round-trip test decodes into
float64, which holds every (code, scale) pair."""

import functools

import pytest
import torch

from petals_amd.ops import mxfp4 as mx

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPI_RAW, EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU = -1, 0, 2, 3
LEVELS = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]

# (in, out): one block x one lane; two blocks x 8 lanes; 7 k-blocks with a
# second wave of one live lane (520 = 512 + 8); 32 k-blocks x 4 waves
GEMV_SHAPES = [(32, 8), (64, 64), (224, 520), (1024, 2048)]
GEMV_SPLITS = [0, 1, 2, 5]
GEMV_BATCHES = [1, 3, 5, 8]  # 5 and 8 run the shallower-unroll instantiations

TILE = 128
GEMM_M = (1, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 44)
GEMM_OUT = (64, TILE + 64, 3 * TILE)
GEMM_IN = (64, 192, 512, 576)
M_MAX = max(GEMM_M)


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared fixtures


@functools.lru_cache(maxsize=None)
def _weights(in_dim: int, out_dim: int):
    """Random W (scale ~0.05) whose every (32-row block, column) is multiplied
    by a random power of two in [2^-3, 2^3], so a wrong scale index cannot
    hide; quantized once on the CPU by the reference."""
    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    w = torch.randn(in_dim, out_dim, generator=g) * 0.05
    pw = torch.randint(-3, 4, (in_dim // 32, out_dim), generator=g).float()
    w = (w * torch.exp2(pw).repeat_interleave(32, dim=0)).to(torch.bfloat16)
    packed, scales = mx.quantize(w)
    bias = (torch.randn(out_dim, generator=g) * 0.5).to(torch.bfloat16)
    return dict(w=w, packed=packed, scales=scales, bias=bias, deq=mx.dequantize(packed, scales))


@functools.lru_cache(maxsize=None)
def _x_gemm_random(in_dim: int):
    g = torch.Generator().manual_seed(77 + in_dim)
    return torch.randn(M_MAX, in_dim, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _x_gemm_onehot(in_dim: int):
    g = torch.Generator().manual_seed(5 + in_dim)
    perm = torch.cat([torch.randperm(in_dim, generator=g) for _ in range(-(-M_MAX // in_dim))])[:M_MAX]
    x = torch.zeros(M_MAX, in_dim, dtype=torch.bfloat16)
    x[torch.arange(M_MAX), perm] = 1.0
    return x, perm


@functools.lru_cache(maxsize=None)
def _x_gemv_random(in_dim: int):
    g = torch.Generator().manual_seed(31 + in_dim)
    return torch.randn(8, in_dim, generator=g)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def _gemm_bound(ref, x, wdeq):
    """test_prefill_gemm._bound: one bf16 rounding of the result plus twice
    the worst-case fp32 summation error over `in` terms."""
    return 2.0 ** -8 * ref.abs() + x.shape[1] * 2.0 ** -23 * (x.double().abs() @ wdeq.double().abs())


def _gemv_bound(x, wdeq):
    return x.shape[1] * 2.0 ** -23 * (x.double().abs() @ wdeq.double().abs())


def _decode_ocp(blocks: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Direct float64 decode of the checkpoint layout, element by element of
    the definition: W[out, k], k = 32 * block + 2 * byte + (0 low | 1 high)."""
    out_dim, nblk, _ = blocks.shape
    lv = torch.tensor(LEVELS, dtype=torch.float64)
    w = torch.empty(out_dim, nblk * 32, dtype=torch.float64)
    for half, nib in ((0, blocks & 0xF), (1, blocks >> 4)):
        mag = lv[(nib & 7).long()] * torch.where((nib & 8) != 0, -1.0, 1.0).double()
        val = mag * torch.exp2(scales.double() - 127.0)[:, :, None]  # [out, nblk, 16]
        w[:, half::2] = val.reshape(out_dim, nblk * 16)
    return w


# --------------------------------------------------------- CPU: the reference


def _column(vals):
    """One 32-row block in column 0 of a [32, 8] weight, the rest zero."""
    w = torch.zeros(32, 8)
    w[: len(vals), 0] = torch.tensor(vals)
    return w


def _codes_of(packed):
    nib = torch.empty(packed.shape[0] * 2, packed.shape[1], dtype=torch.uint8)
    nib[0::2], nib[1::2] = packed & 0xF, packed >> 4
    return nib


def test_reference_ties_saturation_and_zero_block():
    # amax 6 -> e = 0: every midpoint between neighbouring levels is a tie
    p, s = mx.quantize(_column([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]))
    assert s[0, 0].item() == 127
    assert _codes_of(p)[:8, 0].tolist() == [7, 0, 2, 2, 4, 4, 6, 6], "ties go to the even code"
    p, s = mx.quantize(_column([-6.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0]))
    assert _codes_of(p)[:8, 0].tolist() == [15, 0, 10, 10, 12, 12, 14, 14], "a rounded-to-zero value has no sign"
    # amax 7.5: floor(log2) = 2 -> e = 0; 7.5 saturates to 6
    p, s = mx.quantize(_column([7.5, -7.9, 1.0]))
    assert s[0, 0].item() == 127 and _codes_of(p)[:3, 0].tolist() == [7, 15, 2]
    assert mx.dequantize(p, s)[:3, 0].tolist() == [6.0, -6.0, 1.0]
    # the other columns are zero blocks
    assert (s[0, 1:] == 127).all() and (p[:, 1:] == 0).all()
    # scale choice at the binade edges: amax in [4, 8) -> e = 0, [8, 16) -> e = 1
    for amax, want_s in ((4.0, 127), (7.99, 127), (8.0, 128), (3.99, 126), (2.0 ** -20, 127 - 22)):
        assert mx.quantize(_column([amax]))[1][0, 0].item() == want_s, amax


@pytest.mark.parametrize("s", [1, 120, 127, 134, 254])
def test_reference_round_trip_every_code(s):
    """Every code but negative zero, in a block that also holds +-6, survives
    dequantize -> quantize at the smallest, the largest and three ordinary
    scales. float64 carries the values: 2, 3, 4 and 6 at s = 254 overflow bf16."""
    nib = torch.zeros(32, 8, dtype=torch.uint8)
    codes = [c for c in range(16) if c != 8]
    nib[: len(codes), 0] = torch.tensor(codes, dtype=torch.uint8)
    nib[15:17, 0] = torch.tensor([7, 15], dtype=torch.uint8)
    nib[:, 1] = nib[:, 0].flip(0)  # the same codes on the other nibble parity
    nib[0, 2:] = 7  # amax of every column is 6 * scale
    nib[1:16, 2:] = torch.tensor(codes, dtype=torch.uint8)[:, None]
    packed = nib[0::2] | (nib[1::2] << 4)
    scales = torch.full((1, 8), s, dtype=torch.uint8)
    w = mx.dequantize(packed, scales, dtype=torch.float64)
    assert torch.isfinite(w).all()
    p2, s2 = mx.quantize(w)
    assert torch.equal(s2, scales) and torch.equal(p2, packed)
    if s != 254:  # everything below the overflow is exact in bf16 as well
        wb = mx.dequantize(packed, scales)
        assert wb.dtype == torch.bfloat16 and torch.equal(wb.double(), w)
        p3, s3 = mx.quantize(wb)
        assert torch.equal(s3, scales) and torch.equal(p3, packed)


def test_reference_commutes_with_column_permutation_and_concat():
    w = _weights(64, 64)["w"]
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    p, s = mx.quantize(w)
    pp, sp = mx.quantize(w[:, perm].contiguous())
    assert torch.equal(pp, p[:, perm]) and torch.equal(sp, s[:, perm])
    pc, sc = mx.quantize(torch.cat([w, w[:, :8]], dim=1))
    assert torch.equal(pc, torch.cat([p, p[:, :8]], 1)) and torch.equal(sc, torch.cat([s, s[:, :8]], 1))


def test_from_ocp_blocks_matches_direct_decode():
    g = torch.Generator().manual_seed(3)
    out_dim, nblk = 24, 3
    blocks = torch.randint(0, 256, (out_dim, nblk, 16), generator=g).to(torch.uint8)
    scales = torch.randint(100, 150, (out_dim, nblk), generator=g).to(torch.uint8)
    scales[0, 0], scales[1, 1] = 1, 250  # the ends of the accepted range (250: still finite in bf16)
    packed, sc = mx.from_ocp_blocks(blocks, scales)
    assert packed.shape == (nblk * 16, out_dim) and sc.shape == (nblk, out_dim)
    assert packed.is_contiguous() and sc.is_contiguous()
    want = _decode_ocp(blocks, scales).t()  # [in, out]
    assert torch.equal(mx.dequantize(packed, sc, dtype=torch.float64), want)
    assert torch.equal(mx.dequantize(packed, sc).double(), want), "exact in bf16"
    for bad in (0, 255):
        s_bad = scales.clone()
        s_bad[5, 2] = bad
        with pytest.raises(ValueError):
            mx.from_ocp_blocks(blocks, s_bad)
    with pytest.raises(ValueError):  # out % 8 != 0
        mx.from_ocp_blocks(blocks[:12 + 1], scales[:12 + 1])


def test_float64_bounds_reject_corrupted_references():
    """Both bounds are tight enough to matter: each corrupted reference (the
    scale of the neighbouring column, the scale of the neighbouring 32-row
    block, rows 2j and 2j+1 swapped) breaks each bound by >= 2x on at least
    one case, while the honest result stays inside."""
    names = ("scale of the next column", "scale of the next block", "rows 2j / 2j+1 swapped")
    worst = {(kind, n): 0.0 for kind in ("gemm", "gemv") for n in names}
    for in_dim in GEMM_IN:
        for out_dim in GEMM_OUT:
            w = _weights(in_dim, out_dim)
            p, s = w["packed"], w["scales"]
            mutants = {
                names[0]: mx.dequantize(p, s.roll(-1, dims=1)),
                names[1]: mx.dequantize(p, s.roll(-1, dims=0)),  # no-op at in = 32: one block
                names[2]: mx.dequantize((p >> 4) | ((p & 0xF) << 4), s),
            }
            wdeq = w["deq"].double()
            xg = _x_gemm_random(in_dim)[: TILE + 1]
            ref = xg.double() @ wdeq
            bound = _gemm_bound(ref, xg, wdeq).clamp_min(1e-300)
            assert ((ref.to(torch.bfloat16).double() - ref).abs() <= bound).all()
            xv = _x_gemv_random(in_dim)
            refv = xv.double() @ wdeq
            boundv = _gemv_bound(xv, wdeq).clamp_min(1e-300)
            assert (((xv @ wdeq.float()).double() - refv).abs() <= boundv).all()
            for n, m in mutants.items():
                out = (xg.double() @ m.double()).to(torch.bfloat16).double()
                worst[("gemm", n)] = max(worst[("gemm", n)], ((out - ref).abs() / bound).max().item())
                outv = xv.double() @ m.double()
                worst[("gemv", n)] = max(worst[("gemv", n)], ((outv - refv).abs() / boundv).max().item())
    for key, ratio in worst.items():
        assert ratio >= 2.0, f"mutant {key} stays within {ratio:.2f}x of the bound"


# ------------------------------------------------------------- CPU: plumbing


def test_fastweight_cpu_shapes_and_dense():
    from petals_amd.ops.fused_decode import _FastWeight

    w = _weights(64, 64)
    fw = _FastWeight(w["w"], None, "mxfp4")
    assert fw.shape == (64, 64)
    assert torch.equal(fw.mx_packed, w["packed"]) and torch.equal(fw.mx_scales, w["scales"])
    assert torch.equal(_bits(fw.dense()), _bits(w["deq"]))
    x = _x_gemm_random(64)[:6].reshape(2, 3, 64)
    assert torch.equal(fw.matmul(x, w["bias"]), torch.matmul(x, w["deq"]) + w["bias"])
    for shape in ((48, 64), (64, 12), (31, 8)):
        with pytest.raises(ValueError, match=rf"\[{shape[0]}, {shape[1]}\]"):
            _FastWeight(torch.zeros(shape, dtype=torch.bfloat16), None, "mxfp4")


def test_fused_gemm_eligible_mxfp4():
    from petals_amd.ops.fused_decode import FUSED_GEMM_MAX_ROWS, fused_gemm_eligible

    rows = FUSED_GEMM_MAX_ROWS["mxfp4"]
    assert rows >= 1
    assert fused_gemm_eligible("mxfp4", 1, 64, 64)
    assert fused_gemm_eligible("mxfp4", rows, 8192, 57344)
    assert not fused_gemm_eligible("mxfp4", rows + 1, 8192, 57344)
    assert not fused_gemm_eligible("mxfp4", 0, 64, 64)
    assert not fused_gemm_eligible("mxfp4", 16, 96, 128)  # the GEMM's k step is 64, not the 32-row block
    assert not fused_gemm_eligible("mxfp4", 16, 128, 104)  # out % 8 == 0 serves the gemv only


def test_block_param_bytes_and_cli(monkeypatch):
    import petals_amd.cli.run_server as rs
    from petals_amd.server.server import Server

    srv = Server("test-llama", device="cpu", num_blocks=1, quant_type="mxfp4")
    assert srv.quant_type == "mxfp4"
    cfg = srv.config
    h, inter, kv = cfg.hidden_size, cfg.intermediate_size, cfg.n_kv_heads * cfg.head_dim
    params = 2 * h * h + 2 * h * kv + 3 * h * inter
    assert srv._block_param_bytes() == int(params * 0.53125)  # 4 bits + 8 bits per 32 params

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
    rs.main(["test-llama", "--quant_type", "mxfp4"])
    assert captured["quant_type"] == "mxfp4"
    with pytest.raises(SystemExit):
        rs.main(["test-llama", "--quant_type", "fp4"])


def test_mixtral_mxfp4_not_implemented():
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config

    blk = get_model_block(load_model_config("test-mixtral"), 0)
    with pytest.raises(NotImplementedError, match="MXFP4"):
        blk.optimize_for_inference(quant="mxfp4")


# ----------------------------------------- GPU: quantize / dequantize kernels


def _planted(in_dim: int, out_dim: int) -> torch.Tensor:
    """_weights plus planted blocks: exact ties, a saturating block, a zero
    block, and the bf16 extremes (largest finite, smallest normal, subnormals)."""
    w = _weights(in_dim, out_dim)["w"].clone()
    w[:8, 0] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]).to(torch.bfloat16)
    w[8:32, 0] = 0
    w[:8, 1] = -w[:8, 0] * 2.0 ** -9
    w[8:32, 1] = 0
    w[:32, 2] = 0
    w[:3, 2] = torch.tensor([7.5, -7.75, 1.0]).to(torch.bfloat16)
    w[:32, 3] = 0
    big = torch.finfo(torch.bfloat16).max
    w[:32, 4] = 0
    w[:4, 4] = torch.tensor([big, -big, big / 2, big / 64]).to(torch.bfloat16)
    w[:32, 5] = 0
    w[:4, 5] = torch.tensor([2.0 ** -126, -(2.0 ** -127), 2.0 ** -128, 2.0 ** -133]).to(torch.bfloat16)
    w[:32, 6] = 0
    w[:3, 6] = torch.tensor([2.0 ** -127, 2.0 ** -129, -(2.0 ** -133)]).to(torch.bfloat16)  # subnormal amax
    w[:32, 7] = 0
    w[:2, 7] = torch.tensor([big, 2.0 ** -133]).to(torch.bfloat16)
    return w


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", [(32, 8), (64, 520), (4544, 64)])
def test_quantize_dequantize_kernels_bit_identical(hip, in_dim, out_dim):
    w = _planted(in_dim, out_dim)
    p_ref, s_ref = mx.quantize(w)
    p, s = hip.mxfp4_quantize(w.cuda())
    assert p.dtype == torch.uint8 and p.shape == p_ref.shape and s.shape == s_ref.shape
    assert torch.equal(s.cpu(), s_ref), (s.cpu() != s_ref).nonzero()[:4]
    assert torch.equal(p.cpu(), p_ref), (p.cpu() != p_ref).nonzero()[:4]
    d = hip.mxfp4_dequantize(p, s)
    assert d.dtype == torch.bfloat16 and d.shape == (in_dim, out_dim)
    assert torch.equal(_bits(d.cpu()), _bits(mx.dequantize(p_ref, s_ref)))


@requires_gpu
@pytest.mark.gpu
def test_dequantize_kernel_every_code_and_scale_edge(hip):
    """All 16 nibbles on both parities at s = 1 (the bf16 subnormal 2^-127),
    ordinary scales, and 252..254 (the overflow to infinity of the reference)."""
    g = torch.Generator().manual_seed(9)
    packed = torch.randint(0, 256, (32, 16), generator=g).to(torch.uint8)
    packed[:16, 0] = torch.arange(16, dtype=torch.uint8) * 17  # every nibble, both halves
    scales = torch.tensor([[1, 1, 2, 100, 127, 134, 200, 250, 251, 252, 252, 253, 253, 254, 254, 127],
                           [254, 1, 127, 127, 126, 128, 3, 252, 253, 254, 1, 2, 3, 4, 5, 6]], dtype=torch.uint8)
    packed[16:, 0] = packed[:16, 0]
    want = mx.dequantize(packed, scales)
    got = hip.mxfp4_dequantize(packed.cuda(), scales.cuda()).cpu()
    assert torch.equal(_bits(got), _bits(want)), (_bits(got) != _bits(want)).nonzero()[:4]


# ------------------------------------------------------------------ GPU: gemv


def _gemv(hip, w_gpu, x, epi, splits, ws=None, residual=None, bias=None):
    """One gemv_mxfp4 call on a NaN-filled workspace of the fast paths' size."""
    out_dim = w_gpu[0].shape[1]
    if ws is None:
        ws = torch.empty(64 * x.shape[0] * out_dim, device="cuda")
    ws.fill_(float("nan"))
    return hip.gemv_mxfp4(w_gpu[0], w_gpu[1], x, ws, residual, epi, splits, bias)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMV_SHAPES)
def test_gemv_one_hot_exact(hip, in_dim, out_dim):
    """x = 1.5 e_i per batch row: the output row is 1.5 W[i, :] bit for bit
    (one nonzero product per column, exact in fp32; every other term is a
    signed zero). Pins the nibble order of the hardware conversion, the scale
    byte per column and block, the split chunking and the live-lane test."""
    w = _weights(in_dim, out_dim)
    w_gpu = (w["packed"].cuda(), w["scales"].cuda())
    deq = w["deq"].float()
    g = torch.Generator().manual_seed(in_dim + out_dim)
    n_call = 0
    for splits in GEMV_SPLITS:
        for B in GEMV_BATCHES:
            # first and last row, an odd and an even row, then random ones
            idx = torch.cat([torch.tensor([0, in_dim - 1, 1, in_dim - 2]),
                             torch.randint(0, in_dim, (4,), generator=g)])
            idx = idx.roll(n_call)[:B]  # B = 1 still visits more than row 0
            n_call += 1
            x = torch.zeros(B, in_dim)
            x[torch.arange(B), idx] = 1.5
            want = 1.5 * deq[idx]
            n_splits = hip.gemv_mxfp4_splits(in_dim, out_dim, B, splits)
            assert 1 <= n_splits <= in_dim // 32
            if splits > 0:
                assert n_splits <= splits
            out = _gemv(hip, w_gpu, x.cuda(), EPI_PLAIN, splits)
            assert out.shape == (B, out_dim) and out.dtype == torch.float32
            assert torch.equal(out.cpu(), want), (splits, B, (out.cpu() != want).nonzero()[:4])
            raw = _gemv(hip, w_gpu, x.cuda(), EPI_RAW, splits)
            assert raw.shape == (n_splits, B, out_dim)
            assert torch.equal(raw.sum(0).cpu(), want), (splits, B)


def _silu(t):
    return t / (1.0 + torch.exp(-t))


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", [(224, 520), (1024, 2048)])
def test_gemv_random_vs_float64(hip, in_dim, out_dim):
    """Random x against float64. Plain output: the GEMV bound. The epilogue
    cases add what their own arithmetic adds: +bias is one more fp32 rounding
    (2^-23 |ref|, doubled like the rest); the residual epilogue rounds
    residual + sum to bf16 once (2^-8 |ref|); SwiGLU propagates the gate and
    up bounds bg, bu through silu (|silu'| <= 1.1) and adds 2^-17 |ref| for
    the fast exponential and the three fp32 operations after it."""
    w = _weights(in_dim, out_dim)
    w_gpu = (w["packed"].cuda(), w["scales"].cuda())
    wdeq = w["deq"].double()
    x_all = _x_gemv_random(in_dim)
    g = torch.Generator().manual_seed(2)
    res_all = torch.randn(8, out_dim, generator=g).to(torch.bfloat16)
    half = out_dim // 2
    ws_shared = torch.empty(64 * 8 * out_dim, device="cuda")
    for B in GEMV_BATCHES:
        x = x_all[:B]
        ref = x.double() @ wdeq
        bnd = _gemv_bound(x, wdeq)
        refb = ref + w["bias"].double()
        gt, up = refb[:, :half], refb[:, half:]
        bg, bu = bnd[:, :half] + 2.0 ** -23 * gt.abs(), bnd[:, half:] + 2.0 ** -23 * up.abs()
        ref_sw = _silu(gt) * up
        cases = {
            "plain": (EPI_PLAIN, None, None, ref, bnd),
            "bias": (EPI_PLAIN, None, w["bias"].cuda(), refb, bnd + 2.0 ** -23 * refb.abs()),
            "residual": (EPI_RESIDUAL, res_all[:B].cuda(), None, ref + res_all[:B].double(),
                         bnd + 2.0 ** -8 * (ref + res_all[:B].double()).abs()),
            "swiglu": (EPI_SWIGLU, None, w["bias"].cuda(), ref_sw,
                       1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * ref_sw.abs()),
        }
        for splits in (0, 3):
            for name, (epi, res, bias, want, bound) in cases.items():
                out = _gemv(hip, w_gpu, x.cuda(), epi, splits, ws_shared, res, bias).clone()
                assert not bool(torch.isnan(ws_shared[0])), "the partials must land in the caller's workspace"
                again = _gemv(hip, w_gpu, x.cuda(), epi, splits, ws_shared, res, bias)
                assert torch.equal(out, again), f"{name} B={B} splits={splits}: two runs differ"
                out = out.cpu().double()
                assert out.shape == want.shape and torch.isfinite(out).all()
                err = (out - want).abs()
                ratio = (err / bound.clamp_min(1e-300)).max().item()
                print(f"gemv {in_dim}x{out_dim} B={B} splits={splits} {name}: max err/bound = {ratio:.3f}")
                assert (err <= bound).all(), f"{name} B={B} splits={splits}: max err/bound = {ratio:.3f}"


@requires_gpu
@pytest.mark.gpu
def test_gemv_rejects_bad_operands(hip):
    w = _weights(64, 64)
    p, s = w["packed"].cuda(), w["scales"].cuda()
    ws = torch.empty(64 * 64, device="cuda")
    x = torch.randn(2, 64, device="cuda")
    with pytest.raises(RuntimeError):  # batch > 8
        hip.gemv_mxfp4(p, s, torch.randn(9, 64, device="cuda"), ws, None, EPI_PLAIN, 0, None)
    with pytest.raises(RuntimeError):  # bf16 x
        hip.gemv_mxfp4(p, s, x.bfloat16(), ws, None, EPI_PLAIN, 0, None)
    with pytest.raises(RuntimeError):  # in mismatch
        hip.gemv_mxfp4(p, s, x[:, :32].contiguous(), ws, None, EPI_PLAIN, 0, None)
    with pytest.raises(RuntimeError):  # scales of another weight
        hip.gemv_mxfp4(p, s[:1].contiguous(), x, ws, None, EPI_PLAIN, 0, None)
    with pytest.raises(RuntimeError):  # out % 8 != 0
        hip.gemv_mxfp4(p[:, :12].contiguous(), s[:, :12].contiguous(), x, ws, None, EPI_PLAIN, 0, None)
    with pytest.raises(RuntimeError):  # in % 32 != 0
        hip.mxfp4_quantize(torch.zeros(48, 64, device="cuda", dtype=torch.bfloat16))


# ------------------------------------------------------------------ GPU: gemm


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim", GEMM_IN)
@pytest.mark.parametrize("out_dim", GEMM_OUT)
def test_gemm_one_hot_exact(hip, out_dim, in_dim):
    """Row m of the output is row perm(m) of mxfp4.dequantize, bit for bit."""
    w = _weights(in_dim, out_dim)
    x, perm = _x_gemm_onehot(in_dim)
    p, s = w["packed"].cuda(), w["scales"].cuda()
    rows = w["deq"]
    assert (rows.float().abs() >= 2.0 ** -126).logical_or(rows == 0).all(), "nothing subnormal"
    for m in GEMM_M:
        out = hip.gemm_mxfp4(p, s, x[:m].cuda(), None)
        assert out.shape == (m, out_dim) and out.dtype == torch.bfloat16
        again = hip.gemm_mxfp4(p, s, x[:m].cuda(), None)
        out, again = out.cpu(), again.cpu()
        assert torch.equal(_bits(out), _bits(again)), f"M={m}: two runs differ"
        bad = (_bits(out) != _bits(rows[perm[:m]])).nonzero()
        assert bad.numel() == 0, f"M={m}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("in_dim", GEMM_IN)
@pytest.mark.parametrize("out_dim", GEMM_OUT)
def test_gemm_random_vs_float64(hip, out_dim, in_dim, with_bias):
    w = _weights(in_dim, out_dim)
    x = _x_gemm_random(in_dim)
    p, s = w["packed"].cuda(), w["scales"].cuda()
    wdeq = w["deq"]
    ref_all = x.double() @ wdeq.double()
    if with_bias:
        ref_all = ref_all + w["bias"].double()
    bound_all = _gemm_bound(ref_all, x, wdeq)
    bias_gpu = w["bias"].cuda() if with_bias else None
    for m in GEMM_M:
        out = hip.gemm_mxfp4(p, s, x[:m].cuda(), bias_gpu)
        again = hip.gemm_mxfp4(p, s, x[:m].cuda(), bias_gpu)
        out, again = out.cpu(), again.cpu()
        assert torch.equal(_bits(out), _bits(again)), f"M={m}: two runs differ"
        err = (out.double() - ref_all[:m]).abs()
        ratio = (err / bound_all[:m].clamp_min(1e-300)).max().item()
        print(f"gemm in={in_dim} out={out_dim} M={m} bias={with_bias}: max err/bound = {ratio:.3f}")
        assert (err <= bound_all[:m]).all(), f"M={m}: max err/bound = {ratio:.3f}"


@requires_gpu
@pytest.mark.gpu
def test_gemm_rejects_bad_operands(hip):
    w = _weights(64, 64)
    p, s = w["packed"].cuda(), w["scales"].cuda()
    x = _x_gemm_random(64)[:4].cuda()
    with pytest.raises(RuntimeError):  # fp32 x
        hip.gemm_mxfp4(p, s, x.float(), None)
    with pytest.raises(RuntimeError):  # in % 64 != 0
        hip.gemm_mxfp4(p[:16].contiguous(), s[:1].contiguous(), x[:, :32].contiguous(), None)
    with pytest.raises(RuntimeError):  # bias of the wrong length
        hip.gemm_mxfp4(p, s, x, w["bias"][:32].contiguous().cuda())
    with pytest.raises(RuntimeError):  # scales of another shape
        hip.gemm_mxfp4(p, s[:1].contiguous(), x, None)


# ---------------------------------------------------------------- GPU: blocks


def _round_trip_linears_(block) -> None:
    """Every nn.Linear weight [out, in] -> bf16 -> MXFP4 along `in` -> back, so
    the CPU block computes with the very values the GPU block dequantizes."""
    with torch.no_grad():
        for mod in block.modules():
            if isinstance(mod, torch.nn.Linear):
                wt = mod.weight.detach().to(torch.bfloat16).t().contiguous()  # [in, out]
                mod.weight.copy_(mx.dequantize(*mx.quantize(wt)).t().to(mod.weight.dtype))


def _block_pair(preset):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk_cpu = get_model_block(cfg, 0)
    init_random_block_(blk_cpu, cfg, 0)
    blk_cpu = blk_cpu.float().eval()
    blk_gpu = get_model_block(cfg, 0)
    blk_gpu.load_state_dict(blk_cpu.state_dict())
    blk_gpu = blk_gpu.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="mxfp4")
    assert blk_gpu._fast is not None and blk_gpu._fast.quant == "mxfp4", f"{preset} must take the fused path"
    _round_trip_linears_(blk_cpu)
    return cfg, blk_cpu, blk_gpu


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["test-llama-hd128", "test-bloom-hd64", "test-falcon-hd64"])
def test_block_mxfp4_matches_round_tripped_cpu(hip, monkeypatch, preset):
    """B = 2, a 6-token prefill then 3 decode steps against the fp32 CPU block
    holding the round-tripped weights (tolerance of the bf16 block tests);
    then the same prefill in dense and fused mode."""
    from petals_amd.ops import fused_decode

    monkeypatch.delenv("PETALS_AMD_PREFILL_GEMM", raising=False)
    cfg, blk_cpu, blk_gpu = _block_pair(preset)
    torch.manual_seed(5)
    B, S = 2, 9
    x = torch.randn(B, S, cfg.hidden_size) * 0.5
    ks, vs = blk_cpu.kv_cache_shape(B, 32)
    kc, vc = torch.zeros(ks), torch.zeros(vs)
    kg = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
    vg = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
    with torch.inference_mode():
        y_cpu = [blk_cpu(x[:, :6], kv_cache=(kc, vc), prefix_length=0)]
        y_gpu = [blk_gpu(x[:, :6].cuda().bfloat16(), kv_cache=(kg, vg), prefix_length=0)]
        for t in range(6, S):
            y_cpu.append(blk_cpu(x[:, t : t + 1], kv_cache=(kc, vc), prefix_length=t))
            y_gpu.append(blk_gpu(x[:, t : t + 1].cuda().bfloat16(), kv_cache=(kg, vg), prefix_length=t))
    ref = torch.cat(y_cpu, 1)
    out = torch.cat([y.float().cpu() for y in y_gpu], 1)
    print(f"{preset}: max |gpu - cpu| = {(out - ref).abs().max().item():.4f}")
    assert torch.allclose(out, ref, atol=0.05, rtol=0.05), (out - ref).abs().max()

    results = {}
    for mode in ("dense", "fused"):
        monkeypatch.setenv("PETALS_AMD_PREFILL_GEMM", mode)
        fused_decode._dequant_cache = None  # a fresh process-wide cache
        fused_decode._dequant_cache_bytes = 0
        k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
        with torch.inference_mode():
            y = blk_gpu(x[:, :6].cuda().bfloat16(), kv_cache=(k, v), prefix_length=0)
        results[mode] = (y.float().cpu(), k.float().cpu(), fused_decode._dequant_cache_bytes)
    fused_decode._dequant_cache = None
    fused_decode._dequant_cache_bytes = 0
    (yd, kd, bytes_dense), (yf, kf, bytes_fused) = results["dense"], results["fused"]
    assert bytes_dense > 0, "dense mode dequantizes through the LRU"
    assert bytes_fused == 0, "fused mode must leave the dequant LRU empty"
    assert torch.isfinite(yf).all()
    assert torch.allclose(yf, yd, atol=2e-2, rtol=2e-2), (yf - yd).abs().max()
    assert kd.abs().sum() > 0 and torch.allclose(kf, kd, atol=2e-2, rtol=2e-2)


# ------------------------------------------------- GPU: workspace, graph, serve


@requires_gpu
@pytest.mark.gpu
def test_decode_workspace_holds_partials(hip):
    """At every decode batch 1..8 the workspace the fast path sizes
    (64 * B * _max_gemv_out floats) is the buffer each of the block's gemvs
    writes its partials into, with the split count the weight was tuned to;
    a too-small workspace would leave the NaN sentinel. A decode step leaves
    the shared workspace where it was."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops.fused_decode import _get_ws
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config("test-llama-hd128")
    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    blk = blk.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="mxfp4")
    fp = blk._fast
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cuda").manual_seed(3)
    weights = {"qkv": fp.wqkv_t, "o": fp.wo_t, "gate|up": fp.wgateup_t, "down": fp.wdown_t}
    with torch.inference_mode():
        for B in range(1, 9):
            numel = 64 * B * fp._max_gemv_out()
            for name, fw in weights.items():
                assert fw.quant == "mxfp4" and 0 <= fw.splits <= 64
                n_splits = hip.gemv_mxfp4_splits(fw.in_dim, fw.out_dim, B, fw.splits)
                assert n_splits * B * fw.out_dim <= numel, f"B={B} {name}: {n_splits} splits overflow the workspace"
                ws = torch.full((numel,), float("nan"), device="cuda")
                x = torch.randn(B, fw.in_dim, device="cuda", generator=g)
                y = fw.gemv(x, ws, None, EPI_PLAIN)
                assert not bool(torch.isnan(ws[0])), f"B={B} {name}: partials did not land in the workspace"
                assert bool(torch.isfinite(ws[: n_splits * B * fw.out_dim]).all())
                assert y.shape == (B, fw.out_dim) and bool(torch.isfinite(y).all())
            before = _get_ws(dev, "gemv", numel).data_ptr()
            ks, vs = blk.kv_cache_shape(B, 16)
            kv = (torch.zeros(ks, device="cuda", dtype=torch.bfloat16),
                  torch.zeros(vs, device="cuda", dtype=torch.bfloat16))
            h = torch.randn(B, 1, cfg.hidden_size, device="cuda", generator=g).to(torch.bfloat16)
            out = blk(h, kv_cache=kv, prefix_length=0)
            assert bool(torch.isfinite(out.float()).all())
            assert _get_ws(dev, "gemv", numel).data_ptr() == before, f"B={B}: workspace moved"


@requires_gpu
@pytest.mark.gpu
def test_decode_graph_capture_matches_eager(hip):
    """One captured decode step replayed over new tokens equals the eager
    fused path of a second block with the same weights."""
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.server.from_pretrained import init_random_block_
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config("test-llama-hd128")
    blks = []
    for _ in range(2):
        b = get_model_block(cfg, 0)
        init_random_block_(b, cfg, 0)
        blks.append(b.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="mxfp4"))
    blk, blk2 = blks
    assert blk._fast is not None and blk._fast.graph_safe

    torch.manual_seed(7)
    B = 2
    ks, vs = blk.kv_cache_shape(B, 16)
    kg = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
    vg = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
    kg2, vg2 = kg.clone(), vg.clone()
    xs = [torch.randn(B, 1, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5 for _ in range(4)]
    ctx = DecodeContext(torch.device("cuda"))
    ctx.set_position(0)
    h_in = torch.empty_like(xs[0])

    def step():
        return blk(h_in, kv_cache=(kg, vg), ctx=ctx)

    graph = GraphedCallable(step, [])
    for t, x in enumerate(xs):
        ctx.set_position(t)
        h_in.copy_(x)
        og = graph.replay().clone()
        oe = blk2(x, kv_cache=(kg2, vg2), prefix_length=t)
        assert torch.equal(_bits(og.cpu()), _bits(oe.cpu())), (t, (og.float() - oe.float()).abs().max())
    assert torch.equal(kg, kg2) and torch.equal(vg, vg2)


@requires_gpu
@pytest.mark.gpu
def test_llama_hd128_mxfp4_serving_uses_span_graph(monkeypatch):
    """One GPU server of MXFP4 blocks serving a client generate(): decode
    goes through the whole-span hipGraph."""
    from petals_amd.dht.node import DHT
    from petals_amd.server import handler
    from petals_amd.server.server import Server
    from petals_amd.utils.auto_config import AutoDistributedModelForCausalLM

    monkeypatch.delenv("PETALS_AMD_NO_GRAPHS", raising=False)
    calls = []
    real_step = handler._SpanDecodeGraph.step

    def counting_step(self, hidden_states, prefix_length):
        calls.append(prefix_length)
        return real_step(self, hidden_states, prefix_length)

    monkeypatch.setattr(handler._SpanDecodeGraph, "step", counting_step)

    preset, prefix = "test-llama-hd128", "gpu-mxfp4"
    boot = DHT(host="127.0.0.1")
    server = Server(
        preset, initial_peers=[boot.listen_addr], host="127.0.0.1", device="cuda",
        torch_dtype="bfloat16", block_indices="0:4", dht_prefix=prefix, throughput=1.0,
        quant_type="mxfp4",
    ).start()
    try:
        for backend in server.backends.values():
            assert backend.block._fast is not None and backend.block._fast.quant == "mxfp4"
        model = AutoDistributedModelForCausalLM.from_pretrained(
            preset, initial_peers=[boot.listen_addr], dht_prefix=prefix, show_route=False, max_retries=1,
        )
        torch.manual_seed(2)
        ids = torch.randint(0, 128, (1, 5))
        out = model.generate(ids, max_new_tokens=6, do_sample=False)
        assert out.shape == (1, 11)
        with model.transformer.h.inference_session(max_length=16) as sess:
            with model.transformer.h.use_session(sess):
                with torch.no_grad():
                    model(input_ids=ids)
                    logits = model(input_ids=out[:, 5:6]).logits
        assert logits.shape == (1, 1, 128) and bool(torch.isfinite(logits.float()).all())
        assert len(calls) >= 1, "the span decode graph was never stepped"
        model.transformer.h.sequence_manager.shutdown()
    finally:
        server.shutdown()
        boot.shutdown()
