"""Opt-in FP8 (OCP E4M3, `torch.float8_e4m3fn`) KV cache: the reference
quantizer (`petals_amd/ops/kv_fp8.py`), the cache accounting, the kernels that
read and write fp8 caches, the Llama / Mixtral fused blocks and a served span.

How the kernel checks are built. An fp8 cache holds values that are exactly
representable in bf16, and the fp8 instantiations convert them exactly before
the unchanged bf16 arithmetic. So

  (a) a kernel reading an fp8 cache must be BIT-IDENTICAL to the bf16 kernel
      reading `dequantize(cache, bf16)`, no tolerance;
  (b) against float64 attention over the dequantized K/V it must meet
      TOL_FP8_*, which is 4x the worst error of `emulated_attention_f64` on
      the round-tripped case tables (the rule and the factor of
      tests/test_attention_numerics.py), measured on the CPU below.

The tables are those of test_attention_numerics with K/V passed through
`quantize`; the needles are placed again ON the E4M3 grid (alpha raised until
they hold >= NEEDLE_MASS of their row), the poison past kv_len becomes needle
K rows, V = 448 and, in a second run, V = NaN (code 0x7F).
"""

import asyncio
import dataclasses
import functools
import math

import pytest
import torch

from petals_amd.ops import kv_fp8
from test_attention_numerics import (
    ALPHA0,
    DECODE_CASES,
    DECODE_MUTANTS,
    DECODE_PARAMS,
    NEEDLE_MASS,
    PREFILL_CASES,
    PREFILL_MUTANTS,
    PREFILL_PARAMS,
    WRITER_B,
    WRITER_KH,
    WRITER_PARAMS,
    WRITER_QH,
    _poison,
    _unit,
    _worst_rejection,
    decode_inputs,
    mfma_auto_splits,
    nerr,
    prefill_inputs,
    ref_attention_f64,
    ref_probs_f64,
    writer_inputs,
)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
FP8 = torch.float8_e4m3fn

# --------------------------------------------------------------- tolerances
#
# TOL_FP8_* = 4 x max over the round-tripped tables of nerr(emulated, ref),
# rounded up to 3 significant digits (`test_fp8_tolerance_constants_are_measured`
# recomputes the maxima, `test_fp8_emulated_error_within_quarter_tol` checks
# every case). Measured on the CPU, float64:
#
#   decode: all of DECODE_PARAMS and the cache-writer attention cases (131
#   inputs; test_fp8_emulated_error_within_quarter_tol prints each). The three
#   largest: D-hd64-gq29-...-kv333 needle1 0.00867, needle0 0.00863, pair 0.00863
#   worst 0.00867 -> x4, rounded up
TOL_FP8_DECODE = 0.0347
#   prefill, the three largest: b1-qh8-kvh8-s130-hd64-off70-causal-alibi diag
#   0.01148, b2-qh4-kvh2-s70-hd64-off0-full diag 0.01134,
#   b1-qh8-kvh2-s130-hd64-off70-causal diag 0.00986
#   worst 0.01148 -> x4, rounded up (the worst is above TOL_PREFILL / 4 =
#   0.0107, so the bf16 constant cannot be reused)
TOL_FP8_PREFILL = 0.0460


# ------------------------------------------------------- reference quantizer


def _q(vals):
    return kv_fp8.quantize(torch.tensor(vals, dtype=torch.float32)).to(torch.float32)


def test_quantize_rounds_to_nearest_even():
    assert _q([1.0625, 1.1875, -1.0625, -1.1875]).tolist() == [1.0, 1.25, -1.0, -1.25]
    # inside a binade: spacing 1/8 at [1, 2)
    assert _q([1.06, 1.07, 1.9]).tolist() == [1.0, 1.125, 1.875]


def test_quantize_small_values():
    assert _q([2.0**-10, -(2.0**-10), 2.0**-9, -(2.0**-9), 0.0]).tolist() == [0.0, -0.0, 2.0**-9, -(2.0**-9), 0.0]
    assert _q([1.5 * 2.0**-9]).tolist() == [2.0**-8]  # tie -> even subnormal code
    assert _q([1e-30]).tolist() == [0.0]


def test_quantize_saturates_and_keeps_nan():
    assert _q([448.0, -448.0]).tolist() == [448.0, -448.0]
    assert _q([464.0, 500.0, 1e4, -464.0, -500.0, -1e4]).tolist() == [448.0] * 3 + [-448.0] * 3
    # the bare torch cast is not the reference
    assert torch.isnan(torch.tensor([500.0]).to(FP8).float()).all()
    q = kv_fp8.quantize(torch.tensor([float("nan"), 1.0]))
    assert torch.isnan(q.float()[0]) and q.float()[1] == 1.0
    assert (q.view(torch.uint8)[0].item() & 0x7F) == 0x7F
    assert kv_fp8.quantize(torch.tensor([1e4], dtype=torch.bfloat16)).float().item() == 448.0


def test_all_finite_codes_round_trip_and_are_bf16_exact():
    codes = torch.arange(256, dtype=torch.uint8)
    vals = codes.view(FP8).to(torch.float32)
    finite = ~torch.isnan(vals)
    assert int(finite.sum()) == 254 and not torch.isinf(vals).any()
    assert torch.equal(kv_fp8.quantize(vals[finite]).view(torch.uint8), codes[finite])
    for dt in (torch.bfloat16, torch.float32):
        deq = kv_fp8.dequantize(codes.view(FP8), dt)
        assert torch.equal(deq[finite].to(torch.float64), vals[finite].to(torch.float64))
    assert vals[finite].abs().max() == 448.0 and vals[finite][vals[finite] > 0].min() == 2.0**-9


def test_spacing_matches_the_code_table():
    vals = torch.arange(128, dtype=torch.uint8).view(FP8).to(torch.float64)[:127]  # positive finite
    gaps = vals[1:] - vals[:-1]
    assert torch.equal(kv_fp8.spacing(vals[1:-1]), gaps[1:])  # gap above each value
    assert kv_fp8.spacing(torch.tensor([0.0, 1e-4])).tolist() == [2.0**-9] * 2


# ----------------------------------------------------------------- accounting


def _cpu_backend(preset="test-llama-hd128", cache_dtype=None):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.backend import TransformerBackend
    from petals_amd.server.memory_cache import MemoryCache

    cfg = load_model_config(preset)
    blk = get_model_block(cfg, 0)
    mc = MemoryCache(1 << 30, torch.device("cpu"))
    return TransformerBackend("u.0", blk, config=cfg, memory_cache=mc, dtype=torch.bfloat16, cache_dtype=cache_dtype)


def test_cache_bytes_per_token_halves():
    bf16, fp8 = _cpu_backend(), _cpu_backend(cache_dtype=FP8)
    assert bf16.cache_bytes_per_token() == 2 * fp8.cache_bytes_per_token() > 0
    assert bf16.cache_bytes_per_token(4) == 2 * fp8.cache_bytes_per_token(4)
    assert [d.dtype for d in fp8.get_inference_cache_descriptors(2, 16)] == [FP8, FP8]
    assert [d.dtype for d in bf16.get_inference_cache_descriptors(2, 16)] == [torch.bfloat16] * 2
    assert fp8.get_info()["kv_cache_dtype"] == "fp8" and bf16.get_info()["kv_cache_dtype"] == "bf16"


def test_cli_flag():
    from petals_amd.cli.run_server import build_parser

    p = build_parser()
    assert p.parse_args(["llama-2-70b"]).kv_cache_dtype == "bf16"
    assert p.parse_args(["llama-2-70b", "--kv_cache_dtype", "fp8"]).kv_cache_dtype == "fp8"
    with pytest.raises(SystemExit):
        p.parse_args(["llama-2-70b", "--kv_cache_dtype", "fp4"])


def test_server_rejects_unsupported_fp8_setups(monkeypatch):
    from petals_amd.server.server import Server

    kw = dict(initial_peers=[], block_indices="0:1", throughput=1.0)
    with pytest.raises(ValueError, match="GPU"):
        Server("test-llama-hd128", device="cpu", kv_cache_dtype="fp8", **kw)
    with pytest.raises(ValueError, match="expected one of"):
        Server("test-llama-hd128", device="cpu", kv_cache_dtype="fp4", **kw)
    # construction touches no device, so the GPU-side rules are checkable here
    for preset in ("test-bloom-hd64", "test-falcon-hd64"):
        with pytest.raises(ValueError, match="Llama and Mixtral"):
            Server(preset, device="cuda", kv_cache_dtype="fp8", **kw)
    with pytest.raises(ValueError, match="tensor-parallel"):
        Server("test-llama-hd128", device="cuda", kv_cache_dtype="fp8", tensor_parallel_ranks=2, **kw)
    s = Server("test-llama-hd128", device="cuda", kv_cache_dtype="fp8", **kw)
    assert s.cache_torch_dtype == FP8
    assert Server("test-llama-hd128", device="cpu", **kw).cache_torch_dtype == torch.float32


def test_choose_num_blocks_charges_half_the_cache(monkeypatch):
    from petals_amd.server.server import Server

    class _Props:
        total_memory = 0

    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: _Props)
    kw = dict(initial_peers=[], block_indices="0:1", throughput=1.0, device="cuda", torch_dtype="bfloat16")
    servers = {name: Server("test-llama-hd128", kv_cache_dtype=name, **kw) for name in ("bf16", "fp8")}
    cfg = servers["fp8"].config
    tokens = 1 << 22
    per_block = {
        name: s._block_param_bytes() + 2 * cfg.n_kv_heads * cfg.head_dim * tokens * nbytes
        for (name, s), nbytes in zip(servers.items(), (2, 1))
    }
    # memory for 3.5 fp8 blocks: 3 of them fit, and 1 bf16 block (the preset has 4)
    _Props.total_memory = int((3.5 * per_block["fp8"] + (2 << 30)) / 0.92) + 1
    assert cfg.num_blocks == 4 and per_block["bf16"] > 1.9 * per_block["fp8"]
    assert servers["fp8"]._choose_num_blocks(tokens) == 3
    assert servers["bf16"]._choose_num_blocks(tokens) == 1


def test_fallback_attention_dequantizes_fp8_cache():
    from petals_amd import ops

    g = torch.Generator().manual_seed(0)
    q = torch.randn(2, 4, 1, 16, generator=g)
    k = kv_fp8.roundtrip(torch.randn(2, 2, 8, 16, generator=g))
    v = kv_fp8.roundtrip(torch.randn(2, 2, 8, 16, generator=g))
    out = ops.attention_decode(q, kv_fp8.quantize(k), kv_fp8.quantize(v), 5)
    assert torch.equal(out, ops.attention_decode(q, k, v, 5))


def test_hypo_reorder_moves_fp8_bytes_cpu():
    g = torch.Generator().manual_seed(1)
    codes = torch.randint(0, 256, (4, 2, 8, 16), generator=g, dtype=torch.uint8)  # NaN codes included
    idx = torch.tensor([2, 2, 0, 1])
    assert torch.equal(kv_fp8.index_rows(codes.view(FP8), idx).view(torch.uint8), codes[idx])


# ------------------------------------------------- fp8 tables (CPU, float64)


def _place_needles_on_grid(q, k, needles, alphas, mass_of, gq):
    """test_attention_numerics._place_needles with every needle row passed
    through the quantizer; alpha grows (x1.5 per round, per needle) from the
    bf16 table's value until the mass holds on the quantized grid."""
    k = k.clone()
    alphas = list(alphas)
    qhat = _unit(q)
    for _ in range(40):
        for (bi, h, row, key), a in zip(needles, alphas):
            k[bi, h // gq, key] = kv_fp8.roundtrip((a * qhat[bi, h, row]).to(torch.bfloat16))
        mass = mass_of(k)
        bad = [i for i, m in enumerate(mass) if not m >= NEEDLE_MASS]
        if not bad:
            return k, tuple(alphas)
        for i in bad:
            alphas[i] *= 1.5
    raise AssertionError(f"needles never reached {NEEDLE_MASS} on the e4m3 grid: {min(mass)}")


@functools.lru_cache(maxsize=None)
def fp8_decode_inputs(case, variant):
    base = decode_inputs(case, variant)
    if base is None:
        return None
    k, v = kv_fp8.roundtrip(base.k), kv_fp8.roundtrip(base.v)
    alphas = base.alphas
    if base.needles:

        def mass_of(kk):
            p = ref_probs_f64(base.q, kk, base.kv_len, base.scale, False, 0, base.slopes)
            return [p[bi, hh, row, key].item() for (bi, hh, row, key) in base.needles]

        k, alphas = _place_needles_on_grid(base.q, k, base.needles, base.alphas, mass_of, case.gq)
    # poison again at the (possibly raised) needle strength, then onto the grid:
    # K needles, V = 1e4 -> 448
    _poison(base.q, k, v, base.kv_len, case.gq, max(alphas, default=ALPHA0), torch.zeros(1, dtype=torch.long))
    k, v = kv_fp8.roundtrip(k), kv_fp8.roundtrip(v)
    return dataclasses.replace(base, k=k, v=v, alphas=alphas)


@functools.lru_cache(maxsize=None)
def fp8_prefill_inputs(case, pattern):
    base = prefill_inputs(case, pattern)
    shift = 0 if pattern == "diag" else 1
    k, v = kv_fp8.roundtrip(base.k), kv_fp8.roundtrip(base.v)

    def mass_of(kk):
        p = ref_probs_f64(base.q, kk, base.kv_len + shift, base.scale, case.causal, case.off + shift, base.slopes)
        return [p[bi, hh, row, key].item() for (bi, hh, row, key) in base.needles]

    k, alphas = _place_needles_on_grid(base.q, k, base.needles, base.alphas, mass_of, case.qh // case.kvh)
    inp = dataclasses.replace(base, k=k, v=v, alphas=alphas)
    if pattern == "forbid":
        p = ref_probs_f64(inp.q, k, inp.kv_len, inp.scale, case.causal, case.off, inp.slopes)
        assert all(key >= inp.kv_len or p[bi, hh, row, key] == 0 for (bi, hh, row, key) in inp.needles)
    return inp


@functools.lru_cache(maxsize=None)
def fp8_writer_attn(kernel, hd, pos):
    """The decode problem over the EXPECTED fp8 cache of a writer case: the
    bf16 case's cache through the quantizer, with the needle row (position
    `pos`) strengthened on the grid where the round trip cost it its mass."""
    base = writer_inputs(kernel, hd, pos).attn
    k, v = kv_fp8.roundtrip(base.k), kv_fp8.roundtrip(base.v)

    def mass_of(kk):
        p = ref_probs_f64(base.q, kk, base.kv_len, base.scale, False, 0, None)
        return [p[bi, hh, row, key].item() for (bi, hh, row, key) in base.needles]

    k, alphas = _place_needles_on_grid(base.q, k, base.needles, base.alphas, mass_of, WRITER_QH // WRITER_KH)
    return dataclasses.replace(base, k=k, v=v, alphas=alphas)


def _fp8_decode_like():
    for p in DECODE_PARAMS:
        yield p.id, fp8_decode_inputs(*p.values)
    for p in WRITER_PARAMS:
        yield "W-" + p.id, fp8_writer_attn(*p.values)


def _fp8_prefill_like():
    for p in PREFILL_PARAMS:
        yield p.id, fp8_prefill_inputs(*p.values)


def test_fp8_tables_are_on_the_grid_and_needles_dominate():
    for _, inp in list(_fp8_decode_like()) + list(_fp8_prefill_like()):
        for t in (inp.k, inp.v):
            assert torch.equal(kv_fp8.roundtrip(t).view(torch.int16), t.view(torch.int16))
        if inp.kernel == "decode":
            p = ref_probs_f64(inp.q, inp.k, inp.kv_len, inp.scale, False, 0, inp.slopes)
            assert all(p[bi, h, row, key] >= NEEDLE_MASS for bi, h, row, key in inp.needles)
        if inp.kv_len < inp.k.shape[2]:
            assert (inp.v[:, :, inp.kv_len :] == 448.0).all()
            assert (kv_fp8.quantize(inp.v_nan()).view(torch.uint8)[:, :, inp.kv_len :] == 0x7F).all()


def test_fp8_emulated_error_within_quarter_tol():
    for tol, kind, items in (
        (TOL_FP8_DECODE, "decode", _fp8_decode_like()),
        (TOL_FP8_PREFILL, "prefill", _fp8_prefill_like()),
    ):
        for name, inp in items:
            e = nerr(inp.emulated, inp.ref)
            print(f"fp8 emulated {kind:8s} {name:64s} nerr={e:.5f}  alpha_max={max(inp.alphas, default=0):.0f}")
            assert e <= tol / 4, (name, e, tol)


def test_fp8_tolerance_constants_are_measured():
    """TOL_FP8_* = 4 x the measured worst emulation error on the round-tripped
    tables, rounded up: neither stale-low nor padded."""
    for tol, items in ((TOL_FP8_DECODE, _fp8_decode_like()), (TOL_FP8_PREFILL, _fp8_prefill_like())):
        worst = max(nerr(inp.emulated, inp.ref) for _, inp in items)
        print(f"worst emulated nerr {worst:.5f} (tol {tol})")
        assert 0.95 * tol / 4 <= worst <= tol / 4, (worst, tol)


@pytest.mark.parametrize("mutant", DECODE_MUTANTS, ids=lambda m: m.__name__)
def test_fp8_decode_mutant_rejected(mutant):
    e, where = _worst_rejection(mutant, DECODE_PARAMS, fp8_decode_inputs)
    print(f"{mutant.__name__}: nerr={e:.4f} at {where} (needs >= {2 * TOL_FP8_DECODE})")
    assert e >= 2 * TOL_FP8_DECODE, (mutant.__name__, e, where)


@pytest.mark.parametrize("mutant", PREFILL_MUTANTS, ids=lambda m: m.__name__)
def test_fp8_prefill_mutant_rejected(mutant):
    e, where = _worst_rejection(mutant, PREFILL_PARAMS, fp8_prefill_inputs)
    print(f"{mutant.__name__}: nerr={e:.4f} at {where} (needs >= {2 * TOL_FP8_PREFILL})")
    assert e >= 2 * TOL_FP8_PREFILL, (mutant.__name__, e, where)


# ---------------------------------------------------------- GPU: the kernels


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


def _bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == FP8:
        return t.contiguous().view(torch.uint8)
    return t.contiguous().view(torch.int16)


def _gpu_decode_subset():
    """Every regime of DECODE_CASES: kv_len 1 / 31 / 32 / 33 / 128 at one
    split, the 640-row (5 splits) and 8192-row (64 splits) caches, explicit
    splits 3 and 7, the multi-group gq 29 / 71 at hd 64, one ALiBi case."""
    want = {
        ("A", 1), ("A", 31), ("A", 32), ("A", 33), ("A", 128), ("B", 500), ("B", 640),
        ("C", 2049), ("C", 8192), ("E", 500),
    }
    out = [c for c in DECODE_CASES if (c.group, c.kv_len) in want]
    out += [c for c in DECODE_CASES if c.group == "D" and (c.gq, c.kv_len) in ((29, 333), (71, 95))]
    out += [c for c in DECODE_CASES if c.group == "F" and (c.hd, c.kv_len) == (128, 1500)]
    return out


FP8_DECODE_PARAMS = [
    pytest.param(c, var, id=f"{c.id}-{var}")
    for c in _gpu_decode_subset()
    for var in ("sharp", "needle0", "pair")
    if fp8_decode_inputs(c, var) is not None
]


def test_gpu_decode_subset_reaches_its_regimes():
    cases = _gpu_decode_subset()
    assert {c.kv_len for c in cases if c.group == "A"} == {1, 31, 32, 33, 128}
    assert {mfma_auto_splits(c.b, c.kvh, c.lmax) for c in cases if c.group in "BC"} == {5, 64}
    assert {c.n_splits for c in cases if c.group == "E"} == {3, 7}
    assert {(c.hd, c.gq) for c in cases if c.group == "D"} == {(64, 29), (64, 71)}
    assert sum(c.alibi for c in cases) == 1 and len(cases) == 14
    assert {p.values[1] for p in FP8_DECODE_PARAMS} == {"sharp", "needle0", "pair"}


def _decode_once(hip, inp, case, k_dev, v_dev):
    """One attn_decode_fused call with NaN-filled, oversize split workspaces
    (they must be written before they are read)."""
    b, h, _, hd = inp.q.shape
    ns = case.n_splits or mfma_auto_splits(case.b, case.kvh, case.lmax)
    part_o = torch.full((b * case.kvh * ns * case.gq * hd + 4099,), float("nan"), device="cuda")
    part_ml = torch.full((b * case.kvh * ns * case.gq * 2 + 131,), float("nan"), device="cuda")
    q = inp.q.reshape(b, h * hd).contiguous().cuda()
    kv_len_t = torch.tensor([inp.kv_len], dtype=torch.int32, device="cuda")
    slopes = inp.slopes.cuda() if inp.slopes is not None else None
    out = hip.attn_decode_fused(q, k_dev, v_dev, kv_len_t, case.gq, case.n_splits, part_o, part_ml, inp.scale, slopes)
    return out.cpu().view(b, h, 1, hd)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case,variant", FP8_DECODE_PARAMS)
def test_attn_decode_fp8(hip, case, variant):
    """fp8 caches: (a) bit-identical to the bf16 kernel on the dequantized
    cache, same n_splits; (b) within TOL_FP8_DECODE of float64. Poison tails
    V = 448 and V = NaN (0x7F); every call twice."""
    inp = fp8_decode_inputs(case, variant)
    k8 = kv_fp8.quantize(inp.k).cuda()
    for v in (inp.v, inp.v_nan()):
        v8 = kv_fp8.quantize(v).cuda()
        assert torch.equal(_bits(kv_fp8.dequantize(v8.cpu(), torch.bfloat16)), _bits(v))  # same problem
        out8 = _decode_once(hip, inp, case, k8, v8)
        assert torch.equal(_bits(out8), _bits(_decode_once(hip, inp, case, k8, v8))), "fp8 run is not reproducible"
        out16 = _decode_once(hip, inp, case, kv_fp8.dequantize(k8, torch.bfloat16), kv_fp8.dequantize(v8, torch.bfloat16))
        e = nerr(out8, inp.ref)
        print(f"decode fp8 {case.id}-{variant}: nerr={e:.5f} tol={TOL_FP8_DECODE}")
        assert torch.equal(_bits(out8), _bits(out16)), (out8 - out16).abs().max()
        assert e <= TOL_FP8_DECODE, e


FP8_PREFILL_PARAMS = [
    pytest.param(c, pat, id=f"{c.id}-{pat}")
    for c in (PREFILL_CASES[0], PREFILL_CASES[1], PREFILL_CASES[2], PREFILL_CASES[4])
    for pat in ("diag", "forbid")
    if c.causal or pat == "diag"
]


def test_gpu_prefill_subset_is_the_issue_list():
    got = [(c.b, c.qh, c.kvh, c.s, c.hd, c.off, c.causal) for c in dict.fromkeys(p.values[0] for p in FP8_PREFILL_PARAMS)]
    assert got == [
        (2, 4, 2, 17, 128, 0, True), (1, 4, 4, 65, 128, 63, True), (1, 8, 2, 130, 64, 70, True),
        (2, 4, 2, 70, 64, 0, False),
    ]
    assert all(fp8_prefill_inputs(*p.values).k.shape[2] - fp8_prefill_inputs(*p.values).kv_len == 37 for p in FP8_PREFILL_PARAMS)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case,pattern", FP8_PREFILL_PARAMS)
def test_attn_prefill_fp8(hip, case, pattern):
    inp = fp8_prefill_inputs(case, pattern)
    q, k8 = inp.q.cuda(), kv_fp8.quantize(inp.k).cuda()

    def run(k, v):
        return hip.attn_prefill_fused(q, k, v, inp.kv_len, inp.kv_offset, inp.scale, inp.causal, None).cpu()

    for v in (inp.v, inp.v_nan()):
        v8 = kv_fp8.quantize(v).cuda()
        out8 = run(k8, v8)
        assert torch.equal(_bits(out8), _bits(run(k8, v8))), "fp8 run is not reproducible"
        out16 = run(kv_fp8.dequantize(k8, torch.bfloat16), kv_fp8.dequantize(v8, torch.bfloat16))
        e = nerr(out8, inp.ref)
        print(f"prefill fp8 {case.id}-{pattern}: nerr={e:.5f} tol={TOL_FP8_PREFILL}")
        assert torch.equal(_bits(out8), _bits(out16)), (out8.float() - out16.float()).abs().max()
        assert e <= TOL_FP8_PREFILL, e


@pytest.mark.gpu
@requires_gpu
def test_kernels_reject_mixed_cache_dtypes(hip):
    k8 = torch.zeros(1, 2, 32, 128, device="cuda", dtype=FP8)
    v16 = torch.zeros(1, 2, 32, 128, device="cuda", dtype=torch.bfloat16)
    q = torch.zeros(1, 8 * 128, device="cuda")
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    empty = torch.empty(0, device="cuda")
    with pytest.raises(RuntimeError):
        hip.attn_decode_fused(q, k8, v16, one, 4, 0, empty, empty, 1.0, None)
    with pytest.raises(RuntimeError):
        hip.attn_prefill_fused(torch.zeros(1, 8, 4, 128, device="cuda", dtype=torch.bfloat16), k8, v16, 4, 0, 1.0, True, None)
    with pytest.raises(RuntimeError):
        hip.kv_cache_write(torch.zeros(1, 12 * 128, device="cuda"), one, k8, v16, 8, 2)
    with pytest.raises(RuntimeError):
        hip.kv_cache_store_fp8(torch.zeros(1, 2, 4, 128, device="cuda", dtype=torch.bfloat16), v16, 0)
    with pytest.raises(RuntimeError):  # past the end of the cache
        hip.kv_cache_store_fp8(torch.zeros(1, 2, 4, 128, device="cuda", dtype=torch.bfloat16), k8, 29)


# ----------------------------------------------------------- GPU: the writers


def _ordered_codes(c):
    """e4m3 codes mapped to integers monotonic in the value."""
    b = c.contiguous().view(torch.uint8).to(torch.int32)
    return torch.where(b >= 128, -(b & 0x7F), b)


def _call_writer(hip, kernel, w, src, pos, k_cache, v_cache):
    qh, kh = WRITER_QH, WRITER_KH
    hd = k_cache.shape[-1]
    pos_t = torch.tensor([pos], dtype=torch.int32, device="cuda")
    if kernel == "rope_cache_write":
        hip.rope_cache_write(src, w.cos.cuda(), w.sin.cuda(), pos_t, k_cache, v_cache, qh, kh)
        return src[:, : qh * hd].contiguous()
    if kernel == "kv_cache_write":
        hip.kv_cache_write(src, pos_t, k_cache, v_cache, qh, kh)
        return src[:, : qh * hd].contiguous()
    if kernel == "qkv_rope_reduce_rope":
        return hip.qkv_rope_reduce(src, w.cos.cuda(), w.sin.cuda(), pos_t, k_cache, v_cache, qh, kh, True, None)
    return hip.qkv_rope_reduce(src, None, None, pos_t, k_cache, v_cache, qh, kh, False, w.bias.cuda())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("kernel,hd,pos", WRITER_PARAMS)
def test_cache_writers_fp8(hip, kernel, hd, pos):
    """The decode-step writers into fp8 caches at device positions 0, 1, 2047.

    V, and K where the kernel does not rotate: the written byte is
    `quantize(x)` of the kernel's fp32 value x. For rope_cache_write and
    kv_cache_write x IS the fp32 input, so the bytes are compared exactly. The
    qkv_rope_reduce forms first sum three split partials (and a bias) in fp32;
    the summation order is the compiler's, so x is known to
    3 * 2^-24 * sum|terms| and the byte must lie between the quantized ends of
    that interval (the same byte except within that distance of a rounding
    boundary). Rotated K: |dequantized - ref64| <= spacing/2 + 1e-5 |ref64|
    (the fp32 rotation may contract FMAs: the 1e-5 the bf16 test grants q)."""
    w = writer_inputs(kernel, hd, pos)
    b, qh, kh = WRITER_B, WRITER_QH, WRITER_KH
    rope = kernel in ("rope_cache_write", "qkv_rope_reduce_rope")
    reduce = kernel.startswith("qkv_rope_reduce")
    k0, v0 = kv_fp8.quantize(w.k0), kv_fp8.quantize(w.v0)
    k_cache, v_cache = k0.cuda(), v0.cuda()
    q = _call_writer(hip, kernel, w, w.src.clone().cuda(), pos, k_cache, v_cache)
    k_got, v_got = k_cache.cpu(), v_cache.cpu()

    q_got = q.cpu().to(torch.float64).view(b, qh, hd)
    q_err = ((q_got - w.q_ref).abs().amax(-1) / w.q_ref.abs().amax(-1)).max().item()
    assert q_err <= 1e-5, q_err

    def check_unrotated(got_row, ref64, lo_hd):
        if not reduce:
            x = w.src.view(b, qh + 2 * kh, hd)[:, lo_hd : lo_hd + kh]
            assert torch.equal(_bits(got_row), _bits(kv_fp8.quantize(x)))
            return
        terms = w.src.to(torch.float64).abs().sum(0)
        if w.bias is not None:
            terms = terms + w.bias.to(torch.float64).abs()
        slack = 3 * 2.0**-24 * terms.view(b, qh + 2 * kh, hd)[:, lo_hd : lo_hd + kh]
        lo, hi = kv_fp8.quantize(ref64 - slack), kv_fp8.quantize(ref64 + slack)
        code = _ordered_codes(got_row)
        assert ((_ordered_codes(lo) <= code) & (code <= _ordered_codes(hi))).all()
        assert (_ordered_codes(lo) == _ordered_codes(hi)).float().mean() > 0.99  # the check is sharp

    check_unrotated(v_got[:, :, pos], w.v_ref, qh + kh)
    if rope:
        deq = kv_fp8.dequantize(k_got[:, :, pos], torch.float32).to(torch.float64)
        bound = 0.5 * kv_fp8.spacing(w.k_ref) + 1e-5 * w.k_ref.abs()
        assert w.k_ref.abs().max() < 448
        assert ((deq - w.k_ref).abs() <= bound).all(), ((deq - w.k_ref).abs() / bound).max()
    else:
        check_unrotated(k_got[:, :, pos], w.k_ref, qh)

    # every other byte of both caches is untouched
    for got, before in ((k_got, k0), (v_got, v0)):
        rest = got.clone()
        rest[:, :, pos] = before[:, :, pos]
        assert torch.equal(_bits(rest), _bits(before))

    # reader and writer agree: decode attention over the written cache, (b)
    written = dataclasses.replace(
        w.attn, q=q.cpu().view(b, qh, 1, hd), k=kv_fp8.dequantize(k_got), v=kv_fp8.dequantize(v_got)
    )
    ref = fp8_writer_attn(kernel, hd, pos)
    # the expected cache and the written one differ by at most a neighbour
    # flip in the written row; judge against float64 over what was written
    ref64 = ref_attention_f64(*written.args())
    case = type("C", (), dict(n_splits=0, b=b, kvh=kh, lmax=k_got.shape[2], gq=qh // kh))
    for v in (written.v, written.v_nan()):
        out = _decode_once(hip, written, case, k_cache, kv_fp8.quantize(v).cuda())
        e = nerr(out, ref64)
        print(f"writer fp8 {kernel}-hd{hd}-pos{pos}: q_err={q_err:.2e} attn nerr={e:.5f} tol={TOL_FP8_DECODE}")
        assert e <= TOL_FP8_DECODE, e
    p = ref_probs_f64(written.q, written.k, written.kv_len, written.scale)
    if pos > 0:  # the written row still carries the needle (0.98: a neighbour flip of the expected 0.99 row)
        assert min(p[bi, h, 0, key].item() for bi, h, _, key in ref.needles) >= 0.98

    # planted overflow: beyond +-448 saturates, never NaN (second call, fresh caches)
    src = w.src.clone()
    flat = src.view(-1, src.shape[-1])  # last split (or the only row set) carries the plants
    plant = torch.tensor([1e4, -1e4, 464.0, -600.0, 3e38, -3e38])
    kv_cols = torch.arange(qh * hd, (qh + 2 * kh) * hd)
    cols = kv_cols[torch.arange(len(plant)) * 37 % len(kv_cols)]
    rows = flat[-b:]
    big = plant.repeat(b, 1)
    if reduce:  # make the three-term sum itself the planted value
        rows[:, cols] = big - (src[:-1].sum(0)[:, cols] + (w.bias.float()[cols] if w.bias is not None else 0))
    else:
        rows[:, cols] = big
    k2, v2 = k0.cuda(), v0.cuda()
    _call_writer(hip, kernel, w, src.cuda(), pos, k2, v2)
    for c in (k2.cpu(), v2.cpu()):
        row = kv_fp8.dequantize(c[:, :, pos], torch.float32)
        assert not torch.isnan(row).any(), "overflow became NaN"
    both = torch.cat([kv_fp8.dequantize(k2.cpu()[:, :, pos], torch.float32).reshape(b, -1),
                      kv_fp8.dequantize(v2.cpu()[:, :, pos], torch.float32).reshape(b, -1)], 1)
    sat = both[:, cols - qh * hd]
    if not rope:
        assert torch.equal(sat, torch.sign(big) * 448.0)
    else:  # K plants are rotated with their (ordinary) partners: still huge, so saturated
        is_v = cols >= (qh + kh) * hd
        assert torch.equal(sat[:, is_v], (torch.sign(big) * 448.0)[:, is_v])
        assert (both.abs() <= 448.0).all()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("s,off", [(1, 0), (17, 0), (1, 63), (17, 63)])
def test_kv_cache_store_fp8(hip, s, off):
    """The prefill store: bytes equal `quantize`, rows outside [off, off+s)
    and batch rows past B untouched; NaN stays NaN, overflow saturates."""
    g = torch.Generator().manual_seed(100 * s + off)
    for hd in (64, 128):
        b, bc, kh, lmax = 2, 3, 2, 96
        new = (3.0 * torch.randn(b, kh, s, hd, generator=g)).to(torch.bfloat16)
        new.view(-1)[::7] *= 200.0  # overflow on both signs
        new.view(-1)[5::11] *= 2.0**-9  # subnormals and zeros
        new[0, 0, 0, 3] = float("nan")
        new[1, 1, s - 1, hd - 1] = float("inf")
        before = torch.randint(0, 256, (bc, kh, lmax, hd), generator=g, dtype=torch.uint8)
        cache = before.view(FP8).cuda()
        hip.kv_cache_store_fp8(new.cuda(), cache, off)
        # a transposed (non-contiguous) source, as the prefill path passes V
        cache_t = before.view(FP8).cuda()
        hip.kv_cache_store_fp8(new.transpose(1, 2).contiguous().cuda().transpose(1, 2), cache_t, off)
        want = before.clone()
        want[:b, :, off : off + s] = kv_fp8.quantize(new).view(torch.uint8)
        assert torch.equal(cache.cpu().view(torch.uint8), want)
        assert torch.equal(cache_t.cpu().view(torch.uint8), want)
        got = kv_fp8.dequantize(cache.cpu()[:b, :, off : off + s], torch.float32)
        assert torch.isnan(got[0, 0, 0, 3]) and int(torch.isnan(got).sum()) == 1 and got[1, 1, s - 1, hd - 1] == 448.0


# ------------------------------------------------- blocks (CPU reference, GPU)

BLOCK_PRESETS = ("test-llama-hd128", "test-mixtral-hd64")
BLOCK_B, BLOCK_PREFILL, BLOCK_STEPS, BLOCK_LMAX = 2, 5, 3, 16

# Block tolerance, as |out - ref| <= tol * (1 + |ref|) (the form of the bf16
# block tests' atol = rtol = 2e-2). tol is the larger of that 2e-2 and 4x the
# change of the REFERENCE ITSELF when K/V are rounded to bf16 before the
# quantizer, as the GPU prefill does (its projections come out in bf16): a value
# that lands on the other side of an e4m3 rounding boundary moves a whole
# spacing (the neighbour flip). Measured on the CPU, fp32 blocks
# (`test_block_tolerance_is_measured`):
#   test-llama-hd128   0.01103 (1.44 % of K entries flip) -> x4 = 0.0442 > 2e-2
#   test-mixtral-hd64  0.00385 (1.86 % of K entries flip) -> x4 = 0.0154 < 2e-2
BLOCK_FLIP_MEASURED = {"test-llama-hd128": 0.01103, "test-mixtral-hd64": 0.00385}
BLOCK_TOL = {"test-llama-hd128": 0.0442, "test-mixtral-hd64": 2e-2}


def _block_err(out, ref):
    return ((out - ref).abs() / (1 + ref.abs())).max().item()


def _cpu_block(preset):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.server.from_pretrained import init_random_block_

    cfg = load_model_config(preset)
    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    blk = blk.float().eval()
    with torch.no_grad():  # the values the bf16 GPU block holds
        for p in blk.parameters():
            p.copy_(p.to(torch.bfloat16).to(p.dtype))
    return cfg, blk


def _block_inputs(cfg):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(BLOCK_B, BLOCK_PREFILL + BLOCK_STEPS, cfg.hidden_size, generator=g) * 0.5
    return x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _block_reference(preset, pre_bf16: bool):
    """fp32 CPU block over a 5-token prefill and 3 decode steps whose K/V pass
    through `quantize` after each write (before the attention reads them);
    `pre_bf16` rounds them to bf16 first. Returns (outputs, k_cache, v_cache)."""
    from petals_amd import ops

    cfg, blk = _cpu_block(preset)
    x = _block_inputs(cfg)
    real = ops.attention_decode

    def quantizing(q, k_cache, v_cache, kv_len, **kw):
        for c in (k_cache, v_cache):
            rows = c[:, :, :kv_len]
            if pre_bf16:
                rows = rows.to(torch.bfloat16).to(c.dtype)
            c[:, :, :kv_len] = kv_fp8.roundtrip(rows)  # idempotent on the older rows
        return real(q, k_cache, v_cache, kv_len, **kw)

    ks, vs = blk.kv_cache_shape(BLOCK_B, BLOCK_LMAX)
    kc, vc = torch.zeros(ks), torch.zeros(vs)
    ops.attention_decode = quantizing
    try:
        with torch.inference_mode():
            ys = [blk(x[:, :BLOCK_PREFILL], kv_cache=(kc, vc), prefix_length=0)]
            for t in range(BLOCK_PREFILL, x.shape[1]):
                ys.append(blk(x[:, t : t + 1], kv_cache=(kc, vc), prefix_length=t))
    finally:
        ops.attention_decode = real
    return torch.cat(ys, 1), kc, vc


@pytest.mark.parametrize("preset", BLOCK_PRESETS)
def test_block_tolerance_is_measured(preset):
    ref, kc, _ = _block_reference(preset, False)
    ref16, kc16, _ = _block_reference(preset, True)
    change = _block_err(ref16, ref)
    flips = (kc != kc16).float().mean().item()
    print(f"{preset}: reference change under bf16-first rounding {change:.5f}, {flips:.4%} of K entries flip")
    assert torch.equal(kv_fp8.roundtrip(kc), kc) and kc.abs().sum() > 0
    assert flips > 0, "the bf16-first rounding moved no entry: the measurement is vacuous"
    m = BLOCK_FLIP_MEASURED[preset]
    assert 0.9 * m <= change <= 1.1 * m, (change, m)
    assert BLOCK_TOL[preset] == max(2e-2, math.ceil(4 * m * 1e4) / 1e4)


def _gpu_block(preset, cpu_blk):
    from petals_amd.models import get_model_block

    blk = get_model_block(cpu_blk.config, 0)
    blk.load_state_dict(cpu_blk.state_dict())
    blk = blk.to("cuda", torch.bfloat16).eval().optimize_for_inference()
    assert blk._fast is not None, f"{preset} must take the fused path"
    return blk


def _fp8_caches(blk, b, lmax):
    ks, vs = blk.kv_cache_shape(b, lmax)
    return torch.zeros(ks, device="cuda", dtype=FP8), torch.zeros(vs, device="cuda", dtype=FP8)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("preset", BLOCK_PRESETS)
def test_block_fp8_cache_matches_quantizing_cpu_block(hip, preset):
    ref, kc, vc = _block_reference(preset, False)
    cfg, cpu_blk = _cpu_block(preset)
    blk = _gpu_block(preset, cpu_blk)
    x = _block_inputs(cfg).cuda().to(torch.bfloat16)
    kg, vg = _fp8_caches(blk, BLOCK_B, BLOCK_LMAX)
    with torch.inference_mode():
        ys = [blk(x[:, :BLOCK_PREFILL], kv_cache=(kg, vg), prefix_length=0)]
        for t in range(BLOCK_PREFILL, x.shape[1]):
            ys.append(blk(x[:, t : t + 1], kv_cache=(kg, vg), prefix_length=t))
    out = torch.cat([y.float().cpu() for y in ys], 1)
    e = _block_err(out, ref)
    print(f"{preset}: fp8-cache block err {e:.5f} (tol {BLOCK_TOL[preset]})")
    assert kg.dtype == FP8 and torch.isfinite(out).all()
    assert e <= BLOCK_TOL[preset], e
    # the caches hold what the reference's hold, up to neighbour flips
    n = x.shape[1]
    for got, want in ((kg, kc), (vg, vc)):
        got = kv_fp8.dequantize(got.cpu(), torch.float32)
        assert (got[:, :, n:] == 0).all()
        d = (got[:, :, :n] - want[:, :, :n]).abs()
        assert (d <= kv_fp8.spacing(want[:, :, :n]) * 1.001 + 2.0**-9).all()
        assert (d == 0).float().mean() > 0.9


@pytest.mark.gpu
@requires_gpu
def test_block_fp8_adapter_path_writes_through_rope_cache_write(hip):
    """A LoRA adapter routes the decode step through rope_cache_write; a zero
    adapter must reproduce the adapter-free step. The two paths sum the qkv
    split partials in different fp32 orders, so a cache entry may land on the
    neighbouring code; nearly all are equal."""
    from petals_amd.utils.peft import BlockAdapter, add_adapter_to_block, using_adapter

    cfg, cpu_blk = _cpu_block("test-llama-hd128")
    blk = _gpu_block("test-llama-hd128", cpu_blk)
    r, hsz = 2, cfg.hidden_size
    kvd = cfg.n_kv_heads * cfg.head_dim
    weights = {
        key: (torch.zeros(r, hsz), torch.zeros(out, r), 1.0)
        for key, out in (("q", hsz), ("k", kvd), ("v", kvd))
    }
    add_adapter_to_block(blk, BlockAdapter("zero", weights))
    x = _block_inputs(cfg).cuda().to(torch.bfloat16)
    (k1, v1), (k2, v2) = _fp8_caches(blk, BLOCK_B, BLOCK_LMAX), _fp8_caches(blk, BLOCK_B, BLOCK_LMAX)
    with torch.inference_mode():
        for t in range(3):
            y1 = blk(x[:, t : t + 1], kv_cache=(k1, v1), prefix_length=t)
            with using_adapter("zero"):
                y2 = blk(x[:, t : t + 1], kv_cache=(k2, v2), prefix_length=t)
            assert torch.allclose(y1.float(), y2.float(), atol=2e-2, rtol=2e-2)
    for c1, c2 in ((k1, k2), (v1, v2)):
        d1, d2 = kv_fp8.dequantize(c1.cpu(), torch.float32), kv_fp8.dequantize(c2.cpu(), torch.float32)
        assert ((d1 - d2).abs() <= kv_fp8.spacing(d1) * 1.001).all()
        assert (_bits(c1) == _bits(c2)).float().mean() > 0.999
        assert c1.view(torch.uint8)[:, :, :3].any() and not c1.view(torch.uint8)[:, :, 3:].any()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("preset", BLOCK_PRESETS)
def test_block_fp8_decode_graph_matches_eager(hip, preset):
    """One captured decode step over fp8 caches, replayed with a moving device
    position, equals the eager step of a second block bit for bit."""
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.utils.graphs import GraphedCallable

    cfg, cpu_blk = _cpu_block(preset)
    blk, blk2 = _gpu_block(preset, cpu_blk), _gpu_block(preset, cpu_blk)
    assert blk._fast.graph_safe
    x = _block_inputs(cfg).cuda().to(torch.bfloat16)
    (kg, vg), (kg2, vg2) = _fp8_caches(blk, BLOCK_B, BLOCK_LMAX), _fp8_caches(blk, BLOCK_B, BLOCK_LMAX)
    ctx = DecodeContext(torch.device("cuda"))
    ctx.set_position(0)
    h_in = torch.empty_like(x[:, :1])
    graph = GraphedCallable(lambda: blk(h_in, kv_cache=(kg, vg), ctx=ctx), [])
    with torch.inference_mode():
        for t in range(4):
            ctx.set_position(t)
            h_in.copy_(x[:, t : t + 1])
            og = graph.replay().clone()
            oe = blk2(x[:, t : t + 1].contiguous(), kv_cache=(kg2, vg2), prefix_length=t)
            assert torch.equal(_bits(og.cpu()), _bits(oe.cpu())), (t, (og.float() - oe.float()).abs().max())
    assert torch.equal(_bits(kg), _bits(kg2)) and torch.equal(_bits(vg), _bits(vg2))
    assert kg.view(torch.uint8)[:, :, :4].any() and not kg.view(torch.uint8)[:, :, 4:].any()


@pytest.mark.gpu
@requires_gpu
def test_backend_hypo_reorder_permutes_fp8_bytes(hip):
    from petals_amd.data_structures import InferenceMetadata
    from petals_amd.server.backend import TransformerBackend
    from petals_amd.server.memory_cache import MemoryCache

    cfg, cpu_blk = _cpu_block("test-llama-hd128")
    blk = _gpu_block("test-llama-hd128", cpu_blk)
    mc = MemoryCache(1 << 26, torch.device("cuda"))
    be = TransformerBackend("u.0", blk, config=cfg, memory_cache=mc, dtype=torch.bfloat16, cache_dtype=FP8)
    b, lmax, pos = 3, 16, 6
    hypo = torch.tensor([2, 0, 0])
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(b, 1, cfg.hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()

    async def run():
        async with mc.allocate_cache(*be.get_inference_cache_descriptors(b, lmax)) as handles:
            with mc.use_cache(*handles) as (k, v):
                assert k.dtype == FP8 and v.dtype == FP8
                codes = [torch.randint(0, 256, k.shape, generator=g, dtype=torch.uint8) for _ in range(2)]
                k.view(torch.uint8).copy_(codes[0])  # every byte pattern, NaN codes included
                v.view(torch.uint8).copy_(codes[1])
            be.inference_step(x, hypo, InferenceMetadata("u.0", pos, tuple(handles), None))
            with mc.use_cache(*handles) as (k, v):
                return codes, k.cpu().view(torch.uint8), v.cpu().view(torch.uint8)

    codes, k_after, v_after = asyncio.run(run())
    for before, after in zip(codes, (k_after, v_after)):
        want = before[hypo]
        keep = torch.ones(lmax, dtype=torch.bool)
        keep[pos] = False  # the step then wrote row `pos`
        assert torch.equal(after[:, :, keep], want[:, :, keep])
        assert not torch.equal(after[:, :, pos], want[:, :, pos])


@pytest.mark.gpu
@requires_gpu
def test_llama_hd128_fp8_cache_serving_uses_span_graph(monkeypatch):
    """A GPU server with kv_cache_dtype="fp8": generate() steps the span
    graph over fp8 cache tensors, rpc_info reports the dtype."""
    from petals_amd.dht.node import DHT
    from petals_amd.server import handler
    from petals_amd.server.server import Server
    from petals_amd.utils.auto_config import AutoDistributedModelForCausalLM

    monkeypatch.delenv("PETALS_AMD_NO_GRAPHS", raising=False)
    calls, cache_dtypes = [], set()
    real_init, real_step = handler._SpanDecodeGraph.__init__, handler._SpanDecodeGraph.step

    def recording_init(self, blocks, cache_pairs, *a, **kw):
        cache_dtypes.update(t.dtype for pair in cache_pairs for t in pair)
        return real_init(self, blocks, cache_pairs, *a, **kw)

    def counting_step(self, hidden_states, prefix_length):
        calls.append(prefix_length)
        return real_step(self, hidden_states, prefix_length)

    monkeypatch.setattr(handler._SpanDecodeGraph, "__init__", recording_init)
    monkeypatch.setattr(handler._SpanDecodeGraph, "step", counting_step)

    preset, prefix = "test-llama-hd128", "gpu-kvfp8"
    boot = DHT(host="127.0.0.1")
    kw = dict(initial_peers=[boot.listen_addr], host="127.0.0.1", device="cuda", torch_dtype="bfloat16",
              block_indices="0:4", dht_prefix=prefix, throughput=1.0, attn_cache_tokens=4096)
    server = Server(preset, kv_cache_dtype="fp8", **kw).start()
    try:
        cfg = server.config
        assert server.memory_cache.max_size_bytes == 2 * cfg.n_kv_heads * cfg.head_dim * 4096 * 1 * 4
        for backend in server.backends.values():
            assert backend.block._fast is not None and backend.cache_dtype == FP8
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
            live = list(server.memory_cache._tensors.values())
            assert live and all(t.dtype == FP8 for t in live)
        assert logits.shape == (1, 1, 128) and bool(torch.isfinite(logits.float()).all())
        assert len(calls) >= 1, "the span decode graph was never stepped"
        assert cache_dtypes == {FP8}

        class _Capture:
            msg = None

            async def close(self, msg=None):
                self.msg = msg

        cap = _Capture()
        asyncio.run_coroutine_threadsafe(server.handler.rpc_info(None, cap), server.loop).result(30)
        assert cap.msg.meta["kv_cache_dtype"] == "fp8"
        first = next(iter(server.backends.values()))
        assert cap.msg.meta["cache_tokens_left"] == server.memory_cache.bytes_left // first.cache_bytes_per_token()
        model.transformer.h.sequence_manager.shutdown()
    finally:
        server.shutdown()
        boot.shutdown()
