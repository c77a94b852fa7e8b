"""Device-routed int8 MoE experts: stacking (CPU), the routed decode GEMV
`gemv_int8_moe`, the int8 mode of the grouped prefill GEMM `moe_gemm`, and
the Mixtral block / serving paths built on them (GPU, `pytest -m gpu`).

The GPU kernels are judged against float64 references computed once on the
CPU from the very int8 codes and bf16 scales the kernels read, with bounds
that come from the arithmetic, not from the kernels' output:

* routed GEMV, fp32 accumulation of `in` terms over S splits plus the scale
  multiply: `|out - ref| <= in * 2^-23 * (|x| @ |q * scale|)` — the standard
  (n + S + 1) u bound with u = 2^-24, doubled;
* grouped GEMM, the same accumulation followed by one bf16 rounding:
  `2^-8 |ref| + in * 2^-23 * (|X| @ |W|)`.

A CPU self-check corrupts the reference three ways (expert id ignored, token
index r instead of r / k, scale taken from expert 0) and requires each to
break those bounds by >= 2x on the test inputs, so the bounds are known to
catch the indexing mistakes the kernels could make.
"""

import functools

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPI_PLAIN, EPI_SWIGLU = 0, 3
E = 4
GEMV_SHAPES = [(64, 64), (200, 520), (1024, 2048)]
GEMV_BK = [(1, 2), (3, 2), (8, 2), (5, 1)]
GEMV_SPLITS = [0, 1, 2, 5]
# distinct and repeated experts, every id in [0, E)
SEL_PATTERN = [1, 3, 0, 2, 2, 1, 3, 3, 0, 1, 2, 0, 3, 1, 0, 2]
GEMM_SHAPES = [(64, 128), (64, 384), (192, 128), (192, 384)]
GEMM_T, GEMM_K = 40, 2


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared inputs


@functools.lru_cache(maxsize=None)
def _stacked(in_dim: int, out_dim: int):
    """CPU int8 stack for (in, out); expert magnitudes differ so every expert
    has its own scales."""
    from petals_amd.ops.fused_moe import _StackedExperts

    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    wts = [
        (torch.randn(in_dim, out_dim, generator=g) * 0.03 * (e + 1)).to(torch.bfloat16)
        for e in range(E)
    ]
    return _StackedExperts(wts, None, "int8"), wts


def _w64(st) -> torch.Tensor:
    return st.q8_all.double() * st.scale8_all.double().unsqueeze(1)  # [E, in, out]


def _routed_ref(w64, x64, sel, k, *, ignore_expert=False, token_is_row=False, scale0_of=None):
    """float64 out[r] = x[r // k] @ W[sel[r]] and the |x| @ |W| magnitude.
    The keyword switches build the three corrupted references."""
    n_tok = x64.shape[0]
    rows, mags = [], []
    for r, e in enumerate(sel):
        w = w64[0 if ignore_expert else e]
        if scale0_of is not None:  # this expert's codes with expert 0's scales
            w = scale0_of.q8_all[e].double() * scale0_of.scale8_all[0].double()
        xr = x64[(r % n_tok) if token_is_row else (r // k)]
        rows.append(xr @ w)
        mags.append(xr.abs() @ w.abs())
    return torch.stack(rows), torch.stack(mags)


@functools.lru_cache(maxsize=None)
def _gemv_case(in_dim: int, out_dim: int, B: int, k: int):
    st, _ = _stacked(in_dim, out_dim)
    g = torch.Generator().manual_seed(7 + 31 * B + k)
    x = torch.randn(B, in_dim, generator=g)
    sel = SEL_PATTERN[: B * k]
    ref, mag = _routed_ref(_w64(st), x.double(), sel, k)
    bound = in_dim * 2.0 ** -23 * mag
    return st, x, sel, ref, bound


def _gemm_sel() -> torch.Tensor:
    """[T, K] expert ids: expert 2 empty, expert 1 over-full (two MT tiles)."""
    g = torch.Generator().manual_seed(5)
    sel = torch.tensor([0, 1, 3])[torch.randint(0, 3, (GEMM_T, GEMM_K), generator=g)]
    sel[:36, 0] = 1
    return sel


@functools.lru_cache(maxsize=None)
def _gemm_case(in_dim: int, out_dim: int):
    st, _ = _stacked(in_dim, out_dim)
    g = torch.Generator().manual_seed(3 + in_dim + out_dim)
    x = (torch.randn(GEMM_T, in_dim, generator=g) * 0.5).to(torch.bfloat16)
    sel = _gemm_sel()
    flat = sel.reshape(-1).tolist()
    ref, mag = _routed_ref(_w64(st), x.double(), flat, GEMM_K)
    bound = 2.0 ** -8 * ref.abs() + in_dim * 2.0 ** -23 * mag
    return st, x, sel, ref, bound


def _one_hot_rows(n: int, in_dim: int):
    """Row b is zero except one entry: 1.0 or -2.0 at a position that differs
    per row and reaches the last input rows (the kernels' tail loop)."""
    x = torch.zeros(n, in_dim)
    pos, val = [], []
    for b in range(n):
        p = (in_dim - 1 - 5 * b) % in_dim if b % 2 == 0 else (7 * b + 3) % in_dim
        v = -2.0 if b % 3 == 1 else 1.0
        x[b, p] = v
        pos.append(p)
        val.append(v)
    return x, pos, val


# ---------------------------------------------------------------- CPU tests


def test_stacked_int8_cpu_layout_and_dense():
    """int8 stacking is plain torch: constructible with hip=None on the CPU,
    and dense(e) is bit-equal to _FastWeight's quantize / dequantize formula."""
    from petals_amd.ops.fused_moe import _StackedExperts

    in_dim, out_dim = 48, 40
    g = torch.Generator().manual_seed(0)
    wts = [(torch.randn(in_dim, out_dim, generator=g) * 0.1 * (e + 1)).to(torch.bfloat16) for e in range(E)]
    wts[1][:, 3] = 0  # an all-zero column exercises the clamp_min on the scale
    st = _StackedExperts(wts, None, "int8")
    assert st.q8_all.shape == (E, in_dim, out_dim) and st.q8_all.dtype == torch.int8
    assert st.scale8_all.shape == (E, out_dim) and st.scale8_all.dtype == torch.bfloat16
    assert st.q8_all.is_contiguous() and st.scale8_all.is_contiguous()
    assert int(st.q8_all.abs().max()) <= 127
    for e in range(E):
        w = wts[e].float()
        scale = w.abs().amax(dim=0).clamp_min(1e-8) / 127.0
        q = torch.round(w / scale).clamp(-127, 127).to(torch.int8)
        s8 = scale.to(torch.bfloat16)
        assert torch.equal(st.q8_all[e], q) and torch.equal(st.scale8_all[e], s8)
        assert torch.equal(st.dense(e), (q.float() * s8.float()).bfloat16())


def test_moe_int8_mode_switch(monkeypatch):
    from petals_amd.ops.fused_moe import moe_int8_mode

    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    assert moe_int8_mode() == "device"
    monkeypatch.setenv("PETALS_AMD_MOE_INT8", "host")
    assert moe_int8_mode() == "host"
    monkeypatch.setenv("PETALS_AMD_MOE_INT8", "bogus")
    with pytest.raises(ValueError):
        moe_int8_mode()


def test_mixtral_hd64_preset():
    from petals_amd.models.config_base import load_model_config

    cfg = load_model_config("test-mixtral-hd64")
    assert cfg.hidden_size // cfg.num_attention_heads == 64
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads) == (256, 4, 2)
    assert (cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size) == (512, 4, 128)
    assert (cfg.num_local_experts, cfg.num_experts_per_tok) == (4, 2)


def _worst_break(corrupt: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    return float(((corrupt - ref).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("in_dim,out_dim", GEMV_SHAPES)
@pytest.mark.parametrize("B,k", [(3, 2), (8, 2)])
def test_reference_catches_corruptions_gemv(in_dim, out_dim, B, k):
    """A kernel that ignored the expert id, indexed x by r instead of r / k,
    or took expert 0's scales would miss the float64 bound by >= 2x."""
    st, x, sel, ref, bound = _gemv_case(in_dim, out_dim, B, k)
    w64, x64 = _w64(st), x.double()
    for name, kw in [
        ("expert id ignored", dict(ignore_expert=True)),
        ("token index r", dict(token_is_row=True)),
        ("scale of expert 0", dict(scale0_of=st)),
    ]:
        bad, _ = _routed_ref(w64, x64, sel, k, **kw)
        assert _worst_break(bad, ref, bound) >= 2.0, name


@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
def test_reference_catches_corruptions_gemm(in_dim, out_dim):
    st, x, sel, ref, bound = _gemm_case(in_dim, out_dim)
    w64, x64, flat = _w64(st), x.double(), sel.reshape(-1).tolist()
    for name, kw in [
        ("expert id ignored", dict(ignore_expert=True)),
        ("token index r", dict(token_is_row=True)),
        ("scale of expert 0", dict(scale0_of=st)),
    ]:
        bad, _ = _routed_ref(w64, x64, flat, GEMM_K, **kw)
        assert _worst_break(bad, ref, bound) >= 2.0, name


# ------------------------------------------------- GPU: gemv_int8_moe (op)


def _valid_splits(in_dim: int):
    return [s for s in GEMV_SPLITS if s <= -(-in_dim // 128)]


def _gpu_stack(st):
    return st.q8_all.cuda(), st.scale8_all.cuda()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMV_SHAPES)
@pytest.mark.parametrize("B,k", GEMV_BK)
def test_gemv_int8_moe_index_mapping_exact(hip, in_dim, out_dim, B, k):
    """One-hot x rows: out[r] == v * q8_all[e, p, :] * scale8_all[e, :] bit
    for bit (the product is exact in fp32 and every other term is zero), so a
    wrong expert, token, input row or column shows as an unequal value."""
    st, _ = _stacked(in_dim, out_dim)
    q8, s8 = _gpu_stack(st)
    x, pos, val = _one_hot_rows(B, in_dim)
    sel = SEL_PATTERN[: B * k]
    want = torch.stack([
        val[r // k] * st.q8_all[e, pos[r // k]].float() * st.scale8_all[e].float()
        for r, e in enumerate(sel)
    ])
    ws = torch.empty(64 * 16 * out_dim, device="cuda")
    sel_d = torch.tensor(sel, dtype=torch.int32, device="cuda")
    for S in _valid_splits(in_dim):
        out = hip.gemv_int8_moe(q8, s8, x.cuda(), sel_d, k, ws, EPI_PLAIN, S)
        assert out.shape == (B * k, out_dim) and out.dtype == torch.float32
        assert torch.equal(out.cpu(), want), (S, (out.cpu() - want).abs().max())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMV_SHAPES)
@pytest.mark.parametrize("B,k", GEMV_BK)
def test_gemv_int8_moe_random_vs_float64(hip, in_dim, out_dim, B, k):
    st, x, sel, ref, bound = _gemv_case(in_dim, out_dim, B, k)
    q8, s8 = _gpu_stack(st)
    ws = torch.empty(64 * 16 * out_dim, device="cuda")
    sel_d = torch.tensor(sel, dtype=torch.int32, device="cuda")
    xd = x.cuda()
    for S in _valid_splits(in_dim):
        out = hip.gemv_int8_moe(q8, s8, xd, sel_d, k, ws, EPI_PLAIN, S).cpu()
        again = hip.gemv_int8_moe(q8, s8, xd, sel_d, k, ws, EPI_PLAIN, S).cpu()
        assert torch.equal(out, again), f"splits={S}: not bit-reproducible"
        err = (out.double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"in={in_dim} out={out_dim} B={B} k={k} S={S}: max err/bound = {worst:.3f}")
        assert bool((err <= bound).all()), (S, worst)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMV_SHAPES)
@pytest.mark.parametrize("B,k", GEMV_BK)
def test_gemv_int8_moe_same_arithmetic_as_dense_kernel(hip, in_dim, out_dim, B, k):
    """Row r is bit-identical to gemv_int8 on that expert's slice at the same
    explicit split count: same inner loop, same scale fold, and a reduce whose
    order depends only on the split count."""
    st, x, sel, _, _ = _gemv_case(in_dim, out_dim, B, k)
    q8, s8 = _gpu_stack(st)
    ws = torch.empty(64 * 16 * out_dim, device="cuda")
    sel_d = torch.tensor(sel, dtype=torch.int32, device="cuda")
    xd = x.cuda()
    for S in _valid_splits(in_dim):
        S_dense = S if S > 0 else hip.gemv_int8_moe_splits(in_dim, out_dim, B * k)
        for epi in (EPI_PLAIN, EPI_SWIGLU):
            out = hip.gemv_int8_moe(q8, s8, xd, sel_d, k, ws, epi, S).clone()
            for r, e in enumerate(sel):
                t = r // k
                row = hip.gemv_int8(q8[e], s8[e], xd[t : t + 1].contiguous(), ws, None, epi, S_dense)
                assert torch.equal(out[r], row[0]), (S, epi, r, (out[r] - row[0]).abs().max())


@pytest.mark.gpu
@requires_gpu
def test_gemv_int8_moe_host_checks(hip):
    st, _ = _stacked(64, 64)
    q8, s8 = _gpu_stack(st)
    ws = torch.empty(64 * 16 * 64, device="cuda")

    def sel(n):
        return torch.tensor(SEL_PATTERN * 2, dtype=torch.int32, device="cuda")[:n].contiguous()

    with pytest.raises(RuntimeError):  # rows = 18 > 16
        hip.gemv_int8_moe(q8, s8, torch.zeros(9, 64, device="cuda"), sel(18), 2, ws, EPI_PLAIN)
    with pytest.raises(RuntimeError):  # sel length != B * k
        hip.gemv_int8_moe(q8, s8, torch.zeros(3, 64, device="cuda"), sel(5), 2, ws, EPI_PLAIN)
    q_bad = torch.zeros(E, 64, 68, dtype=torch.int8, device="cuda")
    s_bad = torch.ones(E, 68, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):  # out % 8 != 0
        hip.gemv_int8_moe(q_bad, s_bad, torch.zeros(1, 64, device="cuda"), sel(2), 2, ws, EPI_PLAIN)
    with pytest.raises(RuntimeError):  # scale8_all shape
        hip.gemv_int8_moe(q8, s8[:, :32].contiguous(), torch.zeros(1, 64, device="cuda"), sel(2), 2,
                          ws, EPI_PLAIN)
    with pytest.raises(RuntimeError):  # x dtype
        hip.gemv_int8_moe(q8, s8, torch.zeros(1, 64, device="cuda", dtype=torch.bfloat16), sel(2), 2,
                          ws, EPI_PLAIN)


@pytest.mark.gpu
@requires_gpu
def test_mixtral_int8_decode_workspace_holds_partials(hip, monkeypatch):
    """A real 8x7B int8 block: at every decode batch 1..8 the workspace the
    block sizes (64 * B * _max_gemv_out floats) is the buffer the routed gemvs
    write their split partials into — the op falls back to a buffer of its
    own when the workspace is too small, which would leave the NaN sentinel —
    and a decode step leaves the shared workspace where it was."""
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops.fused_decode import _get_ws
    from petals_amd.server.from_pretrained import build_empty_block, init_random_block_

    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    cfg = load_model_config("mixtral-8x7b")
    blk = build_empty_block(cfg, 0, "cuda:0", torch.bfloat16)
    init_random_block_(blk, cfg, 0)
    blk = blk.eval().optimize_for_inference(quant="int8")
    fp = blk._fast
    assert fp.graph_safe and fp.stacked_gu.quant == "int8"
    H, K, n_exp = cfg.hidden_size, fp.top_k, cfg.num_local_experts
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(3)
    with torch.inference_mode():
        for B in range(1, 9):
            numel = 64 * B * fp._max_gemv_out()
            sel = torch.randint(0, n_exp, (B * K,), device="cuda", generator=g).to(torch.int32)
            x = torch.randn(B, H, device="cuda", generator=g)
            ws = torch.full((numel,), float("nan"), device="cuda")
            act = fp.stacked_gu.moe_gemv(x, sel, K, ws, EPI_SWIGLU)
            assert not bool(torch.isnan(ws[0])), f"B={B}: gate+up partials did not fit the workspace"
            ws.fill_(float("nan"))
            down = fp.stacked_down.moe_gemv(act.contiguous(), sel, 1, ws, EPI_PLAIN)
            assert not bool(torch.isnan(ws[0])), f"B={B}: down partials did not fit the workspace"
            assert down.shape == (B * K, H) and bool(torch.isfinite(down).all())

            before = _get_ws(dev, "gemv", numel).data_ptr()
            ks, vs = blk.kv_cache_shape(B, 16)
            kv = (torch.zeros(ks, device="cuda", dtype=torch.bfloat16),
                  torch.zeros(vs, device="cuda", dtype=torch.bfloat16))
            h = torch.randn(B, 1, H, device="cuda", generator=g).to(torch.bfloat16)
            out = blk(h, kv_cache=kv, prefix_length=0)
            assert bool(torch.isfinite(out.float()).all())
            assert _get_ws(dev, "gemv", numel).data_ptr() == before, f"B={B}: workspace moved"


# ---------------------------------------------- GPU: grouped int8 moe_gemm


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
def test_moe_gemm_int8_one_hot_exact(hip, in_dim, out_dim):
    """One-hot X rows: C[pair] == bf16(v * q * scale) bit for bit (s8 staged
    as bf16 is exact, the MFMA sum has one nonzero term, the fp32 scale
    product is exact, one bf16 rounding)."""
    from petals_amd.ops.fused_moe import sort_pairs_by_expert

    st, _ = _stacked(in_dim, out_dim)
    q8, s8 = _gpu_stack(st)
    x, pos, val = _one_hot_rows(GEMM_T, in_dim)
    sel = _gemm_sel()
    sorted_pairs, tile_expert = sort_pairs_by_expert(sel.cuda(), E)
    out = hip.moe_gemm(None, None, None, x.cuda().bfloat16(), sorted_pairs, tile_expert,
                       GEMM_K, GEMM_T * GEMM_K, q8, s8).cpu()
    assert out.shape == (GEMM_T * GEMM_K, out_dim) and out.dtype == torch.bfloat16
    for pair, e in enumerate(sel.reshape(-1).tolist()):
        t = pair // GEMM_K
        want = (val[t] * st.q8_all[e, pos[t]].float() * st.scale8_all[e].float()).bfloat16()
        assert torch.equal(out[pair], want), (pair, e)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
def test_moe_gemm_int8_random_vs_float64(hip, in_dim, out_dim):
    from petals_amd.ops.fused_moe import _StackedExperts, sort_pairs_by_expert

    st, x, sel, ref, bound = _gemm_case(in_dim, out_dim)
    gst = _StackedExperts.__new__(_StackedExperts)
    gst.hip, gst.quant, gst.in_dim, gst.out_dim = hip, "int8", in_dim, out_dim
    gst.q8_all, gst.scale8_all = _gpu_stack(st)
    assert gst.gemm_ok
    sorted_pairs, tile_expert = sort_pairs_by_expert(sel.cuda(), E)
    xd = x.cuda()
    out = gst.moe_gemm(xd, sorted_pairs, tile_expert, GEMM_K, GEMM_T * GEMM_K).cpu()
    again = gst.moe_gemm(xd, sorted_pairs, tile_expert, GEMM_K, GEMM_T * GEMM_K).cpu()
    assert torch.equal(out, again), "not bit-reproducible"
    err = (out.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"in={in_dim} out={out_dim}: max err/bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst


@pytest.mark.gpu
@requires_gpu
def test_moe_gemm_old_signature_and_exclusive_weight_forms(hip):
    """bf16 and NF4 callers with the original positional signature still run
    and still match the dense product; mixing weight forms raises."""
    from petals_amd.ops.fused_moe import sort_pairs_by_expert

    in_dim, out_dim = 192, 384
    st, wts = _stacked(in_dim, out_dim)
    _, x, sel, _, _ = _gemm_case(in_dim, out_dim)
    xd = x.cuda()
    sorted_pairs, tile_expert = sort_pairs_by_expert(sel.cuda(), E)
    R = GEMM_T * GEMM_K
    wt_all = torch.stack(wts).cuda().contiguous()
    packed, absmax = zip(*[hip.nf4_quantize(w.cuda().contiguous()) for w in wts])
    packed_all, absmax_all = torch.stack(packed).contiguous(), torch.stack(absmax).contiguous()
    out_bf16 = hip.moe_gemm(wt_all, None, None, xd, sorted_pairs, tile_expert, GEMM_K, R)
    out_nf4 = hip.moe_gemm(None, packed_all, absmax_all, xd, sorted_pairs, tile_expert, GEMM_K, R)
    flat = sel.reshape(-1).tolist()
    for pair in range(0, R, 7):
        e, xr = flat[pair], xd[pair // GEMM_K].float()
        for got, dense in ((out_bf16, wt_all[e]), (out_nf4, hip.nf4_dequantize(packed_all[e], absmax_all[e]))):
            want = (xr @ dense.float()).bfloat16().float()
            assert torch.allclose(got[pair].float(), want, atol=0.02, rtol=0.02), (pair, e)
    q8, s8 = _gpu_stack(st)
    with pytest.raises(RuntimeError):
        hip.moe_gemm(wt_all, None, None, xd, sorted_pairs, tile_expert, GEMM_K, R, q8, s8)
    with pytest.raises(RuntimeError):
        hip.moe_gemm(None, packed_all, absmax_all, xd, sorted_pairs, tile_expert, GEMM_K, R, q8, s8)
    with pytest.raises(RuntimeError):
        hip.moe_gemm(None, None, None, xd, sorted_pairs, tile_expert, GEMM_K, R)


@pytest.mark.gpu
@requires_gpu
def test_swiglu_covers_more_than_8m_elements(hip):
    """The grouped prefill MLP runs swiglu over [T * k, I]: at Mixtral shapes
    that passes 4096 * 256 * 8 elements from ~300 tokens on, and every element
    must be written (ragged tail included)."""
    n = 4096 * 256 * 8 + 8 * 300 + 3
    g = torch.Generator(device="cuda").manual_seed(9)
    gate = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    up = torch.randn(n, device="cuda", generator=g).to(torch.bfloat16)
    y = hip.swiglu(gate, up)
    ref = torch.nn.functional.silu(gate.float()) * up.float()
    # one bf16 rounding of an fp32 product (the kernel's exp is the fast one)
    assert torch.allclose(y.float(), ref, rtol=2.0 ** -7, atol=1e-6), (y.float() - ref).abs().max()


# ------------------------------------------------------- GPU: block level


def _mixtral_cfg():
    from petals_amd.models.config_base import load_model_config

    cfg = load_model_config("test-mixtral")
    cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size = 512, 4, 2, 1024
    return cfg


def _int8_block(cfg):
    from petals_amd.models import get_model_block
    from petals_amd.server.from_pretrained import init_random_block_

    blk = get_model_block(cfg, 0)
    init_random_block_(blk, cfg, 0)
    return blk.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="int8")


@pytest.mark.gpu
@requires_gpu
def test_mixtral_int8_device_routed_matches_host_routed(hip, monkeypatch):
    """Same weights, same routing; the two paths differ only in fp32
    summation order inside the MLP and the block output is rounded once to
    bf16, so decode agrees to one bf16 rounding (rtol 2^-7, atol 1e-4) and
    the 5-token prefill to the dense-vs-fused prefill tolerance 2e-2."""
    cfg = _mixtral_cfg()
    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    blk_dev = _int8_block(cfg)
    monkeypatch.setenv("PETALS_AMD_MOE_INT8", "host")
    blk_host = _int8_block(cfg)
    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    assert blk_dev._fast.stacked_gu is not None and blk_dev._fast.stacked_gu.quant == "int8"
    assert blk_dev._fast.graph_safe
    assert blk_host._fast.stacked_gu is None and not blk_host._fast.graph_safe
    assert len(blk_host._fast.wgateup_e) == cfg.num_local_experts

    torch.manual_seed(6)
    S = 8
    x = (torch.randn(1, S, 512) * 0.5).cuda().bfloat16()
    ks, vs = blk_dev.kv_cache_shape(1, 16)
    caches = [
        (torch.zeros(ks, device="cuda", dtype=torch.bfloat16), torch.zeros(vs, device="cuda", dtype=torch.bfloat16))
        for _ in range(2)
    ]
    with torch.inference_mode():
        pre = [b(x[:, :5], kv_cache=c, prefix_length=0) for b, c in zip((blk_dev, blk_host), caches)]
        diff = (pre[0].float() - pre[1].float()).abs().max()
        print(f"prefill max |device - host| = {float(diff):.3e}")
        assert torch.allclose(pre[0].float(), pre[1].float(), atol=2e-2, rtol=2e-2), diff
        for t in range(5, S):
            d, h = [b(x[:, t : t + 1], kv_cache=c, prefix_length=t) for b, c in zip((blk_dev, blk_host), caches)]
            diff = (d.float() - h.float()).abs().max()
            print(f"decode t={t} max |device - host| = {float(diff):.3e}")
            assert torch.allclose(d.float(), h.float(), rtol=2.0 ** -7, atol=1e-4), (t, diff)


@pytest.mark.gpu
@requires_gpu
def test_mixtral_int8_decode_graph_capture(hip, monkeypatch):
    """int8 device-routed MoE decode is hipGraph-safe: capture one decode
    step, replay over new tokens, match the eager fused path."""
    from petals_amd.ops.fused_decode import DecodeContext
    from petals_amd.utils.graphs import GraphedCallable

    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    cfg = _mixtral_cfg()
    blk = _int8_block(cfg)
    assert blk._fast is not None and blk._fast.graph_safe, "device-routed int8 MoE must be graph-safe"
    blk2 = _int8_block(cfg)

    torch.manual_seed(7)
    ks, vs = blk.kv_cache_shape(1, 16)
    kg = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
    vg = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
    kg2, vg2 = kg.clone(), vg.clone()
    xs = [torch.randn(1, 1, 512, device="cuda", dtype=torch.bfloat16) * 0.5 for _ in range(4)]

    ctx = DecodeContext(torch.device("cuda"))
    ctx.set_position(0)
    h_in = torch.empty_like(xs[0])

    def step():
        return blk(h_in, kv_cache=(kg, vg), ctx=ctx)

    g = GraphedCallable(step, [])
    outs_graph, outs_eager = [], []
    for t, x in enumerate(xs):
        ctx.set_position(t)
        h_in.copy_(x)
        outs_graph.append(g.replay().clone())
        outs_eager.append(blk2(x, kv_cache=(kg2, vg2), prefix_length=t))
    for og, oe in zip(outs_graph, outs_eager):
        assert torch.allclose(og.float(), oe.float(), atol=1e-3, rtol=1e-3), (og - oe).abs().max()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("quant", ["int8", "nf4"])
def test_mixtral_hd64_serving_uses_span_graph(quant, monkeypatch):
    """One GPU server of quantized Mixtral blocks serving a client generate():
    decode goes through the whole-span hipGraph."""
    from petals_amd.dht.node import DHT
    from petals_amd.server import handler
    from petals_amd.server.server import Server
    from petals_amd.utils.auto_config import AutoDistributedModelForCausalLM

    monkeypatch.delenv("PETALS_AMD_MOE_INT8", raising=False)
    monkeypatch.delenv("PETALS_AMD_NO_GRAPHS", raising=False)
    calls = []
    real_step = handler._SpanDecodeGraph.step

    def counting_step(self, hidden_states, prefix_length):
        calls.append(prefix_length)
        return real_step(self, hidden_states, prefix_length)

    monkeypatch.setattr(handler._SpanDecodeGraph, "step", counting_step)

    preset, prefix = "test-mixtral-hd64", f"gpu-moe-{quant}"
    boot = DHT(host="127.0.0.1")
    server = Server(
        preset, initial_peers=[boot.listen_addr], host="127.0.0.1", device="cuda",
        torch_dtype="bfloat16", block_indices="0:4", dht_prefix=prefix, throughput=1.0,
        quant_type=quant,
    ).start()
    try:
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
