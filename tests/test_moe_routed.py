"""The routed decode GEMVs `gemv_bf16_moe` and `gemv_nf4_moe` and the bf16 and
NF4 modes of the grouped prefill GEMM `moe_gemm` (ops/csrc/moe.hip), judged
the way tests/test_moe_int8.py judges their int8 siblings: float64 references
computed once on the CPU from the very bits the kernels read (bf16 weights;
NF4 codes and bf16 absmax from ops/nf4.py::quantize), E = 4 experts whose
magnitudes differ, that file's selection pattern and (B, k) list.

* routed GEMV, one-hot x[b] = 1.5 e_i: row r returns 1.5 W[sel[r]][i] (bf16)
  or levels * (1.5 absmax) in fp32 (NF4: 1.5 * bf16 is exact, the product
  rounds once) bit for bit. i differs per token and runs over the first and
  last row of every split's chunk and the first row of its per-row tail loop;
  the split rule of each op is restated in `_chunks`;
* routed GEMV, random x: `|out - ref| <= in * 2^-23 * (|x| @ |W[e]|)`, and the
  SwiGLU bound of tests/test_nf4_gemv_wg.py for the fused epilogue, at splits
  {0, 1, 2, 5}, with k_per_tok = 2 and 1 (the down projection's form);
* moe_gemm, every pair: `2^-8 |ref| + in * 2^-23 * (|X| @ |W|)`; the NF4 mode
  stages bf16(LUT * absmax), so its reference weight is
  ops/nf4.py::dequantize bit for bit; one-hot X rows return
  bf16(v * W[e][pos]) bit for bit; the selection has an empty expert and one
  with more than a tile of pairs;
* every call runs twice (the GEMVs on a NaN-filled workspace of exactly the
  needed size) with bit-identical results, and once with an empty workspace;
* CPU: references corrupted three ways (expert id ignored, token r instead
  of r / k, expert 0's absmax with this expert's codes) break those bounds by
  2x or more.

Every expert id is in range: the kernels do not check ids.

Measured worst error / bound: see docs/KERNELS.md."""

import functools

import pytest
import torch

from petals_amd.ops import nf4 as nf4_ref

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPI_PLAIN, EPI_SWIGLU = 0, 3
E = 4
GEMV_SHAPES = {
    "bf16": [(64, 64), (200, 520), (208, 524), (1024, 2048)],
    "nf4": [(64, 64), (200, 576), (1024, 2048)],
}
GEMV_CASES = [(fmt, i, o) for fmt, shapes in GEMV_SHAPES.items() for i, o in shapes]
GEMV_BK = [(1, 2), (3, 2), (8, 2), (5, 1)]
GEMV_SPLITS = [0, 1, 2, 5]
# distinct and repeated experts, every id in [0, E)
SEL_PATTERN = [1, 3, 0, 2, 2, 1, 3, 3, 0, 1, 2, 0, 3, 1, 0, 2]
GEMM_SHAPES = [(64, 128), (64, 384), (192, 128), (192, 384)]
GEMM_T, GEMM_K = 40, 2
FORMATS = ("bf16", "nf4")


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared inputs


def _cdiv(a, b):
    return -(-a // b)


def _chunks(fmt, in_dim, out_dim, rows, splits):
    """[(begin, end)] per split, as gemv_bf16_moe / gemv_nf4_moe cut the input."""
    if fmt == "bf16":
        wgs, target, min_chunk = _cdiv(out_dim, 512) * rows, 768, 256
    else:
        wgs, target, min_chunk = _cdiv(out_dim, 1024) * rows, 1536, 32
    n = splits if splits > 0 else _cdiv(target, wgs)
    n = max(1, min(n, _cdiv(in_dim, min_chunk)))
    per = _cdiv(in_dim, n)
    return [(min(c * per, in_dim), min((c + 1) * per, in_dim)) for c in range(n)]


def _one_hot_rows(chunks):
    rows = set()
    for begin, end in chunks:
        if end > begin:
            rows.update((begin, end - 1))
            if (end - begin) % 16:
                rows.add(begin + (end - begin) // 16 * 16)
    return sorted(rows)


@functools.lru_cache(maxsize=None)
def _experts(fmt: str, in_dim: int, out_dim: int):
    """CPU stack for (in, out); expert magnitudes differ, so every expert has
    its own weights and its own absmax. Never modified afterwards."""
    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    wts = [(torch.randn(in_dim, out_dim, generator=g) * 0.03 * (e + 1)).to(torch.bfloat16) for e in range(E)]
    if fmt == "bf16":
        w_all = torch.stack(wts).contiguous()
        return dict(w_all=w_all, w64=w_all.double(), gemm64=w_all.double(), one_hot=1.5 * w_all.float())
    packed, absmax = zip(*[nf4_ref.quantize(w) for w in wts])
    packed_all, absmax_all = torch.stack(packed).contiguous(), torch.stack(absmax).contiguous()
    idx = torch.empty(E, in_dim, out_dim, dtype=torch.long)
    idx[..., 0::2] = (packed_all & 0xF).long()
    idx[..., 1::2] = (packed_all >> 4).long()
    levels = nf4_ref.NF4_LEVELS[idx]  # f32 [E, in, out]
    scale = absmax_all.float().repeat_interleave(64, dim=2)
    deq = torch.stack([nf4_ref.dequantize(p, a) for p, a in zip(packed, absmax)])  # bf16, as moe_gemm stages
    return dict(
        packed_all=packed_all, absmax_all=absmax_all, levels=levels, scale=scale,
        w64=levels.double() * scale.double(),  # the GEMV's weights, exact: 24-bit x 8-bit significands
        gemm64=deq.double(), gemm_bf16=deq,
        one_hot=levels * (1.5 * scale),  # 1.5 * bf16 is exact; the product rounds once, as the kernel's fma
    )


def _routed_ref(w64, x64, sel, k, *, ignore_expert=False, token_is_row=False, absmax0=None):
    """float64 out[r] = x[r // k] @ W[sel[r]] and the |x| @ |W| magnitude.
    The keyword switches build the corrupted references; absmax0 is a
    [E, in, out] float64 stack of this expert's codes under expert 0's absmax."""
    n_tok = x64.shape[0]
    rows, mags = [], []
    for r, e in enumerate(sel):
        w = w64[0 if ignore_expert else e]
        if absmax0 is not None:
            w = absmax0[e]
        xr = x64[(r % n_tok) if token_is_row else (r // k)]
        rows.append(xr @ w)
        mags.append(xr.abs() @ w.abs())
    return torch.stack(rows), torch.stack(mags)


def _absmax0_stack(ex, gemm: bool):
    """Expert e's codes decoded with expert 0's absmax, in the GEMV's (fp32
    product) or the GEMM's (bf16-staged) form."""
    prod = ex["levels"] * ex["scale"][0]
    return (prod.to(torch.bfloat16) if gemm else prod).double()


@functools.lru_cache(maxsize=None)
def _gemv_case(fmt: str, in_dim: int, out_dim: int, B: int, k: int):
    ex = _experts(fmt, in_dim, out_dim)
    g = torch.Generator().manual_seed(7 + 31 * B + k)
    x = torch.randn(B, in_dim, generator=g)
    sel = SEL_PATTERN[: B * k]
    ref, mag = _routed_ref(ex["w64"], x.double(), sel, k)
    return ex, x, sel, ref, in_dim * 2.0 ** -23 * mag


def _gemm_sel() -> torch.Tensor:
    """[T, K] expert ids: expert 2 empty, expert 1 over-full (two MT tiles)."""
    g = torch.Generator().manual_seed(5)
    sel = torch.tensor([0, 1, 3])[torch.randint(0, 3, (GEMM_T, GEMM_K), generator=g)]
    sel[:36, 0] = 1
    return sel


@functools.lru_cache(maxsize=None)
def _gemm_case(fmt: str, in_dim: int, out_dim: int):
    ex = _experts(fmt, in_dim, out_dim)
    g = torch.Generator().manual_seed(3 + in_dim + out_dim)
    x = (torch.randn(GEMM_T, in_dim, generator=g) * 0.5).to(torch.bfloat16)
    sel = _gemm_sel()
    ref, mag = _routed_ref(ex["gemm64"], x.double(), sel.reshape(-1).tolist(), GEMM_K)
    return ex, x, sel, ref, 2.0 ** -8 * ref.abs() + in_dim * 2.0 ** -23 * mag


def _gemm_one_hot(n: int, in_dim: int):
    """Row t is zero except one entry: 1.0 or -2.0 at a position that differs
    per row and reaches the first and last input rows."""
    x = torch.zeros(n, in_dim)
    pos, val = [], []
    for t in range(n):
        p = (in_dim - 1 - 5 * t) % in_dim if t % 2 == 0 else (7 * t + 3) % in_dim
        if t == 1:
            p = 0
        v = -2.0 if t % 3 == 1 else 1.0
        x[t, p] = v
        pos.append(p)
        val.append(v)
    return x, pos, val


def _silu(t):
    return t / (1.0 + torch.exp(-t))


def _swiglu_ref(ref, bound):
    half = ref.shape[1] // 2
    gt, up, bg, bu = ref[:, :half], ref[:, half:], bound[:, :half], bound[:, half:]
    want = _silu(gt) * up
    return want, 1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * want.abs()


# ---------------------------------------------------------------- CPU tests


def _worst_break(corrupt, ref, bound) -> float:
    return float(((corrupt - ref).abs() / bound.clamp_min(1e-300)).max())


def _corruptions(fmt, ex, gemm):
    out = [("expert id ignored", dict(ignore_expert=True)), ("token index r", dict(token_is_row=True))]
    if fmt == "nf4":
        out.append(("absmax of expert 0", dict(absmax0=_absmax0_stack(ex, gemm))))
    return out


@pytest.mark.parametrize("fmt,in_dim,out_dim", GEMV_CASES)
@pytest.mark.parametrize("B,k", [(3, 2), (8, 2)])
def test_reference_catches_corruptions_gemv(fmt, in_dim, out_dim, B, k):
    ex, x, sel, ref, bound = _gemv_case(fmt, in_dim, out_dim, B, k)
    for name, kw in _corruptions(fmt, ex, gemm=False):
        bad, _ = _routed_ref(ex["w64"], x.double(), sel, k, **kw)
        assert _worst_break(bad, ref, bound) >= 2.0, name
        want, sw_bound = _swiglu_ref(ref, bound)
        assert _worst_break(_swiglu_ref(bad, bound)[0], want, sw_bound) >= 2.0, (name, "swiglu")


@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_catches_corruptions_gemm(fmt, in_dim, out_dim):
    ex, x, sel, ref, bound = _gemm_case(fmt, in_dim, out_dim)
    counts = torch.bincount(sel.reshape(-1), minlength=E).tolist()
    assert counts[2] == 0 and counts[1] > 32, "an empty expert and one with more than a tile of pairs"
    for name, kw in _corruptions(fmt, ex, gemm=True):
        bad, _ = _routed_ref(ex["gemm64"], x.double(), sel.reshape(-1).tolist(), GEMM_K, **kw)
        assert _worst_break(bad, ref, bound) >= 2.0, name


@pytest.mark.parametrize("fmt,in_dim,out_dim", GEMV_CASES)
def test_mirror_covers_the_input_and_one_hot_forms_are_exact(fmt, in_dim, out_dim):
    for rows in (2, 5, 16):
        for splits in GEMV_SPLITS:
            chunks = _chunks(fmt, in_dim, out_dim, rows, splits)
            assert chunks[0][0] == 0 and chunks[-1][1] == in_dim
            assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
            assert all(e > b for b, e in chunks), "no split may be empty"
    ex = _experts(fmt, in_dim, out_dim)
    exact = 1.5 * ex["w64"]
    if fmt == "bf16":
        assert torch.equal(ex["one_hot"].double(), exact), "1.5 W[e][i] is an fp32 number"
    else:  # one fp32 rounding of the exact product
        assert ((ex["one_hot"].double() - exact).abs() <= 2.0 ** -24 * exact.abs()).all()
        # the GEMM stages exactly what ops/nf4.py::dequantize returns
        assert torch.equal(ex["gemm_bf16"], (ex["levels"] * ex["scale"]).to(torch.bfloat16))


# ----------------------------------------------------- GPU: the routed GEMVs


def _gpu_stack(fmt, ex):
    return (ex["w_all"].cuda(),) if fmt == "bf16" else (ex["packed_all"].cuda(), ex["absmax_all"].cuda())


def _gemv(hip, fmt, wg, x, sel_d, k, ws, epi, splits):
    if fmt == "bf16":
        return hip.gemv_bf16_moe(wg[0], x, sel_d, k, ws, epi, splits)
    return hip.gemv_nf4_moe(wg[0], wg[1], x, sel_d, k, ws, epi, splits)


def _twice(hip, fmt, wg, x, sel_d, k, ws, epi, splits):
    """The call on a NaN-filled workspace, twice; asserts the two agree bit for
    bit and that the partials went into the caller's workspace."""
    outs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        outs.append(_gemv(hip, fmt, wg, x, sel_d, k, ws, epi, splits).clone())
        assert not bool(torch.isnan(ws[0])), "the partials must land in the caller's workspace"
    a, b = outs
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"
    return a


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("fmt,in_dim,out_dim", GEMV_CASES)
@pytest.mark.parametrize("B,k", GEMV_BK)
def test_routed_gemv_one_hot_bit_exact(hip, fmt, in_dim, out_dim, B, k):
    ex = _experts(fmt, in_dim, out_dim)
    wg = _gpu_stack(fmt, ex)
    sel = SEL_PATTERN[: B * k]
    rows = B * k
    sel_d = torch.tensor(sel, dtype=torch.int32, device="cuda")
    sel_t = torch.tensor(sel)
    tok = torch.arange(rows) // k
    empty = torch.empty(0, device="cuda")
    for splits in GEMV_SPLITS:
        chunks = _chunks(fmt, in_dim, out_dim, rows, splits)
        ws = torch.empty(len(chunks) * rows * out_dim, device="cuda")
        hot = _one_hot_rows(chunks)
        if len(hot) < B:
            hot = (hot * B)[:B]
        for g in range(0, len(hot), B):
            idx = torch.tensor((hot[g:g + B] + hot[:B])[:B])
            x = torch.zeros(B, in_dim)
            x[torch.arange(B), idx] = 1.5
            want = ex["one_hot"][sel_t, idx[tok]]  # [rows, out]
            out = _twice(hip, fmt, wg, x.cuda(), sel_d, k, ws, EPI_PLAIN, splits).cpu()
            assert out.shape == (rows, out_dim)
            assert torch.equal(out, want), (splits, idx.tolist(), (out != want).nonzero()[:4])
            if g == 0:
                out = _gemv(hip, fmt, wg, x.cuda(), sel_d, k, empty, EPI_PLAIN, splits).cpu()
                assert torch.equal(out, want), ("empty workspace", splits)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("fmt,in_dim,out_dim", GEMV_CASES)
@pytest.mark.parametrize("B,k", GEMV_BK)
def test_routed_gemv_random_vs_float64(hip, fmt, in_dim, out_dim, B, k):
    ex, x, sel, ref, bound = _gemv_case(fmt, in_dim, out_dim, B, k)
    wg = _gpu_stack(fmt, ex)
    rows = B * k
    sel_d = torch.tensor(sel, dtype=torch.int32, device="cuda")
    xd = x.cuda()
    empty = torch.empty(0, device="cuda")
    cases = {"plain": (EPI_PLAIN, ref, bound), "swiglu": (EPI_SWIGLU,) + _swiglu_ref(ref, bound)}
    worst = {}
    for splits in GEMV_SPLITS:
        n = len(_chunks(fmt, in_dim, out_dim, rows, splits))
        ws = torch.empty(n * rows * out_dim, device="cuda")
        for name, (epi, want, bnd) in cases.items():
            out = _twice(hip, fmt, wg, xd, sel_d, k, ws, epi, splits)
            again = _gemv(hip, fmt, wg, xd, sel_d, k, empty, epi, splits)
            assert torch.equal(out, again), ("empty workspace", splits, name)
            out = out.cpu().double()
            assert out.shape == want.shape and torch.isfinite(out).all()
            err = (out - want).abs()
            ratio = float((err / bnd.clamp_min(1e-300)).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert bool((err <= bnd).all()), f"splits={splits} {name}: err/bound {ratio:.3f}"
    print(f"gemv_{fmt}_moe {in_dim}x{out_dim} B={B} k={k} worst err/bound: "
          + "  ".join(f"{n} {v:.4f}" for n, v in worst.items()))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_routed_gemv_has_no_raw_mode(hip, fmt):
    """The shared reduce has no raw epilogue; the routed ops must refuse one
    on the host, as gemv_int8_moe does."""
    ex = _experts(fmt, 64, 64)
    wg = _gpu_stack(fmt, ex)
    sel_d = torch.tensor(SEL_PATTERN[:2], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        _gemv(hip, fmt, wg, torch.zeros(1, 64, device="cuda"), sel_d, 2, torch.empty(0, device="cuda"), -1, 0)


# ------------------------------------------------- GPU: grouped moe_gemm


def _moe_gemm(hip, fmt, wg, x, sorted_pairs, tile_expert):
    R = GEMM_T * GEMM_K
    if fmt == "bf16":
        return hip.moe_gemm(wg[0], None, None, x, sorted_pairs, tile_expert, GEMM_K, R)
    return hip.moe_gemm(None, wg[0], wg[1], x, sorted_pairs, tile_expert, GEMM_K, R)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_moe_gemm_one_hot_exact(hip, fmt, in_dim, out_dim):
    """One-hot X rows: C[pair] == bf16(v * W[e][pos]) bit for bit (the MFMA sum
    has one nonzero term, v is a power of two, one bf16 rounding of a bf16)."""
    from petals_amd.ops.fused_moe import sort_pairs_by_expert

    ex = _experts(fmt, in_dim, out_dim)
    wg = _gpu_stack(fmt, ex)
    w_bf16 = ex["w_all"] if fmt == "bf16" else ex["gemm_bf16"]
    x, pos, val = _gemm_one_hot(GEMM_T, in_dim)
    sel = _gemm_sel()
    sorted_pairs, tile_expert = sort_pairs_by_expert(sel.cuda(), E)
    xd = x.cuda().bfloat16()
    out = _moe_gemm(hip, fmt, wg, xd, sorted_pairs, tile_expert)
    again = _moe_gemm(hip, fmt, wg, xd, sorted_pairs, tile_expert)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two runs differ"
    out = out.cpu()
    assert out.shape == (GEMM_T * GEMM_K, out_dim) and out.dtype == torch.bfloat16
    for pair, e in enumerate(sel.reshape(-1).tolist()):
        t = pair // GEMM_K
        want = (val[t] * w_bf16[e, pos[t]].float()).bfloat16()
        assert torch.equal(out[pair], want), (pair, e)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("in_dim,out_dim", GEMM_SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_moe_gemm_random_vs_float64_every_pair(hip, fmt, in_dim, out_dim):
    from petals_amd.ops.fused_moe import sort_pairs_by_expert

    ex, x, sel, ref, bound = _gemm_case(fmt, in_dim, out_dim)
    wg = _gpu_stack(fmt, ex)
    sorted_pairs, tile_expert = sort_pairs_by_expert(sel.cuda(), E)
    xd = x.cuda()
    out = _moe_gemm(hip, fmt, wg, xd, sorted_pairs, tile_expert)
    again = _moe_gemm(hip, fmt, wg, xd, sorted_pairs, tile_expert)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "two runs differ"
    out = out.cpu().double()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    err = (out - ref).abs()  # every pair, every column
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"moe_gemm {fmt} in={in_dim} out={out_dim}: max err/bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
