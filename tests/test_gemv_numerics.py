"""Dense decode GEMVs `gemv_bf16` (ops/csrc/gemv.hip) and `gemv_int8`
(ops/csrc/int8.hip) with the shared split-K reduce and its epilogues
(ops/csrc/gemv_reduce.h), held to float64 references computed once on the CPU
from the very bits the kernels read.

Shapes (in, out) are the smallest that reach each code path:

    (16, 8)       one live lane, one unrolled step
    (64, 64)      baseline
    (200, 520)    tail rows; second out-wave with one live lane
    (208, 524)    a partial lane with 4 live columns (out % 4 == 0 keeps every
                  vector access dword-aligned)
    (1000, 1536)  three out-waves
    (4360, 72)    more than 16 splits: a reduce group sums two members

Each op's host split rule is restated here (`_chunks`): bf16 aligns chunks to
16 rows and recomputes the split count, int8 uses ceil(in / splits) with chunks
of at least 128 rows. The raw-partials shape checks the restatement, and the
one-hot rows are chosen from it.

* one-hot x[b] = 1.5 e_i returns 1.5 W[i] (bf16) or 1.5 q[i] scale (int8, exact
  in fp32: 9-bit x 8-bit significands) bit for bit through the plain, raw,
  bf16, residual and bias epilogues. i runs over the first and last row of
  every chunk and the first row of every chunk's per-row tail loop, with a
  different i per batch row, for B in {1, 3, 5, 8};
* random x against float64 for every B in 1..8. fp32 accumulation of `in`
  terms over the splits: `in * 2^-23 * (|x| @ |W|)` (the bound of
  tests/test_nf4_gemv_wg.py), `+ 2^-23 |ref|` for the bias add, `+ 2^-8 |ref|`
  for a bf16 output (the bf16 half ulp), the SwiGLU bound of that file, and
  for GELU-tanh, with s the pre-activation sum and b its bound:

      1.13 b + 2^-20 |s| + 2^-22 |ref|

  |gelu'| <= 1.13 carries b through; the kernel evaluates 0.5 s (1 + tanhf(u))
  in fp32, where 1 + t cancels for negative s, so the absolute error of t
  (u's few roundings through tanh' <= 1 with |u| sech^2 u < 0.45, plus tanhf's
  own few ulp: below 2^-21 together) is multiplied by 0.5 |s|: 2^-22 |s|,
  taken 4x; the last term is the two fp32 roundings of the product;
* every call runs twice on a NaN-filled workspace of exactly the needed size
  and must return the same bits, and once with an empty workspace;
* CPU: an fp32 torch emulation of the chunked sum, the reduce order and the
  epilogue stays within 1/4 of every fp32 bound. The bf16 outputs are held to
  1x: their 2^-8 |ref| term is the rounding's exact worst case, which any
  correct rounding attains, and the fp32 part under it is the plain case;
* CPU: four corrupted references (last input row dropped, last chunk counted
  twice, batch row 0's x used for row 1, int8 scales shifted by one column)
  each break the plain bound by 2x or more;
* CPU: a model of the kernel driven by the mirror returns the one-hot values,
  and stops doing so on the chosen rows when a chunk's last row, a chunk's
  tail rows or the partial lane's columns are mis-indexed.

Measured worst error / bound: see docs/KERNELS.md."""

import functools
import math

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPI_RAW, EPI_PLAIN, EPI_BF16, EPI_RESIDUAL, EPI_SWIGLU, EPI_GELU = -1, 0, 1, 2, 3, 4
KINDS = ("bf16", "int8")
SHAPES = [(16, 8), (64, 64), (200, 520), (208, 524), (1000, 1536), (4360, 72)]
ONE_HOT_B = (1, 3, 5, 8)
B_MAX = 8
REDUCE_GROUPS = 16


def _splits_for(in_dim, out_dim):
    return (0, 1, 2, 5) + ((17,) if (in_dim, out_dim) == (4360, 72) else ())


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared inputs


def _cdiv(a, b):
    return -(-a // b)


def _chunks(kind, in_dim, out_dim, splits):
    """[(begin, end)] per split, as the host code of gemv_bf16 / gemv_int8
    cuts the input dimension; len() is the raw-partials row count."""
    out_waves = _cdiv(out_dim, 512)
    if kind == "bf16":
        n = splits if splits > 0 else max(1, min(_cdiv(768, out_waves), _cdiv(in_dim, 256)))
        per = (_cdiv(in_dim, n) + 15) // 16 * 16
        n = _cdiv(in_dim, per)
    else:
        n = splits if splits > 0 else _cdiv(1024, out_waves)
        n = max(1, min(n, _cdiv(in_dim, 128)))
        per = _cdiv(in_dim, n)
    return [(min(c * per, in_dim), min((c + 1) * per, in_dim)) for c in range(n)]


def _one_hot_rows(chunks):
    """First and last row of every chunk and the first row of its tail loop."""
    rows = set()
    for begin, end in chunks:
        if end > begin:
            rows.update((begin, end - 1))
            if (end - begin) % 16:
                rows.add(begin + (end - begin) // 16 * 16)
    return sorted(rows)


def _row_groups(rows, B):
    """Batches of B distinct rows (wrapping round at the end of the list)."""
    if len(rows) < B:
        rows = (rows * B)[:B]  # tiny shapes: repeats are unavoidable
    return [(rows[k:k + B] + rows[:B])[:B] for k in range(0, len(rows), B)]


@functools.lru_cache(maxsize=None)
def _data(in_dim: int, out_dim: int):
    """Built once per shape on the CPU; never modified afterwards."""
    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    w = (torch.randn(in_dim, out_dim, generator=g) * 0.05).to(torch.bfloat16)
    wf = w.float()
    scale = wf.abs().amax(dim=0).clamp_min(1e-8) / 127.0
    q = torch.round(wf / scale).clamp(-127, 127).to(torch.int8)
    s8 = scale.to(torch.bfloat16)
    x = torch.randn(B_MAX, in_dim, generator=g)
    # the last input row carries weight, so losing it is visible at in = 4360
    x[:, -1] = 2.5 * torch.where(x[:, -1] < 0, -1.0, 1.0)
    return dict(
        w=w, q=q, s8=s8, x=x,
        bias=(torch.randn(out_dim, generator=g) * 0.1).to(torch.bfloat16),
        residual=torch.randn(B_MAX, out_dim, generator=g).to(torch.bfloat16),
    )


def _w64(kind, d, s8=None):
    if kind == "bf16":
        return d["w"].double()
    return d["q"].double() * (d["s8"] if s8 is None else s8).double()  # exact


def _silu(t):
    return t / (1.0 + torch.exp(-t))


def _gelu(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t * t * t)))


@functools.lru_cache(maxsize=None)
def _cases(kind: str, in_dim: int, out_dim: int, B: int):
    """name -> (epilogue, residual?, bias?, float64 reference, bound, bf16 out?)"""
    d = _data(in_dim, out_dim)
    x = d["x"][:B]
    w64 = _w64(kind, d)
    half = out_dim // 2
    ref = x.double() @ w64
    bnd = in_dim * 2.0 ** -23 * (x.double().abs() @ w64.abs())
    refb = ref + d["bias"].double()
    bndb = bnd + 2.0 ** -23 * refb.abs()
    ref_res = ref + d["residual"][:B].double()

    def swiglu(r, b):
        gt, up, bg, bu = r[:, :half], r[:, half:], b[:, :half], b[:, half:]
        want = _silu(gt) * up
        return want, 1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * want.abs()

    def gelu(r, b):
        want = _gelu(r)
        return want, 1.13 * b + 2.0 ** -20 * r.abs() + 2.0 ** -22 * want.abs()

    return {
        "plain": (EPI_PLAIN, False, False, ref, bnd, False),
        "bf16": (EPI_BF16, False, False, ref, bnd + 2.0 ** -8 * ref.abs(), True),
        "residual": (EPI_RESIDUAL, True, False, ref_res, bnd + 2.0 ** -8 * ref_res.abs(), True),
        "swiglu": (EPI_SWIGLU, False, False) + swiglu(ref, bnd) + (False,),
        "gelu": (EPI_GELU, False, False) + gelu(ref, bnd) + (False,),
        "plain+bias": (EPI_PLAIN, False, True, refb, bndb, False),
        "swiglu+bias": (EPI_SWIGLU, False, True) + swiglu(refb, bndb) + (False,),
        "gelu+bias": (EPI_GELU, False, True) + gelu(refb, bndb) + (False,),
    }


# ------------------------------------------------------- fp32 kernel models


def _partials_fp32(kind, d, x, chunks):
    """One fp32 partial per chunk, the int8 scale folded in per partial."""
    w32 = d["w"].float() if kind == "bf16" else d["q"].float()
    parts = [x[:, b:e].float() @ w32[b:e] for b, e in chunks]
    if kind == "int8":
        parts = [p * d["s8"].float() for p in parts]
    return parts


def _reduce_fp32(parts):
    """gemv_reduce_kernel's order: group g sums partials g, g + 16, ...; then
    the 16 groups in index order."""
    total = torch.zeros_like(parts[0])
    for g in range(min(REDUCE_GROUPS, len(parts))):
        acc = torch.zeros_like(parts[0])
        for s in range(g, len(parts), REDUCE_GROUPS):
            acc = acc + parts[s]
        total = total + acc
    return total


def _epilogue_fp32(s, epi, residual, bias):
    if bias is not None:
        s = s + bias.float()
    if epi == EPI_PLAIN:
        return s
    if epi == EPI_BF16:
        return s.to(torch.bfloat16)
    if epi == EPI_RESIDUAL:
        return (residual.float() + s).to(torch.bfloat16)
    if epi == EPI_SWIGLU:
        half = s.shape[1] // 2
        return _silu(s[:, :half]) * s[:, half:]
    return _gelu(s)


# ------------------------------------------------------------------ CPU tests


@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_mirror_covers_the_input_and_reaches_the_paths(kind, in_dim, out_dim):
    for splits in _splits_for(in_dim, out_dim):
        chunks = _chunks(kind, in_dim, out_dim, splits)
        assert chunks[0][0] == 0 and chunks[-1][1] == in_dim
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert all(e > b for b, e in chunks), "no split may be empty"
        if kind == "bf16":
            assert all(b % 16 == 0 for b, e in chunks)
    if (in_dim, out_dim) == (4360, 72):
        for kind_, splits in (("bf16", 17), ("int8", 17), ("bf16", 0), ("int8", 0)):
            assert len(_chunks(kind_, in_dim, out_dim, splits)) > REDUCE_GROUPS
    if in_dim in (200, 1000):  # bf16: the last chunk has tail rows; int8: every chunk
        for splits in (1, 2):
            chunks = _chunks(kind, in_dim, out_dim, splits)
            assert all((e - b) % 16 for b, e in (chunks[-1:] if kind == "bf16" else chunks))


@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_emulation_within_a_quarter_of_every_bound(kind, in_dim, out_dim):
    d = _data(in_dim, out_dim)
    for B in (1, 5, 8):
        x = d["x"][:B]
        for splits in _splits_for(in_dim, out_dim):
            s = _reduce_fp32(_partials_fp32(kind, d, x, _chunks(kind, in_dim, out_dim, splits)))
            for name, (epi, use_res, use_bias, want, bound, is_bf16) in _cases(kind, in_dim, out_dim, B).items():
                out = _epilogue_fp32(s, epi, d["residual"][:B] if use_res else None, d["bias"] if use_bias else None)
                err = (out.double() - want).abs()
                limit = bound if is_bf16 else bound / 4
                ratio = (err / bound.clamp_min(1e-300)).max().item()
                assert (err <= limit).all(), (B, splits, name, ratio)


@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_plain_bound_rejects_corrupted_references(kind, in_dim, out_dim):
    d = _data(in_dim, out_dim)
    x64, w64 = d["x"].double(), _w64(kind, d)
    _, _, _, ref, bnd, _ = _cases(kind, in_dim, out_dim, B_MAX)["plain"]

    def worst(bad):
        return float(((bad - ref).abs() / bnd.clamp_min(1e-300)).max())

    assert worst(x64[:, :-1] @ w64[:-1]) >= 2.0, "last input row dropped"
    swapped = x64.clone()
    swapped[1] = x64[0]
    assert worst(swapped @ w64) >= 2.0, "batch row 0's x used for row 1"
    for splits in _splits_for(in_dim, out_dim):
        begin, end = _chunks(kind, in_dim, out_dim, splits)[-1]
        assert worst(ref + x64[:, begin:end] @ w64[begin:end]) >= 2.0, ("last chunk counted twice", splits)
    if kind == "int8" and out_dim > 1:
        assert worst(x64 @ _w64(kind, d, torch.roll(d["s8"], 1))) >= 2.0, "scales shifted by one column"


def _model_one_hot(w32, x, chunks, mutant=None):
    """The kernel as the mirror describes it: per chunk, 16-row unrolled steps
    then the per-row tail; the partial lane (out % 8 columns) on its own path."""
    out_dim = w32.shape[1]
    read = torch.zeros(w32.shape[0])  # 1 for every input row some chunk reads
    for begin, end in chunks:
        tail = begin + (end - begin) // 16 * 16
        read[begin:end] = 1.0
        if mutant == "chunk's last row lost":
            read[end - 1] = 0.0
        if mutant == "tail loop starts one row late" and tail < end:
            read[tail] = 0.0
    out = (x * read) @ w32  # one nonzero product per column: exact
    if mutant == "partial lane reads one column early" and out_dim % 8:
        first = out_dim // 8 * 8
        out[:, first:] = torch.roll(out, 1, dims=1)[:, first:]
    return out


@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_rows_expose_misindexing(kind, in_dim, out_dim):
    d = _data(in_dim, out_dim)
    w32 = _w64(kind, d).float()  # both forms are exact in fp32
    for splits in _splits_for(in_dim, out_dim):
        chunks = _chunks(kind, in_dim, out_dim, splits)
        rows = _one_hot_rows(chunks)
        has_tail = any((e - b) % 16 for b, e in chunks)
        for B in ONE_HOT_B:
            caught = {"chunk's last row lost": False}
            if has_tail:
                caught["tail loop starts one row late"] = False
            if out_dim % 8:
                caught["partial lane reads one column early"] = False
            for idx in _row_groups(rows, B):
                x = torch.zeros(B, in_dim)
                x[torch.arange(B), torch.tensor(idx)] = 1.5
                want = 1.5 * w32[torch.tensor(idx)]
                assert torch.equal(_model_one_hot(w32, x, chunks), want)
                for name in caught:
                    caught[name] |= not torch.equal(_model_one_hot(w32, x, chunks, name), want)
            assert all(caught.values()), (splits, B, caught)


# ------------------------------------------------------------------ GPU tests


def _gpu_weights(kind, d):
    return (d["w"].cuda(),) if kind == "bf16" else (d["q"].cuda(), d["s8"].cuda())


def _call(hip, kind, wg, x, ws, residual, epi, splits, bias):
    if kind == "bf16":
        return hip.gemv_bf16(wg[0], x, ws, residual, epi, splits, bias)
    return hip.gemv_int8(wg[0], wg[1], x, ws, residual, epi, splits, bias)


def _twice(hip, kind, wg, x, ws, epi, splits, residual=None, bias=None):
    """The call on a NaN-filled workspace, twice; asserts the two agree bit for
    bit and that the partials went into the caller's workspace."""
    outs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        outs.append(_call(hip, kind, wg, x, ws, residual, epi, splits, bias).clone())
        assert not bool(torch.isnan(ws[0])), "the partials must land in the caller's workspace"
    a, b = outs
    assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"
    return a


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_bit_exact(hip, kind, in_dim, out_dim):
    d = _data(in_dim, out_dim)
    wg = _gpu_weights(kind, d)
    # bf16: 1.5 W[i]; int8: 1.5 q[i] scale, 17 significand bits. Exact in fp32.
    want_all = (1.5 * _w64(kind, d)).float().cuda()
    assert torch.equal(want_all.double().cpu(), 1.5 * _w64(kind, d))
    bias_g, res_all = d["bias"].cuda(), d["residual"].cuda()
    empty = torch.empty(0, device="cuda")
    for splits in _splits_for(in_dim, out_dim):
        chunks = _chunks(kind, in_dim, out_dim, splits)
        n = len(chunks)
        rows = _one_hot_rows(chunks)
        for B in ONE_HOT_B:
            ws = torch.empty(n * B * out_dim, device="cuda")
            res_g = res_all[:B].contiguous()
            for k, idx in enumerate(_row_groups(rows, B)):
                x = torch.zeros(B, in_dim)
                x[torch.arange(B), torch.tensor(idx)] = 1.5
                x = x.cuda()
                want = want_all[torch.tensor(idx)]
                where = (splits, B, idx)
                out = _twice(hip, kind, wg, x, ws, EPI_PLAIN, splits)
                assert out.shape == (B, out_dim) and out.dtype == torch.float32
                assert torch.equal(out, want), (where, (out != want).nonzero()[:4])
                raw = _twice(hip, kind, wg, x, ws, EPI_RAW, splits)
                assert raw.shape == (n, B, out_dim), (raw.shape, n)
                assert torch.equal(raw.sum(0), want), where
                out = _twice(hip, kind, wg, x, ws, EPI_BF16, splits)
                assert out.dtype == torch.bfloat16 and torch.equal(out, want.to(torch.bfloat16)), where
                out = _twice(hip, kind, wg, x, ws, EPI_RESIDUAL, splits, residual=res_g)
                assert out.dtype == torch.bfloat16
                assert torch.equal(out, (res_g.float() + want).to(torch.bfloat16)), where
                out = _twice(hip, kind, wg, x, ws, EPI_PLAIN, splits, bias=bias_g)
                assert torch.equal(out, want + bias_g.float()), where
                if k == 0:
                    out = _call(hip, kind, wg, x, empty, None, EPI_PLAIN, splits, None)
                    assert torch.equal(out, want), ("empty workspace", where)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_random_vs_float64(hip, kind, in_dim, out_dim):
    d = _data(in_dim, out_dim)
    wg = _gpu_weights(kind, d)
    bias_g, res_all = d["bias"].cuda(), d["residual"].cuda()
    empty = torch.empty(0, device="cuda")
    worst = {}
    for B in range(1, B_MAX + 1):
        xg = d["x"][:B].cuda()
        res_g = res_all[:B].contiguous()
        cases = _cases(kind, in_dim, out_dim, B)
        for splits in _splits_for(in_dim, out_dim):
            n = len(_chunks(kind, in_dim, out_dim, splits))
            ws = torch.empty(n * B * out_dim, device="cuda")
            for name, (epi, use_res, use_bias, want, bound, is_bf16) in cases.items():
                r, bias = (res_g if use_res else None), (bias_g if use_bias else None)
                out = _twice(hip, kind, wg, xg, ws, epi, splits, r, bias)
                if name == "plain":
                    again = _call(hip, kind, wg, xg, empty, None, epi, splits, None)
                    assert torch.equal(out, again), ("empty workspace", B, splits)
                assert out.dtype == (torch.bfloat16 if is_bf16 else torch.float32)
                out = out.cpu().double()
                assert out.shape == want.shape and torch.isfinite(out).all()
                err = (out - want).abs()
                ratio = (err / bound.clamp_min(1e-300)).max().item()
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert (err <= bound).all(), f"B={B} splits={splits} {name}: err/bound {ratio:.3f}"
    print(f"gemv_{kind} {in_dim}x{out_dim} worst err/bound: "
          + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
