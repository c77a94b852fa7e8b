"""RMSNorm, LayerNorm, SwiGLU and prefill RoPE (ops/csrc/elementwise.hip) held
to float64 references computed once on the CPU from the bf16 values (and, for
RoPE, the fp32 tables) the kernels read.

Norms. Rows {1, 4, 5} cover both instantiations (T = 1024 threads for
rows <= 4, else 256); dims 8, 1004 (ragged tail of 4), 2048 and 2056 (one
T = 256 chunk exactly, and one element group past it), 8200 (past one
T = 1024 chunk) and 14336. Rows differ in scale; LayerNorm rows run through
(mean, std) = (0.3, 2), (16, 0.5), (64, 0.5), (128, 1) and a constant row.
Each input carries outliers that hold >= 1/3 of their row's (centred) sum of
squares each: one at the row's last element, or a pair on both sides of one
chunk boundary, so a kernel that loses either moves the whole row by > 15 %.

    f32 out:   |out - ref| <= TOL_N * (|x - mean| * inv * |w| + |b|)
    bf16 out:  the same + 2^-8 |ref|          (RMSNorm: no mean, no b)

TOL_N = 1.6e-6 is 4x the worst error, in that metric and over these very
cases, of an fp32 two-pass emulation (torch fp32: per-thread chunks, the wave
butterfly, the waves in order) against float64: 3.8e-7. The 4x is the margin
of tests/test_attention_numerics.py and covers summation order and rsqrtf.
Two things about that emulation, and so about the kernel, are not obvious:

* the metric is relative to |x - mean|, and an fp32 mean is only good to
  2^-24 |mean| (7.6e-6 at mean 128, next to elements 0.01 from it). The
  emulation is therefore the *corrected* two-pass: the second pass also sums
  c = x - mean, and d = sum(c) / dim, what the rounded mean missed, is taken
  off again: var = sum(c^2) / dim - d^2, y = (c - d) inv w + b. Without d the
  same emulation sits at 5.1e-5 in this metric, past the 2^-16 a sound fp32
  kernel may need, and an emulation of the one-pass form at 1.1e-3;
* under an element that sits on the mean the metric's floor is TOL_N |b|, and
  no fp32 sum places the mean better than about 2^-24 of the row's rms, so the
  test's biases keep |b| >= 0.25.

The one-pass E[x^2] - mean^2 this kernel used to compute misses the bound by
orders of magnitude on the offset rows (docs/KERNELS.md).

CPU mutants, each >= 2x the tolerance: the last element left out of the
moments, row 0's statistics used for row 1, the bias skipped, eps skipped on
the constant row.

SwiGLU. Gates +-{0, 1e-3, 20, 88, 100} among N(0, 3) data, n = 8 * 256 * k
and 8 * 256 * k + 3: `2^-8 |ref| + 2^-16 |ref| + 1e-30` (the bf16 half ulp;
the fast exponential's argument scaling, about |g| 2^-24 relative for
|g| <= 100), and no NaN or inf anywhere.

RoPE. One case past the 4096-block grid cap (1,088,000 work items), one with
b = 3 and different, non-monotonic positions per batch row including 0 and the
table's last row, at hd 64 and 128: `2^-8 |ref| + 2^-22 (|x1 c| + |x2 s|)`.
The inputs stay untouched. Mutant: batch row 0's positions used for all rows.

Every GPU call runs twice and must return the same bits.

Measured worst error / bound: see docs/KERNELS.md."""

import functools

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPS = 1e-5
TOL_N = 1.6e-6  # 4 x 3.8e-7, the fp32 emulation's worst (see above); recorded in docs/KERNELS.md
NORM_ROWS = (1, 4, 5)
NORM_DIMS = (8, 1004, 2048, 2056, 8200, 14336)
LN_KINDS = ((0.3, 2.0), (16.0, 0.5), (64.0, 0.5), (128.0, 1.0), "const")
CONST_VALUE = 3.0


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# -------------------------------------------------------------- norm inputs


def _threads(rows):
    return 1024 if rows <= 4 else 256


def _placements(rows, dim):
    """Outlier positions per variant: the last element; then one pair per
    boundary between two T * 8 chunks of the instantiation that runs."""
    chunk = 8 * _threads(rows)
    return [(dim - 1,)] + [(c - 1, c) for c in range(chunk, dim, chunk)]


def _plant(row, centre, places, recentre):
    """Overwrite row[places] with outliers that each hold >= 1/3 of the row's
    sum of squares about `centre` (1/2 for one, 0.36 each for a pair)."""
    rest = torch.ones(row.shape[0], dtype=torch.bool)
    rest[list(places)] = False
    s_rest = ((row[rest].double() - centre) ** 2).sum()
    factor = 1.0 if len(places) == 1 else 1.3
    for _ in range(20):  # bf16 is coarse next to a large centre: grow until the rounded values hold it
        amp = float(torch.sqrt(factor * s_rest))
        for n, p in enumerate(places):
            row[p] = torch.tensor(centre + (amp if n % 2 == 0 else -amp)).to(torch.bfloat16).float()
        centred = row.double() - (row.double().mean() if recentre else 0.0)
        if all(centred[p] ** 2 >= 0.34 * (centred ** 2).sum() for p in places):
            return
        factor *= 1.3
    raise AssertionError("could not plant the outliers")


@functools.lru_cache(maxsize=None)
def _norm_inputs(norm: str, rows: int, dim: int):
    """[(x bf16 [rows, dim], places, row kinds)] per variant, plus w and b.
    Built once on the CPU; never modified afterwards."""
    g = torch.Generator().manual_seed(100 * dim + rows + (0 if norm == "rms" else 7))
    w = torch.randn(dim, generator=g).to(torch.bfloat16)
    # |b| >= 0.25: the metric's floor under an element that sits on the row's
    # mean is TOL_N |b|, and no fp32 mean is better than 2^-24 of the row's rms
    z = torch.randn(dim, generator=g)
    b = (torch.where(z < 0, -1.0, 1.0) * (0.25 + z.abs())).to(torch.bfloat16)
    places_all = _placements(rows, dim)
    # LayerNorm: every row kind meets the last-element outlier in every row slot
    plan = [(places_all[0], ko) for ko in range(len(LN_KINDS) if norm == "layer" else 1)]
    plan += [(pl, n + 1) for n, pl in enumerate(places_all[1:])]
    variants = []
    for places, ko in plan:
        x = torch.empty(rows, dim)
        kinds = []
        for r in range(rows):
            z = torch.randn(dim, generator=g)
            if norm == "rms":
                kind = (0.0, 0.25 * 2.0 ** ((r + ko) % 5))
            else:
                kind = LN_KINDS[(r + ko) % len(LN_KINDS)]
            kinds.append(kind)
            if kind == "const":
                x[r] = CONST_VALUE
                continue
            x[r] = (kind[0] + kind[1] * z).to(torch.bfloat16).float()
            _plant(x[r], kind[0], places, recentre=norm == "layer")
        variants.append((x.to(torch.bfloat16), places, tuple(kinds)))
    return variants, w, b


def _ref64(norm, x, w, b, *, drop_last=False, stats_of_row0_for_row1=False, no_bias=False, no_eps=False):
    """float64 reference and the tolerance metric's scale. The keyword
    switches build the mutants."""
    x64, w64, b64 = x.double(), w.double(), b.double()
    m = x64[:, :-1] if drop_last else x64
    eps = 0.0 if no_eps else EPS
    if norm == "rms":
        mean = torch.zeros(x64.shape[0], 1, dtype=torch.float64)
        inv = 1.0 / torch.sqrt((m * m).mean(dim=1, keepdim=True) + eps)
    else:
        mean = m.mean(dim=1, keepdim=True)
        inv = 1.0 / torch.sqrt(((m - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    if stats_of_row0_for_row1 and x64.shape[0] > 1:
        mean, inv = mean.clone(), inv.clone()
        mean[1], inv[1] = mean[0], inv[0]
    out = (x64 - mean) * inv * w64
    scale = (x64 - mean).abs() * inv * w64.abs()
    if norm == "layer":
        scale = scale + b64.abs()
        if not no_bias:
            out = out + b64
    return out, scale


def _thread_tree_sum(v, T):
    """fp32 sum of each row of v in the kernel's order: every thread its 8
    elements of each T * 8 chunk, the 64-lane butterfly, the waves in order."""
    rows, dim = v.shape
    chunk = 8 * T
    n_chunks = -(-dim // chunk)
    v = torch.nn.functional.pad(v, (0, n_chunks * chunk - dim)).view(rows, n_chunks, T, 8)
    acc = torch.zeros(rows, T)
    for c in range(n_chunks):
        for j in range(8):
            acc = acc + v[:, c, :, j]
    acc = acc.view(rows, T // 64, 64)
    width = 64
    while width > 1:
        acc = acc[..., : width // 2] + acc[..., width // 2: width]
        width //= 2
    tot = torch.zeros(rows)
    for i in range(T // 64):
        tot = tot + acc[:, i, 0]
    return tot


def _emulate_fp32(norm, x, w, b):
    """Two-pass moments in fp32, then the kernel's output expression."""
    rows, dim = x.shape
    T = _threads(rows)
    xf, wf, bf = x.float(), w.float(), b.float()
    if norm == "rms":
        inv = torch.rsqrt(_thread_tree_sum(xf * xf, T) / dim + EPS).unsqueeze(1)
        return xf * inv * wf
    mean = (_thread_tree_sum(xf, T) / dim).unsqueeze(1)
    c = xf - mean
    d = _thread_tree_sum(c, T) / dim  # what the rounded mean missed
    inv = torch.rsqrt(_thread_tree_sum(c * c, T) / dim - d * d + EPS).unsqueeze(1)
    return (c - d.unsqueeze(1)) * inv * wf + bf


NORM_CASES = [(norm, rows, dim) for norm in ("rms", "layer") for rows in NORM_ROWS for dim in NORM_DIMS]


def _ratio(err, tol):
    return float((err / tol.clamp_min(1e-300)).max())


# ------------------------------------------------------------ norm CPU tests


@pytest.mark.parametrize("norm,rows,dim", NORM_CASES)
def test_norm_outliers_hold_a_third_and_move_the_row(norm, rows, dim):
    variants, w, b = _norm_inputs(norm, rows, dim)
    assert len(variants) >= 1 + len(_placements(rows, dim)) - 1
    for x, places, kinds in variants:
        x64 = x.double()
        for r, kind in enumerate(kinds):
            if kind == "const":
                assert bool((x64[r] == CONST_VALUE).all())
                continue
            centred = x64[r] - (0.0 if norm == "rms" else x64[r].mean())
            total = (centred ** 2).sum()
            keep = torch.ones(dim, dtype=torch.bool)
            for p in places:
                assert centred[p] ** 2 >= total / 3, (places, r, kind, float(centred[p] ** 2 / total))
                keep[:] = True
                keep[p] = False
                # the row without this outlier: every output moves by > 15 %
                lost = centred[keep] - (0.0 if norm == "rms" else centred[keep].mean())
                inv_full = 1.0 / torch.sqrt(total / dim + EPS)
                inv_lost = 1.0 / torch.sqrt((lost ** 2).sum() / dim + EPS)
                assert inv_lost / inv_full > 1.15, (places, r, kind)


@pytest.mark.parametrize("norm,rows,dim", NORM_CASES)
def test_norm_emulation_within_a_quarter_of_the_tolerance(norm, rows, dim):
    variants, w, b = _norm_inputs(norm, rows, dim)
    worst = 0.0
    for x, places, kinds in variants:
        ref, scale = _ref64(norm, x, w, b)
        err = (_emulate_fp32(norm, x, w, b).double() - ref).abs()
        worst = max(worst, _ratio(err, scale))
    print(f"{norm} rows={rows} dim={dim}: fp32 two-pass emulation worst err/scale = {worst:.3e}")
    assert worst <= TOL_N / 4, worst
    assert TOL_N / 4 <= 2.0 ** -16


@pytest.mark.parametrize("norm,rows,dim", NORM_CASES)
def test_norm_tolerance_rejects_mutants(norm, rows, dim):
    variants, w, b = _norm_inputs(norm, rows, dim)
    x, places, kinds = variants[0]  # the outlier sits on the last element
    ref, scale = _ref64(norm, x, w, b)
    tol = TOL_N * scale

    def breaks(**kw):
        bad, _ = _ref64(norm, x, w, b, **kw)
        err = (bad - ref).abs()
        return float("inf") if not bool(torch.isfinite(bad).all()) else _ratio(err, tol)

    if kinds != ("const",):
        assert breaks(drop_last=True) >= 2.0, "last element left out of the moments"
    if rows > 1:
        assert breaks(stats_of_row0_for_row1=True) >= 2.0, "row 0's statistics used for row 1"
    if norm == "layer":
        assert breaks(no_bias=True) >= 2.0, "bias skipped"
        const = [v for v in variants if "const" in v[2]]
        assert const, "every LayerNorm case has a constant row"
        for xc, _, kinds_c in const:
            ref_c, scale_c = _ref64(norm, xc, w, b)
            bad, _ = _ref64(norm, xc, w, b, no_eps=True)
            r = kinds_c.index("const")
            assert not bool(torch.isfinite(bad[r]).all()), "eps skipped on the constant row: 0 * inf"
            assert bool(torch.isfinite(ref_c).all()) and torch.equal(ref_c[r], b.double())


# ------------------------------------------------------------ norm GPU tests


def _run_twice(fn):
    a, b = fn(), fn()
    assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"
    return a


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("norm,rows,dim", NORM_CASES)
def test_norm_vs_float64(hip, norm, rows, dim):
    variants, w, b = _norm_inputs(norm, rows, dim)
    wg, bg = w.cuda(), b.cuda()
    worst = {"f32": 0.0, "bf16": 0.0}
    for n, (x, places, kinds) in enumerate(variants):
        ref, scale = _ref64(norm, x, w, b)
        xg = x.cuda()
        if norm == "rms":
            out32 = _run_twice(lambda: hip.rms_norm_f32out(xg, wg, EPS))
            out16 = _run_twice(lambda: hip.rms_norm(xg, wg, EPS))
        else:
            out32 = _run_twice(lambda: hip.layer_norm_f32out(xg, wg, bg, EPS))
            out16 = _run_twice(lambda: hip.layer_norm(xg, wg, bg, EPS))
        assert out32.dtype == torch.float32 and out32.shape == (rows, dim)
        assert out16.dtype == torch.bfloat16 and out16.shape == (rows, dim)
        for name, out, tol in (("f32", out32, TOL_N * scale),
                               ("bf16", out16, TOL_N * scale + 2.0 ** -8 * ref.abs())):
            out = out.cpu().double()
            assert bool(torch.isfinite(out).all()), (name, n, places, kinds)
            err = (out - ref).abs()
            ratio = _ratio(err, tol)
            print(f"{norm} rows={rows} dim={dim} variant {n} {places} {name}: err/bound {ratio:.4f}")
            worst[name] = max(worst[name], ratio)
            assert bool((err <= tol).all()), f"variant {n} outliers {places} kinds {kinds} {name}: err/bound {ratio:.3f}"
    print(f"{norm}_norm rows={rows} dim={dim} worst err/bound: f32out {worst['f32']:.4f}  bf16 {worst['bf16']:.4f}")


# ------------------------------------------------------------------- swiglu

SWIGLU_N = (8 * 256, 8 * 256 + 3, 8 * 256 * 3, 8 * 256 * 3 + 3)
SWIGLU_GATES = (0.0, 1e-3, 20.0, 88.0, 100.0)


@functools.lru_cache(maxsize=None)
def _swiglu_case(n: int):
    g = torch.Generator().manual_seed(n)
    gate = torch.randn(n, generator=g) * 3.0
    up = torch.randn(n, generator=g) * 3.0
    special = torch.tensor([s * v for v in SWIGLU_GATES for s in (1.0, -1.0)])
    # at the front, at the back (the ragged tail), and in the middle
    for start in (0, n - len(special), n // 2):
        gate[start:start + len(special)] = special
    gate, up = gate.to(torch.bfloat16), up.to(torch.bfloat16)
    g64, u64 = gate.double(), up.double()
    ref = g64 / (1.0 + torch.exp(-g64)) * u64
    return gate, up, ref, 2.0 ** -8 * ref.abs() + 2.0 ** -16 * ref.abs() + 1e-30


@pytest.mark.parametrize("n", SWIGLU_N)
def test_swiglu_reference_is_finite_and_bound_rejects_a_lost_tail(n):
    gate, up, ref, bound = _swiglu_case(n)
    assert bool(torch.isfinite(ref).all())
    for v in SWIGLU_GATES:
        assert bool((gate.float() == torch.tensor(v).to(torch.bfloat16).float()).any())
        assert bool((gate.float() == -torch.tensor(v).to(torch.bfloat16).float()).any())
    bad = ref.clone()
    bad[-3:] = 0.0  # the ragged tail left unwritten
    assert _ratio((bad - ref).abs(), bound) >= 2.0
    shifted = torch.roll(ref, 8)  # an 8-element group written one group late
    assert _ratio((shifted - ref).abs(), bound) >= 2.0


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("n", SWIGLU_N)
def test_swiglu_vs_float64(hip, n):
    gate, up, ref, bound = _swiglu_case(n)
    gg, ug = gate.cuda(), up.cuda()
    out = _run_twice(lambda: hip.swiglu(gg, ug))
    assert out.dtype == torch.bfloat16 and out.shape == (n,)
    out = out.cpu().double()
    assert bool(torch.isfinite(out).all()), "NaN or inf in the output"
    err = (out - ref).abs()
    ratio = _ratio(err, bound)
    print(f"swiglu n={n} worst err/bound: {ratio:.4f}")
    assert bool((err <= bound).all()), ratio


# --------------------------------------------------------------------- rope

# name -> (b, qh, kh, len, hd, table rows)
ROPE_CASES = {
    "past-grid-cap": (1, 8, 2, 1700, 128, 2048),
    "per-row-positions-hd64": (3, 4, 2, 9, 64, 64),
    "per-row-positions-hd128": (3, 4, 2, 9, 128, 64),
}


def _rope_ref(x, cos, sin, pos):
    """x [b, h, len, hd] bf16 -> float64 rotation from the fp32 tables, and
    |x1 c| + |x2 s| (the same for both halves)."""
    half = x.shape[-1] // 2
    c = cos.double()[pos][:, None, :, :half]  # [b, 1, len, half]
    s = sin.double()[pos][:, None, :, :half]
    x1, x2 = x.double()[..., :half], x.double()[..., half:]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return ref, 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag


@functools.lru_cache(maxsize=None)
def _rope_case(name: str):
    from petals_amd.ops import reference

    b, qh, kh, length, hd, max_pos = ROPE_CASES[name]
    g = torch.Generator().manual_seed(hd + length)
    q = torch.randn(b, qh, length, hd, generator=g).to(torch.bfloat16)
    k = torch.randn(b, kh, length, hd, generator=g).to(torch.bfloat16)
    cos, sin = reference.build_rope_cache(hd, max_pos)
    assert cos.dtype == torch.float32 and cos.shape == (max_pos, hd)
    if b == 1:
        pos = (torch.arange(length) + (max_pos - length)).unsqueeze(0)
    else:
        pos = torch.stack([torch.randperm(max_pos, generator=g)[:length] for _ in range(b)])
        pos[0, 3], pos[1, 0], pos[2, 5] = 0, max_pos - 1, 0
        pos[2, 1] = max_pos - 1
    refs = {"q": _rope_ref(q, cos, sin, pos), "k": _rope_ref(k, cos, sin, pos)}
    return q, k, cos, sin, pos, refs


def test_rope_cases_reach_the_paths_and_bound_rejects_row0_positions():
    b, qh, kh, length, hd, _ = ROPE_CASES["past-grid-cap"]
    assert b * (qh + kh) * length * (hd // 2) == 1_088_000 > 4096 * 256
    for name in ROPE_CASES:
        q, k, cos, sin, pos, refs = _rope_case(name)
        if pos.shape[0] == 1:
            continue
        assert int(pos.min()) == 0 and int(pos.max()) == cos.shape[0] - 1
        assert all(not torch.equal(pos[0], pos[r]) for r in range(1, pos.shape[0]))
        assert bool((pos[:, 1:] < pos[:, :-1]).any()), "non-monotonic"
        pos0 = pos[:1].expand_as(pos)
        for key, x in (("q", q), ("k", k)):
            bad, _ = _rope_ref(x, cos, sin, pos0)
            ref, bound = refs[key]
            assert _ratio((bad - ref).abs(), bound) >= 2.0, (name, key)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROPE_CASES))
def test_apply_rope_vs_float64(hip, name):
    q, k, cos, sin, pos, refs = _rope_case(name)
    qg, kg, cg, sg, pg = q.cuda(), k.cuda(), cos.cuda(), sin.cuda(), pos.cuda()
    outs = [hip.apply_rope(qg, kg, cg, sg, pg) for _ in range(2)]
    assert torch.equal(qg.cpu(), q) and torch.equal(kg.cpu(), k), "the op returns copies; the inputs stay"
    for key, first, second in (("q", outs[0][0], outs[1][0]), ("k", outs[0][1], outs[1][1])):
        assert first.dtype == torch.bfloat16
        assert torch.equal(first.view(torch.int16), second.view(torch.int16)), "two runs differ"
        ref, bound = refs[key]
        out = first.cpu().double()
        assert out.shape == ref.shape and bool(torch.isfinite(out).all())
        err = (out - ref).abs()
        ratio = _ratio(err, bound)
        print(f"apply_rope {name} {key} worst err/bound: {ratio:.4f}")
        assert bool((err <= bound).all()), (key, ratio)
