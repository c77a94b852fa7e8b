"""gemv_nf4_wg_kernel: the NF4 decode GEMV whose workgroup is 4, 8 or 16
waves that split K among them and combine in LDS (ops/csrc/nf4.hip,
`gemv_nf4(..., wg_waves, nt)`), and the `(wg_waves, splits, nt)` tuning of
_FastWeight.

The kernel keeps the one-wave kernel's K chunks and mirrors the reduce's
grouping (workgroup g = reduce group g, wave w = chunk g + 16 w), so for a
given split count it must return the one-wave kernel's bits. The split rule is
restated here (`_sub_chunks`) so the tests know every wave's rows; the raw
epilogue's row count checks the restatement.

* bit for bit the one-wave kernel's output on the same inputs, through every
  epilogue, for every (wg_waves, splits, nt, B), including a shape with 128
  chunks (8 chunks per group; 4 waves cannot hold it and must fall back);
* one-hot x = 1.5 e_i reproduces row i bit for bit: one product per column
  rounds once, every other row contributes an exact zero. i runs over the
  first and last row of every wave's chunk and the tail rows;
* random x against float64 over the exactly decoded weights, within
  `in * 2^-23 * (|x| @ |W|)` (the bound of tests/test_mxfp4.py), through the
  plain, bias, residual-bf16 and SwiGLU epilogues, for the old kernel too;
* every call runs twice on a NaN-filled workspace: bit-identical results;
* a CPU self-check that the bound passes an fp32 emulation of the kernel's
  summation order and rejects, by 2x or more, a reference that drops or
  doubles any one wave's chunk;
* a Llama block on seeded `(wg_waves, splits, nt)`: eager equals graph replay
  bit for bit and equals the block on the old kernel bit for bit (the issue's
  2e-2 included).

Measured worst error / bound over the random cases: see docs/KERNELS.md."""

import functools

import pytest
import torch

from petals_amd.ops import nf4 as nf4_ref

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPI_RAW, EPI_PLAIN, EPI_RESIDUAL, EPI_SWIGLU = -1, 0, 2, 3

# (in, out): most waves and lanes idle; ragged second column tile; 13 unroll
# blocks, uneven over 4 and 8 waves; tail rows; several tiles and splits
SHAPES = [(32, 64), (64, 576), (208, 1024), (200, 512), (1024, 2048)]
WAVES = (4, 8)
SPLITS = (0, 1, 2, 5)
BATCHES = (1, 3, 4)
B_MAX = max(BATCHES)


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


# ------------------------------------------------------------ shared fixtures


@functools.lru_cache(maxsize=None)
def _weights(in_dim: int, out_dim: int):
    """Quantized once per shape on the CPU; never modified afterwards."""
    g = torch.Generator().manual_seed(1000 * in_dim + out_dim)
    w = (torch.randn(in_dim, out_dim, generator=g) * 0.05).to(torch.bfloat16)
    packed, absmax = nf4_ref.quantize(w)
    idx = torch.empty(in_dim, out_dim, dtype=torch.long)
    idx[:, 0::2] = (packed & 0xF).long()
    idx[:, 1::2] = (packed >> 4).long()
    levels = nf4_ref.NF4_LEVELS[idx]  # f32 [in, out]
    scale = absmax.to(torch.float32).repeat_interleave(64, dim=1)
    return dict(
        packed=packed, absmax=absmax, absmax_t=absmax.t().contiguous(),
        levels=levels, scale=scale,
        deq64=levels.double() * scale.double(),  # exact: 24-bit x 8-bit significands
        x=torch.randn(B_MAX, in_dim, generator=g),
        bias=(torch.randn(out_dim, generator=g) * 0.1).to(torch.bfloat16),
        residual=torch.randn(B_MAX, out_dim, generator=g).to(torch.bfloat16),
    )


def _sub_chunks(in_dim: int, out_dim: int, waves: int, splits: int):
    """The host split rule of gemv_nf4 and the wg kernel's assignment:
    (partial rows, [[(begin, end) per wave] per workgroup]). The chunks are the
    one-wave kernel's; workgroup g holds chunks g, g + 16, g + 32, ..."""
    out_tiles = -(-out_dim // 512)
    n = splits if splits > 0 else -(-1536 // out_tiles)
    n = max(1, min(n, -(-in_dim // 32)))
    per_split = (-(-in_dim // n) + 15) // 16 * 16
    n = -(-in_dim // per_split)
    assert n <= 16 * waves, "the test shapes fit the wave counts they are run at"
    groups = []
    for g in range(min(n, 16)):
        row = []
        for w in range(waves):
            c = g + 16 * w
            begin = c * per_split if c < n else in_dim
            row.append((begin, min(begin + per_split, in_dim)))
        groups.append(row)
    return min(n, 16), groups


def _bound(x, wdeq):
    return x.shape[1] * 2.0 ** -23 * (x.double().abs() @ wdeq.abs())


def _silu(t):
    return t / (1.0 + torch.exp(-t))


def _emulate_fp32(x, w, chunks):
    """fp32 partial sums in the kernel's order: rows inside a chunk, then the
    waves of a workgroup in index order, then the workgroups (reduce groups)."""
    w32 = (w["levels"] * w["scale"]).float()
    total = torch.zeros(x.shape[0], w32.shape[1])
    for row in chunks:
        part = torch.zeros_like(total)
        for begin, end in row:
            part = part + x[:, begin:end].float() @ w32[begin:end]
        total = total + part
    return total


# ------------------------------------------------------------------ CPU tests


@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
def test_bound_passes_emulation_and_rejects_lost_or_doubled_sub_chunk(in_dim, out_dim):
    w = _weights(in_dim, out_dim)
    x = w["x"]
    ref = x.double() @ w["deq64"]
    bnd = _bound(x, w["deq64"])
    for waves in WAVES:
        for splits in SPLITS:
            n, chunks = _sub_chunks(in_dim, out_dim, waves, splits)
            assert sum(e - b for row in chunks for b, e in row) == in_dim
            assert all(row[0][1] > row[0][0] for row in chunks), "no workgroup may be empty"
            assert all(b % 16 == 0 for row in chunks for b, e in row if e > b)
            err = (_emulate_fp32(x, w, chunks).double() - ref).abs()
            assert (err <= bnd).all(), (waves, splits, (err / bnd).max())
            live = [(b, e) for row in chunks for b, e in row if e > b]
            if len(live) < 2:  # one chunk in all: nothing to lose or double
                assert in_dim <= 32 or splits == 1
                continue
            for begin, end in live:
                piece = x[:, begin:end].double() @ w["deq64"][begin:end]
                # dropped: ref - piece; counted twice: ref + piece. Same distance.
                worst = (piece.abs() / bnd).max().item()
                assert worst >= 2.0, (waves, splits, begin, end, worst)


def test_fastweight_accepts_tuple_and_int_tuning():
    from petals_amd.ops import fused_decode as fd

    class _Hip:
        def nf4_quantize(self, t):
            return nf4_ref.quantize(t)

    t = (torch.randn(64, 128) * 0.05).to(torch.bfloat16)
    key = ("nf4", 64, 128)
    saved = fd._split_autotune_cache.get(key)
    try:
        fd._split_autotune_cache[key] = (8, 16, True)
        fw = fd._FastWeight(t, _Hip(), "nf4")
        assert (fw.wg_waves, fw.splits, fw.nt) == (8, 16, True)
        fd._split_autotune_cache[key] = 64  # a bare split count selects the one-wave kernel
        fw = fd._FastWeight(t, _Hip(), "nf4")
        assert (fw.wg_waves, fw.splits, fw.nt) == (0, 64, False)
    finally:
        if saved is None:
            fd._split_autotune_cache.pop(key, None)
        else:
            fd._split_autotune_cache[key] = saved


# ------------------------------------------------------------------ GPU tests


def _gpu(w):
    return w["packed"].cuda(), w["absmax"].cuda(), w["absmax_t"].cuda()


def _twice(hip, wg, x, ws, epi, splits, waves, nt, residual=None, bias=None):
    """The call on a NaN-filled workspace, twice; asserts the two agree bit for bit."""
    outs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        outs.append(hip.gemv_nf4(wg[0], wg[1], x, ws, residual, epi, splits, bias, wg[2], waves, nt).clone())
    a, b = outs
    assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two runs differ"
    return a


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", SHAPES + [(4096, 512)])
def test_bit_identical_to_one_wave_kernel(hip, in_dim, out_dim):
    """(4096, 512) at splits 0 is 128 chunks of 32 rows: 8 per reduce group, so
    8 and 16 waves run the wg kernel and 4 waves fall back; splits 200 gives
    171 chunks of 24 rows (tail rows in every chunk, a ragged last group)."""
    w = _weights(in_dim, out_dim)
    wg = _gpu(w)
    ws = torch.empty(64 * B_MAX * out_dim, device="cuda")
    bias_g = w["bias"].cuda()
    big = in_dim == 4096
    for B in BATCHES:
        xg = w["x"][:B].cuda()
        res_g = w["residual"][:B].cuda()
        for splits in (SPLITS + (200,) if big else SPLITS):
            for epi, r, bias in ((EPI_PLAIN, None, None), (EPI_PLAIN, None, bias_g),
                                 (EPI_RESIDUAL, res_g, None), (EPI_SWIGLU, None, bias_g)):
                want = _twice(hip, wg, xg, ws, epi, splits, 0, False, r, bias)
                for waves in WAVES + (16,):
                    for nt in (False, True):
                        out = _twice(hip, wg, xg, ws, epi, splits, waves, nt, r, bias)
                        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8)), (B, splits, epi, waves, nt)
            raw_old = _twice(hip, wg, xg, ws, EPI_RAW, splits, 0, False)
            for waves in WAVES + (16,):
                raw = _twice(hip, wg, xg, ws, EPI_RAW, splits, waves, True)
                fits = raw_old.shape[0] <= 16 * waves and not (waves == 16 and B == 4)
                assert raw.shape[0] == (min(raw_old.shape[0], 16) if fits else raw_old.shape[0]), (B, splits, waves)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
def test_one_hot_bit_exact(hip, in_dim, out_dim):
    w = _weights(in_dim, out_dim)
    wg = _gpu(w)
    # NF4_LEVELS[nibble] * (1.5 * absmax): 1.5 * bf16 is exact, the product rounds once
    want_all = (w["levels"] * (1.5 * w["scale"])).cuda()
    ws = torch.empty(64 * B_MAX * out_dim, device="cuda")
    for waves in WAVES:
        for splits in SPLITS:
            n, chunks = _sub_chunks(in_dim, out_dim, waves, splits)
            rows = set()
            for row in chunks:
                for begin, end in row:
                    if end > begin:
                        rows.update((begin, end - 1))
                        if (end - begin) % 16:  # a row of the per-row tail loop
                            rows.add(begin + (end - begin) // 16 * 16)
            rows = sorted(rows)
            for nt in (False, True):
                for B in BATCHES:
                    for k in range(0, len(rows), B):
                        idx = (rows[k:k + B] + rows[:B])[:B]
                        x = torch.zeros(B, in_dim)
                        x[torch.arange(B), torch.tensor(idx)] = 1.5
                        x = x.cuda()
                        want = want_all[torch.tensor(idx)]
                        out = _twice(hip, wg, x, ws, EPI_PLAIN, splits, waves, nt)
                        assert out.shape == (B, out_dim) and out.dtype == torch.float32
                        assert torch.equal(out, want), (waves, splits, nt, B, idx, (out != want).nonzero()[:4])
                        raw = _twice(hip, wg, x, ws, EPI_RAW, splits, waves, nt)
                        assert raw.shape == (n, B, out_dim), (raw.shape, n)
                        assert torch.equal(raw.sum(0), want), (waves, splits, nt, B, idx)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("in_dim,out_dim", SHAPES)
def test_random_vs_float64(hip, in_dim, out_dim):
    """Epilogue bounds as in tests/test_mxfp4.py: +bias is one more fp32
    rounding; the residual epilogue rounds residual + sum to bf16 once
    (2^-8 |ref|); SwiGLU propagates the gate and up bounds through silu
    (|silu'| <= 1.1) and adds 2^-17 |ref| for the fast exponential."""
    w = _weights(in_dim, out_dim)
    wg = _gpu(w)
    half = out_dim // 2
    ws = torch.empty(64 * B_MAX * out_dim, device="cuda")
    bias_g = w["bias"].cuda()
    worst = {}
    for B in BATCHES:
        x = w["x"][:B]
        xg = x.cuda()
        res = w["residual"][:B]
        res_g = res.cuda()
        ref = x.double() @ w["deq64"]
        bnd = _bound(x, w["deq64"])
        refb = ref + w["bias"].double()
        gt, up = refb[:, :half], refb[:, half:]
        bg, bu = bnd[:, :half] + 2.0 ** -23 * gt.abs(), bnd[:, half:] + 2.0 ** -23 * up.abs()
        ref_sw = _silu(gt) * up
        ref_res = ref + res.double()
        cases = {
            "plain": (EPI_PLAIN, None, None, ref, bnd),
            "bias": (EPI_PLAIN, None, bias_g, refb, bnd + 2.0 ** -23 * refb.abs()),
            "residual": (EPI_RESIDUAL, res_g, None, ref_res, bnd + 2.0 ** -8 * ref_res.abs()),
            "swiglu": (EPI_SWIGLU, None, bias_g, ref_sw,
                       1.1 * bg * up.abs() + _silu(gt).abs() * bu + 1.1 * bg * bu + 2.0 ** -17 * ref_sw.abs()),
        }
        # (0, splits, False) is the old one-wave kernel on the same inputs
        configs = [(0, s, False) for s in SPLITS]
        configs += [(wv, s, nt) for wv in WAVES for s in SPLITS for nt in (False, True)]
        for waves, splits, nt in configs:
            for name, (epi, r, bias, want, bound) in cases.items():
                out = _twice(hip, wg, xg, ws, epi, splits, waves, nt, r, bias)
                assert not bool(torch.isnan(ws[0])), "the partials must land in the caller's workspace"
                out = out.cpu().double()
                assert out.shape == want.shape and torch.isfinite(out).all()
                err = (out - want).abs()
                ratio = (err / bound.clamp_min(1e-300)).max().item()
                kind = ("old" if waves == 0 else "wg", name)
                worst[kind] = max(worst.get(kind, 0.0), ratio)
                assert (err <= bound).all(), f"waves={waves} splits={splits} nt={nt} B={B} {name}: err/bound {ratio:.3f}"
    print(f"gemv_nf4 {in_dim}x{out_dim} worst err/bound: "
          + "  ".join(f"{k[0]}/{k[1]} {v:.4f}" for k, v in sorted(worst.items())))


@requires_gpu
@pytest.mark.gpu
def test_rejects_bad_wg_arguments(hip):
    w = _weights(32, 64)
    wg = _gpu(w)
    x = w["x"][:1].cuda()
    ws = torch.empty(64 * 64, device="cuda")
    for waves, nt in ((2, False), (32, False), (0, True), (1, True)):
        with pytest.raises(RuntimeError):
            hip.gemv_nf4(wg[0], wg[1], x, ws, None, EPI_PLAIN, 0, None, wg[2], waves, nt)
    # batch 5..8 keep the one-wave kernel whatever wg_waves says
    x5 = torch.randn(5, 32, device="cuda")
    a = hip.gemv_nf4(wg[0], wg[1], x5, ws, None, EPI_PLAIN, 0, None, wg[2], 8, False)
    b = hip.gemv_nf4(wg[0], wg[1], x5, ws, None, EPI_PLAIN, 0, None, wg[2])
    assert torch.equal(a, b)


@requires_gpu
@pytest.mark.gpu
@pytest.mark.parametrize("nt", [False, True])
def test_block_on_wg_kernel_graph_equals_eager_and_matches_old(hip, monkeypatch, nt):
    from petals_amd.models import get_model_block
    from petals_amd.models.config_base import load_model_config
    from petals_amd.ops import fused_decode as fd
    from petals_amd.server.from_pretrained import init_random_block_
    from petals_amd.utils.graphs import GraphedCallable

    cfg = load_model_config("test-llama-hd128")
    hd = cfg.hidden_size // cfg.num_attention_heads
    qkv_out = cfg.hidden_size + 2 * cfg.num_key_value_heads * hd
    shapes = [(cfg.hidden_size, qkv_out), (cfg.hidden_size, cfg.hidden_size),
              (cfg.hidden_size, 2 * cfg.intermediate_size), (cfg.intermediate_size, cfg.hidden_size)]

    def block(tuned):
        for s in shapes:
            monkeypatch.setitem(fd._split_autotune_cache, ("nf4",) + s, tuned)
        b = get_model_block(cfg, 0)
        init_random_block_(b, cfg, 0)
        b = b.to("cuda", torch.bfloat16).eval().optimize_for_inference(quant="nf4")
        fp = b._fast
        assert fp is not None and fp.graph_safe
        for fw in (fp.wqkv_t, fp.wo_t, fp.wgateup_t, fp.wdown_t):
            assert fw.shape in shapes and (fw.wg_waves, fw.splits, fw.nt) == tuned
        return b

    torch.manual_seed(11)
    B = 1  # the batch at which _FastWeight routes to the wg kernel
    xs = [torch.randn(B, 1, cfg.hidden_size, device="cuda", dtype=torch.bfloat16) * 0.5 for _ in range(3)]
    old = block((0, 0, False))
    ks, vs = old.kv_cache_shape(B, 16)

    def eager(blk):
        k = torch.zeros(ks, device="cuda", dtype=torch.bfloat16)
        v = torch.zeros(vs, device="cuda", dtype=torch.bfloat16)
        with torch.no_grad():
            return [blk(x, kv_cache=(k, v), prefix_length=t).clone() for t, x in enumerate(xs)], k, v

    outs_old, k_old, v_old = eager(old)
    for tuned in ((8, 16, nt), (4, 8, nt)):
        blk = block(tuned)
        outs, k_e, v_e = eager(blk)
        for o, oo in zip(outs, outs_old):
            assert torch.allclose(o.float(), oo.float(), atol=2e-2, rtol=2e-2), (tuned, (o.float() - oo.float()).abs().max())
        assert torch.allclose(k_e.float(), k_old.float(), atol=2e-2, rtol=2e-2)
        assert torch.allclose(v_e.float(), v_old.float(), atol=2e-2, rtol=2e-2)
        # same split count on both kernels: the wg kernel owes the same bits
        old_same = block((0, tuned[1], False))
        outs_same, k_s, v_s = eager(old_same)
        for o, oo in zip(outs, outs_same):
            assert torch.equal(o.view(torch.int16), oo.view(torch.int16)), tuned
        assert torch.equal(k_e, k_s) and torch.equal(v_e, v_s)

        kg, vg = torch.zeros_like(k_e), torch.zeros_like(v_e)
        ctx = fd.DecodeContext(torch.device("cuda"))
        ctx.set_position(0)
        h_in = torch.zeros_like(xs[0])
        with torch.no_grad():
            graph = GraphedCallable(lambda: blk(h_in, kv_cache=(kg, vg), ctx=ctx), [])
        kg.zero_()
        vg.zero_()
        for t, x in enumerate(xs):
            ctx.set_position(t)
            h_in.copy_(x)
            og = graph.replay().clone()
            assert torch.equal(og.view(torch.int16), outs[t].view(torch.int16)), (tuned, t)
        assert torch.equal(kg, k_e) and torch.equal(vg, v_e)
