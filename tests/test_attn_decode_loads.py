"""Decode attention: the order in which `mfma_decode_kernel` and
`attn_decode_combine_kernel` issue their loads must not change a single output
bit.

`tests/golden/attn_decode_loads.npz` holds the float32 outputs of
`attn_decode_fused` for the seeded inputs below, recorded on an MI355X from the
kernels as they were BEFORE their loads were batched (the parent of the commit
that added this file). Every case is compared with `torch.equal`; there is no
tolerance.

The lengths cover, for the 4-wave / 32-key-tile kernel: empty waves (kv_len 1,
31, 32, 33), a partial last tile (31, 33, 100, 129, 600), exactly one tile per
wave (kv_len 208 at 2 splits is 104 rows, 4 tiles; kv_len 129 at 1 split), two
tiles per wave with a partial last one (600 at 1 and 2 splits), and an empty
split (kv_len 1 at 2 and 5 splits, 33 at 5). Three more cases (kv_len 2100 at
16, 37 and 64 splits) hold the split combine kernel, which loads the partials
of 8 splits at a time, to the sums of the plain loop over the splits.

Guards: the same cases with the cache rows [kv_len, lmax) holding V = NaN and
K needle rows (50 x the unit q of the group's first head: one attended needle
takes the whole softmax row), and NaN-filled split workspaces. One more run
puts the cache in a tensor of exactly kv_len rows, so a read past `j_end` of
the last (batch, head) is a read past the tensor.

Regenerating the fixture (only ever from a build whose kernel is known good):
    python tests/test_attn_decode_loads.py --write tests/golden/attn_decode_loads.npz
"""

import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from petals_amd.ops import kv_fp8  # noqa: E402

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_decode_loads.npz")
FP8 = torch.float8_e4m3fn
KV_LENS = (1, 31, 32, 33, 100, 129, 208, 600)


@dataclasses.dataclass(frozen=True)
class Case:
    fmt: str  # "bf16" | "fp8"
    hd: int
    gq: int
    n_splits: int  # 0: the host's split policy
    kv_len: int
    b: int
    kvh: int
    alibi: bool = False

    @property
    def id(self):
        return (f"{self.fmt}-hd{self.hd}-gq{self.gq}-ns{self.n_splits}-kv{self.kv_len}-b{self.b}"
                + ("-alibi" if self.alibi else ""))

    @property
    def lmax(self):
        return -(-self.kv_len // 64) * 64 + 64


CASES = (
    [Case("bf16", 128, 8, ns, kv, b, 1) for ns in (1, 2, 5) for kv in KV_LENS for b in (1, 3)]
    + [Case("bf16", 64, 71, 2, 100, 1, 1)]
    + [Case("bf16", 128, 8, 0, 208, 1, 2, alibi=True)]
    + [Case("fp8", 128, 8, 2, kv, 1, 2) for kv in (33, 208)]
    # many splits: attn_decode_combine_kernel loads its partials in batches of 8
    + [Case("bf16", 128, 8, ns, 2100, 1, 1) for ns in (16, 37, 64)]
)
PARAMS = [pytest.param(c, id=c.id) for c in CASES]


@dataclasses.dataclass(frozen=True)
class Inputs:
    q: torch.Tensor  # [B, KV*GQ*HD] f32
    k: torch.Tensor  # [B, KV, lmax, HD] bf16 (fp8 cases: values on the E4M3 grid)
    v: torch.Tensor
    slopes: object
    scale: float


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    shape = (case.b, case.kvh, case.lmax, case.hd)
    q = torch.randn(case.b, case.kvh * case.gq * case.hd, generator=g)
    k = torch.randn(shape, generator=g).to(torch.bfloat16)
    v = torch.randn(shape, generator=g).to(torch.bfloat16)
    if case.fmt == "fp8":
        k, v = kv_fp8.roundtrip(k), kv_fp8.roundtrip(v)
    slopes = None
    if case.alibi:
        h = case.kvh * case.gq
        slopes = torch.tensor([2.0 ** (-8.0 * (i + 1) / h) for i in range(h)], dtype=torch.float32)
    return Inputs(q, k, v, slopes, case.hd**-0.5)


def poisoned(case, inp):
    """Rows [kv_len, lmax): V = NaN, K = needles for the first head of the group."""
    k, v = inp.k.clone(), inp.v.clone()
    q0 = inp.q.view(case.b, case.kvh, case.gq, case.hd)[:, :, 0]
    needle = 50.0 * q0 / q0.norm(dim=-1, keepdim=True)
    k[:, :, case.kv_len :] = needle[:, :, None].to(torch.bfloat16)
    v[:, :, case.kv_len :] = float("nan")
    return k, v


def to_cache(case, t):
    return (kv_fp8.quantize(t) if case.fmt == "fp8" else t).cuda()


def host_splits(case, lmax):
    """attn_decode_fused's split policy (attention.hip)."""
    if case.n_splits:
        return case.n_splits
    bkv = max(1, case.b * case.kvh)
    return max(1, min(768 // bkv, lmax // 512), min(256 // bkv, (lmax + 127) // 128))


def run(hip, case, inp, k_dev, v_dev, nan_workspaces=False):
    ns = host_splits(case, k_dev.shape[2])
    if nan_workspaces:
        n = case.b * case.kvh * ns * case.gq
        part_o = torch.full((n * case.hd + 4099,), float("nan"), device="cuda")
        part_ml = torch.full((n * 2 + 131,), float("nan"), device="cuda")
    else:
        part_o = part_ml = torch.empty(0, device="cuda")
    kv_len_t = torch.tensor([case.kv_len], dtype=torch.int32, device="cuda")
    slopes = inp.slopes.cuda() if inp.slopes is not None else None
    out = hip.attn_decode_fused(inp.q.cuda(), k_dev, v_dev, kv_len_t, case.gq, case.n_splits, part_o, part_ml,
                                inp.scale, slopes)
    return out.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(GOLDEN), f"fixture missing: {GOLDEN}"
    with np.load(GOLDEN) as f:
        return {name: torch.from_numpy(f[name]) for name in f.files}


def test_case_table_is_the_issue_list():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids)) == 3 * 8 * 2 + 1 + 1 + 2 + 3
    main = [c for c in CASES if c.fmt == "bf16" and c.hd == 128 and not c.alibi and c.kv_len != 2100]
    assert {(c.n_splits, c.kv_len, c.b) for c in main} == {(n, kv, b) for n in (1, 2, 5) for kv in KV_LENS for b in (1, 3)}
    assert all(c.lmax == -(-c.kv_len // 64) * 64 + 64 and c.lmax - c.kv_len >= 64 for c in CASES)
    alibi = [c for c in CASES if c.alibi]
    assert len(alibi) == 1 and host_splits(alibi[0], alibi[0].lmax) > 1


def test_fixture_holds_every_case_and_only_float32():
    assert os.path.getsize(GOLDEN) < 512 * 1024
    with np.load(GOLDEN) as f:
        assert sorted(f.files) == sorted(c.id for c in CASES)
        for c in CASES:
            a = f[c.id]
            assert a.dtype == np.float32 and a.shape == (c.b, c.kvh * c.gq * c.hd)
            assert np.isfinite(a).all() and np.abs(a).max() > 0


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", PARAMS)
def test_bit_identical_to_recorded_outputs(hip, golden, case):
    inp = make_inputs(case)
    k_dev, v_dev = to_cache(case, inp.k), to_cache(case, inp.v)
    out = run(hip, case, inp, k_dev, v_dev)
    assert torch.equal(bits(out), bits(run(hip, case, inp, k_dev, v_dev))), "not reproducible"
    want = golden[case.id]
    assert torch.equal(bits(out), bits(want)), (out - want).abs().max()


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", PARAMS)
def test_guards_hold_under_poison(hip, golden, case):
    inp = make_inputs(case)
    k, v = poisoned(case, inp)
    k_dev, v_dev = to_cache(case, k), to_cache(case, v)
    assert torch.isnan(v_dev[:, :, case.kv_len :].float()).all()
    out = run(hip, case, inp, k_dev, v_dev, nan_workspaces=True)
    assert torch.equal(bits(out), bits(run(hip, case, inp, k_dev, v_dev, nan_workspaces=True))), "not reproducible"
    want = golden[case.id]
    assert torch.equal(bits(out), bits(want)), (out - want).abs().max()


EXACT = [c for c in CASES if c.n_splits == 2 and c.kv_len in (33, 100) and (c.b == 3 or c.fmt == "fp8" or c.hd == 64)]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in EXACT])
def test_cache_of_exactly_kv_len_rows(hip, golden, case):
    """lmax = kv_len: a read past j_end of the last (batch, head) would leave
    the tensor. Same bits as the same rows in the larger cache."""
    assert len(EXACT) == 4
    inp = make_inputs(case)
    k_dev = to_cache(case, inp.k[:, :, : case.kv_len].contiguous())
    v_dev = to_cache(case, inp.v[:, :, : case.kv_len].contiguous())
    assert k_dev.shape[2] == case.kv_len
    out = run(hip, case, inp, k_dev, v_dev, nan_workspaces=True)
    assert torch.equal(bits(out), bits(run(hip, case, inp, k_dev, v_dev, nan_workspaces=True))), "not reproducible"
    assert torch.equal(bits(out), bits(golden[case.id]))


def write_fixture(path):
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, ops._hip_import_error
    arrays = {}
    for case in CASES:
        inp = make_inputs(case)
        out = run(mod, case, inp, to_cache(case, inp.k), to_cache(case, inp.v))
        assert out.dtype == torch.float32 and torch.isfinite(out).all()
        arrays[case.id] = out.numpy()
    np.savez(path, **arrays)
    print(f"wrote {len(arrays)} cases, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--write", __doc__
    write_fixture(sys.argv[2])
