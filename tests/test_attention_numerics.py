"""Sharp numerics tests for the attention path: `attn_decode_fused`,
`attn_prefill_fused`, and the decode-step cache writers that produce the rows
the attention reads.

How the checks are built (see also docs/KERNELS.md, "How attention numerics
are tested"):

* reference: plain float64 attention (`ref_attention_f64`);
* metric: `nerr` = max over (batch, head, q row) of max_d|out-ref| / max_d|ref|;
* tolerance: 4x the worst error of `emulated_attention_f64`, a float64 model
  of the kernels' documented bf16 rounding points, measured on the CPU over
  every case below (never from a kernel's output);
* inputs: "sharp" random scores (std ~2), "needle" keys that carry >= 0.99 of
  one row's softmax mass at the positions where kernels go wrong, and
  "poison" (needle K rows + 1e4 / NaN V rows) in every cache row past kv_len;
* CPU self-checks: corrupted references ("mutants") must be rejected at
  >= 2x the tolerance, so the suite's discriminating power is itself tested.

The CPU self-checks run without a GPU; GPU tests carry the `gpu` mark.
"""

import dataclasses
import functools
import math
import zlib
from typing import List, Optional, Tuple

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

LOG2E = 1.4426950408889634
ALPHA0 = 16.0  # needle strength: K[j] = alpha * q_h / |q_h|
NEEDLE_MASS = 0.99
POISON_V = 1.0e4

# In the pair variant V[j2] = -V[j1] + PAIR_NOISE * N(0,1): the two needles
# split the row's mass ~50/50, so the output is ~0.5 * PAIR_NOISE * N(0,1)
# while a relative mis-weighting eps of one split moves it by
# ~eps/4 * 2|V[j1]|. With PAIR_NOISE = 0.5 that amplifies a split-weight
# error ~8x relative to a row of independent V rows; the emulated rounding
# error is amplified alike and is part of the TOL_DECODE measurement.
PAIR_NOISE = 0.5

# --------------------------------------------------------------- tolerances
#
# TOL_* = 4 x max over the case tables of nerr(emulated_attention_f64, ref),
# rounded up to 3 significant digits. The factor 4 covers what the emulation
# does not model: the online-softmax rescale rounds at tile boundaries, and
# __expf/exp2f are a few ulp off. `test_tolerance_constants_are_measured`
# recomputes the maxima, `test_emulated_error_within_quarter_tol` checks every
# case, so a new case cannot silently outgrow the constants.
#
# Measured nerr(emulated, ref) per case and variant (CPU, float64):
#
#   case                                           sharp   needle0 needle1 pair
#   A-hd128-gq8-kvh2-b1-lmax128-kv1                0.00000 0.00000 0.00000    -
#   A-hd128-gq8-kvh2-b1-lmax128-kv31               0.00460 0.00461 0.00462    -
#   A-hd128-gq8-kvh2-b1-lmax128-kv32               0.00440 0.00446 0.00336    -
#   A-hd128-gq8-kvh2-b1-lmax128-kv33               0.00513 0.00546 0.00545    -
#   A-hd128-gq8-kvh2-b1-lmax128-kv127              0.00627 0.00484 0.00626    -
#   A-hd128-gq8-kvh2-b1-lmax128-kv128              0.00711 0.00709 0.00478    -
#   B-hd128-gq8-kvh2-b2-lmax640-kv129              0.00618 0.00510 0.00322 0.00492
#   B-hd128-gq8-kvh2-b2-lmax640-kv500              0.00582 0.00583 0.00376 0.00582
#   B-hd128-gq8-kvh2-b2-lmax640-kv640              0.00585 0.00453 0.00399 0.00595
#   C-hd128-gq4-kvh1-b2-lmax8192-kv100             0.00604 0.00000 0.00000 0.00605
#   C-hd128-gq4-kvh1-b2-lmax8192-kv2049            0.00451 0.00002 0.00002 0.00452
#   C-hd128-gq4-kvh1-b2-lmax8192-kv8192            0.00506 0.00002 0.00002 0.00506
#   D-hd64-gq29-kvh1-b1-lmax1024-kv95              0.00651 0.00676 0.00641 0.00656
#   D-hd64-gq29-kvh1-b1-lmax1024-kv333             0.00989 0.00990 0.00994 0.00989
#   D-hd64-gq29-kvh1-b1-lmax1024-kv1024            0.00604 0.00611 0.00602 0.00604
#   D-hd64-gq71-kvh1-b1-lmax1024-kv95              0.00618 0.00679 0.00833 0.00603
#   D-hd64-gq71-kvh1-b1-lmax1024-kv333             0.00588 0.00588 0.00588 0.00588
#   D-hd64-gq71-kvh1-b1-lmax1024-kv1024            0.00655 0.00649 0.00666 0.00661
#   D'-hd64-gq32-kvh2-b2-lmax512-kv200             0.00605 0.00582 0.00595 0.00589
#   D'-hd128-gq32-kvh2-b2-lmax512-kv200            0.00763 0.00767 0.00757 0.00788
#   E-hd128-gq6-kvh4-b2-lmax640-kv500-splits3      0.00649 0.00001 0.00001 0.00649
#   E-hd128-gq6-kvh4-b2-lmax640-kv500-splits7      0.00688 0.00001 0.00001 0.00689
#   F-hd64-gq1-kvh8-b2-lmax2048-kv73               0.00613 0.00007 0.00006 0.00475
#   F-hd64-gq1-kvh8-b2-lmax2048-kv1500             0.00649 0.00004 0.00009 0.00649
#   F-hd128-gq4-kvh4-b2-lmax2048-kv73              0.00692 0.00001 0.00017 0.00692
#   F-hd128-gq4-kvh4-b2-lmax2048-kv1500            0.00590 0.00000 0.00008 0.00590
#
#   cache-writer cases (kv_len = pos + 1, needle at pos)   pos0    pos1    pos2047
#   rope_cache_write-hd64                                  0.00000 0.00490 0.00655
#   rope_cache_write-hd128                                 0.00000 0.00250 0.00524
#   qkv_rope_reduce_rope-hd64                              0.00000 0.00566 0.00538
#   qkv_rope_reduce_rope-hd128                             0.00000 0.00384 0.00489
#   qkv_rope_reduce_bias-hd64                              0.00000 0.00335 0.00430
#   qkv_rope_reduce_bias-hd128                             0.00000 0.00327 0.00630
#   kv_cache_write-hd64                                    0.00000 0.00169 0.00445
#   kv_cache_write-hd128                                   0.00000 0.00268 0.00854
#
#   worst 0.00994 -> x4, rounded up
TOL_DECODE = 0.0398
#
#   case                                           diag    forbid
#   b2-qh4-kvh2-s17-hd128-off0-causal              0.00519 0.00614
#   b1-qh4-kvh4-s65-hd128-off63-causal             0.00778 0.00745
#   b1-qh8-kvh2-s130-hd64-off70-causal             0.00958 0.00866
#   b1-qh4-kvh1-s64-hd128-off1-causal              0.00691 0.00750
#   b2-qh4-kvh2-s70-hd64-off0-full                 0.00813    -
#   b1-qh8-kvh8-s130-hd64-off70-causal-alibi       0.01069 0.00874
#   b1-qh4-kvh4-s200-hd128-off0-causal-alibi       0.00847 0.00867
#   b1-qh4-kvh4-s15-hd128-off100-causal-alibi      0.00802 0.00717
#
#   worst 0.01069 -> x4, rounded up
TOL_PREFILL = 0.0428


# ------------------------------------------------------ reference and metric


def ref_probs_f64(q, k, kv_len, scale, causal=False, kv_offset=0, slopes=None):
    """Plain float64 softmax probabilities [B, H, S, kv_len]. q [B, H, S, D];
    k [B, KVH, L >= kv_len, D] (rows past kv_len are ignored); `slopes` [H]
    adds slope[h] * key_pos; `causal` masks key > kv_offset + q_row."""
    b, h, s, _ = q.shape
    q64 = q.to(torch.float64)
    k64 = k[:, :, :kv_len].to(torch.float64).repeat_interleave(h // k.shape[1], dim=1)
    logits = torch.einsum("bhsd,bhld->bhsl", q64, k64) * scale
    key_pos = torch.arange(kv_len, dtype=torch.float64)
    if slopes is not None:
        logits = logits + slopes.to(torch.float64)[None, :, None, None] * key_pos
    if causal:
        q_abs = kv_offset + torch.arange(s, dtype=torch.float64)
        logits = logits.masked_fill(key_pos[None, :] > q_abs[:, None], float("-inf"))
    return torch.softmax(logits, dim=-1)


def ref_attention_f64(q, k, v, kv_len, scale, causal=False, kv_offset=0, slopes=None):
    """Plain float64 attention with GQA repeat; v like k. Returns [B, H, S, D]."""
    probs = ref_probs_f64(q, k, kv_len, scale, causal, kv_offset, slopes)
    v64 = v[:, :, :kv_len].to(torch.float64).repeat_interleave(q.shape[1] // v.shape[1], dim=1)
    return torch.einsum("bhsl,bhld->bhsd", probs, v64)


def _round_bf16(x64):
    return x64.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def emulated_attention_f64(q, k, v, kv_len, scale, causal=False, kv_offset=0, slopes=None, kernel="decode"):
    """The same maths in float64 with only the kernels' documented rounding
    points: q*scale -> bf16 (prefill: q*scale*log2e, exp2 softmax), the
    probabilities -> bf16 before PV (the normaliser sums the unrounded ones),
    and for prefill the output -> bf16. No tiling, no online softmax."""
    b, h, s, _ = q.shape
    rep = h // k.shape[1]
    prefill = kernel == "prefill"
    # the kernels form q*scale in f32 and round that product to bf16
    qscale = torch.tensor(scale, dtype=torch.float32)
    if prefill:
        qscale = qscale * torch.tensor(LOG2E, dtype=torch.float32)
    qs = (q.to(torch.float32) * qscale).to(torch.bfloat16).to(torch.float64)
    k64 = k[:, :, :kv_len].to(torch.float64).repeat_interleave(rep, dim=1)
    v64 = v[:, :, :kv_len].to(torch.float64).repeat_interleave(rep, dim=1)
    logits = torch.einsum("bhsd,bhld->bhsl", qs, k64)
    key_pos = torch.arange(kv_len, dtype=torch.float64)
    if slopes is not None:
        sl = slopes.to(torch.float32)
        if prefill:
            sl = sl * torch.tensor(LOG2E, dtype=torch.float32)
        logits = logits + sl.to(torch.float64)[None, :, None, None] * key_pos
    if causal:
        q_abs = kv_offset + torch.arange(s, dtype=torch.float64)
        logits = logits.masked_fill(key_pos[None, :] > q_abs[:, None], float("-inf"))
    shifted = logits - logits.amax(dim=-1, keepdim=True)
    p = torch.exp2(shifted) if prefill else torch.exp(shifted)
    out = torch.einsum("bhsl,bhld->bhsd", _round_bf16(p), v64) / p.sum(dim=-1, keepdim=True)
    return _round_bf16(out) if prefill else out


def nerr(out, ref):
    """max over (batch, head, q row) of max_d|out-ref| / max_d|ref|. Normalised
    per output row; a NaN or inf anywhere in `out` gives inf."""
    diff = (out.to(torch.float64) - ref.to(torch.float64)).abs()
    diff = torch.nan_to_num(diff, nan=float("inf"), posinf=float("inf"))
    return (diff.amax(dim=-1) / ref.to(torch.float64).abs().amax(dim=-1)).max().item()


# ------------------------------------------------------------------- inputs


@dataclasses.dataclass
class Inputs:
    """One attention problem. `v` carries the 1e4 poison; `v_nan()` the NaN one."""

    q: torch.Tensor  # [B, H, S, D]: f32 (decode) or bf16 (prefill)
    k: torch.Tensor  # [B, KVH, lmax, D] bf16
    v: torch.Tensor
    kv_len: int
    scale: float
    causal: bool = False
    kv_offset: int = 0
    slopes: Optional[torch.Tensor] = None
    kernel: str = "decode"
    needles: Tuple = ()  # (batch, head, q_row, key)
    alphas: Tuple = ()

    def args(self):
        return (self.q, self.k, self.v, self.kv_len, self.scale, self.causal, self.kv_offset, self.slopes)

    def v_nan(self):
        v = self.v.clone()
        v[:, :, self.kv_len :] = float("nan")
        return v

    @functools.cached_property
    def ref(self):
        return ref_attention_f64(*self.args())

    @functools.cached_property
    def emulated(self):
        return emulated_attention_f64(*self.args(), kernel=self.kernel)


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _sharp_kv(g, b, kvh, lmax, hd):
    k = (2.0 * torch.randn(b, kvh, lmax, hd, generator=g)).to(torch.bfloat16)
    v = torch.randn(b, kvh, lmax, hd, generator=g).to(torch.bfloat16)
    return k, v


def _unit(x):
    x = x.to(torch.float64)
    return x / x.norm(dim=-1, keepdim=True)


def _place_needles(q, k, needles, mass_of, gq):
    """Overwrite K[key] = alpha * q_row/|q_row| for every needle (b, h, row, key)
    and raise alpha (x1.5 per round, per needle) until `mass_of(k)` reports
    >= NEEDLE_MASS for all of them. The bound itself is never relaxed."""
    k = k.clone()
    alphas = [ALPHA0] * len(needles)
    qhat = _unit(q)
    for _ in range(40):
        for (bi, h, row, key), a in zip(needles, alphas):
            k[bi, h // gq, key] = (a * qhat[bi, h, row]).to(torch.bfloat16)
        mass = mass_of(k)
        bad = [i for i, m in enumerate(mass) if not m >= NEEDLE_MASS]
        if not bad:
            return k, tuple(alphas)
        for i in bad:
            alphas[i] *= 1.5
    raise AssertionError(f"needles never reached {NEEDLE_MASS} of their row's mass: {min(mass)}")


def _poison(q, k, v, kv_len, gq, alpha, rows):
    """Rows [kv_len, lmax): K = needles aimed at the live queries (head and q
    row cycle with the key index), V = 1e4."""
    lmax = k.shape[2]
    if kv_len >= lmax:
        return
    qhat = _unit(q)
    j = torch.arange(kv_len, lmax)
    for kh in range(k.shape[1]):
        heads = kh * gq + (j % gq)
        k[:, kh, kv_len:] = (alpha * qhat[:, heads, rows[j % len(rows)]]).to(torch.bfloat16)
    v[:, :, kv_len:] = POISON_V


# ------------------------------------------------------------- decode cases


@dataclasses.dataclass(frozen=True)
class DecodeCase:
    group: str
    hd: int
    gq: int
    kvh: int
    b: int
    lmax: int
    kv_len: int
    n_splits: int = 0  # 0 = the kernel's own policy
    alibi: bool = False

    @property
    def id(self):
        s = f"{self.group}-hd{self.hd}-gq{self.gq}-kvh{self.kvh}-b{self.b}-lmax{self.lmax}-kv{self.kv_len}"
        return s + (f"-splits{self.n_splits}" if self.n_splits else "")


def mfma_auto_splits(b, kvh, lmax):
    """Mirror of the MFMA split policy in attention.hip; used only to aim
    needles at split boundaries and to check that the table reaches the
    regimes it claims (never to judge an output)."""
    bkv = max(1, b * kvh)
    by_occ = min(768 // bkv, lmax // 512)
    by_min = min(256 // bkv, (lmax + 127) // 128)
    return max(1, by_occ, by_min)


DECODE_CASES: List[DecodeCase] = (
    [DecodeCase("A", 128, 8, 2, 1, 128, n) for n in (1, 31, 32, 33, 127, 128)]
    + [DecodeCase("B", 128, 8, 2, 2, 640, n) for n in (129, 500, 640)]
    + [DecodeCase("C", 128, 4, 1, 2, 8192, n) for n in (100, 2049, 8192)]
    + [DecodeCase("D", 64, gq, 1, 1, 1024, n) for gq in (29, 71) for n in (95, 333, 1024)]
    + [DecodeCase("D'", hd, 32, 2, 2, 512, 200) for hd in (64, 128)]
    + [DecodeCase("E", 128, 6, 4, 2, 640, 500, n_splits=n) for n in (3, 7)]
    + [
        DecodeCase("F", hd, gq, kvh, 2, 2048, n, alibi=True)
        for (hd, gq, kvh) in ((64, 1, 8), (128, 4, 4))
        for n in (73, 1500)
    ]
)
DECODE_VARIANTS = ("sharp", "needle0", "needle1", "pair")


def _splits(case: DecodeCase) -> int:
    return case.n_splits or mfma_auto_splits(case.b, case.kvh, case.lmax)


def decode_needle_positions(case: DecodeCase) -> List[int]:
    """{0, 31, 32, kv_len-1} plus the first and last key of the second split."""
    pos = [0, 31, 32, case.kv_len - 1]
    n = _splits(case)
    rps = -(-case.kv_len // n)
    if n > 1 and rps < case.kv_len:
        pos += [rps, min(2 * rps, case.kv_len) - 1]
    return sorted({p for p in pos if 0 <= p < case.kv_len})


@functools.lru_cache(maxsize=None)
def decode_inputs(case: DecodeCase, variant: str) -> Optional[Inputs]:
    """sharp: no needles. needle0/needle1: needles at `decode_needle_positions`,
    owned by distinct heads of each kv head; the position a head owns shifts
    with the batch row and the kv head, and needle1 moves the needles to the
    next set of heads. pair: two equal needles for one head per kv head, in
    the first and the second split, whose V rows nearly cancel, so that row's
    output is the small difference of two split partials (None where the
    case has a single split). All variants: poison past kv_len."""
    g = _gen(case.id)
    b, kvh, gq, hd, lmax, kv_len = case.b, case.kvh, case.gq, case.hd, case.lmax, case.kv_len
    h = kvh * gq
    q = torch.randn(b, h, 1, hd, generator=g)
    k, v = _sharp_kv(g, b, kvh, lmax, hd)
    slopes = None
    if case.alibi:
        from petals_amd.ops import reference

        slopes = reference.build_alibi_slopes(h).to(torch.float32)
    scale = 1.0 / math.sqrt(hd)
    needles = []
    if variant in ("needle0", "needle1"):
        rot = int(variant[-1])
        pos = decode_needle_positions(case)
        n = min(gq, len(pos))
        for bi in range(b):
            for kh in range(kvh):
                for i in range(n):
                    head = kh * gq + (i + rot * n) % gq
                    needles.append((bi, head, 0, pos[(i + bi + kh + rot) % len(pos)]))
    elif variant == "pair":
        n = _splits(case)
        rps = -(-kv_len // n)
        if n == 1 or rps >= kv_len:
            return None
        j1, j2 = rps - 1, rps  # last key of split 0, first key of split 1
        for bi in range(b):
            for kh in range(kvh):
                head = kh * gq + (bi + kh) % gq
                k[bi, kh, j1] = k[bi, kh, j2] = (ALPHA0 * _unit(q)[bi, head, 0]).to(torch.bfloat16)
                noise = torch.randn(hd, generator=g)
                v[bi, kh, j2] = (-v[bi, kh, j1].float() + PAIR_NOISE * noise).to(torch.bfloat16)
    alphas = ()
    if needles:

        def mass_of(kk):
            p = ref_probs_f64(q, kk, kv_len, scale, False, 0, slopes)
            return [p[bi, hh, row, key].item() for (bi, hh, row, key) in needles]

        k, alphas = _place_needles(q, k, needles, mass_of, gq)
    _poison(q, k, v, kv_len, gq, max(alphas, default=ALPHA0), torch.zeros(1, dtype=torch.long))
    return Inputs(q, k, v, kv_len, scale, slopes=slopes, needles=tuple(needles), alphas=alphas)


DECODE_PARAMS = [
    pytest.param(c, var, id=f"{c.id}-{var}")
    for c in DECODE_CASES
    for var in DECODE_VARIANTS
    if not (var == "pair" and (_splits(c) == 1 or -(-c.kv_len // _splits(c)) >= c.kv_len))
]


# ------------------------------------------------------------ prefill cases


@dataclasses.dataclass(frozen=True)
class PrefillCase:
    b: int
    qh: int
    kvh: int
    s: int
    hd: int
    off: int
    causal: bool
    alibi: bool

    @property
    def id(self):
        return (
            f"b{self.b}-qh{self.qh}-kvh{self.kvh}-s{self.s}-hd{self.hd}-off{self.off}"
            f"-{'causal' if self.causal else 'full'}{'-alibi' if self.alibi else ''}"
        )


PREFILL_CASES = [
    PrefillCase(2, 4, 2, 17, 128, 0, True, False),
    PrefillCase(1, 4, 4, 65, 128, 63, True, False),
    PrefillCase(1, 8, 2, 130, 64, 70, True, False),
    PrefillCase(1, 4, 1, 64, 128, 1, True, False),
    PrefillCase(2, 4, 2, 70, 64, 0, False, False),  # non-causal with a kv tail
    PrefillCase(1, 8, 8, 130, 64, 70, True, True),  # ALiBi, interior tiles reached
    PrefillCase(1, 4, 4, 200, 128, 0, True, True),
    PrefillCase(1, 4, 4, 15, 128, 100, True, True),
]
PREFILL_POISON_ROWS = 37  # lmax = kv_len + 37: no multiple of any tile size

# "forbid" needs a key the row may not see, which a non-causal case does not
# have inside kv_len (past kv_len it is the poison, present in every run)
PREFILL_PARAMS = [
    pytest.param(c, pat, id=f"{c.id}-{pat}")
    for c in PREFILL_CASES
    for pat in ("diag", "forbid")
    if c.causal or pat == "diag"
]


def prefill_needle_rows(s: int) -> List[int]:
    return sorted({i for i in [0, 15, 16, 63, 64, s - 1] + list(range(5, s, 13)) if 0 <= i < s})


@functools.lru_cache(maxsize=None)
def prefill_inputs(case: PrefillCase, pattern: str) -> Inputs:
    """diag: for q row i the needle sits at key off+i, the last key the row may
    see. forbid: at key off+i+1, the first key it may NOT see (zero mass in
    the reference; asserted to carry >= 0.99 if it were unmasked). Rows are
    dealt round-robin to the heads of each kv head, shifted by batch row."""
    g = _gen(case.id)
    b, qh, kvh, s, hd, off = case.b, case.qh, case.kvh, case.s, case.hd, case.off
    gq = qh // kvh
    kv_len = off + s
    lmax = kv_len + PREFILL_POISON_ROWS
    q = torch.randn(b, qh, s, hd, generator=g).to(torch.bfloat16)
    k, v = _sharp_kv(g, b, kvh, lmax, hd)
    slopes = None
    if case.alibi:
        from petals_amd.ops import reference

        slopes = reference.build_alibi_slopes(qh).to(torch.float32)
    scale = 1.0 / math.sqrt(hd)
    shift = 0 if pattern == "diag" else 1
    rows = prefill_needle_rows(s)
    # poison first: a forbidden needle of the last row lands in the poison zone
    _poison(q, k, v, kv_len, gq, ALPHA0, torch.tensor(rows[::-1]))
    needles = [
        (bi, kh * gq + (n + bi) % gq, i, off + i + shift)
        for bi in range(b)
        for kh in range(kvh)
        for n, i in enumerate(rows)
    ]

    def mass_of(kk):
        # forbid: the mass the key WOULD carry under a mask that lets it through
        p = ref_probs_f64(q, kk, kv_len + shift, scale, case.causal, off + shift, slopes)
        return [p[bi, hh, row, key].item() for (bi, hh, row, key) in needles]

    k, alphas = _place_needles(q, k, needles, mass_of, gq)
    inp = Inputs(q, k, v, kv_len, scale, case.causal, off, slopes, "prefill", tuple(needles), alphas)
    if pattern == "forbid":
        p = ref_probs_f64(q, k, kv_len, scale, case.causal, off, slopes)
        assert all(key >= kv_len or p[bi, hh, row, key] == 0 for (bi, hh, row, key) in needles)
    return inp


# ------------------------------------------------------- cache-writer cases

WRITER_KERNELS = ("rope_cache_write", "qkv_rope_reduce_rope", "qkv_rope_reduce_bias", "kv_cache_write")
WRITER_B, WRITER_QH, WRITER_KH, WRITER_LMAX = 2, 8, 2, 2048
WRITER_PARAMS = [
    pytest.param(kern, hd, pos, id=f"{kern}-hd{hd}-pos{pos}")
    for kern in WRITER_KERNELS
    for hd in (64, 128)
    for pos in (0, 1, 2047)
]


@dataclasses.dataclass
class WriterInputs:
    src: torch.Tensor  # f32 [3, b, row] split partials (qkv_rope_reduce) or [b, row] qkv
    cos: Optional[torch.Tensor]
    sin: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]  # bf16 [row]
    k0: torch.Tensor  # pre-filled caches (random live rows, poison past pos)
    v0: torch.Tensor
    q_ref: torch.Tensor  # f64 [b, qh, hd]
    k_ref: torch.Tensor  # f64 [b, kh, hd]
    v_ref: torch.Tensor
    attn: Inputs  # the decode problem over the EXPECTED cache, kv_len = pos + 1


@functools.lru_cache(maxsize=None)
def writer_inputs(kernel: str, hd: int, pos: int) -> WriterInputs:
    from petals_amd.ops import reference

    b, qh, kh, lmax = WRITER_B, WRITER_QH, WRITER_KH, WRITER_LMAX
    gq = qh // kh
    row = (qh + 2 * kh) * hd
    half = hd // 2
    g = _gen(f"writer-{kernel}-{hd}-{pos}")
    rope = kernel in ("rope_cache_write", "qkv_rope_reduce_rope")
    reduce = kernel.startswith("qkv_rope_reduce")
    cos = sin = bias = None
    if rope:
        cos, sin = reference.build_rope_cache(hd, lmax)
    if kernel == "qkv_rope_reduce_bias":
        bias = (0.5 * torch.randn(row, generator=g)).to(torch.bfloat16)
    bias64 = bias.to(torch.float64) if bias is not None else torch.zeros(row, dtype=torch.float64)
    total = torch.randn(b, row, generator=g, dtype=torch.float64)  # target sum over splits
    parts = torch.randn(2, b, row, generator=g)
    k0, v0 = _sharp_kv(g, b, kh, lmax, hd)
    kv_len = pos + 1
    scale = 1.0 / math.sqrt(hd)
    owners = [(bi, khi * gq + (bi + khi) % gq) for bi in range(b) for khi in range(kh)]

    def reference_rows(alpha):
        """Build the kernel input whose K rows are needles for `owners`, then
        the float64 reference of what the kernel must produce from it."""
        tot = total.clone()
        qfin = (tot[:, : qh * hd] + bias64[: qh * hd]).view(b, qh, hd)
        kview = tot[:, qh * hd : (qh + kh) * hd].view(b, kh, hd)
        for (bi, head), a in zip(owners, alpha):
            kview[bi, head // gq] = a * _unit(qfin[bi, head]) - bias64[qh * hd :].view(-1, hd)[head // gq]
        if reduce:
            src = torch.cat([parts, (tot - parts.to(torch.float64).sum(0)).to(torch.float32)[None]])
            summed = src.to(torch.float64).sum(0) + bias64
        else:
            src = tot.to(torch.float32)
            summed = src.to(torch.float64)
        heads = summed.view(b, qh + 2 * kh, hd)
        qk, vv = heads[:, : qh + kh], heads[:, qh + kh :]
        if rope:
            c = cos[pos, :half].to(torch.float64)
            s = sin[pos, :half].to(torch.float64)
            x1, x2 = qk[..., :half], qk[..., half:]
            qk = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
        return src, qk[:, :qh], qk[:, qh:], vv

    def expected(alpha):
        src, q_ref, k_ref, v_ref = reference_rows(alpha)
        ke, ve = k0.clone(), v0.clone()
        ke[:, :, pos] = k_ref.to(torch.bfloat16)
        ve[:, :, pos] = v_ref.to(torch.bfloat16)
        return src, q_ref, k_ref, v_ref, ke, ve

    needles = [(bi, head, 0, pos) for bi, head in owners]
    alpha = [ALPHA0] * len(owners)
    for _ in range(40):
        src, q_ref, k_ref, v_ref, ke, ve = expected(alpha)
        q4 = q_ref.to(torch.float32)[:, :, None, :]
        p = ref_probs_f64(q4, ke, kv_len, scale, False, 0, None)
        bad = [i for i, (bi, hh, _, key) in enumerate(needles) if not p[bi, hh, 0, key] >= NEEDLE_MASS]
        if not bad:
            break
        for i in bad:
            alpha[i] *= 1.5
    else:
        raise AssertionError("writer needles never dominated")
    # poison past pos goes into the PRE-FILLED caches: the writers must leave it bit-identical
    _poison(q4, k0, v0, kv_len, gq, max(alpha), torch.zeros(1, dtype=torch.long))
    src, q_ref, k_ref, v_ref, ke, ve = expected(alpha)
    attn = Inputs(q4, ke, ve, kv_len, scale, needles=tuple(needles), alphas=tuple(alpha))
    return WriterInputs(src, cos, sin, bias, k0, v0, q_ref, k_ref, v_ref, attn)


# ------------------------------------------------ all CPU-measurable cases


def _decode_like_inputs():
    for p in DECODE_PARAMS:
        yield p.id, decode_inputs(*p.values)
    for p in WRITER_PARAMS:
        yield "W-" + p.id, writer_inputs(*p.values).attn


def _prefill_like_inputs():
    for p in PREFILL_PARAMS:
        yield p.id, prefill_inputs(*p.values)


# ------------------------------------------------------------------ mutants
#
# Corrupted references: `_variant_attention_f64` is `ref_attention_f64` with
# hooks for exactly the mistakes below (checked equal to it when no hook is
# used). Each mutant returns None where it does not apply to a case.


def _variant_attention_f64(inp, kv_len=None, k=None, v=None, key_bias=None, alibi_pos=None, masked=None):
    kv_len = inp.kv_len if kv_len is None else kv_len
    k = inp.k if k is None else k
    v = inp.v if v is None else v
    b, h, s, _ = inp.q.shape
    rep = h // k.shape[1]
    q64 = inp.q.to(torch.float64)
    k64 = k[:, :, :kv_len].to(torch.float64).repeat_interleave(rep, dim=1)
    v64 = v[:, :, :kv_len].to(torch.float64).repeat_interleave(rep, dim=1)
    logits = torch.einsum("bhsd,bhld->bhsl", q64, k64) * inp.scale
    key_pos = torch.arange(kv_len, dtype=torch.float64)
    if inp.slopes is not None:
        pos = key_pos if alibi_pos is None else alibi_pos(key_pos)
        logits = logits + inp.slopes.to(torch.float64)[None, :, None, None] * pos
    if key_bias is not None:
        logits = logits + key_bias
    if inp.causal:
        q_abs = inp.kv_offset + torch.arange(s, dtype=torch.float64)
        m = key_pos[None, :] > q_abs[:, None] if masked is None else masked(key_pos[None, :], q_abs[:, None])
        logits = logits.masked_fill(m, float("-inf"))
    # a row with every key masked gives 0, as the kernels do (1/l guarded)
    probs = torch.nan_to_num(torch.softmax(logits, dim=-1), nan=0.0)
    return torch.einsum("bhsl,bhld->bhsd", probs, v64)


def _drop_keys(inp, lo, hi):
    if hi > inp.kv_len or inp.kv_len <= hi - lo:
        return None
    bias = torch.zeros(inp.kv_len, dtype=torch.float64)
    bias[lo:hi] = float("-inf")
    return _variant_attention_f64(inp, key_bias=bias)


def mutant_drop_last_key(inp, case):
    return _variant_attention_f64(inp, kv_len=inp.kv_len - 1) if inp.kv_len > 1 else None


def mutant_drop_key_32(inp, case):
    return _drop_keys(inp, 32, 33)


def mutant_drop_tile(inp, case):
    return _drop_keys(inp, 32, 64)


def mutant_first_split_weight(inp, case):
    n = _splits(case)
    rps = -(-inp.kv_len // n)
    if n == 1 or rps >= inp.kv_len:
        return None
    bias = torch.zeros(inp.kv_len, dtype=torch.float64)
    bias[:rps] = math.log(1.05)
    return _variant_attention_f64(inp, key_bias=bias)


def mutant_swap_heads(inp, case):
    if case.gq < 2:
        return None
    perm = torch.arange(inp.q.shape[1])
    perm[0], perm[1] = 1, 0  # heads 0 and 1 share kv head 0
    if case.gq > 3:
        perm[case.gq - 2], perm[case.gq - 1] = case.gq - 1, case.gq - 2
    return inp.ref[:, perm]


def mutant_batch0_cache(inp, case):
    if inp.q.shape[0] < 2:
        return None
    k, v = inp.k.clone(), inp.v.clone()
    k[1], v[1] = k[0], v[0]
    return _variant_attention_f64(inp, k=k, v=v)


def mutant_alibi_chunk_local(inp, case):
    if inp.slopes is None or inp.kv_len <= 128:
        return None
    return _variant_attention_f64(inp, alibi_pos=lambda p: p % 128)


def mutant_causal_one_late(inp, case):  # masks key > q_abs + 1
    if not inp.causal:
        return None
    kv_len = min(inp.kv_len + 1, inp.k.shape[2])
    return _variant_attention_f64(inp, kv_len=kv_len, masked=lambda key, q_abs: key > q_abs + 1)


def mutant_causal_one_early(inp, case):  # masks key >= q_abs
    if not inp.causal:
        return None
    return _variant_attention_f64(inp, masked=lambda key, q_abs: key >= q_abs)


def mutant_poisoned_row(inp, case):
    if inp.kv_len >= inp.k.shape[2]:
        return None
    return _variant_attention_f64(inp, kv_len=inp.kv_len + 1, masked=lambda key, q_abs: key > q_abs + 1)


DECODE_MUTANTS = [
    mutant_drop_last_key,
    mutant_drop_key_32,
    mutant_drop_tile,
    mutant_first_split_weight,
    mutant_swap_heads,
    mutant_batch0_cache,
    mutant_alibi_chunk_local,
    mutant_poisoned_row,
]
PREFILL_MUTANTS = [
    mutant_drop_last_key,
    mutant_drop_key_32,
    mutant_drop_tile,
    mutant_batch0_cache,
    mutant_alibi_chunk_local,
    mutant_causal_one_late,
    mutant_causal_one_early,
    mutant_poisoned_row,
]


def _worst_rejection(mutant, params, make):
    best, where = 0.0, None
    for p in params:
        inp = make(*p.values)
        out = mutant(inp, p.values[0])
        if out is not None:
            e = nerr(out, inp.ref)
            if e > best:
                best, where = e, p.id
    return best, where


# ------------------------------------------------------- CPU self-checks


def test_variant_reference_is_the_reference():
    for make, p in ((decode_inputs, DECODE_PARAMS[-2]), (prefill_inputs, PREFILL_PARAMS[-1])):
        inp = make(*p.values)
        assert torch.equal(_variant_attention_f64(inp), inp.ref)


def test_decode_table_reaches_its_regimes():
    by_group = {}
    for c in DECODE_CASES:
        by_group.setdefault(c.group, set()).add(_splits(c))
    assert by_group["A"] == {1} and by_group["B"] == {5} and by_group["C"] == {64}
    c = DECODE_CASES[9]
    assert (c.group, c.kv_len) == ("C", 100) and -(-c.kv_len // 64) == 2  # rows_per_split = 2


@pytest.mark.parametrize("case,variant", DECODE_PARAMS)
def test_decode_needles_dominate(case, variant):
    inp = decode_inputs(case, variant)
    p = ref_probs_f64(inp.q, inp.k, inp.kv_len, inp.scale, False, 0, inp.slopes)
    for bi, h, row, key in inp.needles:
        assert p[bi, h, row, key] >= NEEDLE_MASS
    # different batch rows and different heads of one kv head own different keys
    owned = {}
    for bi, h, row, key in inp.needles:
        assert owned.setdefault((bi, h // case.gq, key), h) == h
    if variant.startswith("needle") and len(decode_needle_positions(case)) > 1 and case.b > 1:
        per_batch = [{(h, key) for bi, h, _, key in inp.needles if bi == b_} for b_ in range(case.b)]
        assert per_batch[0].isdisjoint(per_batch[1])


def test_emulated_error_within_quarter_tol():
    for tol, kind, items in (
        (TOL_DECODE, "decode", _decode_like_inputs()),
        (TOL_PREFILL, "prefill", _prefill_like_inputs()),
    ):
        for name, inp in items:
            e = nerr(inp.emulated, inp.ref)
            print(f"emulated {kind:8s} {name:64s} nerr={e:.5f}  alpha_max={max(inp.alphas, default=0):.0f}")
            assert e <= tol / 4, (name, e, tol)


def test_tolerance_constants_are_measured():
    """TOL_* = 4 x the measured worst emulation error (rounded up): neither
    stale-low nor padded."""
    for tol, items in ((TOL_DECODE, _decode_like_inputs()), (TOL_PREFILL, _prefill_like_inputs())):
        worst = max(nerr(inp.emulated, inp.ref) for _, inp in items)
        assert 0.95 * tol / 4 <= worst <= tol / 4, (worst, tol)


@pytest.mark.parametrize("mutant", DECODE_MUTANTS, ids=lambda m: m.__name__)
def test_decode_mutant_rejected(mutant):
    e, where = _worst_rejection(mutant, DECODE_PARAMS, decode_inputs)
    print(f"{mutant.__name__}: nerr={e:.4f} at {where} (needs >= {2 * TOL_DECODE})")
    assert e >= 2 * TOL_DECODE, (mutant.__name__, e, where)


@pytest.mark.parametrize("mutant", PREFILL_MUTANTS, ids=lambda m: m.__name__)
def test_prefill_mutant_rejected(mutant):
    e, where = _worst_rejection(mutant, PREFILL_PARAMS, prefill_inputs)
    print(f"{mutant.__name__}: nerr={e:.4f} at {where} (needs >= {2 * TOL_PREFILL})")
    assert e >= 2 * TOL_PREFILL, (mutant.__name__, e, where)


def test_nan_output_is_an_error():
    ref = torch.ones(1, 1, 2, 4, dtype=torch.float64)
    out = ref.clone()
    out[0, 0, 1, 2] = float("nan")
    assert nerr(out, ref) == float("inf") and nerr(ref, ref) == 0.0


# ---------------------------------------------------------------- GPU tests


@pytest.fixture(scope="module")
def hip():
    from petals_amd import ops

    mod = ops._load_hip_ops()
    assert mod is not None, f"HIP extension must load on a GPU box: {ops._hip_import_error!r}"
    return mod


def _run_decode(hip, inp: Inputs, gq: int, v=None, n_splits: int = 0, nan_workspace: bool = False):
    b, h, _, hd = inp.q.shape
    kvh = inp.k.shape[1]
    q = inp.q.reshape(b, h * hd).contiguous().cuda()
    kv_len_t = torch.tensor([inp.kv_len], dtype=torch.int32, device="cuda")
    if nan_workspace:  # caller-supplied, oversize, stale: must be written before it is read
        part_o = torch.full((b * kvh * n_splits * gq * hd + 4099,), float("nan"), device="cuda")
        part_ml = torch.full((b * kvh * n_splits * gq * 2 + 131,), float("nan"), device="cuda")
    else:
        part_o = part_ml = torch.empty(0, device="cuda")
    slopes = inp.slopes.cuda() if inp.slopes is not None else None
    v = inp.v if v is None else v
    out = hip.attn_decode_fused(q, inp.k.cuda(), v.cuda(), kv_len_t, gq, n_splits, part_o, part_ml, inp.scale, slopes)
    return out.cpu().view(b, h, 1, hd)


def _decode_errors(hip, case: DecodeCase, variant: str):
    inp = decode_inputs(case, variant)
    kw = dict(n_splits=case.n_splits, nan_workspace=case.n_splits > 0)
    return (
        nerr(_run_decode(hip, inp, case.gq, **kw), inp.ref),
        nerr(_run_decode(hip, inp, case.gq, v=inp.v_nan(), **kw), inp.ref),
    )


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case,variant", DECODE_PARAMS)
def test_attn_decode_numerics(hip, case, variant):
    """MFMA decode vs float64, 1e4-poisoned and NaN-poisoned cache tails."""
    e_big, e_nan = _decode_errors(hip, case, variant)
    print(f"decode {case.id}-{variant}: nerr={e_big:.5f} (1e4 poison) {e_nan:.5f} (NaN poison) tol={TOL_DECODE}")
    assert e_big <= TOL_DECODE and e_nan <= TOL_DECODE, (e_big, e_nan)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case,pattern", PREFILL_PARAMS)
def test_attn_prefill_numerics(hip, case, pattern):
    """MFMA prefill vs float64 with diagonal / forbidden needles and poison."""
    inp = prefill_inputs(case, pattern)
    slopes = inp.slopes.cuda() if inp.slopes is not None else None
    errs = []
    for v in (inp.v, inp.v_nan()):
        out = hip.attn_prefill_fused(
            inp.q.cuda(), inp.k.cuda(), v.cuda(), inp.kv_len, inp.kv_offset, inp.scale, inp.causal, slopes
        )
        errs.append(nerr(out.cpu(), inp.ref))
    print(f"prefill {case.id}-{pattern}: nerr={errs[0]:.5f} (1e4 poison) {errs[1]:.5f} (NaN poison) tol={TOL_PREFILL}")
    assert max(errs) <= TOL_PREFILL, errs


def _ordered_bits(x_bf16):
    """bf16 bit patterns mapped to integers that are monotonic in the value, so
    a difference of 1 is one bf16 ulp (also across zero)."""
    bits = x_bf16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("kernel,hd,pos", WRITER_PARAMS)
def test_cache_writers_at_real_positions(hip, kernel, hd, pos):
    """The decode-step writers at device positions 0, 1 and lmax-1: rotated q,
    the written K/V row, every other byte of both caches, and then the
    attention over the written cache with a needle in the written row."""
    w = writer_inputs(kernel, hd, pos)
    b, qh, kh = WRITER_B, WRITER_QH, WRITER_KH
    k_cache, v_cache = w.k0.cuda(), w.v0.cuda()
    pos_t = torch.tensor([pos], dtype=torch.int32, device="cuda")
    src = w.src.cuda()
    if kernel == "rope_cache_write":
        hip.rope_cache_write(src, w.cos.cuda(), w.sin.cuda(), pos_t, k_cache, v_cache, qh, kh)
        q = src[:, : qh * hd]
    elif kernel == "kv_cache_write":
        hip.kv_cache_write(src, pos_t, k_cache, v_cache, qh, kh)
        q = src[:, : qh * hd]
    elif kernel == "qkv_rope_reduce_rope":
        q = hip.qkv_rope_reduce(src, w.cos.cuda(), w.sin.cuda(), pos_t, k_cache, v_cache, qh, kh, True, None)
    else:
        q = hip.qkv_rope_reduce(src, None, None, pos_t, k_cache, v_cache, qh, kh, False, w.bias.cuda())
    q = q.contiguous()
    k_got, v_got = k_cache.cpu(), v_cache.cpu()

    # q: a few f32 ulp of a three-term sum and one rotation, 10x margin
    q_got = q.cpu().to(torch.float64).view(b, qh, hd)
    q_err = ((q_got - w.q_ref).abs().amax(-1) / w.q_ref.abs().amax(-1)).max().item()
    assert q_err <= 1e-5, q_err
    # the written row: bf16 rounding of the reference, to within 1 bf16 ulp
    for got, ref in ((k_got, w.k_ref), (v_got, w.v_ref)):
        d = (_ordered_bits(got[:, :, pos]) - _ordered_bits(ref.to(torch.float32).to(torch.bfloat16))).abs()
        assert d.max().item() <= 1, d.max()
    # every other byte of both caches is untouched
    for got, before in ((k_got, w.k0), (v_got, w.v0)):
        rest = got.clone()
        rest[:, :, pos] = before[:, :, pos]
        assert torch.equal(rest.view(torch.int16), before.view(torch.int16))

    # writer and reader agree on the row: attention over the cache just written
    written = dataclasses.replace(w.attn, q=q.cpu().view(b, qh, 1, hd), k=k_got, v=v_got)
    errs = [
        nerr(_run_decode(hip, written, qh // kh), w.attn.ref),
        nerr(_run_decode(hip, written, qh // kh, v=written.v_nan()), w.attn.ref),
    ]
    print(f"writer {kernel}-hd{hd}-pos{pos}: q_err={q_err:.2e} attn nerr={errs[0]:.5f} {errs[1]:.5f} tol={TOL_DECODE}")
    assert max(errs) <= TOL_DECODE, errs
