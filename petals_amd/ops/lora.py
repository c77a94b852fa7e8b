"""LoRA inside the Llama decode kernel chain (PETALS_AMD_LORA_DECODE=fused).

Projections that share an input form a group: qkv (q | k | v), o, gateup
(gate | up), down. Under an eligible adapter a group runs

    base GEMV (RAW partials) -> hip.lora_shrink -> hip.lora_reduce

(ops/csrc/lora.hip) instead of the GEMV with its own epilogue followed by
BlockAdapter.delta in torch. `LoraPack` is what the two kernels read for one
group: the present members' A matrices stacked into `a_cat` [R, in], their B
matrices transposed and laid one after the other in `bt`, and the member table
(column range of the fused output, offset into t, rank, offset into bt, scale).
Packs are built once, at the first fused call, and cached on the BlockAdapter;
a session's first steps run eagerly before a span graph is captured, so no
capture ever builds one.
"""

from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Tuple

import torch

LORA_MAX_RANK = 64  # per projection
LORA_MAX_R = 256  # stacked ranks of a group (lora.hip's LDS t[rows][R])
LORA_MAX_ROWS = 8  # the decode GEMVs' native batch

# group -> member projection keys, in the order their columns are fused
GROUP_KEYS = {"qkv": ("q", "k", "v"), "o": ("o",), "gateup": ("gate", "up"), "down": ("down",)}


@dataclasses.dataclass
class LoraPack:
    a_cat: torch.Tensor  # [R, in] bf16
    bt: torch.Tensor  # [sum r_p * out_p] bf16: member p's B^T as [r_p, out_p] row-major
    segments: List[int]  # per member: c0, c1, t_off, rank, bt_off
    scales: List[float]  # per member


def lora_fused_eligible(fast, adapter, rows: int) -> bool:
    """Whether `fast` serves `adapter` on `rows` rows with the fused kernels:
    mode `fused`, one GPU, rows <= 8, every present rank in 1..64, at most 256
    stacked ranks per group, inputs a multiple of 8 wide, adapter tensors bf16
    on the fast path's device. Anything else keeps the torch deltas."""
    from petals_amd.ops.fused_decode import lora_decode_mode

    if lora_decode_mode() != "fused" or adapter is None:
        return False
    if fast.tp_world != 1 or not 1 <= rows <= LORA_MAX_ROWS:
        return False
    cache = adapter.__dict__.setdefault("_lora_cache", {})
    ok = cache.get(("eligible", fast.device))
    if ok is None:
        ok = cache[("eligible", fast.device)] = _adapter_fits(adapter, fast.device)
    return ok


def _adapter_fits(adapter, device) -> bool:
    for keys in GROUP_KEYS.values():
        total = 0
        for key in keys:
            entry = adapter.projections.get(key)
            if entry is None:
                continue
            a, b, _ = entry
            rank = a.shape[0]
            if not 1 <= rank <= LORA_MAX_RANK or b.shape[1] != rank or a.shape[1] % 8:
                return False
            for t in (a, b):
                if t.dtype != torch.bfloat16 or t.device != device:
                    return False
            total += rank
        if total > LORA_MAX_R:
            return False
    return True


def build_pack(adapter, members: Sequence[Tuple[str, int, int]]) -> Optional[LoraPack]:
    """members: (projection key, c0, c1) in column order. None when the adapter
    has none of them."""
    a_rows, bt_rows, segments, scales = [], [], [], []
    t_off = bt_off = 0
    for key, c0, c1 in members:
        entry = adapter.projections.get(key)
        if entry is None:
            continue
        a, b, scale = entry
        rank = a.shape[0]
        if b.shape != (c1 - c0, rank):
            raise ValueError(f"LoRA {key!r}: B is {tuple(b.shape)}, the projection wants {(c1 - c0, rank)}")
        a_rows.append(a)
        bt_rows.append(b.t().contiguous().view(-1))
        segments += [c0, c1, t_off, rank, bt_off]
        scales.append(float(scale))
        t_off += rank
        bt_off += rank * (c1 - c0)
    if not a_rows:
        return None
    return LoraPack(torch.cat(a_rows, 0).contiguous(), torch.cat(bt_rows).contiguous(), segments, scales)


def get_pack(fast, adapter, group: str, members: Sequence[Tuple[str, int, int]]) -> Optional[LoraPack]:
    """The (fast path, adapter, group) pack, built at the first call."""
    cache = adapter.__dict__.setdefault("_lora_cache", {})
    key = (id(fast), group)
    if key not in cache:
        cache[key] = build_pack(adapter, members)
    return cache[key]
