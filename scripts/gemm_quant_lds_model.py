"""LDS address model for gemm_quant.hip (docs/KERNELS.md, "Cross-cutting
rules": wide LDS ops are checked for injectivity and per-instruction bank
multiplicity before they run).

Image: [row][k] tile, 128-byte rows, the eight 16-byte chunks of a row
XOR-permuted by row & 7 (GQ_BYTE). Checked accesses, one wave-instruction each:
  A stage  ds_write_b128  row = tid>>3 (+32*i), chunk = tid&7
  B stage  ds_write_b64   column = (tid>>4)*8 + v, k quad = tid&15
  fragment ds_read_b128   row = base + (lane&15), k byte = kc*64 + (lane>>4)*16

Bank rules (CDNA4 LDS): ds_write_b64 is served in 4 groups of 16 contiguous
lanes over 32 dword banks, ds_write_b128 in 8 groups of 8 over 32 banks,
ds_read_b128 in 4 groups of 16 (the interleaved lane sets below) over 64
banks. Prints the worst number of distinct addresses per bank per group
(1 = conflict-free)."""

ROWB = 128
ROWS = 128


def gq_byte(r, kb):
    return r * ROWB + (kb ^ ((r & 7) << 4))


def worst(groups, addr_of, width, banks):
    w = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            a = addr_of(lane)
            for d in range(width // 4):
                per_bank.setdefault(((a // 4) + d) % banks, set()).add(a // 4 + d)
        w = max(w, max(len(v) for v in per_bank.values()))
    return w


def main():
    # injectivity + bounds over every 8-byte cell the kernel writes
    seen = set()
    for r in range(ROWS):
        for kb in range(0, 128, 8):
            a = gq_byte(r, kb)
            assert 0 <= a and a + 8 <= ROWS * ROWB, (r, kb, a)
            assert a % 8 == 0 and a not in seen, (r, kb, a)
            seen.add(a)
    # a 16-byte access stays one aligned 16-byte cell
    for r in range(ROWS):
        for kb in range(0, 128, 16):
            assert gq_byte(r, kb) % 16 == 0 and gq_byte(r, kb + 8) == gq_byte(r, kb) + 8
    print(f"injective: {len(seen)} 8-byte cells inside {ROWS * ROWB} B")

    g16 = [list(range(i, i + 16)) for i in range(0, 64, 16)]
    g8 = [list(range(i, i + 8)) for i in range(0, 64, 8)]
    rd = [
        [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
        [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    ]
    rd += [[l + 32 for l in g] for g in rd]

    res = {}
    for wave in range(4):
        for i in range(4):
            res["A ds_write_b128"] = max(res.get("A ds_write_b128", 0), worst(
                g8, lambda l: gq_byte(((wave * 64 + l) >> 3) + 32 * i, ((wave * 64 + l) & 7) * 16), 16, 32))
        for v in range(8):
            res["B ds_write_b64"] = max(res.get("B ds_write_b64", 0), worst(
                g16, lambda l: gq_byte(((wave * 64 + l) >> 4) * 8 + v, ((wave * 64 + l) & 15) * 8), 8, 32))
    for base in range(0, ROWS, 16):
        for kc in range(2):
            res["frag ds_read_b128"] = max(res.get("frag ds_read_b128", 0), worst(
                rd, lambda l: gq_byte(base + (l & 15), kc * 64 + (l >> 4) * 16), 16, 64))
    for k, v in res.items():
        print(f"{k}: worst {v} address(es) per bank per lane group")


if __name__ == "__main__":
    main()
