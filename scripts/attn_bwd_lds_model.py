"""LDS address model for attn_bwd.hip (docs/KERNELS.md, "Training attention";
sibling of gemm_quant_lds_model.py: wide LDS ops are checked for injectivity
and per-instruction bank multiplicity before they run).

Images, for a staged tile of T rows (keys in the dQ pass, q rows in the dK/dV
pass) and head dim HD:
  row-major   [T][HD + 8] bf16           byte = row * (HD + 8) * 2 + dim * 2
  transposed  [HD][T + 8] bf16, swizzled byte = (dim * (T + 8) * 2 + row * 2) ^ (((dim >> 3) & 7) << 4)
  scratch     [16][T + 8] bf16 per wave  byte = r * (T + 8) * 2 + c * 2

Checked accesses, one wave-instruction each:
  stage   ds_write_b128 (row-major)  row = idx / (HD/8), chunk = idx % (HD/8)
  stage   ds_write_b16  (transposed) dim = chunk * 8 + e, same (row, chunk)
  B frag  ds_read_b128  (row-major)  row = nb*16 + (lane&15), dim = kc*32 + (lane>>4)*8
  B frag  ds_read_b128  (transposed) dim = d*16 + (lane&15),  row = pk*32 + (lane>>4)*8
  scratch ds_write_b16  r = (lane>>4)*4 + rr, c = nb*16 + (lane&15)
  A frag  ds_read_b128  (scratch)    r = lane&15, c = pk*32 + (lane>>4)*8

Bank rules as in gemm_quant_lds_model.py: ds_write_b128 in 8 groups of 8
contiguous lanes over 32 dword banks, ds_read_b128 in 4 interleaved groups of
16 over 64 banks; ds_write_b16 is taken as the whole wave over 32 banks (two
lanes per bank is its floor). Prints the worst number of distinct dwords per
bank per group (1 = conflict-free, 2 = the b16 floor)."""

from gemm_quant_lds_model import worst

G8 = [list(range(i, i + 8)) for i in range(0, 64, 8)]
G64 = [list(range(64))]
RD = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
]
RD += [[l + 32 for l in g] for g in RD]


def rm_byte(hd, row, dim):
    return row * (hd + 8) * 2 + dim * 2


def tr_byte(t, dim, row_byte):
    return (dim * (t + 8) * 2 + row_byte) ^ (((dim >> 3) & 7) << 4)


def check(hd, t):
    size = hd * (t + 8) * 2
    seen = set()
    for dim in range(hd):
        for row in range(t):
            a = tr_byte(t, dim, row * 2)
            assert 0 <= a and a + 2 <= size and a not in seen, (hd, t, dim, row, a)
            seen.add(a)
        for rb in range(0, t * 2, 16):  # a 16-byte read stays one aligned 16-byte cell
            a = tr_byte(t, dim, rb)
            assert a % 16 == 0 and all(tr_byte(t, dim, rb + 2 * i) == a + 2 * i for i in range(8))
    res = {}

    def put(name, w):
        res[name] = max(res.get(name, 0), w)

    cpr = hd // 8  # 16-byte chunks per row
    for it in range(t * cpr // 256):
        for wave in range(4):
            idx = lambda l: it * 256 + wave * 64 + l
            put("stage row-major ds_write_b128",
                worst(G8, lambda l: rm_byte(hd, idx(l) // cpr, (idx(l) % cpr) * 8), 16, 32))
            for e in range(8):
                put("stage transposed ds_write_b16",
                    worst(G64, lambda l: tr_byte(t, (idx(l) % cpr) * 8 + e, (idx(l) // cpr) * 2), 4, 32))
    for nb in range(t // 16):
        for kc in range(hd // 32):
            put("row-major B ds_read_b128",
                worst(RD, lambda l: rm_byte(hd, nb * 16 + (l & 15), kc * 32 + (l >> 4) * 8), 16, 64))
    for d in range(hd // 16):
        for pk in range(t // 32):
            put("transposed B ds_read_b128",
                worst(RD, lambda l: tr_byte(t, d * 16 + (l & 15), pk * 64 + (l >> 4) * 16), 16, 64))
    sp = (t + 8) * 2
    for rr in range(4):
        for nb in range(t // 16):
            put("scratch ds_write_b16",
                worst(G64, lambda l: ((l >> 4) * 4 + rr) * sp + (nb * 16 + (l & 15)) * 2, 4, 32))
    for pk in range(t // 32):
        put("scratch A ds_read_b128", worst(RD, lambda l: (l & 15) * sp + pk * 64 + (l >> 4) * 16, 16, 64))
    print(f"HD {hd} T {t}: transposed image injective, {len(seen)} cells inside {size} B")
    for k, v in res.items():
        print(f"  {k}: worst {v}")


if __name__ == "__main__":
    for hd in (64, 128):
        check(hd, 64)  # dQ pass: 64-key tiles
        check(hd, 32)  # dK/dV pass: 32-row q tiles
