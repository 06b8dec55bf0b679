"""Case generators of test_gpu_coding_launch.py and coding_fixed_order_child.py
(numpy and the oracle only, so test_coding_launch_cases.py checks them without a
GPU).

Part 1, every GF(2^8) product in every byte lane: product_matrices(k, r) is a
series of r x k matrices whose entries together take every value 0..255, and
product_cells gives inputs in which every 16-byte block position sees every
byte value, so every (coefficient, byte) pair and with it every entry of the
three v_perm product tables (x & 7, (x >> 3) & 7, x >> 6) is used in every byte
lane of a dword.  The expected outputs come from ec_oracle.matmul_shards.

Part 2, small launches: tile_count_cases(k, cus) lists (stripes, cell) pairs
whose wave-tile counts T = stripes * ceil(cell / W) sit on every branch of the
work queue's deal (tile = round * n + counter, n = min(grid, 8), grid =
min(CUs, T); two rounds per atomic at k = 2 and 3), ordered so that large and
tiny launches alternate."""
import functools

import numpy as np

import ec_oracle as O

PRODUCT_K = (2, 3, 6, 10)       # the compile-time-k register kernels
RUNTIME_K = (5, 12)             # the runtime-k kernel (256- and 512-thread blocks)
PRODUCT_R = (1, 2, 3, 4)
PRODUCT_CELL = 4096             # one wave-tile at k <= 6, two at k = 10
PRODUCT_STRIPES = 2
UNALIGNED_CELL = 4096 + 13      # the dword kernel up to 4104, the byte kernel behind it
BYTE_CELL = 7                   # the byte kernel alone
PITCH_GAP = 64                  # rows have a pitch of cell + 64
RS = {2: 1, 3: 2, 6: 3, 10: 4}  # the RS m of each register-kernel k


def wave_tile_bytes(k):
    """Bytes of a cell one wave-tile of the queue kernel covers (64 lanes x U x 16)."""
    return 4096 if k <= 6 else 2048


def product_matrices(k, r):
    """M_t[j][i] = (t*r*k + j*k + i) mod 256 for t < ceil(256 / (r*k))."""
    count = -(-256 // (r * k))
    return [[[(t * r * k + j * k + i) % 256 for i in range(k)] for j in range(r)] for t in range(count)]


def product_cell(i, stripe=0, rep=0, cell=PRODUCT_CELL):
    """cell[16*v + p] = (v + 17*p + 29*i + 101*stripe + 53*rep) mod 256: over
    any 4096 consecutive bytes every block position p sees every byte value."""
    x = np.arange(cell, dtype=np.int64)
    return ((x // 16 + 17 * (x % 16) + 29 * i + 101 * stripe + 53 * rep) % 256).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def product_cells(k, route="aligned", rep=0):
    """The inputs of a route as a read-only [S, k, cell] array.  "aligned" and
    "unaligned": PRODUCT_STRIPES stripes of 4096 / 4109 bytes; "bytes": the 4096
    bytes of stripe 0 cut into 7-byte cells, one stripe each (the last one
    runs on into the pattern), so the byte kernel still sees every value."""
    if route == "bytes":
        stripes = -(-PRODUCT_CELL // BYTE_CELL)
        out = np.stack([product_cell(i, 0, rep, stripes * BYTE_CELL).reshape(stripes, BYTE_CELL) for i in range(k)],
                       axis=1)
    else:
        cell = UNALIGNED_CELL if route == "unaligned" else PRODUCT_CELL
        out = np.stack([np.stack([product_cell(i, s, rep, cell) for i in range(k)]) for s in range(PRODUCT_STRIPES)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def product_expected(k, r, route="aligned", rep=0):
    """matmul_shards of every matrix of the series over product_cells: a
    read-only [matrices, S, r, cell] array, computed once per process."""
    cells = product_cells(k, route, rep)
    S, _, cell = cells.shape
    flat = [np.ascontiguousarray(cells[:, i]).reshape(-1) for i in range(k)]
    mats = product_matrices(k, r)
    out = np.empty((len(mats), S, r, cell), dtype=np.uint8)
    for t, mat in enumerate(mats):
        for j, row in enumerate(O.matmul_shards(mat, flat)):
            out[t, :, j] = row.reshape(S, cell)
    out.setflags(write=False)
    return out


# ---- part 2 ---------------------------------------------------------------------------

SMALL_T = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33)
GRAPH_T = ("1", "7", "9", "cus+1")  # the tile counts of the captured sequence
FIXED_ORDER_T = (1, 9)              # the tile counts of the fixed-order child


def tile_counts(cus):
    """Every T the issue names, in ascending order, with the name of each
    CU-relative one (a T that is both keeps its plain number)."""
    named = {t: str(t) for t in SMALL_T}
    for name, t in (("cus-1", cus - 1), ("cus", cus), ("cus+1", cus + 1), ("2cus+3", 2 * cus + 3)):
        if t >= 1:
            named.setdefault(t, name)
    return sorted(named.items())


def tile_count_cases(k, cus):
    """[(T, stripes, cell, tag)] for RS(k, RS[k]).  Every T up to 17 comes in
    every split S x tiles-per-stripe with 1, 2, 3 or 5 tiles per stripe (so S
    takes 1, 2, 3, 5, 7 and groups of 4 stripes leave every remainder), larger T
    in the split with the most tiles per stripe; the last tile of a cell is 16
    bytes, W - 16 bytes or full by rotation.  Ordered largest, smallest, second
    largest, second smallest, ..."""
    W = wave_tile_bytes(k)
    cases = []
    for T, name in tile_counts(cus):
        splits = [tps for tps in (1, 2, 3, 5) if T % tps == 0]
        if T > 17:
            splits = splits[-1:]
        for tps in splits:
            last = (16, W - 16, W)[len(cases) % 3]
            cases.append((T, T // tps, (tps - 1) * W + last, name))
    cases.sort(key=lambda c: (c[0], c[1]))
    order = []
    lo, hi = 0, len(cases) - 1
    while lo <= hi:
        order.append(cases[hi])
        if lo < hi:
            order.append(cases[lo])
        lo, hi = lo + 1, hi - 1
    return order


def case_tiles(k, stripes, cell):
    return stripes * -(-cell // wave_tile_bytes(k))


def mixed_masks(k, m, stripes):
    """Three presence masks by rotation over the stripes: data unit 0 lost; data
    unit 1 and parity unit 0 lost; the first m data units lost."""
    full = (1 << (k + m)) - 1
    three = (full & ~1, full & ~(1 << 1) & ~(1 << k), full & ~((1 << m) - 1))
    return [three[s % 3] for s in range(stripes)]


def rs_data(k, stripes, cell, seed):
    """Random data of a batch, [stripes, k, cell]."""
    return np.random.default_rng(seed).integers(0, 256, size=(stripes, k, cell), dtype=np.uint8)
