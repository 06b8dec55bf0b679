"""Case lists of test_gpu_rows_shapes.py and test_gpu_rows_patterns.py (pure
Python, so test_rows_shape_cases.py checks them without a GPU).

Part 1, shapes: every instantiation of the four short-stripe ("rows") register
kernels that the launchers can pick (pick_kr over k in {2, 3, 6, 10} and 1..4
rows, read_rows_fn with 0 rows as well), each with the code and the call
arguments that reach it:

  repair  gf_crc_rows<RowsRepair<verify>, K, R, SLABS, kind>   RS(K,4), R lost and wanted units
  encode  gf_crc_rows<RowsEncode, K, R, SLABS, kind>           RS(K,R)
  scrub   gf_scrub_crc_rows<K, E, SLABS, kind>                 RS(K,4) with 4 - E parity units absent,
                                                               or RS(K,E) complete
  read    gf_read_rows<verify, K, R, SLABS, kind>              RS(K,4), R lost data units

Part 2, patterns and cuts: every set of at most m lost units of RS(3,2), RS(6,3)
and RS(10,4), and the lengths r = u * c + x of a stripe cut in unit u, x over
X(c); batches(code) puts them together, one batch per (code, cut unit) (RS(3,2):
one batch in all)."""
import itertools
from collections import namedtuple

REGISTER_K = (2, 3, 6, 10)  # the compile-time-k register kernels
ROWS = (1, 2, 3, 4)
KINDS = ("crc32c", "crc32")
KIND_ID = {"crc32c": 0, "crc32": 1}  # crc::kCrc32c, crc::kCksum as the kernel names print them
SHAPE_M = 4                 # the repair, the read and the masked scrub run RS(K, 4)
SHAPE_CELL = 9232           # two wave-tiles at SLABS 8, three at SLABS 4
SHAPE_UNIFORM_STRIPES = 3
SHAPE_MIXED_STRIPES = 12


def rows_slabs(k, r):
    """KiB of every cell per wave-tile of the repair, the encode and the read."""
    return 8 if (r <= 3 and k <= 6) else 4


def scrub_rows_slabs(k, e):
    return 8 if (e == 1 and k <= 6) else 4


RepairShape = namedtuple("RepairShape", "k m r verify kind")
EncodeShape = namedtuple("EncodeShape", "k m kind")
ScrubShape = namedtuple("ScrubShape", "k e kind")
ReadShape = namedtuple("ReadShape", "k m r verify")  # verify: "crc32c", "crc32" or None

REPAIR_SHAPES = [RepairShape(k, SHAPE_M, r, v, kind) for k in REGISTER_K for r in ROWS for v in (True, False)
                 for kind in KINDS]
ENCODE_SHAPES = [EncodeShape(k, m, kind) for k in REGISTER_K for m in ROWS for kind in KINDS]
SCRUB_SHAPES = [ScrubShape(k, e, kind) for k in REGISTER_K for e in ROWS for kind in KINDS]
READ_SHAPES = [ReadShape(k, SHAPE_M, r, v) for k in REGISTER_K for r in range(0, min(4, k) + 1)
               for v in ("crc32c", "crc32", None)]


def kernel_name(shape):
    """The template-id a kernel trace prints for the shape's register kernel."""
    if isinstance(shape, RepairShape):
        return "gf_crc_rows<hec::RowsRepair<%s>, %d, %d, %d, %d>" % (
            "true" if shape.verify else "false", shape.k, shape.r, rows_slabs(shape.k, shape.r), KIND_ID[shape.kind])
    if isinstance(shape, EncodeShape):
        return "gf_crc_rows<hec::RowsEncode, %d, %d, %d, %d>" % (shape.k, shape.m, rows_slabs(shape.k, shape.m),
                                                                  KIND_ID[shape.kind])
    if isinstance(shape, ScrubShape):
        return "gf_scrub_crc_rows<%d, %d, %d, %d>" % (shape.k, shape.e, scrub_rows_slabs(shape.k, shape.e),
                                                      KIND_ID[shape.kind])
    # without verification the launcher takes the CRC32C instantiation, whose kind is then unused
    return "gf_read_rows<%s, %d, %d, %d, %d>" % ("true" if shape.verify else "false", shape.k, shape.r,
                                                 rows_slabs(shape.k, shape.r), KIND_ID[shape.verify or "crc32c"])


def shape_id(shape):
    return "-".join(str(v) for v in shape)


# ---- lengths of the shape tests -------------------------------------------------------

def middle_unit(k):
    return max(1, k // 2)


def shape_lengths(k, cell=SHAPE_CELL):
    """r of the short stripe: the cut in a middle unit with 1, 17, 513, 4625 and
    c - 1 bytes of it, and r = 1, c, c + 1, k * c - 1."""
    cu = middle_unit(k)
    rs = [cu * cell + x for x in (1, 17, 513, 4625, cell - 1)] + [1, cell, cell + 1, k * cell - 1]
    assert all(1 <= r < k * cell for r in rs)
    return list(dict.fromkeys(rs))  # at k = 2 two of them coincide


def mixed_shape_lengths(k, cell=SHAPE_CELL, S=SHAPE_MIXED_STRIPES):
    """One length per stripe of the mixed form: shape_lengths, a full stripe
    (as 0 and as k * c) and a cut in the last unit; at k = 2 two cuts in unit 0
    make up the twelve."""
    full = k * cell
    rs = shape_lengths(k, cell) + [0, full]
    for r in ((k - 1) * cell + 4625, 17, cell - 1, 4625):
        if len(rs) < S and r not in rs:
            rs.append(r)
    assert len(rs) == S
    # large and small by turns
    return [rs[(5 * s + 2) % S] for s in range(S)]


def cut_unit(cell, r):
    return (r - 1) // cell


def nearest_data_units(k, cu, count):
    """The `count` data units nearest unit cu (the lower one first on a tie)."""
    return tuple(sorted(sorted(range(k), key=lambda u: (abs(u - cu), u))[:count]))


def repair_targets(k, m, r_rows, cu):
    """[(lost, want)] of a repair with r_rows rows: the lost units nearest the
    cut (data units while there are any, then parity units), all wanted; one
    set with a parity target; one want subset of a larger loss (none at four
    rows: RS(k,4) cannot lose five)."""
    def fill(data_count, total):
        data = nearest_data_units(k, cu, min(data_count, k))
        return tuple(sorted(data + tuple(range(k, k + total - len(data)))))
    near = fill(r_rows, r_rows)
    sets = [(near, near)]
    with_parity = fill(r_rows - 1, r_rows)
    if with_parity == near:  # already holds a parity unit: the last parity unit in place of the first
        with_parity = tuple(sorted(with_parity[:-1] + (k + m - 1,))) if with_parity[-1] != k + m - 1 else near
    sets.append((with_parity, with_parity))
    if r_rows < m:
        lost = fill(r_rows + 1, r_rows + 1)
        sets.append((lost, lost[:r_rows] if lost[r_rows] >= k else lost[1:]))
    return sets


def read_losses(k, m, r_rows, cu):
    """The r_rows lost data units nearest the cut, without and with a lost
    parity unit (no room for one at four rows)."""
    data = nearest_data_units(k, cu, r_rows)
    sets = [data]
    if r_rows < m:
        sets.append(data + (k + (cu % m),))
    return sets


def scrub_absent_sets(k, e, m=SHAPE_M):
    """The masks of RS(k, m) that leave e extras: every choice of m - e absent
    parity units, and (where e < m) unit `middle` absent with m - e - 1 parity
    units, which puts a parity unit among the survivors."""
    sets = [tuple(c) for c in itertools.combinations(range(k, k + m), m - e)]
    if e < m:
        sets += [(middle_unit(k) % k,) + tuple(c) for c in itertools.combinations(range(k, k + m), m - e - 1)]
    return sets


# ---- patterns and cuts ------------------------------------------------------------------

PATTERN_CODES = ((3, 2), (6, 3), (10, 4))
PATTERN_COUNT = {(3, 2): 16, (6, 3): 130, (10, 4): 1471}
PATTERN_CELL = {(3, 2): 9232, (6, 3): 9232, (10, 4): 4096 + 1040}
X_VALUES = (1, 15, 16, 17, 511, 512, 513, 1040, 4097, 4625, 8193, 8721)


def patterns(k, m):
    """Every set of at most m lost units, by size, then in lexical order."""
    return [tuple(c) for size in range(m + 1) for c in itertools.combinations(range(k + m), size)]


def cut_x(cell):
    """X(c): the bytes of the cut unit; x = c cuts at a unit boundary."""
    xs = sorted(set(x for x in X_VALUES + (cell - 16, cell - 1, cell) if 1 <= x <= cell))
    return xs


PatternBatch = namedtuple("PatternBatch", "k m cell cut_units rs losts")


def batch_ids(k, m):
    """The batches of a code: one per cut unit, RS(3,2) one in all."""
    return [None] if (k, m) == (3, 2) else list(range(k))


def batch(k, m, cut=None):
    """The stripes (lengths rs and lost units losts) of one batch.

    RS(3,2): every pattern x every cut unit x every x.  RS(6,3): every pattern
    x every x at cut unit `cut`.  RS(10,4): every pattern once at cut unit
    `cut`, x = X[pattern index mod |X|].  u = k - 1 with x = c is a full
    stripe and stays: it puts full and short stripes into one plan's lists."""
    cell = PATTERN_CELL[(k, m)]
    pats, xs = patterns(k, m), cut_x(cell)
    rs, losts = [], []
    if (k, m) == (3, 2):
        assert cut is None
        for p in pats:
            for u in range(k):
                for x in xs:
                    rs.append(u * cell + x)
                    losts.append(p)
        cuts = tuple(range(k))
    elif (k, m) == (6, 3):
        for p in pats:
            for x in xs:
                rs.append(cut * cell + x)
                losts.append(p)
        cuts = (cut,)
    else:
        for i, p in enumerate(pats):
            rs.append(cut * cell + xs[i % len(xs)])
            losts.append(p)
        cuts = (cut,)
    return PatternBatch(k, m, cell, cuts, rs, losts)


def all_batches():
    """[(k, m, cut)] of every batch, 17 in all."""
    return [(k, m, cut) for (k, m) in PATTERN_CODES for cut in batch_ids(k, m)]


def unit_lens(k, n, cell, r):
    """len(u) of every unit of a stripe of r logical bytes."""
    n0 = min(cell, r)
    return [min(cell, max(0, r - u * cell)) if u < k else n0 for u in range(n)]


def scrub_flips(b):
    """[(stripe, unit, byte)]: in every second stripe one byte below the length
    of one present unit, the unit and the position rotating over the stripe
    index."""
    n = b.k + b.m
    flips = []
    for s in range(1, len(b.rs), 2):
        lens = unit_lens(b.k, n, b.cell, b.rs[s])
        pres = [u for u in range(n) if u not in b.losts[s] and lens[u]]
        u = pres[(s // 2) % len(pres)]
        flips.append((s, u, (977 * (s // 2) + s // 31) % lens[u]))
    return flips
