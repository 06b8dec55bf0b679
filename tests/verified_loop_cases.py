"""Case lists of test_gpu_verified_loops.py (pure Python, so
test_verified_loop_cases.py checks them without a GPU): launches of the register
kernels behind the verified calls in which a block goes round its tile loop
`for (tile = blockIdx.x; tile < total; tile += gridDim.x)` a second time.

The families, by kernel:

  recon        gf_reconstruct_crc<K, R, SLABS, KIND, VERIFY_IN, true>    ec_reconstruct_crc.hip
  sums         the same with STORE_OUT = false                            ec_reconstruct_sums.hip
  scrub        gf_scrub_crc<K, E, SLABS, KIND>                            ec_scrub_crc.hip
  repair_rows  gf_crc_rows<RowsRepair<VERIFY_IN>, K, R, SLABS, KIND>      ec_reconstruct_rows.hip
  encode_rows  gf_crc_rows<RowsEncode, K, R, SLABS, KIND>                 ec_encode_rows.hip
  scrub_rows   gf_scrub_crc_rows<K, E, SLABS, KIND>                       ec_scrub_rows.hip
  read_rows    gf_read_rows<VERIFY_IN, K, R, SLABS, KIND>                 ec_read_rows.hip

Part 1 is a model of the launchers' tile arithmetic (tile_geometry, tile_order,
tile_coords): block_tiles() says which block takes which (launch stripe, tile
column), in which order.  Everything the GPU cases claim about their own inputs
(every block loops, a flip lies in a second or later tile, a short tile is
followed by a full one) is asserted from it, not assumed from the queue order.

Part A: the product library on its default grid.  The tile count exceeds the
grid because the stripe count does: S follows from the device's CU count.
Part B: the measurement build with a grid of 1 and 5 blocks (tune key 7) and
tile-order groups of 8 (the default), 1 and 3 stripes (tune key 8): small
batches of multi-tile cells."""
import collections

import rows_shape_cases as P

GROUP = 8                       # set_tile_order(a, tn, 8u) in every launcher of these kernels
CU_COUNTS = (64, 256)           # the smallest CU count worth supporting, and the MI355X
CELL_BYTES_LIMIT = 256 << 20    # of one batch's cell buffer
FAMILIES = ("recon", "sums", "scrub", "repair_rows", "encode_rows", "scrub_rows", "read_rows")


# ---- the launchers' rules, restated -----------------------------------------------------

def recon_crc_slabs(k, r):
    """recon_crc_slabs (ec_reconstruct_crc_kernel.hpp): launch_reconstruct_crc, launch_reconstruct_sums."""
    return 8 if (r <= 3 and k <= 6) else 4


def scrub_crc_slabs(k, e):
    """scrub_crc_slabs (ec_scrub_crc.hip): launch_scrub_crc."""
    return 8 if (e == 1 and k <= 6) else 4


rows_slabs = P.rows_slabs               # rows_slabs (ec_rows_kernel.hpp): the repair, the encode and the read
scrub_rows_slabs = P.scrub_rows_slabs   # scrub_rows_slabs (ec_rows_kernel.hpp): the rows scrub


def blocks_per_cu(family, with_list=False):
    """The default grid of a launch, in blocks per CU: launch_reconstruct_crc,
    launch_reconstruct_sums, launch_read_rows and the grid_per_cu that the
    repair and the encode pass to launch_rows_crc: 32.  launch_scrub_crc and
    the grid_per_cu of the rows scrub: `cs.stripe_list ? 2 : 4`."""
    if family in ("scrub", "scrub_rows"):
        return 2 if with_list else 4
    return 32


def rows_of(family, k, m, lost):
    """The kernel's second template argument for a code RS(k, m) with the units
    `lost` absent (and, for the repair, all wanted)."""
    if family in ("recon", "sums", "repair_rows"):
        return len(lost)
    if family in ("scrub", "scrub_rows"):
        return k + m - len(lost) - k    # the extras: present units past the first k
    if family == "encode_rows":
        return m
    return sum(1 for u in lost if u < k)  # read_rows: the lost data units


def tile_bytes(family, k, m, lost=()):
    """4096 * SLABS: four waves of SLABS KiB."""
    r = rows_of(family, k, m, lost)
    if family in ("recon", "sums"):
        return 4096 * recon_crc_slabs(k, r)
    if family == "scrub":
        return 4096 * scrub_crc_slabs(k, r)
    if family == "scrub_rows":
        return 4096 * scrub_rows_slabs(k, r)
    return 4096 * rows_slabs(k, r)


# ---- part 1: the model ------------------------------------------------------------------

def tile_geometry(stripes, cell_len, tile):
    """(tiles_per_stripe, total_tiles) of launch_parts.hpp tile_geometry."""
    tps = -(-cell_len // tile)
    return tps, tps * stripes


def tile_order(stripes, tps, want):
    """(group, grouped_tiles) of gf_device.hpp tile_order."""
    group = 1 if want < 1 else (max(stripes, 1) if stripes < want else want)
    return group, (stripes // group) * group * tps


def tile_coords(tile, tps, group, grouped):
    """(launch stripe, tile column) of gf_device.hpp tile_coords."""
    if group <= 1 or tile >= grouped:
        return tile // tps, tile % tps
    g, r = divmod(tile, group * tps)
    tcol = r // group
    return g * group + (r - tcol * group), tcol


def block_tiles(stripes, cell_len, tile, group, grid):
    """Every block's [(launch stripe, tile column)] in the order it takes them:
    the launchers clamp the grid to the tile count, block b takes tiles b,
    b + grid, ..."""
    tps, total = tile_geometry(stripes, cell_len, tile)
    g, grouped = tile_order(stripes, tps, group)
    n = min(grid, total)
    return [[tile_coords(t, tps, g, grouped) for t in range(b, total, n)] for b in range(n)]


def tile_len(length, tile, tcol):
    """Bytes of tile column tcol below `length` (0: the tile lies past the end)."""
    return max(0, min(tile, length - tcol * tile))


def wave_live(length, tile, tcol, wave):
    """Does wave `wave` of a block work in this tile, or `continue`?"""
    return tcol * tile + wave * (tile // 4) < length


def late_tiles(blocks):
    """[(launch stripe, tile column)] of every block's second and later tiles."""
    return [t for b in blocks for t in b[1:]]


def spread(items, count):
    """`count` of items: the first, the last, the rest evenly between."""
    if len(items) <= count:
        return list(items)
    return [items[(len(items) - 1) * x // (count - 1)] for x in range(count)]


def list_layout(n_main):
    """A batch in which the stripes of one pattern are no run: every stripe s
    with s % 16 == 5 belongs to another pattern.  Returns (S, main) with
    main[launch stripe] = batch stripe, len(main) == n_main."""
    main, s = [], 0
    while len(main) < n_main:
        if s % 16 != 5:
            main.append(s)
        s += 1
    return s, main


# ---- lengths of short stripes -----------------------------------------------------------

def short_kinds(k, cell, tile):
    """r of a stripe that ends in unit 0 (inside the cell's last tile, mid-chunk),
    mid-chunk in a middle unit, one byte short of full; `tile` = the bytes of
    the cell in front of its last tile."""
    head = (-(-cell // tile) - 1) * tile
    return [head + 300, P.middle_unit(k) * cell + head + 200, k * cell - 1]


def n0_of(cell, r):
    return min(cell, r)


# ---- part A -----------------------------------------------------------------------------

ReconA = collections.namedtuple("ReconA", "family name k m lost other cell form expected ctype")
RowsA = collections.namedtuple("RowsA", "family name k m lost cell form which ctype")
ScrubA = collections.namedtuple("ScrubA", "family name k m absent form ctype")

EXTRA_STRIPES = 37


def recon_stripes(cus):
    """Stripes of the pattern under test: single-tile cells, 37 tiles past the grid."""
    return 32 * cus + EXTRA_STRIPES


def _rec(family, k, m, lost, other, cell, form, expected, ctype="crc32c"):
    name = "%s-rs%d.%d-r%d-c%d-%s-%s-%s" % (family, k, m, len(lost), cell, form, "exp" if expected else "noexp", ctype)
    return ReconA(family, name, k, m, tuple(lost), tuple(other), cell, form, expected, ctype)


# 528 B: wave 0 holds one full chunk and a 16-B chunk, waves 1 to 3 skip.  4624 B at 4 slabs:
# wave 0 full, wave 1 short.  RS(10,4) with 4 units lost is the 4-slab kernel without register
# prefetch (R * SLABS <= 24 fails only at 8 slabs; R = 4 never has 8).  Its 14 units at 4624 B
# and 8229 stripes are 533 MB, over the limit, so the 4624-byte cell runs the 4-slab kernel of
# fewest units instead, RS(2,4) with 4 lost (6 units, 228 MB at 256 CUs).
RECON_A = [
    _rec("recon", 2, 1, (0,), (2,), 528, "uniform", True),
    _rec("recon", 6, 3, (1, 7), (0,), 528, "uniform", False),
    _rec("recon", 6, 3, (1, 7), (0,), 528, "mixed", True, "crc32"),
    _rec("recon", 6, 3, (0, 4, 8), (2,), 528, "mixed", True),
    _rec("recon", 10, 4, (0, 5, 9, 12), (3, 13), 528, "mixed", False),
    _rec("recon", 10, 4, (0, 5, 9, 12), (3, 13), 528, "uniform", True),
    _rec("recon", 2, 4, (0, 2, 3, 5), (1,), 4624, "uniform", True),
    _rec("sums", 2, 1, (1,), (0,), 528, "mixed", True),
    _rec("sums", 6, 3, (1, 7), (0,), 528, "uniform", True, "crc32"),
    _rec("sums", 6, 3, (1, 7), (0,), 528, "mixed", False),
    _rec("sums", 10, 4, (0, 5, 9, 12), (3, 13), 528, "mixed", True),
    _rec("sums", 2, 4, (0, 2, 3, 5), (1,), 4624, "uniform", True),
]


def recon_batch(case, cus):
    """(S, main) of a Part-A reconstruction batch: uniform calls run S stripes
    of one pattern; mixed calls interleave stripes of `other` and complete
    stripes (list_layout), so the pattern's launch reads a stripe list."""
    n = recon_stripes(cus)
    if case.form == "uniform":
        return n, list(range(n))
    return list_layout(n)


def recon_losts(case, S, main):
    """The lost units of every batch stripe: the case's pattern at the main
    stripes; the others lose `other` and nothing by turns."""
    losts = [()] * S
    for s in main:
        losts[s] = case.lost
    rest = [s for s in range(S) if losts[s] == ()]
    for x, s in enumerate(rest):
        losts[s] = case.other if x % 2 == 0 else ()
    return losts


def survivors(n, k, lost):
    return [u for u in range(n) if u not in lost][:k]


def late_flips(blocks, main, surv, length_of, tile, count=3):
    """[(batch stripe, unit, byte)]: one bent byte in each of `count` second or
    later tiles (spread over the launch), in a survivor that rotates, at byte
    3 of the tile, at its last byte and in its middle by turns.  length_of(launch
    stripe, unit) = the bytes of that cell that count."""
    late = [t for t in late_tiles(blocks) if tile_len(length_of(t[0], surv[0]), tile, t[1]) > 0]
    flips = []
    for x, (ls, tcol) in enumerate(spread(late, count)):
        units = [u for u in surv if tile_len(length_of(ls, u), tile, tcol) > 0]
        unit = units[(len(units) - 1) * (x % 2)] if x < 2 else units[x % len(units)]
        n = tile_len(length_of(ls, unit), tile, tcol)
        flips.append((main[ls], unit, tcol * tile + (3 % n, n - 1, n // 2)[x % 3]))
    return flips


def flip_tile(flip, main, tile):
    """(launch stripe, tile column) that holds a flip of late_flips."""
    s, _, byte = flip
    return main.index(s), byte // tile


def recon_flips(case, cus):
    S, main = recon_batch(case, cus)
    tile = tile_bytes(case.family, case.k, case.m, case.lost)
    blocks = block_tiles(len(main), case.cell, tile, GROUP, 32 * cus)
    return late_flips(blocks, main, survivors(case.k + case.m, case.k, case.lost), lambda ls, u: case.cell, tile)


# The rows kernels: more short stripes than the grid, every stripe one tile (cell 528 B), the
# three lengths of short_kinds rotating so that the consecutive tiles of a block differ
# (rows_lengths).  form "mixed": one length per stripe (stripe_bytes), all short, so that the
# rows kernel's one launch holds them all.  form "data_len": S - 1 full stripes and the last
# one short, length number `which`; the full stripes go to the full-stripe kernel of the call,
# which then loops, and the short one is the rows kernel's single stripe.
ROWS_CELL = 528


def _rows(family, k, m, lost, form, which=0, ctype="crc32c"):
    name = "%s-rs%d.%d-%s%s-%s" % (family, k, m, form, "-len%d" % which if form == "data_len" else "", ctype)
    return RowsA(family, name, k, m, tuple(lost), ROWS_CELL, form, which, ctype)


ROWS_A = []
for _family, _k, _m, _lost in (("repair_rows", 6, 3, (1, 7)), ("encode_rows", 6, 3, ()), ("read_rows", 6, 3, (2, 4)),
                               ("scrub_rows", 6, 3, ())):
    ROWS_A.append(_rows(_family, _k, _m, _lost, "mixed"))
    ROWS_A += [_rows(_family, _k, _m, _lost, "data_len", w) for w in range(3)]
ROWS_A += [_rows("repair_rows", 10, 4, (0, 5, 9, 12), "mixed", ctype="crc32"),
           _rows("encode_rows", 10, 4, (), "mixed", ctype="crc32"),
           _rows("read_rows", 10, 4, (0, 5, 9), "mixed", ctype="crc32"),
           _rows("scrub_rows", 6, 3, (1,), "mixed", ctype="crc32")]
# the rows scrub once more with the two-tile cells of the scrub cases below (tile + 528 B): every
# length ends in the second tile, so both tiles of every stripe are live
for _lost, _ctype in (((), "crc32"), ((1,), "crc32c")):
    _cell = tile_bytes("scrub_rows", 6, 3, _lost) + 528
    _name = "scrub_rows-rs6.3-e%d-c%d-mixed-%s" % (3 - len(_lost), _cell, _ctype)
    ROWS_A.append(RowsA("scrub_rows", _name, 6, 3, _lost, _cell, "mixed", 0, _ctype))


def rows_grid(case, cus):
    return blocks_per_cu(case.family, with_list=case.form == "mixed" and case.family == "scrub_rows") * cus


def rows_stripes(case, cus):
    """37 tiles past the grid (38 with two-tile cells)."""
    tps = tile_geometry(1, case.cell, tile_bytes(case.family, case.k, case.m, case.lost))[0]
    return -(-(rows_grid(case, cus) + EXTRA_STRIPES) // tps)


def rows_lengths(case, cus):
    """rs of the batch.  mixed: tile t of a one-tile-per-stripe launch is stripe
    t, block t % grid takes it as its (t // grid)-th: the kind is their sum mod
    3, so a block's consecutive tiles never share a length.  With two-tile
    cells the model's lists decide."""
    k, cell, S, grid = case.k, case.cell, rows_stripes(case, cus), rows_grid(case, cus)
    kinds = short_kinds(k, cell, tile_bytes(case.family, k, case.m, case.lost))
    if case.form == "data_len":
        return [k * cell] * (S - 1) + [kinds[case.which]]
    tile = tile_bytes(case.family, k, case.m, case.lost)
    if cell > tile:  # two tiles a stripe: the first kind that no neighbour in a block's list has yet
        near = collections.defaultdict(set)
        for tiles in block_tiles(S, cell, tile, GROUP, grid):
            for (a, _), (b, _) in zip(tiles, tiles[1:]):
                near[a].add(b)
                near[b].add(a)
        pick = {}
        for s in range(S):
            taken = {pick[t] for t in near[s] if t in pick}
            pick[s] = next(x for x in ((s + i) % 3 for i in range(3)) if x not in taken)
        return [kinds[pick[s]] for s in range(S)]
    return [kinds[(s % grid + s // grid) % 3] for s in range(S)]


def rows_flips(case, cus, count=3):
    """Bent survivor bytes of a mixed batch, below their unit's length."""
    k, n = case.k, case.k + case.m
    rs = rows_lengths(case, cus)
    tile = tile_bytes(case.family, k, case.m, case.lost)
    blocks = block_tiles(len(rs), case.cell, tile, GROUP, rows_grid(case, cus))
    surv = survivors(n, k, case.lost) if case.family != "scrub_rows" else [u for u in range(n) if u not in case.lost]
    return late_flips(blocks, list(range(len(rs))), surv, lambda ls, u: P.unit_lens(k, n, case.cell, rs[ls])[u], tile,
                      count)


# gf_scrub_crc: two-tile cells of tile + 528 B.  uniform: 2 CUs + 19 stripes, 4 CUs + 38 tiles on
# 4 CUs blocks; degraded: CUs + 19 stripes of one mask behind a stripe list (list_layout; the
# other stripes are complete), 2 CUs + 38 tiles on 2 CUs blocks.
def _scrub(k, m, absent, form, ctype="crc32c"):
    name = "scrub-rs%d.%d-e%d-%s-%s" % (k, m, m - len(absent), form, ctype)
    return ScrubA("scrub", name, k, m, tuple(absent), form, ctype)


SCRUB_A = [_scrub(6, 3, (), "uniform"), _scrub(2, 1, (), "uniform", "crc32"), _scrub(6, 3, (1,), "degraded"),
           _scrub(10, 4, (2, 11), "degraded", "crc32")]


def scrub_cell(case):
    return tile_bytes(case.family, case.k, case.m, case.absent) + 528


def scrub_grid(case, cus):
    return blocks_per_cu(case.family, with_list=case.form == "degraded") * cus


def scrub_batch(case, cus):
    """(S, main): the stripes of the launch under test, 38 tiles past its grid."""
    n = scrub_grid(case, cus) // 2 + 19
    if case.form == "uniform":
        return n, list(range(n))
    return list_layout(n)


Corruption = collections.namedtuple("Corruption", "stripe unit byte silent")


def scrub_corruptions(blocks, main, units, cell, tile):
    """Three launch stripes whose tiles are all some block's second or later
    tile: a silent flip in tile column 1 of the first, a checksum-visible flip
    in tile column 0 of the second, both in the third (silent in column 0,
    visible in column 1, two units).  units: the present units."""
    late = set(late_tiles(blocks))
    tps = -(-cell // tile)
    whole = [ls for ls in range(len(main)) if all((ls, c) in late for c in range(tps))]
    a, b, c = spread(whole, 3)
    last = tps - 1
    return [Corruption(main[a], units[0], last * tile + 17, True),
            Corruption(main[b], units[-1], 700, False),
            Corruption(main[c], units[1 % len(units)], 513, True),
            Corruption(main[c], units[-1], cell - 3, False)]


def scrub_case_corruptions(case, cus):
    S, main = scrub_batch(case, cus)
    cell, tile = scrub_cell(case), tile_bytes(case.family, case.k, case.m, case.absent)
    blocks = block_tiles(len(main), cell, tile, GROUP, scrub_grid(case, cus))
    units = [u for u in range(case.k + case.m) if u not in case.absent]
    return scrub_corruptions(blocks, main, units, cell, tile)


def rows_scrub_corruptions(blocks, rs, k, n, cell, tile, absent):
    """The corruptions of a rows-scrub batch with the lengths rs, every one in a
    tile that is some block's second or later: ([Corruption], (stripe, unit,
    byte)).  A silent flip near the end of the last parity unit of one stripe,
    a checksum-visible flip at byte 100 of the first unit of another, both in a
    third (silent at byte 100 of the first unit, visible near the end of the
    last: with a stripe of two or more live tiles that is two tile columns),
    and in a fourth stripe the expected sum of the chunk that holds the byte
    returned last, wrong.  The first unit is unit 0, or the first parity unit
    where unit 0 is absent: both hold n0 bytes, like the last parity unit."""
    late = set(late_tiles(blocks))
    first, last = (0 if 0 not in absent else k), n - 1
    assert first not in absent and last not in absent and first != last

    def n0(ls):
        return n0_of(cell, rs[ls])

    def cols(ls):
        return (n0(ls) - 1) // tile + 1

    whole = [ls for ls in range(len(rs)) if all((ls, c) in late for c in range(cols(ls)))]
    many = [ls for ls in whole if cols(ls) > 1] or whole
    c = many[len(many) // 2]
    a, b, d = spread([ls for ls in whole if ls != c], 3)
    found = [Corruption(a, last, n0(a) - 3, True), Corruption(b, first, 100, False),
             Corruption(c, first, 100, True), Corruption(c, last, n0(c) - 3, False)]
    return found, (d, last, n0(d) - 1)


def rows_scrub_case_corruptions(case, cus):
    rs = rows_lengths(case, cus)
    tile = tile_bytes(case.family, case.k, case.m, case.lost)
    blocks = block_tiles(len(rs), case.cell, tile, GROUP, rows_grid(case, cus))
    return rows_scrub_corruptions(blocks, rs, case.k, case.k + case.m, case.cell, tile, case.lost)


def merging_blocks(blocks):
    """The blocks that take two tiles of one launch stripe (a scrub block then
    merges that stripe's findings twice)."""
    out = []
    for b, tiles in enumerate(blocks):
        stripes = [ls for ls, _ in tiles]
        if len(set(stripes)) < len(stripes):
            out.append(b)
    return out


# ---- part B -----------------------------------------------------------------------------

LoopB = collections.namedtuple("LoopB", "family name k m lost S cell grid group ctype verify")
BLOCK_GRIDS = (1, 5)            # tune key 7
ORDER_GROUPS = (0, 1, 3)        # tune key 8; 0 = the launcher's default, 8


def _loop(family, k, m, lost, S, long_cell, grid, group=0, ctype="crc32c", verify=True):
    tile = tile_bytes(family, k, m, lost)
    cell = 3 * tile + 1040 if long_cell else 50192
    name = "%s-rs%d.%d-S%d-c%d-grid%d-group%d-%s%s" % (family, k, m, S, cell, grid, group or GROUP, ctype,
                                                      "" if verify else "-noverify")
    return LoopB(family, name, k, m, tuple(lost), S, cell, grid, group, ctype, verify)


_LOOP_SHAPE = {"recon": (6, 3, (1, 7)), "sums": (6, 3, (0, 8)), "scrub": (6, 3, ()), "repair_rows": (6, 3, (2, 6)),
               "encode_rows": (6, 3, ()), "scrub_rows": (6, 3, ()), "read_rows": (6, 3, (1, 4))}
LOOP_B = []
for _family in FAMILIES:
    _k, _m, _lost = _LOOP_SHAPE[_family]
    LOOP_B += [_loop(_family, _k, _m, _lost, 9, False, 1), _loop(_family, _k, _m, _lost, 17, True, 5),
               _loop(_family, _k, _m, _lost, 17, False, 5, group=1), _loop(_family, _k, _m, _lost, 9, True, 1, group=3)]
# VERIFY_IN off and the second checksum kind, one shape each (the scrubs always verify; the
# encode has no input sums)
LOOP_B += [_loop("recon", 10, 4, (0, 5, 9, 12), 9, False, 5, verify=False),
           _loop("sums", 6, 3, (0, 8), 9, False, 5, verify=False),
           _loop("repair_rows", 6, 3, (2, 6), 9, False, 5, verify=False),
           _loop("read_rows", 6, 3, (1, 4), 9, False, 5, verify=False)]
LOOP_B += [_loop(_family, *_LOOP_SHAPE[_family], 17, False, 5, ctype="crc32") for _family in FAMILIES]


def loop_rows(case):
    return case.family.endswith("_rows")


def loop_lengths(case):
    """rs of a Part-B rows batch: the three short kinds against the cell's last
    tile and, every fourth stripe, 300 bytes (every tile column past the first
    is then dead for all four waves)."""
    tile = tile_bytes(case.family, case.k, case.m, case.lost)
    kinds = short_kinds(case.k, case.cell, tile) + [300]
    return [kinds[s % 4] for s in range(case.S)]


def loop_blocks(case):
    return block_tiles(case.S, case.cell, tile_bytes(case.family, case.k, case.m, case.lost), case.group or GROUP,
                       case.grid)


def loop_units(case):
    """The units a flip may hit: the survivors the plan reads; for the scrubs
    every present unit."""
    n = case.k + case.m
    if case.family in ("scrub", "scrub_rows"):
        return [u for u in range(n) if u not in case.lost]
    return survivors(n, case.k, case.lost)


def loop_length_of(case):
    if not loop_rows(case):
        return lambda ls, u: case.cell
    rs = loop_lengths(case)
    return lambda ls, u: P.unit_lens(case.k, case.k + case.m, case.cell, rs[ls])[u]


def loop_scrub_rows_corruptions(case):
    tile = tile_bytes(case.family, case.k, case.m, case.lost)
    return rows_scrub_corruptions(loop_blocks(case), loop_lengths(case), case.k, case.k + case.m, case.cell, tile,
                                  case.lost)


def loop_flips(case, count=4):
    tile = tile_bytes(case.family, case.k, case.m, case.lost)
    return late_flips(loop_blocks(case), list(range(case.S)), loop_units(case), loop_length_of(case), tile, count)


# ---- part 5: the byte-wise kernels ------------------------------------------------------

# launch_rows_bytes and launch_reconstruct_sums_bytes: one lane per item, 256 lanes a block,
# at most 8 blocks per CU, every lane strides by grid * 256.  An item is one checksum chunk
# of one row of one stripe: (stripe, row, chunk), rows = the targets (+ the k survivors when
# they are verified) for gf_reconstruct_sums_bytes and gf_reconstruct_rows_bytes, the m parity
# units (+ the k data units when their sums are asked for) for gf_encode_rows_bytes, the k
# data units + the parity units read for gf_read_rows_bytes, the present units for
# gf_scrub_rows_bytes.  `rows` below is each kernel's least count at the case's shape.
# 16-byte chunks of a 9232-byte cell are 577 per row, so 8 * 256 CUs * 256 lanes = 524288 items
# are passed by 455 stripes of 2 rows: 38 MB of cells.  The register kernels take 512-byte
# chunks only, so every call with 16-byte chunks runs its byte-wise kernel.
BYTES_BPC = 16
BYTES_CELL = 9232
ByteCase = collections.namedtuple("ByteCase", "family name k m lost rows")
BYTE_CASES = [ByteCase("sums", "sums-bytes", 6, 3, (1, 7), 2),  # the call verifies the survivors in a launch of its own
              ByteCase("repair_rows", "repair-bytes", 6, 3, (1, 7), 2 + 6),
              ByteCase("encode_rows", "encode-bytes", 6, 3, (), 3),
              ByteCase("read_rows", "read-bytes", 6, 3, (2, 4), 6),
              ByteCase("scrub_rows", "scrub-bytes", 6, 3, (), 9)]


def byte_lanes(cus):
    return 8 * cus * 256


def byte_stripes(case, cus):
    """Stripes so that the items exceed the lanes by 37 stripes' worth."""
    per_stripe = -(-BYTES_CELL // BYTES_BPC) * case.rows
    return -(-byte_lanes(cus) // per_stripe) + EXTRA_STRIPES


def byte_lengths(case, cus):
    """rs of a rows batch of the byte-wise kernels: all short, so that one
    launch holds every stripe."""
    kinds = short_kinds(case.k, BYTES_CELL, BYTES_CELL)
    return [kinds[s % 3] for s in range(byte_stripes(case, cus))]


def byte_flips(case, cus):
    """[(stripe, unit, byte)]: byte 3 of the first unit the call verifies in the
    last stripe, the last byte of the last such unit in the stripe before."""
    k, n, S = case.k, case.k + case.m, byte_stripes(case, cus)
    units = survivors(n, k, case.lost) if case.family != "scrub_rows" else list(range(n))
    rs = [k * BYTES_CELL] * S if case.family == "sums" else byte_lengths(case, cus)
    flips = []
    for x, s in enumerate((S - 1, S - 2)):
        lens = P.unit_lens(k, n, BYTES_CELL, rs[s])
        live = [u for u in units if lens[u] > 3]
        unit = live[-x]
        flips.append((s, unit, (lens[unit] - 1) if x else 3))
    return flips
