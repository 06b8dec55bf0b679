"""verified_loop_cases.py without a GPU: the model of the tile order against
its own definition, and the conditions the GPU cases of
test_gpu_verified_loops.py must meet, asserted from the model for 64 and 256
CUs.  They are conditions on inputs: a case that misses one is a wrong case, it
is not skipped."""
import pytest

import rows_shape_cases as P
import verified_loop_cases as L


# ---- the model --------------------------------------------------------------------------

GEOMETRIES = [(S, cell, tile, group, grid)
              for S in (1, 7, 8, 9, 16, 17, 23) for cell in (528, 32768, 50192, 99344) for tile in (16384, 32768)
              for group in (1, 3, 8) for grid in (1, 5, 64)]


def test_every_tile_is_taken_once_by_block_tile_mod_grid():
    for S, cell, tile, group, grid in GEOMETRIES:
        tps, total = L.tile_geometry(S, cell, tile)
        blocks = L.block_tiles(S, cell, tile, group, grid)
        n = min(grid, total)
        assert len(blocks) == n
        g, grouped = L.tile_order(S, tps, group)
        seen = {}
        for b, tiles in enumerate(blocks):
            for i, t in enumerate(tiles):
                assert t not in seen, (S, cell, tile, group, grid, t)
                seen[t] = (b, b + i * n)  # the block, and the tile index its loop holds
        assert set(seen) == {(s, c) for s in range(S) for c in range(tps)}
        assert sorted(index for _, index in seen.values()) == list(range(total))
        for (s, c), (b, index) in seen.items():
            assert L.tile_coords(index, tps, g, grouped) == (s, c) and index % n == b


def test_order_inside_a_group_is_column_major_and_the_remainder_stripe_major():
    # 17 stripes in groups of 8, 2 tiles each: two whole groups, then stripe 16 on its own
    tps, total = L.tile_geometry(17, 50192, 32768)
    assert (tps, total) == (2, 34)
    g, grouped = L.tile_order(17, tps, 8)
    assert (g, grouped) == (8, 32)
    order = [L.tile_coords(t, tps, g, grouped) for t in range(total)]
    assert order[:16] == [(s, 0) for s in range(8)] + [(s, 1) for s in range(8)]
    assert order[16:32] == [(s, 0) for s in range(8, 16)] + [(s, 1) for s in range(8, 16)]
    assert order[32:] == [(16, 0), (16, 1)]


@pytest.mark.parametrize("S,group,whole,rest", [(9, 8, 8, 1), (17, 8, 16, 1), (17, 3, 15, 2), (9, 3, 9, 0),
                                                (17, 1, 17, 0), (5, 8, 5, 0), (8229, 8, 8224, 5)])
def test_stripe_counts_with_a_remainder_group(S, group, whole, rest):
    g, grouped = L.tile_order(S, 2, group)
    assert grouped == whole * 2 and S - grouped // 2 == rest
    assert g == min(group, S)
    if rest:  # the remainder runs stripe-major behind the whole groups
        assert [L.tile_coords(t, 2, g, grouped) for t in range(grouped, 2 * S)] == \
            [(s, c) for s in range(whole, S) for c in range(2)]


def test_restated_slab_rules():
    assert [L.recon_crc_slabs(k, r) for k, r in ((2, 1), (6, 3), (6, 4), (10, 1), (10, 4))] == [8, 8, 4, 4, 4]
    assert [L.scrub_crc_slabs(k, e) for k, e in ((2, 1), (6, 1), (6, 3), (10, 1))] == [8, 8, 4, 4]
    assert L.tile_bytes("recon", 10, 4, (0, 5, 9, 12)) == 16384 and L.tile_bytes("recon", 6, 3, (1, 7)) == 32768
    assert L.tile_bytes("scrub", 6, 3, ()) == 16384 and L.tile_bytes("scrub", 2, 1, ()) == 32768
    assert L.tile_bytes("read_rows", 6, 3, (1, 4)) == 32768 and L.tile_bytes("scrub_rows", 6, 3, (1,)) == 16384
    assert L.tile_bytes("encode_rows", 10, 4) == 16384 and L.tile_bytes("repair_rows", 6, 3, (2, 6)) == 32768


# ---- part A: (d) and (e) ----------------------------------------------------------------

@pytest.mark.parametrize("cus", L.CU_COUNTS)
@pytest.mark.parametrize("case", L.RECON_A, ids=lambda c: c.name)
def test_part_a_reconstruction_batches(case, cus):
    S, main = L.recon_batch(case, cus)
    tile = L.tile_bytes(case.family, case.k, case.m, case.lost)
    grid = L.blocks_per_cu(case.family) * cus
    tps, total = L.tile_geometry(len(main), case.cell, tile)
    assert tps == 1 and total > grid == 32 * cus
    assert S * (case.k + case.m) * case.cell < L.CELL_BYTES_LIMIT
    losts = L.recon_losts(case, S, main)
    assert [s for s in range(S) if losts[s] == case.lost] == main and case.other != case.lost
    if case.form == "mixed":
        assert main != list(range(len(main)))  # the launch reads a list that is no identity
    blocks = L.block_tiles(len(main), case.cell, tile, L.GROUP, grid)
    late = set(L.late_tiles(blocks))
    assert len(late) == L.EXTRA_STRIPES
    flips = L.recon_flips(case, cus)
    surv = L.survivors(case.k + case.m, case.k, case.lost)
    assert len(flips) == 3 and len({s for s, _, _ in flips}) == 3
    for f in flips:
        assert L.flip_tile(f, main, tile) in late and f[1] in surv and 0 <= f[2] < case.cell
    assert {f[2] // 512 for f in flips} >= {0, (case.cell - 1) // 512}  # a full chunk and the 16-byte one


def test_part_a_cells_reach_the_waves_they_are_there_for():
    """528 B: wave 0 alone.  4624 B at 4 slabs: wave 0 full, wave 1 with one
    full chunk and a 16-byte one."""
    for tile in (16384, 32768):
        assert [L.wave_live(528, tile, 0, w) for w in range(4)] == [True, False, False, False]
    assert [L.wave_live(4624, 16384, 0, w) for w in range(4)] == [True, True, False, False]
    assert 4624 - 4096 == 528
    shapes = {(c.family, L.tile_bytes(c.family, c.k, c.m, c.lost)) for c in L.RECON_A}
    assert shapes == {(f, t) for f in ("recon", "sums") for t in (16384, 32768)}
    for family in ("recon", "sums"):
        mine = [c for c in L.RECON_A if c.family == family]
        assert {(c.form, c.expected) for c in mine} >= {("uniform", True), ("mixed", True), ("mixed", False)}
        assert {c.ctype for c in mine} == {"crc32c", "crc32"}
        assert any(c.cell == 4624 and L.tile_bytes(family, c.k, c.m, c.lost) == 16384 for c in mine)
    # R * SLABS <= 24 fails for no compiled shape but 8 slabs with R > 3, which recon_crc_slabs never picks
    assert all(r * L.recon_crc_slabs(k, r) <= 24 for k in P.REGISTER_K for r in P.ROWS)


def check_rows_scrub_corruptions(got, late, rs, k, n, cell, tile, absent, two_columns):
    """Silent, visible, both in one stripe (in two tile columns where the
    stripes have two), a wrong sum in a fourth stripe: all in late tiles, below
    their unit's length, in present units."""
    found, by_sum = got
    assert [c.silent for c in found] == [True, False, True, False]
    assert found[2].stripe == found[3].stripe and found[2].unit != found[3].unit
    assert len({c.stripe for c in found} | {by_sum[0]}) == 4
    if two_columns:
        assert found[2].byte // tile != found[3].byte // tile
    for s, u, byte in [c[:3] for c in found] + [by_sum]:
        assert (s, byte // tile) in late and u not in absent and byte < P.unit_lens(k, n, cell, rs[s])[u]


@pytest.mark.parametrize("cus", L.CU_COUNTS)
@pytest.mark.parametrize("case", L.ROWS_A, ids=lambda c: c.name)
def test_part_a_rows_batches(case, cus):
    k, n, cell = case.k, case.k + case.m, case.cell
    rs, grid = L.rows_lengths(case, cus), L.rows_grid(case, cus)
    tile = L.tile_bytes(case.family, k, case.m, case.lost)
    tps, total = L.tile_geometry(len(rs), cell, tile)
    assert total > grid and tps == (2 if cell > L.ROWS_CELL else 1) and total - grid in (37, 38)
    assert len(rs) * n * cell < L.CELL_BYTES_LIMIT
    if tps == 2:  # both tiles of every stripe are live
        assert case.family == "scrub_rows" and cell == tile + 528 and all(L.n0_of(cell, r) > tile for r in rs)
    kinds = L.short_kinds(k, cell, tile)
    assert P.cut_unit(cell, kinds[0]) == 0 and kinds[0] % 512 not in (0, 511) and kinds[0] % 16
    assert 0 < P.cut_unit(cell, kinds[1]) < k - 1 and kinds[1] % cell % 512 and kinds[1] % 16
    assert kinds[2] == k * cell - 1
    blocks = L.block_tiles(len(rs), cell, tile, L.GROUP, grid)
    if case.form == "data_len":
        assert all(r == k * cell for r in rs[:-1]) and rs[-1] == kinds[case.which]
        assert (len(rs) - 1, 0) in L.late_tiles(blocks)
        return
    assert all(0 < r < k * cell for r in rs) and set(rs) == set(kinds)
    for tiles in blocks:  # consecutive tiles of a block never share a length
        assert all(rs[a[0]] != rs[b[0]] for a, b in zip(tiles, tiles[1:]))
    if case.family == "encode_rows":
        return
    late = set(L.late_tiles(blocks))
    if case.family == "scrub_rows":
        check_rows_scrub_corruptions(L.rows_scrub_case_corruptions(case, cus), late, rs, k, n, cell, tile, case.lost,
                                     two_columns=tps == 2)
        return
    flips = L.rows_flips(case, cus)
    assert len(flips) == 3
    for s, u, byte in flips:
        assert (s, byte // tile) in late and u not in case.lost
        assert byte < P.unit_lens(k, n, cell, rs[s])[u]


@pytest.mark.parametrize("cus", L.CU_COUNTS)
@pytest.mark.parametrize("case", L.SCRUB_A, ids=lambda c: c.name)
def test_part_a_scrub_batches(case, cus):
    S, main = L.scrub_batch(case, cus)
    cell, tile = L.scrub_cell(case), L.tile_bytes(case.family, case.k, case.m, case.absent)
    grid = L.scrub_grid(case, cus)
    assert grid == (4 if case.form == "uniform" else 2) * cus
    tps, total = L.tile_geometry(len(main), cell, tile)
    assert tps == 2 and cell == tile + 528 and total == grid + 38
    assert S * (case.k + case.m) * cell < L.CELL_BYTES_LIMIT
    if case.form == "degraded":
        assert main != list(range(len(main)))
    blocks = L.block_tiles(len(main), cell, tile, L.GROUP, grid)
    late = set(L.late_tiles(blocks))
    found = L.scrub_case_corruptions(case, cus)
    assert [c.silent for c in found] == [True, False, True, False]
    assert found[2].stripe == found[3].stripe and found[2].unit != found[3].unit
    assert found[2].byte // tile != found[3].byte // tile
    assert len({c.stripe for c in found}) == 3
    for c in found:
        assert (main.index(c.stripe), c.byte // tile) in late and c.unit not in case.absent and c.byte < cell
    # on a grid this large no block holds two tiles of one stripe: they lie 1 or 8 tiles apart
    assert L.merging_blocks(blocks) == []


def test_part_a_covers_both_slab_counts_of_the_scrub():
    assert {L.tile_bytes(c.family, c.k, c.m, c.absent) for c in L.SCRUB_A} == {16384, 32768}
    assert {(c.form, c.ctype) for c in L.SCRUB_A} == {(f, t) for f in ("uniform", "degraded")
                                                      for t in ("crc32c", "crc32")}


# ---- part B: (a), (b), (c), (e) ---------------------------------------------------------

def tile_extent(case):
    """length(launch stripe): what the kernel measures a tile against: the cell,
    or the short stripe's n0."""
    if not L.loop_rows(case):
        return lambda ls: case.cell
    rs = L.loop_lengths(case)
    return lambda ls: L.n0_of(case.cell, rs[ls])


@pytest.mark.parametrize("case", L.LOOP_B, ids=lambda c: c.name)
def test_part_b_every_block_takes_two_tiles(case):
    blocks = L.loop_blocks(case)
    assert len(blocks) == case.grid in L.BLOCK_GRIDS
    assert all(len(tiles) >= 2 for tiles in blocks)
    late = set(L.late_tiles(blocks))
    tile = L.tile_bytes(case.family, case.k, case.m, case.lost)
    length_of = L.loop_length_of(case)
    if case.family == "scrub_rows":
        rs = L.loop_lengths(case)
        check_rows_scrub_corruptions(L.loop_scrub_rows_corruptions(case), late, rs, case.k, case.k + case.m, case.cell,
                                     tile, case.lost, two_columns=True)
        return
    flips = L.loop_flips(case)
    assert len(flips) == 4 and len(set(flips)) == 4
    for s, u, byte in flips:
        assert (s, byte // tile) in late and u in L.loop_units(case) and byte < length_of(s, u)


@pytest.mark.parametrize("family", L.FAMILIES)
def test_part_b_family_conditions(family):
    cases = [c for c in L.LOOP_B if c.family == family]
    assert {c.group for c in cases} == set(L.ORDER_GROUPS) and {c.grid for c in cases} == set(L.BLOCK_GRIDS)
    assert {c.ctype for c in cases} == {"crc32c", "crc32"} and {c.S for c in cases} == {9, 17}
    if family in ("recon", "sums", "repair_rows", "read_rows"):
        assert {c.verify for c in cases} == {True, False}
    seen = set()
    for case in cases:
        tile = L.tile_bytes(family, case.k, case.m, case.lost)
        assert {case.cell} <= {50192, 3 * tile + 1040}
        extent = tile_extent(case)
        blocks = L.loop_blocks(case)
        group = case.group or L.GROUP
        whole = (case.S // group) * group
        for tiles in blocks:
            lens = [L.tile_len(extent(ls), tile, c) for ls, c in tiles]
            for (a, b), ((ls0, c0), (ls1, c1)) in zip(zip(lens, lens[1:]), zip(tiles, tiles[1:])):
                if a == tile and 0 < b < tile:
                    seen.add("full then short")
                if 0 < a < tile and b == tile:
                    seen.add("short then full")
                for w in range(4):
                    if a and not L.wave_live(extent(ls0), tile, c0, w) and L.wave_live(extent(ls1), tile, c1, w):
                        seen.add("a wave skips, then works")
            stripes = [ls for ls, _ in tiles]
            if len(set(stripes)) < len(stripes):
                seen.add("two tiles of one stripe")
            if whole < case.S and min(stripes) < whole <= max(stripes):
                seen.add("a whole group and the remainder")
    assert seen == {"full then short", "short then full", "a wave skips, then works", "two tiles of one stripe",
                    "a whole group and the remainder"}


# ---- part 5 -----------------------------------------------------------------------------

@pytest.mark.parametrize("cus", L.CU_COUNTS)
@pytest.mark.parametrize("case", L.BYTE_CASES, ids=lambda c: c.name)
def test_byte_kernel_items_exceed_the_lanes(case, cus):
    S = L.byte_stripes(case, cus)
    chunks = -(-L.BYTES_CELL // L.BYTES_BPC)
    assert chunks == 577 and S * chunks * case.rows > L.byte_lanes(cus) == 8 * cus * 256
    assert S * (case.k + case.m) * L.BYTES_CELL < L.CELL_BYTES_LIMIT
    flips = L.byte_flips(case, cus)
    assert len(flips) == 2 and {s for s, _, _ in flips} == {S - 1, S - 2}
    for s, u, byte in flips:  # every item of these stripes lies past the first stride of every lane
        assert s * chunks * case.rows >= L.byte_lanes(cus) and u not in case.lost
    if case.family != "sums":
        rs = L.byte_lengths(case, cus)
        assert len(rs) == S and all(0 < r < case.k * L.BYTES_CELL for r in rs)
        for s, u, byte in flips:
            assert byte < P.unit_lens(case.k, case.k + case.m, L.BYTES_CELL, rs[s])[u]
