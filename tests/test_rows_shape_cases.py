"""The case lists of the short-stripe shape and pattern tests
(rows_shape_cases.py) meet the conditions that keep test_gpu_rows_shapes.py and
test_gpu_rows_patterns.py from being vacuous.  CPU only."""
import collections
import math

import pytest

import rows_shape_cases as C


# ---- shapes ---------------------------------------------------------------------------

def test_shape_counts():
    assert len(C.REPAIR_SHAPES) == 64 and len(C.ENCODE_SHAPES) == 32
    assert len(C.SCRUB_SHAPES) == 32 and len(C.READ_SHAPES) == 51 == 3 * (3 + 4 + 5 + 5)
    for shapes in (C.REPAIR_SHAPES, C.ENCODE_SHAPES, C.SCRUB_SHAPES, C.READ_SHAPES):
        names = [C.kernel_name(s) for s in shapes]
        assert len(set(names)) == len(names) == len(set(C.shape_id(s) for s in shapes))
    assert {(s.k, s.r) for s in C.REPAIR_SHAPES} == {(k, r) for k in C.REGISTER_K for r in C.ROWS}
    assert {(s.k, s.m) for s in C.ENCODE_SHAPES} == {(k, r) for k in C.REGISTER_K for r in C.ROWS}
    assert {(s.k, s.e) for s in C.SCRUB_SHAPES} == {(k, r) for k in C.REGISTER_K for r in C.ROWS}
    assert {(s.k, s.r) for s in C.READ_SHAPES} == {(k, r) for k in C.REGISTER_K for r in range(5) if r <= k}


def test_four_rows_are_the_only_half_slab_shapes_up_to_k6():
    for k in (2, 3, 6):
        assert [C.rows_slabs(k, r) for r in C.ROWS] == [8, 8, 8, 4]
        assert [C.scrub_rows_slabs(k, e) for e in C.ROWS] == [8, 4, 4, 4]
    assert {C.rows_slabs(10, r) for r in range(5)} == {4} == {C.scrub_rows_slabs(10, e) for e in C.ROWS}
    # the cell: two wave-tiles at 8 KiB, three at 4 KiB, neither a whole number
    assert math.ceil(C.SHAPE_CELL / 8192) == 2 and math.ceil(C.SHAPE_CELL / 4096) == 3
    assert C.SHAPE_CELL % 4096 and C.SHAPE_CELL % 16 == 0


@pytest.mark.parametrize("k", C.REGISTER_K)
def test_shape_lengths(k):
    cell, cu = C.SHAPE_CELL, C.middle_unit(k)
    rs = C.shape_lengths(k)
    # the middle unit is unit 1 at k = 2 and 3: c + 1 (and at k = 2 also k * c - 1) is named twice
    assert len(rs) == {2: 7, 3: 8}.get(k, 9) == len(set(rs)) and 1 <= cu < max(k, 2)
    assert {r - cu * cell for r in rs if C.cut_unit(cell, r) == cu and r > cu * cell} >= {1, 17, 513, 4625, cell - 1}
    assert {1, cell, cell + 1, k * cell - 1} <= set(rs)
    mixed = C.mixed_shape_lengths(k)
    assert len(mixed) == C.SHAPE_MIXED_STRIPES == len(set(mixed))
    assert set(mixed) >= set(rs + [0, k * cell, (k - 1) * cell + 4625])


@pytest.mark.parametrize("shape", [s for s in C.REPAIR_SHAPES if s.verify and s.kind == "crc32c"], ids=C.shape_id)
def test_repair_targets_reach_the_shape(shape):
    k, m, n = shape.k, shape.m, shape.k + shape.m
    for r in C.shape_lengths(k):
        cu = C.cut_unit(C.SHAPE_CELL, r)
        sets = C.repair_targets(k, m, shape.r, cu)
        assert len(sets) == (3 if shape.r < m else 2)
        for lost, want in sets:
            assert len(want) == shape.r and set(want) <= set(lost) and len(set(lost)) == len(lost) <= m
            assert all(0 <= u < n for u in lost) and list(lost) == sorted(lost)
        near = sets[0][0]
        data = [u for u in near if u < k]
        assert len(data) == min(shape.r, k) and (cu in data)
        assert max(abs(u - cu) for u in data) <= min(shape.r, k)
        assert any(u >= k for u in sets[1][1])
        if shape.r < m:
            assert len(sets[2][0]) == shape.r + 1


@pytest.mark.parametrize("shape", [s for s in C.READ_SHAPES if s.verify == "crc32c"], ids=C.shape_id)
def test_read_losses_reach_the_shape(shape):
    k, m = shape.k, shape.m
    for r in C.shape_lengths(k):
        cu = C.cut_unit(C.SHAPE_CELL, r)
        sets = C.read_losses(k, m, shape.r, cu)
        assert len(sets) == (2 if shape.r < m else 1)
        for lost in sets:
            assert sum(u < k for u in lost) == shape.r and len(lost) <= m and len(set(lost)) == len(lost)
        assert shape.r == 0 or cu in sets[0]
        assert all(u < k for u in sets[0])
        assert len(sets) == 1 or sum(u >= k for u in sets[1]) == 1


@pytest.mark.parametrize("shape", [s for s in C.SCRUB_SHAPES if s.kind == "crc32c"], ids=C.shape_id)
def test_scrub_masks_leave_e_extras(shape):
    k, m, n = shape.k, C.SHAPE_M, shape.k + C.SHAPE_M
    sets = C.scrub_absent_sets(k, shape.e)
    assert len(sets) == math.comb(m, m - shape.e) + (math.comb(m, m - shape.e - 1) if shape.e < m else 0)
    assert len(set(sets)) == len(sets)
    for absent in sets:
        present = [u for u in range(n) if u not in absent]
        assert len(present) - k == shape.e
        assert all(u >= k for u in present[k:])  # every extra is a parity unit
    if shape.e < m:
        assert any(any(u >= k for u in [x for x in range(n) if x not in a][:k]) for a in sets)


# ---- patterns, cuts, batches ----------------------------------------------------------

@pytest.mark.parametrize("k,m", C.PATTERN_CODES)
def test_pattern_counts(k, m):
    pats = C.patterns(k, m)
    assert len(pats) == C.PATTERN_COUNT[(k, m)] == sum(math.comb(k + m, i) for i in range(m + 1))
    assert {16: (3, 2), 130: (6, 3), 1471: (10, 4)}[len(pats)] == (k, m)
    assert len(set(pats)) == len(pats) and pats[0] == ()
    assert all(len(p) <= m and list(p) == sorted(set(p)) and all(0 <= u < k + m for u in p) for p in pats)


def test_cut_values():
    assert C.cut_x(9232) == [1, 15, 16, 17, 511, 512, 513, 1040, 4097, 4625, 8193, 8721, 9216, 9231, 9232]
    assert C.cut_x(5136) == [1, 15, 16, 17, 511, 512, 513, 1040, 4097, 4625, 5120, 5135, 5136]
    assert C.PATTERN_CELL == {(3, 2): 9232, (6, 3): 9232, (10, 4): 5136}


def test_batch_list():
    ids = C.all_batches()
    assert len(ids) == 1 + 6 + 10
    assert [i for i in ids if i[:2] == (3, 2)] == [(3, 2, None)]
    assert [i[2] for i in ids if i[:2] == (6, 3)] == list(range(6))
    assert [i[2] for i in ids if i[:2] == (10, 4)] == list(range(10))


def _props(b):
    """Which of the issue's five stripes a batch holds."""
    k, m, cell = b.k, b.m, b.cell
    got = collections.Counter()
    for r, lost in zip(b.rs, b.losts):
        cu = C.cut_unit(cell, r)
        lens = C.unit_lens(k, k + m, cell, r)
        n0 = min(cell, r)
        assert lens[cu] > 0 and all(lens[u] == 0 for u in range(cu + 1, k)) and all(lens[u] == cell for u in range(cu))
        if cu in lost:
            got["cut unit lost"] += 1
        if cu + 1 < k and cu + 1 in lost:
            got["first empty unit lost"] += 1
        if 0 in lost and r < cell:
            got["unit 0 lost, r < c"] += 1
        survivors = [u for u in range(k + m) if u not in lost][:k]
        if 0 in lost and any(u < k and lens[u] < n0 for u in survivors):
            got["unit 0 lost, a surviving data unit ends early"] += 1
        if lost and all(u >= k for u in lost):
            got["only parity lost"] += 1
        if lost == C.nearest_data_units(k, cu, m):
            got["m data units nearest the cut lost"] += 1
    return got


@pytest.mark.parametrize("k,m,cut", C.all_batches(), ids=lambda v: str(v))
def test_batch_contents(k, m, cut):
    b = C.batch(k, m, cut)
    pats, xs = C.patterns(k, m), C.cut_x(b.cell)
    S = len(b.rs)
    assert S == len(b.losts) == {(3, 2): 16 * 3 * 15, (6, 3): 1950, (10, 4): 1471}[(k, m)]
    assert b.cell % 16 == 0 and all(1 <= r <= k * b.cell for r in b.rs)
    pairs = collections.Counter((C.cut_unit(b.cell, r), r - C.cut_unit(b.cell, r) * b.cell) for r in b.rs)
    cuts = list(range(k)) if cut is None else [cut]
    assert set(pairs) == {(u, x) for u in cuts for x in xs}
    by_pattern = collections.defaultdict(set)
    for r, lost in zip(b.rs, b.losts):
        by_pattern[lost].add(r)
    assert set(by_pattern) == set(pats)  # every pattern in every batch
    if (k, m) == (10, 4):
        assert min(pairs.values()) >= 100
        assert all(len(v) == 1 for v in by_pattern.values())
    else:
        assert all(v == {u * b.cell + x for u in cuts for x in xs} for v in by_pattern.values())
    # a full stripe only where the last unit is cut at its end
    assert (k * b.cell in b.rs) == (k - 1 in cuts)
    got = _props(b)
    # what the geometry allows: no unit is empty when the last one is cut, and
    # r < c needs the cut in unit 0
    assert got["cut unit lost"] and got["only parity lost"] and got["m data units nearest the cut lost"]
    assert bool(got["first empty unit lost"]) == (cuts != [k - 1])
    assert bool(got["unit 0 lost, r < c"]) == (0 in cuts)
    assert got["unit 0 lost, a surviving data unit ends early"]
    if (k, m) == (10, 4):
        # one x per pattern: the stripes above must not all sit on x = c
        assert got["cut unit lost"] >= 100


@pytest.mark.parametrize("k,m", C.PATTERN_CODES)
def test_every_code_holds_every_kind_of_stripe(k, m):
    total = collections.Counter()
    for cut in C.batch_ids(k, m):
        total.update(_props(C.batch(k, m, cut)))
    assert all(total[name] for name in ("cut unit lost", "first empty unit lost", "unit 0 lost, r < c",
                                        "only parity lost", "m data units nearest the cut lost"))


@pytest.mark.parametrize("k,m,cut", [(3, 2, None), (6, 3, 0), (6, 3, 5), (10, 4, 4)], ids=lambda v: str(v))
def test_scrub_flips(k, m, cut):
    b = C.batch(k, m, cut)
    flips = C.scrub_flips(b)
    n = k + m
    assert [s for s, _, _ in flips] == list(range(1, len(b.rs), 2))
    for s, u, byte in flips:
        assert u not in b.losts[s] and 0 <= byte < C.unit_lens(k, n, b.cell, b.rs[s])[u]
    # every unit that holds a byte in some stripe is hit somewhere
    last_cut = max(C.cut_unit(b.cell, r) for r in b.rs)
    assert {u for _, u, _ in flips} == set(range(last_cut + 1)) | set(range(k, n))
    # in survivors and in extras, in the cut unit, in the first and the last byte of a unit
    hit_cut = [f for f in flips if f[1] == C.cut_unit(b.cell, b.rs[f[0]])]
    assert len(hit_cut) >= 3
