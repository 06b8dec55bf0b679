"""The case generators of test_gpu_coding_launch.py (coding_launch_cases.py)
meet their own conditions, and the reference they are compared with is pinned
to a product table built from ec_oracle.gf_mul.  CPU only."""
import numpy as np
import pytest

import coding_launch_cases as C
import ec_oracle as O

ALL_K = C.PRODUCT_K + C.RUNTIME_K


@pytest.fixture(scope="module")
def gf_table():
    """c * x for every pair, one gf_mul at a time."""
    return np.array([[O.gf_mul(c, x) for x in range(256)] for c in range(256)], dtype=np.uint8)


@pytest.mark.parametrize("k", ALL_K)
@pytest.mark.parametrize("r", C.PRODUCT_R)
def test_matrices_take_every_coefficient(k, r):
    mats = C.product_matrices(k, r)
    assert len(mats) == -(-256 // (r * k))
    assert all(len(m) == r and all(len(row) == k for row in m) for m in mats)
    assert {v for m in mats for row in m for v in row} == set(range(256))


@pytest.mark.parametrize("route", ["aligned", "unaligned", "bytes"])
@pytest.mark.parametrize("k", ALL_K)
def test_every_block_position_sees_every_byte(k, route):
    for rep in (0, 1):
        cells = C.product_cells(k, route, rep)
        S, kk, cell = cells.shape
        assert kk == k and not cells.flags.writeable
        if route == "bytes":
            assert cell == C.BYTE_CELL and S * cell >= C.PRODUCT_CELL
            # the 7-byte cells are the 4096-byte pattern in order
            for i in range(k):
                flat = cells[:, i].reshape(-1)
                assert np.array_equal(flat, C.product_cell(i, 0, rep, flat.size))
                for p in range(16):
                    assert set(flat[:C.PRODUCT_CELL][p::16].tolist()) == set(range(256)), (i, p)
            continue
        assert S == C.PRODUCT_STRIPES and cell == (C.UNALIGNED_CELL if route == "unaligned" else C.PRODUCT_CELL)
        for s in range(S):
            for i in range(k):
                for p in range(16):
                    assert set(cells[s, i, p:C.PRODUCT_CELL:16].tolist()) == set(range(256)), (s, i, p)
    assert not np.array_equal(C.product_cells(k, route, 0), C.product_cells(k, route, 1))


def test_unaligned_and_byte_cells_take_their_routes():
    """4109 = 8 * 513 + 5: the dword kernel and a 5-byte tail; 7 < 8: the byte kernel alone."""
    assert C.UNALIGNED_CELL % 8 == 5 and C.UNALIGNED_CELL > C.PRODUCT_CELL
    assert C.BYTE_CELL < 8
    assert C.PRODUCT_CELL == C.wave_tile_bytes(6) == 2 * C.wave_tile_bytes(10)


@pytest.mark.parametrize("k,r,route", [(k, r, "aligned") for k in ALL_K for r in C.PRODUCT_R] +
                         [(6, 3, "unaligned"), (6, 3, "bytes")])
def test_reference_equals_gf_mul_table(gf_table, k, r, route):
    """matmul_shards on these inputs against sum_i table[M[j][i]][in[i]]."""
    cells = C.product_cells(k, route)
    got = C.product_expected(k, r, route)
    mats = C.product_matrices(k, r)
    assert got.shape == (len(mats), cells.shape[0], r, cells.shape[2])
    for t, mat in enumerate(mats):
        for j, row in enumerate(mat):
            want = np.zeros(cells[:, 0].shape, dtype=np.uint8)
            for i, c in enumerate(row):
                want ^= gf_table[c][cells[:, i]]
            assert np.array_equal(got[t, :, j], want), (t, j)


def test_gf_mul_table_is_the_field(gf_table):
    """The table itself: 0 and 1, commutative, x * 2 by the modulus 0x11D, distributive over XOR."""
    assert not gf_table[0].any() and not gf_table[:, 0].any()
    assert np.array_equal(gf_table[1], np.arange(256, dtype=np.uint8))
    assert np.array_equal(gf_table, gf_table.T)
    x = np.arange(256)
    assert np.array_equal(gf_table[2], ((x << 1) ^ np.where(x & 0x80, 0x11D, 0)).astype(np.uint8))
    for c in (3, 0x1D, 0x8E, 0xFF):
        assert np.array_equal(gf_table[c][x ^ 0x5A], gf_table[c][x] ^ gf_table[c][0x5A])
    assert np.array_equal(gf_table, O.MUL_TABLE)


@pytest.mark.parametrize("cus", [256, 304, 64])
@pytest.mark.parametrize("k", C.PRODUCT_K)
def test_tile_counts_reach_every_branch(k, cus):
    W = C.wave_tile_bytes(k)
    cases = C.tile_count_cases(k, cus)
    want = set(C.SMALL_T) | {cus - 1, cus, cus + 1, 2 * cus + 3}
    assert {t for t, _, _, _ in cases} == want
    for T, S, cell, _ in cases:
        assert C.case_tiles(k, S, cell) == T and cell % 16 == 0 and cell > 0
    assert {1, 2, 3, 5, 7} <= {S for _, S, _, _ in cases}
    assert {S % 4 for _, S, _, _ in cases} == {0, 1, 2, 3}
    assert {-(-cell // W) for _, _, cell, _ in cases} == {1, 2, 3, 5}
    assert {cell % W for _, _, cell, _ in cases} == {16, W - 16, 0}
    # the queue's branches: fewer tiles than counters, either side of a multiple
    # of 8 and of the CU count, and (two rounds per atomic) a batch whose first
    # round is inside the launch and whose second is past its end
    assert any(T < 8 for T in want) and {7, 8, 9, 15, 16, 17} <= want

    def past_end_inside_a_batch(T):
        n = min(T, cus, 8)
        return any(2 * v * n + q < T <= (2 * v + 1) * n + q for q in range(n) for v in range(T // (2 * n) + 1))

    inside = {T for T in want if past_end_inside_a_batch(T)}
    assert {1, 7, 9, 17, cus + 1} <= inside and 16 not in inside
    # large and tiny alternate: every launch of the larger half is followed by one of the smaller half
    ts = [t for t, _, _, _ in cases]
    mid = sorted(ts)[len(ts) // 2]
    assert all(ts[i] >= mid >= ts[i + 1] for i in range(0, len(ts) - 1, 2))
    # the named tile counts of the captured sequence and of the fixed-order child exist
    names = {name for _, _, _, name in cases}
    assert set(C.GRAPH_T) <= names and {str(t) for t in C.FIXED_ORDER_T} <= names


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_masks_are_three_decodable_patterns(k, m):
    masks = C.mixed_masks(k, m, 7)
    assert len(set(masks)) == 3 and masks[0] == masks[3] == masks[6]
    for mask in masks:
        present = [(mask >> i) & 1 == 1 for i in range(k + m)]
        assert sum(present) >= k and not all(present[:k])
        O.decode_plan(k, m, present)
