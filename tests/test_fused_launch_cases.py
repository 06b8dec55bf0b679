"""The case generators of test_gpu_fused_launch.py and fused_generic_child.py
(fused_launch_cases.py) meet their own counts and conditions, and the reference
they are compared with stands on its own: the published check values, the POSIX
cksum vectors of tests/golden/cksum_vectors.json, ec_oracle's Python CRCs and
ec_oracle.verified_read_row.  CPU only."""
import json
import os

import numpy as np
import pytest

import ec_oracle as O
import fused_launch_cases as C


def test_counts():
    """23 fused encode cases, 5 fallback cases, 20 specialised cases; of the 32
    generic (K, E, type) the 26 a caller can reach (E <= K) and the 6 nobody can."""
    enc, fb, gen, spec = C.encode_cases(), C.fallback_cases(), C.generic_cases(), C.specialised_cases()
    assert (len(enc), len(fb), len(spec)) == (23, 5, 20)
    assert len(gen) == 26 and len(gen) + 2 * len(C.UNREACHABLE) == 32
    assert C.UNREACHABLE == ((2, 3), (2, 4), (3, 4)) and all(e > k for k, e in C.UNREACHABLE)
    for cases in (enc, fb, gen, spec):
        assert len({c.name for c in cases}) == len(cases)
    assert {(c.k, c.m) for c in enc if c.codec == "rs"} == {(k, m) for k in C.FUSED_K for m in C.FUSED_R}
    assert [(c.k, c.m) for c in enc if c.codec == "rs-legacy"] == [(3, 2), (6, 3), (10, 4)]
    assert [(c.k, c.m) for c in enc if c.codec == "xor"] == [(2, 1), (3, 1), (6, 1), (10, 1)]
    assert {(c.k, c.e, c.ctype) for c in gen} == {(k, e, t) for k in C.FUSED_K for e in C.FUSED_R if e <= k
                                                  for t in (C.CRC32, C.CRC32C)}
    assert {(c.k, c.m, c.e, c.ctype) for c in spec} == {(k, C.RS[k], e, t) for k in C.FUSED_K
                                                        for e in range(1, C.RS[k] + 1) for t in (C.CRC32, C.CRC32C)}


def test_cells_reach_every_branch_of_a_block_tile():
    one, two = C.CELLS
    assert one == 8 * 4 * 1024            # one tile of 4 waves x 8 slabs
    assert two == one + 3 * 1024 + 528 and two % 16 == 0 and two % 512 == 16
    for wave_bytes in (8192, 4096):       # 8 and 4 slabs a wave
        tile = 4 * wave_bytes
        last = two % tile
        assert 0 < last < wave_bytes      # the last tile: one live wave, the others past the end
        assert last % 1024 == 528         # a partial slab ...
        assert wave_bytes // 1024 - (last // 1024 + 1) == (4 if wave_bytes == 8192 else 0)  # ... dead ones at 8 slabs


def test_fused_and_fallback_conditions():
    """launch_fused takes k in 2, 3, 6, 10 with m <= 4, 512-byte chunks, cells
    of a multiple of 16 bytes and 16-byte aligned bases and strides."""
    def fused(c, cell):
        return c.k in C.FUSED_K and c.m <= 4 and c.bpc == 512 and cell % 16 == 0 and c.data_off % 16 == 0 \
            and (cell + C.PITCH_GAP) % 16 == 0
    for c in C.encode_cases():
        assert c.cells == C.CELLS and all(fused(c, cell) for cell in c.cells), c
    fb = C.fallback_cases()
    assert all(not fused(c, cell) for c in fb for cell in c.cells)
    # each fallback case misses exactly one condition
    assert [(c.m > 4, c.k not in C.FUSED_K, c.cells[0] % 16 != 0, c.bpc != 512, c.data_off != 0) for c in fb] == \
        [tuple(i == j for j in range(5)) for i in range(5)]


@pytest.mark.parametrize("cell", C.CELLS + (1000,))
def test_every_batch_has_a_stripe_of_each_kind(cell):
    assert C.STRIPES == len(C.DATA_KINDS) == 4
    assert [C.stripe_kind(s) for s in range(6)] == ["random", "zero", "ones", "last-byte", "random", "random"]
    for k in (2, 10):
        d = C.batch_data(k, C.STRIPES, cell, seed=k)
        assert len(np.unique(d[0])) > 200 and not d[1].any() and (d[2] == 0xFF).all()
        assert not d[3, :, :-1].any() and (d[3, :, -1] == C.LAST_BYTE).all()
        big = C.batch_data(k, 6, cell, seed=k)
        assert all(len(np.unique(big[s])) > 200 for s in (0, 4, 5))
        assert np.array_equal(d, C.batch_data(k, C.STRIPES, cell, seed=k))       # reproducible
        assert not np.array_equal(d[0], C.batch_data(k, C.STRIPES, cell, seed=k + 1)[0])


@pytest.mark.parametrize("case", C.generic_cases() + C.specialised_cases(), ids=lambda c: c.name)
def test_verify_case_conditions(case):
    k, m, e = case.k, case.m, case.e
    assert len(case.lost_data) == e and all(0 <= i < k for i in case.lost_data)
    assert case.lost_parity in ((), (0,)) and e + len(case.lost_parity) <= m
    av = C.available(case)
    assert len(av) == k + m - e - len(case.lost_parity) >= k
    present = [i in av for i in range(k + m)]
    survivors, missing, dm = O.decode_plan(k, m, present)  # the oracle's plan: the kernel's inputs and rows
    assert survivors == av[:k] and missing == list(case.lost_data) and len(dm) == e
    if case.lost_parity:
        # the survivors skip parity unit 0: shard ids are not the identity and not contiguous
        assert k not in av and any(u >= k for u in av[:k]) and C.spares(case) == m - e - 1
    for cell in case.cells:
        flips = C.verify_flips(case, cell)
        assert flips[0] == (4, av[0], 3) and flips[1] == (5, av[k - 1], cell - 1)
        if cell % C.BPC:
            assert cell - 1 >= cell // C.BPC * C.BPC  # in the short last chunk
        extra = flips[2:]
        if C.spares(case):
            assert [s for s, _, _ in extra] == [6] * (C.spares(case) + 1)
            assert [u for _, u, _ in extra] == av[:C.spares(case) + 1]
        else:
            assert not extra
        assert all(u in av and 0 <= b < cell for _, u, b in flips)
        # the four special-data stripes stay clean, the bent ones are random data
        assert {s for s, _, _ in flips} <= {4, 5, 6} and all(C.stripe_kind(s) == "random" for s, _, _ in flips)
        assert C.verify_flips(case, cell, 6) == flips[:2]


def test_generic_halves_and_lost_units():
    gen = C.generic_cases()
    with_p = [c for c in gen if c.lost_parity]
    assert len(with_p) == len(gen) // 2 == 13
    for ctype in (C.CRC32, C.CRC32C):       # either type sees both halves
        assert 0 < sum(1 for c in with_p if c.ctype == ctype) < 13
    for k in C.FUSED_K:                     # every shape sees both halves
        for e in range(1, min(k, 4) + 1):
            assert {bool(c.lost_parity) for c in gen if (c.k, c.e) == (k, e)} == {True, False}
    assert all(c.m == c.e + (2 if c.lost_parity else 0) for c in gen)
    assert all(C.spares(c) == (1 if c.lost_parity else 0) for c in gen)
    spec = C.specialised_cases()
    assert all(C.spares(c) == c.m - c.e - len(c.lost_parity) for c in spec)
    assert any(c.lost_parity for c in spec) and any(C.spares(c) == 0 for c in spec)
    assert C.lost_units(6, 3) == (1, 3, 5) and C.lost_units(10, 4) == (2, 4, 7, 9) and C.lost_units(2, 2) == (0, 1)
    # in most cases the first survivor is a data unit (its flag makes the call rebuild it) ...
    assert sum(1 for c in gen + spec if 0 not in c.lost_data) > len(gen + spec) // 2
    # ... and the last survivor is always a parity unit
    assert all(C.available(c)[c.k - 1] >= c.k for c in gen + spec)


def test_reference_checksums_reproduce_published_vectors():
    """The reference call of every sum in these tests, alone: the catalogue's
    check values and the POSIX cksum vectors (coreutils, an independent
    implementation; cksum = CRC-32/CKSUM of the message and its length)."""
    assert C.checksum(C.CRC32C, b"123456789") == 0xE3069283
    assert C.checksum(C.CRC32, b"123456789") == 0x765E7680
    with open(os.path.join(os.path.dirname(__file__), "golden", "cksum_vectors.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 10
    for case in cases:
        data = bytes.fromhex(case["hex"])
        n, tail = len(data), b""
        while n:
            tail += bytes([n & 0xFF])
            n >>= 8
        assert C.checksum(C.CRC32, data + tail) == case["posix_cksum"]


@pytest.mark.parametrize("ctype", [C.CRC32, C.CRC32C])
def test_chunk_sums_equal_the_python_oracle(ctype):
    cells = C.batch_data(3, 4, 512 * 3 + 16, seed=5)
    got = C.chunk_sums(cells, ctype)
    assert got.shape == (4, 3, 4, 4)
    for s in range(4):
        for u in range(3):
            assert got[s, u].tobytes() == O.chunk_checksums(cells[s, u].tobytes(), C.BPC, ctype), (s, u)
    big = C.chunk_sums(cells, ctype, 4096)
    assert big.shape == (4, 3, 1, 4) and big[0, 0].tobytes() == O.chunk_checksums(cells[0, 0].tobytes(), 4096, ctype)
    many = C.batch_data(2, 40, 528, seed=6)          # enough stripes for the threaded path
    assert np.array_equal(C.chunk_sums(many, ctype)[33], C.chunk_sums(many[33:34], ctype)[0])


def test_parity_and_decode_references():
    data = C.batch_data(6, 40, 528, seed=9)
    par = C.encode_ref(6, 3, data)
    for s in (0, 1, 2, 3, 17, 39):
        want = O.encode(6, 3, list(data[s]))
        assert all(np.array_equal(par[s, j], want[j]) for j in range(3)), s
    present = sum(1 << i for i in range(9) if i not in (1, 3, 5))
    back = C.decode_ref(6, 3, data, par, present)
    assert np.array_equal(back, data[:, [1, 3, 5]])
    # the rows of a codec's matrix over the data: rs through both references
    rows = O.codec_matrix("rs", 6, 3)[6:]
    assert np.array_equal(C.matrix_parity(rows, data[:4]), par[:4])
    assert np.array_equal(C.matrix_parity(O.codec_matrix("xor", 6, 1)[6:], data[:4])[:, 0],
                          np.bitwise_xor.reduce(data[:4], axis=1))


@pytest.mark.parametrize("case", [c for c in C.generic_cases() + C.specialised_cases()
                                  if (c.k, c.e) in ((2, 1), (3, 2), (6, 3)) and c.ctype == C.CRC32C],
                         ids=lambda c: c.name)
def test_verify_truth_equals_the_python_oracle(case):
    """VerifyTruth at a 528-byte cell against ec_oracle.verified_read_row,
    stripe by stripe: data, flags, which stripes cannot be rebuilt."""
    k, m, cell = case.k, case.m, 528
    t = C.VerifyTruth(case, cell, seed=77)
    lost = set(case.lost_data) | {k + j for j in case.lost_parity}
    assert t.units.shape == (C.VERIFY_STRIPES, k + m, cell) and (t.units[:, sorted(lost)] == 0xEE).all()
    assert sorted(t.flips) == sorted(C.verify_flips(case, cell))
    failed = set()
    for s in range(C.VERIFY_STRIPES):
        cells = [None if i in lost else t.units[s, i].tobytes() for i in range(k + m)]
        sums = [t.sums[s, i].tobytes() for i in range(k + m)]
        try:
            got, bad = O.verified_read_row(k, m, cells, sums, C.BPC, case.ctype)
        except O.NotEnoughShards:
            failed.add(s)
            assert {(s, i) for i in case.lost_data} <= set(t.free)
            if t.flags_checked[s]:  # no spare: exactly the bent unit
                assert t.bad[s].tolist() == [int((s, i) in {(f[0], f[1]) for f in t.flips}) for i in range(k + m)]
            continue
        assert t.flags_checked[s] and t.bad[s].tolist() == list(bad), s
        for i in range(k):
            if i in case.lost_data or bad[i]:
                assert t.out[(s, i)].tobytes() == got[i], (s, i)
            else:
                assert (s, i) not in t.out
    assert t.raises == bool(failed)
    assert {s for s, _ in t.free} == failed and not failed & {0, 1, 2, 3}
    # every lost cell of the clean special-data stripes is compared
    assert all((s, i) in t.out for s in range(4) for i in case.lost_data) and C.VERIFY_STRIPES == 7
    if C.spares(case):
        assert failed == {6} and not t.flags_checked[6]
    else:
        assert failed == {4, 5} and t.flags_checked.all()


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_queue_tile_counts_and_shapes(cus):
    W = C.queue_waves(cus)
    counts = dict(C.queue_tile_counts(cus))
    assert tuple(counts) == C.QUEUE_T
    assert counts["3w+5"] > 3 * W and counts["2cus-1"] < 2 * cus < counts["2cus+1"] <= W
    assert [counts[n] for n in ("1", "7", "8", "9")] == [1, 7, 8, 9]
    for _, k, m, e, wt in C.QUEUE_KERNELS:
        for name, T in counts.items():
            S, cell = C.queue_shape(T, wt)
            assert C.fused_tiles(S, cell, wt) == T and cell % 16 == 0
            assert cell % wt == C.LAST_TILE and cell % 512 == 16   # dead slabs and a 16-byte last chunk
        S, cell = C.queue_shape(counts["3w+5"], wt)
        assert S > 32 and S * cell * (k + m) <= 400 << 20   # a late tile exists; the oracle's share stays small
    case = C.VerifyCase(6, 3, 3, C.CRC32C, (0, 1, 2), (), (), "late")
    assert C.late_flip(case, 40, 4096 + C.LAST_TILE) == [(39, 8, 4096 + C.LAST_TILE - 1)]


def test_block_tile_and_sequence_cases():
    assert C.BLOCK_CELL == 36368 and C.BLOCK_STRIPES == 6 and C.BLOCK_GRIDS == (1, 5)
    # 12 tiles of 32 KiB (8 slabs) or 18 of 16 KiB (4 slabs): more than 5 blocks can take in one pass
    assert C.fused_tiles(6, C.BLOCK_CELL, 32768) == 12 and C.fused_tiles(6, C.BLOCK_CELL, 16384) == 18
    plans = {(k, e, g): C.block_lost(k, e, g) for k, _, e in C.BLOCK_VERIFY for g in C.BLOCK_GRIDS}
    assert len(set(plans.values())) == len(plans)
    assert all(len(v) == e for (_, e, _), v in plans.items())
    assert C.sequence_tiles(256) == (3 * 2048 + 5, 1, 9, 9) and C.sequence_tiles(256, graph=True) == (513, 1, 9, 9)
