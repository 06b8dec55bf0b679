"""The register kernels behind the verified calls in launches where a block
takes a second and later tile (`for (tile = blockIdx.x; tile < total; tile +=
gridDim.x)`): gf_reconstruct_crc with and without its output stores,
gf_scrub_crc, gf_crc_rows<RowsRepair>, gf_crc_rows<RowsEncode>,
gf_scrub_crc_rows and gf_read_rows.  On the product library's grids (32, 4 or 2
blocks per CU) that takes more than 8192, 1024 or 512 tiles on 256 CUs; the
other tests of these kernels stay below 100, so the second pass of the loop
(accumulators zeroed again, the LDS checksum stage written over what the last
tile left, another stripe's lengths, the stripe list read again, findings of
two tiles merged) ran in no test.

  Part A  the product library on its default grid: many small stripes, the
          stripe count computed from the device's CU count
  Part B  the measurement build on a grid of 1 and 5 blocks (tune key 7) with
          tile-order groups of 8, 1 and 3 stripes (tune key 8): small batches
          of multi-tile cells, every block loops
  Part 5  the byte-wise kernels with more work items than their 8 blocks per CU
          hold lanes

verified_loop_cases.py holds the case lists and a model of the tile order;
test_verified_loop_cases.py asserts from it that the cases loop where they
claim to.  The reference is the oracle throughout, through the buffer classes
of the tests that swept these kernels at small tile counts: every cell, sum,
flag and result word of every buffer is compared for equality."""
import numpy as np
import pytest

import hdfs_native_ec as H
import rows_shape_cases as P
import test_gpu_encode_crc_rows as ER
import test_gpu_reconstruct_crc as RC
import test_gpu_reconstruct_crc_rows as RR
import test_gpu_reconstruct_sums as RS
import test_gpu_scrub_crc as SC
import test_gpu_scrub_crc_rows as SR
import verified_loop_cases as L
from test_gpu_encode_crc_rows import Enc
from test_gpu_fused_launch import cu_count, needs_measurement_build
from test_gpu_read_crc_rows import ReadCase
from test_gpu_reconstruct_crc_rows import Case as RepairCase
from test_gpu_scrub_crc_rows import Batch as ScrubRowsBatch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CT = {"crc32c": H.CHECKSUM_CRC32C, "crc32": H.CHECKSUM_CRC32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def forget_large_batches():
    """The truth of a batch is kept by the modules that build it; the batches
    here hold tens of MB each."""
    yield
    for module in (RC, RR, ER, SR):
        module.forget(8 << 20)


_coders = {}


def coder(k, m, lib=None):
    key = (k, m, id(lib))
    if key not in _coders:
        _coders[key] = H.Coder(k, m, 0, "rs", lib=lib)
    return _coders[key]


# ---- one call of each family, clean and with bent bytes -----------------------------------

def run_recon(dev, family, cod, k, m, S, cell, losts, form, verify, ctype, flips, what, bpc=512):
    """gf_reconstruct_crc: the uniform call or the mixed one (a stripe list per
    pattern), rebuilt cells stored (recon) or checksummed only (sums).  Clean:
    every rebuilt byte and sum, no flag.  With flips (verify only): exactly the
    bent survivors' cells flagged, nothing else changes."""
    mod = RC if family == "recon" else RS
    for corrupt in ([], flips) if verify else ([],):
        kw = dict(expected="sep" if verify else None, corrupt=corrupt, ctype=ctype, bpc=bpc)
        if form == "uniform":
            c = mod.uniform_case(cod, k, m, S, cell, losts[0], dev, **kw)
            c.uniform()
        else:
            c = mod.mixed_case(cod, k, m, S, cell, losts, dev, **kw)
            if family == "recon":
                c.mixed()
            else:
                H.reconstruct_sums_batch(cod, c.cells, [RC.present_mask(k + m, l) for l in losts], c.sums,
                                         expected=c.expected, bad=c.bad if verify else None, checksum_type=ctype,
                                         bytes_per_checksum=bpc)
        torch.cuda.synchronize()
        assert int(c.exp_bad.sum()) == len(corrupt) and c.dirty == {s for s, _, _ in corrupt}
        c.check((what, "bent", corrupt))


def run_scrub(dev, cod, k, m, S, cell, masks, ctype, found, what):
    """gf_scrub_crc, uniform (masks None) or behind a stripe list per mask.
    found: L.Corruption; a silent one has its chunk sum recomputed to match."""
    for bent in ([], found):
        cells, sums = SC.clean("rs", k, m, S, cell, ctype=ctype)
        for c in bent:
            cells[c.stripe, c.unit, c.byte] ^= 0x40
        for c in bent:
            if c.silent:
                SC.resum(cells, sums, c.stripe, c.unit, ctype=ctype)
        b = SC.Batch("rs", k, m, cells, sums, dev, masks=masks, ctype=ctype)
        b.call(cod)
        # what the corruptions are there to show, from the references alone
        assert sorted(map(tuple, np.argwhere(b.want_bad))) == sorted({(c.stripe, c.unit) for c in bent if not c.silent})
        assert set(np.nonzero(b.want_res[:, 1])[0]) == {c.stripe for c in bent}
        b.check((what, "bent", bent))


def run_rows(dev, family, cod, k, m, cell, rs, lost, form, verify, ctype, flips, what, bpc=512):
    """The short-stripe calls: form "mixed" = one length per stripe, "data_len" =
    the uniform call with a short last stripe."""
    S, n = len(rs), k + m
    for corrupt in ([], flips) if flips else ([],):
        if family == "repair_rows":
            c = RepairCase(cod, k, m, cell, rs, [lost] * S, dev, expected="sep" if verify else None, corrupt=corrupt,
                           ctype=ctype, bpc=bpc)
            c.mixed() if form == "mixed" else c.uniform()
        elif family == "encode_rows":
            c = Enc(cod, k, m, cell, rs, dev, ctype=ctype, bpc=bpc)
            c.mixed() if form == "mixed" else c.uniform()
        else:
            c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev, verify=verify, corrupt=corrupt, ctype=ctype, bpc=bpc)
            c.mixed() if form == "mixed" else c.uniform()
        torch.cuda.synchronize()
        if family in ("repair_rows", "read_rows"):
            assert c.dirty == {s for s, _, _ in corrupt}
            if verify:
                assert int(c.exp_bad.sum()) == len(corrupt)
        c.check((what, "bent", corrupt))


def run_scrub_rows(dev, cod, k, m, cell, rs, absent, form, ctype, found, by_sum, what, bpc=512):
    """gf_scrub_crc_rows (16-byte chunks: gf_scrub_rows_bytes).  found:
    L.Corruption, silent ones with their unit's sums recomputed; by_sum =
    (stripe, unit, byte): the expected sum of that byte's chunk is wrong
    instead (None: none)."""
    S, n = len(rs), k + m
    masks = [RC.present_mask(n, absent)] * S if absent else None
    lens = [P.unit_lens(k, n, cell, r) for r in rs]
    for bent in ([], found) if found else ([],):
        sums = [(by_sum[0], by_sum[1], by_sum[2] // bpc)] if bent and by_sum else []
        c = ScrubRowsBatch("rs", k, m, cell, rs, dev, masks=masks, corrupt=[f[:3] for f in bent if not f.silent],
                           silent=[f[:3] for f in bent if f.silent], corrupt_sums=sums, ctype=ctype, bpc=bpc)
        c.mixed(cod) if form == "mixed" else c.uniform(cod)
        # what the corruptions are there to show, from the references alone
        assert all(f.byte < lens[f.stripe][f.unit] for f in bent)
        assert sorted(map(tuple, np.argwhere(c.want_bad))) == sorted({(f.stripe, f.unit) for f in bent if not f.silent}
                                                                     | {f[:2] for f in sums})
        assert set(np.nonzero(c.want_res[:, 1])[0]) == {f.stripe for f in bent}
        torch.cuda.synchronize()
        c.check((what, "bent", bent, sums))


# ---- part A: the product library, default grid ----------------------------------------------

@pytest.mark.parametrize("case", L.RECON_A, ids=lambda c: c.name)
def test_default_grid_reconstruction(dev, case):
    """32 CUs + 37 stripes of single-tile cells: 37 blocks take a second tile."""
    cus = cu_count()
    S, main = L.recon_batch(case, cus)
    losts = L.recon_losts(case, S, main)
    run_recon(dev, case.family, coder(case.k, case.m), case.k, case.m, S, case.cell, losts, case.form, case.expected,
              CT[case.ctype], L.recon_flips(case, cus), case.name)


@pytest.mark.parametrize("case", L.SCRUB_A, ids=lambda c: c.name)
def test_default_grid_scrub(dev, case):
    """Two-tile cells, 38 tiles past the grid of 4 (uniform) or 2 (stripe list)
    blocks per CU."""
    cus, n = cu_count(), case.k + case.m
    S, main = L.scrub_batch(case, cus)
    masks = None
    if case.form == "degraded":
        masks = [SC.full(n)] * S
        for s in main:
            masks[s] = SC.lose(n, case.absent)
    run_scrub(dev, coder(case.k, case.m), case.k, case.m, S, L.scrub_cell(case), masks, CT[case.ctype],
              L.scrub_case_corruptions(case, cus), case.name)


@pytest.mark.parametrize("case", L.ROWS_A, ids=lambda c: c.name)
def test_default_grid_rows(dev, case):
    """More short stripes than the grid, a block's consecutive tiles of
    different lengths; and the same lengths as the short last stripe of a
    data_len call whose full stripes outnumber the grid."""
    cus = cu_count()
    rs = L.rows_lengths(case, cus)
    if case.family == "scrub_rows":
        found, by_sum = L.rows_scrub_case_corruptions(case, cus) if case.form == "mixed" else ([], None)
        run_scrub_rows(dev, coder(case.k, case.m), case.k, case.m, case.cell, rs, case.lost, case.form, CT[case.ctype],
                       found, by_sum, case.name)
        return
    flips = L.rows_flips(case, cus) if case.form == "mixed" and case.family != "encode_rows" else []
    run_rows(dev, case.family, coder(case.k, case.m), case.k, case.m, case.cell, rs, case.lost, case.form, True,
             CT[case.ctype], flips, case.name)


# ---- part B: the measurement build, 1 and 5 blocks ------------------------------------------

@needs_measurement_build
@pytest.mark.parametrize("case", L.LOOP_B, ids=lambda c: c.name)
def test_small_grid_loops(dev, case):
    """Every block takes at least two tiles: full and short ones in both
    orders, tiles of one stripe, of a whole group and of the remainder."""
    xlib = H.experimental_lib()
    k, m, n, ctype = case.k, case.m, case.k + case.m, CT[case.ctype]
    cod = coder(k, m, xlib)
    flips = L.loop_flips(case)
    try:
        H.tune_set(7, case.grid, xlib)
        H.tune_set(8, case.group, xlib)
        if case.family in ("recon", "sums"):
            run_recon(dev, case.family, cod, k, m, case.S, case.cell, [case.lost] * case.S, "uniform", case.verify,
                      ctype, flips, case.name)
        elif case.family == "scrub":
            found = [L.Corruption(s, u, b, x % 2 == 0) for x, (s, u, b) in enumerate(flips)]
            run_scrub(dev, cod, k, m, case.S, case.cell, None, ctype, found, case.name)
        elif case.family == "scrub_rows":
            found, by_sum = L.loop_scrub_rows_corruptions(case)
            run_scrub_rows(dev, cod, k, m, case.cell, L.loop_lengths(case), case.lost, "mixed", ctype, found, by_sum,
                           case.name)
        else:
            if case.family == "encode_rows" or not case.verify:
                flips = []
            run_rows(dev, case.family, cod, k, m, case.cell, L.loop_lengths(case), case.lost, "mixed", case.verify,
                     ctype, flips, case.name)
    finally:
        H.tune_set(7, 0, xlib)
        H.tune_set(8, 0, xlib)


# ---- part 5: the byte-wise kernels ------------------------------------------------------------

@pytest.mark.parametrize("case", L.BYTE_CASES, ids=lambda c: c.name)
def test_byte_kernels_past_their_lanes(dev, case):
    """16-byte chunks: more (stripe, row, chunk) items than 8 blocks per CU have
    lanes, so the lanes stride on to a second item.  One byte bent in each of the last
    two stripes, whose items all lie past the first stride."""
    cus = cu_count()
    k, m, S, cell = case.k, case.m, L.byte_stripes(case, cus), L.BYTES_CELL
    flips = L.byte_flips(case, cus)
    if case.family == "sums":
        run_recon(dev, "sums", coder(k, m), k, m, S, cell, [case.lost] * S, "uniform", True, CT["crc32c"], flips,
                  case.name, bpc=L.BYTES_BPC)
        return
    rs = L.byte_lengths(case, cus)
    if case.family == "scrub_rows":
        found = [L.Corruption(*flips[0], False), L.Corruption(*flips[1], True)]
        run_scrub_rows(dev, coder(k, m), k, m, cell, rs, case.lost, "mixed", CT["crc32c"], found, None, case.name,
                       bpc=L.BYTES_BPC)
        return
    run_rows(dev, case.family, coder(k, m), k, m, cell, rs, case.lost, "mixed", True, CT["crc32c"],
             [] if case.family == "encode_rows" else flips, case.name, bpc=L.BYTES_BPC)
