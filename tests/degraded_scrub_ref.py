"""Reference for the degraded scrub (hec_scrub_degraded, hec_scrub_device_mixed),
shared by test_scrub_degraded.py and test_gpu_scrub_mixed.py.  It does not use
the engine's algebra (syndromes against G, 2x2 minors); it restates the result
as rebuilds and comparisons over the oracle's matrix routines:

  * a position is bad when some present unit differs from the codeword rebuilt
    from the first k present units;
  * a present unit t is NOT ruled out iff replacing t by its rebuild from the
    first k of the OTHER present units leaves every other present unit
    consistent with that codeword;
  * a missing unit is ruled out as soon as a position is bad;
  * k present units or fewer: nothing to check against, (0, 0).

Two shortcuts keep it quick, neither changes the statement.  The second step
looks at the bad positions only: where every present unit already agrees with
one codeword, replacing a unit by its rebuild reproduces that codeword, so no
unit is ruled out there.  And the rebuild of a unit the codeword was rebuilt
from is that unit (its row of C . inverse(C[S]) is a unit vector), so only the
rows of the other units are multiplied out."""
import functools

import numpy as np

import ec_oracle as O


@functools.lru_cache(maxsize=None)
def _matrix(codec, k, m):
    return O.codec_matrix(codec, k, m)


@functools.lru_cache(maxsize=None)
def _rebuild_rows(codec, k, m, basis, rows):
    """Rows `rows` of C . inverse(select_rows(C, basis))."""
    C = _matrix(codec, k, m)
    return O.matmul(O.select_rows(C, rows), O.invert(O.select_rows(C, basis)))


def present_units(n, mask):
    return [i for i in range(n) if (mask >> i) & 1]


def oracle_plan(codec, k, m, mask):
    """(survivors, extras, G) of a presence mask by the oracle."""
    pres = present_units(k + m, mask)
    if len(pres) <= k:
        return [], [], []
    S, E = pres[:k], pres[k:]
    return S, E, _rebuild_rows(codec, k, m, tuple(S), tuple(E))


def _disagree(codec, k, m, units, basis, others):
    """Per position: does some unit of `others` differ from the codeword the
    units of `basis` span?"""
    out = np.zeros(len(units[basis[0]]), dtype=bool)
    if not others:
        return out
    rebuilt = O.matmul_shards(_rebuild_rows(codec, k, m, tuple(basis), tuple(others)), [units[i] for i in basis])
    for r, t in zip(rebuilt, others):
        out |= r != units[t]
    return out


def ref_batch(codec, k, m, cells, masks):
    """uint64 [stripes, 2] for a batch cells[stripes, k+m, cell] with one mask
    per stripe: ref_scrub of every stripe.  The first step runs once per
    distinct mask over all of its stripes at once; a stripe it finds clean is
    (0, 0) by ref_scrub's own first step."""
    n = k + m
    out = np.zeros((cells.shape[0], 2), dtype=np.uint64)
    groups = {}
    for st, mask in enumerate(masks):
        groups.setdefault(int(mask) & ((1 << n) - 1), []).append(st)
    for mask, idx in groups.items():
        pres = present_units(n, mask)
        if len(pres) <= k:
            continue
        flat = {t: np.ascontiguousarray(cells[idx, t]).reshape(-1) for t in pres}
        bad = _disagree(codec, k, m, flat, pres[:k], pres[k:]).reshape(len(idx), -1)
        for x in np.nonzero(bad.any(axis=1))[0]:
            out[idx[x]] = ref_scrub(codec, k, m, cells[idx[x]], mask)
    return out


def ref_scrub(codec, k, m, units, mask):
    """(ruled_out, bad_bytes) of one stripe; units[t] is read only for the
    units in mask (uint8 arrays of one length)."""
    n = k + m
    pres = present_units(n, mask)
    if len(pres) <= k:
        return 0, 0
    bad = np.nonzero(_disagree(codec, k, m, units, pres[:k], pres[k:]))[0]
    if len(bad) == 0:
        return 0, 0
    at_bad = {t: np.ascontiguousarray(units[t][bad]) for t in pres}
    ruled = ~mask & ((1 << n) - 1)
    for t in pres:
        others = [i for i in pres if i != t]
        if _disagree(codec, k, m, at_bad, others[:k], others[k:]).any():
            ruled |= 1 << t
    return ruled, len(bad)
