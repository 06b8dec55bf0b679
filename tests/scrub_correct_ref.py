"""The definition of scrub correction (hec_scrub_correct[_device]) restated in
numpy over the oracle's matrix and product table, shared by
test_scrub_correct.py and test_gpu_scrub_correct.py:

  the scrub's pair    syndromes s_j = sum_i P[j][i] u_i ^ u_{k+j}; bad_bytes =
                      positions with a non-zero syndrome vector; ruled_out bit
                      t when some position's vector has a non-zero 2x2 minor
                      against column t of H = [P | I];
  the verdict         cand = ~ruled_out & ((1 << (k+m)) - 1); LOCATED iff
                      bad_bytes != 0 and popcount(cand) == 1, t = ctz(cand);
                      -1 for a clean stripe, -2 for any other;
  the correction      u_t ^= scale * s_row, with row = the first j with
                      P[j][t] != 0 and scale = 1 / P[j][t] for a data unit,
                      row = t - k and scale = 1 for a parity unit.
"""
import numpy as np

import ec_oracle as O

CLEAN, UNLOCATED = -1, -2


def verdict(ruled_out, bad_bytes, n):
    if bad_bytes == 0:
        return CLEAN
    cand = ~int(ruled_out) & ((1 << n) - 1)
    if bin(cand).count("1") != 1:
        return UNLOCATED
    return cand.bit_length() - 1


def _inverse(c):
    (x,) = [x for x in range(1, 256) if O.MUL_TABLE[c][x] == 1]
    return x


def correct_batch(codec, k, m, cells):
    """cells: uint8 [stripes, k+m, cell].  -> (results uint64 [stripes, 2] of
    the cells as given, units int32 [stripes], the corrected cells)."""
    C = O.codec_matrix(codec, k, m)
    P = np.array(C[k:], dtype=np.uint8)
    Hm = np.concatenate([P, np.eye(m, dtype=np.uint8)], axis=1)
    s = np.ascontiguousarray(cells[:, k:].transpose(1, 0, 2)).copy()  # [m, stripes, cell]
    for j in range(m):
        for i in range(k):
            s[j] ^= np.asarray(O.MUL_TABLE[P[j, i]], dtype=np.uint8)[cells[:, i]]
    results = np.zeros((cells.shape[0], 2), dtype=np.uint64)
    units = np.full(cells.shape[0], CLEAN, dtype=np.int32)
    out = np.array(cells)
    for st in np.nonzero(s.any(axis=(0, 2)))[0]:
        bad = np.nonzero(s[:, st].any(axis=0))[0]
        sb = s[:, st][:, bad]
        ruled = 0
        for t in range(k + m):
            for i in range(m):
                for j in range(i + 1, m):
                    if (np.asarray(O.MUL_TABLE[Hm[j, t]], dtype=np.uint8)[sb[i]]
                            ^ np.asarray(O.MUL_TABLE[Hm[i, t]], dtype=np.uint8)[sb[j]]).any():
                        ruled |= 1 << t
        results[st] = (ruled, len(bad))
        t = verdict(ruled, len(bad), k + m)
        units[st] = t
        if t >= 0:
            if t < k:
                row = [j for j in range(m) if P[j, t] != 0][0]
                scale = _inverse(int(P[row, t]))
            else:
                row, scale = t - k, 1
            out[st, t] ^= np.asarray(O.MUL_TABLE[scale], dtype=np.uint8)[s[row, st]]
    return results, units, out


def correct_stripe(codec, k, m, units):
    """One stripe as a list of k+m uint8 arrays.  -> (ruled_out, bad_bytes,
    unit, the corrected units as one [k+m, len] array)."""
    results, unit, out = correct_batch(codec, k, m, np.stack(units)[None])
    return int(results[0, 0]), int(results[0, 1]), int(unit[0]), out[0]
