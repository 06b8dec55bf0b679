"""Cases for the composite-CRC tests, with the oracle as ground truth: random
cells, their chunk sums from the oracle's orc_chunk_checksum, and the cell,
unit and group CRCs as the oracle's CRC over the actual concatenated bytes."""
import ctypes

import numpy as np

from composite_crc_ref import CRC32, cell_lengths


def oracle_crc(clib, ctype, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    fn = clib.orc_crc32_cksum if ctype == CRC32 else clib.orc_crc32c
    return fn(arr.ctypes.data_as(ctypes.c_void_p), arr.size)


def data_len_cases(k, cell, stripes):
    """0, the full length, the last stripe cut to one byte, cut exactly at a
    cell boundary, cut inside a cell so that the data cells after it are empty."""
    before = (stripes - 1) * k * cell
    boundary = before + max(1, k // 2) * cell
    inside = before + (cell if k >= 3 else 0) + max(1, cell // 2)
    return [0, stripes * k * cell, before + 1, boundary, inside]


def build(clib, ctype, n, k, cell, stripes, bpc, data_len, seed, dead=0xA5):
    """Returns (sums, cells, units, group): sums is uint8 [stripes][n][nck][4]
    with the slots no chunk covers filled with `dead`; the expected CRCs are
    uint32 arrays [stripes][n] and [n] and an int."""
    rng = np.random.default_rng(seed)
    lens = cell_lengths(n, k, cell, stripes, data_len)
    nck = -(-cell // bpc)
    raw = rng.integers(0, 256, (stripes, n, cell), dtype=np.uint8)
    sums = np.full((stripes, n, nck, 4), dead, dtype=np.uint8)
    cells = np.zeros((stripes, n), dtype=np.uint32)
    for s in range(stripes):
        for u in range(n):
            part = np.ascontiguousarray(raw[s, u, :lens[s][u]])
            cells[s, u] = oracle_crc(clib, ctype, part)
            if part.size:
                out = np.zeros((-(-part.size // bpc), 4), dtype=np.uint8)
                clib.orc_chunk_checksum(ctype, part.ctypes.data_as(ctypes.c_void_p), part.size, bpc,
                                        out.ctypes.data_as(ctypes.c_void_p))
                sums[s, u, :out.shape[0]] = out
    units = np.array([oracle_crc(clib, ctype, np.concatenate([raw[s, u, :lens[s][u]] for s in range(stripes)]))
                      for u in range(n)], dtype=np.uint32)
    logical = sum(lens[s][u] for s in range(stripes) for u in range(k))
    group = oracle_crc(clib, ctype, np.ascontiguousarray(raw[:, :k, :]).reshape(-1)[:logical])
    return sums, cells, units, group


def be_words(buf, shape=None):
    """Big-endian u32 of a byte buffer, as a uint32 array."""
    w = np.frombuffer(bytes(buf), dtype=">u4").astype(np.uint32)
    return w if shape is None else w.reshape(shape)
