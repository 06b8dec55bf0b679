"""Composite CRCs restated from their definition, one bit at a time, on
Python ints: the second reference of test_composite_crc.py and
test_gpu_composite_crc.py, for sums that are the CRC of no data.

Polynomials are ints with bit i the coefficient of x^i, whatever the CRC's
own bit order; a reflected register is bit-reversed on the way in and out.

    crc(A || B) = L_|B|(crc(A) ^ xorout ^ init) ^ crc(B),  L_n(r) = r x^(8n) mod P
"""
import functools

CRC32 = 1   # CRC_32_CKSUM: MSB-first, init 0, xorout 0xFFFFFFFF
CRC32C = 2  # CRC_32_ISCSI: reflected, init and xorout 0xFFFFFFFF

_SPEC = {  # full polynomial (x^32 included), reflected, init, xorout
    CRC32: (0x104C11DB7, False, 0x00000000, 0xFFFFFFFF),
    CRC32C: (0x11EDC6F41, True, 0xFFFFFFFF, 0xFFFFFFFF),
}


def _rev32(v):
    return int(format(v, "032b")[::-1], 2)


def _mulmod(a, b, poly):
    prod = 0
    while b:  # carry-less product
        if b & 1:
            prod ^= a
        a <<= 1
        b >>= 1
    for bit in range(prod.bit_length() - 1, 31, -1):  # reduce mod P
        if prod >> bit & 1:
            prod ^= poly << (bit - 32)
    return prod


@functools.lru_cache(maxsize=None)
def _xpow8(ctype, n):
    """x^(8n) mod P by repeated squaring."""
    poly = _SPEC[ctype][0]
    result, square = 1, 1 << 8
    while n:
        if n & 1:
            result = _mulmod(result, square, poly)
        square = _mulmod(square, square, poly)
        n >>= 1
    return result


def crc_empty(ctype):
    _, _, init, xorout = _SPEC[ctype]
    return init ^ xorout


def concat(ctype, crc_a, crc_b, len_b):
    poly, reflected, init, xorout = _SPEC[ctype]
    r = crc_a ^ xorout ^ init
    if reflected:
        r = _rev32(r)
    r = _mulmod(r, _xpow8(ctype, len_b), poly)
    if reflected:
        r = _rev32(r)
    return r ^ crc_b


def cell_lengths(n, k, cell, stripes, data_len):
    """len(s, u) of the issue's definition, as [stripes][n]."""
    total = stripes * k * cell
    if data_len == 0:
        data_len = total
    assert total - k * cell < data_len <= total
    r = data_len - (stripes - 1) * k * cell
    last = [min(cell, max(0, r - u * cell)) if u < k else min(cell, r) for u in range(n)]
    return [[cell] * n for _ in range(stripes - 1)] + [last]


def composite(ctype, sums, n, k, cell, stripes, bpc, data_len=0):
    """sums[s][u][c]: chunk CRCs as ints.  Returns (cell_crcs [stripes][n],
    unit_crcs [n], group_crc)."""
    lens = cell_lengths(n, k, cell, stripes, data_len)
    cells = []
    for s in range(stripes):
        row = []
        for u in range(n):
            crc, left, c = crc_empty(ctype), lens[s][u], 0
            while left:
                part = min(bpc, left)
                crc = concat(ctype, crc, sums[s][u][c], part)
                left -= part
                c += 1
            row.append(crc)
        cells.append(row)
    units = []
    for u in range(n):
        crc = crc_empty(ctype)
        for s in range(stripes):
            crc = concat(ctype, crc, cells[s][u], lens[s][u])
        units.append(crc)
    group = crc_empty(ctype)
    for s in range(stripes):
        for u in range(k):
            group = concat(ctype, group, cells[s][u], lens[s][u])
    return cells, units, group
