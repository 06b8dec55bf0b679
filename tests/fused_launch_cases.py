"""Case generators and host references of test_gpu_fused_launch.py and
fused_generic_child.py (numpy and the oracle only, so test_fused_launch_cases.py
checks them without a GPU).

Part 1, every instantiation of gf_fused_crc the product library compiles
(csrc/ec_fused.hip launch_fused), at the two smallest cells that reach every
branch of a block tile: 32768 bytes (exactly one 8-slab block tile) and 36368
bytes = 32 KiB + 3 KiB + 528 (a second tile in which most waves are past the
end, dead slabs, a last chunk of 16 bytes; still a multiple of 16, so the fused
path is taken), 4 stripes.  encode_cases(): the 23 encode + CRC cases;
fallback_cases(): 5 shapes launch_fused refuses, so the two-pass path is pinned
the same way; generic_cases() and specialised_cases(): decode + verify.

A decode + verify case names K, the number E of lost data units (the kernel's
R) and the checksum type.  launch_fused compiles the generic kernel for all 16
(K, R), but a stripe has K data units, so E <= K: (2,3), (2,4) and (3,4) cannot
be asked for through hec_decode_verify_device by any caller (UNREACHABLE).  The
13 reachable shapes x 2 checksum types are the generic cases.  Half of them
(by rotation, so every shape and either type sees both) run as Coder(K, E) with
E data units lost: no spare unit, every survivor needed.  The other half run as
Coder(K, E + 2) with parity unit 0 lost as well: the survivors then start
behind a lost parity unit (shard_id is not the identity and skips a parity
index) and one spare unit is left for the re-plan.  The specialised cases keep
the policy's own m, with parity unit 0 lost where E + 1 <= m, by the same
rotation.

Every verify batch holds 7 stripes (verify_flips).  Stripes 0 to 3 are the
four data kinds below and stay clean, so that what the kernel itself rebuilds
from all-zero, all-0xFF and last-byte data is compared (a bent stripe's cells
are written again by the re-plan, or left unspecified).  The bent stripes are
random data:
  stripe 4  byte 3 of the first survivor flipped;
  stripe 5  the last byte of the last survivor flipped (at 36368-byte cells it
            lies in the 16-byte last chunk, which one lane walks bytewise);
  stripe 6  with spare units: one failure too many (the first spare + 1
            available units bent at bytes 100, 101, ...), which must raise and
            whose flags are not compared; without a spare: clean.
Without a spare, stripes 4 and 5 cannot be rebuilt either: the call raises, the
flag of exactly the bent unit is set, and their lost cells are unspecified.

Data of a batch (batch_data): stripe 0 random, stripe 1 all zero, stripe 2 all
0xFF, stripe 3 zero except its last byte, any further stripe random.  The last
three are there for the CRCs' init / xorout and the GF zero handling.

Part 2, waves that take several tiles: queue_tile_counts(cus) and queue_shape.
Part 3, one stream and a graph: sequence_tiles.

References: parity from orc_encode_batch, rebuilt data from orc_decode (the
oracle's own plan: the first k present units), chunk sums from
orc_chunk_checksum; verified_read_expect restates ec_oracle.verified_read_row
over them (the Python CRC of ec_oracle would take a minute for the 26 + 20
batches; test_fused_launch_cases.py holds the two against each other).  No
device kernel is a reference anywhere."""
import collections
import threading

import numpy as np

import ec_oracle as O

BPC = 512
PITCH_GAP = 64                  # rows have a pitch of cell + 64
CELLS = (32768, 36368)
STRIPES = 4                     # encode batches: one stripe of each data kind
VERIFY_STRIPES = 7              # verify batches: the four kinds clean, three random stripes to bend
DATA_KINDS = ("random", "zero", "ones", "last-byte")
LAST_BYTE = 0x5A                # the one non-zero byte of a "last-byte" stripe
FLIP = 0x40
CRC32, CRC32C = O.CHECKSUM_CRC32, O.CHECKSUM_CRC32C
FUSED_K = (2, 3, 6, 10)
FUSED_R = (1, 2, 3, 4)
RS = {2: 1, 3: 2, 6: 3, 10: 4}  # the policies' m
THREADS = 16                    # at most; the oracle calls release the GIL

_clib = []


def clib():
    if not _clib:
        _clib.append(O.load_c_oracle())
    return _clib[0]


def _parallel(stripes, work):
    """work(a, b) over [0, stripes) cut into at most THREADS ranges."""
    n = max(1, min(THREADS, stripes // 8))
    if n == 1:
        work(0, stripes)
        return
    ths = [threading.Thread(target=work, args=(stripes * t // n, stripes * (t + 1) // n)) for t in range(n)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()


# ---- data -------------------------------------------------------------------------------

def stripe_kind(s):
    return DATA_KINDS[s] if s < len(DATA_KINDS) else "random"


def batch_data(k, stripes, cell, seed):
    """[stripes, k, cell]: random, with stripes 1, 2 and 3 (where they exist)
    all zero, all 0xFF and zero except the last byte of every unit."""
    data = np.random.default_rng(seed).integers(0, 256, size=(stripes, k, cell), dtype=np.uint8)
    for s in range(min(stripes, len(DATA_KINDS))):
        kind = stripe_kind(s)
        if kind == "zero":
            data[s] = 0
        elif kind == "ones":
            data[s] = 0xFF
        elif kind == "last-byte":
            data[s] = 0
            data[s, :, cell - 1] = LAST_BYTE
    return data


# ---- references --------------------------------------------------------------------------

def encode_ref(k, m, data):
    """The C oracle's RS parity of data [S, k, cell]: [S, m, cell]."""
    S, _, n = data.shape
    data = np.ascontiguousarray(data)
    par = np.empty((S, m, n), dtype=np.uint8)
    rcs = []

    def work(a, b):
        rcs.append(clib().orc_encode_batch(k, m, data[a:b].ctypes.data, n, b - a, par[a:b].ctypes.data))

    _parallel(S, work)
    assert all(rc == 0 for rc in rcs), rcs
    return par


def matrix_parity(rows, data):
    """ec_oracle.matmul_shards of the parity rows of a codec's matrix over data
    [S, k, cell]: [S, len(rows), cell].  This pins a kernel against the matrix
    it was given, not the matrix itself."""
    S, k, n = data.shape
    flat = [np.ascontiguousarray(data[:, i]).reshape(-1) for i in range(k)]
    out = O.matmul_shards([list(r) for r in rows], flat)
    return np.stack([o.reshape(S, n) for o in out], axis=1)


def decode_ref(k, m, data, parity, present):
    """The C oracle's decode with the units of the bit mask `present`: the lost
    data units in ascending order, [S, e, cell]."""
    import ctypes
    S, _, n = data.shape
    e = sum(1 for i in range(k) if not (present >> i) & 1)
    data, parity = np.ascontiguousarray(data), np.ascontiguousarray(parity)
    out = np.empty((S, e, n), dtype=np.uint8)
    rcs = []

    def work(a, b):
        rcs.append(clib().orc_decode_batch(k, m, data[a:b].ctypes.data, parity[a:b].ctypes.data, n, b - a,
                                           ctypes.c_uint64(present), out[a:b].ctypes.data))

    _parallel(S, work)
    assert all(rc == 0 for rc in rcs), rcs
    return out


def chunk_sums(cells, ctype, bpc=BPC):
    """orc_chunk_checksum of every cell of cells [S, n, cell]: [S, n, nck, 4]."""
    S, n, cell = cells.shape
    cells = np.ascontiguousarray(cells)
    nck = -(-cell // bpc)
    out = np.empty((S, n, nck, 4), dtype=np.uint8)

    def work(a, b):
        lib = clib()
        for s in range(a, b):
            for u in range(n):
                lib.orc_chunk_checksum(ctype, cells[s, u].ctypes.data, cell, bpc, out[s, u].ctypes.data)

    _parallel(S, work)
    return out


def checksum(ctype, message):
    """One checksum of a whole message through the same reference call."""
    buf = np.frombuffer(bytes(message), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint8)
    if len(buf):
        clib().orc_chunk_checksum(ctype, buf.ctypes.data, len(buf), len(buf), out.ctypes.data)
        return int.from_bytes(out.tobytes(), "big")
    return {CRC32: 0xFFFFFFFF, CRC32C: 0}[ctype]


def verified_read_row(k, m, cells, sums, ctype, bpc=BPC):
    """ec_oracle.verified_read_row over the C oracle: cells [k + m] (None = no
    reader) are taken in index order, one whose chunk sums differ from sums[i]
    is flagged and the next unit read, until k good ones are held; then the
    oracle's decode.  Returns (data [k] or None when fewer than k verify, flags
    [k + m]); in the None case the flags are those of every available cell
    that fails, as test_gpu_parity._verified_read_expect states them."""
    n = k + m
    bad = np.zeros(n, dtype=np.uint8)
    good, held = [None] * n, 0

    def fails(i):
        return not np.array_equal(chunk_sums(cells[i][None, None], ctype, bpc)[0, 0], sums[i])

    for i in range(n):
        if held == k:
            break
        if cells[i] is None:
            continue
        if fails(i):
            bad[i] = 1
        else:
            good[i] = cells[i]
            held += 1
    if held < k:
        for i in range(n):
            bad[i] = 1 if cells[i] is not None and fails(i) else 0
        return None, bad
    full = O.c_decode(clib(), k, m, good)
    return [np.asarray(full[i]) for i in range(k)], bad


# ---- part 1: encode + CRC ----------------------------------------------------------------

EncodeCase = collections.namedtuple("EncodeCase", "codec k m cells bpc data_off name")


def _enc(codec, k, m, cells=CELLS, bpc=BPC, data_off=0, tag=""):
    return EncodeCase(codec, k, m, tuple(cells), bpc, data_off, "%s-%d-%d%s" % (codec, k, m, tag))


def encode_cases():
    """The 23 shapes the fused encode + CRC takes: the RS matrix at all 16 (k,
    m) (the bit-sliced RsNet where a network exists, else the v_perm PermNet;
    the work queue at RS(3,2) and RS(10,4)), rs-legacy at the three policies
    (PermNet where rs runs RsNet) and xor at every k (PermNet, one row)."""
    cases = [_enc("rs", k, m) for k in FUSED_K for m in FUSED_R]
    cases += [_enc("rs-legacy", k, m) for k, m in ((3, 2), (6, 3), (10, 4))]
    cases += [_enc("xor", k, 1) for k in FUSED_K]
    return cases


def fallback_cases():
    """Shapes launch_fused refuses (encode, then a checksum pass): five parity
    units, k = 5, a cell that is no multiple of 16, 4096-byte chunks, and every
    data base one byte off the 16-byte grid."""
    big = CELLS[1:]
    return [_enc("rs", 6, 5, big, tag="-m5"), _enc("rs", 5, 3, big, tag="-k5"), _enc("rs", 6, 3, (1000,), tag="-cell1000"),
            _enc("rs", 6, 3, big, bpc=4096, tag="-bpc4096"), _enc("rs", 6, 3, big, data_off=1, tag="-off1")]


# ---- part 1: decode + verify -------------------------------------------------------------

VerifyCase = collections.namedtuple("VerifyCase", "k m e ctype lost_data lost_parity cells name")
UNREACHABLE = tuple((k, e) for k in FUSED_K for e in FUSED_R if e > k)


def lost_units(k, e):
    """e data units spread from the last one down: k - 1 - floor(j k / e)."""
    lost = sorted({k - 1 - (j * k) // e for j in range(e)})
    assert len(lost) == e
    return tuple(lost)


def _ver(k, m, e, ctype, parity_lost):
    name = "%d-%d-e%d-%s%s" % (k, m, e, "crc32c" if ctype == CRC32C else "crc32", "-p0" if parity_lost else "")
    return VerifyCase(k, m, e, ctype, lost_units(k, e), (0,) if parity_lost else (), CELLS, name)


def generic_cases():
    cases, x = [], 0
    for k in FUSED_K:
        for e in FUSED_R:
            if (k, e) in UNREACHABLE:
                continue
            for t, ctype in enumerate((CRC32C, CRC32)):
                parity_lost = (x + t) % 2 == 1
                cases.append(_ver(k, e + 2 if parity_lost else e, e, ctype, parity_lost))
            x += 1
    return cases


SPECIALISED_SHAPES = tuple((k, e) for k in FUSED_K for e in range(1, RS[k] + 1))


def specialised_cases():
    cases = []
    for x, (k, e) in enumerate(SPECIALISED_SHAPES):
        for t, ctype in enumerate((CRC32C, CRC32)):
            cases.append(_ver(k, RS[k], e, ctype, (x + t) % 2 == 1 and e + 1 <= RS[k]))
    return cases


def available(case):
    k = case.k
    return [i for i in range(k + case.m) if (i not in case.lost_data if i < k else i - k not in case.lost_parity)]


def spares(case):
    return len(available(case)) - case.k


def verify_flips(case, cell, stripes=VERIFY_STRIPES):
    """[(stripe, unit, byte)] of the batch's bent bytes (module docstring); a
    batch of 6 stripes has no stripe with one failure too many."""
    av, k = available(case), case.k
    flips = [(4, av[0], 3), (5, av[k - 1], cell - 1)]
    if spares(case) and stripes > 6:
        flips += [(6, av[t], 100 + t) for t in range(spares(case) + 1)]
    return flips


class VerifyTruth:
    """The batch of one verify case at one cell and what the call must leave.
      units  [S, k + m, cell]  data and parity as read: bent, the lost units' slots `garbage`
      sums   [S, k + m, nck, 4]  the true units' chunk sums (the lost units' words `garbage`)
      out    {(stripe, unit): cell}  every data cell the call must write
      free   [(stripe, unit)]  cells it may leave in any state (lost units of a stripe that cannot be rebuilt)
      bad    [S, k + m], flags_checked [S], raises"""

    def __init__(self, case, cell, seed, stripes=VERIFY_STRIPES, flips=None, garbage=0xEE):
        k, m, n = case.k, case.m, case.k + case.m
        self.case, self.cell, self.S = case, cell, stripes
        data = batch_data(k, stripes, cell, seed)
        true = np.concatenate([data, encode_ref(k, m, data)], axis=1)
        self.sums = chunk_sums(true, case.ctype)
        self.units = true.copy()
        self.flips = verify_flips(case, cell, stripes) if flips is None else flips
        for s, u, b in self.flips:
            self.units[s, u, b] ^= FLIP
        lost = list(case.lost_data) + [k + j for j in case.lost_parity]
        self.units[:, lost] = garbage
        self.sums[:, lost] = garbage
        self.out, self.free = {}, []
        self.bad = np.zeros((stripes, n), dtype=np.uint8)
        self.flags_checked = np.ones(stripes, dtype=bool)
        self.raises = False
        bent = {s for s, _, _ in self.flips}
        for s in range(stripes):
            if s not in bent:
                continue
            cells = [None if i in lost else self.units[s, i] for i in range(n)]
            got, self.bad[s] = verified_read_row(k, m, cells, self.sums[s], case.ctype)
            if got is None:
                self.raises = True
                self.free += [(s, i) for i in case.lost_data]
                self.flags_checked[s] = spares(case) == 0
            else:
                for i in range(k):
                    if i in case.lost_data or self.bad[s, i]:
                        self.out[(s, i)] = got[i]
        rest = [s for s in range(stripes) if s not in bent]
        if rest:  # the clean stripes in one batched decode
            present = sum(1 << i for i in range(n) if i not in lost)
            clean = decode_ref(k, m, true[rest, :k], true[rest, k:], present)
            for x, s in enumerate(rest):
                for j, i in enumerate(case.lost_data):
                    self.out[(s, i)] = clean[x, j]


# ---- part 2: waves that must take several tiles -----------------------------------------

QUEUE_KERNELS = (("encode", 3, 2, 0, 8192), ("encode", 10, 4, 0, 4096),
                 ("verify", 2, 1, 1, 4096), ("verify", 6, 3, 3, 4096))  # (call, k, m, e, wave-tile bytes)
LAST_TILE = 1024 + 528          # a cell's last wave-tile: one full slab, one of 528 bytes, the rest dead


def queue_waves(cus):
    """Waves of a work-queue launch of the fused kernels: 2 blocks of 4 per CU."""
    return 8 * cus


def queue_tile_counts(cus):
    """[(name, T)]: 1, 7, 8, 9 (n = min(grid, 8) counters on both sides), 2 CUs
    -+ 1 (the grid clamp) and 3 W + 5 (some wave takes four tiles)."""
    return [("1", 1), ("7", 7), ("8", 8), ("9", 9), ("2cus-1", 2 * cus - 1), ("2cus+1", 2 * cus + 1),
            ("3w+5", 3 * queue_waves(cus) + 5)]


QUEUE_T = tuple(name for name, _ in queue_tile_counts(1))


def queue_shape(T, wave_tile):
    """(stripes, cell) with stripes * ceil(cell / wave_tile) == T exactly.  The
    issue's cell is 5 wave-tiles + 1 KiB + 528 B, 6 tiles a stripe; most of its
    counts are no multiple of 6, so a stripe takes the divisor d of T in 1..13
    nearest 6 (the smaller of two equally near) and its cell d - 1 wave-tiles +
    1 KiB + 528 B: T = 3 W + 5 = 6149 at 256 CUs gives 559 stripes of 11."""
    d = min((d for d in range(1, 14) if T % d == 0), key=lambda d: (abs(d - 6), d))
    return T // d, (d - 1) * wave_tile + LAST_TILE


def fused_tiles(stripes, cell, tile_bytes):
    return stripes * -(-cell // tile_bytes)


def late_flip(case, stripes, cell):
    """One bent byte in the last tile of the last stripe: the last stripe is in
    the last tile-order group (or its remainder), behind every whole group, so
    with more than 32 stripes the tile lies in the last quarter of the order."""
    return [(stripes - 1, available(case)[case.k - 1], cell - 1)]


BLOCK_GRIDS = (1, 5)            # tune key 7 on the measurement build
BLOCK_CELL, BLOCK_STRIPES = CELLS[1], 6
BLOCK_ENCODE = ((6, 3), (2, 1), (6, 4))
BLOCK_VERIFY = ((6, 3, 2), (10, 4, 4))  # (k, m, e): the generic kernel


def block_lost(k, e, grid):
    """A plan of its own for every (shape, grid), none of them lost_units(k, e):
    a plan's first call queues its compile and runs the generic kernel."""
    first = 1 + BLOCK_GRIDS.index(grid)
    lost = tuple(sorted((first + 2 * j) % k for j in range(e)))
    assert len(set(lost)) == e and lost != lost_units(k, e)
    return lost


# ---- part 3: one stream, both counter sets, a graph -------------------------------------

SEQUENCE_KM = ((3, 2), (10, 4))


def sequence_tiles(cus, graph=False):
    """Tile counts of the four launches of a round: fused large, fused 1, plain
    (sized like the 9), fused 9.  In a graph the large one is 2 CUs + 1."""
    return (2 * cus + 1 if graph else 3 * queue_waves(cus) + 5, 1, 9, 9)
