// crc_compose.hpp -- composite CRCs: the CRC of a concatenation from the CRCs
// of its parts (Hadoop's COMPOSITE_CRC / CrcComposer), for the two chunk
// checksums of checksum_tables.hpp.
//
// With I = init, X = xorout and L_n(r) = r * x^(8n) mod P (the register after
// n zero bytes, in the CRC's own bit order):
//     crc(A || B) = L_|B|(crc(A) ^ X ^ I) ^ crc(B)
// In t = crc ^ X ^ I this is linear, t(A || B) = L_|B|(t(A)) ^ t(B), and
// t(empty) = 0 for both kinds, so the t of any sequence of parts is
//     XOR_i  x^(8 * bytes after part i) * t_i
// Everything below works on t and turns it back into a CRC at the end.
//
// Host part (no HIP): multiply mod P in either bit order, x^(8n) for 64-bit n
// by square-and-multiply, the concat step, the stripe geometry of a sums
// array and the host fold hec_composite_crc runs.  The multiply and the byte
// swap are also the device's (crc_compose.hip), which only ever multiplies by
// constants the host raised.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "checksum_tables.hpp"

#if defined(__HIPCC__)
#define HEC_CC_HD __host__ __device__
#else
#define HEC_CC_HD
#endif

namespace hec {
namespace crc {

constexpr size_t kComposeMaxUnits = 64;

// crc ^ kAffine<KIND> = t
template <int KIND>
constexpr uint32_t kAffine = Spec<KIND>::kInit ^ Spec<KIND>::kXorout;

// The polynomial 1.  Reflected: bit 31 is x^0 and bit 0 is x^31; MSB-first:
// bit i is x^i.
template <bool R>
HEC_CC_HD constexpr uint32_t poly_one() {
    return R ? 0x80000000u : 1u;
}

// b * x mod P
template <int KIND>
HEC_CC_HD constexpr uint32_t xtime(uint32_t b) {
    return Spec<KIND>::kReflected ? (b >> 1) ^ (Spec<KIND>::kPoly & (0u - (b & 1u)))
                                  : (b << 1) ^ (Spec<KIND>::kPoly & (0u - (b >> 31)));
}

// all ones when a has the term x^i
template <bool R>
HEC_CC_HD constexpr uint32_t term_mask(uint32_t a, int i) {
    return 0u - ((R ? a >> (31 - i) : a >> i) & 1u);
}

// a * b mod P, carry-less: 32 conditional XORs of b * x^i
template <int KIND>
HEC_CC_HD constexpr uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & term_mask<Spec<KIND>::kReflected>(a, i);
        b = xtime<KIND>(b);
    }
    return p;
}

// x^(8n) mod P = (x^8)^n
template <int KIND>
constexpr uint32_t xpow8(uint64_t n) {
    uint32_t r = poly_one<Spec<KIND>::kReflected>();
    uint32_t sq = Spec<KIND>::kReflected ? 0x00800000u : 0x00000100u;  // x^8
    for (; n; n >>= 1) {
        if (n & 1) r = mulmod<KIND>(r, sq);
        sq = mulmod<KIND>(sq, sq);
    }
    return r;
}

// crc(A || B) from crc(A), crc(B) and |B|
template <int KIND>
constexpr uint32_t concat(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return mulmod<KIND>(crc_a ^ kAffine<KIND>, xpow8<KIND>(len_b)) ^ crc_b;
}

HEC_CC_HD inline uint32_t bswap32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, v, 0x00010203u);  // one v_perm_b32
#else
    return __builtin_bswap32(v);
#endif
}

// ---- host only from here ---------------------------------------------------

// Multiplication by one constant as four byte tables (the host fold's per-chunk step).
template <int KIND>
struct ByteMul {
    uint32_t t[4][256];
    explicit ByteMul(uint32_t c) {
        uint32_t col[32];  // col[j] = c * (the polynomial with only bit j set)
        for (int j = 0; j < 32; j++) col[j] = mulmod<KIND>(1u << j, c);
        for (int b = 0; b < 4; b++)
            for (int x = 0; x < 256; x++) {
                uint32_t v = 0;
                for (int j = 0; j < 8; j++)
                    if (x & (1 << j)) v ^= col[8 * b + j];
                t[b][x] = v;
            }
    }
    uint32_t operator()(uint32_t a) const {
        return t[0][a & 0xFF] ^ t[1][(a >> 8) & 0xFF] ^ t[2][(a >> 16) & 0xFF] ^ t[3][a >> 24];
    }
};

// The sums array [stripes][n][nck] of a block group and the length of every
// cell: cell_len except in the last stripe, where data unit u holds
// min(C, max(0, r - u C)) of the stripe's r logical bytes and every parity
// unit is as long as the first cell (CellBuffer::encode sizes parity so).
struct Geometry {
    uint64_t n = 0, k = 0, cell_len = 0, stripes = 0, bpc = 0;
    uint64_t nck = 0;       // ceil(cell_len / bpc): chunk slots per cell
    uint64_t last_len = 0;  // r: logical bytes of the last stripe
    uint64_t len_last[kComposeMaxUnits] = {};
};

// False for sizes outside the call's contract.  stripes == 0 is in range
// (with data_len == 0) and describes no cell.
inline bool make_geometry(size_t n_units, size_t data_units, size_t cell_len, size_t stripes,
                          size_t bytes_per_checksum, uint64_t data_len, Geometry* g) {
    if (n_units < 1 || n_units > kComposeMaxUnits || data_units < 1 || data_units > n_units || cell_len == 0 ||
        bytes_per_checksum == 0)
        return false;
    const unsigned __int128 row = static_cast<unsigned __int128>(data_units) * cell_len;
    const unsigned __int128 full = row * stripes;
    if (full >> 64) return false;
    if (data_len != 0 && (stripes == 0 || data_len > uint64_t(full) || data_len <= uint64_t(full - row))) return false;
    g->n = n_units;
    g->k = data_units;
    g->cell_len = cell_len;
    g->stripes = stripes;
    g->bpc = bytes_per_checksum;
    g->nck = cell_len / bytes_per_checksum + (cell_len % bytes_per_checksum != 0);
    g->last_len = stripes == 0 ? 0 : data_len == 0 ? uint64_t(row) : data_len - uint64_t(full - row);
    for (size_t u = 0; u < n_units; u++) {
        const uint64_t before = u < data_units ? uint64_t(u) * cell_len : 0;
        const uint64_t left = g->last_len > before ? g->last_len - before : 0;
        g->len_last[u] = left < cell_len ? left : cell_len;
    }
    return true;
}

inline uint32_t load_be32(const uint8_t* p) {
    return uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | uint32_t(p[3]);
}
inline void store_be32(uint8_t* p, uint32_t v) {
    p[0] = uint8_t(v >> 24);
    p[1] = uint8_t(v >> 16);
    p[2] = uint8_t(v >> 8);
    p[3] = uint8_t(v);
}

// The host fold: one pass over the chunk sums in file order, each output
// optional.  Reads only the slots below ceil(len / bpc) of each cell.
template <int KIND>
void composite_host(const Geometry& g, const uint8_t* sums, uint8_t* cell_crcs, uint8_t* unit_crcs,
                    uint8_t* group_crc) {
    constexpr uint32_t A = kAffine<KIND>;
    const ByteMul<KIND> by_chunk(xpow8<KIND>(g.bpc));
    const uint32_t by_cell = xpow8<KIND>(g.cell_len);
    uint32_t unit_t[kComposeMaxUnits] = {};
    uint32_t group_t = 0;
    for (uint64_t s = 0; s < g.stripes; s++)
        for (uint64_t u = 0; u < g.n; u++) {
            const uint64_t len = s + 1 < g.stripes ? g.cell_len : g.len_last[u];
            const uint64_t nc = len / g.bpc + (len % g.bpc != 0);
            const uint8_t* p = sums + (s * g.n + u) * g.nck * 4;
            uint32_t t = 0;
            for (uint64_t c = 0; c + 1 < nc; c++) t = by_chunk(t) ^ load_be32(p + 4 * c) ^ A;
            if (nc) t = mulmod<KIND>(t, xpow8<KIND>(len - (nc - 1) * g.bpc)) ^ load_be32(p + 4 * (nc - 1)) ^ A;
            if (cell_crcs) store_be32(cell_crcs + (s * g.n + u) * 4, t ^ A);
            const uint32_t by_len = len == g.cell_len ? by_cell : xpow8<KIND>(len);
            unit_t[u] = mulmod<KIND>(unit_t[u], by_len) ^ t;
            if (u < g.k) group_t = mulmod<KIND>(group_t, by_len) ^ t;
        }
    if (unit_crcs)
        for (uint64_t u = 0; u < g.n; u++) store_be32(unit_crcs + 4 * u, unit_t[u] ^ A);
    if (group_crc) store_be32(group_crc, group_t ^ A);
}

// Bytes of device workspace the unit and group folds need: the cells' t
// ([stripes][n] u32) and one partial per 1024 folded cells for each of the n
// unit folds and the group fold.
constexpr uint64_t kComposeBlockItems = 1024;
inline uint64_t compose_partials_per_fold(uint64_t n_units, uint64_t stripes) {
    return stripes < 2 ? 0 : ((stripes - 1) * n_units + kComposeBlockItems - 1) / kComposeBlockItems;
}
inline uint64_t compose_workspace_bytes(uint64_t n_units, uint64_t stripes) {
    return 4 * (stripes * n_units + (n_units + 1) * compose_partials_per_fold(n_units, stripes));
}

}  // namespace crc
}  // namespace hec

// ---- the device launcher (crc_compose.hip) ---------------------------------

struct ihipStream_t;  // hipStream_t, without the HIP headers

namespace hec {

// Kernel arguments: the geometry and every constant the kernels multiply by,
// raised on the host.  "levels" are c^(2^l), l = 0 .. 6.
struct ComposeArgs {
    const uint32_t* sums;  // [stripes][n][nck] big-endian
    uint32_t* cell_out;    // [stripes][n] big-endian, or null
    uint32_t* unit_out;    // [n] big-endian, or null
    uint32_t* group_out;   // [1] big-endian, or null
    uint32_t* ws_cells;    // workspace: t of every cell, [stripes][n]; null when only cell_out is asked for
    uint32_t* ws_part;     // workspace: [n + 1][part_stride] partial folds
    uint64_t stripes, nck;
    uint32_t n, k;
    uint32_t part_stride;
    uint32_t log_w;         // lanes per cell = 1 << log_w
    uint32_t lvl_chunk[7];  // levels of x^(8 bpc)
    uint32_t lvl_cell[7];   // levels of x^(8 cell_len)
    uint32_t lvl_part[7];   // levels of x^(8 cell_len kComposeBlockItems)
    uint32_t tail_full;     // x^(8 * length of a full cell's last chunk)
    uint32_t last_stripe;   // x^(8 r)
    // the last stripe's cells, per unit
    uint64_t last_nc[crc::kComposeMaxUnits];     // chunks
    uint32_t last_tail[crc::kComposeMaxUnits];   // x^(8 * length of the last chunk)
    uint32_t last_unit[crc::kComposeMaxUnits];   // x^(8 len)
    uint32_t last_group[crc::kComposeMaxUnits];  // x^(8 * data bytes of the stripe after the unit)
};

// Queues the kernels on `stream`; d_workspace must hold
// crc::compose_workspace_bytes(g.n, g.stripes) when a unit or group CRC is
// asked for.  0 ok, -1 invalid sizes, >0 hipError_t.
int launch_composite_crc(int kind, const crc::Geometry& g, const uint8_t* d_sums, uint8_t* d_cell_crcs,
                         uint8_t* d_unit_crcs, uint8_t* d_group_crc, void* d_workspace, int device,
                         ihipStream_t* stream);

}  // namespace hec
