// host_gf.hpp -- the engine's host-side GF(2^8) stripe multiply, for rows
// too small to pay a PCIe round trip (the per-call drop-in's small-row path,
// hec_encode / hec_decode below the coder's host limit; hec_gf_matmul_host).
//
//   out[j][b] = XOR_i M[j][i] * in[i][b]    (GF(2^8), modulus 0x11D)
//
// Same map as the device kernels and the reference's hot loop
// (rust/src/ec/matrix.rs:204-231), restated for the CPU's byte-vector units:
//   * AVX-512BW + GFNI: multiplication by a constant c is GF(2)-linear on a
//     byte, so one vgf2p8affineqb applies c's 8x8 bit matrix to 64 bytes
//     (the instruction's own field is irrelevant: the matrix encodes 0x11D);
//     3-input XORs (vpternlogq) accumulate; masked loads/stores take any
//     length and alignment.
//   * AVX2: split-nibble product tables, two vpshufb per 32 bytes.
//   * scalar: log/antilog tables.
// The ISA is picked once at run time (CPUID).  No device, no allocation, no
// lock: thread-safe.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace hec {
namespace host {

enum Isa { kScalar = 0, kAvx2 = 1, kAvx512Gfni = 2 };

// The best ISA this CPU supports.
Isa best_isa();
const char* isa_name(Isa isa);

// The 8x8 GF(2) matrix of y = c * x as a vgf2p8affineqb qword (byte 7 - i =
// the input-bit mask of output bit i).
uint64_t affine_matrix(uint8_t c);

// affine_matrix of every entry of a rows x cols matrix (row-major), so that
// hot callers (a coder's encode matrix, a cached decode plan) build it once.
std::vector<uint64_t> affine_matrices(const uint8_t* mat, size_t n_entries);

// out[j] = sum_i mat[j*cols + i] * in[i] (n bytes each) with the given ISA
// (kAvx512Gfni / kAvx2 fall back to what the CPU supports).  rows, cols >= 1;
// aff = affine_matrices(mat) or null (then built per call).
void gf_matmul(Isa isa, const uint8_t* mat, const uint64_t* aff, size_t rows, size_t cols, const uint8_t* const* in,
               uint8_t* const* out, size_t n);

inline void gf_matmul(const uint8_t* mat, const uint64_t* aff, size_t rows, size_t cols, const uint8_t* const* in,
                      uint8_t* const* out, size_t n) {
    gf_matmul(best_isa(), mat, aff, rows, cols, in, out, n);
}

// The same with rows of at least split_min_bytes() (256 KiB) per shard cut
// into column ranges coded by a small process-wide worker pool plus the
// calling thread ($HEC_HOST_THREADS threads in all, default 4; 1 = never
// split).  A row that long is bound by one core's memory bandwidth, not its
// GFNI units; the pieces are 4 KiB aligned.  If another call holds the pool,
// the row is coded on the calling thread.  cols <= 64.
void gf_matmul_split(Isa isa, const uint8_t* mat, const uint64_t* aff, size_t rows, size_t cols,
                     const uint8_t* const* in, uint8_t* const* out, size_t n);
size_t split_min_bytes();

inline void gf_matmul_split(const uint8_t* mat, const uint64_t* aff, size_t rows, size_t cols,
                            const uint8_t* const* in, uint8_t* const* out, size_t n) {
    gf_matmul_split(best_isa(), mat, aff, rows, cols, in, out, n);
}

// Stripe scrub on the host (hec_scrub): with P the m x k parity block
// (row-major) and H = [P | I_m], the syndromes s_j(b) = sum_i P[j][i] *
// units[i][b] ^ units[k+j][b] of every byte position b < n.  *bad_bytes =
// positions with a non-zero syndrome vector; *ruled_out bit t (t < k+m) set
// when some position's vector is not a GF(2^8) multiple of column t of H (some
// 2x2 minor s_i * H[j][t] ^ s_j * H[i][t] is non-zero).  The syndromes are
// computed by gf_matmul in blocks of scrub_block_bytes() per unit into a
// scratch of m such blocks (the only allocation: nothing grows with n); the
// locate runs over the non-zero positions only.  k + m <= 64, aff as gf_matmul.
void scrub(Isa isa, const uint8_t* P, const uint64_t* aff, size_t k, size_t m, const uint8_t* const* units, size_t n,
           uint64_t* ruled_out, uint64_t* bad_bytes);
size_t scrub_block_bytes();

// Scrub correction on the host (hec_scrub_correct): scrub() as above, then the
// verdict of hec_scrub_verdict over k + m units.  Returns -1 for a clean
// stripe and -2 for one that is not LOCATED (nothing written); for a LOCATED
// unit t, returns t after units[t][b] ^= scale * s_row(b) for every b < n,
// with row the first j with P[j][t] != 0 and scale = 1 / P[j][t] for a data
// unit, row = t - k and scale = 1 for a parity unit.  The one syndrome row is
// computed by gf_matmul in blocks of scrub_block_bytes() into a scratch of
// two such blocks: nothing grows with n.  *ruled_out / *bad_bytes receive the
// pair scrub() found (before the correction).
int scrub_correct(Isa isa, const uint8_t* P, const uint64_t* aff, size_t k, size_t m, uint8_t* const* units, size_t n,
                  uint64_t* ruled_out, uint64_t* bad_bytes);

}  // namespace host
}  // namespace hec
