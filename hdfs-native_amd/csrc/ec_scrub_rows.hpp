// ec_scrub_rows.hpp -- argument blocks and launchers of the verified scrub of
// short stripes (see ec_scrub_rows.hip): stripes that hold r < k * cell_len
// logical bytes, every unit checked and verified at its own length.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#include "ec_reconstruct_rows.hpp"
#include "ec_scrub_crc.hpp"

namespace hec {

// gf_scrub_crc_rows: launch_scrub_crc for short stripes.  Every unit counts as
// zero from its length on and is verified over its own bytes; only positions
// below n0 are checked or counted.  a / c as launch_scrub_crc, a.k = the code's
// k (units below it are data units), and every extra must be a parity unit
// (it holds n0 bytes: an ended unit's loads are sent there).  Same shapes (k in
// {2,3,6,10}, a.r <= kMaxR, 512-B chunks, 16-B aligned bases, strides and
// cell_len < 2^31, row 0 of G without a zero), any lengths.  Without a stripe
// list, launch stripe s is batch stripe lens.stripe0 + s.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_scrub_crc_rows(const MatmulArgs& a, const ScrubCrcArgs& c, const ReconRowsLens& lens, int device,
                          hipStream_t stream);

constexpr int kScrubRowsMaxE = 16;  // HEC_MAX_PARITY_UNITS

// Argument block of gf_scrub_rows_bytes: any k <= kMaxK, any e <= 16 (0: sums
// only), any chunk size, cell_len and alignment.
struct ScrubRowsBytesArgs {
    const uint8_t* in[kMaxShards];         // ns survivors, then e extras
    uint64_t in_stride[kMaxShards];
    uint8_t id[kMaxShards];                // unit index of each
    uint8_t coef[kScrubRowsMaxE * kMaxK];  // row j (extra j), survivor i at [j*kMaxK + i]
    int32_t ns;                            // survivors: k where e > 0, else the present units (<= k)
    int32_t e;
    uint32_t data_units;                   // units below it are data units
    uint32_t n_total;
    const uint8_t* expected;               // [stripe][n_total][nck] big-endian u32
    uint8_t* bad;
    uint64_t* results;                     // [stripe][2], zeroed in stream order
    uint64_t missing;                      // ORed into ruled_out of a dirty stripe
    int32_t kind;                          // crc::Kind
    const uint32_t* stripe_list;           // launch stripe s is batch stripe stripe_list[s]; null: lens.stripe0 + s
    uint64_t stripes;                      // stripes of the launch
    ReconRowsLens lens;
    uint64_t cell_len;
    uint64_t bytes_per_checksum;
    uint64_t nck;                          // filled by the launcher: ceil(cell_len / bytes_per_checksum)
};

// Per stripe: the syndromes of every position below n0 (units masked at their
// length) located as gf_scrub_mixed_bytes does, then one work item per
// (present unit, chunk of its own bytes) against the expected sums.
// 0 ok, -1 invalid sizes (nothing was launched), >0 hipError_t.
int launch_scrub_rows_bytes(const ScrubRowsBytesArgs& a, int device, hipStream_t stream);

}  // namespace hec
