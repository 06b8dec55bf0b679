// ec_reconstruct_rows.hpp -- argument blocks and launchers of the verified
// reconstruction of short stripes (see ec_reconstruct_rows.hip): stripes that
// hold r < k * cell_len logical bytes, every unit at its own length.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#include "ec_reconstruct_crc.hpp"

namespace hec {

// The logical bytes of the launch's stripes.  A stripe of r bytes, 1 <= r <=
// k * cell_len, has n0 = min(cell_len, r); data unit u < k holds
// min(cell_len, max(0, r - u * cell_len)) bytes and every parity unit n0
// (crc::make_geometry's len_last[]).
struct ReconRowsLens {
    const uint64_t* stripe_bytes;  // launch stripe s holds stripe_bytes[s] bytes; null: every stripe holds `bytes`
    uint64_t bytes;
    uint64_t stripe0;              // without a stripe list, launch stripe s is batch stripe stripe0 + s
};

// gf_crc_rows<RowsRepair>: launch_reconstruct_crc for short stripes.  The
// survivors count as zero from their length on and are verified over their
// own bytes; a target gets its computed bytes, zeros up to n0, and the sums
// of its own bytes; nothing at or past n0 is written.  a.in / a.out /
// c.shard_id as launch_reconstruct_crc, a.k = the code's k (units below it
// are data units); same shapes (k in {2,3,6,10}, a.r <= kMaxR, 512-B chunks,
// 16-B aligned bases, strides and cell_len), any lengths.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_reconstruct_crc_rows(const MatmulArgs& a, const ReconCrcArgs& c, const ReconRowsLens& lens, int device,
                                hipStream_t stream);

// Argument block of gf_reconstruct_rows_bytes: any k <= kMaxK, r <= kMaxR
// rows, any chunk size, cell_len and alignment.
struct ReconRowsBytesArgs {
    const uint8_t* in[kMaxK];     // the plan's k survivors
    uint64_t in_stride[kMaxK];
    uint8_t* out[kMaxR];          // the r targets
    uint64_t out_stride[kMaxR];
    uint8_t coef[kMaxR * kMaxK];  // row j, column i at [j*kMaxK + i]
    uint8_t out_id[kMaxR];        // unit index of target j
    uint8_t in_id[kMaxK];         // ... of survivor i
    int32_t k;
    int32_t r;
    uint32_t data_units;          // units below it are data units
    uint32_t n_total;
    uint8_t* sums;                // [stripe][n_total][nck] big-endian u32
    const uint8_t* expected;      // null: no verification; may be `sums`
    uint8_t* bad;
    int32_t kind;                 // crc::Kind
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s]; null: lens.stripe0 + s
    uint64_t stripes;             // stripes of the launch
    ReconRowsLens lens;
    uint64_t cell_len;
    uint64_t bytes_per_checksum;
    uint64_t nck;                 // filled by the launcher: ceil(cell_len / bytes_per_checksum)
};

// One work item per (stripe, target row, chunk below n0): the row's bytes
// formed from the survivors, stored (zeros from the target's length on) and
// stepped through the CRC, the sum stored where the chunk has a byte of the
// target.  With a.expected, one more per (stripe, survivor, chunk of its own
// bytes).  0 ok, -1 invalid sizes (nothing was launched), >0 hipError_t.
int launch_reconstruct_rows_bytes(const ReconRowsBytesArgs& a, int device, hipStream_t stream);

}  // namespace hec
