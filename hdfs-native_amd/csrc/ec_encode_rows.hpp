// ec_encode_rows.hpp -- argument blocks and launchers of the encode with
// chunk sums of short stripes (see ec_encode_rows.hip): stripes that hold
// r < k * cell_len logical bytes, every unit at its own length
// (ReconRowsLens, ec_reconstruct_rows.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#include "ec_reconstruct_rows.hpp"

namespace hec {

// Checksum side of gf_crc_rows<RowsEncode>.  The coding side is a MatmulArgs: in[]
// = the k data units, out[] = the a.r parity units, coef = their rows of the
// encode matrix.
struct EncodeRowsCrcArgs {
    uint8_t* sums;     // written: [stripe][n_total][nck] big-endian u32; data unit i at i, parity j at k + j
    uint32_t n_total;  // units per stripe in the sums layout (k + m)
    int32_t kind;      // crc::Kind
};

// gf_crc_rows<RowsEncode>: the data units count as zero from their length on and
// none of their slot bytes at or past it influences an output; an empty data
// unit is not read.  Parity j gets its n0 computed bytes at [0, n0), nothing
// at or past n0 is written; every unit's sums are those of its own bytes,
// slots past its last live chunk are not written.  Shapes as
// launch_reconstruct_crc_rows (k in {2,3,6,10}, a.r <= kMaxR, 512-B chunks,
// 16-B aligned bases, strides and cell_len, cell_len < 2^31), any lengths.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_encode_crc_rows(const MatmulArgs& a, const EncodeRowsCrcArgs& c, const ReconRowsLens& lens, int device,
                           hipStream_t stream);

// Argument block of gf_encode_rows_bytes: any k <= kMaxK, r <= kMaxR parity
// rows, any chunk size, cell_len and alignment.
struct EncodeRowsBytesArgs {
    const uint8_t* in[kMaxK];     // the k data units
    uint64_t in_stride[kMaxK];
    uint8_t* out[kMaxR];          // the r parity units of this launch
    uint64_t out_stride[kMaxR];
    uint8_t coef[kMaxR * kMaxK];  // row j, column i at [j*kMaxK + i]
    uint8_t out_id[kMaxR];        // unit index of parity row j in the sums layout
    int32_t k;
    int32_t r;
    int32_t data_sums;            // != 0: the data units' sums too (the first launch of a stripe's rows)
    uint32_t n_total;
    uint8_t* sums;                // [stripe][n_total][nck] big-endian u32
    int32_t kind;                 // crc::Kind
    uint64_t stripes;             // stripes of the launch
    ReconRowsLens lens;
    uint64_t cell_len;
    uint64_t bytes_per_checksum;
    uint64_t nck;                 // filled by the launcher: ceil(cell_len / bytes_per_checksum)
};

// One work item per (stripe, parity row, chunk below n0): the row's bytes
// formed from the data units (each zero from its own length on), stored and
// stepped through the CRC, the sum stored.  With a.data_sums, one more per
// (stripe, data unit, chunk of its own bytes).
// 0 ok, -1 invalid sizes (nothing was launched), >0 hipError_t.
int launch_encode_rows_bytes(const EncodeRowsBytesArgs& a, int device, hipStream_t stream);

}  // namespace hec
