// ec_read_rows.hpp -- argument blocks and launchers of the verified striped
// read into a file-order buffer (see ec_read_rows.hip): the survivors of every
// stripe verified over their own bytes, the lost data units rebuilt, and all k
// data units written at file + stripe * file_stride + u * cell_len, each for
// its own length (ReconRowsLens, ec_reconstruct_rows.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#include "ec_reconstruct_rows.hpp"

namespace hec {

// Checksum and file side of gf_read_rows.  The coding side is a MatmulArgs:
// in[] = the plan's k survivors, coef = the lost data units' rows over them,
// a.k = the code's k, a.r = the lost data units (0 .. kMaxR); a.out is unused.
struct ReadRowsCrcArgs {
    const uint8_t* expected;      // VERIFY_IN: the survivors' sums, [stripe][n_total][nck] big-endian u32
    uint8_t* bad;                 // VERIFY_IN: bad[stripe * n_total + unit] = 1 on a mismatch
    uint8_t* file;                // data unit u of batch stripe s at file + s * file_stride + u * cell_len
    uint64_t file_stride;
    uint32_t n_total;             // units per stripe in the sums / flags layouts (k + m)
    int32_t kind;                 // crc::Kind
    uint8_t shard_id[64];         // unit index of input i (0 .. K-1) and of lost data unit j (at K + j)
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s]; null: lens.stripe0 + s
};

// gf_read_rows: one pass of k reads + k writes.  With c.expected every
// survivor is verified over its own bytes; a survivor that is a data unit is
// stored to its file slot from the registers it was loaded into, a lost data
// unit is rebuilt and stored, each over [0, len(u)) and no further.  Shapes as
// launch_reconstruct_crc_rows (k in {2,3,6,10}, 512-B chunks, 16-B aligned
// bases, strides and cell_len) with a.r = 0 allowed and file, file_stride
// 16-B aligned; any lengths.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_read_crc_rows(const MatmulArgs& a, const ReadRowsCrcArgs& c, const ReconRowsLens& lens, int device,
                         hipStream_t stream);

constexpr uint8_t kReadRowsLost = 0x80;  // role: | row of coef
constexpr uint8_t kReadRowsSkip = 0xFF;  // role: not this launch's

// Argument block of gf_read_rows_bytes: any k <= kMaxK, r <= kMaxR lost data
// units per launch, any chunk size, cell_len, file_stride and alignment.
struct ReadRowsBytesArgs {
    const uint8_t* in[kMaxK];     // the plan's k survivors, ascending: data units first
    uint64_t in_stride[kMaxK];
    uint8_t coef[kMaxR * kMaxK];  // row j, column i at [j*kMaxK + i]
    uint8_t in_id[kMaxK];         // unit index of survivor i
    uint8_t role[kMaxK];          // of data unit u: its survivor slot (verify and copy), kReadRowsLost | row
                                  // (rebuild and store), or kReadRowsSkip
    int32_t k;                    // the code's k
    int32_t r;                    // rows of coef in use
    int32_t parity_in;            // the last parity_in survivors are parity units, verified by lanes of their own
    uint32_t n_total;
    uint8_t* file;
    uint64_t file_stride;
    const uint8_t* expected;      // null: no verification
    uint8_t* bad;
    int32_t kind;                 // crc::Kind
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s]; null: lens.stripe0 + s
    uint64_t stripes;             // stripes of the launch
    ReconRowsLens lens;
    uint64_t cell_len;
    uint64_t bytes_per_checksum;
    uint64_t nck;                 // filled by the launcher: ceil(cell_len / bytes_per_checksum)
};

// One work item per (stripe, data unit, chunk of its own bytes): a survivor's
// bytes verified (with a.expected) and copied, a lost unit's formed from the
// survivors and stored; a.parity_in more per stripe and chunk below n0 verify
// the parity survivors.  0 ok, -1 invalid sizes (nothing was launched), >0
// hipError_t.
int launch_read_rows_bytes(const ReadRowsBytesArgs& a, int device, hipStream_t stream);

}  // namespace hec
