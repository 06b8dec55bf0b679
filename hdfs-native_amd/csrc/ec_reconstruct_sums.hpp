// ec_reconstruct_sums.hpp -- launchers of the checksum-only reconstruction
// (see ec_reconstruct_sums.hip): the chunk sums of lost units from their
// survivors, with nothing rebuilt written to memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#include "ec_reconstruct_crc.hpp"

namespace hec {

// gf_reconstruct_crc without the output stores.  a.out / a.out_stride are not
// read; everything else as launch_reconstruct_crc (k in {2,3,6,10}, a.r <=
// kMaxR, 512-B chunks, 16-B aligned survivor bases, strides and cell_len).
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_reconstruct_sums(const MatmulArgs& a, const ReconCrcArgs& c, int device, hipStream_t stream);

// Argument block of gf_reconstruct_sums_bytes: any k <= kMaxK, r <= kMaxR
// rows, any chunk size and alignment, a length per unit.
struct ReconSumsArgs {
    const uint8_t* in[kMaxK];     // the plan's k survivors
    uint64_t in_stride[kMaxK];
    uint64_t in_len[kMaxK];       // bytes read of survivor i; it is zero from there on
    uint64_t out_len[kMaxR];      // bytes of target j: chunks c < ceil(out_len / bpc), the last one short
    uint8_t coef[kMaxR * kMaxK];  // row j, column i at [j*kMaxK + i]
    uint8_t out_id[kMaxR];        // unit index of target j in the sums and flags layouts
    uint8_t in_id[kMaxK];         // ... of survivor i (verify mode)
    int32_t k;
    int32_t r;
    uint8_t* sums;                // [stripe][n_total][nck] big-endian u32
    // verify mode (null: off): survivor i's chunks below ceil(in_len[i] / bpc),
    // the last one short, compared with these sums (same layout, may be
    // `sums`); bad[stripe * n_total + unit] = 1 on a mismatch
    const uint8_t* expected;
    uint8_t* bad;
    uint32_t n_total;
    int32_t kind;                 // crc::Kind
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s]; null: stripe0 + s
    uint64_t stripe0;
    uint64_t stripes;             // stripes of the launch
    uint64_t bytes_per_checksum;
    uint64_t nck;                 // chunk slots per cell in the sums layout
    uint64_t chunks;              // filled by the launcher: chunks of the longest unit it works on
};

// One work item per (stripe, target row, chunk): the row's bytes formed from
// the survivors and stepped through the CRC, the sum stored.  Verify mode adds
// one per (stripe, survivor, chunk).
// 0 ok, -1 invalid sizes (nothing was launched), >0 hipError_t.
int launch_reconstruct_sums_bytes(const ReconSumsArgs& a, int device, hipStream_t stream);

}  // namespace hec
