// ec_scrub_crc.hpp -- argument block and launcher of the fused scrub + chunk
// checksum kernel (see ec_scrub_crc.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"

namespace hec {

// Checksum and result side of gf_scrub_crc.  The coding side is a MatmulArgs:
// in[0 .. k-1] = the plan's k survivors, in[k .. k+r-1] = its r extras, coef =
// the rows of G (extra j over the survivors), stripes = stripes of this launch.
struct ScrubCrcArgs {
    const uint8_t* expected;      // every read unit's sums, [stripe][n_total][nck] big-endian u32
    uint8_t* bad;                 // bad[stripe * n_total + unit] = 1 on a mismatch
    uint64_t* results;            // [stripe][2] (ruled_out, bad_bytes), 8-B aligned, zeroed in stream order
    uint64_t missing;             // bit t: unit t is missing (ORed into ruled_out of a dirty stripe)
    uint32_t n_total;             // units per stripe in the sums / flags layouts (k + m)
    int32_t kind;                 // crc::Kind
    uint8_t shard_id[64];         // unit index of survivor i (0 .. k-1) and of extra j (at k + j)
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s] (addresses, sums, flags,
                                  // results); null = identity
};

// Scrubs every stripe of the launch over its k survivors and a.r <= kMaxR
// extras and verifies the chunk sums of all k + r units -- one pass over the
// cells, nothing written but flags and the results of dirty stripes.  Needs k
// in {2,3,6,10}, 512-B checksum chunks, 16-B aligned bases, strides and
// cell_len, 4-B aligned sums, and a row 0 of G without a zero.  Fixed tile
// order, no counters: capturable as is.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_scrub_crc(const MatmulArgs& a, const ScrubCrcArgs& c, int device, hipStream_t stream);

}  // namespace hec
