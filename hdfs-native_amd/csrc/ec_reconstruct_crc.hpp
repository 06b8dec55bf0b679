// ec_reconstruct_crc.hpp -- argument block and launcher of the fused
// reconstruction + chunk checksum kernel (see ec_reconstruct_crc.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"

namespace hec {

// Checksum side of gf_reconstruct_crc.  The coding side is a MatmulArgs: in[]
// = the plan's k survivors, out[] = the r target units, coef = the targets'
// rows over the survivors, stripes = stripes of this launch.
struct ReconCrcArgs {
    uint8_t* sums;                // written: the targets' chunk sums, [stripe][n_total][nck] big-endian u32
    const uint8_t* expected;      // VERIFY_IN: the survivors' sums, same layout (may be `sums`)
    uint8_t* bad;                 // VERIFY_IN: bad[stripe * n_total + unit] = 1 on a mismatch
    uint32_t n_total;             // units per stripe in the sums / flags layouts (k + m)
    int32_t kind;                 // crc::Kind
    uint8_t shard_id[64];         // unit index of input i (0 .. K-1) and of output j (at K + j)
    const uint32_t* stripe_list;  // launch stripe s is batch stripe stripe_list[s] (addresses, sums, flags); null = identity
};

// Rebuilds a.r <= kMaxR target units of every stripe of the launch from its k
// survivors, writes the targets' chunk sums and, with c.expected, verifies the
// survivors' -- one pass over the cells.  Needs k in {2,3,6,10}, 512-B
// checksum chunks, 16-B aligned bases, strides and cell_len, 4-B aligned
// sums.  Fixed tile order, no counters: capturable as is.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_reconstruct_crc(const MatmulArgs& a, const ReconCrcArgs& c, int device, hipStream_t stream);

}  // namespace hec
