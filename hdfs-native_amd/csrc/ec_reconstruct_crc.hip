// ec_reconstruct_crc.hip -- reconstruction fused with the chunk checksums on
// both sides of it, for the repair worker: the k survivors of a stripe arrive
// with one CRC per 512-B chunk and are verified while the lost units are
// rebuilt from the same registers (HDFS-15759: a silently bad survivor
// poisons every rebuilt unit), and the rebuilt units leave with fresh chunk
// sums (WritePacket::calculate_checksum, connection.rs:568-584) computed from
// the registers that were just stored.  One pass of k reads + t writes where
// verify + reconstruct + checksum make 2k reads + t writes + t reads.
//
// gf_reconstruct_crc (ec_reconstruct_crc_kernel.hpp; this file instantiates
// it with STORE_OUT = true) has the shape of gf_fused_crc's plain path
// (ec_fused_kernel.hpp): one input at a time with the next one prefetched,
// 256-thread blocks, two per CU; the checksum rounds are crc_stage.hpp's.
// Particular to it is what is checksummed: the inputs only when VERIFY_IN (compared against
// the expected sums), the outputs always (their sums stored), both addressed
// by unit index in the engine's [stripe][k+m] layouts, and an optional stripe
// list, so a mixed batch takes one launch per distinct pattern.  Block tiles
// in the fixed order: no counters, nothing to zero, capturable as is.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_reconstruct_crc_kernel.hpp"
#include "launch_parts.hpp"

namespace hec {

namespace {

struct ReconCrcFn {
    template <int K, int R>
    static const void* fn(int kind, bool verify_in) {
        constexpr int SL = recon_crc_slabs(K, R);
        if (kind == crc::kCrc32c)
            return verify_in ? reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCrc32c, true>)
                             : reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCrc32c, false>);
        return verify_in ? reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCksum, true>)
                         : reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCksum, false>);
    }
};

}  // namespace

int launch_reconstruct_crc(const MatmulArgs& in, const ReconCrcArgs& cs, int device, hipStream_t stream) {
    MatmulArgs a = in;
    if (cs.kind != crc::kCrc32c && cs.kind != crc::kCksum) return -1;
    if (a.r < 1 || a.r > kMaxR || a.cell_len % 16 != 0 || !cs.sums || (cs.expected && !cs.bad)) return -1;
    if ((reinterpret_cast<uintptr_t>(cs.sums) | reinterpret_cast<uintptr_t>(cs.expected)) & 3u) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || ((reinterpret_cast<uintptr_t>(a.in[i]) | a.in_stride[i]) & 15u)) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || ((reinterpret_cast<uintptr_t>(a.out[j]) | a.out_stride[j]) & 15u)) return -1;
    const bool verify_in = cs.expected != nullptr;
    const void* fn = pick_kr<ReconCrcFn>(a.k, a.r, cs.kind, verify_in);
    if (!fn) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * recon_crc_slabs(a.k, a.r))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    // groups of 8 stripes and 32 blocks per CU (2 resident), as launch_fused's
    // block-tile case
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * 32;
    if (grid > total) grid = total;
    ReconCrcArgs c = cs;
    void* args[] = {&a, &c};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
