// ec_reconstruct_rows.hip -- verified reconstruction of short stripes: the
// last stripe of a block group, or every stripe of a batch of small files,
// holds r < k * cell_len logical bytes, so its units have different lengths
// (ec_reconstruct_rows.hpp).  The survivors arrive with chunk sums over their
// own bytes, the rebuilt units leave with sums over theirs, and the slots are
// what a reader hands out: the unit's bytes, zeros up to n0 = min(cell_len,
// r), nothing of the caller's behind.
//
// Two kernels, in a translation unit of their own so that the full-stripe
// kernels (ec_reconstruct_crc.hip, ec_reconstruct_sums.hip) keep their
// machine code.
//
// The register kernel is gf_crc_rows<RowsRepair<VERIFY_IN>> (ec_rows_kernel.hpp,
// with the rules of the short-stripe kernels): the survivors verified against
// their expected sums where there are some, a target cut to its own length.
//
// gf_reconstruct_rows_bytes is the byte-wise route for every other shape, in
// the style of gf_reconstruct_sums_bytes with the rebuilt bytes stored too.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_reconstruct_rows.hpp"
#include "ec_rows_kernel.hpp"

namespace hec {

// Byte-wise route: one lane per (stripe, row, chunk slot); the rows of a
// stripe are the r targets, then (verify mode) the k survivors.  Bytes from
// global memory, log/antilog products and a slice-by-1 CRC step from LDS, as
// gf_reconstruct_sums_bytes.  A target's lane works on its chunk's bytes
// below n0: the bytes below the target's length are formed from the survivors
// (each zero from its own length on), stored and summed, the rest stored as
// zero; the sum is stored when the chunk has a byte of the target.
template <int KIND>
__global__ __launch_bounds__(kBlock) void gf_reconstruct_rows_bytes(ReconRowsBytesArgs a) {
    using Spec = crc::Spec<KIND>;
    __shared__ uint32_t s_crc[256];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_lc[kMaxR * kMaxK];  // log of each coefficient
    __shared__ uint8_t s_nz[kMaxR * kMaxK];
    const int tid = threadIdx.x;
    rows_stage_byte_tables<KIND>(s_crc, s_exp, s_log);
    if (tid < kMaxR * kMaxK) {
        const uint8_t c = a.coef[tid];
        s_lc[tid] = kDevGf.log[c];
        s_nz[tid] = c != 0;
    }
    __syncthreads();
    const uint64_t bpc = a.bytes_per_checksum, cell_len = a.cell_len;
    const int rows = a.r + (a.expected ? a.k : 0);
    const uint64_t per_stripe = a.nck * uint64_t(rows);
    const uint64_t total = per_stripe * a.stripes;
    uint32_t* sums = reinterpret_cast<uint32_t*>(a.sums);
    for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += uint64_t(gridDim.x) * kBlock) {
        const uint64_t s = g / per_stripe;
        const uint64_t rest = g - s * per_stripe;
        const int j = int(rest / a.nck);
        const uint64_t chunk = rest - uint64_t(j) * a.nck;
        const uint64_t begin = chunk * bpc;
        const uint64_t r = rows_stripe_bytes(a.lens, s);
        const uint64_t n0 = r < cell_len ? r : cell_len;
        if (begin >= n0) continue;
        const uint64_t stripe = rows_batch_stripe(a.stripe_list, a.lens, s);
        if (j >= a.r) {  // a survivor's own bytes against its expected sums
            const int i = j - a.r;
            const uint64_t len = rows_unit_len(a.in_id[i], a.data_units, r, n0, cell_len);
            if (begin >= len) continue;
            const uint32_t sum = rows_own_chunk_sum<KIND>(s_crc, a.in[i] + stripe * a.in_stride[i], begin, len, bpc);
            const uint64_t cell = stripe * a.n_total + a.in_id[i];
            if (reinterpret_cast<const uint32_t*>(a.expected)[cell * a.nck + chunk] != sum) a.bad[cell] = 1;
            continue;
        }
        uint32_t crc = Spec::kInit;
        const uint64_t olen = rows_unit_len(a.out_id[j], a.data_units, r, n0, cell_len);
        const uint64_t end = n0 - begin < bpc ? n0 : begin + bpc;
        uint8_t* q = a.out[j] + stripe * a.out_stride[j];
        for (uint64_t b = begin; b < end; b++) {
            uint32_t acc = 0;
            if (b < olen) {
                for (int i = 0; i < a.k; i++) {
                    // survivor i has a byte b: a parity unit always (b < n0), a data unit below its cut
                    const uint32_t uid = a.in_id[i];
                    if (!s_nz[j * kMaxK + i] || (uid < a.data_units && uint64_t(uid) * cell_len + b >= r)) continue;
                    const uint8_t x = a.in[i][stripe * a.in_stride[i] + b];
                    if (x) acc ^= s_exp[uint32_t(s_log[x]) + s_lc[j * kMaxK + i]];
                }
                crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, acc);
            }
            q[b] = uint8_t(acc);
        }
        if (begin < olen)
            sums[(stripe * a.n_total + a.out_id[j]) * a.nck + chunk] = __builtin_bswap32(crc ^ Spec::kXorout);
    }
}

namespace {

struct ReconRowsFn {
    template <int K, int R>
    static const void* fn(int kind, bool verify_in) {
        constexpr int SL = rows_slabs(K, R);
        if (kind == crc::kCrc32c)
            return verify_in ? reinterpret_cast<const void*>(&gf_crc_rows<RowsRepair<true>, K, R, SL, crc::kCrc32c>)
                             : reinterpret_cast<const void*>(&gf_crc_rows<RowsRepair<false>, K, R, SL, crc::kCrc32c>);
        return verify_in ? reinterpret_cast<const void*>(&gf_crc_rows<RowsRepair<true>, K, R, SL, crc::kCksum>)
                         : reinterpret_cast<const void*>(&gf_crc_rows<RowsRepair<false>, K, R, SL, crc::kCksum>);
    }
};

}  // namespace

int launch_reconstruct_crc_rows(const MatmulArgs& a, const ReconCrcArgs& cs, const ReconRowsLens& lens, int device,
                                hipStream_t stream) {
    if (!cs.sums || (cs.expected && !cs.bad)) return -1;
    if ((reinterpret_cast<uintptr_t>(cs.sums) | reinterpret_cast<uintptr_t>(cs.expected)) & 3u) return -1;
    // grid as launch_reconstruct_crc
    return launch_rows_crc(pick_kr<ReconRowsFn>(a.k, a.r, cs.kind, cs.expected != nullptr), rows_slabs(a.k, a.r), a, cs,
                           lens, a.k, a.r, 32, device, stream);
}

int launch_reconstruct_rows_bytes(const ReconRowsBytesArgs& in, int device, hipStream_t stream) {
    ReconRowsBytesArgs a = in;
    if (a.k < 1 || a.k > kMaxK || a.r < 1 || a.r > kMaxR || !a.sums || (reinterpret_cast<uintptr_t>(a.sums) & 3u) ||
        !rows_bytes_args_ok(a, a.data_units))
        return -1;
    if (a.expected && (!a.bad || (reinterpret_cast<uintptr_t>(a.expected) & 3u))) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || a.out_id[j] >= a.n_total) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || a.in_id[i] >= a.n_total) return -1;
    a.nck = rows_nck(a.cell_len, a.bytes_per_checksum);
    const uint64_t total = a.nck * uint64_t(a.r + (a.expected ? a.k : 0)) * a.stripes;
    if (total == 0) return 0;
    return launch_rows_bytes(&gf_reconstruct_rows_bytes<crc::kCrc32c>, &gf_reconstruct_rows_bytes<crc::kCksum>, a, total,
                             0, device, stream);
}

}  // namespace hec
