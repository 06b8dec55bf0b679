// ec_encode_rows.hip -- encode with chunk sums of short stripes: the writer's
// side of ec_reconstruct_rows.hip and ec_scrub_rows.hip.  The last stripe of
// a block group, or every stripe of a batch of small files, holds r < k *
// cell_len logical bytes, so its data units have different lengths
// (ec_encode_rows.hpp).  The parity units leave with their n0 = min(cell_len,
// r) bytes and every unit with the chunk sums of its own bytes: the sums the
// rows repair, the rows scrub and the composite fold expect.
//
// Two kernels, in a translation unit of their own so that the full-stripe
// kernels (ec_fused.hip) keep their machine code.
//
// The register kernel is gf_crc_rows<RowsEncode> (ec_rows_kernel.hpp, with the
// rules of the short-stripe kernels): unit i < K is data unit i, unit K + j
// parity row j of the launch, and their sums go to cells i and K + j of the
// stripe.
//
// gf_encode_rows_bytes is the byte-wise route for every other shape, in the
// style of gf_reconstruct_rows_bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_encode_rows.hpp"
#include "ec_rows_kernel.hpp"

namespace hec {

// Byte-wise route: one lane per (stripe, row, chunk slot); the rows of a
// stripe are the r parity rows of the launch, then (a.data_sums) the k data
// units.  Bytes from global memory, log/antilog products and a slice-by-1 CRC
// step from LDS, as gf_reconstruct_rows_bytes.  A parity lane forms, stores
// and sums its chunk's bytes below n0, each data unit zero from its own length
// on; a data lane sums its unit's own bytes.
template <int KIND>
__global__ __launch_bounds__(kBlock) void gf_encode_rows_bytes(EncodeRowsBytesArgs a) {
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
    const int rows = a.r + (a.data_sums ? a.k : 0);
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
        const uint64_t stripe = a.lens.stripe0 + s;
        if (j >= a.r) {  // a data unit's own bytes
            const int i = j - a.r;
            const uint64_t len = rows_data_unit_len(uint32_t(i), r, cell_len);
            if (begin >= len) continue;
            sums[(stripe * a.n_total + uint32_t(i)) * a.nck + chunk] =
                rows_own_chunk_sum<KIND>(s_crc, a.in[i] + stripe * a.in_stride[i], begin, len, bpc);
            continue;
        }
        uint32_t crc = Spec::kInit;
        const uint64_t end = n0 - begin < bpc ? n0 : begin + bpc;
        uint8_t* q = a.out[j] + stripe * a.out_stride[j];
        for (uint64_t b = begin; b < end; b++) {
            uint32_t acc = 0;
            for (int i = 0; i < a.k; i++) {
                // data unit i has a byte b below its cut
                if (!s_nz[j * kMaxK + i] || uint64_t(i) * cell_len + b >= r) continue;
                const uint8_t x = a.in[i][stripe * a.in_stride[i] + b];
                if (x) acc ^= s_exp[uint32_t(s_log[x]) + s_lc[j * kMaxK + i]];
            }
            crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, acc);
            q[b] = uint8_t(acc);
        }
        sums[(stripe * a.n_total + a.out_id[j]) * a.nck + chunk] = __builtin_bswap32(crc ^ Spec::kXorout);
    }
}

namespace {

struct EncodeRowsFn {
    template <int K, int R>
    static const void* fn(int kind) {
        constexpr int SL = rows_slabs(K, R);
        return kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_crc_rows<RowsEncode, K, R, SL, crc::kCrc32c>)
                                    : reinterpret_cast<const void*>(&gf_crc_rows<RowsEncode, K, R, SL, crc::kCksum>);
    }
};

}  // namespace

int launch_encode_crc_rows(const MatmulArgs& a, const EncodeRowsCrcArgs& cs, const ReconRowsLens& lens, int device,
                           hipStream_t stream) {
    if (a.cell_len == 0 || !cs.sums || (reinterpret_cast<uintptr_t>(cs.sums) & 3u) ||
        cs.n_total < uint32_t(a.k + a.r))
        return -1;
    // grid as launch_reconstruct_crc_rows
    return launch_rows_crc(pick_kr<EncodeRowsFn>(a.k, a.r, cs.kind), rows_slabs(a.k, a.r), a, cs, lens, a.k, a.r, 32,
                           device, stream);
}

int launch_encode_rows_bytes(const EncodeRowsBytesArgs& in, int device, hipStream_t stream) {
    EncodeRowsBytesArgs a = in;
    if (a.k < 1 || a.k > kMaxK || a.r < 1 || a.r > kMaxR || !a.sums || (reinterpret_cast<uintptr_t>(a.sums) & 3u) ||
        !rows_bytes_args_ok(a, uint64_t(a.k)))
        return -1;
    if (uint32_t(a.k) > a.n_total) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || a.out_id[j] >= a.n_total) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i]) return -1;
    a.nck = rows_nck(a.cell_len, a.bytes_per_checksum);
    const uint64_t total = a.nck * uint64_t(a.r + (a.data_sums ? a.k : 0)) * a.stripes;
    if (total == 0) return 0;
    return launch_rows_bytes(&gf_encode_rows_bytes<crc::kCrc32c>, &gf_encode_rows_bytes<crc::kCksum>, a, total, 0, device,
                             stream);
}

}  // namespace hec
