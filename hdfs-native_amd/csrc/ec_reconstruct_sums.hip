// ec_reconstruct_sums.hip -- checksum-only reconstruction, for the block and
// block-group checksum of a degraded group (StripedBlockChecksumReconstructor,
// HDFS-9833 / HDFS-13056): the chunk sums of the lost units computed from the
// k survivors, the rebuilt bytes themselves never written anywhere.  k reads
// per stripe where reconstruct + checksum make k reads + t writes.
//
// Two kernels.  The fused shapes run gf_reconstruct_crc
// (ec_reconstruct_crc_kernel.hpp) with STORE_OUT = false: the accumulators go
// from the GF step straight into the checksum rounds.  Every other shape, and
// the short last stripe of a group, runs gf_reconstruct_sums_bytes below.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_reconstruct_crc_kernel.hpp"
#include "ec_reconstruct_sums.hpp"
#include "launch_parts.hpp"

namespace hec {

// Generic route: one lane per (stripe, target row, chunk), bytes from global
// memory, log/antilog products and a slice-by-1 CRC step from LDS, in the
// style of checksum_chunks_bytes and gf_matmul_bytes.  Survivor i counts as
// zero from in_len[i] on (nothing is read there); target j has out_len[j]
// bytes, its last chunk is short, the slots past it are not written.  With
// a.expected the launch also verifies each survivor over its own in_len[i]
// bytes, one lane per chunk (the short last stripe: checksum_launch knows one
// length per launch and derives the sums layout from it).
template <int KIND>
__global__ __launch_bounds__(kBlock) void gf_reconstruct_sums_bytes(ReconSumsArgs a) {
    using Spec = crc::Spec<KIND>;
    __shared__ uint32_t s_crc[256];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_lc[kMaxR * kMaxK];  // log of each coefficient
    __shared__ uint8_t s_nz[kMaxR * kMaxK];
    const int tid = threadIdx.x;
    s_crc[tid] = fused_tables<KIND>().slice[0][tid];
    s_exp[tid] = kDevGf.exp[tid];
    s_exp[tid + 256] = kDevGf.exp[tid + 256];
    s_log[tid] = kDevGf.log[tid];
    if (tid < kMaxR * kMaxK) {
        const uint8_t c = a.coef[tid];
        s_lc[tid] = kDevGf.log[c];
        s_nz[tid] = c != 0;
    }
    __syncthreads();
    const uint64_t bpc = a.bytes_per_checksum;
    // rows of work per stripe: the r targets, then (verify mode) the k survivors
    const int rows = a.r + (a.expected ? a.k : 0);
    const uint64_t per_stripe = a.chunks * uint64_t(rows);
    const uint64_t total = per_stripe * a.stripes;
    uint32_t* sums = reinterpret_cast<uint32_t*>(a.sums);
    for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += uint64_t(gridDim.x) * kBlock) {
        const uint64_t s = g / per_stripe;
        const uint64_t rest = g - s * per_stripe;
        const int j = int(rest / a.chunks);
        const uint64_t chunk = rest - uint64_t(j) * a.chunks;
        const uint64_t begin = chunk * bpc;
        const uint64_t olen = j < a.r ? a.out_len[j] : a.in_len[j - a.r];
        if (begin >= olen) continue;
        const uint64_t end = olen - begin < bpc ? olen : begin + bpc;
        const uint64_t stripe = a.stripe_list ? a.stripe_list[s] : a.stripe0 + s;
        uint32_t crc = Spec::kInit;
        if (j >= a.r) {  // a survivor's own bytes against its expected sum
            const int i = j - a.r;
            const uint8_t* p = a.in[i] + stripe * a.in_stride[i];
            for (uint64_t b = begin; b < end; b++) crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, p[b]);
            const uint64_t cell = stripe * a.n_total + a.in_id[i];
            if (reinterpret_cast<const uint32_t*>(a.expected)[cell * a.nck + chunk] !=
                __builtin_bswap32(crc ^ Spec::kXorout))
                a.bad[cell] = 1;
            continue;
        }
        for (uint64_t b = begin; b < end; b++) {
            uint32_t acc = 0;
            for (int i = 0; i < a.k; i++) {
                if (b >= a.in_len[i] || !s_nz[j * kMaxK + i]) continue;
                const uint8_t x = a.in[i][stripe * a.in_stride[i] + b];
                if (x) acc ^= s_exp[uint32_t(s_log[x]) + s_lc[j * kMaxK + i]];
            }
            crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, acc);
        }
        sums[(stripe * a.n_total + a.out_id[j]) * a.nck + chunk] = __builtin_bswap32(crc ^ Spec::kXorout);
    }
}

namespace {

struct ReconSumsFn {
    template <int K, int R>
    static const void* fn(int kind, bool verify_in) {
        constexpr int SL = recon_crc_slabs(K, R);
        if (kind == crc::kCrc32c)
            return verify_in
                       ? reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCrc32c, true, false>)
                       : reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCrc32c, false, false>);
        return verify_in ? reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCksum, true, false>)
                         : reinterpret_cast<const void*>(&gf_reconstruct_crc<K, R, SL, crc::kCksum, false, false>);
    }
};

}  // namespace

int launch_reconstruct_sums(const MatmulArgs& in, const ReconCrcArgs& cs, int device, hipStream_t stream) {
    MatmulArgs a = in;
    if (cs.kind != crc::kCrc32c && cs.kind != crc::kCksum) return -1;
    if (a.r < 1 || a.r > kMaxR || a.cell_len % 16 != 0 || !cs.sums || (cs.expected && !cs.bad)) return -1;
    if ((reinterpret_cast<uintptr_t>(cs.sums) | reinterpret_cast<uintptr_t>(cs.expected)) & 3u) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || ((reinterpret_cast<uintptr_t>(a.in[i]) | a.in_stride[i]) & 15u)) return -1;
    for (int j = 0; j < kMaxR; j++) {  // never read: the kernel has no output store
        a.out[j] = nullptr;
        a.out_stride[j] = 0;
    }
    const bool verify_in = cs.expected != nullptr;
    const void* fn = pick_kr<ReconSumsFn>(a.k, a.r, cs.kind, verify_in);
    if (!fn) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * recon_crc_slabs(a.k, a.r))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    // tile order and grid as launch_reconstruct_crc
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * 32;
    if (grid > total) grid = total;
    ReconCrcArgs c = cs;
    void* args[] = {&a, &c};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

int launch_reconstruct_sums_bytes(const ReconSumsArgs& in, int device, hipStream_t stream) {
    ReconSumsArgs a = in;
    if (a.kind != crc::kCrc32c && a.kind != crc::kCksum) return -1;
    if (a.k < 1 || a.k > kMaxK || a.r < 1 || a.r > kMaxR || a.bytes_per_checksum == 0 || a.nck == 0 || !a.sums ||
        (reinterpret_cast<uintptr_t>(a.sums) & 3u))
        return -1;
    uint64_t longest = 0;
    for (int j = 0; j < a.r; j++) {
        if (a.out_id[j] >= a.n_total) return -1;
        if (a.out_len[j] > longest) longest = a.out_len[j];
    }
    if (a.expected && (!a.bad || (reinterpret_cast<uintptr_t>(a.expected) & 3u))) return -1;
    for (int i = 0; i < a.k; i++) {
        if ((!a.in[i] && a.in_len[i] != 0) || a.in_id[i] >= a.n_total) return -1;
        if (a.expected && a.in_len[i] > longest) longest = a.in_len[i];
    }
    a.chunks = (longest + a.bytes_per_checksum - 1) / a.bytes_per_checksum;
    if (a.chunks > a.nck) return -1;  // a unit longer than the cell of the sums layout
    const uint64_t total = a.chunks * uint64_t(a.r + (a.expected ? a.k : 0)) * a.stripes;
    if (total == 0) return 0;
    uint64_t grid = (total + kBlock - 1) / kBlock;
    const uint64_t cap = uint64_t(num_cus(device)) * 8;
    if (grid > cap) grid = cap;
    const void* fn = a.kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_reconstruct_sums_bytes<crc::kCrc32c>)
                                            : reinterpret_cast<const void*>(&gf_reconstruct_sums_bytes<crc::kCksum>);
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(kBlock), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
