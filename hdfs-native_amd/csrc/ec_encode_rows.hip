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
// gf_encode_crc_rows is gf_reconstruct_crc_rows<VERIFY_IN = true>
// (ec_reconstruct_rows.hip) with the k data units as inputs (shard_id is the
// identity) and the inputs' checksum round storing the sum where that kernel
// compares it.  Everything else is that kernel's, for the reasons written
// there: scalar 32-bit lengths, wave-tiles at or past n0 skipped before any
// load, every unit issuing its SLABS loads (those of an ended unit go to
// offset 0 of unit 0, which always holds n0 bytes), bytes past a unit's length
// masked in registers in the wave that holds its end, a round skipped when all
// its units ended, CrcStage built per round from the length of the unit in the
// lane's slot, parity stored in whole 16-B blocks below n0 & ~15 with the one
// partial block bytewise.
//
// gf_encode_rows_bytes is the byte-wise route for every other shape, in the
// style of gf_reconstruct_rows_bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_encode_rows.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "crc_stage.hpp"
#include "ec_fused_kernel.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

namespace {

// Bytes of data unit `uid` in a stripe of r logical bytes.
__device__ __forceinline__ uint64_t rows_unit_len(uint32_t uid, uint64_t r, uint64_t cell_len) {
    const uint64_t before = uint64_t(uid) * cell_len;
    if (r <= before) return 0;
    const uint64_t left = r - before;
    return left < cell_len ? left : cell_len;
}

// The first `valid` bytes of a 16-B block (memory order), the rest zero.
__device__ __forceinline__ u32x4 keep_bytes(u32x4 v, int32_t valid) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int32_t vb = valid - 4 * d;
        const uint32_t m = vb >= 4 ? 0xFFFFFFFFu : (vb <= 0 ? 0u : ((1u << (8 * vb)) - 1u));
        v[d] &= m;
    }
    return v;
}

constexpr int rows_slabs(int k, int r) { return (r <= 3 && k <= 6) ? 8 : 4; }  // recon_crc_slabs's rule

}  // namespace

// K data units, R parity rows, SLABS KiB of every cell per wave-tile, as
// gf_reconstruct_crc_rows.  Unit i < K is data unit i, unit K + j parity row j
// of the launch; their sums go to cells i and K + j of the stripe.
template <int K, int R, int SLABS, int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_encode_crc_rows(
    MatmulArgs a, EncodeRowsCrcArgs cs, ReconRowsLens ln) {
    static_assert(K > 0 && R >= 1 && R <= kMaxR, "compile-time k, 1..4 rows");
    using Stage = CrcStage<SLABS, KIND>;
    using TL = typename Stage::TL;
    constexpr int SCHEME = Stage::SCHEME, STAGE = Stage::STAGE, SPR = Stage::SPR;
    constexpr int BS = 256, WAVES = BS / 64;
    constexpr uint32_t WAVE_BYTES = SLABS * 1024u, TILE_BYTES = WAVES * WAVE_BYTES;
    constexpr bool PF = R * SLABS <= 24;  // register prefetch of the next data unit
    __shared__ PermTable s_tab[R][K];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[R * kMaxK];
    __shared__ uint32_t s_ctabs[TL::kWords];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES * STAGE];
    prologue<R, BS, K>(a, K, s_tab, s_exp, s_log, s_coef);
    crcdev::stage_tables<SCHEME, BS>(s_ctabs, fused_tables<KIND>());
    __syncthreads();
    const uint32_t kfinal = fused_tables<KIND>().final512;

    const uint64_t cell_len = a.cell_len;
    const uint64_t nck = (cell_len + 511) / 512;  // chunk slots per cell in the sums layout
    const uint32_t total = a.total_tiles;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x / 64)), lane = threadIdx.x & 63;
    const int qi = lane & 3, piece = lane >> 3, sir = piece / SLABS, pslab = piece % SLABS, half = (lane >> 2) & 1;
    uint8_t* stage = s_stage + wave * STAGE;
    uint32_t* out_sums = reinterpret_cast<uint32_t*>(cs.sums);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;
    const uint32_t lane16 = uint32_t(lane) * 16u;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        // coordinates and the stripe's logical bytes in SGPRs: every length
        // below is scalar arithmetic and every branch on one a scalar branch
        lstripe = uint32_t(__builtin_amdgcn_readfirstlane(int(lstripe)));
        tcol = uint32_t(__builtin_amdgcn_readfirstlane(int(tcol)));
        // Lengths in 32 bits: the launcher keeps cell_len below 2^31, r <= k *
        // cell_len, and a data unit starts at a multiple of 16, so r / 16
        // against the start / 16 decides, and the low four bits of r finish
        // the cut unit's length.
        const uint64_t r = uniform64(ln.stripe_bytes ? ln.stripe_bytes[lstripe] : ln.bytes);
        const uint32_t r16 = uint32_t(r >> 4), r_lo = uint32_t(r) & 15u;
        const uint32_t cell32 = uint32_t(cell_len), c16 = cell32 >> 4;
        auto unit_len = [&](uint32_t uid) -> uint32_t {
            const uint32_t before16 = uid < uint32_t(K) ? uid * c16 : 0u;  // parity: n0, as unit 0
            if (r16 < before16) return 0u;
            const uint32_t d16 = r16 - before16;
            return d16 >= c16 ? cell32 : ((d16 << 4) | r_lo);
        };
        const uint32_t n0 = unit_len(0);
        const uint32_t wbyte = tcol * TILE_BYTES + wave_off;  // wave's first byte
        if (wbyte >= n0) continue;  // wave-uniform
        const uint32_t stripe = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(ln.stripe0) + lstripe)));
        // load lanes: live below align_up(n0, 16) <= cell_len, the others
        // re-read offset 0; store lanes: whole blocks below n0 & ~15, the
        // block that holds byte n0 - 1 bytewise when n0 % 16 != 0
        const uint32_t nleft = n0 - wbyte;  // > 0
        const uint32_t lleft = (nleft + 15u) & ~15u;
        uint32_t voff[SLABS];
        bool live[SLABS];
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            const uint32_t o = uint32_t(u) * 1024u + lane16;
            live[u] = o < lleft;
            voff[u] = live[u] ? o : 0u;
        }
        const uint32_t coff = uint32_t(pslab) * 1024u + uint32_t(half) * 512u;  // the lane's chunk in the wave-tile
        const uint64_t cbyte = uint64_t(wbyte) + coff;

        // bytes of unit `uid` that lie at or past the wave's first byte (0:
        // the unit ended before this wave-tile)
        auto unit_left = [&](int uid) -> uint32_t {
            const uint32_t len = unit_len(uint32_t(uid));
            return len > wbyte ? len - wbyte : 0u;
        };
        auto cut = [&](u32x4(&v)[SLABS], uint32_t left) {
            if (left < WAVE_BYTES) {  // wave-uniform: the unit ends inside this wave-tile
#pragma unroll
                for (int u = 0; u < SLABS; u++) v[u] = keep_bytes(v[u], int32_t(left) - int32_t(uint32_t(u) * 1024u + lane16));
            }
        };
        auto sum_cell = [&](int first, int count) {
            const uint32_t sid = (SPR > 1 && sir > 0 && count > 1) ? uint32_t(first + 1) : uint32_t(first);
            return uint64_t(stripe) * cs.n_total + sid;
        };
        const uint64_t dummy_len = 0;
        const bool no = false;
        const Stage putter{s_ctabs, stage, kfinal, dummy_len, lane, qi, sir, cbyte, no, no};
        // A round over `count` units, left0 / left1 = unit_left of the round's
        // two slots: the lane's chunk is measured against the length of the
        // unit in its slot, and its sum goes to that unit's cell.
        auto round = [&](int first, int count, uint32_t left0, uint32_t left1) {
            const uint32_t mine = (SPR > 1 && sir > 0 && count > 1) ? left1 : left0;
            const uint64_t ulen = uint64_t(wbyte) + mine;  // what CrcStage takes for cell_len
            const bool in_cell = coff < mine;
            const bool full = in_cell && mine - coff >= 512u;  // same for a chunk's 4 lanes
            const Stage crc{s_ctabs, stage, kfinal, ulen, lane, qi, sir, cbyte, in_cell, full};
            crc.round(
                count, [] { return 0u; },
                [&](uint32_t sum, uint32_t) { out_sums[sum_cell(first, count) * nck + cbyte / 512] = sum; });
        };
        // Every data unit issues its SLABS loads, so the loads in flight at
        // any point are a compile-time count and the waits stay exact.  A unit
        // that ended before this wave-tile -- an empty unit above all -- reads
        // none of its own slot: its loads go to offset 0 of unit 0, which has
        // n0 bytes, and their result is never used.  The choice is made with a
        // mask the optimizer cannot see through (as a condition it was merged
        // with the branch around the GF step and the loads went back into
        // branches).
        const uint64_t whole_unit = reinterpret_cast<uint64_t>(a.in[0]) + (uint64_t(stripe) * a.in_stride[0] + wbyte);
        auto load_in = [&](int i, u32x4(&dst)[SLABS]) {
            uint32_t here = unit_left(i) != 0 ? 0xFFFFFFFFu : 0u;  // wave-uniform
            asm volatile("" : "+v"(here));
            const uint64_t sel = (uint64_t(here) << 32) | here;
            const uint64_t own = reinterpret_cast<uint64_t>(a.in[i]) + (uint64_t(stripe) * a.in_stride[i] + wbyte);
            const gbyte* p = gptr((own & sel) | (whole_unit & ~sel));
#pragma unroll
            for (int u = 0; u < SLABS; u++) dst[u] = gload16(p + (voff[u] & here));
        };

        u32x4 acc[SLABS][R];
#pragma unroll
        for (int u = 0; u < SLABS; u++)
#pragma unroll
            for (int j = 0; j < R; j++) acc[u][j] = u32x4{0, 0, 0, 0};
        u32x4 x[SLABS], xn[SLABS];
        load_in(0, x);
#pragma unroll
        for (int i = 0; i < K; i++) {
            if (PF && i + 1 < K) load_in(i + 1, xn);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t left_i = unit_left(i);
            if (left_i != 0) {  // wave-uniform
                cut(x, left_i);
#pragma unroll
                for (int u = 0; u < SLABS; u++) putter.put(i % SPR, u, x[u]);
                uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
                asm volatile("" : "+v"(toff));
#pragma unroll
                for (int u = 0; u < SLABS; u++) {
                    asm volatile("" : "+v"(x[u]));
#pragma unroll
                    for (int j = 0; j < R; j++) asm volatile("" : "+v"(acc[u][j]) : "v"(toff));
                }
                uint32_t tb[R][5];
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const PermTable& t =
                        *reinterpret_cast<const PermTable*>(reinterpret_cast<const char*>(&s_tab[j][0]) + toff);
                    tb[j][0] = t.t0lo;
                    tb[j][1] = t.t0hi;
                    tb[j][2] = t.t1lo;
                    tb[j][3] = t.t1hi;
                    tb[j][4] = t.t2;
                }
#pragma unroll
                for (int u = 0; u < SLABS; u++)
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const Sel sl = make_sel(x[u][d]);
#pragma unroll
                        for (int j = 0; j < R; j++)
                            acc[u][j][d] ^=
                                gf_mul4(tb[j][0], tb[j][1], tb[j][2], tb[j][3], tb[j][4], sl.s0, sl.s1, sl.s2);
                    }
            }
            __builtin_amdgcn_sched_barrier(0);
            // a round once its SPR data units are staged, or at the last one;
            // skipped when all of them ended before this wave-tile
            if (i % SPR == SPR - 1 || i == K - 1) {
                const int first = i - i % SPR, count = i % SPR + 1;
                const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_i : 0u;
                if ((l0 | l1) != 0) round(first, count, l0, l1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < K) {
                if constexpr (PF) {
#pragma unroll
                    for (int u = 0; u < SLABS; u++) x[u] = xn[u];
                } else {
                    load_in(i + 1, x);
                }
            }
        }
        // the R parity units: n0 bytes each (nleft > 0 of them in this
        // wave-tile), cut there, stored, staged, their sums written
#pragma unroll
        for (int j = 0; j < R; j++) {
            u32x4 part = u32x4{0, 0, 0, 0};
            uint32_t part_off = 0, part_len = 0;
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
                const uint32_t o = uint32_t(u) * 1024u + lane16;
                if (nleft < WAVE_BYTES) acc[u][j] = keep_bytes(acc[u][j], int32_t(nleft) - int32_t(o));
                if (live[u]) {
                    if (o + 16u <= nleft) {
                        store16<true>(a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + o, acc[u][j]);
                    } else {  // one lane of one wave of the stripe
                        part = acc[u][j];
                        part_off = o;
                        part_len = nleft - o;
                    }
                }
                putter.put(j % SPR, u, acc[u][j]);
            }
            if (part_len != 0) {
                uint8_t* p = a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + part_off;
#pragma unroll
                for (int b = 0; b < 15; b++)
                    if (uint32_t(b) < part_len) p[b] = uint8_t(part[b >> 2] >> (8 * (b & 3)));
            }
            if (j % SPR == SPR - 1 || j == R - 1) {
                const int first = K + j - j % SPR, count = j % SPR + 1;
                round(first, count, nleft, count > 1 ? nleft : 0u);
            }
        }
    }
}

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
        const uint64_t r = a.lens.stripe_bytes ? a.lens.stripe_bytes[s] : a.lens.bytes;
        const uint64_t n0 = r < cell_len ? r : cell_len;
        if (begin >= n0) continue;
        const uint64_t stripe = a.lens.stripe0 + s;
        uint32_t crc = Spec::kInit;
        if (j >= a.r) {  // a data unit's own bytes
            const int i = j - a.r;
            const uint64_t len = rows_unit_len(uint32_t(i), r, cell_len);
            if (begin >= len) continue;
            const uint64_t end = len - begin < bpc ? len : begin + bpc;
            const uint8_t* p = a.in[i] + stripe * a.in_stride[i];
            for (uint64_t b = begin; b < end; b++) crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, p[b]);
            sums[(stripe * a.n_total + uint32_t(i)) * a.nck + chunk] = __builtin_bswap32(crc ^ Spec::kXorout);
            continue;
        }
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
        return kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_encode_crc_rows<K, R, SL, crc::kCrc32c>)
                                    : reinterpret_cast<const void*>(&gf_encode_crc_rows<K, R, SL, crc::kCksum>);
    }
};

}  // namespace

int launch_encode_crc_rows(const MatmulArgs& in, const EncodeRowsCrcArgs& cs, const ReconRowsLens& lens, int device,
                           hipStream_t stream) {
    MatmulArgs a = in;
    if (cs.kind != crc::kCrc32c && cs.kind != crc::kCksum) return -1;
    if (a.r < 1 || a.r > kMaxR || a.cell_len == 0 || a.cell_len % 16 != 0 || !cs.sums ||
        cs.n_total < uint32_t(a.k + a.r))
        return -1;
    if (reinterpret_cast<uintptr_t>(cs.sums) & 3u) return -1;
    if (reinterpret_cast<uintptr_t>(lens.stripe_bytes) & 7u) return -1;
    if (!lens.stripe_bytes && (lens.bytes == 0 || lens.bytes > uint64_t(a.k) * a.cell_len)) return -1;
    if (lens.stripe0 + a.stripes > 0xFFFFFFFFull || a.cell_len > 0x7FFFFFFFull) return -1;  // 32-bit lengths
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || ((reinterpret_cast<uintptr_t>(a.in[i]) | a.in_stride[i]) & 15u)) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || ((reinterpret_cast<uintptr_t>(a.out[j]) | a.out_stride[j]) & 15u)) return -1;
    const void* fn = pick_kr<EncodeRowsFn>(a.k, a.r, cs.kind);
    if (!fn) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * rows_slabs(a.k, a.r))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    // tile order and grid as launch_reconstruct_crc_rows
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * 32;
    if (grid > total) grid = total;
    EncodeRowsCrcArgs c = cs;
    ReconRowsLens l = lens;
    void* args[] = {&a, &c, &l};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

int launch_encode_rows_bytes(const EncodeRowsBytesArgs& in, int device, hipStream_t stream) {
    EncodeRowsBytesArgs a = in;
    if (a.kind != crc::kCrc32c && a.kind != crc::kCksum) return -1;
    if (a.k < 1 || a.k > kMaxK || a.r < 1 || a.r > kMaxR || a.bytes_per_checksum == 0 || a.cell_len == 0 || !a.sums ||
        (reinterpret_cast<uintptr_t>(a.sums) & 3u) || (reinterpret_cast<uintptr_t>(a.lens.stripe_bytes) & 7u))
        return -1;
    if (!a.lens.stripe_bytes && (a.lens.bytes == 0 || a.lens.bytes > uint64_t(a.k) * a.cell_len)) return -1;
    if (uint32_t(a.k) > a.n_total) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || a.out_id[j] >= a.n_total) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i]) return -1;
    a.nck = a.cell_len / a.bytes_per_checksum + (a.cell_len % a.bytes_per_checksum != 0);
    const uint64_t total = a.nck * uint64_t(a.r + (a.data_sums ? a.k : 0)) * a.stripes;
    if (total == 0) return 0;
    uint64_t grid = (total + kBlock - 1) / kBlock;
    const uint64_t cap = uint64_t(num_cus(device)) * 8;
    if (grid > cap) grid = cap;
    const void* fn = a.kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_encode_rows_bytes<crc::kCrc32c>)
                                            : reinterpret_cast<const void*>(&gf_encode_rows_bytes<crc::kCksum>);
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(kBlock), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
