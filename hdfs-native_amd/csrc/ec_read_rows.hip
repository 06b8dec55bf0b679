// ec_read_rows.hip -- verified striped read into a file-order buffer, short
// stripes included (ec_read_rows.hpp): the mirror of the encode of
// ec_encode_rows.hip.  The survivors of a stripe arrive with chunk sums over
// their own bytes; all k data units leave at their file-order place, the
// present ones copied, the lost ones rebuilt, each cut to its own length and
// nothing written at or past the stripe's logical end.
//
// Two kernels, in a translation unit of their own so that the kernels of the
// other short-stripe calls keep their machine code; ec_rows_kernel.hpp is
// included as it stands.
//
// gf_read_rows is the register kernel.  It is gf_crc_rows<RowsRepair>
// (ec_rows_kernel.hpp) with the stores changed, written as a sibling because
// that kernel keeps its assembly in one spelling only (profiles/rows_parts/):
// the same tiles, scalar 32-bit lengths, tile skipping at n0, redirected loads
// of ended units, cut before the GF step and before put, and verify rounds with
// per-slot lengths.  What differs:
//   - An input whose unit is a data unit is stored to its file slot from the
//     registers it was loaded into, after cut, over its own length: whole 16-B
//     blocks below len & ~15, the one partial block bytewise.
//   - The R outputs are the lost data units: masked to their own length and
//     stored over [0, len) only.  They are neither staged nor summed.
//   - R = 0 has no product tables, accumulators or GF step: the verify rounds
//     and the copies alone.
//
// gf_read_rows_bytes is the byte-wise route for every other shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_read_rows.hpp"
#include "ec_rows_kernel.hpp"

namespace hec {

namespace {

// The first `len` <= 15 bytes of a block, one by one.
__device__ __forceinline__ void read_rows_store_part(uint8_t* p, u32x4 v, uint32_t len) {
#pragma unroll
    for (int b = 0; b < 15; b++)
        if (uint32_t(b) < len) p[b] = uint8_t(v[b >> 2] >> (8 * (b & 3)));
}

}  // namespace

// K inputs = the code's k, R lost data units, SLABS KiB of every cell per
// wave-tile, as gf_crc_rows.  Without VERIFY_IN no CRC table is staged and KIND
// has no effect.
template <bool VERIFY_IN, int K, int R, int SLABS, int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_read_rows(MatmulArgs a,
                                                                                                ReadRowsCrcArgs cs,
                                                                                                ReconRowsLens ln) {
    static_assert(K > 0 && R >= 0 && R <= kMaxR, "compile-time k, 0..4 rows");
    using Stage = CrcStage<SLABS, KIND>;
    using TL = typename Stage::TL;
    constexpr int SCHEME = Stage::SCHEME, STAGE = Stage::STAGE, SPR = Stage::SPR;
    constexpr int BS = 256, WAVES = BS / 64;
    constexpr uint32_t WAVE_BYTES = SLABS * 1024u, TILE_BYTES = WAVES * WAVE_BYTES;
    constexpr bool PF = R * SLABS <= 24;  // register prefetch of the next input
    constexpr int RT = R > 0 ? R : 1;     // no zero-length array; without a use the array takes no LDS
    __shared__ PermTable s_tab[RT][K];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[RT * kMaxK];
    __shared__ uint32_t s_ctabs[TL::kWords];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES * STAGE];
    if constexpr (R > 0) prologue<R, BS, K>(a, K, s_tab, s_exp, s_log, s_coef);
    if constexpr (VERIFY_IN) {
        crcdev::stage_tables<SCHEME, BS>(s_ctabs, fused_tables<KIND>());
        __syncthreads();
    }
    const uint32_t kfinal = fused_tables<KIND>().final512;

    const uint64_t cell_len = a.cell_len;
    const uint64_t nck = (cell_len + 511) / 512;  // chunk slots per cell in the sums layout
    const uint32_t total = a.total_tiles;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x / 64)), lane = threadIdx.x & 63;
    const int qi = lane & 3, piece = lane >> 3, sir = piece / SLABS, pslab = piece % SLABS, half = (lane >> 2) & 1;
    uint8_t* stage = s_stage + wave * STAGE;
    const uint32_t* exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;
    const uint32_t lane16 = uint32_t(lane) * 16u;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        // coordinates and the stripe's logical bytes into SGPRs, as gf_crc_rows
        lstripe = uint32_t(__builtin_amdgcn_readfirstlane(int(lstripe)));
        tcol = uint32_t(__builtin_amdgcn_readfirstlane(int(tcol)));
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
        const uint32_t stripe = uint32_t(__builtin_amdgcn_readfirstlane(
            int(cs.stripe_list ? cs.stripe_list[lstripe] : uint32_t(ln.stripe0) + lstripe)));
        // load lanes: live below align_up(n0, 16) <= cell_len, the others
        // re-read offset 0
        const uint32_t nleft = n0 - wbyte;  // > 0
        const uint32_t lleft = (nleft + 15u) & ~15u;
        uint32_t voff[SLABS];
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            const uint32_t o = uint32_t(u) * 1024u + lane16;
            voff[u] = o < lleft ? o : 0u;
        }
        const uint32_t coff = uint32_t(pslab) * 1024u + uint32_t(half) * 512u;  // the lane's chunk in the wave-tile
        const uint64_t cbyte = uint64_t(wbyte) + coff;

        // bytes of the unit in `slot` that lie at or past the wave's first byte
        // (0: the unit ended before this wave-tile)
        auto unit_left = [&](int slot) -> uint32_t {
            const uint32_t len = unit_len(cs.shard_id[slot]);
            return len > wbyte ? len - wbyte : 0u;
        };
        auto cut = [&](u32x4(&v)[SLABS], uint32_t left) {
            if (left < WAVE_BYTES) {  // wave-uniform: the unit ends inside this wave-tile
#pragma unroll
                for (int u = 0; u < SLABS; u++) v[u] = keep_bytes(v[u], int32_t(left) - int32_t(uint32_t(u) * 1024u + lane16));
            }
        };
        // v, cut to `left` bytes, to data unit uid's place in the file: whole
        // blocks, then the one partial block (one lane of one wave of the
        // stripe) bytewise; nothing at or past `left`
        auto to_file = [&](uint32_t uid, const u32x4(&v)[SLABS], uint32_t left) {
            uint8_t* f = cs.file + (uint64_t(stripe) * cs.file_stride + uint64_t(uid) * cell_len + wbyte);
            u32x4 part = u32x4{0, 0, 0, 0};
            uint32_t part_off = 0, part_len = 0;
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
                const uint32_t o = uint32_t(u) * 1024u + lane16;
                if (o + 16u <= left) {
                    store16<true>(f + o, v[u]);
                } else if (o < left) {
                    part = v[u];
                    part_off = o;
                    part_len = left - o;
                }
            }
            if (part_len != 0) read_rows_store_part(f + part_off, part, part_len);
        };
        auto sum_cell = [&](int first, int count) {
            const uint32_t sid =
                (SPR > 1 && sir > 0 && count > 1) ? uint32_t(cs.shard_id[first + 1]) : uint32_t(cs.shard_id[first]);
            return uint64_t(stripe) * cs.n_total + sid;
        };
        // where the loads of an ended unit go: unit 0 if it survived, else the
        // last survivor, which is then a parity unit; both hold n0 bytes
        const uint64_t whole_unit =
            cs.shard_id[0] == 0 ? reinterpret_cast<uint64_t>(a.in[0]) + (uint64_t(stripe) * a.in_stride[0] + wbyte)
                                : reinterpret_cast<uint64_t>(a.in[K - 1]) + (uint64_t(stripe) * a.in_stride[K - 1] + wbyte);
        auto load_in = [&](int i, u32x4(&dst)[SLABS]) {
            uint32_t here = unit_left(i) != 0 ? 0xFFFFFFFFu : 0u;  // wave-uniform
            asm volatile("" : "+v"(here));
            const uint64_t sel = (uint64_t(here) << 32) | here;
            const uint64_t own = reinterpret_cast<uint64_t>(a.in[i]) + (uint64_t(stripe) * a.in_stride[i] + wbyte);
            const gbyte* p = gptr((own & sel) | (whole_unit & ~sel));
#pragma unroll
            for (int u = 0; u < SLABS; u++) dst[u] = gload16(p + (voff[u] & here));
        };

        const uint64_t dummy_len = 0;
        const bool no = false;
        const Stage putter{s_ctabs, stage, kfinal, dummy_len, lane, qi, sir, cbyte, no, no};
        u32x4 acc[SLABS][RT];
        if constexpr (R > 0) {
#pragma unroll
            for (int u = 0; u < SLABS; u++)
#pragma unroll
                for (int j = 0; j < R; j++) acc[u][j] = u32x4{0, 0, 0, 0};
        }
        u32x4 x[SLABS], xn[SLABS];
        load_in(0, x);
#pragma unroll
        for (int i = 0; i < K; i++) {
            if (PF && i + 1 < K) load_in(i + 1, xn);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t left_i = unit_left(i);
            if (left_i != 0) {  // wave-uniform
                cut(x, left_i);
                if constexpr (VERIFY_IN) {
#pragma unroll
                    for (int u = 0; u < SLABS; u++) putter.put(i % SPR, u, x[u]);
                }
                const uint32_t uid = cs.shard_id[i];
                if (uid < uint32_t(K)) to_file(uid, x, left_i);  // wave-uniform: a data unit
                if constexpr (R > 0) {
                    uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
                    asm volatile("" : "+v"(toff));
#pragma unroll
                    for (int u = 0; u < SLABS; u++) {
                        asm volatile("" : "+v"(x[u]));
#pragma unroll
                        for (int j = 0; j < R; j++) asm volatile("" : "+v"(acc[u][j]) : "v"(toff));
                    }
                    uint32_t tb[RT][5];
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
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (VERIFY_IN) {
                // a round once its SPR inputs are staged, or at the last one;
                // skipped when all of them ended before this wave-tile
                if (i % SPR == SPR - 1 || i == K - 1) {
                    const int first = i - i % SPR, count = i % SPR + 1;
                    const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_i : 0u;
                    if ((l0 | l1) != 0) {
                        // the lane's chunk against the length of the unit in its round slot
                        const uint32_t mine = (SPR > 1 && sir > 0 && count > 1) ? l1 : l0;
                        const uint64_t ulen = uint64_t(wbyte) + mine;  // what CrcStage takes for cell_len
                        const bool in_cell = coff < mine;
                        const bool full = in_cell && mine - coff >= 512u;  // same for a chunk's 4 lanes
                        const Stage crc{s_ctabs, stage, kfinal, ulen, lane, qi, sir, cbyte, in_cell, full};
                        crc.round(
                            count, [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                            [&](uint32_t sum, uint32_t want) {
                                if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                            });
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (i + 1 < K) {
                if constexpr (PF) {
#pragma unroll
                    for (int u = 0; u < SLABS; u++) x[u] = xn[u];
                } else {
                    load_in(i + 1, x);
                }
            }
        }
        // the R lost data units: cut to their own length, stored over it
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; j++) {
                const uint32_t left_j = unit_left(K + j);
                if (left_j == 0) continue;  // wave-uniform: empty here
                u32x4 y[SLABS];
#pragma unroll
                for (int u = 0; u < SLABS; u++) y[u] = acc[u][j];
                cut(y, left_j);
                to_file(cs.shard_id[K + j], y, left_j);
            }
        }
    }
}

// Byte-wise route: one lane per (stripe, item, chunk slot); the items of a
// stripe are the k data units, then the a.parity_in parity survivors.  Bytes
// from global memory, log/antilog products and a slice-by-1 CRC step from LDS,
// as gf_reconstruct_rows_bytes.  A data unit's lane works on its chunk's bytes
// below the unit's length: a survivor's are verified against the expected sum
// and copied, a lost unit's formed from the survivors (each zero from its own
// length on) and stored.  A parity survivor's lane verifies and stores nothing.
template <int KIND>
__global__ __launch_bounds__(kBlock) void gf_read_rows_bytes(ReadRowsBytesArgs a) {
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
    const uint32_t k = uint32_t(a.k);
    const uint64_t per_stripe = a.nck * uint64_t(a.k + a.parity_in);
    const uint64_t total = per_stripe * a.stripes;
    const uint32_t* expected = reinterpret_cast<const uint32_t*>(a.expected);
    for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += uint64_t(gridDim.x) * kBlock) {
        const uint64_t s = g / per_stripe;
        const uint64_t rest = g - s * per_stripe;
        const uint32_t item = uint32_t(rest / a.nck);
        const uint64_t chunk = rest - uint64_t(item) * a.nck;
        const uint64_t begin = chunk * bpc;
        const uint64_t r = rows_stripe_bytes(a.lens, s);
        const uint64_t n0 = r < cell_len ? r : cell_len;
        if (begin >= n0) continue;
        const uint64_t stripe = rows_batch_stripe(a.stripe_list, a.lens, s);
        // the survivor slot whose own bytes this lane verifies (-1: none)
        int vi = -1;
        uint32_t role = kReadRowsSkip;
        if (item >= k) {
            vi = a.k - a.parity_in + int(item - k);
        } else {
            role = a.role[item];
            if (role < k) vi = int(role);
        }
        uint64_t len = 0;
        if (vi >= 0) {
            len = rows_unit_len(a.in_id[vi], k, r, n0, cell_len);
            if (begin >= len) continue;
            if (expected) {
                const uint32_t sum = rows_own_chunk_sum<KIND>(s_crc, a.in[vi] + stripe * a.in_stride[vi], begin, len, bpc);
                const uint64_t cell = stripe * a.n_total + a.in_id[vi];
                if (expected[cell * a.nck + chunk] != sum) a.bad[cell] = 1;
            }
        }
        if (item >= k || role == kReadRowsSkip) continue;
        uint8_t* q = a.file + (stripe * a.file_stride + uint64_t(item) * cell_len);
        if (vi >= 0) {  // a present data unit: its own bytes of the chunk
            const uint8_t* p = a.in[vi] + stripe * a.in_stride[vi];
            const uint64_t end = len - begin < bpc ? len : begin + bpc;
            for (uint64_t b = begin; b < end; b++) q[b] = p[b];
            continue;
        }
        len = rows_data_unit_len(item, r, cell_len);
        if (begin >= len) continue;
        const int j = int(role & 3u);
        const uint64_t end = len - begin < bpc ? len : begin + bpc;
        for (uint64_t b = begin; b < end; b++) {
            uint32_t acc = 0;
            for (int i = 0; i < a.k; i++) {
                // survivor i has a byte b: a parity unit always (b < n0), a data unit below its cut
                const uint32_t uid = a.in_id[i];
                if (!s_nz[j * kMaxK + i] || (uid < k && uint64_t(uid) * cell_len + b >= r)) continue;
                const uint8_t x = a.in[i][stripe * a.in_stride[i] + b];
                if (x) acc ^= s_exp[uint32_t(s_log[x]) + s_lc[j * kMaxK + i]];
            }
            q[b] = uint8_t(acc);
        }
    }
}

namespace {

template <int K, int R>
const void* read_rows_fn_r(int kind, bool verify_in) {
    constexpr int SL = rows_slabs(K, R);
    if (!verify_in) return reinterpret_cast<const void*>(&gf_read_rows<false, K, R, SL, crc::kCrc32c>);
    return kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_read_rows<true, K, R, SL, crc::kCrc32c>)
                                : reinterpret_cast<const void*>(&gf_read_rows<true, K, R, SL, crc::kCksum>);
}

// pick_kr with r = 0 as well.
template <int K>
const void* read_rows_fn_k(int r, int kind, bool verify_in) {
    switch (r) {
        case 0: return read_rows_fn_r<K, 0>(kind, verify_in);
        case 1: return read_rows_fn_r<K, 1>(kind, verify_in);
        case 2: return read_rows_fn_r<K, 2>(kind, verify_in);
        case 3: return read_rows_fn_r<K, 3>(kind, verify_in);
        case 4: return read_rows_fn_r<K, 4>(kind, verify_in);
        default: return nullptr;
    }
}

const void* read_rows_fn(int k, int r, int kind, bool verify_in) {
    switch (k) {
        case 2: return read_rows_fn_k<2>(r, kind, verify_in);
        case 3: return read_rows_fn_k<3>(r, kind, verify_in);
        case 6: return read_rows_fn_k<6>(r, kind, verify_in);
        case 10: return read_rows_fn_k<10>(r, kind, verify_in);
        default: return nullptr;
    }
}

}  // namespace

// launch_rows_crc's checks and launch with a.r = 0 allowed and the file in
// place of the output slots.
int launch_read_crc_rows(const MatmulArgs& in, const ReadRowsCrcArgs& cs, const ReconRowsLens& lens, int device,
                         hipStream_t stream) {
    MatmulArgs a = in;
    if (!rows_kind_ok(cs.kind) || a.k < 1 || a.k > kMaxK || a.r < 0 || a.r > kMaxR) return -1;
    const void* fn = read_rows_fn(a.k, a.r, cs.kind, cs.expected != nullptr);
    if (!fn) return -1;
    if (a.cell_len == 0 || a.cell_len % 16 != 0 || a.cell_len > 0x7FFFFFFFull || !rows_lens_ok(lens, uint64_t(a.k), a.cell_len))
        return -1;
    if (lens.stripe0 + a.stripes > 0xFFFFFFFFull) return -1;
    if (!rows_slots_aligned(a.in, a.in_stride, a.k)) return -1;
    if (!cs.file || ((reinterpret_cast<uintptr_t>(cs.file) | cs.file_stride) & 15u) ||
        cs.file_stride < uint64_t(a.k) * a.cell_len)
        return -1;
    if (cs.expected && (!cs.bad || (reinterpret_cast<uintptr_t>(cs.expected) & 3u))) return -1;
    for (int i = 0; i < a.k + a.r; i++)
        if (cs.shard_id[i] >= cs.n_total || (i >= a.k && cs.shard_id[i] >= a.k)) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * uint32_t(rows_slabs(a.k, a.r)))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * 32;  // as launch_reconstruct_crc_rows
    if (grid > total) grid = total;
    ReadRowsCrcArgs c = cs;
    ReconRowsLens l = lens;
    void* args[] = {&a, &c, &l};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

int launch_read_rows_bytes(const ReadRowsBytesArgs& in, int device, hipStream_t stream) {
    ReadRowsBytesArgs a = in;
    if (a.k < 1 || a.k > kMaxK || a.r < 0 || a.r > kMaxR || a.parity_in < 0 || a.parity_in > a.k || !a.file ||
        a.file_stride < uint64_t(a.k) * a.cell_len || !rows_bytes_args_ok(a, uint64_t(a.k)))
        return -1;
    if (a.expected && (!a.bad || (reinterpret_cast<uintptr_t>(a.expected) & 3u))) return -1;
    if (!a.expected && a.parity_in != 0) return -1;
    for (int i = 0; i < a.k; i++) {
        if (!a.in[i] || a.in_id[i] >= a.n_total) return -1;
        const uint8_t role = a.role[i];
        if (role != kReadRowsSkip && !(role < a.k && a.in_id[role] == i) &&
            !((role & kReadRowsLost) && int(role & ~kReadRowsLost) < a.r))
            return -1;
    }
    a.nck = rows_nck(a.cell_len, a.bytes_per_checksum);
    const uint64_t total = a.nck * uint64_t(a.k + a.parity_in) * a.stripes;
    if (total == 0) return 0;
    return launch_rows_bytes(&gf_read_rows_bytes<crc::kCrc32c>, &gf_read_rows_bytes<crc::kCksum>, a, total, 0, device,
                             stream);
}

}  // namespace hec
