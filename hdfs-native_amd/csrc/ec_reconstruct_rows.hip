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
// gf_reconstruct_crc_rows is gf_reconstruct_crc (ec_reconstruct_crc_kernel.hpp)
// with a length per unit: same tiles, 16-B loads, GF step and checksum rounds
// (crc_stage.hpp), one pass of k reads + t writes over [0, n0).
//   - Tiles at or past n0 are skipped per wave (wave-uniform: n0 is a scalar).
//   - A survivor whose length ends at or before the wave's first byte is
//     neither multiplied nor staged and no byte of its slot is read
//     (wave-uniform again); a round whose units all ended is skipped.
//   - The load lanes are the tile's: live below align_up(n0, 16), the others
//     re-read offset 0.  Bytes at or past a unit's length are masked to zero
//     in registers before the GF step and before they are staged; the mask is
//     only computed in the wave that holds the unit's end.
//   - A checksum round takes the length of the unit in the lane's round slot
//     where gf_reconstruct_crc takes cell_len, so two units of different
//     lengths share a round (SLABS == 4) and sums slots past a unit's last
//     live chunk are neither read nor written.
//   - Targets: masked to their length (zeros up to n0), whole 16-B stores
//     below n0 & ~15, the one partial block bytewise.
//
// gf_reconstruct_rows_bytes is the byte-wise route for every other shape, in
// the style of gf_reconstruct_sums_bytes with the rebuilt bytes stored too.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_reconstruct_rows.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "crc_stage.hpp"
#include "ec_fused_kernel.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

namespace {

// Bytes of unit `uid` in a stripe of r logical bytes (n0 = min(cell_len, r)).
__device__ __forceinline__ uint64_t rows_unit_len(uint32_t uid, uint32_t data_units, uint64_t r, uint64_t n0,
                                                  uint64_t cell_len) {
    if (uid >= data_units) return n0;
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

// K survivors = the code's k, R target rows, SLABS KiB of every cell per
// wave-tile, as gf_reconstruct_crc.
template <int K, int R, int SLABS, int KIND, bool VERIFY_IN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_reconstruct_crc_rows(
    MatmulArgs a, ReconCrcArgs cs, ReconRowsLens ln) {
    static_assert(K > 0 && R >= 1 && R <= kMaxR, "compile-time k, 1..4 rows");
    using Stage = CrcStage<SLABS, KIND>;
    using TL = typename Stage::TL;
    constexpr int SCHEME = Stage::SCHEME, STAGE = Stage::STAGE, SPR = Stage::SPR;
    constexpr int BS = 256, WAVES = BS / 64;
    constexpr uint32_t WAVE_BYTES = SLABS * 1024u, TILE_BYTES = WAVES * WAVE_BYTES;
    constexpr bool PF = R * SLABS <= 24;  // register prefetch of the next survivor
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
    const uint32_t* exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;
    const uint32_t lane16 = uint32_t(lane) * 16u;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        // The tile's coordinates (their division runs on the VALU) and the
        // stripe's logical bytes (the list is read with a vector load) moved
        // into SGPRs: every length below is scalar arithmetic and every branch
        // on one a scalar branch.
        lstripe = uint32_t(__builtin_amdgcn_readfirstlane(int(lstripe)));
        tcol = uint32_t(__builtin_amdgcn_readfirstlane(int(tcol)));
        // Lengths in 32 bits (SALU has no ordered 64-bit compare): the
        // launcher keeps cell_len below 2^31, r <= k * cell_len, and a data
        // unit starts at a multiple of 16, so r / 16 against the start / 16
        // decides, and the low four bits of r finish the cut unit's length.
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

        // bytes of unit slot `slot` of shard_id that lie at or past the
        // wave's first byte (0: the unit ended before this wave-tile)
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
        auto sum_cell = [&](int first, int count) {
            const uint32_t sid = (SPR > 1 && sir > 0 && count > 1) ? cs.shard_id[first + 1] : cs.shard_id[first];
            return uint64_t(stripe) * cs.n_total + sid;
        };
        const uint64_t dummy_len = 0;
        const bool no = false;
        const Stage putter{s_ctabs, stage, kfinal, dummy_len, lane, qi, sir, cbyte, no, no};
        // A round over `count` units, left0 / left1 = unit_left of the round's
        // two slots: the lane's chunk is measured against the length of the
        // unit in its slot.
        auto round = [&](int count, uint32_t left0, uint32_t left1, auto&& before, auto&& after) {
            const uint32_t mine = (SPR > 1 && sir > 0 && count > 1) ? left1 : left0;
            const uint64_t ulen = uint64_t(wbyte) + mine;  // what CrcStage takes for cell_len
            const bool in_cell = coff < mine;
            const bool full = in_cell && mine - coff >= 512u;  // same for a chunk's 4 lanes
            const Stage crc{s_ctabs, stage, kfinal, ulen, lane, qi, sir, cbyte, in_cell, full};
            crc.round(count, before, after);
        };
        // Every survivor issues its SLABS loads, so the loads in flight at any
        // point are a compile-time count and the waits stay exact (loads in a
        // branch made every wait cover the prefetch too).  A survivor that
        // ended before this wave-tile -- an empty unit above all -- reads none
        // of its own slot: its loads go to offset 0 of a survivor that has n0
        // bytes (unit 0, or else the last survivor, which is then a parity
        // unit) and their result is never used.
        // The choice is made with a mask the optimizer cannot see through:
        // as a condition it was merged with the branch around the GF step
        // and the loads went back into branches.
        const uint64_t whole_unit =
            cs.shard_id[0] == 0
                ? reinterpret_cast<uint64_t>(a.in[0]) + (uint64_t(stripe) * a.in_stride[0] + wbyte)
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
                if constexpr (VERIFY_IN) {
#pragma unroll
                    for (int u = 0; u < SLABS; u++) putter.put(i % SPR, u, x[u]);
                }
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
            if constexpr (VERIFY_IN) {
                // a round once its SPR survivors are staged, or at the last
                // one; skipped when all of them ended before this wave-tile
                if (i % SPR == SPR - 1 || i == K - 1) {
                    const int first = i - i % SPR, count = i % SPR + 1;
                    const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_i : 0u;
                    if ((l0 | l1) != 0)
                        round(
                            count, l0, l1,
                            [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                            [&](uint32_t sum, uint32_t want) {
                                if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                            });
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
        // the R rebuilt units: cut to their length, stored up to n0, staged,
        // the sums of their own bytes written
#pragma unroll
        for (int j = 0; j < R; j++) {
            const uint32_t left_j = unit_left(K + j);
            u32x4 part = u32x4{0, 0, 0, 0};
            uint32_t part_off = 0, part_len = 0;
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
                const uint32_t o = uint32_t(u) * 1024u + lane16;
                if (left_j < WAVE_BYTES) acc[u][j] = keep_bytes(acc[u][j], int32_t(left_j) - int32_t(o));
                if (live[u]) {
                    if (o + 16u <= nleft) {
                        store16<true>(a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + o, acc[u][j]);
                    } else {  // one lane of one wave of the stripe
                        part = acc[u][j];
                        part_off = o;
                        part_len = nleft - o;
                    }
                }
                if (left_j != 0) putter.put(j % SPR, u, acc[u][j]);
            }
            if (part_len != 0) {
                uint8_t* p = a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + part_off;
#pragma unroll
                for (int b = 0; b < 15; b++)
                    if (uint32_t(b) < part_len) p[b] = uint8_t(part[b >> 2] >> (8 * (b & 3)));
            }
            if (j % SPR == SPR - 1 || j == R - 1) {
                const int first = K + j - j % SPR, count = j % SPR + 1;
                const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_j : 0u;
                if ((l0 | l1) != 0)
                    round(
                        count, l0, l1, [] { return 0u; },
                        [&](uint32_t sum, uint32_t) { out_sums[sum_cell(first, count) * nck + cbyte / 512] = sum; });
            }
        }
    }
}

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
        const uint64_t r = a.lens.stripe_bytes ? a.lens.stripe_bytes[s] : a.lens.bytes;
        const uint64_t n0 = r < cell_len ? r : cell_len;
        if (begin >= n0) continue;
        const uint64_t stripe = a.stripe_list ? a.stripe_list[s] : a.lens.stripe0 + s;
        uint32_t crc = Spec::kInit;
        if (j >= a.r) {  // a survivor's own bytes against its expected sums
            const int i = j - a.r;
            const uint64_t len = rows_unit_len(a.in_id[i], a.data_units, r, n0, cell_len);
            if (begin >= len) continue;
            const uint64_t end = len - begin < bpc ? len : begin + bpc;
            const uint8_t* p = a.in[i] + stripe * a.in_stride[i];
            for (uint64_t b = begin; b < end; b++) crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, p[b]);
            const uint64_t cell = stripe * a.n_total + a.in_id[i];
            if (reinterpret_cast<const uint32_t*>(a.expected)[cell * a.nck + chunk] !=
                __builtin_bswap32(crc ^ Spec::kXorout))
                a.bad[cell] = 1;
            continue;
        }
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
            return verify_in ? reinterpret_cast<const void*>(&gf_reconstruct_crc_rows<K, R, SL, crc::kCrc32c, true>)
                             : reinterpret_cast<const void*>(&gf_reconstruct_crc_rows<K, R, SL, crc::kCrc32c, false>);
        return verify_in ? reinterpret_cast<const void*>(&gf_reconstruct_crc_rows<K, R, SL, crc::kCksum, true>)
                         : reinterpret_cast<const void*>(&gf_reconstruct_crc_rows<K, R, SL, crc::kCksum, false>);
    }
};

}  // namespace

int launch_reconstruct_crc_rows(const MatmulArgs& in, const ReconCrcArgs& cs, const ReconRowsLens& lens, int device,
                                hipStream_t stream) {
    MatmulArgs a = in;
    if (cs.kind != crc::kCrc32c && cs.kind != crc::kCksum) return -1;
    if (a.r < 1 || a.r > kMaxR || a.cell_len % 16 != 0 || !cs.sums || (cs.expected && !cs.bad)) return -1;
    if ((reinterpret_cast<uintptr_t>(cs.sums) | reinterpret_cast<uintptr_t>(cs.expected)) & 3u) return -1;
    if (reinterpret_cast<uintptr_t>(lens.stripe_bytes) & 7u) return -1;
    if (!lens.stripe_bytes && (lens.bytes == 0 || lens.bytes > uint64_t(a.k) * a.cell_len)) return -1;
    if (lens.stripe0 + a.stripes > 0xFFFFFFFFull || a.cell_len > 0x7FFFFFFFull) return -1;  // 32-bit lengths
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || ((reinterpret_cast<uintptr_t>(a.in[i]) | a.in_stride[i]) & 15u)) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || ((reinterpret_cast<uintptr_t>(a.out[j]) | a.out_stride[j]) & 15u)) return -1;
    const bool verify_in = cs.expected != nullptr;
    const void* fn = pick_kr<ReconRowsFn>(a.k, a.r, cs.kind, verify_in);
    if (!fn) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * rows_slabs(a.k, a.r))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    // tile order and grid as launch_reconstruct_crc
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * 32;
    if (grid > total) grid = total;
    ReconCrcArgs c = cs;
    ReconRowsLens l = lens;
    void* args[] = {&a, &c, &l};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

int launch_reconstruct_rows_bytes(const ReconRowsBytesArgs& in, int device, hipStream_t stream) {
    ReconRowsBytesArgs a = in;
    if (a.kind != crc::kCrc32c && a.kind != crc::kCksum) return -1;
    if (a.k < 1 || a.k > kMaxK || a.r < 1 || a.r > kMaxR || a.bytes_per_checksum == 0 || a.cell_len == 0 || !a.sums ||
        (reinterpret_cast<uintptr_t>(a.sums) & 3u) || (reinterpret_cast<uintptr_t>(a.lens.stripe_bytes) & 7u))
        return -1;
    if (!a.lens.stripe_bytes && (a.lens.bytes == 0 || a.lens.bytes > uint64_t(a.data_units) * a.cell_len)) return -1;
    if (a.expected && (!a.bad || (reinterpret_cast<uintptr_t>(a.expected) & 3u))) return -1;
    for (int j = 0; j < a.r; j++)
        if (!a.out[j] || a.out_id[j] >= a.n_total) return -1;
    for (int i = 0; i < a.k; i++)
        if (!a.in[i] || a.in_id[i] >= a.n_total) return -1;
    a.nck = a.cell_len / a.bytes_per_checksum + (a.cell_len % a.bytes_per_checksum != 0);
    const uint64_t total = a.nck * uint64_t(a.r + (a.expected ? a.k : 0)) * a.stripes;
    if (total == 0) return 0;
    uint64_t grid = (total + kBlock - 1) / kBlock;
    const uint64_t cap = uint64_t(num_cus(device)) * 8;
    if (grid > cap) grid = cap;
    const void* fn = a.kind == crc::kCrc32c ? reinterpret_cast<const void*>(&gf_reconstruct_rows_bytes<crc::kCrc32c>)
                                            : reinterpret_cast<const void*>(&gf_reconstruct_rows_bytes<crc::kCksum>);
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(kBlock), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
