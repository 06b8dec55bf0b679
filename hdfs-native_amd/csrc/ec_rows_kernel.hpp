// ec_rows_kernel.hpp -- the shared parts of the short-stripe calls
// (ec_reconstruct_rows.hip, ec_scrub_rows.hip, ec_encode_rows.hip): a stripe
// holds r < k * cell_len logical bytes, so data unit u has min(cell_len,
// max(0, r - u * cell_len)) bytes and every parity unit n0 = min(cell_len, r)
// (ReconRowsLens, ec_reconstruct_rows.hpp).
//
// gf_crc_rows is the register kernel of the repair and of the encode, each
// instantiated in its own translation unit so that neither moves the other's
// machine code (profiles/rows_parts/).  It is gf_reconstruct_crc
// (ec_reconstruct_crc_kernel.hpp) with a length per unit: same tiles, 16-B
// loads, GF step and checksum rounds (crc_stage.hpp), one pass of k reads +
// r writes over [0, n0).  The rules, which gf_scrub_crc_rows
// (ec_scrub_rows.hip) follows for its k + e reads as well:
//   - Lengths live in SGPRs, in 32 bits (SALU has no ordered 64-bit compare):
//     the launcher keeps cell_len below 2^31, r <= k * cell_len, and a data
//     unit starts at a multiple of 16, so r / 16 against the start / 16
//     decides, and the low four bits of r finish the cut unit's length.
//   - Tiles at or past n0 are skipped per wave before any load or store
//     (wave-uniform: n0 is a scalar).
//   - A unit whose length ends at or before the wave's first byte is neither
//     multiplied nor staged and no byte of its slot is read; a round whose
//     units all ended is skipped.
//   - Every unit still issues its SLABS loads, so the loads in flight at any
//     point are a compile-time count and the waits stay exact (loads in a
//     branch made every wait cover the prefetch too).  Those of an ended unit
//     -- an empty unit above all -- go to offset 0 of a unit the mode knows to
//     hold n0 bytes, and their result is never used.  The choice is made with
//     a mask the optimizer cannot see through: as a condition it was merged
//     with the branch around the GF step and the loads went back into
//     branches.
//   - The load lanes are the tile's: live below align_up(n0, 16) <= cell_len,
//     the others re-read offset 0.  Bytes at or past a unit's length are
//     masked to zero in registers before the GF step and before they are
//     staged; the mask is only computed in the wave that holds the unit's end.
//   - A checksum round takes the length of the unit in the lane's round slot
//     where gf_reconstruct_crc takes cell_len, so two units of different
//     lengths share a round (SLABS == 4) and sums slots past a unit's last
//     live chunk are neither read nor written.
//   - Outputs: masked to their length (zeros up to n0), whole 16-B stores
//     below n0 & ~15, the one partial block bytewise, nothing at or past n0.
//
// Below the kernel: the parts of the three byte-wise kernels, and the host
// checks and launch steps of the six launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "ec_encode_rows.hpp"
#include "ec_reconstruct_rows.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "crc_stage.hpp"
#include "ec_fused_kernel.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

namespace {  // per translation unit

// Bytes of data unit `uid` in a stripe of r logical bytes.
__device__ __forceinline__ uint64_t rows_data_unit_len(uint32_t uid, uint64_t r, uint64_t cell_len) {
    const uint64_t before = uint64_t(uid) * cell_len;
    if (r <= before) return 0;
    const uint64_t left = r - before;
    return left < cell_len ? left : cell_len;
}
// ... of any unit: units below data_units are data units, the others hold
// n0 = min(cell_len, r) bytes.
__device__ __forceinline__ uint64_t rows_unit_len(uint32_t uid, uint32_t data_units, uint64_t r, uint64_t n0,
                                                  uint64_t cell_len) {
    return uid >= data_units ? n0 : rows_data_unit_len(uid, r, cell_len);
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

// f(integral_constant<int, 0>), f(<1>), ... in order
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}

// KiB of every cell per wave-tile
constexpr int rows_slabs(int k, int r) { return (r <= 3 && k <= 6) ? 8 : 4; }        // recon_crc_slabs's rule
constexpr int scrub_rows_slabs(int k, int e) { return (e == 1 && k <= 6) ? 8 : 4; }  // scrub_crc_slabs's rule

}  // namespace

// The two modes of gf_crc_rows.  Unit slots 0 .. K-1 are the inputs, K + j is
// output row j.
//
// Repair: the inputs are the plan's survivors, the outputs the lost units,
// slot s is unit shard_id[s].  With VERIFY_IN the inputs' rounds compare with
// the expected sums and set `bad`; without, the inputs are not staged.  An
// ended unit's loads go to unit 0 if it survived, else to the last survivor,
// which is then a parity unit.  An output has its own length.
template <bool VERIFY_IN>
struct RowsRepair {
    using Args = ReconCrcArgs;
    static constexpr bool kEncode = false, kSumIn = VERIFY_IN;
};
// Encode: the inputs are the k data units, the outputs parity units of n0
// bytes, slot s is unit s of the sums layout and every round stores its sums.
// An ended unit's loads go to data unit 0.  No stripe list.
struct RowsEncode {
    using Args = EncodeRowsCrcArgs;
    static constexpr bool kEncode = true, kSumIn = true;
};

// K inputs = the code's k, R output rows, SLABS KiB of every cell per
// wave-tile, as gf_reconstruct_crc.
template <class M, int K, int R, int SLABS, int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_crc_rows(MatmulArgs a,
                                                                                               typename M::Args cs,
                                                                                               ReconRowsLens ln) {
    static_assert(K > 0 && R >= 1 && R <= kMaxR, "compile-time k, 1..4 rows");
    using Stage = CrcStage<SLABS, KIND>;
    using TL = typename Stage::TL;
    constexpr int SCHEME = Stage::SCHEME, STAGE = Stage::STAGE, SPR = Stage::SPR;
    constexpr int BS = 256, WAVES = BS / 64;
    constexpr uint32_t WAVE_BYTES = SLABS * 1024u, TILE_BYTES = WAVES * WAVE_BYTES;
    constexpr bool PF = R * SLABS <= 24;  // register prefetch of the next input
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
    const uint32_t* exp_sums = nullptr;  // the inputs' expected sums (repair)
    if constexpr (!M::kEncode) exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
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
        uint32_t stripe;
        if constexpr (M::kEncode)
            stripe = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(ln.stripe0) + lstripe)));
        else
            stripe = uint32_t(__builtin_amdgcn_readfirstlane(
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

        // the unit in slot `slot`
        auto unit_of = [&](int slot) -> uint32_t {
            if constexpr (M::kEncode)
                return uint32_t(slot);
            else
                return cs.shard_id[slot];
        };
        // bytes of that unit that lie at or past the wave's first byte (0:
        // the unit ended before this wave-tile)
        auto unit_left = [&](int slot) -> uint32_t {
            const uint32_t len = unit_len(unit_of(slot));
            return len > wbyte ? len - wbyte : 0u;
        };
        auto cut = [&](u32x4(&v)[SLABS], uint32_t left) {
            if (left < WAVE_BYTES) {  // wave-uniform: the unit ends inside this wave-tile
#pragma unroll
                for (int u = 0; u < SLABS; u++) v[u] = keep_bytes(v[u], int32_t(left) - int32_t(uint32_t(u) * 1024u + lane16));
            }
        };
        auto sum_cell = [&](int first, int count) {
            const uint32_t sid = (SPR > 1 && sir > 0 && count > 1) ? unit_of(first + 1) : unit_of(first);
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
        // ... whose sums go to the cells of its units
        auto store_round = [&](int first, int count, uint32_t left0, uint32_t left1) {
            round(
                count, left0, left1, [] { return 0u; },
                [&](uint32_t sum, uint32_t) { out_sums[sum_cell(first, count) * nck + cbyte / 512] = sum; });
        };
        // where the loads of an ended unit go
        uint64_t whole_unit;
        if constexpr (M::kEncode)
            whole_unit = reinterpret_cast<uint64_t>(a.in[0]) + (uint64_t(stripe) * a.in_stride[0] + wbyte);
        else
            whole_unit =
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
                if constexpr (M::kSumIn) {
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
            if constexpr (M::kSumIn) {
                // a round once its SPR inputs are staged, or at the last one;
                // skipped when all of them ended before this wave-tile
                if (i % SPR == SPR - 1 || i == K - 1) {
                    const int first = i - i % SPR, count = i % SPR + 1;
                    const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_i : 0u;
                    if ((l0 | l1) != 0) {
                        if constexpr (M::kEncode) {
                            store_round(first, count, l0, l1);
                        } else {
                            round(
                                count, l0, l1, [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                                [&](uint32_t sum, uint32_t want) {
                                    if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                                });
                        }
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
        // the R outputs: cut to their length (a parity unit's is n0, and
        // nleft > 0 of it lie in this wave-tile), stored up to n0, staged, the
        // sums of their own bytes written
#pragma unroll
        for (int j = 0; j < R; j++) {
            const uint32_t left_j = M::kEncode ? nleft : unit_left(K + j);
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
                if (M::kEncode || left_j != 0) putter.put(j % SPR, u, acc[u][j]);
            }
            if (part_len != 0) {
                uint8_t* p = a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + part_off;
#pragma unroll
                for (int b = 0; b < 15; b++)
                    if (uint32_t(b) < part_len) p[b] = uint8_t(part[b >> 2] >> (8 * (b & 3)));
            }
            if (j % SPR == SPR - 1 || j == R - 1) {
                const int first = K + j - j % SPR, count = j % SPR + 1;
                const uint32_t l0 = M::kEncode ? nleft : unit_left(first), l1 = count > 1 ? left_j : 0u;
                if (M::kEncode || (l0 | l1) != 0) store_round(first, count, l0, l1);
            }
        }
    }
}

namespace {

// ---- the byte-wise kernels' parts ----

// The slice-by-1 CRC table and the log/antilog tables into LDS, one entry per
// thread of a kBlock block; the caller's barrier follows.
template <int KIND>
__device__ __forceinline__ void rows_stage_byte_tables(uint32_t (&s_crc)[256], uint8_t (&s_exp)[512],
                                                       uint8_t (&s_log)[256]) {
    static_assert(kBlock == 256, "one table entry per thread");
    const int tid = threadIdx.x;
    s_crc[tid] = fused_tables<KIND>().slice[0][tid];
    s_exp[tid] = kDevGf.exp[tid];
    s_exp[tid + 256] = kDevGf.exp[tid + 256];
    s_log[tid] = kDevGf.log[tid];
}

// Logical bytes of launch stripe s, and its batch stripe.
__device__ __forceinline__ uint64_t rows_stripe_bytes(const ReconRowsLens& lens, uint64_t s) {
    return lens.stripe_bytes ? lens.stripe_bytes[s] : lens.bytes;
}
__device__ __forceinline__ uint64_t rows_batch_stripe(const uint32_t* stripe_list, const ReconRowsLens& lens,
                                                      uint64_t s) {
    return stripe_list ? stripe_list[s] : lens.stripe0 + s;
}

// The sum, as it is stored in memory, of a unit's own bytes of the chunk that
// starts at `begin` < len: p = the unit's slot, len = its length.
template <int KIND>
__device__ __forceinline__ uint32_t rows_own_chunk_sum(const uint32_t (&s_crc)[256], const uint8_t* p, uint64_t begin,
                                                       uint64_t len, uint64_t bpc) {
    using Spec = crc::Spec<KIND>;
    const uint64_t end = len - begin < bpc ? len : begin + bpc;
    uint32_t crc = Spec::kInit;
    for (uint64_t b = begin; b < end; b++) crc = crcdev::byte_step<Spec::kReflected, 1>(s_crc, crc, p[b]);
    return __builtin_bswap32(crc ^ Spec::kXorout);
}

// ---- the launchers' parts (host) ----

inline bool rows_kind_ok(int kind) { return kind == crc::kCrc32c || kind == crc::kCksum; }

// The lengths of a launch over `data_units` data units per stripe.
inline bool rows_lens_ok(const ReconRowsLens& lens, uint64_t data_units, uint64_t cell_len) {
    if (reinterpret_cast<uintptr_t>(lens.stripe_bytes) & 7u) return false;
    return lens.stripe_bytes || (lens.bytes != 0 && lens.bytes <= data_units * cell_len);
}

// n unit slots, each present and with a 16-B aligned base and stride.
inline bool rows_slots_aligned(const uint8_t* const* base, const uint64_t* stride, int n) {
    for (int i = 0; i < n; i++)
        if (!base[i] || ((reinterpret_cast<uintptr_t>(base[i]) | stride[i]) & 15u)) return false;
    return true;
}

// What the three register launchers share.  Checks: the kind, 1 .. kMaxR
// rows, cell_len a multiple of 16 and below 2^31 with stripe0 + stripes below
// 2^32 (the kernels' 32-bit lengths), the lengths, n_in input and n_out output
// slots aligned, a kernel for the shape (fn) and tile counts that fit.  Then
// the tile order and grid of the full-stripe launchers, grid_per_cu blocks per
// CU, and the launch.  0 ok, -1 unsupported (nothing was launched), >0
// hipError_t.
template <class CrcArgs>
int launch_rows_crc(const void* fn, int slabs, MatmulArgs a, CrcArgs c, ReconRowsLens l, int n_in, int n_out,
                    uint32_t grid_per_cu, int device, hipStream_t stream) {
    if (!fn || !rows_kind_ok(c.kind)) return -1;
    if (a.r < 1 || a.r > kMaxR || a.cell_len % 16 != 0 || !rows_lens_ok(l, uint64_t(a.k), a.cell_len)) return -1;
    if (l.stripe0 + a.stripes > 0xFFFFFFFFull || a.cell_len > 0x7FFFFFFFull) return -1;
    if (!rows_slots_aligned(a.in, a.in_stride, n_in) || !rows_slots_aligned(a.out, a.out_stride, n_out)) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * uint32_t(slabs))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * grid_per_cu;
    if (grid > total) grid = total;
    void* args[] = {&a, &c, &l};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

// What the three byte launchers check alike: kind, chunk size, cell_len, the
// lengths over a.data_units data units.
template <class Args>
bool rows_bytes_args_ok(const Args& a, uint64_t data_units) {
    return rows_kind_ok(a.kind) && a.bytes_per_checksum != 0 && a.cell_len != 0 &&
           rows_lens_ok(a.lens, data_units, a.cell_len);
}
inline uint64_t rows_nck(uint64_t cell_len, uint64_t bpc) { return cell_len / bpc + (cell_len % bpc != 0); }

// Launches Kernel<KIND> over one lane per work item, at least min_grid blocks,
// at most 8 per CU.
template <class Args>
int launch_rows_bytes(void (*crc32c)(Args), void (*cksum)(Args), Args& a, uint64_t items, uint64_t min_grid, int device,
                      hipStream_t stream) {
    uint64_t grid = (items + kBlock - 1) / kBlock;
    if (grid < min_grid) grid = min_grid;
    const uint64_t cap = uint64_t(num_cus(device)) * 8;
    if (grid > cap) grid = cap;
    const void* fn = a.kind == crc::kCrc32c ? reinterpret_cast<const void*>(crc32c) : reinterpret_cast<const void*>(cksum);
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(kBlock), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace

}  // namespace hec
