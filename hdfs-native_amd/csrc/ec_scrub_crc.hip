// ec_scrub_crc.hip -- scrub fused with the chunk checksums of every unit it
// reads, for the block scanner and the end of a repair: are the present units
// of a stripe consistent with each other (the parity check catches a unit
// whose sums were computed from the wrong bytes, HDFS-15759), and does every
// unit still match the sums that travel with it (what the scanner exists
// for)?  One pass of k + e reads where hec_checksum_verify_device +
// hec_scrub_device make 2 (k + e).
//
// gf_scrub_crc has gf_reconstruct_crc<.., VERIFY_IN = true>'s survivor loop
// (ec_reconstruct_crc.hip; the verify rounds are crc_stage.hpp's) and in the
// place of its output rows the e extras, which are inputs too: loaded into the
// same registers, staged and verified in the same rounds, and XORed into their
// accumulator row, so the accumulators end as the syndromes
//     s_j(b) = XOR_i G[j][i] * u_{S_i}(b)  ^  u_{E_j}(b),   j < e.
// What follows is a register-lean form of gf_scrub_mixed's locate tail
// (ec_scrub_mixed.hip): one OR-reduce and a ballot, a clean
// wave-tile writes nothing; otherwise bad positions are counted, extras ruled
// out by "any other row non-zero", survivors by the packed minors against row
// 0, and one lane sends two plain 64-bit atomics.  Uniform plan per launch,
// optional stripe list, block tiles in the fixed order: no counters, nothing
// to zero but the results, capturable as is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "ec_scrub_crc.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "crc_stage.hpp"
#include "ec_fused_kernel.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

namespace {
// f(integral_constant<int, 0>), f(<1>), ... in order
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
}  // namespace

// K survivors, E extras (= rows of G), SLABS KiB of every cell per wave-tile;
// a checksum round is 64 quarters = 8 / SLABS cells' share.
// Needs G[0][i] != 0 for every survivor i (the launcher checks): a vector s is
// then a multiple of column i exactly when the e-1 minors
// s_0 * G[j][i] ^ s_j * G[0][i] vanish.
template <int K, int E, int SLABS, int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_scrub_crc(MatmulArgs a,
                                                                                                ScrubCrcArgs cs) {
    static_assert(K > 0 && E >= 1 && E <= kMaxR, "compile-time k, 1..4 checks");
    constexpr int N = K + E;  // cells read per stripe
    using Stage = CrcStage<SLABS, KIND>;
    using TL = typename Stage::TL;
    constexpr int SCHEME = Stage::SCHEME, STAGE = Stage::STAGE, SPR = Stage::SPR;
    constexpr int BS = 256, WAVES = BS / 64;
    constexpr uint32_t WAVE_BYTES = SLABS * 1024u, TILE_BYTES = WAVES * WAVE_BYTES;
    constexpr bool PF = E * SLABS <= 24;  // register prefetch of the next unit
    __shared__ PermTable s_tab[E][K];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[E * kMaxK];
    __shared__ uint32_t s_ctabs[TL::kWords];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[WAVES * STAGE];
    prologue<E, BS, K>(a, K, s_tab, s_exp, s_log, s_coef);
    crcdev::stage_tables<SCHEME, BS>(s_ctabs, fused_tables<KIND>());
    __syncthreads();
    const uint32_t kfinal = fused_tables<KIND>().final512;

    const uint64_t cell_len = a.cell_len;
    const uint64_t nck = (cell_len + 511) / 512;  // checksum chunks per cell
    const uint32_t total = a.total_tiles;
    // the wave index as a scalar: byte offsets, unit bases and the stage
    // pointer stay in SGPRs (saddr + 32-bit lane offset accesses)
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x / 64)), lane = threadIdx.x & 63;
    // this lane's quarter in a round: row `lane` = piece lane/8 = (cell slot
    // sir, slab), chunk half (lane/4)&1 of that slab, quarter qi
    const int qi = lane & 3, piece = lane >> 3, sir = piece / SLABS, pslab = piece % SLABS, half = (lane >> 2) & 1;
    uint8_t* stage = s_stage + wave * STAGE;
    const uint32_t* exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(cs.results);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        const uint64_t wbyte = uint64_t(tcol) * TILE_BYTES + wave_off;  // wave's first byte
        if (wbyte >= cell_len) continue;  // wave-uniform
        // the batch stripe of this launch stripe: addresses, sums, flags, results
        const uint32_t stripe = cs.stripe_list ? cs.stripe_list[lstripe] : lstripe;
        // dead slabs of a short last tile re-read offset 0 and are masked out
        // of the findings (32-bit compare: see gf_fused_crc)
        const uint64_t left = cell_len - wbyte;
        const uint32_t left32 = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(left);
        uint32_t voff[SLABS];
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            const uint32_t o = uint32_t(u) * 1024u + uint32_t(lane) * 16u;
            voff[u] = o < left32 ? o : 0u;
        }
        const uint64_t cbyte = wbyte + uint64_t(pslab) * 1024u + uint64_t(half) * 512u;
        const bool in_cell = cbyte < cell_len;
        const bool full = in_cell && cell_len - cbyte >= 512u;  // same for a chunk's 4 lanes

        // The cell of this lane's quarter in a round whose slot 0 is unit
        // shard_id[first] (`first` is a compile-time constant at every
        // unrolled call site: scalar kernarg reads); slot 1 only exists when
        // the round has two cells.
        auto sum_cell = [&](int first, int count) {
            const uint32_t sid = (SPR > 1 && sir > 0 && count > 1) ? cs.shard_id[first + 1] : cs.shard_id[first];
            return uint64_t(stripe) * cs.n_total + sid;
        };
        const Stage crc{s_ctabs, stage, kfinal, cell_len, lane, qi, sir, cbyte, in_cell, full};
        // `count` cells starting at unit slot `first` of shard_id, compared
        // against the expected sums
        auto verify_round = [&](int first, int count) {
            crc.round(
                count, [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                [&](uint32_t sum, uint32_t want) {
                    if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                });
        };
        auto load_in = [&](int i, u32x4(&dst)[SLABS]) {
#pragma unroll
            for (int u = 0; u < SLABS; u++)
                dst[u] = load16<true>(a.in[i] + (uint64_t(stripe) * a.in_stride[i] + wbyte) + voff[u]);
        };

        u32x4 acc[SLABS][E];
#pragma unroll
        for (int u = 0; u < SLABS; u++)
#pragma unroll
            for (int j = 0; j < E; j++) acc[u][j] = u32x4{0, 0, 0, 0};
        u32x4 x[SLABS], xn[SLABS];
        load_in(0, x);
        // units 0 .. K-1: the survivors, multiplied into every row; units
        // K .. N-1: the extras, each XORed into its own row
        // (a step per unit through static_for: the unit index is a constant
        // in every step, so no accumulator is ever indexed at run time)
        auto unit_step = [&](auto unit) __attribute__((always_inline)) {
            constexpr int i = decltype(unit)::value;
            if constexpr (PF && i + 1 < N) load_in(i + 1, xn);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < SLABS; u++) crc.put(i % SPR, u, x[u]);
            if constexpr (i < K) {
                // opaque per-input table offset threaded through the
                // accumulators: keeps the table reads (and the GF math) of
                // input i from being hoisted next to those of the others
                uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
                asm volatile("" : "+v"(toff));
#pragma unroll
                for (int u = 0; u < SLABS; u++) {
                    asm volatile("" : "+v"(x[u]));
#pragma unroll
                    for (int j = 0; j < E; j++) asm volatile("" : "+v"(acc[u][j]) : "v"(toff));
                }
                uint32_t tb[E][5];
#pragma unroll
                for (int j = 0; j < E; j++) {
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
                        for (int j = 0; j < E; j++)
                            acc[u][j][d] ^=
                                gf_mul4(tb[j][0], tb[j][1], tb[j][2], tb[j][3], tb[j][4], sl.s0, sl.s1, sl.s2);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < SLABS; u++) acc[u][i - K] ^= x[u];
            }
            __builtin_amdgcn_sched_barrier(0);
            // a round once its SPR units are staged, or at the last one
            if constexpr (i % SPR == SPR - 1 || i == N - 1) verify_round(i - i % SPR, i % SPR + 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i + 1 < N) {
                if constexpr (PF) {
#pragma unroll
                    for (int u = 0; u < SLABS; u++) x[u] = xn[u];
                } else {
                    load_in(i + 1, x);
                }
            }
        };
        static_for(unit_step, std::make_integer_sequence<int, N>{});
        // acc = the syndromes.  One OR-reduce and a ballot: a clean wave-tile
        // ends here (wave-uniform branch; no store, no atomic)
        uint32_t nz = 0;
#pragma unroll
        for (int u = 0; u < SLABS; u++)
#pragma unroll
            for (int j = 0; j < E; j++) nz |= acc[u][j][0] | acc[u][j][1] | acc[u][j][2] | acc[u][j][3];
        if (__builtin_amdgcn_ballot_w64(nz != 0) == 0) continue;
        // this lane's bad byte positions and ruled-out positions of the plan:
        // bit i < K survivor i, bit K + j extra j
        uint32_t cnt = 0, ruled = 0;
        uint32_t anyj[E];  // OR of s_j over this lane's positions
#pragma unroll
        for (int j = 0; j < E; j++) anyj[j] = 0;
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            // a lane past the cell contributes nothing: masked in place
            const uint32_t keep = uint32_t(u) * 1024u + uint32_t(lane) * 16u < left32 ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int d = 0; d < 4; d++) {
                uint32_t b = 0;
#pragma unroll
                for (int j = 0; j < E; j++) {
                    acc[u][j][d] &= keep;
                    anyj[j] |= acc[u][j][d];
                    b |= acc[u][j][d];
                }
                // bit 0 of every byte = the byte is non-zero
                b |= b >> 4;
                b |= b >> 2;
                b |= b >> 1;
                cnt += uint32_t(__builtin_popcount(b & 0x01010101u));
            }
            __builtin_amdgcn_sched_barrier(0);  // one slab at a time: no pile of temporaries
        }
        // extra j0 (column e_j0): ruled out when any other s_j is non-zero at
        // some position (such a position is a bad one whatever s_j0 is there)
#pragma unroll
        for (int j0 = 0; j0 < E; j0++) {
            uint32_t other = 0;
#pragma unroll
            for (int j = 0; j < E; j++)
                if (j != j0) other |= anyj[j];
            ruled |= other != 0 ? (1u << (K + j0)) : 0u;
        }
        if constexpr (E > 1) {
            // survivor t: the packed minors s_0 * G[j][t] ^ s_j * G[0][t],
            // 1 <= j < e, ORed over the lane's positions.  One slab at a
            // time (its syndromes are dead afterwards) and one survivor at a
            // time, the selectors made on the way: the rare path stays small
            // in registers
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
#pragma unroll 1
                for (int t = 0; t < K; t++) {
                    // opaque per survivor: the selectors are loop invariants,
                    // and hoisted they take 3 registers per syndrome dword
#pragma unroll
                    for (int j = 0; j < E; j++) asm volatile("" : "+v"(acc[u][j]));
                    uint32_t tb[E][5];
#pragma unroll
                    for (int j = 0; j < E; j++) {
                        const PermTable& p = s_tab[j][t];
                        tb[j][0] = p.t0lo;
                        tb[j][1] = p.t0hi;
                        tb[j][2] = p.t1lo;
                        tb[j][3] = p.t1hi;
                        tb[j][4] = p.t2;
                    }
                    uint32_t r = 0;
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const Sel s0 = make_sel(acc[u][0][d]);
#pragma unroll
                        for (int j = 1; j < E; j++) {
                            const Sel sj = make_sel(acc[u][j][d]);
                            r |= gf_mul4(tb[j][0], tb[j][1], tb[j][2], tb[j][3], tb[j][4], s0.s0, s0.s1, s0.s2) ^
                                 gf_mul4(tb[0][0], tb[0][1], tb[0][2], tb[0][3], tb[0][4], sj.s0, sj.s1, sj.s2);
                        }
                    }
                    ruled |= r != 0 ? (1u << t) : 0u;
                }
            }
        }
        // over the wave, then one lane maps the plan's positions to unit
        // indices, adds the missing units and sends plain atomics
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += uint32_t(__shfl_xor(int(cnt), o, 64));
            ruled |= uint32_t(__shfl_xor(int(ruled), o, 64));
        }
        if (lane == 0 && cnt != 0) {
            unsigned long long units = cs.missing;
#pragma unroll
            for (int i = 0; i < N; i++)
                if ((ruled >> i) & 1u) units |= 1ull << (cs.shard_id[i] & 63u);
            if (units != 0) atomicOr(results + 2 * uint64_t(stripe), units);
            atomicAdd(results + 2 * uint64_t(stripe) + 1, static_cast<unsigned long long>(cnt));
        }
    }
}

namespace {

// SLABS by fused_slabs's rule (ec_fused.hip: 8 slabs per wave while k <= 6
// and e <= 3, else 4), cut down to the shapes that stay out of scratch: with
// 8 slabs every e >= 2 spills (the syndromes stay live through the locate
// tail, where gf_reconstruct_crc's rows are stored and gone), so only e == 1
// keeps them
constexpr int scrub_crc_slabs(int k, int e) { return (e == 1 && k <= 6) ? 8 : 4; }

struct ScrubCrcFn {
    template <int K, int E>
    static const void* fn(int kind) {
        constexpr int SL = scrub_crc_slabs(K, E);
        if (kind == crc::kCrc32c) return reinterpret_cast<const void*>(&gf_scrub_crc<K, E, SL, crc::kCrc32c>);
        return reinterpret_cast<const void*>(&gf_scrub_crc<K, E, SL, crc::kCksum>);
    }
};

}  // namespace

int launch_scrub_crc(const MatmulArgs& in, const ScrubCrcArgs& cs, int device, hipStream_t stream) {
    MatmulArgs a = in;
    if (cs.kind != crc::kCrc32c && cs.kind != crc::kCksum) return -1;
    if (a.k < 1 || a.k > kMaxK - kMaxR || a.r < 1 || a.r > kMaxR || a.cell_len == 0 || a.cell_len % 16 != 0 ||
        !cs.expected || !cs.bad || !cs.results || cs.n_total == 0)
        return -1;
    if ((reinterpret_cast<uintptr_t>(cs.expected) & 3u) || (reinterpret_cast<uintptr_t>(cs.results) & 7u)) return -1;
    for (int i = 0; i < a.k + a.r; i++)
        if (!a.in[i] || ((reinterpret_cast<uintptr_t>(a.in[i]) | a.in_stride[i]) & 15u) ||
            cs.shard_id[i] >= cs.n_total)
            return -1;
    for (int i = 0; i < a.k; i++)
        if (a.coef[i] == 0) return -1;  // the minors divide by row 0
    const void* fn = pick_kr<ScrubCrcFn>(a.k, a.r, cs.kind);
    if (!fn) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 4096u * scrub_crc_slabs(a.k, a.r))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    // groups of 8 stripes as launch_reconstruct_crc, but 4 blocks per CU (2
    // resident) where it takes 32, and only the resident 2 for a launch over
    // a stripe list: a mixed batch is one launch per mask over a ninth or a
    // fourteenth of the stripes, and with 32 most blocks staged their tables
    // for a single tile (measured: DESIGN.md 3.4f)
    set_tile_order(a, tn, 8u);
    uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(num_cus(device)) * (cs.stripe_list ? 2 : 4);
    if (grid > total) grid = total;
    ScrubCrcArgs c = cs;
    void* args[] = {&a, &c};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
