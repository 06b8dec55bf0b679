// ec_reconstruct_crc_kernel.hpp -- the kernel of ec_reconstruct_crc.hip
// (gf_reconstruct_crc, described there), in a header so that its two sets of
// instantiations compile apart: STORE_OUT = true in ec_reconstruct_crc.hip
// (the rebuilt units stored and checksummed), STORE_OUT = false in
// ec_reconstruct_sums.hip (checksummed only: a.out is never dereferenced and
// no cell byte is written).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_reconstruct_crc.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "crc_stage.hpp"
#include "ec_fused_kernel.hpp"
#pragma clang diagnostic pop

namespace hec {

// K survivors, R target rows, SLABS KiB of every cell per wave-tile; a
// checksum round is 64 quarters = 8 / SLABS cells' share.
template <int K, int R, int SLABS, int KIND, bool VERIFY_IN, bool STORE_OUT = true>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_reconstruct_crc(MatmulArgs a,
                                                                                                      ReconCrcArgs cs) {
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
    const uint64_t nck = (cell_len + 511) / 512;  // checksum chunks per cell
    const uint32_t total = a.total_tiles;
    // the wave index as a scalar: byte offsets, unit bases and the stage
    // pointer stay in SGPRs (saddr + 32-bit lane offset accesses)
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x / 64)), lane = threadIdx.x & 63;
    // this lane's quarter in a round: row `lane` = piece lane/8 = (cell slot
    // sir, slab), chunk half (lane/4)&1 of that slab, quarter qi
    const int qi = lane & 3, piece = lane >> 3, sir = piece / SLABS, pslab = piece % SLABS, half = (lane >> 2) & 1;
    uint8_t* stage = s_stage + wave * STAGE;
    uint32_t* out_sums = reinterpret_cast<uint32_t*>(cs.sums);
    const uint32_t* exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        const uint64_t wbyte = uint64_t(tcol) * TILE_BYTES + wave_off;  // wave's first byte
        if (wbyte >= cell_len) continue;  // wave-uniform
        // the batch stripe of this launch stripe: addresses, sums and flags
        const uint32_t stripe = cs.stripe_list ? cs.stripe_list[lstripe] : lstripe;
        // dead slabs of a short last tile re-read offset 0 and never store
        // (32-bit compare: see gf_fused_crc)
        const uint64_t left = cell_len - wbyte;
        const uint32_t left32 = left > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(left);
        uint32_t voff[SLABS];
        bool live[SLABS];
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            const uint32_t o = uint32_t(u) * 1024u + uint32_t(lane) * 16u;
            live[u] = o < left32;
            voff[u] = live[u] ? o : 0u;
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
        // `count` cells starting at unit slot `first` of shard_id.  Survivors:
        // compared against the expected sums; rebuilt units: their sums stored.
        auto verify_round = [&](int first, int count) {
            crc.round(
                count, [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                [&](uint32_t sum, uint32_t want) {
                    if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                });
        };
        auto output_round = [&](int first, int count) {
            crc.round(
                count, [] { return 0u; },
                [&](uint32_t sum, uint32_t) { out_sums[sum_cell(first, count) * nck + cbyte / 512] = sum; });
        };
        auto load_in = [&](int i, u32x4(&dst)[SLABS]) {
#pragma unroll
            for (int u = 0; u < SLABS; u++)
                dst[u] = load16<true>(a.in[i] + (uint64_t(stripe) * a.in_stride[i] + wbyte) + voff[u]);
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
            if constexpr (VERIFY_IN) {
#pragma unroll
                for (int u = 0; u < SLABS; u++) crc.put(i % SPR, u, x[u]);
            }
            // opaque per-input table offset threaded through the accumulators:
            // keeps the table reads (and the GF math) of input i from being
            // hoisted next to those of the other inputs
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
                        acc[u][j][d] ^= gf_mul4(tb[j][0], tb[j][1], tb[j][2], tb[j][3], tb[j][4], sl.s0, sl.s1, sl.s2);
                }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (VERIFY_IN) {
                // a round once its SPR survivors are staged, or at the last one
                if (i % SPR == SPR - 1 || i == K - 1) verify_round(i - i % SPR, i % SPR + 1);
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
        // the R rebuilt units: stored (STORE_OUT), staged, their sums written
#pragma unroll
        for (int j = 0; j < R; j++) {
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
                if (STORE_OUT && live[u])
                    store16<true>(a.out[j] + (uint64_t(stripe) * a.out_stride[j] + wbyte) + voff[u], acc[u][j]);
                crc.put(j % SPR, u, acc[u][j]);
            }
            if (j % SPR == SPR - 1 || j == R - 1) output_round(K + j - j % SPR, j % SPR + 1);
        }
    }
}

// SLABS by fused_slabs's rule (ec_fused.hip): 8 slabs per wave while the
// r x 8 accumulators fit (k <= 6, r <= 3), else 4
constexpr int recon_crc_slabs(int k, int r) { return (r <= 3 && k <= 6) ? 8 : 4; }

}  // namespace hec
