// ec_scrub_rows.hip -- verified scrub of short stripes: the last stripe of a
// block group, or every stripe of a batch of small files, holds r < k *
// cell_len logical bytes, so its units have different lengths
// (ec_reconstruct_rows.hpp).  Every present unit counts as its own bytes
// followed by zeros up to n0 = min(cell_len, r): the parity check runs over
// the positions below n0, and each unit is verified against the chunk sums of
// its own bytes.  Nothing is written but flags and the results of dirty
// stripes.
//
// Two kernels, in a translation unit of their own so that the full-stripe
// kernels (ec_scrub_crc.hip, ec_scrub_mixed.hip) keep their machine code.
//
// gf_scrub_crc_rows is gf_scrub_crc (ec_scrub_crc.hip) with the length
// handling of gf_crc_rows, by the rules written in ec_rows_kernel.hpp: same
// tiles, 16-B loads, GF step, checksum rounds (crc_stage.hpp) and locate
// tail, one pass of k + e reads over [0, n0).  Its own:
//   - The unit loop runs over k + e units; an extra is XORed into its row.
//   - An ended unit's loads go to offset 0 of extra 0, which is a parity unit
//     and so holds n0 bytes.
//   - Every unit is staged and verified, every round compares.
//   - The locate tail masks lanes at or past n0 out of the findings.
// The kernel keeps the text of its tile preamble (lengths, cut, load_in,
// product step, verify round): see profiles/rows_parts/README.md.
//
// gf_scrub_rows_bytes is the byte-wise route for every other shape, in the
// style of gf_scrub_mixed_bytes plus gf_reconstruct_rows_bytes' verify lanes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "ec_rows_kernel.hpp"
#include "ec_scrub_rows.hpp"

namespace hec {

// K survivors = the code's k, E extras (= rows of G, parity units all), SLABS
// KiB of every cell per wave-tile, as gf_scrub_crc.
template <int K, int E, int SLABS, int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gf_scrub_crc_rows(
    MatmulArgs a, ScrubCrcArgs cs, ReconRowsLens ln) {
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
    const uint64_t nck = (cell_len + 511) / 512;  // chunk slots per cell in the sums layout
    const uint32_t total = a.total_tiles;
    const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x / 64)), lane = threadIdx.x & 63;
    const int qi = lane & 3, piece = lane >> 3, sir = piece / SLABS, pslab = piece % SLABS, half = (lane >> 2) & 1;
    uint8_t* stage = s_stage + wave * STAGE;
    const uint32_t* exp_sums = reinterpret_cast<const uint32_t*>(cs.expected);
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(cs.results);
    const uint32_t wave_off = uint32_t(wave) * WAVE_BYTES;
    const uint32_t lane16 = uint32_t(lane) * 16u;

    for (uint32_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        uint32_t lstripe, tcol;
        tile_coords(tile, a, lstripe, tcol);
        // The scalar-length scheme of gf_crc_rows (ec_rows_kernel.hpp): the tile's
        // coordinates and the stripe's logical bytes in SGPRs, lengths in 32
        // bits from r / 16 and r % 16 (the launcher keeps cell_len below
        // 2^31; a data unit starts at a multiple of 16).
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
        // re-read offset 0 and are masked out of the findings
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

        // bytes of unit slot `slot` of shard_id that lie at or past the
        // wave's first byte (0: the unit ended before this wave-tile); an
        // extra is a parity unit: n0 bytes
        auto unit_left = [&](int slot) -> uint32_t {
            if (slot >= K) return nleft;
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
        // A verify round over `count` units, left0 / left1 = unit_left of the
        // round's two slots: the lane's chunk is measured against the length
        // of the unit in its slot, so sums slots past a unit's last live chunk
        // are not read.
        auto verify_round = [&](int first, int count, uint32_t left0, uint32_t left1) {
            const uint32_t mine = (SPR > 1 && sir > 0 && count > 1) ? left1 : left0;
            const uint64_t ulen = uint64_t(wbyte) + mine;  // what CrcStage takes for cell_len
            const bool in_cell = coff < mine;
            const bool full = in_cell && mine - coff >= 512u;  // same for a chunk's 4 lanes
            const Stage crc{s_ctabs, stage, kfinal, ulen, lane, qi, sir, cbyte, in_cell, full};
            crc.round(
                count, [&] { return exp_sums[sum_cell(first, count) * nck + cbyte / 512]; },
                [&](uint32_t sum, uint32_t want) {
                    if (sum != want) cs.bad[sum_cell(first, count)] = 1;
                });
        };
        // Every unit issues its SLABS loads, so the loads in flight at any
        // point are a compile-time count and the waits stay exact.  A unit
        // that ended before this wave-tile reads none of its own slot: its
        // loads go to offset 0 of extra 0 and their result is never used.
        // The choice is made with a mask the optimizer cannot see through
        // (as a condition it would be merged with the branch around the GF
        // step and the loads would go back into branches).
        const uint64_t whole_unit = reinterpret_cast<uint64_t>(a.in[K]) + (uint64_t(stripe) * a.in_stride[K] + wbyte);
        auto load_in = [&](int i, u32x4(&dst)[SLABS]) {
            uint32_t here = unit_left(i) != 0 ? 0xFFFFFFFFu : 0u;  // wave-uniform
            asm volatile("" : "+v"(here));
            const uint64_t sel = (uint64_t(here) << 32) | here;
            const uint64_t own = reinterpret_cast<uint64_t>(a.in[i]) + (uint64_t(stripe) * a.in_stride[i] + wbyte);
            const gbyte* p = gptr((own & sel) | (whole_unit & ~sel));
#pragma unroll
            for (int u = 0; u < SLABS; u++) dst[u] = gload16(p + (voff[u] & here));
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
        auto unit_step = [&](auto unit) __attribute__((always_inline)) {
            constexpr int i = decltype(unit)::value;
            if constexpr (PF && i + 1 < N) load_in(i + 1, xn);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t left_i = unit_left(i);
            if (left_i != 0) {  // wave-uniform
                cut(x, left_i);
#pragma unroll
                for (int u = 0; u < SLABS; u++) putter.put(i % SPR, u, x[u]);
                if constexpr (i < K) {
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
            }
            __builtin_amdgcn_sched_barrier(0);
            // a round once its SPR units are staged, or at the last one;
            // skipped when all of them ended before this wave-tile
            if constexpr (i % SPR == SPR - 1 || i == N - 1) {
                constexpr int first = i - i % SPR, count = i % SPR + 1;
                const uint32_t l0 = unit_left(first), l1 = count > 1 ? left_i : 0u;
                if ((l0 | l1) != 0) verify_round(first, count, l0, l1);
            }
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
        // acc = the syndromes; from here gf_scrub_crc's locate tail, with n0
        // where it has cell_len.  One OR-reduce and a ballot: a clean
        // wave-tile ends here (wave-uniform branch; no store, no atomic)
        uint32_t nz = 0;
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            // a lane at or past n0 contributes nothing (it re-read offset 0)
            const uint32_t keep = uint32_t(u) * 1024u + lane16 < nleft ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int j = 0; j < E; j++) nz |= (acc[u][j][0] | acc[u][j][1] | acc[u][j][2] | acc[u][j][3]) & keep;
        }
        if (__builtin_amdgcn_ballot_w64(nz != 0) == 0) continue;
        // this lane's bad byte positions and ruled-out positions of the plan:
        // bit i < K survivor i, bit K + j extra j
        uint32_t cnt = 0, ruled = 0;
        uint32_t anyj[E];  // OR of s_j over this lane's positions
#pragma unroll
        for (int j = 0; j < E; j++) anyj[j] = 0;
#pragma unroll
        for (int u = 0; u < SLABS; u++) {
            const uint32_t keep = uint32_t(u) * 1024u + lane16 < nleft ? 0xFFFFFFFFu : 0u;
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
        // some position
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
            // 1 <= j < e, ORed over the lane's positions; one slab and one
            // survivor at a time
#pragma unroll
            for (int u = 0; u < SLABS; u++) {
#pragma unroll 1
                for (int t = 0; t < K; t++) {
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
                    uint32_t rr = 0;
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const Sel s0 = make_sel(acc[u][0][d]);
#pragma unroll
                        for (int j = 1; j < E; j++) {
                            const Sel sj = make_sel(acc[u][j][d]);
                            rr |= gf_mul4(tb[j][0], tb[j][1], tb[j][2], tb[j][3], tb[j][4], s0.s0, s0.s1, s0.s2) ^
                                  gf_mul4(tb[0][0], tb[0][1], tb[0][2], tb[0][3], tb[0][4], sj.s0, sj.s1, sj.s2);
                        }
                    }
                    ruled |= rr != 0 ? (1u << t) : 0u;
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

// Byte-wise route.  First the parity check (e > 0): one byte position per
// thread, 4 KiB of one stripe per block-tile, positions below n0 only, every
// unit zero from its length on; the full set of 2x2 minors and the block's
// findings combined in LDS, as gf_scrub_mixed_bytes.  Then one lane per
// (stripe, unit, chunk slot) steps the unit's own bytes of that chunk through
// the CRC and compares with the expected sum, as gf_reconstruct_rows_bytes'
// verify lanes: a chunk at or past the unit's length reads neither the slot
// nor the sums.
constexpr uint32_t kRowsByteTile = 4096;  // bytes of a stripe per block-tile
template <int KIND>
__global__ __launch_bounds__(kBlock) void gf_scrub_rows_bytes(ScrubRowsBytesArgs a) {
    __shared__ uint32_t s_crc[256];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[kScrubRowsMaxE * kMaxK];
    __shared__ uint8_t s_syn[kScrubRowsMaxE][kBlock];  // this thread's syndromes at [j][tid]
    __shared__ unsigned long long s_res[2];
    const int tid = threadIdx.x;
    rows_stage_byte_tables<KIND>(s_crc, s_exp, s_log);
    for (int t = tid; t < kScrubRowsMaxE * kMaxK; t += kBlock) s_coef[t] = a.coef[t];
    __syncthreads();
    // clamped: the loops below stay inside the LDS arrays whatever the block holds
    const int k = min(max(a.ns, 0), kMaxK), m = min(max(a.e, 0), kScrubRowsMaxE);
    const uint64_t cell_len = a.cell_len, bpc = a.bytes_per_checksum;
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(a.results);

    if (m > 0) {
        const uint64_t tps = (cell_len + kRowsByteTile - 1) / kRowsByteTile;
        const uint64_t total = tps * a.stripes;
        for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
            const uint64_t s = tile / tps;
            const uint64_t begin = (tile - s * tps) * kRowsByteTile;
            const uint64_t r = rows_stripe_bytes(a.lens, s);
            const uint64_t n0 = r < cell_len ? r : cell_len;
            if (begin >= n0) continue;  // block-uniform: nothing of the tile is read
            const uint64_t stripe = rows_batch_stripe(a.stripe_list, a.lens, s);
            __syncthreads();  // the previous tile's findings are no longer read
            if (tid < 2) s_res[tid] = 0;
            __syncthreads();
            unsigned long long ruled = 0;  // positions of the plan: bit i < k survivor i, bit k + j extra j
            uint32_t cnt = 0;
            for (uint32_t rd = 0; rd < kRowsByteTile / kBlock; rd++) {
                const uint64_t b = begin + rd * uint32_t(kBlock) + uint32_t(tid);
                if (b >= n0) break;
                // an extra is a parity unit: it has a byte at every b < n0
                for (int j = 0; j < m; j++) s_syn[j][tid] = a.in[k + j][stripe * a.in_stride[k + j] + b];
                for (int i = 0; i < k; i++) {
                    if (b >= rows_unit_len(a.id[i], a.data_units, r, n0, cell_len)) continue;  // zero from its length on
                    const uint8_t x = a.in[i][stripe * a.in_stride[i] + b];
                    for (int j = 0; j < m; j++) s_syn[j][tid] ^= lds_gf_mul(s_exp, s_log, s_coef[j * kMaxK + i], x);
                }
                uint8_t any = 0;
                for (int j = 0; j < m; j++) any |= s_syn[j][tid];
                if (any == 0) continue;
                cnt++;
                for (int t = 0; t < k + m; t++) {
                    if ((ruled >> t) & 1) continue;
                    bool out = false;
                    for (int j = 1; j < m && !out; j++) {
                        const uint8_t hj = t < k ? s_coef[j * kMaxK + t] : uint8_t(j == t - k);
                        for (int i = 0; i < j; i++) {
                            const uint8_t hi = t < k ? s_coef[i * kMaxK + t] : uint8_t(i == t - k);
                            if (lds_gf_mul(s_exp, s_log, s_syn[i][tid], hj) != lds_gf_mul(s_exp, s_log, s_syn[j][tid], hi)) {
                                out = true;
                                break;
                            }
                        }
                    }
                    if (out) ruled |= 1ull << t;
                }
            }
            if (cnt != 0) {
                if (ruled != 0) atomicOr(&s_res[0], ruled);
                atomicAdd(&s_res[1], static_cast<unsigned long long>(cnt));
            }
            __syncthreads();
            if (tid == 0 && s_res[1] != 0) {
                unsigned long long units = a.missing;
                for (int i = 0; i < k + m; i++)
                    if ((s_res[0] >> i) & 1) units |= 1ull << (a.id[i] & 63u);
                if (units != 0) atomicOr(results + 2 * stripe, units);
                atomicAdd(results + 2 * stripe + 1, s_res[1]);
            }
        }
    }

    const uint64_t per_stripe = a.nck * uint64_t(k + m);
    const uint64_t items = per_stripe * a.stripes;
    for (uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x; g < items; g += uint64_t(gridDim.x) * kBlock) {
        const uint64_t s = g / per_stripe;
        const uint64_t rest = g - s * per_stripe;
        const int i = int(rest / a.nck);
        const uint64_t chunk = rest - uint64_t(i) * a.nck;
        const uint64_t begin = chunk * bpc;
        const uint64_t r = rows_stripe_bytes(a.lens, s);
        const uint64_t n0 = r < cell_len ? r : cell_len;
        const uint64_t len = rows_unit_len(a.id[i], a.data_units, r, n0, cell_len);
        if (begin >= len) continue;
        const uint64_t stripe = rows_batch_stripe(a.stripe_list, a.lens, s);
        const uint32_t sum = rows_own_chunk_sum<KIND>(s_crc, a.in[i] + stripe * a.in_stride[i], begin, len, bpc);
        const uint64_t cell = stripe * a.n_total + a.id[i];
        if (reinterpret_cast<const uint32_t*>(a.expected)[cell * a.nck + chunk] != sum) a.bad[cell] = 1;
    }
}

namespace {

struct ScrubRowsFn {
    template <int K, int E>
    static const void* fn(int kind) {
        constexpr int SL = scrub_rows_slabs(K, E);
        if (kind == crc::kCrc32c) return reinterpret_cast<const void*>(&gf_scrub_crc_rows<K, E, SL, crc::kCrc32c>);
        return reinterpret_cast<const void*>(&gf_scrub_crc_rows<K, E, SL, crc::kCksum>);
    }
};

}  // namespace

int launch_scrub_crc_rows(const MatmulArgs& a, const ScrubCrcArgs& cs, const ReconRowsLens& lens, int device,
                          hipStream_t stream) {
    if (a.k < 1 || a.k > kMaxK - kMaxR || a.r < 1 || a.r > kMaxR || a.cell_len == 0 || !cs.expected || !cs.bad ||
        !cs.results || cs.n_total == 0)
        return -1;
    if ((reinterpret_cast<uintptr_t>(cs.expected) & 3u) || (reinterpret_cast<uintptr_t>(cs.results) & 7u)) return -1;
    for (int i = 0; i < a.k + a.r; i++)
        if (cs.shard_id[i] >= cs.n_total) return -1;
    for (int i = 0; i < a.k; i++)
        if (a.coef[i] == 0) return -1;  // the minors divide by row 0
    // S is the first k present units and data units have the lowest indices:
    // every extra is a parity unit, n0 bytes long (an ended unit's loads go
    // to extra 0)
    for (int j = 0; j < a.r; j++)
        if (cs.shard_id[a.k + j] < a.k) return -1;
    // grid as launch_scrub_crc
    return launch_rows_crc(pick_kr<ScrubRowsFn>(a.k, a.r, cs.kind), scrub_rows_slabs(a.k, a.r), a, cs, lens, a.k + a.r, 0,
                           cs.stripe_list ? 2 : 4, device, stream);
}

int launch_scrub_rows_bytes(const ScrubRowsBytesArgs& in, int device, hipStream_t stream) {
    ScrubRowsBytesArgs a = in;
    if (a.ns < 0 || a.ns > kMaxK || a.e < 0 || a.e > kScrubRowsMaxE || a.ns + a.e < 1 || !a.expected || !a.bad ||
        (reinterpret_cast<uintptr_t>(a.expected) & 3u) || !rows_bytes_args_ok(a, a.data_units))
        return -1;
    if (a.e > 0 && (!a.results || (reinterpret_cast<uintptr_t>(a.results) & 7u))) return -1;
    for (int i = 0; i < a.ns + a.e; i++)
        if (!a.in[i] || a.id[i] >= a.n_total) return -1;
    for (int j = 0; j < a.e; j++)
        if (a.id[a.ns + j] < a.data_units) return -1;  // an extra is a parity unit
    if (a.stripes == 0) return 0;
    a.nck = rows_nck(a.cell_len, a.bytes_per_checksum);
    const uint64_t tps = (a.cell_len + kRowsByteTile - 1) / kRowsByteTile;
    if (tps > 0xFFFFFFFFFFFFFFFFull / a.stripes) return -1;
    // a block per tile of the parity check where there is one
    return launch_rows_bytes(&gf_scrub_rows_bytes<crc::kCrc32c>, &gf_scrub_rows_bytes<crc::kCksum>, a,
                             a.nck * uint64_t(a.ns + a.e) * a.stripes, a.e > 0 ? tps * a.stripes : 0, device, stream);
}

}  // namespace hec
