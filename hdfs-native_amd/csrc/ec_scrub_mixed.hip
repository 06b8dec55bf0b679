// ec_scrub_mixed.hip -- degraded scrub for gfx950: every stripe of a batch has
// its own presence mask, as a repair worker sees a block group after a
// DataNode died.  Are the units a stripe still has consistent with each other,
// and if not, which one is wrong?  (dfs.datanode.ec.reconstruct.validation,
// HDFS-15759, before the rebuild instead of after it.)
//
// Per stripe: S = the first k present units (the survivors every other call
// of the engine picks), E = the other present units, e = |E|.  With
// G = C[E] . inverse(C[S]) (e x k, built on the host: the rows
// hec_reconstruct_plan returns for present = S, want = E) the syndrome of byte
// position b is
//     s_j(b) = XOR_i G[j][i] * u_{S_i}(b)  ^  u_{E_j}(b),   j < e
// and the parity-check column of survivor S_i is G[:, i], of extra E_j the unit
// vector e_j.  Results as ec_scrub.hip (bad_bytes, ruled_out), with the bit of
// every missing unit set in ruled_out once a stripe has a bad position.  With
// every unit present this is ec_scrub.hip's arithmetic on G = P.
//
// gf_scrub_mixed joins the metadata side of gf_reconstruct_mixed
// (ec_reconstruct.hip: per-stripe plan offsets and plans resident in dynamic
// LDS, three dependent LDS round trips per tile, wave-uniform bases, rows past
// the stripe's e skipped by a scalar branch, launch counters in the workspace)
// to the body of gf_scrub (ec_scrub.hip: the extras loaded into the
// accumulators, one OR-reduce and a ballot, a clean wave-tile writes nothing).
// gf_scrub_mixed_bytes is the byte-granular sibling of gf_scrub_bytes for
// every other shape: same results.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
// the plans arrive with their product tables built (host side)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "gf_device.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

// K survivors, M = the batch's largest e (1..4), U 16-B chunks per lane, BS
// threads.  WQ > 0: rounds of wave-tiles per atomic from the launch's counters
// (a.queue, zeroed by the workspace upload); WQ == 0: the same wave-tiles in a
// fixed order (wave w of the grid takes tiles w, w + waves, ...), for the
// uniform-plan launches, which have no counters of their own.
// a.stripe_off == nullptr is the uniform plan: the one plan at a.plans is
// resident and every stripe of the launch uses it.
// Needs G[0][i] != 0 for every survivor i (the host checks every plan): a
// vector s is then a multiple of column i exactly when the e-1 minors
// s_0 * G[j][i] ^ s_j * G[0][i] vanish.
template <int K, int M, int U, int BS, int WQ>
__global__ __launch_bounds__(BS) void gf_scrub_mixed(ScrubMixedArgs a) {
    static_assert(K > 0 && M >= 1 && M <= kMaxR, "compile-time k, 1..4 checks");
    __shared__ uint64_t s_base[kMaxShards], s_stride[kMaxShards];
    // [stripe plan offsets: u32 x stripes, 16-B padded][plan blob]; uniform: [the plan]
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const int tid = threadIdx.x;
    if (tid < kMaxShards) {
        s_base[tid] = reinterpret_cast<uint64_t>(a.base[tid]);
        s_stride[tid] = a.stride[tid];
    }
    const bool uniform = a.stripe_off == nullptr;
    const uint32_t off_bytes = uniform ? 0u : ((uint32_t(a.stripes) * 4u + 15u) & ~15u);
    {
        const uint32_t off_words = uniform ? 0u : uint32_t(a.stripes);
        for (uint32_t t = tid; t < off_words; t += BS) reinterpret_cast<uint32_t*>(s_dyn)[t] = a.stripe_off[t];
        const uint32_t words = a.blob_bytes / 4;
        for (uint32_t t = tid; t < words; t += BS)
            reinterpret_cast<uint32_t*>(s_dyn + off_bytes)[t] = reinterpret_cast<const uint32_t*>(a.plans)[t];
    }
    __syncthreads();
    const uint32_t chunks = a.chunks;
    const uint32_t total = a.total_tiles;
    constexpr uint32_t TILE = 64 * U;  // chunks per wave-tile
    const uint32_t lcol = threadIdx.x & 63u;
    MatmulArgs order;  // tile_coords reads the tile-order fields only
    order.tiles_per_stripe = a.tiles_per_stripe;
    order.group = a.group;
    order.grouped_tiles = a.grouped_tiles;
    order.stripes = a.stripes;
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(a.results);

    auto run_tile = [&](uint32_t tile) {
        uint32_t stripe, tcol;
        tile_coords(tile, order, stripe, tcol);
        stripe = uint32_t(__builtin_amdgcn_readfirstlane(int(stripe)));
        tcol = uint32_t(__builtin_amdgcn_readfirstlane(int(tcol)));
        uint32_t off = 0;
        if (!uniform) {
            off = uint32_t(__builtin_amdgcn_readfirstlane(int(reinterpret_cast<const uint32_t*>(s_dyn)[stripe])));
            if (off == kNoPlan) return;  // e == 0: nothing of the stripe is read
        }
        // row j, survivor i at tabs[j * K + i]
        const PermTable* tabs = reinterpret_cast<const PermTable*>(s_dyn + off_bytes + off + sizeof(ScrubPlanHeader));
        // The tile's metadata in three dependent LDS round trips, as
        // gf_reconstruct_mixed: the plan offset, the header words (e, survivor
        // and extra bytes, missing mask), every read unit's base / stride.
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(s_dyn + off_bytes + off);
        constexpr int SW = (K + 3) / 4;  // words of survivor bytes (surv[] at byte 4)
        uint32_t w_surv[SW];
        const uint32_t w_e = hw[0];
        const uint32_t w_ext = hw[9];  // extras[] at byte 36: M <= 4 bytes
        const uint32_t w_mlo = hw[13], w_mhi = hw[14];
#pragma unroll
        for (int t = 0; t < SW; t++) w_surv[t] = hw[1 + t];
        uint64_t v_base[K + M], v_stride[K + M];
#pragma unroll
        for (int i = 0; i < K; i++) {
            const uint32_t sh = min((w_surv[i / 4] >> (8 * (i % 4))) & 0xFFu, uint32_t(kMaxShards - 1));
            v_base[i] = s_base[sh];
            v_stride[i] = s_stride[sh];
        }
#pragma unroll
        for (int j = 0; j < M; j++) {
            // rows past e hold 0 (any byte is clamped into the table): a valid
            // slot, never loaded
            const uint32_t sh = min((w_ext >> (8 * j)) & 0xFFu, uint32_t(kMaxShards - 1));
            v_base[K + j] = s_base[sh];
            v_stride[K + j] = s_stride[sh];
        }
        // all of it read before the row-count branches below
        uint32_t w_e2 = w_e;
#pragma unroll
        for (int i = 0; i < K + M; i++) asm volatile("" : "+v"(v_base[i]), "+v"(v_stride[i]), "+v"(w_e2));
        const int ne = int(__builtin_amdgcn_readfirstlane(int(w_e2)));  // this stripe's checks, 1..M
        asm volatile("" ::: "memory");

        uint32_t offs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t col = tcol * TILE + u * 64u + lcol;
            offs[u] = (col < chunks ? col : 0u) * 16u;  // a lane past the cell re-reads offset 0; masked below
        }
        // every unit's loads for all U chunks before any arithmetic; the
        // extras land in the accumulators (rows past e: zero, never touched).
        // The extras go first: their loads sit behind the row-count branches,
        // and hipcc's wait counts at the join assume the shortest path, so
        // with the survivors first the first product waited for every load
        u32x4 x[U][K];
        u32x4 acc[U][M];
#pragma unroll
        for (int j = 0; j < M; j++) {
            if (j == 0 || j < ne) {  // wave-uniform
                const gbyte* eb = gptr(uniform64(v_base[K + j]) + uint64_t(stripe) * uniform64(v_stride[K + j]));
#pragma unroll
                for (int u = 0; u < U; u++) acc[u][j] = gload16(eb + offs[u]);
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) acc[u][j] = u32x4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int i = 0; i < K; i++) {
            const gbyte* ib = gptr(uniform64(v_base[i]) + uint64_t(stripe) * uniform64(v_stride[i]));
#pragma unroll
            for (int u = 0; u < U; u++) x[u][i] = gload16(ib + offs[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < K; i++) {
            // opaque per-input table offset: input i's table reads are not
            // hoisted above this point (as gf_scrub)
            uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
            asm volatile("" : "+v"(toff));
            // the accumulators stay where they are from one input to the next
            // (as gf_reconstruct_mixed): without this the row-count branches
            // below let hipcc interleave the inputs and spill (k = 10) or
            // park the tile in AGPRs (k = 6)
            if (i > 0) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int j = 0; j < M; j++) asm volatile("" : "+v"(acc[u][j]) : "v"(toff));
            }
            Sel s[U][4];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int d = 0; d < 4; d++) s[u][d] = make_sel(x[u][i][d]);
#pragma unroll
            for (int j = 0; j < M; j++) {
                // rows past the plan's e are skipped (ne is wave-uniform: a
                // scalar branch); their accumulators stay zero
                if (j > 0 && j >= ne) break;
                const PermTable& t =
                    *reinterpret_cast<const PermTable*>(reinterpret_cast<const char*>(tabs + j * K) + toff);
                const uint32_t t0lo = t.t0lo, t0hi = t.t0hi, t1lo = t.t1lo, t1hi = t.t1hi, t2 = t.t2;
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int d = 0; d < 4; d++)
                        acc[u][j][d] ^= gf_mul4(t0lo, t0hi, t1lo, t1hi, t2, s[u][d].s0, s[u][d].s1, s[u][d].s2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < M; j++) asm volatile("" : "+v"(acc[u][j]));
        // acc = the syndromes.  One OR-reduce and a ballot: a clean wave-tile
        // ends here (wave-uniform branch; no store, no atomic)
        uint32_t nz = 0;
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < M; j++) nz |= acc[u][j][0] | acc[u][j][1] | acc[u][j][2] | acc[u][j][3];
        if (__builtin_amdgcn_ballot_w64(nz != 0) != 0) {
            // this lane's bad byte positions and ruled-out positions of the
            // plan: bit i < K survivor i, bit K + j extra j
            uint32_t cnt = 0, ruled = 0;
#pragma unroll
            for (int u = 0; u < U; u++) {
                // a lane past the cell contributes nothing
                const uint32_t keep = tcol * TILE + u * 64u + lcol < chunks ? 0xFFFFFFFFu : 0u;
                uint32_t sy[M][4];
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int d = 0; d < 4; d++) sy[j][d] = acc[u][j][d] & keep;
                uint32_t anyj[M];  // OR of s_j over the chunk (0 for rows past e)
#pragma unroll
                for (int j = 0; j < M; j++) anyj[j] = sy[j][0] | sy[j][1] | sy[j][2] | sy[j][3];
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    uint32_t b = 0;
#pragma unroll
                    for (int j = 0; j < M; j++) b |= sy[j][d];
                    // bit 0 of every byte = the byte is non-zero
                    b |= b >> 4;
                    b |= b >> 2;
                    b |= b >> 1;
                    cnt += uint32_t(__builtin_popcount(b & 0x01010101u));
                }
                // extra j0 (column e_j0): ruled out when any other s_j is
                // non-zero; rows past e have no unit (masked when mapped)
#pragma unroll
                for (int j0 = 0; j0 < M; j0++) {
                    uint32_t other = 0;
#pragma unroll
                    for (int j = 0; j < M; j++)
                        if (j != j0) other |= anyj[j];
                    ruled |= other != 0 ? (1u << (K + j0)) : 0u;
                }
                if constexpr (M > 1) {
                    if (ne > 1) {
                        // survivor i: the packed minors s_0 * G[j][i] ^ s_j * G[0][i], 1 <= j < e
                        Sel sl[M][4];
#pragma unroll
                        for (int j = 0; j < M; j++)
#pragma unroll
                            for (int d = 0; d < 4; d++) sl[j][d] = make_sel(sy[j][d]);
#pragma unroll 1
                        for (int t = 0; t < K; t++) {
                            const PermTable& p0 = tabs[t];
                            const uint32_t a0lo = p0.t0lo, a0hi = p0.t0hi, a1lo = p0.t1lo, a1hi = p0.t1hi, a2 = p0.t2;
                            uint32_t r = 0;
#pragma unroll
                            for (int j = 1; j < M; j++) {
                                if (j >= ne) break;  // wave-uniform: no table past the plan's e
                                const PermTable& pj = tabs[j * K + t];
                                const uint32_t b0lo = pj.t0lo, b0hi = pj.t0hi, b1lo = pj.t1lo, b1hi = pj.t1hi,
                                               b2 = pj.t2;
#pragma unroll
                                for (int d = 0; d < 4; d++)
                                    r |= gf_mul4(b0lo, b0hi, b1lo, b1hi, b2, sl[0][d].s0, sl[0][d].s1, sl[0][d].s2) ^
                                         gf_mul4(a0lo, a0hi, a1lo, a1hi, a2, sl[j][d].s0, sl[j][d].s1, sl[j][d].s2);
                            }
                            ruled |= r != 0 ? (1u << t) : 0u;
                        }
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
            if (lcol == 0 && cnt != 0) {
                unsigned long long units = (static_cast<unsigned long long>(w_mhi) << 32) | w_mlo;
#pragma unroll
                for (int i = 0; i < K; i++)
                    if ((ruled >> i) & 1u) units |= 1ull << ((w_surv[i / 4] >> (8 * (i % 4))) & 63u);
#pragma unroll
                for (int j = 0; j < M; j++)
                    if (j < ne && ((ruled >> (K + j)) & 1u)) units |= 1ull << ((w_ext >> (8 * j)) & 63u);
                if (units != 0) atomicOr(results + 2 * uint64_t(stripe), units);
                atomicAdd(results + 2 * uint64_t(stripe) + 1, static_cast<unsigned long long>(cnt));
            }
        }
        // the drain knob of gf_matmul_v16 (tune key 6); a clean tile has
        // nothing of its own in flight here
        if (a.drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    if constexpr (WQ > 0) {
        // the queue of gf_reconstruct_mixed: lane 0 holds the next batch index;
        // the other lanes' copies are never read (readfirstlane)
        const uint32_t nq = gridDim.x < kMixedQueues ? gridDim.x : kMixedQueues;  // every tile has a block
        const uint32_t q = blockIdx.x % nq;
        uint32_t* ctr = a.queue + q * (kMixedQueueStride / 4);
        uint32_t v_next;
        asm volatile("" : "=v"(v_next));  // defined, unread outside lane 0: no merge with the atomic's result
        if ((threadIdx.x & 63u) == 0) v_next = atomicAdd(ctr, 1u);
        for (;;) {
            const uint32_t r0 = uint32_t(__builtin_amdgcn_readfirstlane(int(v_next))) * uint32_t(WQ);
            if (uint64_t(r0) * nq + q >= total) break;  // 64-bit: no wrap past 2^32 tiles
            if ((threadIdx.x & 63u) == 0) v_next = atomicAdd(ctr, 1u);
            for (uint32_t r = r0; r < r0 + uint32_t(WQ); r++) {
                if (uint64_t(r) * nq + q >= total) break;
                run_tile(r * nq + q);
            }
        }
    } else {
        // fixed order: the grid's waves stride over the tiles (the launcher
        // keeps total + the stride below 2^32)
        const uint32_t fx_first = blockIdx.x * uint32_t(BS / 64) + (threadIdx.x >> 6);
        const uint32_t fx_step = gridDim.x * uint32_t(BS / 64);
        for (uint32_t tile = fx_first; tile < total; tile += fx_step) run_tile(tile);
    }
}

// Every other shape: any k <= kMaxK and e <= 16, any alignment and cell_len.
// The body of gf_scrub_bytes (one byte position per thread, 4 KiB of one
// stripe per block-tile, the full set of 2x2 minors, the block's findings
// combined in LDS); the stripe's header and coefficient bytes (row j, survivor
// i at j*k + i) are fetched per block-tile from the blob in global memory.
constexpr int kScrubMixedMaxE = 16;        // HEC_MAX_PARITY_UNITS
constexpr uint32_t kMixedByteTile = 4096;  // bytes of a stripe per block-tile
__global__ __launch_bounds__(256) void gf_scrub_mixed_bytes(ScrubMixedArgs a) {
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_hdr[sizeof(ScrubPlanHeader) / 4];
    __shared__ uint8_t s_coef[kScrubMixedMaxE * kMaxK];
    __shared__ uint8_t s_syn[kScrubMixedMaxE][256];  // this thread's syndromes at [j][tid]
    __shared__ unsigned long long s_res[2];
    const int tid = threadIdx.x;
    const int k = a.k;
    s_exp[tid] = kDevGf.exp[tid];
    s_exp[tid + 256] = kDevGf.exp[tid + 256];
    s_log[tid] = kDevGf.log[tid];
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(a.results);
    const ScrubPlanHeader* const hdr = reinterpret_cast<const ScrubPlanHeader*>(s_hdr);
    const uint64_t tps = (a.cell_len + kMixedByteTile - 1) / kMixedByteTile;
    const uint64_t total = tps * a.stripes;
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const uint64_t stripe = tile / tps;
        const uint64_t begin = (tile - stripe * tps) * kMixedByteTile;
        const uint32_t off = a.stripe_off ? a.stripe_off[stripe] : 0u;
        if (off == kNoPlan) continue;  // block-uniform: nothing of the stripe is read
        const uint8_t* const blob = a.plans + off;
        // clamped: the loops below stay inside the LDS arrays whatever the blob holds
        const int m = min(int(reinterpret_cast<const uint32_t*>(blob)[0]), kScrubMixedMaxE);
        __syncthreads();  // the previous tile's header and coefficients are no longer read
        if (tid < int(sizeof(ScrubPlanHeader) / 4)) s_hdr[tid] = reinterpret_cast<const uint32_t*>(blob)[tid];
        for (int t = tid; t < m * k; t += 256) s_coef[t] = blob[sizeof(ScrubPlanHeader) + t];
        if (tid < 2) s_res[tid] = 0;
        __syncthreads();
        unsigned long long ruled = 0;  // positions of the plan: bit i < k survivor i, bit k + j extra j
        uint32_t cnt = 0;
        for (uint32_t r = 0; r < kMixedByteTile / 256; r++) {
            const uint64_t b = begin + r * 256u + uint32_t(tid);
            if (b >= a.cell_len) break;
            for (int j = 0; j < m; j++) {
                const uint32_t u = min(uint32_t(hdr->extras[j]), uint32_t(kMaxShards - 1));
                s_syn[j][tid] = a.base[u][stripe * a.stride[u] + b];
            }
            for (int i = 0; i < k; i++) {
                const uint32_t u = min(uint32_t(hdr->surv[i]), uint32_t(kMaxShards - 1));
                const uint8_t x = a.base[u][stripe * a.stride[u] + b];
                for (int j = 0; j < m; j++) s_syn[j][tid] ^= lds_gf_mul(s_exp, s_log, s_coef[j * k + i], x);
            }
            uint8_t any = 0;
            for (int j = 0; j < m; j++) any |= s_syn[j][tid];
            if (any == 0) continue;
            cnt++;
            for (int t = 0; t < k + m; t++) {
                if ((ruled >> t) & 1) continue;
                bool out = false;
                for (int j = 1; j < m && !out; j++) {
                    const uint8_t hj = t < k ? s_coef[j * k + t] : uint8_t(j == t - k);
                    for (int i = 0; i < j; i++) {
                        const uint8_t hi = t < k ? s_coef[i * k + t] : uint8_t(i == t - k);
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
            // the plan's positions as unit indices, and the missing units
            unsigned long long units = (static_cast<unsigned long long>(hdr->missing_hi) << 32) | hdr->missing_lo;
            for (int i = 0; i < k; i++)
                if ((s_res[0] >> i) & 1) units |= 1ull << (hdr->surv[i] & 63u);
            for (int j = 0; j < m; j++)
                if ((s_res[0] >> (k + j)) & 1) units |= 1ull << (hdr->extras[j] & 63u);
            if (units != 0) atomicOr(results + 2 * stripe, units);
            atomicAdd(results + 2 * stripe + 1, s_res[1]);
        }
    }
}

namespace {

// Shapes of gf_reconstruct_mixed: U = 4 chunks per lane in 256-thread blocks
// up to k = 6, U = 2 in 512-thread blocks above; one round of wave-tiles per
// atomic for k >= 6, four below.
struct ScrubMixedFn {
    template <int K, int M>
    static const void* fn(bool wq) {
        if constexpr (K > 6)
            return wq ? reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 2, 512, 1>)
                      : reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 2, 512, 0>);
        else if constexpr (K == 6)
            return wq ? reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 4, 256, 1>)
                      : reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 4, 256, 0>);
        else
            return wq ? reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 4, 256, 4>)
                      : reinterpret_cast<const void*>(&gf_scrub_mixed<K, M, 4, 256, 0>);
    }
};

}  // namespace

int launch_scrub_mixed(const ScrubMixedArgs& in, int max_e, int device, hipStream_t stream) {
    ScrubMixedArgs a = in;
    const bool uniform = a.stripe_off == nullptr;
    // lane offsets into a cell are 32-bit: cells of 4 GiB or more are not for this kernel
    if (a.cell_len == 0 || a.cell_len % 16 != 0 || a.cell_len > 0xFFFFFFFFull || a.stripes > 0xFFFFFFFFull ||
        !a.results || !a.plans || (!uniform && !a.queue))
        return -1;
    if (a.stripes == 0) return 0;
    if (!mixed_resident(uniform ? 0 : a.stripes, a.blob_bytes)) return -1;
    const uint64_t dyn = resident_lds_bytes(uniform ? 0 : a.stripes, a.blob_bytes);
    const void* fn = pick_kr<ScrubMixedFn>(a.k, max_e, !uniform);
    if (!fn || !set_resident_lds_attr(fn, dyn)) return -1;
    const Tune tn = tune_snapshot();
    // tile indices (+ the fixed order's stride) in 32 bits
    if (!tile_geometry(a, 1024u * wave_tile_u(a.k), 0xFFF00000ull)) return -1;
    const uint64_t total = a.total_tiles;
    set_tile_order(a, tn, 4u);
    a.drain = tn.drain == 1 ? 0u : 1u;
    if (uniform) a.queue = nullptr;
    // one block per CU: the resident plans are staged once per block
    uint64_t grid = uint64_t(num_cus(device)) * (tn.blocks_per_cu ? tn.blocks_per_cu : 1);
    if (grid > total) grid = total;
    if (grid > 0xFFFFull) grid = 0xFFFF;
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(wave_tile_bs(a.k)), args, uint32_t(dyn), stream);
    return e == hipSuccess ? 0 : int(e);
}

int launch_scrub_mixed_bytes(const ScrubMixedArgs& a, int device, hipStream_t stream) {
    if (a.k < 1 || a.k > kMaxK || a.cell_len == 0 || !a.results || !a.plans) return -1;
    if (a.stripes == 0) return 0;
    const uint64_t btps = (a.cell_len + kMixedByteTile - 1) / kMixedByteTile;
    if (btps > 0xFFFFFFFFFFFFFFFFull / a.stripes) return -1;
    const uint64_t total = btps * a.stripes;
    uint64_t grid = uint64_t(num_cus(device)) * 8;
    if (grid > total) grid = total;
    ScrubMixedArgs b = a;
    void* args[] = {&b};
    const hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&gf_scrub_mixed_bytes), dim3(uint32_t(grid)),
                                         dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
