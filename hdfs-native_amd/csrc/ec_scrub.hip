// ec_scrub.hip -- stripe scrub for gfx950: are the k+m units of every stripe
// of a batch still consistent with each other, and if not, which unit is
// wrong?  What `hdfs debug verifyEC` and dfs.datanode.ec.reconstruct.validation
// (HDFS-15759) ask on the CPU; the reference's reader trusts the packet
// checksums (connection.rs:477-504) and has no counterpart.
//
// With P = C[k:] the m x k parity block and H = [P | I_m] the parity-check
// matrix, the syndrome of byte position b is
//     s_j(b) = XOR_i P[j][i] * u_i(b)  ^  u_{k+j}(b),   j < m
// -- encode's arithmetic with m loads in place of m stores.  Per stripe the
// kernels return two 64-bit words (hec_scrub_result_t): bad_bytes = positions
// with a non-zero syndrome vector, and ruled_out, bit t set when some
// position's syndrome vector is not a multiple of column t of H (one corrupt
// unit t leaves every syndrome vector proportional to that column).
//
// gf_scrub is the sibling of gf_matmul_v16 (ec_kernels.hip): the same
// wave-tiles of 64 lanes x U 16-B chunks, shapes, tile order, work queue and
// v_perm product tables; the parity chunks are loaded into the accumulators
// the products are XORed into, so a tile holds the registers encode holds.
// A wave whose syndromes are all zero (one OR-reduce and a ballot) goes to
// its next tile: clean data is read once and nothing is written.  A wave
// that sees a non-zero syndrome counts and locates in place and sends one
// atomicOr and one atomicAdd to its stripe's words.  gf_scrub_bytes is the
// plain byte-granular kernel for every other shape: same results.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "gf_device.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"
#include "work_queue.hpp"

namespace hec {

// K data units, M parity units (1..4), U 16-B chunks per lane, BS threads.
// WQ > 0: rounds of wave-tiles per atomic from the launch's counters (a.queue,
// as gf_matmul_v16); WQ == 0: the same wave-tiles in a fixed order (wave w of
// the grid takes tiles w, w + waves, ...), for a launch with no counter set.
// Needs P[0][t] != 0 for every data unit t (the launcher checks): a vector s
// is then a multiple of column t exactly when the m-1 minors
// s_0 * P[j][t] ^ s_j * P[0][t] vanish.
template <int K, int M, int U, int BS, int WQ>
__global__ __launch_bounds__(BS) void gf_scrub(ScrubArgs a) {
    static_assert(K > 0 && M >= 1 && M <= kMaxR, "compile-time k, 1..4 parity units");
    __shared__ PermTable s_tab[M][kMaxK];
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[M * kMaxK];
    {
        static_assert(BS >= 256, "the prologue assumes >= 256 threads");
        const int tid = threadIdx.x;
        if (tid < 256) {
            s_exp[tid] = kDevGf.exp[tid];
            s_exp[tid + 256] = kDevGf.exp[tid + 256];
            s_log[tid] = kDevGf.log[tid];
        }
        if (tid < M * kMaxK) s_coef[tid] = a.coef[tid];
        __syncthreads();
        for (int t = tid; t < M * K; t += BS) {
            const int j = t / K, i = t - j * K;
            build_perm_table(&s_tab[j][i], s_coef[j * kMaxK + i], s_exp, s_log);
        }
        __syncthreads();
    }

    const uint32_t chunks = a.chunks;  // 16-B chunks per cell
    const uint32_t total = a.total_tiles;
    constexpr uint32_t TILE = 64 * U;  // chunks per wave-tile
    const uint32_t lcol = threadIdx.x & 63u;
    MatmulArgs order;  // tile_coords reads the tile-order fields only
    order.tiles_per_stripe = a.tiles_per_stripe;
    order.group = a.group;
    order.grouped_tiles = a.grouped_tiles;
    order.stripes = a.stripes;
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(a.results);

    // the queue of gf_matmul_v16: this wave's counter, its next batch (lane 0,
    // in flight) and the rounds left of the current one
    const uint32_t wq_n = gridDim.x < kMixedQueues ? gridDim.x : kMixedQueues;
    const uint32_t wq_q = blockIdx.x % wq_n;
    uint32_t* const wq_ctr = WQ ? a.queue + wq_q * (kMixedQueueStride / 4) : nullptr;
    if constexpr (WQ > 0) queue_zero_next(a.queue_zero);
    uint32_t wq_next, wq_round = 0, wq_left = 0;
    asm volatile("" : "=v"(wq_next));  // defined in every lane; only lane 0's is read
    auto next_tile = [&]() -> uint32_t {
        for (;;) {
            if (wq_left == 0) {
                const uint32_t v = uint32_t(__builtin_amdgcn_readfirstlane(int(wq_next)));
                wq_round = v * uint32_t(WQ);
                wq_left = WQ;
                if (uint64_t(wq_round) * wq_n + wq_q >= total) return total;  // the wave is done
                if ((threadIdx.x & 63u) == 0) wq_next = atomicAdd(wq_ctr, 1u);
            } else {
                wq_round++;
            }
            wq_left--;
            const uint64_t t = uint64_t(wq_round) * wq_n + wq_q;
            if (t < total) return uint32_t(t);
            wq_left = 0;  // past the end inside a batch: read the fetch behind it
        }
    };
    if constexpr (WQ > 0)
        if ((threadIdx.x & 63u) == 0) wq_next = atomicAdd(wq_ctr, 1u);
    // fixed order: the grid's waves stride over the tiles (the launcher keeps
    // total + the stride below 2^32)
    const uint32_t fx_first = blockIdx.x * uint32_t(BS / 64) + (threadIdx.x >> 6);
    const uint32_t fx_step = gridDim.x * uint32_t(BS / 64);
    for (uint32_t tile = WQ ? next_tile() : fx_first; tile < total; tile = WQ ? next_tile() : tile + fx_step) {
        uint32_t stripe, tcol;
        tile_coords(tile, order, stripe, tcol);
        stripe = uint32_t(__builtin_amdgcn_readfirstlane(int(stripe)));
        tcol = uint32_t(__builtin_amdgcn_readfirstlane(int(tcol)));
        // the table reads stay inside the loop (as gf_matmul_v16)
        asm volatile("" ::: "memory");
        uint32_t offs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t col = tcol * TILE + u * 64u + lcol;
            offs[u] = (col < chunks ? col : 0u) * 16u;  // a lane past the cell re-reads offset 0; masked below
        }
        // every unit's loads for all U chunks before any arithmetic; the
        // stored parity lands in the accumulators
        u32x4 x[U][K];
        u32x4 acc[U][M];
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int i = 0; i < K; i++) x[u][i] = load16<true>((a.base[i] + uint64_t(stripe) * a.stride[i]) + offs[u]);
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < M; j++)
                acc[u][j] = load16<true>((a.base[K + j] + uint64_t(stripe) * a.stride[K + j]) + offs[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < K; i++) {
            // opaque per-input table offset: input i's table reads are not
            // hoisted above this point (M*K*5 VGPRs otherwise)
            uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
            asm volatile("" : "+v"(toff));
            Sel s[U][4];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int d = 0; d < 4; d++) s[u][d] = make_sel(x[u][i][d]);
#pragma unroll
            for (int j = 0; j < M; j++) {
                const PermTable& t =
                    *reinterpret_cast<const PermTable*>(reinterpret_cast<const char*>(&s_tab[j][0]) + toff);
                const uint32_t t0lo = t.t0lo, t0hi = t.t0hi, t1lo = t.t1lo, t1hi = t.t1hi, t2 = t.t2;
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int d = 0; d < 4; d++)
                        acc[u][j][d] ^= gf_mul4(t0lo, t0hi, t1lo, t1hi, t2, s[u][d].s0, s[u][d].s1, s[u][d].s2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // acc = the syndromes.  One OR-reduce and a ballot: a clean wave-tile
        // ends here (wave-uniform branch; no store, no atomic)
        uint32_t nz = 0;
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < M; j++) nz |= acc[u][j][0] | acc[u][j][1] | acc[u][j][2] | acc[u][j][3];
        if (__builtin_amdgcn_ballot_w64(nz != 0) != 0) {
            uint32_t cnt = 0, ruled = 0;  // this lane's bad byte positions and ruled-out units (k+m <= 14)
#pragma unroll
            for (int u = 0; u < U; u++) {
                // a lane past the cell contributes nothing (recomputed: not
                // carried through the multiply in a register)
                const uint32_t keep = tcol * TILE + u * 64u + lcol < chunks ? 0xFFFFFFFFu : 0u;
                uint32_t sy[M][4];
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int d = 0; d < 4; d++) sy[j][d] = acc[u][j][d] & keep;
                uint32_t anyj[M];  // OR of s_j over the chunk
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
                // parity unit k+j0 (column e_j0): ruled out when any other s_j is non-zero
#pragma unroll
                for (int j0 = 0; j0 < M; j0++) {
                    uint32_t other = 0;
#pragma unroll
                    for (int j = 0; j < M; j++)
                        if (j != j0) other |= anyj[j];
                    ruled |= other != 0 ? (1u << (K + j0)) : 0u;
                }
                if constexpr (M > 1) {
                    // data unit t: the packed minors s_0 * P[j][t] ^ s_j * P[0][t], j >= 1
                    Sel sl[M][4];
#pragma unroll
                    for (int j = 0; j < M; j++)
#pragma unroll
                        for (int d = 0; d < 4; d++) sl[j][d] = make_sel(sy[j][d]);
#pragma unroll 1
                    for (int t = 0; t < K; t++) {
                        const PermTable& p0 = s_tab[0][t];
                        const uint32_t a0lo = p0.t0lo, a0hi = p0.t0hi, a1lo = p0.t1lo, a1hi = p0.t1hi, a2 = p0.t2;
                        uint32_t r = 0;
#pragma unroll
                        for (int j = 1; j < M; j++) {
                            const PermTable& pj = s_tab[j][t];
                            const uint32_t b0lo = pj.t0lo, b0hi = pj.t0hi, b1lo = pj.t1lo, b1hi = pj.t1hi, b2 = pj.t2;
#pragma unroll
                            for (int d = 0; d < 4; d++)
                                r |= gf_mul4(b0lo, b0hi, b1lo, b1hi, b2, sl[0][d].s0, sl[0][d].s1, sl[0][d].s2) ^
                                     gf_mul4(a0lo, a0hi, a1lo, a1hi, a2, sl[j][d].s0, sl[j][d].s1, sl[j][d].s2);
                        }
                        ruled |= r != 0 ? (1u << t) : 0u;
                    }
                }
            }
            // over the wave, then one lane's plain atomics into the stripe's words
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                cnt += uint32_t(__shfl_xor(int(cnt), off, 64));
                ruled |= uint32_t(__shfl_xor(int(ruled), off, 64));
            }
            if (lcol == 0 && cnt != 0) {
                if (ruled != 0) atomicOr(results + 2 * uint64_t(stripe), static_cast<unsigned long long>(ruled));
                atomicAdd(results + 2 * uint64_t(stripe) + 1, static_cast<unsigned long long>(cnt));
            }
        }
        // the drain knob of gf_matmul_v16 (tune key 6); a clean tile has
        // nothing of its own in flight here
        if (a.drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// Every other shape: any k + m <= kMaxShards, m <= 16, any alignment and
// cell_len.  One thread per byte position, 16 positions per thread and
// 4 KiB of one stripe per block-tile; LDS log/antilog products; the full set
// of 2x2 minors s_i * H[j][t] ^ s_j * H[i][t]; the block's findings are
// combined in LDS and sent as one atomicOr and one atomicAdd.
constexpr int kScrubMaxM = 16;       // HEC_MAX_PARITY_UNITS
constexpr uint32_t kByteTile = 4096;  // bytes of a stripe per block-tile
__global__ __launch_bounds__(256) void gf_scrub_bytes(ScrubArgs a) {
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[kScrubMaxM * kMaxK];
    __shared__ uint8_t s_syn[kScrubMaxM][256];  // this thread's syndromes at [j][tid]
    __shared__ unsigned long long s_res[2];
    const int tid = threadIdx.x;
    const int k = a.k, m = a.m;
    s_exp[tid] = kDevGf.exp[tid];
    s_exp[tid + 256] = kDevGf.exp[tid + 256];
    s_log[tid] = kDevGf.log[tid];
    for (int t = tid; t < m * kMaxK; t += 256) s_coef[t] = a.coef[t];
    __syncthreads();
    unsigned long long* const results = reinterpret_cast<unsigned long long*>(a.results);
    const uint64_t tps = (a.cell_len + kByteTile - 1) / kByteTile;
    const uint64_t total = tps * a.stripes;
    for (uint64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const uint64_t stripe = tile / tps;
        const uint64_t begin = (tile - stripe * tps) * kByteTile;
        if (tid < 2) s_res[tid] = 0;
        __syncthreads();
        unsigned long long ruled = 0;
        uint32_t cnt = 0;
        for (uint32_t r = 0; r < kByteTile / 256; r++) {
            const uint64_t b = begin + r * 256u + uint32_t(tid);
            if (b >= a.cell_len) break;
            for (int j = 0; j < m; j++) s_syn[j][tid] = a.base[k + j][stripe * a.stride[k + j] + b];
            for (int i = 0; i < k; i++) {
                const uint8_t x = a.base[i][stripe * a.stride[i] + b];
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
            if (s_res[0] != 0) atomicOr(results + 2 * stripe, s_res[0]);
            atomicAdd(results + 2 * stripe + 1, s_res[1]);
        }
        __syncthreads();
    }
}

namespace {

// The shapes and the rounds per atomic of gf_matmul_v16 (default_shape,
// default_wq in ec_kernels.hip): U = 4 in 256-thread blocks up to k = 6 (two
// rounds of wave-tiles per atomic for k = 2, 3; one for k = 6), U = 2 in
// 512-thread blocks and one round for k = 10.
struct ScrubFn {
    template <int K, int M>
    static const void* fn(bool wq) {
        if constexpr (K > 6)
            return wq ? reinterpret_cast<const void*>(&gf_scrub<K, M, 2, 512, 1>)
                      : reinterpret_cast<const void*>(&gf_scrub<K, M, 2, 512, 0>);
        else if constexpr (K == 6)
            return wq ? reinterpret_cast<const void*>(&gf_scrub<K, M, 4, 256, 1>)
                      : reinterpret_cast<const void*>(&gf_scrub<K, M, 4, 256, 0>);
        else
            return wq ? reinterpret_cast<const void*>(&gf_scrub<K, M, 4, 256, 2>)
                      : reinterpret_cast<const void*>(&gf_scrub<K, M, 4, 256, 0>);
    }
};

}  // namespace

int launch_scrub(const ScrubArgs& in, int device, hipStream_t stream) {
    ScrubArgs a = in;
    if (a.k < 1 || a.k > kMaxK || a.m < 1 || a.m > kScrubMaxM || a.k + a.m > kMaxShards || a.cell_len == 0 ||
        !a.results)
        return -1;
    if (a.stripes == 0) return 0;
    const Tune tn = tune_snapshot();
    const int cus = num_cus(device);
    bool fast = (a.k == 2 || a.k == 3 || a.k == 6 || a.k == 10) && a.m <= kMaxR && a.cell_len % 16 == 0 &&
                a.cell_len < (uint64_t(1) << 32) && a.stripes <= 0xFFFFFFFFull;
    for (int i = 0; fast && i < a.k + a.m; i++)
        fast = ((reinterpret_cast<uintptr_t>(a.base[i]) | a.stride[i]) & 15u) == 0;
    // the fast kernel's minors pivot on P[0][t]; true for the shipped codecs
    // at these shapes, checked here for any matrix
    for (int t = 0; fast && t < a.k; t++) fast = a.coef[t] != 0;
    // tile indices (+ the fixed order's stride) in 32 bits
    if (fast && !tile_geometry(a, 1024u * wave_tile_u(a.k), 0xFFF00000ull)) fast = false;
    if (fast) {
        QueueLease lease = queue_lease(device, stream);  // empty: the fixed order
        a.queue = lease.use;
        a.queue_zero = lease.zero;
        const void* fn = pick_kr<ScrubFn>(a.k, a.m, bool(lease));
        if (!fn) return -1;
        set_tile_order(a, tn, 4u);
        a.drain = tn.drain == 1 ? 0u : 1u;
        // the queue: resident blocks only, each one drains it; the fixed
        // order: gf_matmul_v16's grids (8 blocks per CU for k = 10)
        const int bpc = tn.blocks_per_cu ? tn.blocks_per_cu : (lease || a.k <= 6) ? 1 : 8;
        uint64_t grid = tn.grid ? uint64_t(tn.grid) : uint64_t(cus) * bpc;
        if (grid > a.total_tiles) grid = a.total_tiles;
        if (grid > 0xFFFFull) grid = 0xFFFF;
        void* args[] = {&a};
        const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(wave_tile_bs(a.k)), args, 0, stream);
        if (e != hipSuccess) return int(e);
        lease.launched();
        return 0;
    }
    const uint64_t btps = (a.cell_len + kByteTile - 1) / kByteTile;
    if (btps > 0xFFFFFFFFFFFFFFFFull / a.stripes) return -1;
    const uint64_t total = btps * a.stripes;
    uint64_t grid = uint64_t(cus) * 8;
    if (grid > total) grid = total;
    void* args[] = {&a};
    const hipError_t e =
        hipLaunchKernel(reinterpret_cast<const void*>(&gf_scrub_bytes), dim3(uint32_t(grid)), dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
