// ec_scrub_correct.hip -- scrub correction for gfx950: fix the unit a scrub
// located, in place, from the scrub's own results (hec_scrub_correct_device).
//
// With P, H = [P | I_m] and the syndromes s_j(b) of ec_scrub.hip: one corrupt
// unit t with error e(b) leaves s_j(b) = H[j][t] * e(b) for every row j, so
// any row with H[j][t] != 0 gives the error back as one product,
//     e(b) = scale[t] * s_row[t](b),   scale[t] = 1 / H[row[t]][t].
// For a data unit row[t] is the first j with P[j][t] != 0; for parity unit
// k + j0 it is j0 with scale 1, which overwrites the cell by row j0 of the
// encode.  The host fills row[] and scale[]; there is no inverse, no plan and
// no workspace, and only one syndrome row is ever computed.
//
// Distribution: dirty stripes are rare and not known to the host.  Every wave
// scans the results array, one stripe (16 B) per lane (L2 hits after the first
// block), forms the verdict of hec_scrub_verdict per lane and
// ballots the LOCATED lanes.  All waves walk the located stripes in the same
// order and deal their wave-tiles round-robin over the waves of the grid (the
// running tile count `rot` is the same in every wave), so one dirty stripe is
// spread over the whole grid and many small ones do not pile up on wave 0.
// A clean or unlocated stripe costs no cell read.  Wave 0 of the block with
// stripe % gridDim.x == blockIdx.x writes d_units[stripe]: once per stripe.
//
// gf_scrub_correct is the register kernel (the wave-tiles, shapes and v_perm
// product tables of gf_scrub); gf_scrub_correct_bytes is the byte-granular
// kernel for every other shape: same results.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "gf_device.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

namespace {

// hec_scrub_verdict on the device: the located unit, kCorrectClean or
// kCorrectUnlocated.  units = k + m <= kMaxShards < 64.
__device__ __forceinline__ int32_t correct_verdict(uint64_t ruled_out, uint64_t bad_bytes, int units) {
    if (bad_bytes == 0) return kCorrectClean;
    const uint64_t cand = ~ruled_out & ((uint64_t(1) << units) - 1);
    if (__builtin_popcountll(cand) != 1) return kCorrectUnlocated;
    return int32_t(__builtin_ctzll(cand));
}

}  // namespace

// K data units, U 16-B chunks per lane, BS threads; m, the located unit and its
// row are wave-uniform run-time values.
template <int K, int U, int BS>
__global__ __launch_bounds__(BS) void gf_scrub_correct(ScrubCorrectArgs a) {
    static_assert(K > 0 && K <= kMaxK, "compile-time k");
    __shared__ PermTable s_tab[kMaxR * K];  // row j, input i at j * K + i
    __shared__ PermTable s_scl[K];          // scale[t], t < K
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[kMaxR * kMaxK];
    const int m = a.m;  // 1 .. kMaxR (the launcher checks)
    {
        static_assert(BS >= 256, "the prologue assumes >= 256 threads");
        const int tid = threadIdx.x;
        if (tid < 256) {
            s_exp[tid] = kDevGf.exp[tid];
            s_exp[tid + 256] = kDevGf.exp[tid + 256];
            s_log[tid] = kDevGf.log[tid];
        }
        if (tid < m * kMaxK) s_coef[tid] = a.coef[tid];
        __syncthreads();
        for (int t = tid; t < m * K + K; t += BS) {
            if (t < m * K) {
                const int j = t / K, i = t - j * K;
                build_perm_table(&s_tab[t], s_coef[j * kMaxK + i], s_exp, s_log);
            } else {
                build_perm_table(&s_scl[t - m * K], a.scale[t - m * K], s_exp, s_log);
            }
        }
        __syncthreads();
    }

    const uint32_t chunks = a.chunks;  // 16-B chunks per cell
    const uint32_t tps = a.tiles_per_stripe;
    constexpr uint32_t TILE = 64 * U;  // chunks per wave-tile
    const uint32_t lcol = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    const uint32_t waves = gridDim.x * uint32_t(BS / 64);
    const uint32_t wave = blockIdx.x * uint32_t(BS / 64) + wib;
    const int units = K + m;
    uint32_t rot = 0;  // located wave-tiles dealt so far, mod waves: the same in every wave

    for (uint64_t s0 = 0; s0 < a.stripes; s0 += 64) {
        const uint64_t mine = s0 + lcol;
        int32_t verdict = kCorrectClean;
        if (mine < a.stripes) {
            // the pair is 8-byte aligned (the C ABI asks no more): two 64-bit words
            verdict = correct_verdict(a.results[2 * mine], a.results[2 * mine + 1], units);
            if (wib == 0 && mine % gridDim.x == blockIdx.x) a.units[mine] = verdict;
        }
        uint64_t located = __builtin_amdgcn_ballot_w64(verdict >= 0);
        while (located != 0) {
            const int lane = __builtin_ctzll(located);
            located &= located - 1;
            const uint64_t stripe = s0 + uint32_t(lane);
            const int t = __builtin_amdgcn_readfirstlane(__shfl(verdict, lane, 64));  // < units
            const int row = __builtin_amdgcn_readfirstlane(int(a.row[t]));            // < m
            const bool data = t < K;
            // this stripe's tiles tcol with (rot + tcol) % waves == wave
            const uint32_t first = wave >= rot ? wave - rot : wave + waves - rot;
            const uint8_t* const par = a.base[K + row] + stripe * a.stride[K + row];
            uint8_t* const dst = a.base[t] + stripe * a.stride[t];
            for (uint64_t tc = first; tc < tps; tc += waves) {
                const uint32_t tcol = uint32_t(tc);
                // the table reads stay inside the loop (as gf_scrub)
                asm volatile("" ::: "memory");
                uint32_t offs[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t col = tcol * TILE + u * 64u + lcol;
                    offs[u] = (col < chunks ? col : 0u) * 16u;  // a lane past the cell re-reads offset 0; never stored
                }
                u32x4 x[U][K];
                u32x4 old[U];  // the located unit's chunk
                u32x4 acc[U];
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int i = 0; i < K; i++) x[u][i] = load16<true>((a.base[i] + stripe * a.stride[i]) + offs[u]);
#pragma unroll
                for (int u = 0; u < U; u++) acc[u] = load16<true>(par + offs[u]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; u++) {
                    old[u] = acc[u];
#pragma unroll
                    for (int i = 0; i < K; i++)
                        if (t == i) old[u] = x[u][i];
                }
                // the one syndrome row
                uint32_t toff = uint32_t(row) * uint32_t(K * sizeof(PermTable));
#pragma unroll
                for (int i = 0; i < K; i++) {
                    const PermTable& p = *reinterpret_cast<const PermTable*>(
                        reinterpret_cast<const char*>(&s_tab[i]) + toff);
                    const uint32_t t0lo = p.t0lo, t0hi = p.t0hi, t1lo = p.t1lo, t1hi = p.t1hi, t2 = p.t2;
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int d = 0; d < 4; d++) {
                            const Sel s = make_sel(x[u][i][d]);
                            acc[u][d] ^= gf_mul4(t0lo, t0hi, t1lo, t1hi, t2, s.s0, s.s1, s.s2);
                        }
                }
                // e = scale[t] * s_row (scale 1 for a parity unit)
                if (data) {
                    const PermTable& p = s_scl[t];
                    const uint32_t t0lo = p.t0lo, t0hi = p.t0hi, t1lo = p.t1lo, t1hi = p.t1hi, t2 = p.t2;
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int d = 0; d < 4; d++) {
                            const Sel s = make_sel(acc[u][d]);
                            acc[u][d] = gf_mul4(t0lo, t0hi, t1lo, t1hi, t2, s.s0, s.s1, s.s2);
                        }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t col = tcol * TILE + u * 64u + lcol;
                    const uint32_t nz = acc[u][0] | acc[u][1] | acc[u][2] | acc[u][3];
                    if (col < chunks && nz != 0) store16<false>(dst + uint64_t(col) * 16u, old[u] ^ acc[u]);
                }
            }
            rot = uint32_t((uint64_t(rot) + tps) % waves);
        }
    }
}

// Every other shape: any k + m <= kMaxShards, m <= 16, any alignment and
// cell_len.  The block scans the results 256 stripes at a time (one per
// thread, verdicts shared through LDS) and deals the located stripes'
// 4 KiB block-tiles round-robin over the blocks of the grid; one thread per
// byte position, LDS log/antilog products.
constexpr int kCorrectMaxM = 16;             // HEC_MAX_PARITY_UNITS
constexpr uint32_t kCorrectByteTile = 4096;  // bytes of a stripe per block-tile
__global__ __launch_bounds__(256) void gf_scrub_correct_bytes(ScrubCorrectArgs a) {
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_coef[kCorrectMaxM * kMaxK];
    __shared__ int32_t s_verdict[256];
    const int tid = threadIdx.x;
    const int k = a.k, m = a.m;
    s_exp[tid] = kDevGf.exp[tid];
    s_exp[tid + 256] = kDevGf.exp[tid + 256];
    s_log[tid] = kDevGf.log[tid];
    for (int t = tid; t < m * kMaxK; t += 256) s_coef[t] = a.coef[t];
    const uint64_t tps = (a.cell_len + kCorrectByteTile - 1) / kCorrectByteTile;
    const uint32_t blocks = gridDim.x;
    uint32_t rot = 0;  // located block-tiles dealt so far, mod blocks: the same in every block
    for (uint64_t s0 = 0; s0 < a.stripes; s0 += 256) {
        __syncthreads();  // the tables (first round); the last round's s_verdict is read
        const uint64_t mine = s0 + uint32_t(tid);
        int32_t verdict = kCorrectClean;
        if (mine < a.stripes) {
            verdict = correct_verdict(a.results[2 * mine], a.results[2 * mine + 1], k + m);
            if (mine % blocks == blockIdx.x) a.units[mine] = verdict;
        }
        s_verdict[tid] = verdict;
        __syncthreads();
        for (int l = 0; l < 256; l++) {
            const int t = s_verdict[l];  // block-uniform
            if (t < 0) continue;
            const uint64_t stripe = s0 + uint32_t(l);
            const int row = a.row[t];
            const uint8_t scale = a.scale[t];
            const uint8_t* const par = a.base[k + row] + stripe * a.stride[k + row];
            uint8_t* const dst = a.base[t] + stripe * a.stride[t];
            const uint32_t first = blockIdx.x >= rot ? blockIdx.x - rot : blockIdx.x + blocks - rot;
            for (uint64_t tile = first; tile < tps; tile += blocks) {
                const uint64_t begin = tile * kCorrectByteTile;
                for (uint32_t r = 0; r < kCorrectByteTile / 256; r++) {
                    const uint64_t b = begin + r * 256u + uint32_t(tid);
                    if (b >= a.cell_len) break;
                    uint8_t s = par[b];
                    for (int i = 0; i < k; i++)
                        s ^= lds_gf_mul(s_exp, s_log, s_coef[row * kMaxK + i], a.base[i][stripe * a.stride[i] + b]);
                    const uint8_t e = lds_gf_mul(s_exp, s_log, scale, s);
                    if (e != 0) dst[b] ^= e;
                }
            }
            rot = uint32_t((uint64_t(rot) + tps) % blocks);
        }
    }
}

namespace {

// U = 4 in 256-thread blocks up to k = 6, U = 2 in 512-thread blocks for
// k = 10 (the shapes of gf_scrub); one kernel per k, m is a run-time value.
struct CorrectFn {
    template <int K, int R>
    static const void* fn() {
        if constexpr (K > 6)
            return reinterpret_cast<const void*>(&gf_scrub_correct<K, 2, 512>);
        else
            return reinterpret_cast<const void*>(&gf_scrub_correct<K, 4, 256>);
    }
};

}  // namespace

int launch_scrub_correct(const ScrubCorrectArgs& in, int device, hipStream_t stream) {
    ScrubCorrectArgs a = in;
    if (a.k < 1 || a.k > kMaxK || a.m < 1 || a.m > kCorrectMaxM || a.k + a.m > kMaxShards || a.cell_len == 0 ||
        !a.results || !a.units)
        return -1;
    if (a.stripes == 0) return 0;
    for (int t = 0; t < a.k + a.m; t++)
        if (a.row[t] >= a.m) return -1;
    const int cus = num_cus(device);
    bool fast = (a.k == 2 || a.k == 3 || a.k == 6 || a.k == 10) && a.m <= kMaxR && a.cell_len % 16 == 0 &&
                a.cell_len < (uint64_t(1) << 32) && a.stripes <= 0xFFFFFFFFull;
    for (int i = 0; fast && i < a.k + a.m; i++)
        fast = ((reinterpret_cast<uintptr_t>(a.base[i]) | a.stride[i]) & 15u) == 0;
    if (fast && !tile_geometry(a, 1024u * wave_tile_u(a.k), 0xFFF00000ull)) fast = false;
    void* args[] = {&a};
    if (fast) {
        const void* fn = pick_kr<CorrectFn>(a.k, 1);
        if (!fn) return -1;
        // one block per CU, capped by the wave-tiles there can be
        const uint32_t wpb = uint32_t(wave_tile_bs(a.k)) / 64u;
        uint64_t grid = uint64_t(cus);
        const uint64_t cap = (uint64_t(a.total_tiles) + wpb - 1) / wpb;
        if (grid > cap) grid = cap;
        if (grid < 1) grid = 1;
        const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(wave_tile_bs(a.k)), args, 0, stream);
        return e == hipSuccess ? 0 : int(e);
    }
    const uint64_t btps = (a.cell_len + kCorrectByteTile - 1) / kCorrectByteTile;
    if (btps > 0xFFFFFFFFFFFFFFFFull / a.stripes) return -1;
    uint64_t grid = uint64_t(cus) * 8;
    if (grid > btps * a.stripes) grid = btps * a.stripes;
    const hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&gf_scrub_correct_bytes), dim3(uint32_t(grid)),
                                         dim3(256), args, 0, stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
