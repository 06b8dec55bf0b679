// ec_reconstruct.hip -- mixed-pattern reconstruction for gfx950: every stripe
// of a batch rebuilds its own set of lost units, data or parity, as a repair
// worker sees them after a DataNode died (each block group it held lost a
// different unit index).  Hadoop's RSRawDecoder.decode(inputs, erasedIndexes,
// outputs) per stripe; the reference's reader (gf256.rs:84-137) only rebuilds
// data units and has no counterpart.
//
// gf_reconstruct_mixed is the sibling of gf_decode_mixed's resident
// work-queue variant (ec_kernels.hip): the same per-tile metadata in three
// LDS round trips, the same register math, the same skip of rows past the
// stripe's e, the same drain and tile counters.  The difference is the output
// side: a plan's target bytes are unit indices over all k+m units, so the
// output bases and strides sit in an LDS table of kMaxShards entries
// (gf_decode_mixed's has kMaxK: data units only).  MixedArgs and
// gf_decode_mixed are untouched; the read path's measured numbers rest on them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ec_kernels.hpp"
// the plans arrive with their product tables built (host side): this file
// never builds one on the device
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "gf_device.hpp"
#pragma clang diagnostic pop
#include "launch_parts.hpp"

namespace hec {

// K inputs, R target rows per launch, U 16-B chunks per lane, BS threads.
// RESIDENT: the per-stripe plan offsets and every plan sit in dynamic LDS for
// the whole launch (the only variant: batches whose plans do not fit take one
// uniform launch per run of stripes, ec_capi.cpp).  WQ: rounds of wave-tiles
// (64 lanes x U chunks of one stripe) a wave takes per atomic from its block's
// launch counter (a.queue, zeroed by the workspace upload).
template <int K, int R, int U, int BS, bool RESIDENT, int WQ>
__global__ __launch_bounds__(BS) void gf_reconstruct_mixed(ReconArgs a) {
    static_assert(RESIDENT && WQ > 0, "resident plans and the work queue only");
    static_assert(K > 0 && R >= 1 && R <= kMaxR, "compile-time k, 1..4 rows");
    __shared__ uint64_t s_base[kMaxShards], s_stride[kMaxShards], s_obase[kMaxShards], s_ostride[kMaxShards];
    // [stripe plan offsets: u32 x stripes, 16-B padded][plan blob]
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const int tid = threadIdx.x;
    if (tid < kMaxShards) {
        s_base[tid] = reinterpret_cast<uint64_t>(a.base[tid]);
        s_stride[tid] = a.stride[tid];
        s_obase[tid] = reinterpret_cast<uint64_t>(a.out[tid]);
        s_ostride[tid] = a.out_stride[tid];
    }
    const uint32_t off_bytes = (uint32_t(a.stripes) * 4u + 15u) & ~15u;
    {
        const uint32_t off_words = uint32_t(a.stripes);
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
    MatmulArgs order;  // tile_coords reads tiles_per_stripe / group only
    order.tiles_per_stripe = a.tiles_per_stripe;
    order.group = a.group;
    order.grouped_tiles = a.grouped_tiles;
    order.stripes = a.stripes;

    u32x4 acc[U][R];  // previous tile's store data, held through the next loads (see gf_matmul_v16)
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int j = 0; j < R; j++) acc[u][j] = u32x4{0, 0, 0, 0};
    auto run_tile = [&](uint32_t tile) {
        uint32_t stripe, tcol;
        tile_coords(tile, order, stripe, tcol);
        const uint32_t off = __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t*>(s_dyn)[stripe]);
        if (off == kNoPlan) return;
        const DevPlanHeader* hdr = reinterpret_cast<const DevPlanHeader*>(s_dyn + off_bytes + off);
        // row r, input i at tabs[r * K + i]
        const PermTable* tabs =
            reinterpret_cast<const PermTable*>(s_dyn + off_bytes + off + sizeof(DevPlanHeader)) + a.row0 * K;
        // The tile's metadata in three dependent LDS round trips, as
        // gf_decode_mixed: the header words (e, survivor and target bytes),
        // every survivor's and output's base / stride, one wait.
        const uint32_t* hw = reinterpret_cast<const uint32_t*>(hdr);
        constexpr int SW = (K + 3) / 4;  // words of survivor bytes (surv[] at byte 4)
        uint32_t w_surv[SW];
        const uint32_t w_e = hw[0];
        const uint32_t w_miss = hw[9 + a.row0 / 4];  // miss[] at byte 36; row0 is a multiple of kMaxR = 4
#pragma unroll
        for (int t = 0; t < SW; t++) w_surv[t] = hw[1 + t];
        uint64_t v_base[K], v_stride[K], v_obase[R], v_ostride[R];
#pragma unroll
        for (int i = 0; i < K; i++) {
            const uint32_t sh = (w_surv[i / 4] >> (8 * (i % 4))) & 0xFFu;
            v_base[i] = s_base[sh];
            v_stride[i] = s_stride[sh];
        }
#pragma unroll
        for (int j = 0; j < R; j++) {
            // the target's unit index over all k+m units; rows past e hold 0
            // (any byte is clamped into the table): a valid slot, never stored
            const uint32_t mi = min((w_miss >> (8 * j)) & 0xFFu, uint32_t(kMaxShards - 1));
            v_obase[j] = s_obase[mi];
            v_ostride[j] = s_ostride[mi];
        }
        // all of it read before the row-count branch below (otherwise hipcc
        // sinks the reads past it: one more round trip)
        uint32_t w_e2 = w_e;
#pragma unroll
        for (int i = 0; i < K; i++) asm volatile("" : "+v"(v_base[i]), "+v"(v_stride[i]), "+v"(w_e2));
        const int nrows = int(__builtin_amdgcn_readfirstlane(w_e2)) - a.row0;  // rows of this launch in the plan
        if (nrows <= 0) return;
        asm volatile("" ::: "memory");

        bool live[U];
        uint32_t offs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t col = tcol * TILE + u * 64u + lcol;
            live[u] = col < chunks;
            offs[u] = (live[u] ? col : 0u) * 16u;
        }
        u32x4 x[U][K];
#pragma unroll
        for (int i = 0; i < K; i++) {
            const gbyte* ib = gptr(uniform64(v_base[i]) + uint64_t(stripe) * uniform64(v_stride[i]));
#pragma unroll
            for (int u = 0; u < U; u++) x[u][i] = gload16(ib + offs[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < R; j++) asm volatile("" ::"v"(acc[u][j]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < K; i++) {
            uint32_t toff = uint32_t(i) * uint32_t(sizeof(PermTable));
            asm volatile("" : "+v"(toff));
            if (i > 0) {
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int j = 0; j < R; j++) asm volatile("" : "+v"(acc[u][j]) : "v"(toff));
            }
            Sel sl[U][4];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int d = 0; d < 4; d++) sl[u][d] = make_sel(x[u][i][d]);
#pragma unroll
            for (int j = 0; j < R; j++) {
                // rows past the plan's e are skipped (nrows is wave-uniform: a
                // scalar branch); their accumulators are never stored
                if (j > 0 && j >= nrows) break;
                const PermTable& t =
                    *reinterpret_cast<const PermTable*>(reinterpret_cast<const char*>(tabs + j * K) + toff);
                const uint32_t t0lo = t.t0lo, t0hi = t.t0hi, t1lo = t.t1lo, t1hi = t.t1hi, t2 = t.t2;
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const uint32_t p = gf_mul4(t0lo, t0hi, t1lo, t1hi, t2, sl[u][d].s0, sl[u][d].s1, sl[u][d].s2);
                        acc[u][j][d] = i == 0 ? p : (acc[u][j][d] ^ p);
                    }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < R; j++) asm volatile("" : "+v"(acc[u][j]));
        const bool full = (tcol + 1) * TILE <= chunks;  // wave-uniform
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (j >= nrows) break;  // wave-uniform
            gbyte* ob = gptr_w(uniform64(v_obase[j]) + uint64_t(stripe) * uniform64(v_ostride[j]));
#pragma unroll
            for (int u = 0; u < U; u++)
                if (full || live[u]) gstore16(ob + offs[u], acc[u][j]);
        }
        if (a.drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // as gf_matmul_v16
    };
    // lane 0 holds the next batch index; the other lanes' copies are never
    // read (readfirstlane), so the atomic's result needs no merge and is
    // first waited for at the next batch, behind the tile drains
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
}

namespace {

// Shapes of gf_decode_mixed: U = 4 chunks per lane in 256-thread blocks up to
// k = 6, U = 2 in 512-thread blocks above; one round of wave-tiles per atomic
// for k >= 6, four below (more atomics per byte there).
struct ReconFn {
    template <int K, int R>
    static const void* fn() {
        if constexpr (K > 6)
            return reinterpret_cast<const void*>(&gf_reconstruct_mixed<K, R, 2, 512, true, 1>);
        else if constexpr (K == 6)
            return reinterpret_cast<const void*>(&gf_reconstruct_mixed<K, R, 4, 256, true, 1>);
        else
            return reinterpret_cast<const void*>(&gf_reconstruct_mixed<K, R, 4, 256, true, 4>);
    }
};

}  // namespace

int launch_reconstruct_mixed(const ReconArgs& in, int rows, int device, hipStream_t stream) {
    ReconArgs a = in;
    // lane offsets into a cell are 32-bit: cells of 4 GiB or more are not for this kernel
    if (a.cell_len % 16 != 0 || a.cell_len > 0xFFFFFFFFull || !a.queue || a.row0 < 0 ||
        a.row0 % kMaxR != 0 || a.row0 >= 16 || a.stripes > 0xFFFFFFFFull)
        return -1;
    if (!mixed_resident(a.stripes, a.blob_bytes)) return -1;
    const uint64_t dyn = resident_lds_bytes(a.stripes, a.blob_bytes);
    const void* fn = pick_kr<ReconFn>(a.k, rows);
    if (!fn || !set_resident_lds_attr(fn, dyn)) return -1;
    const Tune tn = tune_snapshot();
    if (!tile_geometry(a, 1024u * wave_tile_u(a.k))) return -1;
    const uint64_t total = a.total_tiles;
    if (total == 0) return 0;
    set_tile_order(a, tn, 4u);
    a.drain = tn.drain == 1 ? 0u : 1u;
    // one block per CU: the resident plans are staged once per block and the
    // blocks drain the queue
    uint64_t grid = uint64_t(num_cus(device)) * (tn.blocks_per_cu ? tn.blocks_per_cu : 1);
    if (grid > total) grid = total;
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, dim3(uint32_t(grid)), dim3(wave_tile_bs(a.k)), args, uint32_t(dyn), stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace hec
