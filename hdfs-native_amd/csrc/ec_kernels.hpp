// ec_kernels.hpp -- kernel argument block and launcher for the GF(2^8)
// stripe-cell matrix multiply (see ec_kernels.hip).
#pragma once

#ifndef __HIPCC_RTC__  // hiprtc (jit.cpp) provides the HIP runtime itself
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;  // the launchers below are host code: declarations only
#endif

#include <cstdint>

#include "tuning.hpp"

namespace hec {

constexpr int kBlock = 256;  // threads per block (4 waves)
constexpr int kMaxK = 32;    // inputs per launch (HEC_MAX_DATA_UNITS)
constexpr int kMaxR = 4;     // outputs per launch (more rows are split)

// Passed by value as the kernel argument (kernarg segment, ~800 B).
struct MatmulArgs {
    const uint8_t* in[kMaxK];
    uint64_t in_stride[kMaxK];  // bytes between stripes for input i
    uint8_t* out[kMaxR];
    uint64_t out_stride[kMaxR];
    uint8_t coef[kMaxR * kMaxK];  // row j, column i at [j*kMaxK + i]
    int32_t k;                    // inputs used
    int32_t r;                    // outputs used (1..kMaxR)
    uint64_t cell_len;            // bytes per cell
    uint64_t stripes;
    uint64_t byte_begin;          // byte kernel: first byte handled
    uint32_t chunks;              // vec kernel: 16-B chunks per cell
    uint32_t tiles_per_stripe;
    uint32_t total_tiles;
    uint32_t group;               // tile order: G stripes column-interleaved (1 = stripe-major)
    uint32_t grouped_tiles;       // tiles of the whole G-stripe groups; the remainder stripes go stripe-major
    uint32_t drain;               // register kernel: 1 = wait for the tile's stores before the next tile's loads
    uint32_t col_rot = 0;         // tile order: stripe s starts its columns at (s * col_rot) % tiles (0 = none)
    uint32_t* queue = nullptr;       // work-queue kernels: this launch's counters (zero when it starts)
    uint32_t* queue_zero = nullptr;  // the set this launch zeroes for the stream's next launch (nullptr: none)
};

// One coefficient's v_perm_b32 product tables (see ec_kernels.hip): c*x =
// perm(t0hi,t0lo,x&7) ^ perm(t1hi,t1lo,(x>>3)&7) ^ perm(t2,t2,x>>6), 32 B.
struct PermTable {
    uint32_t t0lo, t0hi, t1lo, t1hi, t2, pad0, pad1, pad2;
};

// ---- heterogeneous per-stripe erasure patterns ---------------------------
constexpr int kMaxShards = kMaxK + 16;  // k + m <= 48

// Plan blob entry (device workspace): header, then e x k PermTables.
struct DevPlanHeader {
    uint32_t e;              // missing data shards
    uint8_t surv[kMaxK];     // survivor shard indices (first k present)
    uint8_t miss[16];        // missing data indices, ascending
    uint8_t pad[12];
};
static_assert(sizeof(DevPlanHeader) == 64, "plan header is 64 B");

constexpr uint32_t kNoPlan = 0xFFFFFFFFu;  // stripe with no missing data shard

// Workspace (device): [per-stripe plan offset: u32 x stripes][plan blob]
// [kMixedQueueBytes: zeroed tile counters, kMixedQueues per launch, one per
// kMixedQueueStride bytes];
// plan = DevPlanHeader + e x k PermTables (row r, input i at r*k + i).
constexpr uint32_t kMixedQueues = 8, kMixedQueueStride = 256;
constexpr size_t kMixedQueueBytes = size_t(16) * kMixedQueues * kMixedQueueStride;  // up to 16 launches (64 rows)
struct MixedArgs {
    const uint8_t* base[kMaxShards];  // all k+m shard bases
    uint64_t stride[kMaxShards];
    uint8_t* out[kMaxK];              // reconstructed data shard i -> out[i]
    uint64_t out_stride[kMaxK];
    const uint8_t* plans;             // blob: plan of stripe s at plans + stripe_off[s]
    const uint32_t* stripe_off;       // per stripe; kNoPlan = nothing missing
    uint32_t blob_bytes;              // size of the blob
    int32_t k;
    int32_t row0;                     // first missing row handled by this launch
    uint64_t cell_len;
    uint64_t stripes;
    uint32_t chunks, tiles_per_stripe, total_tiles, group, grouped_tiles;
    uint32_t drain;                   // 1 = wait for a tile's stores before the next tile (tune key 6)
    uint32_t* queue;                  // this launch's zeroed tile counters (work-queue variant, key 26)
};

#ifndef __HIPCC_RTC__
// The work-queue counter sets of one launch (ec_kernels.hip, DESIGN.md §3.1
// "Counter sets").  A direct launch takes its stream's current set (`use`,
// zero) and zeroes the stream's other set (`zero`) for the next launch; the
// stream is held (its sets' lock) from queue_lease() until the lease ends, so
// launches from several threads on one stream still alternate in their
// stream order.  A launch into a stream that is being captured gets a set of
// its own (the graph keeps it for good) zeroed by a kernel node (zero_async)
// captured just before the kernel; `zero` is then nullptr.  An empty lease
// (use == nullptr) means: launch the fixed-order kernel.
struct QueueLease {
    uint32_t* use = nullptr;
    uint32_t* zero = nullptr;
    QueueLease() = default;
    QueueLease(QueueLease&& o) noexcept;
    QueueLease& operator=(QueueLease&& o) noexcept;
    QueueLease(const QueueLease&) = delete;
    QueueLease& operator=(const QueueLease&) = delete;
    ~QueueLease();
    explicit operator bool() const { return use != nullptr; }
    // The kernel was enqueued: the stream's next launch takes `zero`.  A lease
    // whose kernel was not enqueued leaves the stream on `use` (still zero).
    void launched();
    void* st_ = nullptr;  // the stream's sets (held while the lease lives)
};
QueueLease queue_lease(int device, hipStream_t stream);
// Allocates the device's pool of graph-capture sets, outside any capture
// (hec_coder_create calls it); a capture with no set left launches the
// fixed-order kernels.
void queue_reserve(int device);
// Zeroes `bytes` at p in stream order: hipMemsetAsync, and under stream
// capture (8-byte aligned p and bytes) a zeroing kernel node in its place.
hipError_t zero_async(void* p, size_t bytes, hipStream_t stream);
// Counter sets in use on a device: {direct streams, graph sets handed out}.
void queue_stats(int device, uint64_t* streams, uint64_t* graph_sets);
// 1 when streams are told apart by hipStreamGetId, 0 when by handle.
int queue_keyed_by_id();
#endif

// Mixed-pattern decode of one group of missing rows row0 .. row0+rows-1
// (rows <= kMaxR).  Requires k in {2,3,6,10}, 16-B aligned bases/strides
// and cell_len % 16 == 0.  0 ok, -1 unsupported, >0 hipError_t.
int launch_decode_mixed(const MixedArgs& a, int rows, int device, hipStream_t stream);

// ---- reconstruction: any lost unit of a stripe, parity included ------------
// Argument block of gf_reconstruct_mixed (ec_reconstruct.hip).  The workspace
// and the plan blobs are laid out as for MixedArgs; a plan's header holds the
// stripe's e TARGET units in miss[] (unit indices 0 .. k+m-1, ascending) and
// its rows are the targets' rows over the survivors.  Outputs are addressed
// by unit index: all k+m of them.
struct ReconArgs {
    const uint8_t* base[kMaxShards];  // all k+m unit bases
    uint64_t stride[kMaxShards];
    uint8_t* out[kMaxShards];         // rebuilt unit t -> out[t] (may be base[t]: repair in place)
    uint64_t out_stride[kMaxShards];
    const uint8_t* plans;             // blob: plan of stripe s at plans + stripe_off[s]
    const uint32_t* stripe_off;       // per stripe; kNoPlan = no target
    uint32_t blob_bytes;
    int32_t k;
    int32_t row0;                     // first target row handled by this launch
    uint64_t cell_len;
    uint64_t stripes;
    uint32_t chunks, tiles_per_stripe, total_tiles, group, grouped_tiles;
    uint32_t drain;                   // 1 = wait for a tile's stores before the next tile
    uint32_t* queue;                  // this launch's zeroed tile counters
};

// Mixed-pattern reconstruction of one group of target rows row0 ..
// row0+rows-1 (rows <= kMaxR), plans resident in LDS.  Requires k in
// {2,3,6,10}, 16-B aligned bases/strides, cell_len % 16 == 0, the launch
// counters (a.queue) and plan offsets + blob within the resident LDS budget.
// 0 ok, -1 unsupported (nothing was launched), >0 hipError_t.
int launch_reconstruct_mixed(const ReconArgs& a, int rows, int device, hipStream_t stream);
// That budget: plan offsets (u32 per stripe, 16-B padded) + plan blob.  gfx950
// has 160 KiB of LDS per CU and the kernel's static LDS is 1.5 KiB.
constexpr uint64_t kReconResidentMax = 156u << 10;
// True when a batch's plan offsets and blob fit it (a uniform plan has no
// offsets: stripes = 0); gf_scrub_mixed's budget is the same.
inline bool mixed_resident(uint64_t stripes, uint64_t blob_bytes) {
    return ((stripes * 4 + 15) & ~uint64_t(15)) + blob_bytes <= kReconResidentMax && blob_bytes % 4 == 0;
}

// ---- scrub: verify a stripe's parity and locate a corrupt unit --------------
// Argument block of gf_scrub / gf_scrub_bytes (ec_scrub.hip).  Read-only over
// all k+m units; per stripe two 64-bit words in `results` (hec_scrub_result_t:
// ruled_out, bad_bytes), zeroed on the stream before the launch.
struct ScrubArgs {
    const uint8_t* base[kMaxShards];  // all k+m unit bases, none null
    uint64_t stride[kMaxShards];
    uint8_t coef[16 * kMaxK];         // parity block P: row j, column i at [j*kMaxK + i]
    int32_t k, m;
    uint64_t cell_len;
    uint64_t stripes;
    uint64_t* results;                // [stripes][2], 8-B aligned
    uint32_t chunks, tiles_per_stripe, total_tiles, group, grouped_tiles;
    uint32_t drain;                   // as MatmulArgs::drain
    uint32_t* queue;                  // this launch's zeroed tile counters (nullptr: the fixed order)
    uint32_t* queue_zero;             // the set this launch zeroes for the stream's next launch
};

// Scrubs a batch.  The fast kernel takes k in {2,3,6,10}, m <= 4, 16-B aligned
// bases, strides and cell_len and a parity block whose first row has no zero;
// everything else runs the byte-granular kernel (same results).  `results`
// must already be zeroed in stream order.  0 ok, -1 invalid sizes, >0 hipError_t.
int launch_scrub(const ScrubArgs& a, int device, hipStream_t stream);

// ---- scrub correction: fix the located unit in place -------------------------
// Argument block of gf_scrub_correct / gf_scrub_correct_bytes
// (ec_scrub_correct.hip).  Reads `results` (what a scrub of these very cells
// wrote, earlier on the stream), writes `units` for every stripe and, in a
// LOCATED stripe, the located unit's cell; everything else is read-only.
constexpr int32_t kCorrectClean = -1;      // HEC_CORRECT_CLEAN
constexpr int32_t kCorrectUnlocated = -2;  // HEC_CORRECT_UNLOCATED
struct ScrubCorrectArgs {
    uint8_t* base[kMaxShards];        // all k+m unit bases, none null
    uint64_t stride[kMaxShards];
    uint8_t coef[16 * kMaxK];         // parity block P: row j, column i at [j*kMaxK + i]
    uint8_t row[kMaxShards];          // unit t: the syndrome row its error is read from, < m
    uint8_t scale[kMaxShards];        // unit t: 1 / H[row[t]][t]
    int32_t k, m;
    uint64_t cell_len;
    uint64_t stripes;
    const uint64_t* results;          // [stripes][2], 8-B aligned
    int32_t* units;                   // [stripes]: the located unit, kCorrectClean or kCorrectUnlocated
    uint32_t chunks, tiles_per_stripe, total_tiles;  // register kernel (the launcher fills them)
};

// Corrects a batch.  The register kernel takes k in {2,3,6,10}, m <= 4 and
// 16-B aligned bases, strides and cell_len; everything else runs the
// byte-granular kernel (same results).  One kernel launch, no counters, no
// workspace.  0 ok, -1 invalid sizes, >0 hipError_t.
int launch_scrub_correct(const ScrubCorrectArgs& a, int device, hipStream_t stream);

// ---- degraded scrub: one presence mask per stripe ---------------------------
// Plan blob entry of gf_scrub_mixed / gf_scrub_mixed_bytes (ec_scrub_mixed.hip):
// the stripe's survivors S (first k present units), extras E (the other
// present units, ascending) and missing units, then the rows of
// G = C[E] . inverse(C[S]): e x k PermTables (row j, survivor i at j*k + i) for
// the register kernel, e x k coefficient bytes (padded to 16 B) for the byte
// kernel.  Same size and leading fields as DevPlanHeader.
struct ScrubPlanHeader {
    uint32_t e;             // extras = checks of this stripe, >= 1
    uint8_t surv[kMaxK];    // survivor unit indices
    uint8_t extras[16];     // extra unit indices, ascending; 0 past e
    uint32_t missing_lo;    // bit t set: unit t is missing (never the culprit)
    uint32_t missing_hi;
    uint8_t pad[4];
};
static_assert(sizeof(ScrubPlanHeader) == 64, "plan header is 64 B");

// Workspace (device): [per-stripe plan offset: u32 x stripes][plan blob]
// [kMixedQueueStride x kMixedQueues: the launch's zeroed tile counters].
// Read-only over the present units; results as for ScrubArgs.
struct ScrubMixedArgs {
    const uint8_t* base[kMaxShards];  // all k+m unit bases, none null
    uint64_t stride[kMaxShards];
    const uint8_t* plans;             // blob: plan of stripe s at plans + stripe_off[s]
    const uint32_t* stripe_off;       // per stripe; kNoPlan = not checkable (e == 0).  nullptr: the
                                      // uniform plan -- every stripe of the launch uses the plan at `plans`
    uint32_t blob_bytes;              // size of the blob (uniform: of the one plan)
    int32_t k;
    uint64_t cell_len;
    uint64_t stripes;
    uint64_t* results;                // [stripes][2], 8-B aligned, zeroed in stream order
    uint32_t chunks, tiles_per_stripe, total_tiles, group, grouped_tiles;
    uint32_t drain;                   // as MatmulArgs::drain
    uint32_t* queue;                  // this launch's zeroed tile counters (nullptr: the fixed order)
};

// Register kernel, plans resident in LDS: k in {2,3,6,10}, every stripe's
// e <= max_e <= kMaxR, 16-B aligned bases, strides and cell_len, row 0 of every
// plan without a zero (the caller checks).  With a.stripe_off the batch's
// offsets + blob must fit the resident budget (mixed_resident) and
// a.queue is required; without it (uniform plan) the one plan at a.plans is
// resident and the tiles go in the fixed order.  0 ok, -1 unsupported (nothing
// was launched), >0 hipError_t.
int launch_scrub_mixed(const ScrubMixedArgs& a, int max_e, int device, hipStream_t stream);
// Byte-granular kernel: any k <= kMaxK, e <= 16, alignment and cell_len; plans
// with coefficient bytes, read from global memory.  Same results.
int launch_scrub_mixed_bytes(const ScrubMixedArgs& a, int device, hipStream_t stream);

// True when the launch's coefficients are the RS coding matrix's parity rows
// (gen_rs_matrix, gf256.rs:40-57) for its (k, r): the encode kernels then
// run the bit-sliced XOR networks of xor_networks.hpp.
bool rs_parity_matrix(const MatmulArgs& a);

// Launches the multiply for one group of <= kMaxR output rows.  0 on
// success, -1 invalid sizes, otherwise the (positive) hipError_t.
int launch_gf_matmul(const MatmulArgs& a, int device, hipStream_t stream);


}  // namespace hec
