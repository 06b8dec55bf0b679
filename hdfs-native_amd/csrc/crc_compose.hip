// crc_compose.hip -- composite CRCs on the device (crc_compose.hpp has the
// algebra): chunk sums -> cell CRCs, cell CRCs -> unit and block-group CRCs.
//
// Every fold here is the same sum, over items counted from the END of the
// sequence they belong to:  fold = XOR_q M^q * t_q  with one constant M
// (x^(8 bpc) over chunks, x^(8 cell_len) over cells).  A group of W lanes
// (W = 64, or a power of two below when a cell has fewer chunks) takes the
// items q = j + W i of lane j: Horner in M^W over i, then one multiply by the
// lane's own M^j, then an XOR butterfly.  Counting from the end makes M^j
// independent of the sequence length, so the last stripe's shorter cells take
// the same path; whatever does not fit the uniform part (a cell's last chunk,
// the last stripe of a unit or of the group) is one more multiply by a
// constant of its own.  The host raises every constant (the levels M^(2^l),
// the tails, the last stripe's lengths); the device only multiplies.
//
// Multiplying by a constant is a 32x32 GF(2) map.  The chunk kernel's Horner
// step, one per chunk sum and so nearly all of the work, goes through four
// 256-entry byte tables of its constant, built in LDS by each block (as
// apply_shift does for the zero-byte shifts); every other multiply is the
// 32-column conditional XOR of mulmod: with a wave-uniform constant the
// columns c x^i live in SGPRs (scalar ALU), a lane's own constant M^j is
// expanded into 32 VGPR columns once per thread.
#include <hip/hip_runtime.h>

#include "crc_compose.hpp"
#include "tuning.hpp"

// The chunk kernel's Horner step: 1 = four byte tables in LDS (the default),
// 0 = the conditional XOR with the columns in SGPRs.  Measured A/B in
// the tables fold 1 MiB cells 1.9x and 64 KiB cells 1.3x faster.
#ifndef HEC_COMPOSE_LDS_TABLES
#define HEC_COMPOSE_LDS_TABLES 1
#endif

namespace hec {
namespace {

using crc::bswap32;
using crc::kAffine;
using crc::mulmod;

// M^j from the levels M^(2^l)
template <int KIND>
__device__ __forceinline__ uint32_t lane_power(const uint32_t* lvl, uint32_t j) {
    uint32_t p = crc::poly_one<crc::Spec<KIND>::kReflected>();
#pragma unroll
    for (int b = 0; b < 6; b++)
        if ((j >> b) & 1u) p = mulmod<KIND>(p, lvl[b]);
    return p;
}

__device__ __forceinline__ uint32_t xor_butterfly(uint32_t v, uint32_t width) {
    for (uint32_t off = width >> 1; off; off >>= 1) v ^= __shfl_xor(v, int(off));
    return v;
}

// Chunk sums -> t of every cell: to cell_out as a big-endian CRC and / or to
// ws_cells as t for the folds below.  256 / W cells per block, grid-stride.
template <int KIND, bool TABLES>
__global__ __launch_bounds__(256) void compose_cells(const ComposeArgs a) {
    constexpr uint32_t A = kAffine<KIND>;
    const uint32_t W = 1u << a.log_w;
    const uint32_t j = threadIdx.x & (W - 1);
    const uint32_t pj = lane_power<KIND>(a.lvl_chunk, j);  // x^(8 bpc j)
    // full cells: the uniform part ends where the last chunk starts, tail bytes before the end
    uint32_t col[32];
    {
        uint32_t c = mulmod<KIND>(pj, a.tail_full);
#pragma unroll
        for (int i = 0; i < 32; i++) {
            col[i] = c;
            c = crc::xtime<KIND>(c);
        }
    }
    const uint32_t horner = a.lvl_chunk[a.log_w];  // x^(8 bpc W)
    // the Horner step: acc * horner, by the conditional XOR or by four byte tables in LDS
    const uint32_t* tab = nullptr;
    if constexpr (TABLES) {
        __shared__ uint32_t lds[4 * 256];
#pragma unroll
        for (int b = 0; b < 4; b++) lds[256 * b + threadIdx.x] = mulmod<KIND>(threadIdx.x << (8 * b), horner);
        __syncthreads();
        tab = lds;
    }
    auto times_horner = [&](uint32_t r) {
        if constexpr (TABLES)
            return tab[r & 0xFF] ^ tab[256 + ((r >> 8) & 0xFF)] ^ tab[512 + ((r >> 16) & 0xFF)] ^ tab[768 + (r >> 24)];
        else
            return mulmod<KIND>(r, horner);
    };
    const uint64_t cells = a.stripes * a.n;
    const uint64_t first_last = cells - a.n;
    const uint64_t per_block = 256u >> a.log_w;
    for (uint64_t base = uint64_t(blockIdx.x) * per_block; base < cells; base += uint64_t(gridDim.x) * per_block) {
        const uint64_t cell = base + (threadIdx.x >> a.log_w);
        const bool valid = cell < cells;
        const bool last = valid && cell >= first_last;
        const uint32_t u = last ? uint32_t(cell - first_last) : 0u;
        const uint64_t nc = !valid ? 0 : last ? a.last_nc[u] : a.nck;
        const uint64_t m = nc ? nc - 1 : 0;  // chunks of the uniform part
        const uint32_t* p = a.sums + cell * a.nck;
        uint32_t acc = 0;
        if (m > j)
            for (uint64_t i = (m - 1 - j) >> a.log_w;; i--) {
                const uint64_t q = j + (i << a.log_w);
                acc = times_horner(acc) ^ bswap32(p[m - 1 - q]) ^ A;
                if (i == 0) break;
            }
        uint32_t v = 0;
        if (!last) {
#pragma unroll
            for (int i = 0; i < 32; i++) v ^= col[i] & crc::term_mask<crc::Spec<KIND>::kReflected>(acc, i);
        } else {
            v = mulmod<KIND>(acc, pj);
        }
        v = xor_butterfly(v, W);
        if (last) v = mulmod<KIND>(v, a.last_tail[u]);
        if (valid && j == 0) {
            const uint32_t t = nc ? v ^ bswap32(p[nc - 1]) ^ A : 0u;
            if (a.cell_out) a.cell_out[cell] = bswap32(t ^ A);
            if (a.ws_cells) a.ws_cells[cell] = t;
        }
    }
}

// The cells a fold runs over, from the end: task < n is unit `task` (stripes
// S-2 .. 0), task == n the group (stripes S-2 .. 0, data units k-1 .. 0).  The
// last stripe is left to compose_final.
struct FoldTask {
    bool group, wanted;
    uint64_t items;
    __device__ FoldTask(const ComposeArgs& a, uint32_t task)
        : group(task == a.n), wanted(group ? a.group_out != nullptr : a.unit_out != nullptr),
          items((a.stripes - 1) * (group ? a.k : 1u)) {}
};

// One wave per (block of kComposeBlockItems cells, task):
// ws_part[task][b] = XOR_q x^(8 C (q - 1024 b)) t_q over the block's q.
template <int KIND>
__global__ __launch_bounds__(64) void compose_partials(const ComposeArgs a) {
    const uint32_t task = blockIdx.y, j = threadIdx.x;
    const FoldTask f(a, task);
    const uint64_t q0 = uint64_t(blockIdx.x) * crc::kComposeBlockItems;
    if (!f.wanted || q0 >= f.items) return;
    const uint64_t left = f.items - q0;
    const uint32_t cnt = left < crc::kComposeBlockItems ? uint32_t(left) : uint32_t(crc::kComposeBlockItems);
    const uint32_t horner = a.lvl_cell[6];  // x^(8 C 64)
    uint32_t acc = 0;
    for (int i = int(crc::kComposeBlockItems / 64) - 1; i >= 0; i--) {
        const uint32_t ql = j + 64u * uint32_t(i);
        if (ql < cnt) {
            const uint64_t p = f.items - 1 - (q0 + ql);  // position from the start
            const uint64_t idx = f.group ? (p / a.k) * a.n + p % a.k : p * a.n + task;
            acc = mulmod<KIND>(acc, horner) ^ a.ws_cells[idx];
        }
    }
    const uint32_t v = xor_butterfly(mulmod<KIND>(acc, lane_power<KIND>(a.lvl_cell, j)), 64);
    if (j == 0) a.ws_part[uint64_t(task) * a.part_stride + blockIdx.x] = v;
}

// One wave per task: the partials folded in x^(8 C 1024), then the last stripe.
template <int KIND>
__global__ __launch_bounds__(64) void compose_final(const ComposeArgs a) {
    constexpr uint32_t A = kAffine<KIND>;
    const uint32_t task = blockIdx.x, j = threadIdx.x;
    const FoldTask f(a, task);
    if (!f.wanted) return;
    const uint64_t nb = (f.items + crc::kComposeBlockItems - 1) / crc::kComposeBlockItems;
    const uint32_t* part = a.ws_part + uint64_t(task) * a.part_stride;
    const uint32_t horner = a.lvl_part[6];
    uint32_t acc = 0;
    if (nb > j)
        for (uint64_t i = (nb - 1 - j) >> 6;; i--) {
            acc = mulmod<KIND>(acc, horner) ^ part[j + (i << 6)];
            if (i == 0) break;
        }
    const uint32_t v = xor_butterfly(mulmod<KIND>(acc, lane_power<KIND>(a.lvl_part, j)), 64);
    const uint32_t* last = a.ws_cells + (a.stripes - 1) * a.n;
    if (!f.group) {
        if (j == 0) a.unit_out[task] = bswap32(mulmod<KIND>(v, a.last_unit[task]) ^ last[task] ^ A);
    } else {
        // the last stripe's data cells, each moved past the cells after it
        const uint32_t w = xor_butterfly(j < a.k ? mulmod<KIND>(last[j], a.last_group[j]) : 0u, 64);
        if (j == 0) a.group_out[0] = bswap32(mulmod<KIND>(v, a.last_stripe) ^ w ^ A);
    }
}

template <int KIND>
void fill_constants(const crc::Geometry& g, ComposeArgs& a) {
    uint32_t c = crc::xpow8<KIND>(g.bpc);
    for (int l = 0; l < 7; l++, c = mulmod<KIND>(c, c)) a.lvl_chunk[l] = c;
    c = crc::xpow8<KIND>(g.cell_len);
    for (int l = 0; l < 17; l++, c = mulmod<KIND>(c, c)) {
        if (l < 7) a.lvl_cell[l] = c;
        if (l >= 10) a.lvl_part[l - 10] = c;  // kComposeBlockItems = 2^10
    }
    static_assert(crc::kComposeBlockItems == 1024, "lvl_part starts at level 10");
    a.tail_full = crc::xpow8<KIND>(g.cell_len - (g.nck - 1) * g.bpc);
    a.last_stripe = crc::xpow8<KIND>(g.last_len);
    uint64_t after = 0;  // data bytes of the last stripe after unit u
    for (uint64_t u = g.n; u-- > 0;) {
        const uint64_t len = g.len_last[u];
        const uint64_t nc = len / g.bpc + (len % g.bpc != 0);
        a.last_nc[u] = nc;
        a.last_tail[u] = nc ? crc::xpow8<KIND>(len - (nc - 1) * g.bpc) : 0u;
        a.last_unit[u] = crc::xpow8<KIND>(len);
        a.last_group[u] = 0;
        if (u < g.k) {
            a.last_group[u] = crc::xpow8<KIND>(after);
            after += len;
        }
    }
}

template <int KIND>
int launch_kind(const crc::Geometry& g, ComposeArgs& a, int device, hipStream_t stream) {
    fill_constants<KIND>(g, a);
    void* args[] = {&a};
    const uint64_t cells = g.stripes * g.n;
    const uint64_t per_block = 256u >> a.log_w;
    uint64_t grid = (cells + per_block - 1) / per_block;
    const uint64_t cap = uint64_t(num_cus(device)) * 8;
    if (grid > cap) grid = cap;
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&compose_cells<KIND, HEC_COMPOSE_LDS_TABLES != 0>), dim3(uint32_t(grid)), dim3(256),
                                   args, 0, stream);
    if (e != hipSuccess) return int(e);
    if (!a.unit_out && !a.group_out) return 0;
    const uint64_t nb = crc::compose_partials_per_fold(a.group_out ? g.k : 1, g.stripes);
    if (nb) {
        e = hipLaunchKernel(reinterpret_cast<const void*>(&compose_partials<KIND>),
                            dim3(uint32_t(nb), uint32_t(g.n + 1)), dim3(64), args, 0, stream);
        if (e != hipSuccess) return int(e);
    }
    e = hipLaunchKernel(reinterpret_cast<const void*>(&compose_final<KIND>), dim3(uint32_t(g.n + 1)), dim3(64), args, 0,
                        stream);
    return e == hipSuccess ? 0 : int(e);
}

}  // namespace

int launch_composite_crc(int kind, const crc::Geometry& g, const uint8_t* d_sums, uint8_t* d_cell_crcs,
                         uint8_t* d_unit_crcs, uint8_t* d_group_crc, void* d_workspace, int device,
                         hipStream_t stream) {
    if (g.stripes == 0 || (!d_cell_crcs && !d_unit_crcs && !d_group_crc)) return 0;
    const bool folds = d_unit_crcs || d_group_crc;
    if (folds && !d_workspace) return -1;
    const uint64_t part_stride = crc::compose_partials_per_fold(g.n, g.stripes);
    // block indices are 32-bit
    if (part_stride > 0x7FFFFFFFull) return -1;
    ComposeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sums = reinterpret_cast<const uint32_t*>(d_sums);
    a.cell_out = reinterpret_cast<uint32_t*>(d_cell_crcs);
    a.unit_out = reinterpret_cast<uint32_t*>(d_unit_crcs);
    a.group_out = reinterpret_cast<uint32_t*>(d_group_crc);
    if (folds) {
        a.ws_cells = static_cast<uint32_t*>(d_workspace);
        a.ws_part = a.ws_cells + g.stripes * g.n;
    }
    a.stripes = g.stripes;
    a.nck = g.nck;
    a.n = uint32_t(g.n);
    a.k = uint32_t(g.k);
    a.part_stride = uint32_t(part_stride);
    // the lanes of a cell: the uniform part has nck - 1 chunks
    while (a.log_w < 6 && (uint64_t(1) << a.log_w) < g.nck - 1) a.log_w++;
    if (kind == crc::kCrc32c) return launch_kind<crc::kCrc32c>(g, a, device, stream);
    if (kind == crc::kCksum) return launch_kind<crc::kCksum>(g, a, device, stream);
    return -1;
}

}  // namespace hec
