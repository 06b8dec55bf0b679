// launch_parts.hpp -- host-side parts of the launchers in ec_scrub*.hip and
// ec_reconstruct*.hip: which (k, r) have a register kernel, a launch's tile
// counts with their 32-bit guards, the tile order, the dynamic LDS of the
// resident-plan kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ec_kernels.hpp"
#include "gf_device.hpp"  // tile_order

namespace hec {
namespace {  // per translation unit

// The one place that says which shapes are compiled: k in {2, 3, 6, 10}, r in
// 1 .. kMaxR.  F::fn<K, R>(args...) returns the file's kernel for the shape;
// nullptr for every other (k, r).
template <class F, class... A>
const void* pick_kr(int k, int r, A... args) {
    auto pick_r = [&](auto kc) -> const void* {
        constexpr int K = decltype(kc)::value;
        switch (r) {
            case 1: return F::template fn<K, 1>(args...);
            case 2: return F::template fn<K, 2>(args...);
            case 3: return F::template fn<K, 3>(args...);
            case 4: return F::template fn<K, 4>(args...);
            default: return nullptr;
        }
    };
    switch (k) {
        case 2: return pick_r(std::integral_constant<int, 2>{});
        case 3: return pick_r(std::integral_constant<int, 3>{});
        case 6: return pick_r(std::integral_constant<int, 6>{});
        case 10: return pick_r(std::integral_constant<int, 10>{});
        default: return nullptr;
    }
}

// The wave-tile kernels' shapes: U = 4 chunks per lane in 256-thread blocks up
// to k = 6, U = 2 in 512-thread blocks above.
inline int wave_tile_u(int k) { return k > 6 ? 2 : 4; }
inline int wave_tile_bs(int k) { return k > 6 ? 512 : 256; }

// Fills a.chunks / tiles_per_stripe / total_tiles from a.cell_len (a multiple
// of 16) and a.stripes for tiles of tile_bytes of one stripe: 1024 U for the
// wave-tiles of 64 lanes x U 16-B chunks, 4096 SLABS for the block-tiles of 4
// waves x SLABS KiB.  False (nothing written) when a count does not fit: tile
// indices are 32-bit, and `limit` leaves room for what the kernel adds to one
// (the fixed order's stride: 0xFFF00000 for the scrubs).
template <class Args>
bool tile_geometry(Args& a, uint64_t tile_bytes, uint64_t limit = 0xFFFFFFFFull) {
    const uint64_t chunks = a.cell_len / 16;
    const uint64_t tps = (a.cell_len + tile_bytes - 1) / tile_bytes;
    if (chunks > 0xFFFFFFFFull || a.stripes > 0xFFFFFFFFull || tps * a.stripes > limit) return false;
    a.chunks = uint32_t(chunks);
    a.tiles_per_stripe = uint32_t(tps);
    a.total_tiles = uint32_t(tps * a.stripes);
    return true;
}

// The tile order of a launch: groups of tune key `group` stripes, or `dflt`.
template <class Args>
void set_tile_order(Args& a, const Tune& tn, uint32_t dflt) {
    tile_order(a.stripes, a.tiles_per_stripe, tn.group > 0 ? uint32_t(tn.group) : dflt, a.group, a.grouped_tiles);
}

// Dynamic LDS of the resident-plan kernels: plan offsets (u32 per stripe, 16-B
// padded; none for a uniform plan: stripes = 0) + plan blob.
inline uint64_t resident_lds_bytes(uint64_t stripes, uint64_t blob_bytes) {
    return ((stripes * 4 + 15) & ~uint64_t(15)) + blob_bytes;
}
// Past 64 KiB (up to kReconResidentMax) it needs the function attribute, as
// in launch_decode_mixed.  The attribute is set to the resident ceiling, never
// to a launch's size (a coder may be shared by threads).  False: the runtime
// refused the LDS, and the caller launches per run of stripes.
constexpr uint64_t kDynNoAttr = 64u << 10;
inline bool set_resident_lds_attr(const void* fn, uint64_t dyn) {
    if (dyn <= kDynNoAttr) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(kReconResidentMax)) == hipSuccess)
        return true;
    (void)hipGetLastError();
    return false;
}

}  // namespace
}  // namespace hec
