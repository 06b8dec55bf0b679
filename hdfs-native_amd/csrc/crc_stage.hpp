// crc_stage.hpp -- the checksum round of gf_reconstruct_crc and gf_scrub_crc:
// the fold checksum (scheme 12) over a wave-private 9-KiB image of 64 rows of
// 144 B, one row per lane = one quarter of a 512-B chunk.  A round covers 8
// slabs of 1 KiB: with SLABS slabs of every cell in a wave-tile that is
// SPR = 8 / SLABS cells (round slots).  Lane l's row is piece l/8 = (slot sir,
// slab pslab), chunk half (l/4)&1 of that slab, quarter qi = l&3; the chunk
// starts at byte cbyte of the cell and is `full` when all 512 B lie inside it.
// A short last chunk is walked whole, bytewise, by its quarter-0 lane.
//
// CrcStage is built inside the tile loop from REFERENCES to the kernel's own
// locals and is gone after inlining: both kernels keep the machine code they
// had with the round written out in place (profiles/kernel_parts/).
//
// gf_fused_crc (ec_fused_kernel.hpp) keeps a round of its own: its WANT_PF
// mode shuffles the expected sums in every lane and its sums_nt store mode is
// a tuned knob, and the benchmark rests on what that kernel compiles to.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "checksum.hpp"
#include "checksum_device.hpp"
#include "gf_device.hpp"

namespace hec {
namespace {  // per translation unit, as gf_device.hpp

template <int SLABS, int KIND>
struct CrcStage {
    static_assert(SLABS == 4 || SLABS == 8, "one or two cells per checksum round");
    static constexpr int SCHEME = 12;
    static constexpr int PITCH = 144, STAGE = 64 * PITCH, SPR = 8 / SLABS;
    using TL = crcdev::TableLayout<SCHEME>;
    using Spec = crc::Spec<KIND>;
    using BT = crcdev::ByteTable<SCHEME>;

    const uint32_t (&ctabs)[TL::kWords];  // crcdev::stage_tables' image in LDS
    uint8_t* const& stage;                // this wave's image
    const uint32_t& kfinal;
    const uint64_t& cell_len;
    const int &lane, &qi, &sir;  // the lane's place in a round
    const uint64_t& cbyte;       // first byte of the lane's chunk in the cell (this tile)
    const bool &in_cell, &full;

    // slab u of the cell in round slot `slot`: lane l's 16 B -> row
    // 8*(slot*SLABS + u) + l/8, byte 16*(l%8)
    __device__ __forceinline__ void put(int slot, int u, const u32x4& v) const {
        *reinterpret_cast<u32x4*>(stage + (8 * (slot * SLABS + u) + lane / 8) * PITCH + 16 * (lane % 8)) = v;
    }

    // One round over the staged image of `count` cells.  In the quarter-0 lane
    // of every chunk inside the cell: want = before(), issued ahead of the
    // table lookups (a verify round loads the expected sum there, an output
    // round returns 0), then after(sum, want) with the chunk's sum as it is
    // stored in memory (big-endian).
    template <class Before, class After>
    __device__ __forceinline__ void round(int count, Before&& before, After&& after) const {
        constexpr bool REFL = Spec::kReflected;
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        const bool live_c = in_cell && sir < count;
        uint32_t want = 0;
        if (live_c && qi == 0) want = before();
        uint32_t val = 0;
        if (full && sir < count) {
            uint32_t r = crcdev::quarter<SCHEME, REFL>(ctabs, stage + lane * PITCH, lane);
            if (qi < 3) r = crcdev::shift_quarter<SCHEME>(ctabs, qi, r);
            val = r;
        } else if (live_c && qi == 0) {
            const uint32_t len = uint32_t(cell_len - cbyte);
            uint32_t r = Spec::kInit;
            for (uint32_t b = 0; b < len; b++)
                r = crcdev::byte_step<REFL, BT::stride, BT::bswap>(ctabs + BT::off, r,
                                                                   stage[(lane + b / 128) * PITCH + (b % 128)]);
            val = r ^ Spec::kXorout;
        }
        val ^= __shfl_xor(val, 1);
        val ^= __shfl_xor(val, 2);
        if (live_c && qi == 0) after(__builtin_bswap32(full ? (val ^ kfinal) : val), want);
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }
};

}  // namespace
}  // namespace hec
