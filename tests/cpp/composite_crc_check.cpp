// composite_crc_check.cpp -- crc_compose.hpp's host part (the multiply, the
// powers, the geometry and the fold hec_composite_crc runs) compiled into a
// program of its own, so that it can run under AddressSanitizer + UBSan with
// no library to preload.  Every buffer is a malloc of the exact size; the CPU
// oracle's CRC over the actual bytes is the checker.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hdfs-native_amd/csrc/crc_compose.hpp"

extern "C" {
uint32_t orc_crc32c(const uint8_t* p, size_t n);
uint32_t orc_crc32_cksum(const uint8_t* p, size_t n);
void orc_chunk_checksum(int checksum_type, const uint8_t* p, size_t n, size_t bpc, uint8_t* out);
}

namespace {

using namespace hec::crc;

int g_failures = 0;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;

uint8_t next_byte() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint8_t(g_rng >> 32);
}

void expect(bool ok, const char* what, int kind, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    if (ok) return;
    g_failures++;
    std::printf("FAIL %s kind=%d (%llu %llu %llu %llu)\n", what, kind, (unsigned long long)a, (unsigned long long)b,
                (unsigned long long)c, (unsigned long long)d);
}

// a malloc of exactly n bytes (1 when n == 0, never dereferenced then)
uint8_t* exact(size_t n) {
    uint8_t* p = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    if (!p) std::abort();
    return p;
}

template <int KIND>
uint32_t oracle(const uint8_t* p, size_t n) {
    return KIND == kCrc32c ? orc_crc32c(p, n) : orc_crc32_cksum(p, n);
}
template <int KIND>
constexpr int proto_type() {
    return KIND == kCrc32c ? 2 : 1;  // ChecksumTypeProto
}

template <int KIND>
void check_concat() {
    const size_t edges[] = {0, 1, 511, 512, 513, 1300};
    for (size_t la : edges)
        for (size_t lb : edges) {
            uint8_t* buf = exact(la + lb);
            for (size_t i = 0; i < la + lb; i++) buf[i] = next_byte();
            const uint32_t got = concat<KIND>(oracle<KIND>(buf, la), oracle<KIND>(buf + la, lb), lb);
            expect(got == oracle<KIND>(buf, la + lb), "concat", KIND, la, lb, 0, 0);
            std::free(buf);
        }
    // 64-bit lengths: appending in two steps is appending the sum
    const uint64_t big[] = {0xFFFFFFFFull, 0x100000000ull, (uint64_t(1) << 40) + 3, 0x7FFFFFFFFFFFFFFFull};
    for (uint64_t n : big) {
        const uint32_t whole = xpow8<KIND>(n);
        const uint32_t parts = mulmod<KIND>(xpow8<KIND>(n - 12345), xpow8<KIND>(12345));
        expect(whole == parts, "xpow8 split", KIND, n, 0, 0, 0);
    }
}

template <int KIND>
void check_composite(size_t n, size_t k, size_t cell, size_t stripes, size_t bpc, uint64_t data_len) {
    Geometry g;
    if (!make_geometry(n, k, cell, stripes, bpc, data_len, &g)) {
        expect(false, "geometry", KIND, n, cell, stripes, data_len);
        return;
    }
    // cells, each an exact-size buffer; sums with exactly nck slots per cell
    const size_t cells = stripes * n;
    uint8_t** bytes = static_cast<uint8_t**>(std::malloc(cells * sizeof(uint8_t*)));
    size_t* lens = static_cast<size_t*>(std::malloc(cells * sizeof(size_t)));
    uint8_t* sums = exact(cells * g.nck * 4);
    std::memset(sums, 0xA5, cells * g.nck * 4);
    for (size_t s = 0; s < stripes; s++)
        for (size_t u = 0; u < n; u++) {
            const size_t i = s * n + u, len = s + 1 < stripes ? cell : size_t(g.len_last[u]);
            lens[i] = len;
            bytes[i] = exact(len);
            for (size_t b = 0; b < len; b++) bytes[i][b] = next_byte();
            const size_t nc = (len + bpc - 1) / bpc;
            uint8_t* tmp = exact(nc * 4);
            orc_chunk_checksum(proto_type<KIND>(), bytes[i], len, bpc, tmp);
            std::memcpy(sums + i * g.nck * 4, tmp, nc * 4);
            std::free(tmp);
        }
    uint8_t* cell_crcs = exact(cells * 4);
    uint8_t* unit_crcs = exact(n * 4);
    uint8_t* group_crc = exact(4);
    composite_host<KIND>(g, sums, cell_crcs, unit_crcs, group_crc);
    for (size_t i = 0; i < cells; i++)
        expect(load_be32(cell_crcs + 4 * i) == oracle<KIND>(bytes[i], lens[i]), "cell", KIND, n, cell, stripes, i);
    size_t logical = 0;
    for (size_t u = 0; u < n; u++) {
        size_t total = 0;
        for (size_t s = 0; s < stripes; s++) total += lens[s * n + u];
        uint8_t* cat = exact(total);
        size_t at = 0;
        for (size_t s = 0; s < stripes; s++) {
            if (lens[s * n + u]) std::memcpy(cat + at, bytes[s * n + u], lens[s * n + u]);
            at += lens[s * n + u];
        }
        expect(load_be32(unit_crcs + 4 * u) == oracle<KIND>(cat, total), "unit", KIND, n, cell, stripes, u);
        std::free(cat);
        if (u < k) logical += total;
    }
    uint8_t* cat = exact(logical);
    size_t at = 0;
    for (size_t s = 0; s < stripes; s++)
        for (size_t u = 0; u < k; u++) {
            if (lens[s * n + u]) std::memcpy(cat + at, bytes[s * n + u], lens[s * n + u]);
            at += lens[s * n + u];
        }
    expect(at == logical && (data_len == 0 || logical == data_len), "length", KIND, n, cell, stripes, logical);
    expect(load_be32(group_crc) == oracle<KIND>(cat, logical), "group", KIND, n, cell, stripes, data_len);
    std::free(cat);
    // each output alone, the others NULL
    uint8_t* alone = exact(cells * 4);
    composite_host<KIND>(g, sums, alone, nullptr, nullptr);
    expect(std::memcmp(alone, cell_crcs, cells * 4) == 0, "cells alone", KIND, n, cell, stripes, 0);
    composite_host<KIND>(g, sums, nullptr, alone, nullptr);
    expect(std::memcmp(alone, unit_crcs, n * 4) == 0, "units alone", KIND, n, cell, stripes, 0);
    composite_host<KIND>(g, sums, nullptr, nullptr, alone);
    expect(std::memcmp(alone, group_crc, 4) == 0, "group alone", KIND, n, cell, stripes, 0);
    std::free(alone);
    std::free(cell_crcs);
    std::free(unit_crcs);
    std::free(group_crc);
    for (size_t i = 0; i < cells; i++) std::free(bytes[i]);
    std::free(bytes);
    std::free(lens);
    std::free(sums);
}

template <int KIND>
void check_kind() {
    check_concat<KIND>();
    const size_t nk[][2] = {{9, 6}, {14, 10}, {5, 3}, {1, 1}};
    const size_t cell_bpc[][2] = {{16, 512}, {37, 256}, {528, 512}, {1000, 256}, {9232, 4096}};
    const size_t stripe_counts[] = {1, 3, 40};
    for (const auto& g : nk)
        for (const auto& cb : cell_bpc)
            for (size_t stripes : stripe_counts) {
                const size_t n = g[0], k = g[1], cell = cb[0], bpc = cb[1];
                if (stripes == 40 && cell > 1000) continue;  // the larger cells at 1 and 3 stripes
                const uint64_t before = uint64_t(stripes - 1) * k * cell;
                const uint64_t lens[] = {0, uint64_t(stripes) * k * cell, before + 1,
                                         before + (k / 2 ? k / 2 : 1) * cell,
                                         before + (k >= 3 ? cell : 0) + (cell / 2 ? cell / 2 : 1)};
                for (uint64_t data_len : lens) check_composite<KIND>(n, k, cell, stripes, bpc, data_len);
            }
    Geometry g;
    expect(!make_geometry(0, 0, 16, 1, 16, 0, &g) && !make_geometry(65, 6, 16, 1, 16, 0, &g) &&
               !make_geometry(9, 10, 16, 1, 16, 0, &g) && !make_geometry(9, 6, 0, 1, 16, 0, &g) &&
               !make_geometry(9, 6, 16, 1, 0, 0, &g) && !make_geometry(9, 6, 16, 2, 16, 96, &g) &&
               !make_geometry(9, 6, 16, 2, 16, 193, &g) && !make_geometry(9, 6, 16, 0, 16, 1, &g) &&
               !make_geometry(9, 6, SIZE_MAX / 2, 8, 16, 0, &g),
           "geometry refusals", KIND, 0, 0, 0, 0);
}

}  // namespace

int main() {
    check_kind<kCrc32c>();
    check_kind<kCksum>();
    if (g_failures) {
        std::printf("%d FAILURES\n", g_failures);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
