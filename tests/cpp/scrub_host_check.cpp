// scrub_host_check.cpp -- the host scrub routine (hec::host::scrub,
// hdfs-native_amd/csrc/host_gf.cpp) on its own, with a main of its own: this
// file and host_gf.cpp compile into one program, with
// -fsanitize=address,undefined where the sanitizer runtime is installed
// (tests/test_scrub.py; no library is loaded and nothing is preloaded).
// Every unit is an exact-length heap buffer, so a read past a unit or past the
// routine's scratch is a heap overrun.  For every ISA this CPU has, the
// shipped codecs and lengths that end before, on and after a vector width and
// the routine's 64 KiB block: a clean stripe, one flipped bit per unit at the
// first / last / block-edge positions, a wholly random unit, two corrupt
// units -- each against a byte-at-a-time restatement below.
// Prints "ALL OK <checks>" and exits 0 on success.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../hdfs-native_amd/csrc/gf256.hpp"
#include "../../hdfs-native_amd/csrc/host_gf.hpp"

using hec::host::Isa;
typedef std::vector<std::vector<uint8_t>> Units;

static int fails = 0;
static size_t checks = 0;

static uint8_t kMul[256][256];  // the field's product table, filled by main

// the definition, one byte at a time: syndromes, then every 2x2 minor
static void expect(const std::vector<uint8_t>& P, size_t k, size_t m, const Units& u, uint64_t* ruled, uint64_t* bad) {
    *ruled = *bad = 0;
    std::vector<uint8_t> s(m);
    for (size_t b = 0; b < u[0].size(); b++) {
        uint8_t any = 0;
        for (size_t j = 0; j < m; j++) {
            s[j] = u[k + j][b];
            for (size_t i = 0; i < k; i++) s[j] ^= kMul[P[j * k + i]][u[i][b]];
            any |= s[j];
        }
        if (!any) continue;
        ++*bad;
        for (size_t t = 0; t < k + m; t++)
            for (size_t i = 0; i < m; i++)
                for (size_t j = i + 1; j < m; j++) {
                    const uint8_t hi = t < k ? P[i * k + t] : uint8_t(i == t - k);
                    const uint8_t hj = t < k ? P[j * k + t] : uint8_t(j == t - k);
                    if (kMul[s[i]][hj] != kMul[s[j]][hi]) *ruled |= uint64_t(1) << t;
                }
    }
}

static void check(Isa isa, const std::vector<uint8_t>& P, const std::vector<uint64_t>& aff, size_t k, size_t m,
                  const Units& u, const char* what, size_t len) {
    std::vector<const uint8_t*> p;
    for (const auto& v : u) p.push_back(v.data());
    uint64_t ruled = 1, bad = 1, want_ruled, want_bad;
    hec::host::scrub(isa, P.data(), (len & 1) ? aff.data() : nullptr, k, m, p.data(), len, &ruled, &bad);
    expect(P, k, m, u, &want_ruled, &want_bad);
    checks++;
    if (ruled != want_ruled || bad != want_bad) {
        std::printf("FAIL: %s isa %s k %zu m %zu len %zu: (%#llx, %llu) want (%#llx, %llu)\n", what,
                    hec::host::isa_name(isa), k, m, len, (unsigned long long)ruled, (unsigned long long)bad,
                    (unsigned long long)want_ruled, (unsigned long long)want_bad);
        fails++;
    }
}

int main() {
    const Isa best = hec::host::best_isa();
    std::printf("best isa: %s\n", hec::host::isa_name(best));
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) kMul[x][y] = hec::gf_mul(uint8_t(x), uint8_t(y));
    std::mt19937 rng(0x5C2B0001u);
    const size_t lens[] = {1, 15, 16, 17, 64, 4099, 65536 + 17};
    struct Codec {
        const char* name;
        size_t k, m;
    };
    const Codec codecs[] = {{"rs", 3, 2}, {"rs", 6, 3}, {"rs", 10, 4}, {"xor", 5, 1}, {"rs-legacy", 6, 3}};
    for (int isa_i = 0; isa_i <= int(best); isa_i++) {
        const Isa isa = Isa(isa_i);
        for (const Codec& c : codecs) {
            const size_t k = c.k, m = c.m;
            const std::vector<uint8_t> C = !std::strcmp(c.name, "xor")         ? hec::gen_xor_matrix(k)
                                           : !std::strcmp(c.name, "rs-legacy") ? hec::gen_rs_legacy_matrix(k, m)
                                                                               : hec::gen_rs_matrix(k, m);
            const std::vector<uint8_t> P(C.begin() + k * k, C.end());
            const std::vector<uint64_t> aff = hec::host::affine_matrices(P.data(), P.size());
            for (size_t len : lens) {
                Units u(k + m, std::vector<uint8_t>(len));
                for (size_t i = 0; i < k; i++)
                    for (auto& b : u[i]) b = uint8_t(rng());
                for (size_t j = 0; j < m; j++)
                    for (size_t b = 0; b < len; b++) {
                        uint8_t v = 0;
                        for (size_t i = 0; i < k; i++) v ^= hec::gf_mul(P[j * k + i], u[i][b]);
                        u[k + j][b] = v;
                    }
                check(isa, P, aff, k, m, u, "clean", len);
                for (size_t t = 0; t < k + m; t++)
                    for (size_t pos : {size_t(0), len - 1, size_t(65535), size_t(65536)}) {
                        // past a block: the first and the last unit, around the block edge and at the end
                        if (len > 65535 && ((t != 0 && t != k + m - 1) || pos == 0)) continue;
                        if (pos >= len) continue;
                        u[t][pos] ^= 0x20;
                        check(isa, P, aff, k, m, u, "one bit", len);
                        u[t][pos] ^= 0x20;
                    }
                {  // a wholly random unit
                    const size_t t = rng() % (k + m);
                    const std::vector<uint8_t> keep = u[t];
                    for (auto& b : u[t]) b = uint8_t(rng());
                    check(isa, P, aff, k, m, u, "random unit", len);
                    u[t] = keep;
                }
                // two units at one position, then also at another
                u[0][len / 2] ^= 0x11;
                u[k + m - 1][len / 2] ^= 0x0F;
                check(isa, P, aff, k, m, u, "two units, one position", len);
                u[1][0] ^= 0x80;
                check(isa, P, aff, k, m, u, "two positions", len);
            }
        }
    }
    if (fails) return 1;
    std::printf("ALL OK %zu\n", checks);
    return 0;
}
