// scrub_correct_host_check.cpp -- the host correction routine
// (hec::host::scrub_correct, hdfs-native_amd/csrc/host_gf.cpp) on its own, with
// a main of its own: this file and host_gf.cpp compile into one program, with
// -fsanitize=address,undefined where the sanitizer runtime is installed
// (tests/test_scrub_correct.py; no library is loaded and nothing is
// preloaded).  Every unit sits in a malloc block of exactly its length, so a
// read or a write past a unit, or past the routine's scratch, is a heap
// overrun.  For every ISA this CPU has, the shipped codecs and lengths that end
// before, on and after a vector width and the routine's 64 KiB block: a clean
// stripe, every unit corrupted at the first position, the last position and
// as a whole, two corrupt units -- each against a byte-at-a-time restatement
// of the definition below.  Prints "ALL OK <checks>" and exits 0 on success.
#include <cstdio>
#include <cstdlib>
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

// the definition, one byte at a time: the scrub's pair, the verdict, then
// e = scale * s_row XORed into the located unit.  Returns the unit, -1 or -2.
static int expect(const std::vector<uint8_t>& P, size_t k, size_t m, Units& u, uint64_t* ruled, uint64_t* bad) {
    *ruled = *bad = 0;
    const size_t len = u[0].size();
    std::vector<uint8_t> s(m);
    for (size_t b = 0; b < len; b++) {
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
    if (*bad == 0) return -1;
    const uint64_t cand = ~*ruled & ((uint64_t(1) << (k + m)) - 1);
    if (__builtin_popcountll(cand) != 1) return -2;
    const size_t t = size_t(__builtin_ctzll(cand));
    size_t row = t < k ? 0 : t - k;
    uint8_t scale = 1;
    if (t < k) {
        while (P[row * k + t] == 0) row++;
        for (int c = 1; c < 256; c++)
            if (kMul[P[row * k + t]][c] == 1) scale = uint8_t(c);
    }
    for (size_t b = 0; b < len; b++) {
        uint8_t sr = u[k + row][b];
        for (size_t i = 0; i < k; i++) sr ^= kMul[P[row * k + i]][u[i][b]];
        u[t][b] ^= kMul[scale][sr];
    }
    return int(t);
}

static void check(Isa isa, const std::vector<uint8_t>& P, const std::vector<uint64_t>& aff, size_t k, size_t m,
                  const Units& u, const Units* truth, int want_unit, const char* what) {
    const size_t len = u[0].size();
    // exact-size malloc blocks: the routine writes into these
    std::vector<uint8_t*> p;
    for (const auto& v : u) {
        uint8_t* q = static_cast<uint8_t*>(std::malloc(len));
        std::memcpy(q, v.data(), len);
        p.push_back(q);
    }
    uint64_t ruled = 1, bad = 1, want_ruled, want_bad;
    const int unit =
        hec::host::scrub_correct(isa, P.data(), (len & 1) ? aff.data() : nullptr, k, m, p.data(), len, &ruled, &bad);
    Units want = u;
    const int ref_unit = expect(P, k, m, want, &want_ruled, &want_bad);
    checks++;
    bool ok = unit == ref_unit && ruled == want_ruled && bad == want_bad && (want_unit == -3 || unit == want_unit);
    for (size_t i = 0; i < k + m; i++) {
        ok = ok && std::memcmp(p[i], want[i].data(), len) == 0;
        if (truth && unit >= 0) ok = ok && std::memcmp(p[i], (*truth)[i].data(), len) == 0;
        std::free(p[i]);
    }
    if (!ok) {
        std::printf("FAIL: %s isa %s k %zu m %zu len %zu: unit %d (%#llx, %llu) want %d/%d (%#llx, %llu)\n", what,
                    hec::host::isa_name(isa), k, m, len, unit, (unsigned long long)ruled, (unsigned long long)bad,
                    ref_unit, want_unit, (unsigned long long)want_ruled, (unsigned long long)want_bad);
        fails++;
    }
}

int main() {
    const Isa best = hec::host::best_isa();
    std::printf("best isa: %s\n", hec::host::isa_name(best));
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) kMul[x][y] = hec::gf_mul(uint8_t(x), uint8_t(y));
    std::mt19937 rng(0x5C2B0002u);
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
                const Units truth = u;
                check(isa, P, aff, k, m, u, &truth, -1, "clean");
                for (size_t t = 0; t < k + m; t++) {
                    // past a block: the first and the last data and parity units
                    if (len > 65536 && t != 0 && t != k - 1 && t != k && t != k + m - 1) continue;
                    const int want = m > 1 ? int(t) : -2;
                    u[t][0] ^= 0x20;
                    check(isa, P, aff, k, m, u, &truth, want, "first byte");
                    u = truth;
                    u[t][len - 1] ^= 0x07;
                    check(isa, P, aff, k, m, u, &truth, want, "last byte");
                    u = truth;
                    for (auto& b : u[t]) b = uint8_t(rng());
                    if (u[t] == truth[t]) u[t][0] ^= 1;
                    check(isa, P, aff, k, m, u, &truth, want, "random unit");
                    u = truth;
                }
                // two units at one position (m == 2: whatever the definition gives), then also at another
                u[0][len / 2] ^= 0x11;
                u[k + m - 1][len / 2] ^= 0x0F;
                check(isa, P, aff, k, m, u, nullptr, m == 2 ? -3 : -2, "two units, one position");
                u[1][0] ^= 0x80;
                check(isa, P, aff, k, m, u, nullptr, m == 1 ? -2 : (m == 2 || len == 1) ? -3 : -2, "two positions");
            }
        }
    }
    if (fails) return 1;
    std::printf("ALL OK %zu\n", checks);
    return 0;
}
