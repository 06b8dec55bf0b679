// Driver for hdfs_native::ec::Coder::scrub_degraded (csrc/hdfs_ec.hpp) on a
// host-only coder: RS(6,3), every single loss with a clean stripe and with one
// flipped bit in every present unit (72 cases, each LOCATED at that unit with
// the lost unit's bit set), two units lost (e = 1: AMBIGUOUS), three lost
// (unchecked: CLEAN whatever the bytes), nothing lost (scrub's own result), and
// the argument checks.  tests/test_scrub_degraded.py compiles and runs it.
// Prints "ALL OK <cases>" and exits 0 on success.
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <vector>

#include "../../hdfs-native_amd/csrc/hdfs_ec.hpp"

using hdfs_native::ec::Bytes;
using hdfs_native::ec::Coder;

static int fails = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAIL: ");        \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            fails++;                      \
        }                                 \
    } while (0)

int main() {
    const size_t k = 6, m = 3, n = k + m, len = 4099;
    const uint64_t full = (uint64_t(1) << n) - 1;
    Coder coder(k, m, HEC_DEVICE_HOST);
    std::vector<Bytes> stripe(k, Bytes(len));
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (Bytes& d : stripe)
        for (uint8_t& b : d) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            b = uint8_t(x >> 56);
        }
    for (Bytes& p : coder.encode(stripe)) stripe.push_back(std::move(p));
    auto without = [&](const std::vector<Bytes>& v, std::initializer_list<size_t> lost) {
        std::vector<std::optional<Bytes>> u(v.begin(), v.end());
        for (size_t t : lost) u[t].reset();
        return u;
    };

    int cases = 0;
    for (size_t lost = 0; lost < n; lost++) {
        const Coder::ScrubResult clean = coder.scrub_degraded(without(stripe, {lost}));
        EXPECT(clean.ruled_out == 0 && clean.bad_bytes == 0 && clean.verdict() == HEC_SCRUB_CLEAN, "lost %zu: clean", lost);
        for (size_t t = 0; t < n; t++) {
            if (t == lost) continue;
            std::vector<Bytes> v = stripe;
            v[t][(t * 977 + lost) % len] ^= 0x10;
            const Coder::ScrubResult r = coder.scrub_degraded(without(v, {lost}));
            EXPECT(r.ruled_out == (full & ~(uint64_t(1) << t)) && r.bad_bytes == 1, "lost %zu unit %zu: %#llx %llu", lost,
                   t, (unsigned long long)r.ruled_out, (unsigned long long)r.bad_bytes);
            EXPECT(r.verdict() == HEC_SCRUB_LOCATED && r.unit && *r.unit == t, "lost %zu unit %zu: verdict", lost, t);
            cases++;
        }
    }
    {  // e = 1: a bad position, nothing located; the lost units are ruled out
        std::vector<Bytes> v = stripe;
        v[4][9] ^= 1;
        const Coder::ScrubResult r = coder.scrub_degraded(without(v, {2, 7}));
        EXPECT(r.ruled_out == ((uint64_t(1) << 2) | (uint64_t(1) << 7)) && r.bad_bytes == 1 &&
                   r.verdict() == HEC_SCRUB_AMBIGUOUS && !r.unit,
               "two lost: %#llx %llu", (unsigned long long)r.ruled_out, (unsigned long long)r.bad_bytes);
    }
    {  // e = 0: unchecked
        std::vector<Bytes> v = stripe;
        v[4][9] ^= 1;
        const Coder::ScrubResult r = coder.scrub_degraded(without(v, {0, 5, 8}));
        EXPECT(r.ruled_out == 0 && r.bad_bytes == 0 && r.verdict() == HEC_SCRUB_CLEAN, "three lost: unchecked");
    }
    {  // nothing lost: scrub's own result
        std::vector<Bytes> v = stripe;
        v[1][7] ^= 1;
        v[8][2000] ^= 0x80;
        const Coder::ScrubResult a = coder.scrub(v), b = coder.scrub_degraded(without(v, {}));
        EXPECT(a.ruled_out == b.ruled_out && a.bad_bytes == b.bad_bytes && b.verdict() == HEC_SCRUB_MULTIPLE,
               "nothing lost equals scrub");
    }
    {  // a slot short of the stripe, units of unequal length
        bool threw = false;
        std::vector<std::optional<Bytes>> u = without(stripe, {3});
        u.pop_back();
        try {
            coder.scrub_degraded(u);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw, "eight slots must throw invalid_argument");
        threw = false;
        u = without(stripe, {3});
        u[5]->pop_back();
        try {
            coder.scrub_degraded(u);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw, "unequal lengths must throw invalid_argument");
    }
    {  // the device call on a host-only coder
        bool threw = false;
        std::vector<const uint8_t*> ptrs(n);
        for (size_t i = 0; i < n; i++) ptrs[i] = stripe[i].data();
        hec_scrub_result_t res{};
        try {
            coder.scrub_device_mixed(ptrs, std::vector<size_t>(n, len), std::vector<uint64_t>(1, full), len, &res, nullptr,
                                     0);
        } catch (const hdfs_native::HdfsError& e) {
            threw = e.kind == hdfs_native::HdfsErrorKind::Device;
        }
        EXPECT(threw, "scrub_device_mixed on a host-only coder must throw a Device error");
        EXPECT(coder.scrub_mixed_workspace_size(16) > 0, "workspace size");
    }
    if (fails) return 1;
    std::printf("ALL OK %d\n", cases);
    return 0;
}
