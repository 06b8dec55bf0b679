// Driver for hdfs_native::ec::Coder::scrub (csrc/hdfs_ec.hpp) on a host-only
// coder: RS(6,3), a clean stripe, one flipped bit in every unit at the first
// and the last position (18 cases, each LOCATED at that unit), two corrupt
// units at two positions and at one position (MULTIPLE), and the argument
// checks.  tests/test_scrub.py compiles and runs it.  Prints "ALL OK <cases>"
// and exits 0 on success.
#include <cstdio>
#include <cstdlib>
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

    {
        const Coder::ScrubResult r = coder.scrub(stripe);
        EXPECT(r.ruled_out == 0 && r.bad_bytes == 0 && r.verdict() == HEC_SCRUB_CLEAN && !r.unit, "clean stripe");
    }
    int cases = 0;
    for (size_t t = 0; t < n; t++)
        for (size_t pos : {size_t(0), len - 1}) {
            std::vector<Bytes> v = stripe;
            v[t][pos] ^= 0x10;
            const Coder::ScrubResult r = coder.scrub(v);
            EXPECT(r.ruled_out == (full & ~(uint64_t(1) << t)) && r.bad_bytes == 1, "unit %zu pos %zu: %#llx %llu", t,
                   pos, (unsigned long long)r.ruled_out, (unsigned long long)r.bad_bytes);
            EXPECT(r.verdict() == HEC_SCRUB_LOCATED && r.unit && *r.unit == t, "unit %zu pos %zu: verdict", t, pos);
            cases++;
        }
    {  // two units, two positions
        std::vector<Bytes> v = stripe;
        v[1][7] ^= 1;
        v[8][2000] ^= 0x80;
        const Coder::ScrubResult r = coder.scrub(v);
        EXPECT(r.ruled_out == full && r.bad_bytes == 2 && r.verdict() == HEC_SCRUB_MULTIPLE && !r.unit,
               "two units, two positions");
    }
    {  // two units, one position: m = 3 still tells them from one
        std::vector<Bytes> v = stripe;
        v[0][100] ^= 3;
        v[5][100] ^= 0x41;
        const Coder::ScrubResult r = coder.scrub(v);
        EXPECT(r.ruled_out == full && r.bad_bytes == 1 && r.verdict() == HEC_SCRUB_MULTIPLE, "two units, one position");
    }
    {  // a unit short of the stripe, units of unequal length
        bool threw = false;
        try {
            coder.scrub(std::vector<Bytes>(stripe.begin(), stripe.end() - 1));
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw, "eight units must throw invalid_argument");
        threw = false;
        std::vector<Bytes> v = stripe;
        v[3].pop_back();
        try {
            coder.scrub(v);
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
            coder.scrub_device(ptrs, std::vector<size_t>(n, len), len, 1, &res);
        } catch (const hdfs_native::HdfsError& e) {
            threw = e.kind == hdfs_native::HdfsErrorKind::Device;
        }
        EXPECT(threw, "scrub_device on a host-only coder must throw a Device error");
    }
    if (fails) return 1;
    std::printf("ALL OK %d\n", cases);
    return 0;
}
