// Driver for hdfs_native::ec::Coder::reconstruct (csrc/hdfs_ec.hpp) on a
// host-only coder: RS(6,3), every pattern of 1..3 lost units (129), each
// rebuilt slot compared with the original stripe; then the `want` subset, a
// want on a present unit and too few survivors.  tests/test_reconstruct.py
// compiles and runs it.  Prints "ALL OK <patterns>" and exits 0 on success.
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
    const size_t k = 6, m = 3, n = k + m, len = 1000 + 17;
    Coder coder(k, m, HEC_DEVICE_HOST);
    std::vector<Bytes> stripe(k, Bytes(len));
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (Bytes& d : stripe)
        for (uint8_t& b : d) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            b = uint8_t(x >> 56);
        }
    for (Bytes& p : coder.encode(stripe)) stripe.push_back(std::move(p));

    int patterns = 0;
    for (unsigned mask = 1; mask < (1u << n); mask++) {
        if (__builtin_popcount(mask) > int(m)) continue;  // bit i set = unit i lost
        std::vector<std::optional<Bytes>> v(n);
        for (size_t i = 0; i < n; i++)
            if (!((mask >> i) & 1)) v[i] = stripe[i];
        coder.reconstruct(v);
        for (size_t i = 0; i < n; i++) EXPECT(v[i] && *v[i] == stripe[i], "pattern %#x unit %zu", mask, i);
        patterns++;
    }
    EXPECT(patterns == 129, "patterns %d", patterns);

    {  // want: one of two lost units; the other stays None
        std::vector<std::optional<Bytes>> v(stripe.begin(), stripe.end());
        v[2].reset();
        v[7].reset();
        const std::vector<size_t> want{7};
        coder.reconstruct(v, &want);
        EXPECT(v[7] && *v[7] == stripe[7], "want: parity unit 7");
        EXPECT(!v[2], "want: unit 2 was not asked for");
    }
    {  // want on a present unit
        std::vector<std::optional<Bytes>> v(stripe.begin(), stripe.end());
        v[2].reset();
        const std::vector<size_t> want{3};
        bool threw = false;
        try {
            coder.reconstruct(v, &want);
        } catch (const std::invalid_argument&) {
            threw = true;
        }
        EXPECT(threw, "want on a present unit must throw invalid_argument");
    }
    {  // four lost: not enough survivors
        std::vector<std::optional<Bytes>> v(stripe.begin(), stripe.end());
        for (size_t i : {0, 4, 6, 8}) v[i].reset();
        bool threw = false;
        try {
            coder.reconstruct(v);
        } catch (const hdfs_native::HdfsError& e) {
            threw = e.kind == hdfs_native::HdfsErrorKind::ErasureCodingError;
        }
        EXPECT(threw, "4 lost units must throw ErasureCodingError");
        EXPECT(!v[0] && !v[4] && !v[6] && !v[8], "nothing rebuilt on error");
    }
    {  // nothing lost: no work
        std::vector<std::optional<Bytes>> v(stripe.begin(), stripe.end());
        coder.reconstruct(v);
        for (size_t i = 0; i < n; i++) EXPECT(v[i] && *v[i] == stripe[i], "intact unit %zu", i);
    }
    if (fails) return 1;
    std::printf("ALL OK %d\n", patterns);
    return 0;
}
