// encode_rows_check.cpp -- the host side of hec_encode_crc_rows_device*
// (hdfs-native_amd/csrc/ec_capi.cpp: write_encode_rows_image,
// encode_rows_workspace and the argument checks that come before the coder's
// device), in a stand-alone program under AddressSanitizer + UBSan.  The
// library's translation unit is included, so the code checked is the code the
// library compiles; only host-only coders (HEC_DEVICE_HOST) are created and no
// HIP call is made.
//
// Per batch the lengths image is written into a malloc'd buffer of exactly the
// advertised workspace bytes filled with 0xCD and read back: one u64 per
// stripe, a 0 entry rewritten to k * cell_len, nothing behind the end.
// Run by tests/test_encode_crc_rows.py (CPU).
#include "../../hdfs-native_amd/csrc/ec_capi.cpp"

#include <cstdarg>
#include <random>

namespace {

[[noreturn]] void die(const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    std::printf("encode_rows_check: FAIL %s\n", msg);
    std::fflush(stdout);
    _exit(1);
}

size_t g_batches = 0;

void check_batch(hec_coder* c, const std::vector<uint64_t>& bytes, size_t cell_len, const char* what) {
    const size_t S = bytes.size();
    const uint64_t full = uint64_t(c->k) * cell_len;
    const size_t advertised = hec_encode_crc_rows_mixed_workspace_size(c, S);
    if (advertised < 8 * S || advertised % 8 != 0) die("%s: workspace of %zu bytes for %zu stripes", what, advertised, S);
    if (advertised != encode_rows_workspace(S)) die("%s: the call checks another size than it advertises", what);
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(advertised));
    if (!buf) die("%s: malloc", what);
    std::memset(buf, 0xCD, advertised);
    const size_t need = write_encode_rows_image(buf, bytes.data(), S, c->k, cell_len);
    if (need != 8 * S || need > advertised) die("%s: image of %zu bytes, %zu advertised", what, need, advertised);
    for (size_t s = 0; s < S; s++) {
        uint64_t got;
        std::memcpy(&got, buf + 8 * s, 8);
        const uint64_t want = bytes[s] == 0 ? full : bytes[s];
        if (got != want)
            die("%s: stripe %zu holds %llu, want %llu", what, s, (unsigned long long)got, (unsigned long long)want);
    }
    for (size_t i = need; i < advertised; i++)
        if (buf[i] != 0xCD) die("%s: byte %zu behind the image was written", what, i);
    std::free(buf);
    // a host-only coder is refused as such, after the lengths were accepted
    const int rc = hec_encode_crc_rows_device_mixed(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, nullptr, bytes.data(),
                                                    cell_len, S, 512, nullptr, nullptr, 0, nullptr);
    if (rc != HEC_ERR_DEVICE) die("%s: mixed call on a host-only coder: status %d", what, rc);
    g_batches++;
}

int uniform(hec_coder* c, int type, size_t cell_len, size_t stripes, size_t bpc, uint64_t data_len) {
    return hec_encode_crc_rows_device(c, type, nullptr, nullptr, nullptr, nullptr, cell_len, stripes, bpc, data_len,
                                      nullptr, nullptr);
}

int mixed(hec_coder* c, int type, const uint64_t* bytes, size_t cell_len, size_t stripes, size_t bpc) {
    return hec_encode_crc_rows_device_mixed(c, type, nullptr, nullptr, nullptr, nullptr, bytes, cell_len, stripes, bpc,
                                            nullptr, nullptr, 0, nullptr);
}

void check_coder(const char* codec, size_t k, size_t m) {
    hec_coder_t* c = nullptr;
    if (hec_coder_create_codec(codec, k, m, HEC_DEVICE_HOST, &c) != HEC_OK || !c)
        die("hec_coder_create_codec(%s, %zu, %zu)", codec, k, m);
    const size_t cell_len = 9232;
    const uint64_t full = uint64_t(k) * cell_len;
    std::mt19937_64 rng(3000 * k + m);
    size_t last = 0;
    for (size_t S : {size_t(1), size_t(7), size_t(1024), size_t(100000)}) {
        const size_t adv = hec_encode_crc_rows_mixed_workspace_size(c, S);
        if (adv < last) die("workspace size shrinks at %zu stripes", S);
        last = adv;
        for (int variant = 0; variant < 3; variant++) {  // all full, all short, alternating
            std::vector<uint64_t> bytes(S);
            for (size_t s = 0; s < S; s++) {
                const bool is_short = variant == 1 || (variant == 2 && s % 2 == 0);
                bytes[s] = is_short ? 1 + rng() % (full - 1) : (s % 3 == 0 ? full : 0);
            }
            char what[96];
            std::snprintf(what, sizeof(what), "%s(%zu,%zu) S=%zu variant %d", codec, k, m, S, variant);
            check_batch(c, bytes, cell_len, what);
        }
    }
    // the argument checks that come before the coder's device
    const int bad = HEC_ERR_INVALID_ARG, dev = HEC_ERR_DEVICE, t = HEC_CHECKSUM_CRC32C;
    uint64_t two[2] = {full + 1, 0};
    if (mixed(c, t, two, cell_len, 2, 512) != bad) die("stripe_bytes above k * cell_len");
    two[0] = 1, two[1] = uint64_t(1) << 63;
    if (mixed(c, t, two, cell_len, 2, 512) != bad) die("stripe_bytes of 2^63");
    two[1] = full - 1;
    if (mixed(c, HEC_CHECKSUM_CRC32, two, cell_len, 2, 100) != dev) die("a valid mixed call on a host-only coder");
    if (mixed(c, t, nullptr, cell_len, 2, 512) != dev) die("stripe_bytes NULL on a host-only coder");
    if (mixed(c, t, nullptr, cell_len, 0, 512) != dev) die("no stripes on a host-only coder");
    for (int type : {int(HEC_CHECKSUM_NULL), 7}) {
        if (uniform(c, type, cell_len, 2, 512, 0) != bad || mixed(c, type, nullptr, cell_len, 2, 512) != bad)
            die("checksum type %d", type);
    }
    if (uniform(c, t, 0, 2, 512, 0) != bad || mixed(c, t, nullptr, 0, 2, 512) != bad) die("cell_len of 0");
    if (uniform(c, t, cell_len, 2, 0, 0) != bad || mixed(c, t, nullptr, cell_len, 2, 0) != bad) die("chunks of 0 bytes");
    if (uniform(c, t, cell_len, 2, 512, full) != bad) die("data_len that ends the last stripe but one");
    if (uniform(c, t, cell_len, 2, 512, 1) != bad) die("data_len inside the first of two stripes");
    if (uniform(c, t, cell_len, 2, 512, 2 * full + 1) != bad) die("data_len past the group");
    if (uniform(c, t, cell_len, 0, 512, 5) != bad) die("data_len without stripes");
    for (uint64_t data_len : {uint64_t(0), 2 * full, full + 1, 2 * full - 1})
        if (uniform(c, HEC_CHECKSUM_CRC32, cell_len, 2, 512, data_len) != dev)
            die("data_len %llu on a host-only coder", (unsigned long long)data_len);
    if (uniform(c, t, cell_len, 0, 512, 0) != dev) die("no stripes on a host-only coder");
    if (uniform(nullptr, t, cell_len, 2, 512, 0) != bad || mixed(nullptr, t, nullptr, cell_len, 2, 512) != bad)
        die("a NULL coder");
    if (hec_encode_crc_rows_mixed_workspace_size(nullptr, 16) != 0) die("workspace size of a NULL coder");
    hec_coder_destroy(c);
}

}  // namespace

int main() {
    check_coder("rs", 3, 2);
    check_coder("rs", 6, 3);
    check_coder("rs", 10, 4);
    check_coder("rs", 12, 6);
    check_coder("rs-legacy", 6, 3);
    check_coder("xor", 2, 1);
    std::printf("encode_rows_check: ok, %zu batches\n", g_batches);
    return 0;
}
