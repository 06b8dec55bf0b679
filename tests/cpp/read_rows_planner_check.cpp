// read_rows_planner_check.cpp -- the host-side planning of
// hec_read_crc_rows_device_mixed (hdfs-native_amd/csrc/ec_capi.cpp:
// read_rows_group, read_rows_plan, read_rows_layout, write_read_rows_image,
// read_rows_workspace) against a reference built straight from the masks and
// lengths, in a stand-alone program under AddressSanitizer + UBSan.  The
// library's translation unit is included, so the code checked is the code the
// library compiles; only host-only coders (HEC_DEVICE_HOST) are created and no
// HIP call is made.
//
// Per batch: the groups in the order their masks first appear, each group's
// survivors (the first k present units) and lost data units, its stripe list
// and the stripes' lengths (0 rewritten to k * cell_len) are compared with the
// reference; the lost units' rows are checked against the encoding matrix
// (row . C[survivors] = the unit vector of the lost unit); and the image is
// written into a malloc'd buffer of exactly the advertised workspace bytes
// filled with 0xCD, then read back through the documented layout.
// Run by tests/test_read_crc_rows.py (CPU).
#include "../../hdfs-native_amd/csrc/ec_capi.cpp"

#include <cstdarg>
#include <map>
#include <random>

namespace {

[[noreturn]] void die(const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    std::printf("read_rows_planner_check: FAIL %s\n", msg);
    std::fflush(stdout);
    _exit(1);
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

size_t g_batches = 0, g_groups = 0, g_no_loss = 0, g_parity_only = 0, g_rows = 0;

// One batch: present masks and lengths (bytes_null: the array is NULL).
void check_batch(hec_coder* c, const std::vector<uint64_t>& present, const std::vector<uint64_t>& bytes, bool bytes_null,
                 size_t cell_len, const char* what) {
    const size_t k = c->k, m = c->m, n = k + m, S = present.size();
    const uint64_t all = (uint64_t(1) << n) - 1;
    const uint64_t full_bytes = uint64_t(k) * cell_len;

    // the reference: masks in the order they first appear, each with its
    // stripes ascending and their lengths
    struct RefGroup {
        uint64_t mask;
        std::vector<uint32_t> list;
        std::vector<uint64_t> lens;
    };
    std::map<uint64_t, size_t> ids;
    std::vector<RefGroup> ref;
    for (size_t s = 0; s < S; s++) {
        const uint64_t mask = present[s] & all;
        auto it = ids.find(mask);
        if (it == ids.end()) {
            it = ids.emplace(mask, ref.size()).first;
            ref.push_back(RefGroup{mask, {}, {}});
        }
        const uint64_t r = bytes_null ? 0 : bytes[s];
        ref[it->second].list.push_back(uint32_t(s));
        ref[it->second].lens.push_back(r == 0 ? full_bytes : r);
    }

    // the library, called as hec_read_crc_rows_device_mixed calls it
    ReadRowsPlan plan;
    const int rc = read_rows_plan(c, present.data(), bytes_null ? nullptr : bytes.data(), S, cell_len, &plan);
    if (rc != HEC_OK) die("%s: read_rows_plan status %d", what, rc);
    if (plan.groups.size() != ref.size()) die("%s: %zu groups, reference %zu", what, plan.groups.size(), ref.size());
    if (plan.list.size() != S || plan.bytes.size() != S) die("%s: %zu list entries for %zu stripes", what, plan.list.size(), S);
    size_t at = 0;
    for (size_t gi = 0; gi < ref.size(); gi++) {
        const ReadRowsGroup& g = plan.groups[gi];
        const RefGroup& rg = ref[gi];
        if (g.mask != rg.mask) die("%s: group %zu has mask %#llx, reference %#llx", what, gi, (unsigned long long)g.mask,
                                   (unsigned long long)rg.mask);
        if (g.first != at || g.count != rg.list.size())
            die("%s: group %zu covers [%zu, +%zu), reference [%zu, +%zu)", what, gi, g.first, g.count, at, rg.list.size());
        for (size_t i = 0; i < rg.list.size(); i++)
            if (plan.list[at + i] != rg.list[i] || plan.bytes[at + i] != rg.lens[i])
                die("%s: group %zu entry %zu is stripe %u with %llu bytes, reference %u with %llu", what, gi, i,
                    plan.list[at + i], (unsigned long long)plan.bytes[at + i], rg.list[i], (unsigned long long)rg.lens[i]);
        at += rg.list.size();
        // survivors: the first k present units; lost: the absent data units
        std::vector<uint8_t> surv, lost;
        for (size_t u = 0; u < n && surv.size() < k; u++)
            if ((rg.mask >> u) & 1) surv.push_back(uint8_t(u));
        for (size_t u = 0; u < k; u++)
            if (!((rg.mask >> u) & 1)) lost.push_back(uint8_t(u));
        if (g.survivors != surv) die("%s: group %zu (mask %#llx): survivors differ", what, gi, (unsigned long long)rg.mask);
        if (g.lost != lost) die("%s: group %zu (mask %#llx): lost data units differ", what, gi, (unsigned long long)rg.mask);
        if (lost.empty()) {
            if (g.plan) die("%s: group %zu loses no data unit and has a plan", what, gi);
            for (size_t i = 0; i < k; i++)
                if (g.survivors[i] != i) die("%s: group %zu loses no data unit and reads unit %u", what, gi, g.survivors[i]);
            g_no_loss++;
            g_parity_only += rg.mask != all;
            continue;
        }
        // row j of the plan rebuilds lost[j]: row . C[survivors] = e_lost[j]
        if (!g.plan || g.plan->matrix.size() < lost.size() * k) die("%s: group %zu has no rows", what, gi);
        for (size_t j = 0; j < lost.size(); j++) {
            for (size_t col = 0; col < k; col++) {
                uint8_t v = 0;
                for (size_t i = 0; i < k; i++) v ^= hec::gf_mul(g.plan->matrix[j * k + i], c->enc[size_t(surv[i]) * k + col]);
                if (v != (col == lost[j] ? 1 : 0))
                    die("%s: group %zu row %zu does not rebuild unit %u (column %zu is %u)", what, gi, j, lost[j], col, v);
            }
            g_rows++;
        }
    }

    // the image, in a buffer of exactly the advertised size
    const size_t advertised = hec_read_crc_rows_mixed_workspace_size(c, S);
    const ReadRowsLayout w = read_rows_layout(S);
    const size_t bytes_pos = up256(S * 4), need = bytes_pos + S * 8;  // the documented layout, restated
    if (w.bytes_pos != bytes_pos || w.need != need) die("%s: layout (%zu %zu), reference (%zu %zu)", what, w.bytes_pos, w.need, bytes_pos, need);
    if (advertised != need) die("%s: %zu bytes advertised, the image takes %zu", what, advertised, need);
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(advertised));
    std::memset(buf, 0xCD, advertised);
    write_read_rows_image(buf, plan, w);
    for (size_t i = S * 4; i < bytes_pos; i++)
        if (buf[i] != 0) die("%s: pad byte %zu is %#x", what, i, buf[i]);
    at = 0;
    for (size_t gi = 0; gi < ref.size(); gi++) {
        if (std::memcmp(buf + at * 4, ref[gi].list.data(), ref[gi].list.size() * 4) != 0)
            die("%s: group %zu's stripes differ in the image", what, gi);
        if (std::memcmp(buf + bytes_pos + at * 8, ref[gi].lens.data(), ref[gi].lens.size() * 8) != 0)
            die("%s: group %zu's lengths differ in the image", what, gi);
        at += ref[gi].list.size();
    }
    std::free(buf);
    g_batches++;
    g_groups += ref.size();
}

void check_shape(const char* codec, size_t k, size_t m) {
    hec_coder_t* c = nullptr;
    if (hec_coder_acquire(codec, k, m, HEC_DEVICE_HOST, &c) != HEC_OK || !c) die("hec_coder_acquire(%s, %zu, %zu)", codec, k, m);
    const size_t n = k + m, cell_len = 9232;
    const uint64_t all = (uint64_t(1) << n) - 1, full_bytes = uint64_t(k) * cell_len;
    std::mt19937_64 rng(1000 * k + m);
    // every mask with at least k units up to 10 units, a seeded sample of them above
    std::vector<uint64_t> masks;
    if (n <= 10) {
        for (uint64_t mask = 0; mask <= all; mask++)
            if (size_t(__builtin_popcountll(mask)) >= k) masks.push_back(mask);
    } else {
        masks.push_back(all);
        for (size_t u = 0; u < n; u++) masks.push_back(all & ~(uint64_t(1) << u));
        masks.push_back(all & ~(((uint64_t(1) << m) - 1) << k));  // every parity unit lost
        for (int i = 0; i < 200; i++) {
            uint64_t mask = all;
            const size_t lose = 1 + rng() % m;
            while (size_t(__builtin_popcountll(all & ~mask)) < lose) mask &= ~(uint64_t(1) << (rng() % n));
            masks.push_back(mask);
        }
    }
    const uint64_t fixed[] = {0, full_bytes, 1, cell_len, cell_len + 1, full_bytes - 1};
    size_t last = 0;
    for (size_t S : {size_t(1), size_t(7), masks.size() + 5}) {
        const size_t adv = hec_read_crc_rows_mixed_workspace_size(c, S);
        if (adv < last || adv < S * 12) die("workspace size %zu at %zu stripes", adv, S);
        last = adv;
        for (int variant = 0; variant < 4; variant++) {
            std::vector<uint64_t> present(S), bytes(S);
            for (size_t s = 0; s < S; s++) {
                // variant 0, 1: every mask in turn; 2, 3: drawn, so that groups interleave
                present[s] = masks[variant < 2 ? (s + variant) % masks.size() : rng() % masks.size()];
                if (variant == 3 && s % 4 == 0) present[s] |= uint64_t(0xA5) << n;  // bits past k + m are ignored
                const uint64_t pick = rng() % 9;
                bytes[s] = variant == 1 ? 0 : pick < 6 ? fixed[pick] : 1 + rng() % full_bytes;
            }
            char what[96];
            std::snprintf(what, sizeof(what), "%s(%zu,%zu) S=%zu variant %d", codec, k, m, S, variant);
            check_batch(c, present, bytes, variant == 0, cell_len, what);
        }
    }
    // fewer than k units: the status of the plan, nothing planned behind it
    {
        ReadRowsPlan plan;
        uint64_t present[2] = {all, (uint64_t(1) << (k - 1)) - 1};
        const int rc = read_rows_plan(c, present, nullptr, 2, cell_len, &plan);
        if (rc != HEC_ERR_NOT_ENOUGH_SHARDS) die("%s(%zu,%zu): k - 1 units present: status %d", codec, k, m, rc);
    }
    // what is refused before the coder's device is looked at, and the device after it
    {
        uint64_t present = all & ~uint64_t(1), bytes = full_bytes + 1, ok_bytes = 5;
        int rc = hec_read_crc_rows_device_mixed(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, 0, &present, &bytes,
                                                cell_len, 1, 512, nullptr, nullptr, nullptr, 0, nullptr);
        if (rc != HEC_ERR_INVALID_ARG) die("stripe_bytes above k * cell_len: status %d", rc);
        rc = hec_read_crc_rows_device_mixed(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, full_bytes - 1, &present,
                                            &ok_bytes, cell_len, 1, 512, nullptr, nullptr, nullptr, 0, nullptr);
        if (rc != HEC_ERR_INVALID_ARG) die("file_stride below k * cell_len: status %d", rc);
        rc = hec_read_crc_rows_device(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, 16, cell_len, 1, 512, 0, nullptr,
                                      nullptr, nullptr);
        if (rc != HEC_ERR_INVALID_ARG) die("uniform form, file_stride below k * cell_len: status %d", rc);
        rc = hec_read_crc_rows_device_mixed(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, full_bytes + 7, &present,
                                            &ok_bytes, cell_len, 1, 512, nullptr, nullptr, nullptr, 0, nullptr);
        if (rc != HEC_ERR_DEVICE) die("host-only coder, mixed form: status %d", rc);
        rc = hec_read_crc_rows_device(c, HEC_CHECKSUM_CRC32, nullptr, nullptr, nullptr, 0, cell_len, 2, 100,
                                      full_bytes + 1, nullptr, nullptr, nullptr);
        if (rc != HEC_ERR_DEVICE) die("host-only coder, uniform form: status %d", rc);
    }
    hec_coder_release(c);
}

// Every set of at most m lost units of RS(k,m), by size and then in lexical
// order (1471 for RS(10,4)), with the lengths of the GPU pattern tests' batch
// cut in unit k - 1 (tests/rows_shape_cases.py: the cut unit holds x bytes, x
// by rotation over X(cell_len); x == cell_len is a full stripe); behind them
// the same masks once more as full stripes.  Every pattern is a group of its
// own with two stripes, all but those of x == cell_len a short and a full one.
void pattern_batch(size_t k, size_t m, size_t cell_len, std::vector<uint64_t>* present, std::vector<uint64_t>* bytes) {
    const size_t n = k + m;
    const uint64_t all = (uint64_t(1) << n) - 1;
    std::vector<uint64_t> xs;
    for (uint64_t x : {uint64_t(1), uint64_t(15), uint64_t(16), uint64_t(17), uint64_t(511), uint64_t(512), uint64_t(513),
                       uint64_t(1040), uint64_t(4097), uint64_t(4625), uint64_t(8193), uint64_t(8721),
                       uint64_t(cell_len - 16), uint64_t(cell_len - 1), uint64_t(cell_len)})
        if (x >= 1 && x <= cell_len && std::find(xs.begin(), xs.end(), x) == xs.end()) xs.push_back(x);
    std::sort(xs.begin(), xs.end());
    std::vector<uint64_t> masks;
    for (size_t size = 0; size <= m; size++) {
        std::vector<size_t> idx(size);
        for (size_t i = 0; i < size; i++) idx[i] = i;
        for (;;) {
            uint64_t lost = 0;
            for (size_t u : idx) lost |= uint64_t(1) << u;
            masks.push_back(all & ~lost);
            size_t i = size;
            while (i > 0 && idx[i - 1] == n - size + (i - 1)) i--;
            if (i == 0) break;
            idx[i - 1]++;
            for (size_t j = i; j < size; j++) idx[j] = idx[j - 1] + 1;
        }
    }
    present->clear();
    bytes->clear();
    for (size_t i = 0; i < masks.size(); i++) {
        present->push_back(masks[i]);
        bytes->push_back(uint64_t(k - 1) * cell_len + xs[i % xs.size()]);
    }
    for (uint64_t mask : masks) {
        present->push_back(mask);
        bytes->push_back(0);
    }
}

void check_patterns() {
    hec_coder_t* c = nullptr;
    if (hec_coder_acquire("rs", 10, 4, HEC_DEVICE_HOST, &c) != HEC_OK || !c) die("hec_coder_acquire(rs, 10, 4)");
    std::vector<uint64_t> present, bytes;
    pattern_batch(10, 4, 5136, &present, &bytes);
    if (present.size() != 2 * 1471) die("RS(10,4) has %zu patterns, not 1471", present.size() / 2);
    const size_t groups_before = g_groups;
    check_batch(c, present, bytes, false, 5136, "rs(10,4) every pattern");
    if (g_groups - groups_before != 1471) die("every pattern: %zu groups", g_groups - groups_before);
    hec_coder_release(c);
}

}  // namespace

int main() {
    for (const auto& km : {std::pair<size_t, size_t>{2, 1}, {3, 2}, {6, 3}, {10, 4}, {12, 6}}) check_shape("rs", km.first, km.second);
    check_shape("xor", 2, 1);
    check_shape("rs-legacy", 6, 3);
    check_shape("rs-legacy", 10, 4);
    check_patterns();
    if (g_no_loss == 0 || g_parity_only == 0 || g_rows == 0) die("no e = 0 group, no parity-only loss or no row was checked");
    std::printf("read_rows_planner_check: ok, %zu batches, %zu groups (%zu without a lost data unit, %zu of them lacking parity only), %zu rows\n",
                g_batches, g_groups, g_no_loss, g_parity_only, g_rows);
    return 0;
}
