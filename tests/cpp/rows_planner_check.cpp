// rows_planner_check.cpp -- the host-side planning of
// hec_reconstruct_crc_rows_device_mixed (hdfs-native_amd/csrc/ec_capi.cpp:
// rows_lists, rows_layout, write_rows_image, recon_rows_workspace) against a
// reference built straight from the masks and lengths, in a stand-alone
// program under AddressSanitizer + UBSan.  The library's translation unit is
// included, so the code checked is the code the library compiles; only
// host-only coders (HEC_DEVICE_HOST) are created and no HIP call is made.
//
// Per batch: every pair's full and short stripe lists and the short stripes'
// lengths are compared with the reference, and the image is written into a
// malloc'd buffer of exactly the advertised workspace bytes filled with 0xCD,
// then read back through the documented layout.
// Run by tests/test_reconstruct_crc_rows.py (CPU).
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
    std::printf("rows_planner_check: FAIL %s\n", msg);
    std::fflush(stdout);
    _exit(1);
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

size_t g_batches = 0, g_short = 0, g_full = 0;

// One batch: present / want masks (want_null: every lost unit) and lengths
// (bytes_null: the array is NULL).
void check_batch(hec_coder* c, const std::vector<uint64_t>& present, const std::vector<uint64_t>& want, bool want_null,
                 const std::vector<uint64_t>& bytes, bool bytes_null, size_t cell_len, const char* what) {
    const size_t k = c->k, m = c->m, n = k + m, S = present.size();
    const uint64_t all = n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
    const uint64_t full_bytes = uint64_t(k) * cell_len;

    // the reference: pairs with a target in the order they first appear, each
    // with its full and its short stripes, ascending
    struct RefPlan {
        std::vector<uint32_t> full, shrt;
        std::vector<uint64_t> lens;
    };
    std::map<std::pair<uint64_t, uint64_t>, size_t> ids;
    std::vector<RefPlan> ref;
    for (size_t s = 0; s < S; s++) {
        const uint64_t mask = present[s] & all, w = (want_null ? ~mask : want[s]) & all;
        if (!w) continue;
        auto it = ids.find({mask, w});
        if (it == ids.end()) {
            it = ids.emplace(std::make_pair(mask, w), ref.size()).first;
            ref.emplace_back();
        }
        const uint64_t r = bytes_null ? 0 : bytes[s];
        if (r != 0 && r != full_bytes) {
            ref[it->second].shrt.push_back(uint32_t(s));
            ref[it->second].lens.push_back(r);
        } else {
            ref[it->second].full.push_back(uint32_t(s));
        }
    }
    size_t n_full = 0, n_short = 0;
    for (const RefPlan& p : ref) n_full += p.full.size(), n_short += p.shrt.size();

    // the library, called as hec_reconstruct_crc_rows_device_mixed calls it
    Batch b;
    const int rc = group_stripes(
        c, present.data(), S, kNoPlanId, [&](size_t s, uint64_t mask) { return want_null ? ~mask : want[s]; },
        [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &b);
    if (rc != HEC_OK) die("%s: group_stripes status %d", what, rc);
    if (b.plans.size() != ref.size()) die("%s: %zu plans, reference %zu", what, b.plans.size(), ref.size());
    RowsLists l;
    rows_lists(b, bytes_null ? nullptr : bytes.data(), k, cell_len, &l);
    if (l.full.size() != n_full || l.shrt.size() != n_short || l.short_bytes.size() != n_short ||
        l.full_off.size() != ref.size() + 1 || l.short_off.size() != ref.size() + 1)
        die("%s: %zu full, %zu short entries; reference %zu, %zu", what, l.full.size(), l.shrt.size(), n_full, n_short);
    for (size_t p = 0; p < ref.size(); p++) {
        const size_t f0 = l.full_off[p], f1 = l.full_off[p + 1], s0 = l.short_off[p], s1 = l.short_off[p + 1];
        if (f1 - f0 != ref[p].full.size() || s1 - s0 != ref[p].shrt.size() || f1 > n_full || s1 > n_short)
            die("%s: plan %zu has %zu full and %zu short stripes, reference %zu and %zu", what, p, f1 - f0, s1 - s0,
                ref[p].full.size(), ref[p].shrt.size());
    }

    // the image, in a buffer of exactly the advertised size
    const size_t advertised = hec_reconstruct_crc_rows_mixed_workspace_size(c, S);
    const size_t base_ws = hec_reconstruct_crc_mixed_workspace_size(c, S);
    if (advertised < base_ws) die("%s: workspace %zu below the full-stripe call's %zu", what, advertised, base_ws);
    const RowsLayout w = rows_layout(k, m, S, n_full, n_short);
    // the documented layout, restated
    const size_t full_pos = up256(hec_reconstruct_mixed_workspace_size(c, S));
    const size_t short_pos = up256(base_ws), bytes_pos = short_pos + up256(n_short * 4);
    const size_t need = n_short ? bytes_pos + n_short * 8 : full_pos + n_full * 4;
    if (w.full_pos != full_pos || w.short_pos != short_pos || w.bytes_pos != bytes_pos || w.need != need ||
        w.image_bytes != need - full_pos)
        die("%s: layout (%zu %zu %zu %zu), reference (%zu %zu %zu %zu)", what, w.full_pos, w.short_pos, w.bytes_pos,
            w.need, full_pos, short_pos, bytes_pos, need);
    if (need > advertised) die("%s: image needs %zu of %zu advertised bytes", what, need, advertised);
    if (full_pos + n_full * 4 > short_pos) die("%s: the full lists run into the short ones", what);
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(advertised));
    std::memset(buf, 0xCD, advertised);
    write_rows_image(buf + w.full_pos, l, w);
    for (size_t i = 0; i < full_pos; i++)
        if (buf[i] != 0xCD) die("%s: byte %zu before the image was written", what, i);
    for (size_t i = need; i < advertised; i++)
        if (buf[i] != 0xCD) die("%s: byte %zu behind the image was written", what, i);
    for (size_t i = full_pos; i < need; i++) {
        const bool in_full = i < full_pos + n_full * 4;
        const bool in_short = n_short && i >= short_pos && i < short_pos + n_short * 4;
        const bool in_bytes = n_short && i >= bytes_pos;
        if (!in_full && !in_short && !in_bytes && buf[i] != 0) die("%s: pad byte %zu is %#x", what, i, buf[i]);
    }
    size_t fat = 0, sat = 0;
    for (size_t p = 0; p < ref.size(); p++) {
        if (!ref[p].full.empty() && std::memcmp(buf + full_pos + fat * 4, ref[p].full.data(), ref[p].full.size() * 4) != 0)
            die("%s: plan %zu's full stripes differ", what, p);
        if (!ref[p].shrt.empty()) {
            if (std::memcmp(buf + short_pos + sat * 4, ref[p].shrt.data(), ref[p].shrt.size() * 4) != 0)
                die("%s: plan %zu's short stripes differ", what, p);
            if (std::memcmp(buf + bytes_pos + sat * 8, ref[p].lens.data(), ref[p].lens.size() * 8) != 0)
                die("%s: plan %zu's lengths differ", what, p);
        }
        if (fat != l.full_off[p] || sat != l.short_off[p]) die("%s: plan %zu's offsets differ", what, p);
        fat += ref[p].full.size();
        sat += ref[p].shrt.size();
    }
    std::free(buf);
    g_batches++;
    g_short += n_short;
    g_full += n_full;
}

void check_shape(size_t k, size_t m) {
    hec_coder_t* c = nullptr;
    if (hec_coder_create(k, m, HEC_DEVICE_HOST, &c) != HEC_OK || !c) die("hec_coder_create(%zu, %zu)", k, m);
    const size_t n = k + m, cell_len = 9232;
    const uint64_t all = (uint64_t(1) << n) - 1, full_bytes = uint64_t(k) * cell_len;
    std::mt19937_64 rng(1000 * k + m);
    // every single-loss mask, nothing lost, and a seeded sample of multi-loss masks
    std::vector<uint64_t> masks{all};
    for (size_t u = 0; u < n; u++) masks.push_back(all & ~(uint64_t(1) << u));
    for (int i = 0; i < 24; i++) {
        uint64_t mask = all;
        const size_t lose = 2 + rng() % (m - 1);
        while (size_t(__builtin_popcountll(all & ~mask)) < lose) mask &= ~(uint64_t(1) << (rng() % n));
        masks.push_back(mask);
    }
    const uint64_t fixed[] = {0, full_bytes, 1, cell_len, cell_len + 1};
    size_t last = 0;
    for (size_t S : {size_t(1), size_t(7), size_t(1000)}) {
        const size_t adv = hec_reconstruct_crc_rows_mixed_workspace_size(c, S);
        if (adv < last) die("workspace size shrinks at %zu stripes", S);
        last = adv;
        for (int variant = 0; variant < 6; variant++) {
            std::vector<uint64_t> present(S), want(S), bytes(S);
            for (size_t s = 0; s < S; s++) {
                present[s] = masks[(variant < 2 ? 1 + (s + variant) % n : rng() % masks.size())];
                const uint64_t lost = all & ~present[s];
                want[s] = lost;
                if (variant == 4 && lost) want[s] = lost & ~(lost - 1);  // narrower than the loss
                if (variant == 5 && s % 3 == 0) want[s] = 0;
                const uint64_t pick = rng() % 8;
                bytes[s] = variant == 1 ? 0 : pick < 5 ? fixed[pick] : 1 + rng() % full_bytes;
                if (variant == 2) bytes[s] = 1 + rng() % (full_bytes - 1);  // every stripe short
            }
            char what[96];
            std::snprintf(what, sizeof(what), "RS(%zu,%zu) S=%zu variant %d", k, m, S, variant);
            check_batch(c, present, want, variant < 3, bytes, variant == 0, cell_len, what);
        }
    }
    // an entry above k * cell_len is refused before the coder's device is looked at
    {
        uint64_t present = all & ~uint64_t(1), bytes = full_bytes + 1;
        const int rc = hec_reconstruct_crc_rows_device_mixed(c, HEC_CHECKSUM_CRC32C, nullptr, nullptr, nullptr, nullptr,
                                                             &present, nullptr, &bytes, cell_len, 1, 512, nullptr,
                                                             nullptr, nullptr, nullptr, 0, nullptr);
        if (rc != HEC_ERR_INVALID_ARG) die("stripe_bytes above k * cell_len: status %d", rc);
    }
    hec_coder_destroy(c);
}

// Every set of at most m lost units of RS(k,m), by size and then in lexical
// order (1471 for RS(10,4)), with the lengths of the GPU pattern tests' batch
// cut in unit k - 1 (tests/rows_shape_cases.py: the cut unit holds x bytes, x
// by rotation over X(cell_len); x == cell_len is a full stripe); behind them
// the same masks once more as full stripes.  Every pattern with a lost unit is
// a plan of its own, and all but those of x == cell_len have a full and a
// short list.
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
    if (hec_coder_create(10, 4, HEC_DEVICE_HOST, &c) != HEC_OK || !c) die("hec_coder_create(10, 4)");
    std::vector<uint64_t> present, bytes;
    pattern_batch(10, 4, 5136, &present, &bytes);
    if (present.size() != 2 * 1471) die("RS(10,4) has %zu patterns, not 1471", present.size() / 2);
    const size_t short_before = g_short, full_before = g_full;
    check_batch(c, present, {}, true, bytes, false, 5136, "RS(10,4) every pattern");
    // 1470 plans (pattern 0 loses nothing: no target); x == cell_len at patterns 12, 25, ...
    size_t full_cuts = 0;
    for (size_t i = 1; i < 1471; i++) full_cuts += bytes[i] == uint64_t(10) * 5136;
    if (full_cuts != 113 || g_short - short_before != 1470 - full_cuts || g_full - full_before != 1470 + full_cuts)
        die("every pattern: %zu short and %zu full entries", g_short - short_before, g_full - full_before);
    hec_coder_destroy(c);
}

}  // namespace

int main() {
    check_shape(3, 2);
    check_shape(6, 3);
    check_shape(10, 4);
    check_shape(12, 6);
    check_patterns();
    std::printf("rows_planner_check: ok, %zu batches, %zu full and %zu short list entries\n", g_batches, g_full, g_short);
    return 0;
}
