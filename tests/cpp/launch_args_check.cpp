// launch_args_check.cpp -- the argument builder of the verified calls
// (hdfs-native_amd/csrc/ec_capi.cpp: fill_survivors, fill_rows, fill_units,
// mask_units, recon_fused_args) against the filling restated from the plan
// alone, in a stand-alone program under AddressSanitizer + UBSan.  The
// library's translation unit is included, so the code checked is the code the
// library compiles; only host-only coders (HEC_DEVICE_HOST) are created and no
// HIP call is made.
//
// Restated: survivor slot r = unit rec_survivors[r]; row slot j of the group
// that starts at j0 = unit lost[rows[j0 + j]], coef[j*kMaxK + i] =
// rec_matrix[rows[j0 + j]*k + i]; a unit's base and stride come from the
// table the consumer names -- the outputs (repair), the shards (the scrub's
// extra inputs) or none (sums only).  Every array is longer than what is
// filled and holds a sentinel first; every slot the builder must not touch is
// checked to hold it still.
// Run by tests/test_launch_args.py (CPU).
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
    std::printf("launch_args_check: FAIL %s\n", msg);
    std::fflush(stdout);
    _exit(1);
}

constexpr size_t kUnits = HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS;
constexpr size_t kSlots = kUnits + 8;                       // slots of the test arrays, past any fill
constexpr size_t kCoefs = (hec::kMaxR + 2) * hec::kMaxK;    // a block's coef[] and two rows behind it
constexpr uint8_t kIdFill = 0xEE, kCoefFill = 0xCC;
constexpr uint64_t kStrideFill = 0xABABABABABABABABull;
uint8_t g_fill_byte;
uint8_t* const kBaseFill = &g_fill_byte;

size_t g_plans = 0, g_fills = 0;

// Unit storage that tells the tables and the units apart.
struct Tables {
    const uint8_t* shard[kUnits];
    size_t shard_stride[kUnits];
    uint8_t* out[kUnits];
    size_t out_stride[kUnits];
    Tables() {
        static uint8_t shards[kUnits * 16], outs[kUnits * 16];
        for (size_t u = 0; u < kUnits; u++) {
            shard[u] = shards + 16 * u;
            shard_stride[u] = 4096 + 16 * u;
            out[u] = outs + 16 * u;
            out_stride[u] = 8192 + 32 * u;
        }
    }
};

// Slot arrays as an argument block has them, sentinel-filled.
template <typename P>
struct Block {
    P base[kSlots];
    uint64_t stride[kSlots];
    uint8_t id[kSlots];
    uint8_t coef[kCoefs];
    Block() {
        for (size_t i = 0; i < kSlots; i++) {
            base[i] = kBaseFill;
            stride[i] = kStrideFill;
            id[i] = kIdFill;
        }
        std::memset(coef, kCoefFill, sizeof(coef));
    }
};

enum Form { kRepair, kScrub, kSumsOnly };
const char* const kFormName[] = {"repair", "scrub", "sums-only"};

// Slot `s` of a block: unit `u` (u < 0: untouched) with storage from base/stride (null: none).
template <typename P, typename T>
void expect_slot(const Block<P>& b, size_t s, long u, T const* base, const size_t* stride, const char* what) {
    const P want_base = (u < 0 || !base) ? P(kBaseFill) : P(base[u]);
    const uint64_t want_stride = (u < 0 || !base) ? kStrideFill : uint64_t(stride[u]);
    const uint8_t want_id = u < 0 ? kIdFill : uint8_t(u);
    if (b.base[s] != want_base || b.stride[s] != want_stride || b.id[s] != want_id)
        die("%s: slot %zu holds unit %u stride %llu, expected unit %ld stride %llu%s", what, s, unsigned(b.id[s]),
            (unsigned long long)b.stride[s], u, (unsigned long long)want_stride,
            b.base[s] != want_base ? " (base differs)" : "");
}

// The survivors of a plan in slots slot0 .. slot0+k-1 of an input block.
void check_survivors(const hec_coder* c, const RowPlan& rp, const Tables& t, size_t slot0, const char* what) {
    const size_t k = c->k;
    Block<const uint8_t*> b;
    fill_survivors(rp, k, UnitTable<const uint8_t*>{t.shard, t.shard_stride},
                   unit_slots(b.base + slot0, b.stride + slot0, b.id + slot0));
    for (size_t s = 0; s < kSlots; s++) {
        const bool in = s >= slot0 && s < slot0 + k;
        expect_slot(b, s, in ? long(rp.plan->rec_survivors[s - slot0]) : -1, t.shard, t.shard_stride, what);
    }
    for (size_t i = 0; i < kCoefs; i++)
        if (b.coef[i] != kCoefFill) die("%s: the survivors' fill wrote coef[%zu]", what, i);
    g_fills++;
}

// Rows j0 .. j0+rn-1 of a plan as one consumer takes them, from slot `slot0`.
void check_rows(const hec_coder* c, const RowPlan& rp, const Tables& t, Form form, size_t j0, size_t slot0,
                const char* what) {
    const size_t k = c->k, rn = std::min(size_t(hec::kMaxR), rp.rows.size() - j0);
    const DecodePlan& p = *rp.plan;
    char tag[160];
    std::snprintf(tag, sizeof(tag), "%s, %s rows from %zu", what, kFormName[form], j0);
    const auto check_coef = [&](const uint8_t* coef) {
        for (size_t i = 0; i < kCoefs; i++) {
            const size_t j = i / hec::kMaxK, col = i % hec::kMaxK;
            const uint8_t want = j < rn && col < k ? p.rec_matrix[rp.rows[j0 + j] * k + col] : kCoefFill;
            if (coef[i] != want) die("%s: coef[%zu] = %u, expected %u", tag, i, unsigned(coef[i]), unsigned(want));
        }
    };
    const auto unit_of = [&](size_t s) { return s >= slot0 && s < slot0 + rn ? long(p.lost[rp.rows[j0 + s - slot0]]) : -1; };
    if (form == kRepair) {
        Block<uint8_t*> b;
        fill_rows(rp, k, j0, rn, b.coef, UnitTable<uint8_t*>{t.out, t.out_stride},
                  unit_slots(b.base + slot0, b.stride + slot0, b.id + slot0));
        for (size_t s = 0; s < kSlots; s++) expect_slot(b, s, unit_of(s), t.out, t.out_stride, tag);
        check_coef(b.coef);
    } else if (form == kScrub) {
        Block<const uint8_t*> b;
        fill_rows(rp, k, j0, rn, b.coef, UnitTable<const uint8_t*>{t.shard, t.shard_stride},
                  unit_slots(b.base + slot0, b.stride + slot0, b.id + slot0));
        for (size_t s = 0; s < kSlots; s++) expect_slot(b, s, unit_of(s), t.shard, t.shard_stride, tag);
        check_coef(b.coef);
    } else {
        Block<uint8_t*> b;
        fill_rows(rp, k, j0, rn, b.coef, UnitTable<uint8_t*>{nullptr, nullptr}, id_slots(b.id + slot0));
        for (size_t s = 0; s < kSlots; s++)
            expect_slot(b, s, unit_of(s), static_cast<uint8_t* const*>(nullptr), nullptr, tag);
        check_coef(b.coef);
    }
    g_fills++;
}

// The two blocks of a fused reconstruction launch, whole, against the same
// restated filling (writes_units = false: the checksum-only call).
void check_fused_blocks(hec_coder* c, const RowPlan& rp, const Tables& t, bool writes_units, const char* what) {
    if (rp.rows.size() > size_t(hec::kMaxR)) return;  // no fused launch takes it
    const size_t k = c->k;
    const DecodePlan& p = *rp.plan;
    uint8_t expected[4], bad[4], sums[4];
    const uint32_t list[1] = {0};
    const VerifiedCall x{c, hec::crc::kCrc32c, t.shard, t.shard_stride, writes_units ? t.out : nullptr,
                         writes_units ? t.out_stride : nullptr, 4096, 512, expected, bad, sums, nullptr};
    const CrcGroupCall g{&rp, 7, list};
    hec::MatmulArgs a, ra;
    hec::ReconCrcArgs cs, rcs;
    std::memset(&a, 0x5A, sizeof(a));
    std::memset(&cs, 0x5A, sizeof(cs));
    recon_fused_args(x, g, &a, &cs);
    std::memset(&ra, 0, sizeof(ra));
    std::memset(&rcs, 0, sizeof(rcs));
    for (size_t r = 0; r < k; r++) {
        const size_t u = p.rec_survivors[r];
        ra.in[r] = t.shard[u];
        ra.in_stride[r] = t.shard_stride[u];
        rcs.shard_id[r] = uint8_t(u);
    }
    for (size_t j = 0; j < rp.rows.size(); j++) {
        const size_t row = rp.rows[j], u = p.lost[row];
        if (writes_units) {
            ra.out[j] = t.out[u];
            ra.out_stride[j] = t.out_stride[u];
        }
        rcs.shard_id[k + j] = uint8_t(u);
        for (size_t i = 0; i < k; i++) ra.coef[j * hec::kMaxK + i] = p.rec_matrix[row * k + i];
    }
    ra.k = int32_t(k);
    ra.r = int32_t(rp.rows.size());
    ra.cell_len = 4096;
    ra.stripes = 7;
    rcs.sums = sums;
    rcs.expected = expected;
    rcs.bad = bad;
    rcs.n_total = uint32_t(c->k + c->m);
    rcs.kind = hec::crc::kCrc32c;
    rcs.stripe_list = list;
    if (std::memcmp(&a, &ra, sizeof(a)) != 0) die("%s: the coding block of the fused launch differs", what);
    if (std::memcmp(&cs, &rcs, sizeof(cs)) != 0) die("%s: the checksum block of the fused launch differs", what);
    g_fills++;
}

// One (present, want) pattern: its reconstruction plan through every consumer,
// and the check plan of the mask's survivors with everything else as extras.
void check_pattern(hec_coder* c, uint64_t mask, uint64_t wmask, const Tables& t) {
    const size_t k = c->k, n = c->k + c->m;
    char what[96];
    std::snprintf(what, sizeof(what), "RS(%zu,%zu) mask %llx want %llx", k, c->m, (unsigned long long)mask,
                  (unsigned long long)wmask);
    RowPlan rp;
    if (reconstruct_rows(c, mask, wmask, &rp) != HEC_OK) die("%s: reconstruct_rows failed", what);
    size_t wanted = 0;
    for (uint64_t w = wmask; w; w &= w - 1) wanted++;
    if (rp.rows.size() != wanted) die("%s: %zu rows for %zu wanted units", what, rp.rows.size(), wanted);
    for (size_t j = 0; j < rp.rows.size(); j++)
        if (!((wmask >> rp.plan->lost[rp.rows[j]]) & 1)) die("%s: row %zu is not a wanted unit", what, j);
    g_plans++;
    check_survivors(c, rp, t, 0, what);
    check_survivors(c, rp, t, 3, what);
    for (size_t j0 = 0; j0 < rp.rows.size(); j0 += size_t(hec::kMaxR)) {
        check_rows(c, rp, t, kRepair, j0, 0, what);
        check_rows(c, rp, t, kSumsOnly, j0, 0, what);
        check_rows(c, rp, t, kSumsOnly, j0, k, what);  // shard_id[k + j] of the fused blocks
    }
    check_fused_blocks(c, rp, t, true, what);
    check_fused_blocks(c, rp, t, false, what);

    // the scrub: every unit the reconstruction rebuilt is back, so the mask's
    // first k units are the survivors and the others the extras (in[k + j])
    const uint64_t all = unit_bits(n);
    RowPlan sp;
    if (scrub_rows(c, all, &sp) != HEC_OK || sp.rows.size() != c->m) die("%s: scrub_rows of the full mask", what);
    check_survivors(c, sp, t, 0, what);
    for (size_t j0 = 0; j0 < sp.rows.size(); j0 += size_t(hec::kMaxR)) check_rows(c, sp, t, kScrub, j0, k, what);
    RowPlan dp;  // degraded: the units of `mask` only
    if (scrub_rows(c, mask, &dp) != HEC_OK) die("%s: scrub_rows failed", what);
    if (!dp.rows.empty()) {
        g_plans++;
        check_survivors(c, dp, t, 0, what);
        for (size_t j0 = 0; j0 < dp.rows.size(); j0 += size_t(hec::kMaxR)) check_rows(c, dp, t, kScrub, j0, k, what);
    }

    // a mask's own units (a scrub group without an extra): ascending, in a list of their own
    uint8_t units[kUnits + 1];
    std::memset(units, kIdFill, sizeof(units));
    const size_t cnt = mask_units(mask, units);
    Block<const uint8_t*> b;
    fill_units(units, cnt, UnitTable<const uint8_t*>{t.shard, t.shard_stride}, unit_slots(b.base, b.stride, b.id));
    size_t s = 0;
    for (size_t u = 0; u < n; u++)
        if ((mask >> u) & 1) expect_slot(b, s++, long(u), t.shard, t.shard_stride, what);
    if (s != cnt || units[cnt] != kIdFill) die("%s: mask_units counted %zu of %zu units", what, cnt, s);
    for (; s < kSlots; s++) expect_slot(b, s, -1, t.shard, t.shard_stride, what);
    g_fills++;
}

void check_code(size_t k, size_t m, std::mt19937_64& rng) {
    hec_coder_t* c = nullptr;
    if (hec_coder_create(k, m, HEC_DEVICE_HOST, &c) != HEC_OK) die("RS(%zu,%zu): no host-only coder", k, m);
    const Tables t;
    const size_t n = k + m;
    const uint64_t all = unit_bits(n);
    // every single loss
    for (size_t u = 0; u < n; u++) check_pattern(c, all & ~(uint64_t(1) << u), uint64_t(1) << u, t);
    // a seeded sample of multiple losses: everything lost wanted, then fewer
    // units wanted than lost
    for (size_t round = 0; round < 24; round++) {
        const size_t e = 2 + rng() % (m - 1);
        uint64_t lost = 0;
        for (size_t have = 0; have < e;) {
            const uint64_t bit = uint64_t(1) << (rng() % n);
            if (!(lost & bit)) lost |= bit, have++;
        }
        check_pattern(c, all & ~lost, lost, t);
        uint64_t narrower = lost;
        while (narrower == lost || !narrower) narrower = lost & rng();
        check_pattern(c, all & ~lost, narrower, t);
    }
    // every parity unit lost and wanted: m rows, more than one launch's worth for RS(12,6)
    check_pattern(c, unit_bits(k), all & ~unit_bits(k), t);
    hec_coder_destroy(c);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20261021);
    check_code(3, 2, rng);
    check_code(6, 3, rng);
    check_code(10, 4, rng);
    check_code(12, 6, rng);
    std::printf("launch_args_check: ok, %zu plans, %zu fills\n", g_plans, g_fills);
    return 0;
}
