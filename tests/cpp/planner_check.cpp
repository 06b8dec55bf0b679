// planner_check.cpp -- the host-side planner of the per-stripe ("mixed") device
// calls (hdfs-native_amd/csrc/ec_capi.cpp, "planning shared by the
// reconstruction, scrub and per-stripe calls") against a plain reference, in a
// stand-alone program built with AddressSanitizer + UBSan (and, for
// `planner_check threads`, ThreadSanitizer).  The library's translation unit is
// included, so the code checked is the code the library compiles; only
// host-only coders (HEC_DEVICE_HOST) are created and no HIP call is made.
//
// The reference below derives everything from a presence mask on its own: the
// survivors (first k present units), the lost units, the coefficient rows
// C[unit] . inverse(C[S]) over the CPU oracle's matrix routines, the 3-3-2
// product tables from orc_gf_mul, and the workspace layout from the documented
// format (ec_kernels.hpp).  Every image is written into a malloc'd buffer of
// exactly img.need bytes filled with 0xCD and compared byte for byte.
// Run by tests/test_mixed_planner.py (CPU).
#include "../../hdfs-native_amd/csrc/ec_capi.cpp"

#include <cstdarg>
#include <functional>
#include <random>
#include <set>

extern "C" {
uint8_t orc_gf_mul(uint8_t a, uint8_t b);
uint8_t orc_gf_inv(uint8_t a);
int orc_gen_rs_matrix(size_t k, size_t m, uint8_t* out);
int orc_invert(uint8_t* mat, size_t n);
void orc_matmul(const uint8_t* a, const uint8_t* b, size_t ar, size_t ac, size_t bc, uint8_t* out);
}

namespace {

enum Planner { kDecode = 0, kRecon = 1, kScrub = 2 };
const char* const kPlannerName[] = {"decode", "reconstruct", "scrub"};

// ---- where we are, and how a mismatch ends the program -----------------------

struct Where {
    std::string shape;
    const char* planner = "-";
    const char* what = "";
    size_t S = 0;
    long stripe = -1;
};
thread_local Where g_at;
std::atomic<uint64_t> g_batches{0}, g_images{0}, g_plans{0};

[[noreturn]] void die(const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    std::printf("planner_check: FAIL shape=%s planner=%s%s S=%zu stripe=%ld: %s\n", g_at.shape.c_str(), g_at.planner,
                g_at.what, g_at.S, g_at.stripe, msg);
    std::fflush(stdout);
    _exit(1);
}

// ---- the reference --------------------------------------------------------------

// The format, restated from ec_kernels.hpp's description of the workspace.
constexpr size_t kRefAlign = 256, kRefHeader = 64, kRefTable = 32;
constexpr uint32_t kRefNoPlan = 0xFFFFFFFFu;
constexpr size_t kRefQueueBytes = 16 * 8 * 256;      // decode, reconstruction: 16 launches x 8 counters x 256 B
constexpr size_t kRefScrubQueueBytes = 8 * 256;      // scrub: one launch
constexpr uint64_t kRefResidentMax = 156u << 10;     // offsets + blob the fused kernels keep in LDS
inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool ref_register_k(size_t k) { return k == 2 || k == 3 || k == 6 || k == 10; }
inline uint64_t ref_bits(size_t n) { return n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1; }

// One coefficient's product tables: c*e, c*(e<<3) for e < 8, c*(e<<6) for e < 4, 12 zero bytes.
uint8_t g_tables[256][kRefTable];
void init_tables() {
    for (int c = 0; c < 256; c++) {
        std::memset(g_tables[c], 0, kRefTable);
        for (int e = 0; e < 8; e++) {
            g_tables[c][e] = orc_gf_mul(uint8_t(c), uint8_t(e));
            g_tables[c][8 + e] = orc_gf_mul(uint8_t(c), uint8_t(e << 3));
        }
        for (int e = 0; e < 4; e++) g_tables[c][16 + e] = orc_gf_mul(uint8_t(c), uint8_t(e << 6));
    }
}

// The codec's (k+m) x k matrix, as oracle/ec_oracle.py states it.
std::vector<uint8_t> ref_matrix(const std::string& codec, size_t k, size_t m) {
    std::vector<uint8_t> C((k + m) * k, 0);
    if (codec == "rs") {
        if (orc_gen_rs_matrix(k, m, C.data()) != 0) die("orc_gen_rs_matrix");
        return C;
    }
    for (size_t r = 0; r < k; r++) C[r * k + r] = 1;
    if (codec == "xor") {
        for (size_t c = 0; c < k; c++) C[k * k + c] = 1;
        return C;
    }
    // rs-legacy: gen = prod_{i<m} (2^i + x), lowest degree first; parity j of
    // unit vector e_c = coefficient j of x^(m+c) mod gen, by long division
    std::vector<uint8_t> gen{1};
    uint8_t root = 1;
    for (size_t i = 0; i < m; i++) {
        std::vector<uint8_t> nx(gen.size() + 1, 0);
        for (size_t d = 0; d < gen.size(); d++) {
            nx[d] ^= orc_gf_mul(gen[d], root);
            nx[d + 1] ^= gen[d];
        }
        gen = nx;
        root = orc_gf_mul(root, 2);
    }
    const uint8_t inv_top = orc_gf_inv(gen[m]);
    for (size_t c = 0; c < k; c++) {
        std::vector<uint8_t> all(k + m, 0);
        all[m + c] = 1;
        for (size_t i = k; i-- > 0;) {
            const uint8_t ratio = orc_gf_mul(inv_top, all[i + m]);
            for (size_t j = 0; j <= m; j++)
                if (gen[j]) all[i + j] ^= orc_gf_mul(gen[j], ratio);
        }
        for (size_t j = 0; j < m; j++) C[(k + j) * k + c] = all[j];
    }
    return C;
}

// What one (presence, want) pattern asks of a planner.
struct Expect {
    int status = HEC_OK;
    std::vector<uint8_t> surv, targets;  // no target = nothing to compute
    uint64_t missing = 0;                // scrub only
    std::vector<uint8_t> rows;           // targets x k
};

struct Ref {
    std::string codec;
    size_t k, m, n;
    std::vector<uint8_t> C;
    std::unordered_map<uint64_t, std::vector<uint8_t>> inverses;  // survivor mask -> inverse(C[S])

    Ref(const std::string& cd, size_t k_, size_t m_) : codec(cd), k(k_), m(m_), n(k_ + m_), C(ref_matrix(cd, k_, m_)) {}

    const std::vector<uint8_t>& inverse(const std::vector<uint8_t>& surv) {
        uint64_t smask = 0;
        for (uint8_t u : surv) smask |= uint64_t(1) << u;
        auto it = inverses.find(smask);
        if (it != inverses.end()) return it->second;
        std::vector<uint8_t> sub(k * k);
        for (size_t r = 0; r < k; r++) std::memcpy(&sub[r * k], &C[size_t(surv[r]) * k], k);
        if (orc_invert(sub.data(), k) != 0) die("reference: C[S] singular for survivors %#llx", (unsigned long long)smask);
        return inverses.emplace(smask, std::move(sub)).first->second;
    }

    Expect expect(Planner pl, uint64_t mask, uint64_t wmask) {
        Expect x;
        std::vector<uint8_t> present, lost;
        for (size_t u = 0; u < n; u++) ((mask >> u) & 1 ? present : lost).push_back(uint8_t(u));
        if (pl == kDecode) {
            for (uint8_t u : lost)
                if (u < k) x.targets.push_back(u);
        } else if (pl == kRecon) {
            if (wmask & mask) {
                x.status = HEC_ERR_INVALID_ARG;
                return x;
            }
            for (size_t u = 0; u < n; u++)
                if ((wmask >> u) & 1) x.targets.push_back(uint8_t(u));
        } else {
            if (present.size() <= k) return x;  // e == 0: nothing to check against
            x.targets.assign(present.begin() + k, present.end());
            x.missing = ~mask & ref_bits(n);
        }
        if (x.targets.empty()) return x;
        if (present.size() < k) {
            x.targets.clear();
            x.status = HEC_ERR_NOT_ENOUGH_SHARDS;
            return x;
        }
        x.surv.assign(present.begin(), present.begin() + k);
        const std::vector<uint8_t>& inv = inverse(x.surv);
        x.rows.resize(x.targets.size() * k);
        for (size_t r = 0; r < x.targets.size(); r++)
            orc_matmul(&C[size_t(x.targets[r]) * k], inv.data(), 1, k, k, &x.rows[r * k]);
        return x;
    }
};

size_t ref_entry_bytes(size_t k, size_t e, bool tables) { return kRefHeader + (tables ? e * k * kRefTable : up(e * k, 16)); }

void ref_write_entry(uint8_t* at, size_t k, const Expect& x, bool tables) {
    const uint32_t e = uint32_t(x.targets.size());
    at[0] = uint8_t(e), at[1] = uint8_t(e >> 8), at[2] = uint8_t(e >> 16), at[3] = uint8_t(e >> 24);
    for (size_t i = 0; i < k; i++) at[4 + i] = x.surv[i];
    for (size_t j = 0; j < e; j++) at[36 + j] = x.targets[j];
    for (int b = 0; b < 8; b++) at[52 + b] = uint8_t(x.missing >> (8 * b));
    uint8_t* body = at + kRefHeader;
    for (size_t i = 0; i < size_t(e) * k; i++) {
        if (tables) std::memcpy(body + i * kRefTable, g_tables[x.rows[i]], kRefTable);
        else body[i] = x.rows[i];
    }
}

// ---- one batch -------------------------------------------------------------------

struct Pat {
    uint64_t mask, wmask;  // wmask: the reconstruction's want (ignored where the call passes none)
};

struct PairHash {
    size_t operator()(const std::pair<uint64_t, uint64_t>& p) const {
        return size_t(p.first * 0xD6E8FEB86659FD93ull + p.second * 0x9E3779B97F4A7C15ull);
    }
};

// Plans the batch with the library's planner and checks status, structure,
// sizes and the image in both entry formats against the reference.  `between`
// runs after planning and before anything is read from the batch.
void check_batch(hec_coder* c, Ref& ref, Planner pl, const std::vector<Pat>& pats, bool want_null,
                 const std::function<void()>& between = {}) {
    const size_t k = ref.k, m = ref.m, n = ref.n, S = pats.size();
    const uint64_t all = ref_bits(n);
    g_at.planner = kPlannerName[pl];
    g_at.what = pl == kRecon ? (want_null ? "(want=NULL)" : "(want)") : "";
    g_at.S = S;
    g_at.stripe = -1;
    std::vector<uint64_t> present(S), want(S);
    for (size_t s = 0; s < S; s++) {
        present[s] = pats[s].mask;
        want[s] = pats[s].wmask;
    }

    // the reference: distinct patterns in the order they first appear
    std::unordered_map<std::pair<uint64_t, uint64_t>, uint32_t, PairHash> seen;
    std::vector<Expect> plans;  // those with a target
    std::vector<uint32_t> ref_id(S, kRefNoPlan);
    int want_status = HEC_OK;
    for (size_t s = 0; s < S && want_status == HEC_OK; s++) {
        const uint64_t mask = pats[s].mask & all;
        const uint64_t w = pl == kRecon ? (want_null ? ~mask & all : pats[s].wmask & all) : 0;
        auto it = seen.find({mask, w});
        if (it == seen.end()) {
            Expect x = ref.expect(pl, mask, w);
            uint32_t id = kRefNoPlan;
            if (x.status != HEC_OK) {
                want_status = x.status;
                g_at.stripe = long(s);
                break;
            }
            if (!x.targets.empty()) {
                id = uint32_t(plans.size());
                plans.push_back(std::move(x));
            }
            it = seen.emplace(std::make_pair(mask, w), id).first;
        }
        ref_id[s] = it->second;
    }

    // the library's planner, called as its entry points call it
    Batch b;
    int rc;
    auto no_want = [](size_t, uint64_t) { return uint64_t(0); };
    if (pl == kDecode)
        rc = group_stripes(c, present.data(), S, 0xFFFF, no_want,
                           [&](uint64_t mask, uint64_t, RowPlan* rp) { return decode_rows(c, mask, rp); }, &b);
    else if (pl == kRecon)
        rc = group_stripes(
            c, present.data(), S, 0xFFFF, [&](size_t s, uint64_t mask) { return want_null ? ~mask : want[s]; },
            [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &b);
    else
        rc = group_stripes(c, present.data(), S, kNoPlanId, no_want,
                           [&](uint64_t mask, uint64_t, RowPlan* rp) { return scrub_rows(c, mask, rp); }, &b);
    if (rc != want_status) die("status %d, reference %d", rc, want_status);
    g_batches++;
    if (want_status != HEC_OK) return;  // the calls return here: no image, nothing written
    if (between) between();

    // structure
    if (b.stripe_plan.size() != S) die("stripe_plan holds %zu stripes", b.stripe_plan.size());
    if (b.plans.size() != plans.size()) die("%zu plans, reference %zu", b.plans.size(), plans.size());
    size_t max_e = 0;
    uint64_t target_units = 0;
    for (const Expect& x : plans) {
        max_e = std::max(max_e, x.targets.size());
        for (uint8_t u : x.targets) target_units |= uint64_t(1) << u;
    }
    if (b.max_e != max_e) die("max_e %zu, reference %zu", b.max_e, max_e);
    if (b.target_units != target_units)
        die("target_units %#llx, reference %#llx", (unsigned long long)b.target_units, (unsigned long long)target_units);
    for (size_t s = 0; s < S; s++) {
        g_at.stripe = long(s);
        if (b.stripe_plan[s] != (ref_id[s] == kRefNoPlan ? kNoPlanId : ref_id[s]))
            die("plan id %u, reference %u", b.stripe_plan[s], ref_id[s]);
    }
    g_at.stripe = -1;
    for (size_t pi = 0; pi < plans.size(); pi++) {
        const Expect& x = plans[pi];
        const RowPlan& rp = b.plans[pi];
        if (rp.rows.size() != x.targets.size()) die("plan %zu: %zu rows, reference %zu", pi, rp.rows.size(), x.targets.size());
        if (rp.missing != x.missing) die("plan %zu: missing %#llx", pi, (unsigned long long)rp.missing);
        const RowCoefs t(rp, k);
        if (std::memcmp(t.matrix, x.rows.data(), x.rows.size()) != 0) die("plan %zu: RowCoefs rows differ", pi);
        for (size_t r = 0; r < x.targets.size(); r++)
            if (rp.unit(r) != x.targets[r]) die("plan %zu: row %zu is unit %zu, reference %u", pi, r, rp.unit(r), x.targets[r]);
        if (pl == kScrub)
            for (size_t pos = 0; pos < k + x.targets.size(); pos++) {
                const uint8_t u = pos < k ? x.surv[pos] : x.targets[pos - k];
                if (scrub_positions_to_units(rp, k, uint64_t(1) << pos) != uint64_t(1) << u)
                    die("plan %zu: position %zu is not unit %u", pi, pos, u);
            }
    }
    g_plans += plans.size();

    // stripe lists and runs
    std::vector<uint32_t> flat;
    std::vector<size_t> off;
    stripe_lists(b, &flat, &off);
    {
        std::vector<std::vector<uint32_t>> lists(plans.size());
        size_t planned = 0;
        for (size_t s = 0; s < S; s++)
            if (ref_id[s] != kRefNoPlan) lists[ref_id[s]].push_back(uint32_t(s)), planned++;
        if (flat.size() != planned || off.size() != plans.size() + 1 || off[0] != 0)
            die("stripe_lists: %zu entries, %zu offsets; reference %zu, %zu", flat.size(), off.size(), planned, plans.size() + 1);
        // the copy the calls upload: exactly flat.size() * 4 bytes
        uint32_t* up_lists = static_cast<uint32_t*>(std::malloc(flat.size() * sizeof(uint32_t) + (flat.empty() ? 1 : 0)));
        if (!flat.empty()) std::memcpy(up_lists, flat.data(), flat.size() * sizeof(uint32_t));
        for (size_t pi = 0; pi < plans.size(); pi++) {
            if (off[pi + 1] - off[pi] != lists[pi].size() || off[pi + 1] > flat.size())
                die("stripe_lists: plan %zu has %zu stripes, reference %zu", pi, off[pi + 1] - off[pi], lists[pi].size());
            if (std::memcmp(up_lists + off[pi], lists[pi].data(), lists[pi].size() * sizeof(uint32_t)) != 0)
                die("stripe_lists: plan %zu's stripes differ", pi);
        }
        std::free(up_lists);
        std::vector<std::array<size_t, 3>> runs, ref_runs;
        if (for_each_run(b, [&](size_t s0, size_t s1, size_t pi) {
                runs.push_back({s0, s1, pi});
                return 0;
            }) != 0)
            die("for_each_run returned non-zero");
        for (size_t s0 = 0; s0 < S;) {
            size_t s1 = s0 + 1;
            while (s1 < S && ref_id[s1] == ref_id[s0]) s1++;
            if (ref_id[s0] != kRefNoPlan) ref_runs.push_back({s0, s1, size_t(ref_id[s0])});
            s0 = s1;
        }
        if (runs != ref_runs) die("for_each_run: %zu runs, reference %zu (or their bounds differ)", runs.size(), ref_runs.size());
    }

    // the image, in both entry formats
    const size_t queue_bytes = pl == kScrub ? kRefScrubQueueBytes : kRefQueueBytes;
    size_t bare = 0;  // scrub: stripes without a plan that still have a unit to verify
    for (size_t s = 0; s < S; s++) bare += ref_id[s] == kRefNoPlan && (pats[s].mask & all) != 0;
    for (int tables = 1; tables >= 0; tables--) {
        std::vector<size_t> ref_off(plans.size());
        size_t blob = 0;
        for (size_t pi = 0; pi < plans.size(); pi++) {
            ref_off[pi] = blob;
            blob += ref_entry_bytes(k, plans[pi].targets.size(), tables != 0);
        }
        const size_t blob_pos = up(S * 4, kRefAlign), queue_pos = up(blob_pos + blob, kRefAlign), need = queue_pos + queue_bytes;
        const PlanImage img = plan_image(b, k, tables != 0, pl == kScrub ? kScrubQueueBytes : size_t(hec::kMixedQueueBytes));
        if (img.blob_pos != blob_pos || img.blob_bytes != blob || img.queue_pos != queue_pos || img.need != need)
            die("layout (tables=%d): blob at %zu + %zu, counters at %zu, need %zu; reference %zu + %zu, %zu, %zu", tables,
                img.blob_pos, img.blob_bytes, img.queue_pos, img.need, blob_pos, blob, queue_pos, need);
        if (blob % 4 != 0) die("blob of %zu bytes is no multiple of 4", blob);
        if (blob > 0xFFFFFFF0ull) die("reference blob past 32 bits");

        std::vector<uint8_t> expect(need, 0);
        for (size_t s = 0; s < S; s++) {
            const uint32_t o = ref_id[s] == kRefNoPlan ? kRefNoPlan : uint32_t(ref_off[ref_id[s]]);
            for (int x = 0; x < 4; x++) expect[s * 4 + x] = uint8_t(o >> (8 * x));
        }
        for (size_t pi = 0; pi < plans.size(); pi++) ref_write_entry(&expect[blob_pos + ref_off[pi]], k, plans[pi], tables != 0);

        uint8_t* host = static_cast<uint8_t*>(std::malloc(need));  // the redzone sits at `need`
        if (!host) die("malloc(%zu)", need);
        std::memset(host, 0xCD, need);
        write_plan_image(host, b, img, k);
        g_images++;

        std::vector<char> rows_checked(plans.size(), 0);
        for (size_t s = 0; s < S; s++) {
            g_at.stripe = long(s);
            uint32_t o;
            std::memcpy(&o, host + s * 4, 4);
            if (ref_id[s] == kRefNoPlan) {
                if (o != hec::kNoPlan) die("offset %#x where the reference has no plan (tables=%d)", o, tables);
                continue;
            }
            const Expect& x = plans[ref_id[s]];
            if (o == hec::kNoPlan) die("kNoPlan where the reference has %zu rows (tables=%d)", x.targets.size(), tables);
            if (o >= blob || o % 16 != 0) die("offset %u outside a blob of %zu bytes or off the 16-byte grid", o, blob);
            const size_t entry = ref_entry_bytes(k, x.targets.size(), tables != 0);
            if (o + entry > blob) die("entry at %u + %zu runs past the blob (%zu)", o, entry, blob);
            hec::ScrubPlanHeader h;
            std::memcpy(&h, host + blob_pos + o, sizeof(h));
            if (h.e != x.targets.size()) die("header e %u, reference %zu (tables=%d)", h.e, x.targets.size(), tables);
            for (size_t i = 0; i < size_t(hec::kMaxK); i++)
                if (h.surv[i] != (i < k ? x.surv[i] : 0)) die("surv[%zu] = %u (tables=%d)", i, h.surv[i], tables);
            for (size_t j = 0; j < 16; j++)
                if (h.extras[j] != (j < x.targets.size() ? x.targets[j] : 0)) die("extras/miss[%zu] = %u (tables=%d)", j, h.extras[j], tables);
            if (h.missing_lo != uint32_t(x.missing) || h.missing_hi != uint32_t(x.missing >> 32))
                die("missing %#x:%#x, reference %#llx", h.missing_hi, h.missing_lo, (unsigned long long)x.missing);
            for (uint8_t p : h.pad)
                if (p) die("header pad byte %#x", p);
            if (!rows_checked[ref_id[s]]) {
                rows_checked[ref_id[s]] = 1;
                if (std::memcmp(host + blob_pos + o + kRefHeader, &expect[blob_pos + ref_off[ref_id[s]] + kRefHeader],
                                entry - kRefHeader) != 0)
                    die("rows of the entry at %u differ from the reference's (tables=%d)", o, tables);
            }
        }
        g_at.stripe = -1;
        if (std::memcmp(host, expect.data(), need) != 0) {
            size_t at = 0;
            while (host[at] == expect[at]) at++;
            die("image byte %zu of %zu is %#x, reference %#x (tables=%d; offsets end at %zu, blob %zu..%zu, counters at %zu)", at,
                need, host[at], expect[at], tables, S * 4, blob_pos, blob_pos + blob, queue_pos);
        }
        std::free(host);

        // sizes: what the caller allocated from *_workspace_size covers the image
        if (pl == kDecode && tables) {
            if (need > mixed_workspace(k, m, S)) die("decode image %zu > workspace size %zu", need, mixed_workspace(k, m, S));
        } else if (pl == kRecon && tables) {
            const bool resident = up(S * 4, 16) + blob <= kRefResidentMax;
            if (resident != hec::mixed_resident(S, blob)) die("mixed_resident(%zu, %zu) = %d", S, blob, int(!resident));
            if (resident && need > recon_workspace(k, m, S))
                die("reconstruction image %zu > workspace size %zu", need, recon_workspace(k, m, S));
            if (up(recon_workspace(k, m, S), kRefAlign) + flat.size() * 4 > recon_crc_workspace(k, m, S))
                die("verified reconstruction: lists end past the workspace size %zu", recon_crc_workspace(k, m, S));
        } else if (pl == kScrub) {
            if ((!tables || (ref_register_k(k) && max_e <= 4)) && need > scrub_workspace(k, m, S))
                die("scrub image %zu (tables=%d) > workspace size %zu", need, tables, scrub_workspace(k, m, S));
            if (up(scrub_workspace(k, m, S), kRefAlign) + (flat.size() + bare) * 4 > scrub_crc_workspace(k, m, S))
                die("verified scrub: lists end past the workspace size %zu", scrub_crc_workspace(k, m, S));
        }
    }
}

// ---- patterns ------------------------------------------------------------------------

using Rng = std::mt19937_64;

double binomial(size_t n, size_t j) {
    double c = 1;
    for (size_t i = 1; i <= j; i++) c = c * double(n - i + 1) / double(i);
    return c;
}

// f(lost) for every set of j units out of n, ascending as numbers.
template <typename F>
void for_each_loss(size_t n, size_t j, F&& f) {
    if (j == 0) return f(uint64_t(0));
    if (j > n) return;
    const uint64_t end = uint64_t(1) << n;
    for (uint64_t x = (uint64_t(1) << j) - 1; x < end;) {
        f(x);
        const uint64_t c = x & -x, r = x + c;
        x = (((r ^ x) >> 2) / c) | r;
    }
}

uint64_t random_loss(size_t n, size_t j, Rng& rng) {
    uint64_t lost = 0;
    for (size_t got = 0; got < j;) {
        const uint64_t bit = uint64_t(1) << (rng() % n);
        if (!(lost & bit)) lost |= bit, got++;
    }
    return lost;
}

// Presence masks with j_first .. j_last units lost: all of them, or a seeded
// sample of `limit` where there are more.
std::vector<Pat> loss_patterns(size_t n, size_t j_first, size_t j_last, size_t limit, Rng& rng) {
    const uint64_t all = ref_bits(n);
    double count = 0;
    for (size_t j = j_first; j <= j_last; j++) count += binomial(n, j);
    std::vector<Pat> out;
    if (count <= double(limit)) {
        for (size_t j = j_first; j <= j_last; j++)
            for_each_loss(n, j, [&](uint64_t lost) { out.push_back({all & ~lost, 0}); });
        return out;
    }
    std::set<uint64_t> seen;
    while (out.size() < limit) {
        const uint64_t lost = random_loss(n, j_first + rng() % (j_last - j_first + 1), rng);
        if (seen.insert(lost).second) out.push_back({all & ~lost, 0});
    }
    return out;
}

// (mask, non-empty want within its 1 .. m lost units): all, or a seeded sample.
std::vector<Pat> want_patterns(size_t n, size_t m, size_t limit, Rng& rng) {
    const uint64_t all = ref_bits(n);
    double count = 0;
    for (size_t j = 1; j <= m; j++) count += binomial(n, j) * (double(uint64_t(1) << j) - 1);
    std::vector<Pat> out;
    if (count <= double(limit)) {
        for (size_t j = 1; j <= m; j++)
            for_each_loss(n, j, [&](uint64_t lost) {
                for (uint64_t w = lost; w; w = (w - 1) & lost) out.push_back({all & ~lost, w});
            });
        return out;
    }
    std::set<std::pair<uint64_t, uint64_t>> seen;
    while (out.size() < limit) {
        const uint64_t lost = random_loss(n, 1 + rng() % m, rng);
        uint64_t w = 0;
        for (uint64_t l = lost; l; l &= l - 1)
            if (rng() & 1) w |= l & -l;
        if (w && seen.insert({lost, w}).second) out.push_back({all & ~lost, w});
    }
    return out;
}

void shuffle(std::vector<Pat>& v, Rng& rng) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rng() % i]);
}

// The stripe counts of one planner over one pattern list: 1, 7, half, all,
// all + 5 (some repeat), and runs of unequal length.
void check_counts(hec_coder* c, Ref& ref, Planner pl, std::vector<Pat> pats, bool want_null, Rng& rng) {
    shuffle(pats, rng);
    const size_t N = pats.size();
    for (size_t i = 0; i < std::min<size_t>(N, 12); i++) check_batch(c, ref, pl, {pats[(i * 7919) % N]}, want_null);
    std::vector<Pat> seven;
    for (int i = 0; i < 7; i++) seven.push_back(pats[rng() % N]);
    check_batch(c, ref, pl, seven, want_null);
    if (N >= 2) check_batch(c, ref, pl, std::vector<Pat>(pats.begin(), pats.begin() + N / 2), want_null);
    check_batch(c, ref, pl, pats, want_null);
    std::vector<Pat> more = pats;
    for (int i = 0; i < 5; i++) more.insert(more.begin() + rng() % (more.size() + 1), pats[rng() % N]);
    check_batch(c, ref, pl, more, want_null);
    std::vector<Pat> runs;
    const size_t P = std::min<size_t>(N, 24);
    for (size_t i = 0; i < 4 * P; i++) runs.insert(runs.end(), 1 + (i * 5 + i / 3) % 4, pats[(i * 7 + i / 5) % P]);
    check_batch(c, ref, pl, runs, want_null);
}

hec_coder* host_coder(const std::string& codec, size_t k, size_t m) {
    hec_coder_t* c = nullptr;
    const int rc = hec_coder_create_codec(codec.c_str(), k, m, HEC_DEVICE_HOST, &c);
    if (rc != HEC_OK || !c) die("hec_coder_create_codec(%s, %zu, %zu, host) = %d", codec.c_str(), k, m, rc);
    return c;
}

std::string shape_name(const std::string& codec, size_t k, size_t m) {
    return codec + "(" + std::to_string(k) + "," + std::to_string(m) + ")";
}

// The scrub's masks: every one with an extra (fewer than m lost), and among
// them masks with e == 0: exactly k present, and fewer.
std::vector<Pat> scrub_patterns(size_t n, size_t m, size_t limit, Rng& rng) {
    std::vector<Pat> pats = loss_patterns(n, 0, m - 1, limit, rng);
    for (const Pat& p : loss_patterns(n, m, m, 64, rng)) pats.push_back(p);
    if (n > m + 1)
        for (const Pat& p : loss_patterns(n, m + 1, n - 1, 12, rng)) pats.push_back(p);
    pats.push_back({0, 0});
    return pats;
}

struct Shape {
    const char* codec;
    size_t k, m, limit;
};

// Statuses: every one ends the call before an image exists.
void check_statuses(hec_coder* c, Ref& ref, Rng& rng) {
    const size_t k = ref.k, m = ref.m, n = ref.n;
    const uint64_t all = ref_bits(n);
    const Pat fine{all & ~uint64_t(1), 1};  // unit 0 lost and wanted
    // a want that names a present unit
    check_batch(c, ref, kRecon, {fine, fine, {all & ~uint64_t(1), uint64_t(1) | (uint64_t(1) << (n - 1))}, fine}, false);
    // fewer than k present with a target (xor: any two units lost); data unit 0 among the lost
    const uint64_t lost = uint64_t(1) | (random_loss(n - 1, m, rng) << 1);
    check_batch(c, ref, kDecode, {fine, {all & ~lost, 0}}, false);
    check_batch(c, ref, kRecon, {fine, {all & ~lost, 0}}, true);
    check_batch(c, ref, kRecon, {fine, {all & ~lost, 1}}, false);
    (void)k;
}

// The 0xFFFF plan cap of the decode and the reconstruction: 0xFFFF plans pass,
// one more is HEC_ERR_INVALID_ARG.
void check_plan_cap() {
    g_at.S = 0x10000;
    g_at.stripe = -1;
    g_at.what = "(plan cap)";
    {
        // reconstruction, RS(12,6): the 63 wants of masks with six units lost
        g_at.shape = shape_name("rs", 12, 6);
        g_at.planner = kPlannerName[kRecon];
        hec_coder* c = host_coder("rs", 12, 6);
        std::vector<uint64_t> present, want;
        for_each_loss(18, 6, [&](uint64_t lost) {
            for (uint64_t w = lost; w && present.size() < 0x10000; w = (w - 1) & lost) {
                present.push_back(ref_bits(18) & ~lost);
                want.push_back(w);
            }
        });
        for (size_t S : {size_t(0xFFFF), size_t(0x10000)}) {
            Batch b;
            const int rc = group_stripes(
                c, present.data(), S, 0xFFFF, [&](size_t s, uint64_t) { return want[s]; },
                [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &b);
            if (rc != (S == 0xFFFF ? HEC_OK : HEC_ERR_INVALID_ARG)) die("%zu plans: status %d", S, rc);
            if (S == 0xFFFF && b.plans.size() != 0xFFFF) die("%zu plans of 0xFFFF patterns", b.plans.size());
            g_batches++;
        }
        hec_coder_destroy(c);
    }
    {
        // decode: RS(12,6) has 31 116 masks with a data unit lost, fewer than
        // the cap; RS(2,16) has 131 070 (one data unit lost, a parity unit left)
        g_at.shape = shape_name("rs", 2, 16);
        g_at.planner = kPlannerName[kDecode];
        hec_coder* c = host_coder("rs", 2, 16);
        std::vector<uint64_t> present;
        for (uint64_t parity = 1; parity <= 0xFFFF; parity++) present.push_back((parity << 2) | 2);  // data unit 0 lost
        present.push_back((uint64_t(1) << 2) | 1);                                                  // data unit 1 lost
        for (size_t S : {size_t(0xFFFF), size_t(0x10000)}) {
            Batch b;
            const int rc = group_stripes(
                c, present.data(), S, 0xFFFF, [](size_t, uint64_t) { return uint64_t(0); },
                [&](uint64_t mask, uint64_t, RowPlan* rp) { return decode_rows(c, mask, rp); }, &b);
            if (rc != (S == 0xFFFF ? HEC_OK : HEC_ERR_INVALID_ARG)) die("%zu plans: status %d", S, rc);
            if (S == 0xFFFF && b.plans.size() != 0xFFFF) die("%zu plans of 0xFFFF patterns", b.plans.size());
            g_batches++;
        }
        hec_coder_destroy(c);
    }
}

int run_all() {
    // the (32,16) sample is trimmed: each of its plans inverts a 32 x 32 matrix on both sides
    const Shape shapes[] = {{"rs", 2, 1, 50000},  {"rs", 3, 2, 50000},  {"rs", 6, 3, 50000},       {"rs", 10, 4, 50000},
                            {"rs", 5, 3, 50000},  {"rs", 6, 5, 50000},  {"rs", 2, 4, 50000},       {"rs", 1, 2, 50000},
                            {"rs", 12, 6, 50000}, {"rs", 32, 16, 600},  {"xor", 5, 1, 50000},      {"xor", 6, 1, 50000},
                            {"rs-legacy", 6, 3, 50000}};
    size_t count = 0;
    for (const Shape& sh : shapes) {
        const size_t k = sh.k, m = sh.m, n = sh.k + sh.m;
        g_at.shape = shape_name(sh.codec, k, m);
        Rng rng(1000 * k + m);
        Ref ref(sh.codec, k, m);
        hec_coder* c = host_coder(sh.codec, k, m);
        if (c->enc != ref.C) die("the coder's matrix differs from the reference's");
        check_statuses(c, ref, rng);
        const std::vector<Pat> losses = loss_patterns(n, 0, m, sh.limit, rng);
        check_counts(c, ref, kDecode, losses, true, rng);
        check_counts(c, ref, kRecon, losses, true, rng);
        std::vector<Pat> wants = want_patterns(n, m, sh.limit, rng);
        wants.push_back({ref_bits(n) & ~uint64_t(1), 0});  // a stripe that wants nothing
        check_counts(c, ref, kRecon, wants, false, rng);
        check_counts(c, ref, kScrub, scrub_patterns(n, m, sh.limit, rng), true, rng);
        if (k == 12) {
            // plan cache: the batches above held more distinct masks than the
            // cache keeps, so their PlanRefs outlived eviction
            if (losses.size() <= hec_coder::kPlanCacheMax) die("plan cache: only %zu masks", losses.size());
            if (c->plans.size() > hec_coder::kPlanCacheMax) die("plan cache holds %zu plans", c->plans.size());
        }
        hec_coder_destroy(c);
        count++;
    }
    check_plan_cap();
    std::printf("planner_check: ALL OK shapes=%zu batches=%llu images=%llu plans=%llu\n", count,
                (unsigned long long)g_batches.load(), (unsigned long long)g_images.load(), (unsigned long long)g_plans.load());
    return 0;
}

// ---- threads mode: cached_plan's lock and eviction under contention -----------------------
// Four threads share one RS(10,4) and one RS(12,6) coder; each plans its own
// batches (its own reference, its own order) and checks them as above.  Every
// thread feeds each coder more distinct masks than the cache holds.  RS(10,4)
// has only 1471 masks a batch can plan (at most four units lost), so there the
// cache is also churned with masks of fewer than k present units, which are
// cached with their status: half of them between planning a batch and reading
// it, while the batch's PlanRefs are all that keeps its evicted plans alive.
int run_threads() {
    hec_coder* c104 = host_coder("rs", 10, 4);
    hec_coder* c126 = host_coder("rs", 12, 6);
    std::vector<std::thread> threads;
    for (int t = 0; t < 4; t++)
        threads.emplace_back([=] {
            Rng rng(77 + t);
            {
                g_at.shape = shape_name("rs", 10, 4) + "/thread" + std::to_string(t);
                Ref ref("rs", 10, 4);
                std::vector<Pat> churn = loss_patterns(14, 5, 9, 3000, rng);
                size_t next = 0;
                auto churn_some = [&](size_t count) {
                    const Where keep = g_at;
                    for (size_t end = std::min(churn.size(), next + count); next < end; next++)
                        check_batch(c104, ref, kRecon, {churn[next]}, true);  // NOT_ENOUGH_SHARDS, cached
                    g_at = keep;
                };
                std::vector<Pat> losses = loss_patterns(14, 0, 4, 50000, rng);
                shuffle(losses, rng);
                churn_some(500);
                check_batch(c104, ref, kDecode, losses, true, [&] { churn_some(900); });
                check_batch(c104, ref, kRecon, losses, true, [&] { churn_some(900); });
                check_batch(c104, ref, kScrub, scrub_patterns(14, 4, 50000, rng), true, [&] { churn_some(700); });
            }
            {
                g_at.shape = shape_name("rs", 12, 6) + "/thread" + std::to_string(t);
                Ref ref("rs", 12, 6);
                const size_t many = hec_coder::kPlanCacheMax + 200;
                check_batch(c126, ref, kDecode, loss_patterns(18, 0, 6, many, rng), true);
                std::vector<Pat> wants = want_patterns(18, 6, many, rng);
                check_batch(c126, ref, kRecon, wants, false);
                check_batch(c126, ref, kScrub, loss_patterns(18, 0, 5, many, rng), true);
            }
        });
    for (auto& th : threads) th.join();
    if (c104->plans.size() > hec_coder::kPlanCacheMax || c126->plans.size() > hec_coder::kPlanCacheMax)
        die("plan cache holds %zu and %zu plans", c104->plans.size(), c126->plans.size());
    hec_coder_destroy(c104);
    hec_coder_destroy(c126);
    std::printf("planner_check: ALL OK threads=4 batches=%llu images=%llu plans=%llu\n", (unsigned long long)g_batches.load(),
                (unsigned long long)g_images.load(), (unsigned long long)g_plans.load());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    init_tables();  // also initialises the oracle's field tables before any thread starts
    (void)orc_gf_inv(1);
    if (argc > 1 && std::string(argv[1]) == "threads") return run_threads();
    return run_all();
}
