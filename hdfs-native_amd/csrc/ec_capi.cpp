// ec_capi.cpp -- implementation of the C ABI in include/hdfs_ec_amd.h.
//
// Host-side logic of hdfs-native's Coder (rust/src/ec/gf256.rs:25-138) on top
// of the HIP kernels in ec_kernels.hip:
//   * coding matrix (gen_rs_matrix, gf256.rs:40-57) built once per coder;
//   * decode plans (first-k-present survivors, inverse, missing-data rows;
//     gf256.rs:84-126) computed once per erasure mask and cached -- the
//     reference rebuilds Coder and re-inverts per decoded row (ec/mod.rs:71);
//   * host-buffer calls stage through coder-owned device buffers;
//   * device calls only enqueue kernels on the caller's stream.
// Nothing here throws or aborts across the ABI: every entry point catches.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <fstream>
#include <map>
#include <tuple>
#include <memory>
#include <numeric>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../include/hdfs_ec_amd.h"
#include "../../include/hdfs_ec_amd_exp.h"
#include "checksum.hpp"
#include "checksum_tables.hpp"
#include "crc_compose.hpp"
#include "ec_encode_rows.hpp"
#include "ec_read_rows.hpp"
#include "ec_kernels.hpp"
#include "ec_reconstruct_crc.hpp"
#include "ec_reconstruct_rows.hpp"
#include "ec_reconstruct_sums.hpp"
#include "ec_scrub_crc.hpp"
#include "ec_scrub_rows.hpp"
#include "gf256.hpp"
#include "host_gf.hpp"
#include "jit.hpp"

namespace {

thread_local char g_last_error[256] = "";

// Records the failing HIP call for hec_last_error() and returns `status`.
int fail(int status, const char* what, hipError_t err) {
    std::snprintf(g_last_error, sizeof(g_last_error), "%s: %s (%d)", what, hipGetErrorString(err), int(err));
    return status;
}

#define HEC_HIP(call, status)                                  \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) {                                \
            (void)hipGetLastError();                           \
            return fail((status), #call, e_);                  \
        }                                                      \
    } while (0)

struct DecodePlan {
    int status = HEC_OK;
    std::vector<size_t> survivors;  // k
    std::vector<size_t> missing;    // e
    std::vector<uint8_t> matrix;    // e x k
    std::vector<uint64_t> aff;      // e x k: the matrix's host affine qwords (small-row host path)
    // Reconstruction (hec_reconstruct*): every missing unit, parity included.
    // The fields above stay what the decode calls have always seen; these
    // carry one row per lost unit, and a call's `want` selects among them.
    int rec_status = HEC_OK;            // NOT_ENOUGH_SHARDS / SINGULAR apply once a unit is wanted
    std::vector<size_t> rec_survivors;  // k: the first k present units (also when only parity is lost)
    std::vector<size_t> lost;           // every missing unit, ascending (data units first)
    std::vector<uint8_t> rec_matrix;    // lost x k: data unit t -> row t of the inverse,
                                        // parity unit k+j -> enc[k+j] . inverse
    std::vector<uint32_t> rec_perm;     // lost x k x 8: v_perm product tables of rec_matrix
    std::vector<uint64_t> rec_aff;      // lost x k: host affine qwords of rec_matrix
};

// Restores the caller's current HIP device on scope exit.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;  // a host-only coder (HEC_DEVICE_HOST): no device, no HIP call
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct hec_coder {
    size_t k = 0, m = 0;
    int device = 0;
    bool xor_codec = false;
    std::string codec;         // "rs", "xor" or "rs-legacy"
    bool pooled = false;       // handed out by hec_coder_acquire (returned by hec_coder_release)
    bool idle = false;         // pooled and sitting in the pool (guarded by the pool mutex)
    std::vector<uint8_t> enc;  // (k+m) x k
    std::vector<uint64_t> enc_aff;  // m x k: host affine qwords of the parity rows
    // hec_encode / hec_decode rows of at most this many bytes per shard are
    // coded on the host (hec::host), larger ones go through the device
    std::atomic<size_t> host_limit{kDefaultHostLimit};
    // Every row on pageable buffers: the host routine beat the device route at
    // every size measured, cold (rows from a 1 GiB pool) and hot, 4 KiB to
    // 4 MiB per shard (profiles/r04d/); set a limit to route
    // longer rows through the device.
    static constexpr size_t kDefaultHostLimit = SIZE_MAX;

    // Decode plans keyed by presence bitmask (k+m <= 48), bounded: at most
    // kPlanCacheMax entries; past that the least recently used eighth is
    // dropped (mixed and verified reads can feed it any mask).  Entries are
    // shared_ptrs, so a plan a caller still holds outlives its eviction.
    static constexpr size_t kPlanCacheMax = 4096;
    struct PlanSlot {
        std::shared_ptr<const DecodePlan> plan;
        uint64_t last_use;
    };
    std::mutex plan_mu;
    std::unordered_map<uint64_t, PlanSlot> plans;
    uint64_t plan_clock = 0;

    std::mutex host_mu;  // serialises the host-buffer API (staging buffers)
    static constexpr int kSlots = 3;
    hipStream_t stream = nullptr;                       // compute
    hipStream_t copy_stream[2] = {nullptr, nullptr};    // [0] H2D, [1] D2H
    hipEvent_t ev_in[kSlots] = {}, ev_k[kSlots] = {}, ev_out[kSlots] = {};
    uint8_t* dbuf = nullptr;
    size_t dbuf_bytes = 0;
    // hec_encode / hec_decode (one row per call, pageable caller buffers):
    // a persistent pinned bounce buffer and device slots of their own, grown
    // geometrically and released only by hec_coder_destroy
    static constexpr int kCallPieces = 16;  // column pieces of one per-call row (pipeline stages)
    static constexpr int kCallEvents = 3 * kCallPieces;
    uint8_t* call_host = nullptr;  // hipHostMalloc'd
    uint8_t* call_dev = nullptr;
    size_t call_bytes = 0;
    hipEvent_t ev_call[kCallEvents] = {};
    // verified read, phase 2: stripe lists + mixed-decode workspace (device),
    // grown geometrically, released by hec_coder_destroy.  verify_mu is held
    // from the first list upload until the holder's stream has drained, so two
    // threads verifying on one coder never share (or free) it under each
    // other's queued work.
    std::mutex verify_mu;
    uint8_t* verify_ws = nullptr;
    size_t verify_ws_bytes = 0;
    // mixed decode: two pinned staging images for the workspace upload (so
    // the H2D is a real async DMA), each reused once its copy has run
    std::mutex mixed_mu;
    uint8_t* mixed_host[2] = {nullptr, nullptr};
    size_t mixed_host_bytes[2] = {0, 0};
    hipEvent_t ev_mixed[2] = {nullptr, nullptr};
    int mixed_next = 0;
};

namespace {

// launch_gf_matmul: 0 ok, -1 invalid sizes, >0 the hipError_t of the launch.
int to_status(int kernel_rc) {
    if (kernel_rc == 0) return HEC_OK;
    if (kernel_rc == -1) return HEC_ERR_INVALID_ARG;
    return fail(HEC_ERR_DEVICE, "kernel launch", hipError_t(kernel_rc));
}

DecodePlan compute_plan(size_t k, size_t m, const uint8_t* present, const std::vector<uint8_t>& enc) {
    DecodePlan p;
    std::vector<size_t> valid;
    for (size_t i = 0; i < k + m; i++) {
        if (present[i]) {
            valid.push_back(i);
        } else {
            p.lost.push_back(i);
            if (i < k) p.missing.push_back(i);  // gf256.rs:96-97: only data indices
        }
    }
    // inverse(select_rows(enc, first k present)), shared by both sides
    std::vector<uint8_t> sub;
    if (!p.lost.empty()) {
        if (valid.size() < k) {
            p.rec_status = HEC_ERR_NOT_ENOUGH_SHARDS;
        } else {
            p.rec_survivors.assign(valid.begin(), valid.begin() + k);
            sub.resize(k * k);
            for (size_t r = 0; r < k; r++) std::memcpy(&sub[r * k], &enc[p.rec_survivors[r] * k], k);  // select_rows
            if (!hec::invert(sub.data(), k)) {
                p.rec_status = HEC_ERR_SINGULAR;
            } else {
                p.rec_matrix.assign(p.lost.size() * k, 0);
                for (size_t r = 0; r < p.lost.size(); r++) {
                    const size_t t = p.lost[r];
                    if (t < k) {
                        std::memcpy(&p.rec_matrix[r * k], &sub[t * k], k);
                        continue;
                    }
                    for (size_t i = 0; i < k; i++) {  // enc[t] . inverse
                        uint8_t v = 0;
                        for (size_t x = 0; x < k; x++) v ^= hec::gf_mul(enc[t * k + x], sub[x * k + i]);
                        p.rec_matrix[r * k + i] = v;
                    }
                }
                p.rec_perm.resize(p.rec_matrix.size() * 8);
                for (size_t x = 0; x < p.rec_matrix.size(); x++) {
                    const auto w = hec::perm_table_words(p.rec_matrix[x]);
                    std::memcpy(&p.rec_perm[x * 8], w.data(), sizeof(uint32_t) * 8);
                }
                p.rec_aff = hec::host::affine_matrices(p.rec_matrix.data(), p.rec_matrix.size());
            }
        }
    }
    if (p.missing.empty()) return p;  // gf256.rs:102-105
    if (valid.size() < k) {           // gf256.rs:107-111
        p.status = HEC_ERR_NOT_ENOUGH_SHARDS;
        return p;
    }
    p.survivors = p.rec_survivors;  // first k present, ascending
    if (p.rec_status != HEC_OK) {
        p.status = p.rec_status;  // singular
        return p;
    }
    // select_rows(invalid), ascending: `lost` lists the data units first, so
    // the decode's rows and qwords are the first e of rec_* (the mixed decode
    // reads them there, v_perm tables included)
    const size_t ek = p.missing.size() * k;
    p.matrix.assign(p.rec_matrix.begin(), p.rec_matrix.begin() + ek);
    p.aff.assign(p.rec_aff.begin(), p.rec_aff.begin() + ek);
    return p;
}

// The rows of a plan a reconstruction call asks for: positions in p.lost of
// the units in `want_mask` (every lost unit when the caller passed no want).
std::vector<size_t> target_rows(const DecodePlan& p, bool have_want, uint64_t want_mask) {
    std::vector<size_t> rows;
    for (size_t r = 0; r < p.lost.size(); r++)
        if (!have_want || ((want_mask >> p.lost[r]) & 1)) rows.push_back(r);
    return rows;
}

using PlanRef = std::shared_ptr<const DecodePlan>;

PlanRef cached_plan(hec_coder* c, const uint8_t* present) {
    uint64_t key = 0;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (present[i]) key |= uint64_t(1) << i;
    std::lock_guard<std::mutex> lk(c->plan_mu);
    const uint64_t now = ++c->plan_clock;
    auto it = c->plans.find(key);
    if (it != c->plans.end()) {
        it->second.last_use = now;
        return it->second.plan;
    }
    if (c->plans.size() >= hec_coder::kPlanCacheMax) {
        // evict the least recently used eighth (one pass to find the cut)
        std::vector<uint64_t> uses;
        uses.reserve(c->plans.size());
        for (const auto& kv : c->plans) uses.push_back(kv.second.last_use);
        const size_t n_evict = c->plans.size() / 8;
        std::nth_element(uses.begin(), uses.begin() + n_evict, uses.end());
        const uint64_t cut = uses[n_evict];
        for (auto e = c->plans.begin(); e != c->plans.end();)
            e = e->second.last_use < cut ? c->plans.erase(e) : std::next(e);
    }
    PlanRef p = std::make_shared<const DecodePlan>(compute_plan(c->k, c->m, present, c->enc));
    c->plans.emplace(key, hec_coder::PlanSlot{p, now});
    return p;
}

// Runs out[j] = sum_i mat[j*cols+i] * in[i] over a batch, <= 4 rows per launch.
int matmul_batch(int device, const uint8_t* mat, size_t rows, size_t cols, const uint8_t* const* in,
                 const size_t* in_strides, uint8_t* const* out, const size_t* out_strides, size_t cell_len,
                 size_t stripes, hipStream_t stream) {
    if (rows == 0 || cols == 0 || cols > size_t(hec::kMaxK) || cell_len == 0 || !mat || !in || !out ||
        !in_strides || !out_strides)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    for (size_t i = 0; i < cols; i++)
        if (!in[i]) return HEC_ERR_INVALID_ARG;
    for (size_t j = 0; j < rows; j++)
        if (!out[j]) return HEC_ERR_INVALID_ARG;
    for (size_t r0 = 0; r0 < rows; r0 += hec::kMaxR) {
        hec::MatmulArgs a;
        std::memset(&a, 0, sizeof(a));
        const size_t nr = std::min(rows - r0, size_t(hec::kMaxR));
        for (size_t i = 0; i < cols; i++) {
            a.in[i] = in[i];
            a.in_stride[i] = in_strides[i];
        }
        for (size_t j = 0; j < nr; j++) {
            a.out[j] = out[r0 + j];
            a.out_stride[j] = out_strides[r0 + j];
            for (size_t i = 0; i < cols; i++) a.coef[j * hec::kMaxK + i] = mat[(r0 + j) * cols + i];
        }
        a.k = int32_t(cols);
        a.r = int32_t(nr);
        a.cell_len = cell_len;
        a.stripes = stripes;
        const int rc = hec::launch_gf_matmul(a, device, stream);
        if (rc != 0) return to_status(rc);
    }
    return HEC_OK;
}

// Drains the coder's three streams on scope exit, errors ignored: a pipeline
// that fails half-way never returns while its DMA still reads or writes the
// caller's host buffers (or the slot buffers the next call may reallocate).
struct StreamDrain {
    hec_coder* c;
    ~StreamDrain() {
        (void)hipStreamSynchronize(c->copy_stream[0]);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_stream[1]);
        (void)hipGetLastError();
    }
};

// Grows the per-call staging (pinned host + device) to `bytes`, doubling so
// that a stream of growing rows reallocates O(log) times; never shrinks.
int ensure_call_staging(hec_coder* c, size_t bytes) {
    if (c->call_bytes >= bytes) return HEC_OK;
    const size_t want = std::max(bytes, c->call_bytes * 2);
    if (c->call_host) (void)hipHostFree(c->call_host);
    if (c->call_dev) (void)hipFree(c->call_dev);
    c->call_host = c->call_dev = nullptr;
    c->call_bytes = 0;
    HEC_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->call_host), want, hipHostMallocDefault), HEC_ERR_NO_MEMORY);
    HEC_HIP(hipMalloc(&c->call_dev, want), HEC_ERR_NO_MEMORY);
    c->call_bytes = want;
    return HEC_OK;
}

// One row through the device, pageable caller buffers in and out:
//   out[j] = sum_i mat[j*nin + i] * in[i], n bytes each.
// Rows of >= 512 KiB are cut into column pieces (>= 256 KiB of every shard,
// at most kCallPieces) that flow through a three-stage pipeline: the
// caller's thread copies piece p of every input into the pinned bounce
// buffer and queues its H2D (one 2D copy on copy_stream[0]); the compute
// stream runs the kernel on piece p once it has landed; copy_stream[1]
// brings piece p of the outputs back (one 2D copy) and the caller copies it
// out.  Host copies, both PCIe directions and the kernel then overlap within
// one call.  Smaller rows go through in one piece, one DMA each way.
// No allocation on the hot path.
int call_through_device(hec_coder* c, const uint8_t* const* in, size_t nin, uint8_t* const* out, size_t nout,
                        const uint8_t* mat, size_t n) {
    const size_t pitch = (n + 255) & ~size_t(255);
    int rc = ensure_call_staging(c, pitch * (nin + nout));
    if (rc != HEC_OK) return rc;
    StreamDrain drain{c};  // never return with a DMA still touching the bounce buffer
    const uint8_t* din[HEC_MAX_DATA_UNITS];
    uint8_t* dout[HEC_MAX_DATA_UNITS];
    size_t strides[HEC_MAX_DATA_UNITS];
    for (size_t i = 0; i < std::max(nin, nout); i++) strides[i] = pitch;
    uint8_t* hin = c->call_host;
    uint8_t* hout = c->call_host + nin * pitch;
    uint8_t* dinb = c->call_dev;
    uint8_t* doutb = c->call_dev + nin * pitch;

    const int piece_kib = hec::tune_snapshot().call_piece_kib;  // tune key 17 (0 = 256 KiB)
    const size_t kMinPiece = size_t(piece_kib > 0 ? piece_kib : 256) << 10;
    if (n >= 2 * kMinPiece) {
        size_t piece = (n + hec_coder::kCallPieces - 1) / hec_coder::kCallPieces;
        piece = std::max(kMinPiece, (piece + 4095) & ~size_t(4095));
        const size_t pieces = (n + piece - 1) / piece;
        hipStream_t h2d = c->copy_stream[0], d2h = c->copy_stream[1];
        hipEvent_t* ev_in = c->ev_call;
        hipEvent_t* ev_k = c->ev_call + hec_coder::kCallPieces;
        hipEvent_t* ev_out = c->ev_call + 2 * hec_coder::kCallPieces;
        for (size_t q = 0; q < pieces; q++) {
            const size_t off = q * piece, len = std::min(piece, n - off);
            for (size_t i = 0; i < nin; i++) std::memcpy(hin + i * pitch + off, in[i] + off, len);
            HEC_HIP(hipMemcpy2DAsync(dinb + off, pitch, hin + off, pitch, len, nin, hipMemcpyHostToDevice, h2d),
                    HEC_ERR_DEVICE);
            HEC_HIP(hipEventRecord(ev_in[q], h2d), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamWaitEvent(c->stream, ev_in[q], 0), HEC_ERR_DEVICE);
            for (size_t i = 0; i < nin; i++) din[i] = dinb + i * pitch + off;
            for (size_t j = 0; j < nout; j++) dout[j] = doutb + j * pitch + off;
            rc = matmul_batch(c->device, mat, nout, nin, din, strides, dout, strides, len, 1, c->stream);
            if (rc != HEC_OK) return rc;
            HEC_HIP(hipEventRecord(ev_k[q], c->stream), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamWaitEvent(d2h, ev_k[q], 0), HEC_ERR_DEVICE);
            HEC_HIP(hipMemcpy2DAsync(hout + off, pitch, doutb + off, pitch, len, nout, hipMemcpyDeviceToHost, d2h),
                    HEC_ERR_DEVICE);
            HEC_HIP(hipEventRecord(ev_out[q], d2h), HEC_ERR_DEVICE);
        }
        for (size_t q = 0; q < pieces; q++) {
            const size_t off = q * piece, len = std::min(piece, n - off);
            HEC_HIP(hipEventSynchronize(ev_out[q]), HEC_ERR_DEVICE);
            for (size_t j = 0; j < nout; j++) std::memcpy(out[j] + off, hout + j * pitch + off, len);
        }
        return HEC_OK;
    }

    // one piece: one DMA each way on the compute stream (fewer, larger copies
    // beat per-shard ones below 512 KiB: profiles/r02_probe_percall*.log)
    for (size_t i = 0; i < nin; i++) {
        std::memcpy(hin + i * pitch, in[i], n);
        din[i] = dinb + i * pitch;
    }
    HEC_HIP(hipMemcpyAsync(dinb, hin, pitch * (nin - 1) + n, hipMemcpyHostToDevice, c->stream), HEC_ERR_DEVICE);
    for (size_t j = 0; j < nout; j++) dout[j] = doutb + j * pitch;
    rc = matmul_batch(c->device, mat, nout, nin, din, strides, dout, strides, n, 1, c->stream);
    if (rc != HEC_OK) return rc;
    HEC_HIP(hipMemcpyAsync(hout, doutb, pitch * (nout - 1) + n, hipMemcpyDeviceToHost, c->stream), HEC_ERR_DEVICE);
    HEC_HIP(hipStreamSynchronize(c->stream), HEC_ERR_DEVICE);
    for (size_t j = 0; j < nout; j++) std::memcpy(out[j], hout + j * pitch, n);
    return HEC_OK;
}

// One row of pageable host buffers, routed by size: rows of at most the
// coder's host limit are coded on this thread (hec::host, no lock), larger
// ones through the device under the coder's host lock.
int code_row(hec_coder* c, const uint8_t* mat, const uint64_t* aff, const uint8_t* const* in, size_t nin,
             uint8_t* const* out, size_t nout, size_t n) {
    if (c->device == HEC_DEVICE_HOST || n <= c->host_limit.load(std::memory_order_relaxed)) {
        hec::host::gf_matmul_split(mat, aff, nout, nin, in, out, n);
        return HEC_OK;
    }
    std::lock_guard<std::mutex> lk(c->host_mu);
    DeviceGuard g(c->device);
    if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
    return call_through_device(c, in, nin, out, nout, mat, n);
}

int ensure_dbuf(hec_coder* c, size_t bytes) {
    if (c->dbuf_bytes >= bytes) return HEC_OK;
    if (c->dbuf) (void)hipFree(c->dbuf);
    c->dbuf = nullptr;
    c->dbuf_bytes = 0;
    HEC_HIP(hipMalloc(&c->dbuf, bytes), HEC_ERR_NO_MEMORY);
    c->dbuf_bytes = bytes;
    return HEC_OK;
}

// Device-resident calls on a host-only coder (HEC_DEVICE_HOST): an error, never
// a HIP call.
int host_only(const char* what) { return fail(HEC_ERR_DEVICE, what, hipErrorNoDevice); }

template <typename F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return HEC_ERR_NO_MEMORY;
    } catch (...) {
        return fail(HEC_ERR_DEVICE, "unexpected C++ exception", hipErrorUnknown);
    }
}

}  // namespace

extern "C" {

const char* hec_strerror(int status) {
    switch (status) {
        case HEC_OK: return "ok";
        case HEC_ERR_INVALID_ARG: return "invalid argument";
        case HEC_ERR_NOT_ENOUGH_SHARDS: return "erasure coding error: Not enough valid shards";
        case HEC_ERR_UNSUPPORTED_CODEC: return "unsupported erasure coding policy";
        case HEC_ERR_DEVICE: return "HIP device error";
        case HEC_ERR_NO_MEMORY: return "out of memory";
        case HEC_ERR_SINGULAR: return "Matrix is singular";
        case HEC_ERR_CHECKSUM: return "checksum error";
        default: return "unknown status";
    }
}

int hec_abi_version(void) { return HEC_ABI_VERSION; }

const char* hec_last_error(void) { return g_last_error; }

int hec_gen_rs_matrix(size_t data_units, size_t parity_units, uint8_t* out) {
    if (!out || data_units == 0 || data_units + parity_units > 256) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const std::vector<uint8_t> m = hec::gen_rs_matrix(data_units, parity_units);
        std::memcpy(out, m.data(), m.size());
        return HEC_OK;
    });
}

int hec_gen_codec_matrix(const char* codec, size_t data_units, size_t parity_units, uint8_t* out) {
    if (!out || data_units == 0 || parity_units == 0 || data_units + parity_units > 255) return HEC_ERR_INVALID_ARG;
    const std::string name = codec ? codec : "rs";
    if (name != "rs" && name != "xor" && name != "rs-legacy") return HEC_ERR_UNSUPPORTED_CODEC;
    if (name == "xor" && parity_units != 1) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const std::vector<uint8_t> m = name == "xor"         ? hec::gen_xor_matrix(data_units)
                                       : name == "rs-legacy" ? hec::gen_rs_legacy_matrix(data_units, parity_units)
                                                             : hec::gen_rs_matrix(data_units, parity_units);
        std::memcpy(out, m.data(), m.size());
        return HEC_OK;
    });
}

int hec_matrix_invert(uint8_t* mat, size_t n) {
    if (!mat || n == 0) return HEC_ERR_INVALID_ARG;
    return guarded([&] { return hec::invert(mat, n) ? HEC_OK : HEC_ERR_SINGULAR; });
}

int hec_decode_plan(size_t data_units, size_t parity_units, const uint8_t* present, size_t* n_missing,
                    size_t* survivors, size_t* missing, uint8_t* matrix) {
    if (!present || !n_missing || data_units == 0 || parity_units == 0 || data_units + parity_units > 256)
        return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        DecodePlan p = compute_plan(data_units, parity_units, present, hec::gen_rs_matrix(data_units, parity_units));
        *n_missing = p.missing.size();
        if (p.status != HEC_OK) return p.status;
        if (survivors) std::copy(p.survivors.begin(), p.survivors.end(), survivors);
        if (missing) std::copy(p.missing.begin(), p.missing.end(), missing);
        if (matrix) std::copy(p.matrix.begin(), p.matrix.end(), matrix);
        return HEC_OK;
    });
}

int hec_reconstruct_plan(const char* codec, size_t data_units, size_t parity_units, const uint8_t* present,
                         const uint8_t* want, size_t* n_targets, size_t* survivors, size_t* targets,
                         uint8_t* matrix) {
    if (!present || !n_targets || data_units == 0 || parity_units == 0 || data_units + parity_units > 64)
        return HEC_ERR_INVALID_ARG;
    const std::string name = codec ? codec : "rs";
    if (name != "rs" && name != "xor" && name != "rs-legacy") return HEC_ERR_UNSUPPORTED_CODEC;
    if (name == "xor" && parity_units != 1) return HEC_ERR_INVALID_ARG;
    const size_t k = data_units, n = data_units + parity_units;
    uint64_t want_mask = 0;
    if (want)
        for (size_t i = 0; i < n; i++) {
            if (!want[i]) continue;
            if (present[i]) return HEC_ERR_INVALID_ARG;  // a present unit is not rebuilt
            want_mask |= uint64_t(1) << i;
        }
    return guarded([&] {
        const std::vector<uint8_t> enc = name == "xor"         ? hec::gen_xor_matrix(data_units)
                                         : name == "rs-legacy" ? hec::gen_rs_legacy_matrix(data_units, parity_units)
                                                               : hec::gen_rs_matrix(data_units, parity_units);
        const DecodePlan p = compute_plan(data_units, parity_units, present, enc);
        const std::vector<size_t> rows = target_rows(p, want != nullptr, want_mask);
        *n_targets = rows.size();
        if (rows.empty()) return int(HEC_OK);
        if (p.rec_status != HEC_OK) return p.rec_status;
        if (survivors) std::copy(p.rec_survivors.begin(), p.rec_survivors.end(), survivors);
        for (size_t t = 0; t < rows.size(); t++) {
            if (targets) targets[t] = p.lost[rows[t]];
            if (matrix) std::memcpy(matrix + t * k, &p.rec_matrix[rows[t] * k], k);
        }
        return int(HEC_OK);
    });
}

int hec_coder_create_codec(const char* codec, size_t data_units, size_t parity_units, int device,
                           hec_coder_t** out) {
    if (!out) return HEC_ERR_INVALID_ARG;
    *out = nullptr;
    if (data_units == 0 || data_units > HEC_MAX_DATA_UNITS || parity_units == 0 ||
        parity_units > HEC_MAX_PARITY_UNITS)
        return HEC_ERR_INVALID_ARG;
    const std::string name = codec ? codec : "rs";
    if (name != "rs" && name != "xor" && name != "rs-legacy") return HEC_ERR_UNSUPPORTED_CODEC;
    if (name == "xor" && parity_units != 1) return HEC_ERR_INVALID_ARG;  // XOR-k-1 only
    return guarded([&] {
        if (device != HEC_DEVICE_HOST) {
            int ndev = 0;
            HEC_HIP(hipGetDeviceCount(&ndev), HEC_ERR_DEVICE);
            if (device < 0 || device >= ndev) return fail(HEC_ERR_DEVICE, "device ordinal", hipErrorInvalidDevice);
        }
        auto* c = new hec_coder();
        c->k = data_units;
        c->m = parity_units;
        c->device = device;
        c->xor_codec = name == "xor";
        c->codec = name;
        c->enc = c->xor_codec            ? hec::gen_xor_matrix(data_units)
                 : name == "rs-legacy" ? hec::gen_rs_legacy_matrix(data_units, parity_units)
                                       : hec::gen_rs_matrix(data_units, parity_units);
        c->enc_aff = hec::host::affine_matrices(c->enc.data() + data_units * data_units, parity_units * data_units);
        if (device == HEC_DEVICE_HOST) {  // host routine only: no stream, event or buffer
            c->host_limit.store(SIZE_MAX, std::memory_order_relaxed);
            *out = c;
            return int(HEC_OK);
        }
        int rc = [&] {
            DeviceGuard g(device);
            if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
            HEC_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), HEC_ERR_DEVICE);
            for (int i = 0; i < 2; i++)
                HEC_HIP(hipStreamCreateWithFlags(&c->copy_stream[i], hipStreamNonBlocking), HEC_ERR_DEVICE);
            for (int i = 0; i < hec_coder::kCallEvents; i++)
                HEC_HIP(hipEventCreateWithFlags(&c->ev_call[i], hipEventDisableTiming), HEC_ERR_DEVICE);
            for (int i = 0; i < hec_coder::kSlots; i++) {
                HEC_HIP(hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming), HEC_ERR_DEVICE);
                HEC_HIP(hipEventCreateWithFlags(&c->ev_k[i], hipEventDisableTiming), HEC_ERR_DEVICE);
                HEC_HIP(hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming), HEC_ERR_DEVICE);
            }
            hec::queue_reserve(device);  // graph-capture counter sets, outside any capture
            return HEC_OK;
        }();
        if (rc != HEC_OK) {
            hec_coder_destroy(c);
            return rc;
        }
        *out = c;
        return HEC_OK;
    });
}

int hec_coder_create(size_t data_units, size_t parity_units, int device, hec_coder_t** out) {
    return hec_coder_create_codec("rs", data_units, parity_units, device, out);
}

void hec_coder_destroy(hec_coder_t* c) {
    if (!c) return;
    try {
        DeviceGuard g(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        for (auto s : c->copy_stream)
            if (s) (void)hipStreamSynchronize(s);
        if (c->dbuf) (void)hipFree(c->dbuf);
        if (c->call_dev) (void)hipFree(c->call_dev);
        if (c->call_host) (void)hipHostFree(c->call_host);
        if (c->verify_ws) {  // stream-ordered allocation (verified read phase 2)
            (void)hipFreeAsync(c->verify_ws, nullptr);
            (void)hipStreamSynchronize(nullptr);
        }
        for (int i = 0; i < 2; i++) {
            if (c->ev_mixed[i]) (void)hipEventSynchronize(c->ev_mixed[i]);
            if (c->mixed_host[i]) (void)hipHostFree(c->mixed_host[i]);
            if (c->ev_mixed[i]) (void)hipEventDestroy(c->ev_mixed[i]);
        }
        for (hipEvent_t e : c->ev_call)
            if (e) (void)hipEventDestroy(e);
        for (int i = 0; i < hec_coder::kSlots; i++)
            for (hipEvent_t e : {c->ev_in[i], c->ev_k[i], c->ev_out[i]})
                if (e) (void)hipEventDestroy(e);
        for (auto s : c->copy_stream)
            if (s) (void)hipStreamDestroy(s);
        if (c->stream) (void)hipStreamDestroy(c->stream);
    } catch (...) {
    }
    delete c;
}

}  // extern "C"

// ---- coder pool: Coder::new per row (gf256.rs:32-38, ec/mod.rs:71) ----------

namespace {

// Idle coders by (codec, k, m, device).  hec_coder_acquire pops one (or
// creates one); hec_coder_release pushes it back, so a caller that builds a
// Coder per decoded row pays a mutex and a vector pop, not 3 streams, 60
// events and the staging buffers.  A coder is exclusively the acquirer's
// until it is released.  The pool is never destroyed (coders are not freed
// from a static destructor, after the HIP runtime may be gone).
struct CoderPool {
    std::mutex mu;
    std::map<std::tuple<std::string, size_t, size_t, int>, std::vector<hec_coder*>> idle;
    std::atomic<unsigned> next_device{0};
};
constexpr size_t kPoolIdlePerKey = 64;  // idle coders kept per key; more are destroyed on release

CoderPool& coder_pool() {
    static CoderPool* p = new CoderPool;
    return *p;
}

}  // namespace

extern "C" {

int hec_coder_acquire(const char* codec, size_t data_units, size_t parity_units, int device, hec_coder_t** out) {
    if (!out) return HEC_ERR_INVALID_ARG;
    *out = nullptr;
    if (device < HEC_DEVICE_HOST) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const std::string name = codec ? codec : "rs";
        if (device == -1) {  // any device: round-robin over the visible ones; none -> host-only
            int ndev = 0;
            if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
                device = HEC_DEVICE_HOST;
            else
                device = int(coder_pool().next_device.fetch_add(1, std::memory_order_relaxed) % unsigned(ndev));
        }
        CoderPool& pool = coder_pool();
        {
            std::lock_guard<std::mutex> lk(pool.mu);
            auto it = pool.idle.find(std::make_tuple(name, data_units, parity_units, device));
            if (it != pool.idle.end() && !it->second.empty()) {
                *out = it->second.back();
                it->second.pop_back();
                (*out)->idle = false;
                return int(HEC_OK);
            }
        }
        hec_coder_t* c = nullptr;
        const int rc = hec_coder_create_codec(name.c_str(), data_units, parity_units, device, &c);
        if (rc != HEC_OK) return rc;
        c->pooled = true;
        *out = c;
        return int(HEC_OK);
    });
}

void hec_coder_release(hec_coder_t* c) {
    if (!c) return;
    if (c->pooled) {
        try {
            CoderPool& pool = coder_pool();
            std::lock_guard<std::mutex> lk(pool.mu);
            // a second release of a coder already in the pool is ignored: pushing
            // it twice would hand one coder to two "exclusive" acquirers
            if (c->idle) return;
            // the next acquirer gets a coder with default behaviour: a host
            // limit set by this user (e.g. 0 to force the device) does not carry over
            c->host_limit.store(c->device == HEC_DEVICE_HOST ? SIZE_MAX : hec_coder::kDefaultHostLimit,
                                std::memory_order_relaxed);
            auto& v = pool.idle[std::make_tuple(c->codec, c->k, c->m, c->device)];
            if (v.size() < kPoolIdlePerKey) {
                c->idle = true;
                v.push_back(c);
                return;
            }
        } catch (...) {
        }
    }
    hec_coder_destroy(c);
}

size_t hec_coder_pool_trim(void) {
    std::vector<hec_coder*> drop;
    try {
        CoderPool& pool = coder_pool();
        std::lock_guard<std::mutex> lk(pool.mu);
        for (auto& kv : pool.idle) drop.insert(drop.end(), kv.second.begin(), kv.second.end());
        pool.idle.clear();
    } catch (...) {
        return 0;
    }
    for (hec_coder* c : drop) hec_coder_destroy(c);
    return drop.size();
}

size_t hec_coder_data_units(const hec_coder_t* c) { return c ? c->k : 0; }
size_t hec_coder_parity_units(const hec_coder_t* c) { return c ? c->m : 0; }
int hec_coder_device(const hec_coder_t* c) { return c ? c->device : -1; }

int hec_coder_set_host_limit(hec_coder_t* c, size_t max_shard_len) {
    if (!c) return HEC_ERR_INVALID_ARG;
    c->host_limit.store(max_shard_len, std::memory_order_relaxed);
    return HEC_OK;
}

size_t hec_coder_host_limit(const hec_coder_t* c) { return c ? c->host_limit.load(std::memory_order_relaxed) : 0; }

const char* hec_host_isa(void) { return hec::host::isa_name(hec::host::best_isa()); }

int hec_gf_matmul_host(const uint8_t* matrix, size_t rows, size_t cols, const uint8_t* const* in, uint8_t* const* out,
                       size_t len) {
    if (!matrix || !in || !out || rows == 0 || cols == 0 || cols > HEC_MAX_DATA_UNITS || len == 0)
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < cols; i++)
        if (!in[i]) return HEC_ERR_INVALID_ARG;
    for (size_t j = 0; j < rows; j++)
        if (!out[j]) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        hec::host::gf_matmul_split(matrix, nullptr, rows, cols, in, out, len);
        return int(HEC_OK);
    });
}

int hec_gf_matmul_device(hec_coder_t* c, const uint8_t* matrix, size_t rows, size_t cols,
                         const uint8_t* const* d_in, const size_t* in_strides, uint8_t* const* d_out,
                         const size_t* out_strides, size_t cell_len, size_t stripes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_gf_matmul_device");
    if (!c) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        return matmul_batch(c->device, matrix, rows, cols, d_in, in_strides, d_out, out_strides, cell_len, stripes,
                            static_cast<hipStream_t>(hip_stream));
    });
}

int hec_encode_device(hec_coder_t* c, const uint8_t* const* d_data, const size_t* data_strides,
                      uint8_t* const* d_parity, const size_t* parity_strides, size_t cell_len, size_t stripes,
                      void* hip_stream) {
    if (!c) return HEC_ERR_INVALID_ARG;
    return hec_gf_matmul_device(c, c->enc.data() + c->k * c->k, c->m, c->k, d_data, data_strides, d_parity,
                                parity_strides, cell_len, stripes, hip_stream);
}

int hec_decode_device(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                      uint8_t* const* d_out, const size_t* out_strides, size_t cell_len, size_t stripes,
                      void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_decode_device");
    if (!c || !d_shards || !shard_strides || cell_len == 0) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        uint8_t present[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < c->k + c->m; i++) present[i] = d_shards[i] != nullptr;
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;
        if (p.missing.empty()) return HEC_OK;
        if (!d_out || !out_strides) return HEC_ERR_INVALID_ARG;
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        size_t ist[HEC_MAX_DATA_UNITS];
        uint8_t* out[HEC_MAX_DATA_UNITS];
        size_t ost[HEC_MAX_DATA_UNITS];
        for (size_t r = 0; r < c->k; r++) {
            in[r] = d_shards[p.survivors[r]];
            ist[r] = shard_strides[p.survivors[r]];
        }
        for (size_t r = 0; r < p.missing.size(); r++) {
            out[r] = d_out[p.missing[r]];
            ost[r] = out_strides[p.missing[r]];
        }
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        return matmul_batch(c->device, p.matrix.data(), p.missing.size(), c->k, in, ist, out, ost, cell_len, stripes,
                            static_cast<hipStream_t>(hip_stream));
    });
}

int hec_encode(hec_coder_t* c, const uint8_t* const* data, size_t shard_len, uint8_t* const* parity) {
    if (!c || !data || !parity || shard_len == 0) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k; i++)
        if (!data[i]) return HEC_ERR_INVALID_ARG;
    for (size_t j = 0; j < c->m; j++)
        if (!parity[j]) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        // small rows are coded on this thread (no PCIe round trip, no lock)
        return code_row(c, c->enc.data() + c->k * c->k, c->enc_aff.data(), data, c->k, parity, c->m, shard_len);
    });
}

int hec_decode(hec_coder_t* c, const uint8_t* const* shards, size_t shard_len, uint8_t* const* out) {
    if (!c || !shards || shard_len == 0) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        uint8_t present[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < c->k + c->m; i++) present[i] = shards[i] != nullptr;
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;
        if (p.missing.empty()) return HEC_OK;
        if (!out) return HEC_ERR_INVALID_ARG;
        for (size_t i : p.missing)
            if (!out[i]) return HEC_ERR_INVALID_ARG;
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        uint8_t* dst[HEC_MAX_DATA_UNITS];
        for (size_t r = 0; r < c->k; r++) in[r] = shards[p.survivors[r]];
        for (size_t r = 0; r < p.missing.size(); r++) dst[r] = out[p.missing[r]];
        return code_row(c, p.matrix.data(), p.aff.data(), in, c->k, dst, p.missing.size(), shard_len);
    });
}

// ---- planning shared by the reconstruction, scrub and per-stripe calls -----
// Everything the four per-stripe ("mixed") device calls do on the host before
// a kernel is queued, once: which rows of which cached plan a pattern needs
// (RowPlan), the patterns of a batch (group_stripes), its runs of equal-plan
// stripes (for_each_run), the worst-case and actual workspace layout
// (worst_case_plans, workspace_layout, plan_image) and the upload of an image
// through the coder's two pinned buffers (upload_pinned, upload_plan_image).
// The uniform reconstruction and scrub calls describe their plans the same way.

}  // extern "C"

namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t v) { return (v + kAlign - 1) & ~(kAlign - 1); }

// Bits 0 .. n-1.
inline uint64_t unit_bits(size_t n) { return n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1; }

// The k of the register kernels (their launchers check the same).
inline bool register_kernel_k(size_t k) { return k == 2 || k == 3 || k == 6 || k == 10; }

// 16-byte aligned bases and strides of the units in `units`.
bool aligned16(const uint8_t* const* base, const size_t* stride, uint64_t units) {
    bool ok = true;
    for (; units; units &= units - 1) {
        const int i = __builtin_ctzll(units);
        ok &= ((reinterpret_cast<uintptr_t>(base[i]) | stride[i]) & 15u) == 0;
    }
    return ok;
}

bool any_null(uint8_t* const* ptrs, uint64_t units) {
    for (; units; units &= units - 1)
        if (!ptrs[__builtin_ctzll(units)]) return true;
    return false;
}

PlanRef plan_of_mask(hec_coder* c, uint64_t mask) {
    uint8_t pres[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    for (size_t i = 0; i < c->k + c->m; i++) pres[i] = (mask >> i) & 1;
    return cached_plan(c, pres);
}

// Rows of a cached plan: what one uniform call, or the stripes of one pattern
// of a batch, computes.  No row = nothing to do.
struct RowPlan {
    PlanRef plan;
    std::vector<size_t> rows;  // positions in plan->lost
    uint64_t missing = 0;      // the scrub: units the mask lacks; zero elsewhere
    size_t unit(size_t r) const { return plan->lost[rows[r]]; }
    uint64_t units() const {
        uint64_t u = 0;
        for (size_t r : rows) u |= uint64_t(1) << plan->lost[r];
        return u;
    }
};

// A RowPlan's coefficient rows and host affine qwords, contiguous: the plan's
// own arrays where the rows are consecutive, a gathered copy otherwise.
struct RowCoefs {
    const uint8_t* matrix = nullptr;
    const uint64_t* aff = nullptr;
    std::vector<uint8_t> matrix_store;
    std::vector<uint64_t> aff_store;
    RowCoefs(const RowPlan& rp, size_t k) {
        const DecodePlan& p = *rp.plan;
        bool consecutive = true;
        for (size_t r = 0; r < rp.rows.size(); r++) consecutive &= rp.rows[r] == rp.rows[0] + r;
        if (consecutive) {
            matrix = p.rec_matrix.data() + rp.rows[0] * k;
            aff = p.rec_aff.data() + rp.rows[0] * k;
            return;
        }
        for (size_t r : rp.rows) {
            matrix_store.insert(matrix_store.end(), p.rec_matrix.begin() + r * k, p.rec_matrix.begin() + (r + 1) * k);
            aff_store.insert(aff_store.end(), p.rec_aff.begin() + r * k, p.rec_aff.begin() + (r + 1) * k);
        }
        matrix = matrix_store.data();
        aff = aff_store.data();
    }
};

// A RowPlan's rows over stripes s0 .. s0+count-1 of a device batch: the
// plan's survivors in, its units out, <= 4 rows per launch.
int launch_rows(hec_coder* c, const RowPlan& rp, const uint8_t* const* d_shards, const size_t* shard_strides,
                uint8_t* const* d_out, const size_t* out_strides, size_t cell_len, size_t s0, size_t count,
                hipStream_t stream) {
    const size_t k = c->k;
    const RowCoefs t(rp, k);
    const uint8_t* in[HEC_MAX_DATA_UNITS];
    size_t ist[HEC_MAX_DATA_UNITS];
    uint8_t* out[HEC_MAX_PARITY_UNITS];
    size_t ost[HEC_MAX_PARITY_UNITS];
    for (size_t r = 0; r < k; r++) {
        const size_t u = rp.plan->rec_survivors[r];
        in[r] = d_shards[u] + s0 * shard_strides[u];
        ist[r] = shard_strides[u];
    }
    for (size_t r = 0; r < rp.rows.size(); r++) {
        const size_t u = rp.unit(r);
        out[r] = d_out[u] + s0 * out_strides[u];
        ost[r] = out_strides[u];
    }
    return matmul_batch(c->device, t.matrix, rp.rows.size(), k, in, ist, out, ost, cell_len, count, stream);
}

// The uniform reconstruction calls, from their arguments to the rows to
// rebuild: units[k+m] (null = lost) and want[k+m] (NULL = every lost unit).
// `idle` = the call has no stripe to work on.  HEC_OK with rp->rows empty:
// nothing to rebuild; otherwise the plan stands and every target has storage.
int resolve_reconstruct(hec_coder* c, const uint8_t* const* units, const uint8_t* want, uint8_t* const* out,
                        bool have_out, bool idle, RowPlan* rp) {
    const size_t n = c->k + c->m;
    uint64_t mask = 0, want_mask = 0;
    for (size_t i = 0; i < n; i++)
        if (units[i]) mask |= uint64_t(1) << i;
    for (size_t i = 0; want && i < n; i++)
        if (want[i]) want_mask |= uint64_t(1) << i;
    if (want_mask & mask) return HEC_ERR_INVALID_ARG;  // a present unit is not rebuilt
    rp->plan = plan_of_mask(c, mask);
    if (!idle) rp->rows = target_rows(*rp->plan, want != nullptr, want_mask);
    if (rp->rows.empty()) return HEC_OK;
    if (rp->plan->rec_status != HEC_OK) return rp->plan->rec_status;
    if (!have_out || any_null(out, rp->units())) return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// The rows a mixed decode needs for one presence mask: the missing data
// units, which lead the plan's `lost`.
int decode_rows(hec_coder* c, uint64_t mask, RowPlan* rp) {
    rp->plan = plan_of_mask(c, mask);
    if (rp->plan->status != HEC_OK) return rp->plan->status;
    rp->rows.resize(rp->plan->missing.size());
    std::iota(rp->rows.begin(), rp->rows.end(), size_t(0));
    return HEC_OK;
}

// The rows a mixed reconstruction needs for one (presence, want) pattern.
int reconstruct_rows(hec_coder* c, uint64_t mask, uint64_t wmask, RowPlan* rp) {
    if (!wmask) return HEC_OK;
    rp->plan = plan_of_mask(c, mask);
    if (rp->plan->rec_status != HEC_OK) return rp->plan->rec_status;
    rp->rows = target_rows(*rp->plan, true, wmask);
    return HEC_OK;
}

// S = the first k units of `mask`, E = its other units; returns |mask|.
size_t split_survivors(uint64_t mask, size_t k, uint64_t* smask, uint64_t* emask) {
    size_t seen = 0;
    *smask = *emask = 0;
    for (; mask; mask &= mask - 1, seen++) *(seen < k ? smask : emask) |= mask & -mask;
    return seen;
}

// The check plan of a presence mask: the rows of G = C[E] . inverse(C[S]),
// that is the cached reconstruction plan of `present = S only` with the units
// of E wanted (rec_survivors = S; lost = every unit outside S).  No row when
// the mask has no extra (exactly k present, or fewer).
int scrub_rows(hec_coder* c, uint64_t mask, RowPlan* rp) {
    uint64_t smask, emask;
    if (split_survivors(mask, c->k, &smask, &emask) <= c->k) return HEC_OK;
    rp->plan = plan_of_mask(c, smask);
    if (rp->plan->rec_status != HEC_OK) return rp->plan->rec_status;
    rp->rows = target_rows(*rp->plan, true, emask);
    rp->missing = ~mask & unit_bits(c->k + c->m);
    return HEC_OK;
}

// The plan's positions (bit i < k survivor i, bit k + j extra j) as unit indices.
uint64_t scrub_positions_to_units(const RowPlan& sp, size_t k, uint64_t pos) {
    uint64_t units = 0;
    for (size_t i = 0; i < k; i++)
        if ((pos >> i) & 1) units |= uint64_t(1) << sp.plan->rec_survivors[i];
    for (size_t j = 0; j < sp.rows.size(); j++)
        if ((pos >> (k + j)) & 1) units |= uint64_t(1) << sp.unit(j);
    return units;
}

// Worst-case distinct plans of a batch: sum over j = j_first .. j_last of
// C(n, j) * weight(j), j being the units a presence mask lacks, capped by the
// stripe count.
template <typename Weight>
size_t worst_case_plans(size_t n, size_t j_first, size_t j_last, size_t stripes, Weight&& weight) {
    double total = 0, c = 1;  // C(n, 0)
    for (size_t j = 0; j <= j_last; j++) {
        if (j > 0) c = c * double(n - j + 1) / double(j);
        if (j < j_first) continue;
        total += c * weight(j);
        if (total >= double(stripes)) return stripes;
    }
    return std::min(stripes, size_t(total));
}

// A plan's blob entry: a 64-byte header (hec::DevPlanHeader, or
// hec::ScrubPlanHeader: the same leading fields), then e x k PermTables
// (register kernels) or e x k coefficient bytes padded to 16 B (byte kernel).
static_assert(sizeof(hec::DevPlanHeader) == sizeof(hec::ScrubPlanHeader) &&
                  offsetof(hec::DevPlanHeader, surv) == offsetof(hec::ScrubPlanHeader, surv) &&
                  offsetof(hec::DevPlanHeader, miss) == offsetof(hec::ScrubPlanHeader, extras) &&
                  offsetof(hec::DevPlanHeader, pad) == offsetof(hec::ScrubPlanHeader, missing_lo),
              "one writer fills both plan headers");

size_t plan_entry_bytes(size_t k, size_t e, bool tables) {
    return sizeof(hec::ScrubPlanHeader) + (tables ? e * k * sizeof(hec::PermTable) : ((e * k + 15) & ~size_t(15)));
}

void write_plan_entry(uint8_t* at, size_t k, const RowPlan& rp, bool tables) {
    const DecodePlan& p = *rp.plan;
    hec::ScrubPlanHeader hdr;
    std::memset(&hdr, 0, sizeof(hdr));
    hdr.e = uint32_t(rp.rows.size());
    for (size_t r = 0; r < k; r++) hdr.surv[r] = uint8_t(p.rec_survivors[r]);
    for (size_t r = 0; r < rp.rows.size(); r++) hdr.extras[r] = uint8_t(rp.unit(r));
    hdr.missing_lo = uint32_t(rp.missing);
    hdr.missing_hi = uint32_t(rp.missing >> 32);
    std::memcpy(at, &hdr, sizeof(hdr));
    const size_t row_bytes = tables ? k * sizeof(hec::PermTable) : k;
    uint8_t* body = at + sizeof(hdr);
    for (size_t r = 0; r < rp.rows.size(); r++) {
        const size_t x = rp.rows[r] * k;
        std::memcpy(body + r * row_bytes,
                    tables ? static_cast<const void*>(&p.rec_perm[x * 8]) : static_cast<const void*>(&p.rec_matrix[x]),
                    row_bytes);
    }
    const size_t end = sizeof(hdr) + rp.rows.size() * row_bytes;
    std::memset(at + end, 0, plan_entry_bytes(k, rp.rows.size(), tables) - end);
}

// [per-stripe plan offset: u32 x stripes][plan blob][launch tile counters],
// blob and counters on kAlign boundaries: the workspace of every mixed call
// (hec::MixedArgs, hec::ReconArgs, hec::ScrubMixedArgs).
struct WorkspaceLayout {
    size_t blob_pos, queue_pos, need;
};

WorkspaceLayout workspace_layout(size_t stripes, size_t blob_bytes, size_t queue_bytes) {
    WorkspaceLayout w;
    w.blob_pos = align_up(stripes * sizeof(uint32_t));
    w.queue_pos = align_up(w.blob_pos + blob_bytes);
    w.need = w.queue_pos + queue_bytes;
    return w;
}

constexpr size_t kScrubQueueBytes = size_t(hec::kMixedQueues) * hec::kMixedQueueStride;  // one launch

// The four *_workspace_size results: the layout of the worst batch of
// `stripes` patterns.  Decode: masks with 1 .. m units missing, at most
// min(k, m) of them data.
size_t mixed_workspace(size_t k, size_t m, size_t stripes) {
    const size_t p = worst_case_plans(k + m, 1, m, stripes, [](size_t) { return 1.0; });
    return workspace_layout(stripes, p * plan_entry_bytes(k, std::min(k, m), true), hec::kMixedQueueBytes).need;
}

// Reconstruction: pairs of (mask, non-empty wanted subset of its j <= m lost
// units).  Only the fused kernel reads the workspace, and only when offsets +
// blob fit its resident LDS: the blob term is capped there (a larger batch
// runs per run of stripes and never touches the workspace).
size_t recon_workspace(size_t k, size_t m, size_t stripes) {
    const size_t p = worst_case_plans(k + m, 1, m, stripes, [](size_t j) { return double(uint64_t(1) << j) - 1; });
    const size_t blob = std::min(p * plan_entry_bytes(k, m, true), size_t(hec::kReconResidentMax));
    return workspace_layout(stripes, blob, hec::kMixedQueueBytes).need;
}

// [hec_reconstruct_device_mixed's workspace][stripe lists: u32 x stripes]
size_t recon_crc_workspace(size_t k, size_t m, size_t stripes) {
    return align_up(recon_workspace(k, m, stripes)) + align_up(stripes * sizeof(uint32_t));
}

// Scrub: masks with at least one extra, that is with fewer than m units
// missing; an entry of either kernel's format.
size_t scrub_workspace(size_t k, size_t m, size_t stripes) {
    size_t per = plan_entry_bytes(k, m, false);
    if (register_kernel_k(k)) per = std::max(per, plan_entry_bytes(k, std::min(m, size_t(hec::kMaxR)), true));
    const size_t p = worst_case_plans(k + m, 0, m - 1, stripes, [](size_t) { return 1.0; });
    return workspace_layout(stripes, p * per, kScrubQueueBytes).need;
}

// `bytes` of host data to d_dst through the coder's two pinned staging images
// (so the H2D is a real async DMA).  The images alternate; an image is free
// for reuse once its last upload has run (its event), and c->mixed_mu is held
// from taking the image until that event is recorded behind the new copy.
// fill(host) writes every one of the `bytes`.
template <typename Fill>
int upload_pinned(hec_coder* c, size_t bytes, void* d_dst, hipStream_t stream, Fill&& fill) {
    std::lock_guard<std::mutex> lk(c->mixed_mu);
    const int b = c->mixed_next;
    c->mixed_next ^= 1;
    if (!c->ev_mixed[b]) HEC_HIP(hipEventCreateWithFlags(&c->ev_mixed[b], hipEventDisableTiming), HEC_ERR_DEVICE);
    else HEC_HIP(hipEventSynchronize(c->ev_mixed[b]), HEC_ERR_DEVICE);
    if (c->mixed_host_bytes[b] < bytes) {
        if (c->mixed_host[b]) (void)hipHostFree(c->mixed_host[b]);
        c->mixed_host[b] = nullptr;
        c->mixed_host_bytes[b] = 0;
        const size_t grow = std::max(bytes, 2 * c->mixed_host_bytes[b ^ 1]);
        HEC_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->mixed_host[b]), grow, hipHostMallocDefault),
                HEC_ERR_NO_MEMORY);
        c->mixed_host_bytes[b] = grow;
    }
    fill(c->mixed_host[b]);
    HEC_HIP(hipMemcpyAsync(d_dst, c->mixed_host[b], bytes, hipMemcpyHostToDevice, stream), HEC_ERR_DEVICE);
    HEC_HIP(hipEventRecord(c->ev_mixed[b], stream), HEC_ERR_DEVICE);
    return HEC_OK;
}

// The patterns of a batch and the plan of each.
constexpr uint32_t kNoPlanId = 0xFFFFFFFFu;
struct Batch {
    std::vector<uint32_t> stripe_plan;  // per stripe: its entry of `plans`, or kNoPlanId
    std::vector<RowPlan> plans;         // in the order the patterns first appear
    size_t max_e = 0;                   // most rows of one plan
    uint64_t target_units = 0;          // units some plan computes
};

struct PatternHash {
    size_t operator()(const std::pair<uint64_t, uint64_t>& p) const {
        return size_t((p.first * 0x9E3779B97F4A7C15ull) ^ p.second);
    }
};

// One plan per distinct (present[s], want_of(s, mask)) pattern, nothing
// queued: make(mask, wmask, &rp) fills the pattern's RowPlan (no row = no plan
// for these stripes) or returns a status, which ends the call.  A batch of
// `plan_cap` plans or more is HEC_ERR_INVALID_ARG.
template <typename Want, typename Make>
int group_stripes(const hec_coder* c, const uint64_t* present, size_t stripes, size_t plan_cap, Want&& want_of,
                  Make&& make, Batch* b) {
    const uint64_t all = unit_bits(c->k + c->m);
    std::unordered_map<std::pair<uint64_t, uint64_t>, uint32_t, PatternHash> ids;
    b->stripe_plan.resize(stripes);
    for (size_t s = 0; s < stripes; s++) {
        const uint64_t mask = present[s] & all;
        const uint64_t wmask = want_of(s, mask) & all;
        if (wmask & mask) return HEC_ERR_INVALID_ARG;  // a present unit is not rebuilt
        auto it = ids.find({mask, wmask});
        if (it == ids.end()) {
            RowPlan rp;
            const int rc = make(mask, wmask, &rp);
            if (rc != HEC_OK) return rc;
            uint32_t id = kNoPlanId;
            if (!rp.rows.empty()) {
                if (b->plans.size() >= plan_cap) return HEC_ERR_INVALID_ARG;
                id = uint32_t(b->plans.size());
                b->max_e = std::max(b->max_e, rp.rows.size());
                b->target_units |= rp.units();
                b->plans.push_back(std::move(rp));
            }
            it = ids.emplace(std::make_pair(mask, wmask), id).first;
        }
        b->stripe_plan[s] = it->second;
    }
    return HEC_OK;
}

// f(s0, s1, plan id) for each maximal run [s0, s1) of consecutive stripes
// that share a plan, until one returns non-zero.
template <typename F>
int for_each_run(const Batch& b, F&& f) {
    const size_t stripes = b.stripe_plan.size();
    for (size_t s0 = 0; s0 < stripes;) {
        size_t s1 = s0 + 1;
        while (s1 < stripes && b.stripe_plan[s1] == b.stripe_plan[s0]) s1++;
        if (b.stripe_plan[s0] != kNoPlanId) {
            const int rc = f(s0, s1, size_t(b.stripe_plan[s0]));
            if (rc != 0) return rc;
        }
        s0 = s1;
    }
    return 0;
}

// The stripes of every plan, ascending, flat in plan order: plan p's are
// flat[off[p]] .. flat[off[p + 1] - 1].
void stripe_lists(const Batch& b, std::vector<uint32_t>* flat, std::vector<size_t>* off) {
    off->assign(b.plans.size() + 1, 0);
    for (uint32_t id : b.stripe_plan)
        if (id != kNoPlanId) (*off)[id + 1]++;
    for (size_t p = 0; p < b.plans.size(); p++) (*off)[p + 1] += (*off)[p];
    flat->resize(off->back());
    std::vector<size_t> at(off->begin(), off->end() - 1);
    for (size_t s = 0; s < b.stripe_plan.size(); s++)
        if (b.stripe_plan[s] != kNoPlanId) (*flat)[at[b.stripe_plan[s]]++] = uint32_t(s);
}

// hec_reconstruct_crc_rows_device_mixed: stripe s holds stripe_bytes[s]
// logical bytes; 0 and k * cell_len both say "full".
inline bool rows_short(uint64_t bytes, size_t k, size_t cell_len) {
    return bytes != 0 && bytes != uint64_t(k) * cell_len;
}

// stripe_lists with every plan's stripes split in two: its full stripes and
// its short ones (both ascending, flat in plan order), and the short stripes'
// logical bytes beside their list entries.  stripe_bytes = null: all full.
struct RowsLists {
    std::vector<uint32_t> full, shrt;
    std::vector<size_t> full_off, short_off;  // plan p's: [off[p], off[p + 1])
    std::vector<uint64_t> short_bytes;        // of stripe shrt[i]
};

void rows_lists(const Batch& b, const uint64_t* stripe_bytes, size_t k, size_t cell_len, RowsLists* l) {
    const size_t plans = b.plans.size();
    l->full_off.assign(plans + 1, 0);
    l->short_off.assign(plans + 1, 0);
    auto is_short = [&](size_t s) { return stripe_bytes && rows_short(stripe_bytes[s], k, cell_len); };
    for (size_t s = 0; s < b.stripe_plan.size(); s++)
        if (b.stripe_plan[s] != kNoPlanId) (is_short(s) ? l->short_off : l->full_off)[b.stripe_plan[s] + 1]++;
    for (size_t p = 0; p < plans; p++) {
        l->full_off[p + 1] += l->full_off[p];
        l->short_off[p + 1] += l->short_off[p];
    }
    l->full.resize(l->full_off.back());
    l->shrt.resize(l->short_off.back());
    l->short_bytes.resize(l->short_off.back());
    std::vector<size_t> fat(l->full_off.begin(), l->full_off.end() - 1), sat(l->short_off.begin(), l->short_off.end() - 1);
    for (size_t s = 0; s < b.stripe_plan.size(); s++) {
        const uint32_t id = b.stripe_plan[s];
        if (id == kNoPlanId) continue;
        if (is_short(s)) {
            l->short_bytes[sat[id]] = stripe_bytes[s];
            l->shrt[sat[id]++] = uint32_t(s);
        } else {
            l->full[fat[id]++] = uint32_t(s);
        }
    }
}

// Where the lists sit in the workspace: the full stripes' where
// hec_reconstruct_crc_device_mixed keeps its lists, then, behind that call's
// whole workspace, [short lists: u32][pad to kAlign][their bytes: u64].
// image_bytes = what one upload to full_pos carries (without a short stripe:
// the full lists and nothing else, as hec_reconstruct_crc_device_mixed).
struct RowsLayout {
    size_t full_pos, short_pos, bytes_pos, need, image_bytes;
};

RowsLayout rows_layout(size_t k, size_t m, size_t stripes, size_t n_full, size_t n_short) {
    RowsLayout w;
    w.full_pos = align_up(recon_workspace(k, m, stripes));
    w.short_pos = align_up(recon_crc_workspace(k, m, stripes));
    w.bytes_pos = w.short_pos + align_up(n_short * sizeof(uint32_t));
    w.need = n_short ? w.bytes_pos + n_short * sizeof(uint64_t) : w.full_pos + n_full * sizeof(uint32_t);
    w.image_bytes = w.need - w.full_pos;
    return w;
}

// The worst batch of `stripes`: every stripe short.
size_t recon_rows_workspace(size_t k, size_t m, size_t stripes) {
    return rows_layout(k, m, stripes, 0, stripes).bytes_pos + stripes * sizeof(uint64_t);
}

// Writes every byte of the image (lists, lengths, zeroes in the pads); host =
// the image's first byte, which goes to workspace + w.full_pos.
void write_rows_image(uint8_t* host, const RowsLists& l, const RowsLayout& w) {
    const size_t full_bytes = l.full.size() * sizeof(uint32_t), short_bytes = l.shrt.size() * sizeof(uint32_t);
    if (full_bytes) std::memcpy(host, l.full.data(), full_bytes);
    if (l.shrt.empty()) return;
    std::memset(host + full_bytes, 0, w.short_pos - w.full_pos - full_bytes);
    std::memcpy(host + (w.short_pos - w.full_pos), l.shrt.data(), short_bytes);
    std::memset(host + (w.short_pos - w.full_pos) + short_bytes, 0, w.bytes_pos - w.short_pos - short_bytes);
    std::memcpy(host + (w.bytes_pos - w.full_pos), l.short_bytes.data(), l.short_bytes.size() * sizeof(uint64_t));
}

// The workspace image of a batch: the layout, and each plan's offset in the blob.
struct PlanImage : WorkspaceLayout {
    size_t blob_bytes = 0;
    bool tables = true;  // PermTable rows (register kernels), else coefficient bytes
    std::vector<uint32_t> plan_off;
};

PlanImage plan_image(const Batch& b, size_t k, bool tables, size_t queue_bytes) {
    PlanImage img;
    img.tables = tables;
    img.plan_off.resize(b.plans.size());
    for (size_t pi = 0; pi < b.plans.size(); pi++) {
        img.plan_off[pi] = uint32_t(img.blob_bytes);
        img.blob_bytes += plan_entry_bytes(k, b.plans[pi].rows.size(), tables);
    }
    static_cast<WorkspaceLayout&>(img) = workspace_layout(b.stripe_plan.size(), img.blob_bytes, queue_bytes);
    return img;
}

// Writes the image: every byte of img.need (offsets, entries, zeroes in the
// pads and the counters).
void write_plan_image(uint8_t* host, const Batch& b, const PlanImage& img, size_t k) {
    const size_t stripes = b.stripe_plan.size(), blob_end = img.blob_pos + img.blob_bytes;
    uint32_t* soff = reinterpret_cast<uint32_t*>(host);
    for (size_t s = 0; s < stripes; s++)
        soff[s] = b.stripe_plan[s] == kNoPlanId ? hec::kNoPlan : img.plan_off[b.stripe_plan[s]];
    std::memset(host + stripes * sizeof(uint32_t), 0, img.blob_pos - stripes * sizeof(uint32_t));
    for (size_t pi = 0; pi < b.plans.size(); pi++)
        write_plan_entry(host + img.blob_pos + img.plan_off[pi], k, b.plans[pi], img.tables);
    std::memset(host + blob_end, 0, img.need - blob_end);
}

// Writes the image and queues its upload to d_workspace.
int upload_plan_image(hec_coder* c, const Batch& b, const PlanImage& img, void* d_workspace, hipStream_t stream) {
    return upload_pinned(c, img.need, d_workspace, stream,
                         [&](uint8_t* host) { write_plan_image(host, b, img, c->k); });
}

// What hec::MixedArgs, hec::ReconArgs and hec::ScrubMixedArgs share.
template <typename Args>
void set_batch_args(Args& a, const hec_coder* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                    const PlanImage& img, uint8_t* ws, size_t cell_len, size_t stripes) {
    std::memset(&a, 0, sizeof(a));
    for (size_t i = 0; i < c->k + c->m; i++) {
        a.base[i] = d_shards[i];
        a.stride[i] = shard_strides[i];
    }
    a.stripe_off = reinterpret_cast<const uint32_t*>(ws);
    a.plans = ws + img.blob_pos;
    a.blob_bytes = uint32_t(img.blob_bytes);
    a.k = int32_t(c->k);
    a.cell_len = cell_len;
    a.stripes = stripes;
}

// One launch per group of <= 4 rows, each with its own counters behind
// `queues`; returns the first launch result that is not 0.
template <typename Args, typename Launch>
int launch_row_groups(Args& a, size_t max_e, uint8_t* queues, Launch&& launch) {
    for (size_t r0 = 0; r0 < max_e; r0 += hec::kMaxR) {
        a.row0 = int32_t(r0);
        a.queue = reinterpret_cast<uint32_t*>(queues + (r0 / hec::kMaxR) * hec::kMixedQueues * hec::kMixedQueueStride);
        const int rc = launch(a, int(std::min(max_e - r0, size_t(hec::kMaxR))));
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

// ---- heterogeneous per-stripe erasure patterns ---------------------------

size_t hec_decode_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return mixed_workspace(c->k, c->m, stripes);
}

namespace {

// Body of hec_decode_device_mixed.  Shards that no stripe's plan reads may be
// null here (the verified read's phase 2); the public call requires storage
// for every shard index.
int mixed_decode_impl(hec_coder* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                      uint8_t* const* d_out, const size_t* out_strides, const uint64_t* present, size_t cell_len,
                      size_t stripes, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    const size_t k = c->k, n = c->k + c->m;
    // 1. plan per distinct mask (host), fail before launching anything
    Batch batch;
    int rc = group_stripes(
        c, present, stripes, 0xFFFF, [](size_t, uint64_t) { return uint64_t(0); },
        [&](uint64_t mask, uint64_t, RowPlan* rp) { return decode_rows(c, mask, rp); }, &batch);
    if (rc != HEC_OK) return rc;
    if (batch.plans.empty()) return HEC_OK;
    if (any_null(d_out, batch.target_units)) return HEC_ERR_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);

    const bool fused = register_kernel_k(k) && cell_len % 16 == 0 &&
                       aligned16(d_shards, shard_strides, unit_bits(n)) &&
                       aligned16(d_out, out_strides, unit_bits(k));
    if (!fused)  // correct for any shape: one uniform-pattern launch per run of stripes sharing a plan
        return for_each_run(batch, [&](size_t s0, size_t s1, size_t pi) {
            return launch_rows(c, batch.plans[pi], d_shards, shard_strides, d_out, out_strides, cell_len, s0, s1 - s0,
                               stream);
        });

    // 2. workspace image
    const PlanImage img = plan_image(batch, k, true, hec::kMixedQueueBytes);
    if (!d_workspace || workspace_bytes < img.need || img.blob_bytes > 0xFFFFFFF0ull) return HEC_ERR_INVALID_ARG;
    rc = upload_plan_image(c, batch, img, d_workspace, stream);
    if (rc != HEC_OK) return rc;

    // 3. one launch per group of <= 4 missing rows
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    hec::MixedArgs a;
    set_batch_args(a, c, d_shards, shard_strides, img, ws, cell_len, stripes);
    for (size_t i = 0; i < k; i++) {
        a.out[i] = d_out[i];
        a.out_stride[i] = out_strides[i];
    }
    return to_status(launch_row_groups(a, batch.max_e, ws + img.queue_pos, [&](const hec::MixedArgs& ar, int rows) {
        return hec::launch_decode_mixed(ar, rows, c->device, stream);
    }));
}

}  // namespace

int hec_decode_device_mixed(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                            uint8_t* const* d_out, const size_t* out_strides, const uint64_t* present,
                            size_t cell_len, size_t stripes, void* d_workspace, size_t workspace_bytes,
                            void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_decode_device_mixed");
    if (!c || !d_shards || !shard_strides || !d_out || !out_strides || !present || cell_len == 0)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;  // every shard needs storage (present in some stripe)
    return guarded([&] {
        return mixed_decode_impl(c, d_shards, shard_strides, d_out, out_strides, present, cell_len, stripes,
                                 d_workspace, workspace_bytes, hip_stream);
    });
}

// ---- reconstruction: any lost unit, parity included ------------------------
// Hadoop's RSRawDecoder.decode(inputs, erasedIndexes, outputs): what block-
// group repair needs and the reference's reader (gf256.rs:96-97) never does.
// The plan of a presence mask carries a row per lost unit (DecodePlan::rec_*);
// `want` picks the rows of one call.

int hec_reconstruct(hec_coder_t* c, const uint8_t* const* shards, size_t shard_len, const uint8_t* want,
                    uint8_t* const* out) {
    if (!c || !shards || shard_len == 0) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const size_t k = c->k;
        RowPlan rp;
        const int rc = resolve_reconstruct(c, shards, want, out, out != nullptr, false, &rp);
        if (rc != HEC_OK || rp.rows.empty()) return rc;
        const RowCoefs t(rp, k);
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        uint8_t* dst[HEC_MAX_PARITY_UNITS];
        for (size_t r = 0; r < k; r++) in[r] = shards[rp.plan->rec_survivors[r]];
        for (size_t r = 0; r < rp.rows.size(); r++) dst[r] = out[rp.unit(r)];
        return code_row(c, t.matrix, t.aff, in, k, dst, rp.rows.size(), shard_len);
    });
}

int hec_reconstruct_device(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                           uint8_t* const* d_out, const size_t* out_strides, const uint8_t* want, size_t cell_len,
                           size_t stripes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_device");
    if (!c || !d_shards || !shard_strides || cell_len == 0) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        RowPlan rp;
        const int rc = resolve_reconstruct(c, d_shards, want, d_out, d_out && out_strides, false, &rp);
        if (rc != HEC_OK || rp.rows.empty()) return rc;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        // all m parity units of an intact data set: the rows are the coding
        // matrix's parity rows, and launch_gf_matmul (rs_parity_matrix) picks
        // the encode kernels for them -- hec_encode_device by another name
        return launch_rows(c, rp, d_shards, shard_strides, d_out, out_strides, cell_len, 0, stripes,
                           static_cast<hipStream_t>(hip_stream));
    });
}

size_t hec_reconstruct_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return recon_workspace(c->k, c->m, stripes);
}

namespace {

int mixed_reconstruct_impl(hec_coder* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                           uint8_t* const* d_out, const size_t* out_strides, const uint64_t* present,
                           const uint64_t* want, size_t cell_len, size_t stripes, void* d_workspace,
                           size_t workspace_bytes, void* hip_stream) {
    const size_t k = c->k, n = c->k + c->m;
    // 1. plan per distinct (present, want) pair (host); fail before launching anything
    Batch batch;
    int rc = group_stripes(
        c, present, stripes, 0xFFFF, [&](size_t s, uint64_t mask) { return want ? want[s] : ~mask; },
        [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &batch);
    if (rc != HEC_OK) return rc;
    if (batch.plans.empty()) return HEC_OK;
    if (!d_out || !out_strides || any_null(d_out, batch.target_units)) return HEC_ERR_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);

    // Any shape, and plans past the kernel's resident LDS: one uniform-pattern
    // launch per run of consecutive stripes sharing a plan (as the mixed
    // decode does for the shapes it cannot fuse).
    auto per_run = [&]() -> int {
        return for_each_run(batch, [&](size_t s0, size_t s1, size_t pi) {
            return launch_rows(c, batch.plans[pi], d_shards, shard_strides, d_out, out_strides, cell_len, s0, s1 - s0,
                               stream);
        });
    };

    // 2. workspace image
    const PlanImage img = plan_image(batch, k, true, hec::kMixedQueueBytes);
    const bool fused = register_kernel_k(k) && cell_len % 16 == 0 &&
                       cell_len <= 0xFFFFFFFFull &&  // 32-bit lane offsets into a cell
                       aligned16(d_shards, shard_strides, unit_bits(n)) &&
                       aligned16(d_out, out_strides, batch.target_units) &&
                       hec::mixed_resident(stripes, img.blob_bytes);
    if (!fused) return per_run();
    if (!d_workspace || workspace_bytes < img.need) return HEC_ERR_INVALID_ARG;
    rc = upload_plan_image(c, batch, img, d_workspace, stream);
    if (rc != HEC_OK) return rc;

    // 3. one launch per group of <= 4 target rows
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    hec::ReconArgs a;
    set_batch_args(a, c, d_shards, shard_strides, img, ws, cell_len, stripes);
    for (size_t i = 0; i < n; i++)
        if ((batch.target_units >> i) & 1) {
            a.out[i] = d_out[i];
            a.out_stride[i] = out_strides[i];
        }
    rc = launch_row_groups(a, batch.max_e, ws + img.queue_pos, [&](const hec::ReconArgs& ar, int rows) {
        return hec::launch_reconstruct_mixed(ar, rows, c->device, stream);
    });
    // refused (the runtime would not grant the LDS): every row per run; rows
    // an earlier launch wrote are written again with the same bytes
    return rc == -1 ? per_run() : to_status(rc);
}

}  // namespace

int hec_reconstruct_device_mixed(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                                 uint8_t* const* d_out, const size_t* out_strides, const uint64_t* present,
                                 const uint64_t* want, size_t cell_len, size_t stripes, void* d_workspace,
                                 size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_device_mixed");
    if (!c || !d_shards || !shard_strides || !present || cell_len == 0) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;  // every unit needs storage (present in some stripe)
    return guarded([&] {
        return mixed_reconstruct_impl(c, d_shards, shard_strides, d_out, out_strides, present, want, cell_len,
                                      stripes, d_workspace, workspace_bytes, hip_stream);
    });
}

// ---- scrub: verify parity, locate a corrupt unit ---------------------------

int hec_scrub_verdict(uint64_t ruled_out, uint64_t bad_bytes, size_t units, int* unit) {
    if (units == 0 || units > 64) return HEC_ERR_INVALID_ARG;
    if (bad_bytes == 0) return HEC_SCRUB_CLEAN;
    const uint64_t all = units == 64 ? ~uint64_t(0) : (uint64_t(1) << units) - 1;
    const uint64_t left = ~ruled_out & all;  // the units that explain every bad position
    if (left == 0) return HEC_SCRUB_MULTIPLE;
    if ((left & (left - 1)) != 0) return HEC_SCRUB_AMBIGUOUS;
    if (unit) *unit = __builtin_ctzll(left);
    return HEC_SCRUB_LOCATED;
}

int hec_scrub(hec_coder_t* c, const uint8_t* const* shards, size_t shard_len, hec_scrub_result_t* out) {
    if (!c || !shards || shard_len == 0 || !out) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!shards[i]) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        // always the host routine: the answer is 16 bytes and a pageable row
        // never pays for PCIe
        hec::host::scrub(hec::host::best_isa(), c->enc.data() + c->k * c->k, c->enc_aff.data(), c->k, c->m, shards,
                         shard_len, &out->ruled_out, &out->bad_bytes);
        return int(HEC_OK);
    });
}

int hec_scrub_device(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides, size_t cell_len,
                     size_t stripes, hec_scrub_result_t* d_results, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_device");
    if (!c || !d_shards || !shard_strides || cell_len == 0 || !d_results ||
        (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0)
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > SIZE_MAX / sizeof(hec_scrub_result_t)) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        static_assert(sizeof(hec_scrub_result_t) == 16, "two 64-bit words per stripe");
        hec::ScrubArgs a;
        std::memset(&a, 0, sizeof(a));
        for (size_t i = 0; i < c->k + c->m; i++) {
            a.base[i] = d_shards[i];
            a.stride[i] = shard_strides[i];
        }
        for (size_t j = 0; j < c->m; j++)
            for (size_t i = 0; i < c->k; i++) a.coef[j * hec::kMaxK + i] = c->enc[(c->k + j) * c->k + i];
        a.k = int32_t(c->k);
        a.m = int32_t(c->m);
        a.cell_len = cell_len;
        a.stripes = stripes;
        a.results = reinterpret_cast<uint64_t*>(d_results);
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        // the kernels only OR and add into the words: zeroed here, in stream
        // order (a zeroing kernel node under capture)
        HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), stream), HEC_ERR_DEVICE);
        return to_status(hec::launch_scrub(a, c->device, stream));
    });
}

// ---- scrub correction: fix the located unit in place -------------------------

int hec_scrub_correct(hec_coder_t* c, uint8_t* const* shards, size_t shard_len, hec_scrub_result_t* out, int* unit) {
    if (!c || !shards || shard_len == 0 || !unit) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!shards[i]) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        // always the host routine, as hec_scrub
        hec_scrub_result_t r{};
        *unit = hec::host::scrub_correct(hec::host::best_isa(), c->enc.data() + c->k * c->k, c->enc_aff.data(), c->k,
                                         c->m, shards, shard_len, &r.ruled_out, &r.bad_bytes);
        if (out) *out = r;
        return int(HEC_OK);
    });
}

int hec_scrub_correct_device(hec_coder_t* c, uint8_t* const* d_shards, const size_t* shard_strides, size_t cell_len,
                             size_t stripes, const hec_scrub_result_t* d_results, int32_t* d_units,
                             void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_correct_device");
    if (!c || !d_shards || !shard_strides || cell_len == 0 || !d_results || !d_units ||
        (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0 || (reinterpret_cast<uintptr_t>(d_units) & 3u) != 0)
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > SIZE_MAX / sizeof(hec_scrub_result_t)) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const size_t k = c->k, m = c->m;
        hec::ScrubCorrectArgs a;
        std::memset(&a, 0, sizeof(a));
        for (size_t i = 0; i < k + m; i++) {
            a.base[i] = d_shards[i];
            a.stride[i] = shard_strides[i];
        }
        const uint8_t* P = c->enc.data() + k * k;
        for (size_t j = 0; j < m; j++)
            for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = P[j * k + i];
        // unit t's error is scale[t] * s_row[t]: the first row that sees a data
        // unit (a zero column of P: scale 0, nothing is added), its own row
        // for a parity unit
        for (size_t t = 0; t < k; t++) {
            size_t j = 0;
            while (j < m && P[j * k + t] == 0) j++;
            a.row[t] = uint8_t(j < m ? j : 0);
            a.scale[t] = j < m ? hec::gf_inv(P[j * k + t]) : uint8_t(0);
        }
        for (size_t j = 0; j < m; j++) {
            a.row[k + j] = uint8_t(j);
            a.scale[k + j] = 1;
        }
        a.k = int32_t(k);
        a.m = int32_t(m);
        a.cell_len = cell_len;
        a.stripes = stripes;
        a.results = reinterpret_cast<const uint64_t*>(d_results);
        a.units = d_units;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        return to_status(hec::launch_scrub_correct(a, c->device, static_cast<hipStream_t>(hip_stream)));
    });
}

// ---- degraded scrub: one presence mask per stripe ---------------------------

int hec_scrub_plan(const char* codec, size_t data_units, size_t parity_units, const uint8_t* present, size_t* n_checks,
                   size_t* survivors, size_t* extras, uint8_t* matrix) {
    if (!present || !n_checks || data_units == 0 || parity_units == 0 || data_units + parity_units > 64)
        return HEC_ERR_INVALID_ARG;
    const std::string name = codec ? codec : "rs";
    if (name != "rs" && name != "xor" && name != "rs-legacy") return HEC_ERR_UNSUPPORTED_CODEC;
    if (name == "xor" && parity_units != 1) return HEC_ERR_INVALID_ARG;
    const size_t k = data_units, n = data_units + parity_units;
    return guarded([&] {
        uint64_t mask = 0, smask, emask;
        for (size_t i = 0; i < n; i++)
            if (present[i]) mask |= uint64_t(1) << i;
        const size_t seen = split_survivors(mask, k, &smask, &emask);
        *n_checks = seen > k ? seen - k : 0;
        if (seen <= k) return int(HEC_OK);  // nothing to check against
        std::vector<uint8_t> pres(n);
        for (size_t i = 0; i < n; i++) pres[i] = (smask >> i) & 1;
        const std::vector<uint8_t> enc = name == "xor"         ? hec::gen_xor_matrix(data_units)
                                         : name == "rs-legacy" ? hec::gen_rs_legacy_matrix(data_units, parity_units)
                                                               : hec::gen_rs_matrix(data_units, parity_units);
        const DecodePlan p = compute_plan(data_units, parity_units, pres.data(), enc);
        if (p.rec_status != HEC_OK) return p.rec_status;
        const std::vector<size_t> rows = target_rows(p, true, emask);
        if (survivors) std::copy(p.rec_survivors.begin(), p.rec_survivors.end(), survivors);
        for (size_t t = 0; t < rows.size(); t++) {
            if (extras) extras[t] = p.lost[rows[t]];
            if (matrix) std::memcpy(matrix + t * k, &p.rec_matrix[rows[t] * k], k);
        }
        return int(HEC_OK);
    });
}

int hec_scrub_degraded(hec_coder_t* c, const uint8_t* const* shards, size_t shard_len, hec_scrub_result_t* out) {
    if (!c || !shards || shard_len == 0 || !out) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const size_t k = c->k, n = c->k + c->m;
        out->ruled_out = out->bad_bytes = 0;
        uint64_t mask = 0;
        for (size_t i = 0; i < n; i++)
            if (shards[i]) mask |= uint64_t(1) << i;
        RowPlan sp;
        const int rc = scrub_rows(c, mask, &sp);
        if (rc != HEC_OK || sp.rows.empty()) return rc;  // e == 0: unchecked, nothing read
        const RowCoefs t(sp, k);
        // the host routine over the permuted unit list [S..., E...] with G in
        // the place of P; its bits are positions of that list
        const uint8_t* units[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < k; i++) units[i] = shards[sp.plan->rec_survivors[i]];
        for (size_t j = 0; j < sp.rows.size(); j++) units[k + j] = shards[sp.unit(j)];
        uint64_t pos = 0, bad = 0;
        hec::host::scrub(hec::host::best_isa(), t.matrix, t.aff, k, sp.rows.size(), units, shard_len, &pos, &bad);
        out->bad_bytes = bad;
        out->ruled_out = bad ? (scrub_positions_to_units(sp, k, pos) | sp.missing) : 0;
        return int(HEC_OK);
    });
}

size_t hec_scrub_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return scrub_workspace(c->k, c->m, stripes);
}

int hec_scrub_device_mixed(hec_coder_t* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                           const uint64_t* present, size_t cell_len, size_t stripes, hec_scrub_result_t* d_results,
                           void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_device_mixed");
    if (!c || !d_shards || !shard_strides || !present || cell_len == 0 || !d_results ||
        (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0)
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;  // every unit needs storage (present in some stripe)
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        const size_t k = c->k, n = c->k + c->m;
        // 1. plan per distinct mask (host); fail before anything is queued
        Batch batch;
        bool pivots = true;  // row 0 of every plan without a zero
        int rc = group_stripes(
            c, present, stripes, kNoPlanId, [](size_t, uint64_t) { return uint64_t(0); },
            [&](uint64_t mask, uint64_t, RowPlan* sp) {
                const int src = scrub_rows(c, mask, sp);
                if (src != HEC_OK || sp->rows.empty()) return src;
                const uint8_t* row0 = &sp->plan->rec_matrix[sp->rows[0] * k];
                for (size_t i = 0; i < k; i++) pivots &= row0[i] != 0;
                return int(HEC_OK);
            },
            &batch);
        if (rc != HEC_OK) return rc;
        // the worst batch of `stripes` masks, not this one's image
        if (!batch.plans.empty() && (!d_workspace || workspace_bytes < scrub_workspace(k, c->m, stripes) ||
                                     (reinterpret_cast<uintptr_t>(d_workspace) & 15u) != 0))
            return int(HEC_ERR_INVALID_ARG);
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        // the kernels only OR and add into the words: zeroed here, in stream order
        HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), stream), HEC_ERR_DEVICE);
        if (batch.plans.empty()) return int(HEC_OK);  // no stripe can be checked

        // 2. which kernel: the register kernel's shapes, else the byte kernel
        bool fast = register_kernel_k(k) && batch.max_e <= size_t(hec::kMaxR) && pivots && cell_len % 16 == 0 &&
                    cell_len <= 0xFFFFFFFFull && aligned16(d_shards, shard_strides, unit_bits(n));
        {
            const uint64_t wave_tile = uint64_t(1024) * (k > 6 ? 2 : 4);  // bytes (ec_scrub_mixed.hip)
            if (fast && ((cell_len + wave_tile - 1) / wave_tile) * stripes > 0xFFF00000ull) fast = false;
        }

        // 3. workspace image, in that kernel's entry format
        const PlanImage img = plan_image(batch, k, fast, kScrubQueueBytes);
        rc = upload_plan_image(c, batch, img, d_workspace, stream);
        if (rc != HEC_OK) return rc;

        // 4. launch
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        hec::ScrubMixedArgs a;
        set_batch_args(a, c, d_shards, shard_strides, img, ws, cell_len, stripes);
        a.results = reinterpret_cast<uint64_t*>(d_results);
        a.queue = reinterpret_cast<uint32_t*>(ws + img.queue_pos);
        if (!fast) return to_status(hec::launch_scrub_mixed_bytes(a, c->device, stream));
        if (hec::mixed_resident(stripes, img.blob_bytes)) {
            const int lrc = hec::launch_scrub_mixed(a, int(batch.max_e), c->device, stream);
            if (lrc != -1) return to_status(lrc);
            // refused (the runtime would not grant the LDS): per run below
        }
        // Plans past the resident LDS: the same kernel once per run of
        // consecutive stripes sharing a plan, that one plan resident.
        return for_each_run(batch, [&](size_t s0, size_t s1, size_t pi) {
            const size_t e = batch.plans[pi].rows.size();
            hec::ScrubMixedArgs r = a;
            for (size_t i = 0; i < n; i++) r.base[i] = d_shards[i] + s0 * shard_strides[i];
            r.stripe_off = nullptr;
            r.plans = ws + img.blob_pos + img.plan_off[pi];
            r.blob_bytes = uint32_t(plan_entry_bytes(k, e, true));
            r.stripes = s1 - s0;
            r.results = reinterpret_cast<uint64_t*>(d_results + s0);
            r.queue = nullptr;
            return to_status(hec::launch_scrub_mixed(r, int(e), c->device, stream));
        });
    });
}

// Pipelined pinned-host batch, 3 device slots and 3 streams:
//   h2d stream:     [wait kernel(q-3) done: input slot free] H2D(q)  -> ev_in[slot]
//   compute stream: [wait ev_in[slot], D2H(q-3) done: output slot free] encode(q) -> ev_k[slot]
//   d2h stream:     [wait ev_k[slot]] D2H(q) -> ev_out[slot]
// so chunk q+1's H2D, chunk q's encode and chunk q-1's D2H run concurrently
// (PCIe is full duplex; the SDMA engines serve both directions at once).
int hec_encode_host_batch(hec_coder_t* c, const uint8_t* h_data, uint8_t* h_parity, size_t cell_len,
                          size_t stripes, size_t chunk_stripes) {
    if (!c || !h_data || !h_parity || cell_len == 0 || chunk_stripes == 0) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (c->device == HEC_DEVICE_HOST) {  // host-only coder: the host routine, stripe by stripe
        return guarded([&] {
            const size_t k = c->k, m = c->m;
            const uint8_t* in[HEC_MAX_DATA_UNITS];
            uint8_t* out[HEC_MAX_PARITY_UNITS];
            for (size_t s = 0; s < stripes; s++) {
                for (size_t i = 0; i < k; i++) in[i] = h_data + (s * k + i) * cell_len;
                for (size_t j = 0; j < m; j++) out[j] = h_parity + (s * m + j) * cell_len;
                hec::host::gf_matmul_split(c->enc.data() + k * k, c->enc_aff.data(), m, k, in, out, cell_len);
            }
            return int(HEC_OK);
        });
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(c->host_mu);
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        StreamDrain drain{c};
        const size_t k = c->k, m = c->m;
        constexpr int kSlots = hec_coder::kSlots;
        chunk_stripes = std::min(chunk_stripes, stripes);
        const size_t in_bytes = chunk_stripes * k * cell_len;
        const size_t out_bytes = chunk_stripes * m * cell_len;
        const size_t slot_bytes = in_bytes + out_bytes;
        int rc = ensure_dbuf(c, kSlots * slot_bytes);
        if (rc != HEC_OK) return rc;
        hipStream_t h2d = c->copy_stream[0], d2h = c->copy_stream[1];
        const size_t nchunks = (stripes + chunk_stripes - 1) / chunk_stripes;
        for (size_t q = 0; q < nchunks; q++) {
            const int slot = int(q % kSlots);
            uint8_t* din = c->dbuf + slot * slot_bytes;
            uint8_t* dpar = din + in_bytes;
            const size_t s0 = q * chunk_stripes;
            const size_t ns = std::min(chunk_stripes, stripes - s0);
            if (q >= size_t(kSlots)) HEC_HIP(hipStreamWaitEvent(h2d, c->ev_k[slot], 0), HEC_ERR_DEVICE);
            HEC_HIP(hipMemcpyAsync(din, h_data + s0 * k * cell_len, ns * k * cell_len, hipMemcpyHostToDevice, h2d),
                    HEC_ERR_DEVICE);
            HEC_HIP(hipEventRecord(c->ev_in[slot], h2d), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamWaitEvent(c->stream, c->ev_in[slot], 0), HEC_ERR_DEVICE);
            if (q >= size_t(kSlots)) HEC_HIP(hipStreamWaitEvent(c->stream, c->ev_out[slot], 0), HEC_ERR_DEVICE);
            const uint8_t* in[HEC_MAX_DATA_UNITS];
            uint8_t* out[HEC_MAX_PARITY_UNITS];
            size_t ist[HEC_MAX_DATA_UNITS], ost[HEC_MAX_PARITY_UNITS];
            for (size_t i = 0; i < k; i++) {
                in[i] = din + i * cell_len;
                ist[i] = k * cell_len;
            }
            for (size_t j = 0; j < m; j++) {
                out[j] = dpar + j * cell_len;
                ost[j] = m * cell_len;
            }
            rc = matmul_batch(c->device, c->enc.data() + k * k, m, k, in, ist, out, ost, cell_len, ns, c->stream);
            if (rc != HEC_OK) return rc;
            HEC_HIP(hipEventRecord(c->ev_k[slot], c->stream), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamWaitEvent(d2h, c->ev_k[slot], 0), HEC_ERR_DEVICE);
            HEC_HIP(hipMemcpyAsync(h_parity + s0 * m * cell_len, dpar, ns * m * cell_len, hipMemcpyDeviceToHost, d2h),
                    HEC_ERR_DEVICE);
            HEC_HIP(hipEventRecord(c->ev_out[slot], d2h), HEC_ERR_DEVICE);
        }
        HEC_HIP(hipStreamSynchronize(h2d), HEC_ERR_DEVICE);
        HEC_HIP(hipStreamSynchronize(c->stream), HEC_ERR_DEVICE);
        HEC_HIP(hipStreamSynchronize(d2h), HEC_ERR_DEVICE);
        return HEC_OK;
    });
}

// Pipelined pinned-host decode straight into file order (the reader's
// ec_decode + cell split + concatenation, ec/mod.rs:62-89 and
// block_reader.rs:480-554, in one pass).  The k survivors go H2D, one
// contiguous copy per shard per chunk; the decode kernel writes the e missing
// cells to a compact region; only those come back D2H, each as a 2D copy into
// its file slots.  The present data
// cells never make the round trip: host threads copy them from the vertical
// buffers into their file slots while the DMA engines run, so PCIe carries
// k cells in and e cells out per row instead of k in and k out.
int hec_decode_host_batch(hec_coder_t* c, const uint8_t* const* h_vertical, size_t cell_len, size_t rows,
                          uint8_t* h_file, size_t chunk_rows) {
    if (!c || !h_vertical || !h_file || cell_len == 0 || chunk_rows == 0) return HEC_ERR_INVALID_ARG;
    if (rows == 0) return HEC_OK;
    return guarded([&] {
        const size_t k = c->k, m = c->m;
        uint8_t present[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < k + m; i++) present[i] = h_vertical[i] != nullptr;
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;

        // host side: present data cells -> file slots, rows split over up to
        // 4 threads (the caller's thread takes the first share)
        auto copy_rows = [&](size_t ra, size_t rb) {
            for (size_t r = ra; r < rb; r++)
                for (size_t i = 0; i < k; i++)
                    if (h_vertical[i])
                        std::memcpy(h_file + (r * k + i) * cell_len, h_vertical[i] + r * cell_len, cell_len);
        };
        const size_t copy_bytes = rows * (k - p.missing.size()) * cell_len;
        const int tuned_threads = hec::tune_snapshot().host_copy_threads;
        const size_t max_threads = tuned_threads > 0 ? size_t(tuned_threads) : 4;
        const size_t nthreads = std::min<size_t>(max_threads, std::max<size_t>(1, copy_bytes >> 24));  // >= 16 MiB each
        std::vector<std::thread> copiers;
        auto join_copiers = [&] {
            for (auto& t : copiers) t.join();
            copiers.clear();
        };
        size_t own_a = 0, own_b = rows;
        if (nthreads > 1) {
            copiers.reserve(nthreads - 1);
            for (size_t t = 1; t < nthreads; t++) {
                const size_t ra = rows * t / nthreads, rb = rows * (t + 1) / nthreads;
                try {
                    copiers.emplace_back(copy_rows, ra, rb);
                } catch (...) {
                    copy_rows(ra, rb);  // no thread: copy inline
                }
            }
            own_b = rows / nthreads;
        }
        if (p.missing.empty()) {  // nothing to rebuild: a pure host copy
            copy_rows(own_a, own_b);
            join_copiers();
            return HEC_OK;
        }

        int rc = [&]() -> int {
            if (c->device == HEC_DEVICE_HOST) {  // host-only coder: rebuild row by row on this thread
                const size_t e = p.missing.size();
                const uint8_t* in[HEC_MAX_DATA_UNITS];
                uint8_t* out[HEC_MAX_DATA_UNITS];
                for (size_t r = 0; r < rows; r++) {
                    for (size_t i = 0; i < k; i++) in[i] = h_vertical[p.survivors[i]] + r * cell_len;
                    for (size_t i = 0; i < e; i++) out[i] = h_file + (r * k + p.missing[i]) * cell_len;
                    hec::host::gf_matmul_split(p.matrix.data(), p.aff.data(), e, k, in, out, cell_len);
                }
                copy_rows(own_a, own_b);
                return int(HEC_OK);
            }
            std::lock_guard<std::mutex> lk(c->host_mu);
            DeviceGuard g(c->device);
            if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
            StreamDrain drain{c};  // before join_copiers and before returning, also on errors
            constexpr int kSlots = hec_coder::kSlots;
            chunk_rows = std::min(chunk_rows, rows);
            // slot: the k survivors shard-major [k][chunk][cell] (one
            // contiguous H2D per survivor), then the e rebuilt cells
            // [e][chunk][cell] (one 2D D2H per missing shard into its file slots)
            const size_t e = p.missing.size();
            const size_t shard_bytes = chunk_rows * cell_len;
            const size_t slot_bytes = (k + e) * shard_bytes;
            int rc2 = ensure_dbuf(c, kSlots * slot_bytes);
            if (rc2 != HEC_OK) return rc2;
            hipStream_t h2d = c->copy_stream[0], d2h = c->copy_stream[1];
            const size_t nchunks = (rows + chunk_rows - 1) / chunk_rows;
            for (size_t q = 0; q < nchunks; q++) {
                const int slot = int(q % kSlots);
                uint8_t* dsurv = c->dbuf + slot * slot_bytes;
                uint8_t* dmiss = dsurv + k * shard_bytes;
                const size_t r0 = q * chunk_rows;
                const size_t nr = std::min(chunk_rows, rows - r0);
                // slot reuse: the D2H of chunk q-3 (which follows its kernel) is done
                if (q >= size_t(kSlots)) HEC_HIP(hipStreamWaitEvent(h2d, c->ev_out[slot], 0), HEC_ERR_DEVICE);
                for (size_t r = 0; r < k; r++)
                    HEC_HIP(hipMemcpyAsync(dsurv + r * shard_bytes, h_vertical[p.survivors[r]] + r0 * cell_len,
                                           nr * cell_len, hipMemcpyHostToDevice, h2d),
                            HEC_ERR_DEVICE);
                HEC_HIP(hipEventRecord(c->ev_in[slot], h2d), HEC_ERR_DEVICE);
                HEC_HIP(hipStreamWaitEvent(c->stream, c->ev_in[slot], 0), HEC_ERR_DEVICE);
                const uint8_t* in[HEC_MAX_DATA_UNITS];
                size_t ist[HEC_MAX_DATA_UNITS];
                uint8_t* out[HEC_MAX_DATA_UNITS];
                size_t ost[HEC_MAX_DATA_UNITS];
                for (size_t r = 0; r < k; r++) {
                    in[r] = dsurv + r * shard_bytes;
                    ist[r] = cell_len;
                }
                for (size_t r = 0; r < e; r++) {
                    out[r] = dmiss + r * shard_bytes;
                    ost[r] = cell_len;
                }
                rc2 = matmul_batch(c->device, p.matrix.data(), e, k, in, ist, out, ost, cell_len, nr, c->stream);
                if (rc2 != HEC_OK) return rc2;
                HEC_HIP(hipEventRecord(c->ev_k[slot], c->stream), HEC_ERR_DEVICE);
                HEC_HIP(hipStreamWaitEvent(d2h, c->ev_k[slot], 0), HEC_ERR_DEVICE);
                for (size_t r = 0; r < e; r++)  // rebuilt cells only, into their file slots
                    HEC_HIP(hipMemcpy2DAsync(h_file + (r0 * k + p.missing[r]) * cell_len, k * cell_len,
                                             dmiss + r * shard_bytes, cell_len, cell_len, nr, hipMemcpyDeviceToHost,
                                             d2h),
                            HEC_ERR_DEVICE);
                HEC_HIP(hipEventRecord(c->ev_out[slot], d2h), HEC_ERR_DEVICE);
            }
            // every chunk is enqueued (the waits are device-side): the caller's
            // host share runs while the DMA engines and the kernel work
            copy_rows(own_a, own_b);
            HEC_HIP(hipStreamSynchronize(h2d), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamSynchronize(c->stream), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamSynchronize(d2h), HEC_ERR_DEVICE);
            return HEC_OK;
        }();
        join_copiers();  // always, also on a device error (never leave a joinable thread)
        return rc;
    });
}

// ---- whole files: rows of k cells, the last one possibly short ---------------
// CellBuffer (block_writer.rs:791-851) fills cell 0 of a row before cell 1,
// so the last row of a file of data_len bytes holds L = data_len - full*k*cell
// bytes: cell i has min(cell, max(0, L - i*cell)) of them, and encode pads
// every cell with zeros to len(cell 0) = n0 = min(cell, L) and emits parity
// cells of n0 bytes.  The reader pads every short or absent cell with zeros
// to cell_size (CellReader::next_cell, block_reader.rs:343-378) before
// ec_decode, then trims the row to the file length (:524-549).

size_t hec_encode_rows_workspace_size(const hec_coder_t* c, size_t cell_len) {
    if (!c) return 0;
    return c->k * cell_len;  // the last row's short data cells, zero-padded
}

int hec_encode_rows_host(hec_coder_t* c, const uint8_t* h_data, size_t data_len, uint8_t* h_parity, size_t cell_len,
                         size_t chunk_stripes) {
    if (!c || !h_data || !h_parity || cell_len == 0 || chunk_stripes == 0) return HEC_ERR_INVALID_ARG;
    if (data_len == 0) return HEC_OK;
    const size_t k = c->k, m = c->m, row = k * cell_len;
    const size_t full = data_len / row, L = data_len - full * row;
    if (full) {
        const int rc = hec_encode_host_batch(c, h_data, h_parity, cell_len, full, chunk_stripes);
        if (rc != HEC_OK || L == 0) return rc;
    }
    return guarded([&] {
        // the short last row: cells padded to n0 on the host, one row coded
        const size_t n0 = std::min(cell_len, L);
        const uint8_t* base = h_data + full * row;
        std::vector<uint8_t> pad(k * n0, 0);
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        uint8_t* out[HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < k; i++) {
            const size_t have = L > i * cell_len ? std::min(cell_len, L - i * cell_len) : 0;
            if (have == n0) {
                in[i] = base + i * cell_len;  // a full-length cell is read in place
            } else {
                std::memcpy(&pad[i * n0], base + i * cell_len, have);
                in[i] = &pad[i * n0];
            }
        }
        uint8_t* pbase = h_parity + full * m * cell_len;
        for (size_t j = 0; j < m; j++) {
            out[j] = pbase + j * cell_len;
            std::memset(out[j] + n0, 0, cell_len - n0);  // the parity cell holds n0 bytes
        }
        return code_row(c, c->enc.data() + k * k, c->enc_aff.data(), in, k, out, m, n0);
    });
}

int hec_encode_rows_device(hec_coder_t* c, const uint8_t* d_data, size_t data_len, uint8_t* d_parity, size_t cell_len,
                           void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_encode_rows_device");
    if (!c || !d_data || !d_parity || cell_len == 0) return HEC_ERR_INVALID_ARG;
    if (data_len == 0) return HEC_OK;
    const size_t k = c->k, m = c->m, row = k * cell_len;
    const size_t full = data_len / row, L = data_len - full * row;
    const uint8_t* din[HEC_MAX_DATA_UNITS];
    uint8_t* dout[HEC_MAX_PARITY_UNITS];
    size_t ist[HEC_MAX_DATA_UNITS], ost[HEC_MAX_PARITY_UNITS];
    for (size_t i = 0; i < k; i++) {
        din[i] = d_data + i * cell_len;
        ist[i] = row;
    }
    for (size_t j = 0; j < m; j++) {
        dout[j] = d_parity + j * cell_len;
        ost[j] = m * cell_len;
    }
    // validate the workspace before anything is queued: a bad argument must not
    // leave the full rows' parity written and the short row's not.  It is
    // needed only when some cell of the short last row holds fewer than
    // n0 = min(cell, L) bytes (the zero-padded copies); k == 1, or a short
    // row whose cells all reach n0, needs none.
    const size_t n0 = std::min(cell_len, L);
    bool pad = false;
    for (size_t i = 0; i < k && L; i++) pad |= (L > i * cell_len ? std::min(cell_len, L - i * cell_len) : 0) < n0;
    if (pad && (!d_workspace || workspace_bytes < k * n0)) return HEC_ERR_INVALID_ARG;
    if (full) {
        const int rc = hec_encode_device(c, din, ist, dout, ost, cell_len, full, hip_stream);
        if (rc != HEC_OK || L == 0) return rc;
    }
    return guarded([&] {
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        const uint8_t* base = d_data + full * row;
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        for (size_t i = 0; i < k; i++) {
            const size_t have = L > i * cell_len ? std::min(cell_len, L - i * cell_len) : 0;
            din[i] = base + i * cell_len;
            if (have < n0) {  // short or empty cell: zero-padded copy (never read past the data)
                uint8_t* p = ws + i * n0;
                if (have)
                    HEC_HIP(hipMemcpyAsync(p, base + i * cell_len, have, hipMemcpyDeviceToDevice, stream),
                            HEC_ERR_DEVICE);
                HEC_HIP(hipMemsetAsync(p + have, 0, n0 - have, stream), HEC_ERR_DEVICE);
                din[i] = p;
            }
        }
        for (size_t j = 0; j < m; j++) {
            dout[j] = d_parity + full * m * cell_len + j * cell_len;
            if (n0 < cell_len) HEC_HIP(hipMemsetAsync(dout[j] + n0, 0, cell_len - n0, stream), HEC_ERR_DEVICE);
        }
        return matmul_batch(c->device, c->enc.data() + k * k, m, k, din, ist, dout, ost, n0, 1, stream);
    });
}

int hec_decode_rows_host(hec_coder_t* c, const uint8_t* const* h_vertical, const size_t* vertical_len,
                         size_t cell_len, uint8_t* h_file, size_t file_len, size_t chunk_rows) {
    if (!c || !h_vertical || !vertical_len || !h_file || cell_len == 0 || chunk_rows == 0) return HEC_ERR_INVALID_ARG;
    if (file_len == 0) return HEC_OK;
    const size_t k = c->k, m = c->m, row = k * cell_len;
    const size_t full = file_len / row, L = file_len - full * row;
    // full rows: every present shard holds full * cell_len bytes (max_offset)
    for (size_t i = 0; i < k + m; i++)
        if (h_vertical[i] && vertical_len[i] < full * cell_len) return HEC_ERR_INVALID_ARG;
    if (full) {
        const int rc = hec_decode_host_batch(c, h_vertical, cell_len, full, h_file, chunk_rows);
        if (rc != HEC_OK || L == 0) return rc;
    }
    return guarded([&] {
        // the short last row: each present cell zero-padded (CellReader), only
        // the first n0 = min(cell, L) bytes carry data (every data cell of the
        // row is zero past n0, so are the parity cells)
        const size_t n0 = std::min(cell_len, L);
        uint8_t present[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < k + m; i++) present[i] = h_vertical[i] != nullptr;
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;
        uint8_t* frow = h_file + full * row;
        auto cell_have = [&](size_t i) {  // bytes of cell i of the row inside the file
            return L > i * cell_len ? std::min(cell_len, L - i * cell_len) : size_t(0);
        };
        for (size_t i = 0; i < k; i++) {  // present data cells: copied, zero-padded
            if (!h_vertical[i]) continue;
            const size_t want = cell_have(i);
            const size_t avail = vertical_len[i] > full * cell_len ? vertical_len[i] - full * cell_len : 0;
            const size_t cp = std::min(want, avail);
            std::memcpy(frow + i * cell_len, h_vertical[i] + full * cell_len, cp);
            std::memset(frow + i * cell_len + cp, 0, want - cp);
        }
        if (p.missing.empty()) return int(HEC_OK);
        std::vector<uint8_t> surv(k * n0, 0), rec(p.missing.size() * n0);
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        uint8_t* out[HEC_MAX_DATA_UNITS];
        for (size_t r = 0; r < k; r++) {
            const size_t s = p.survivors[r];
            const size_t avail = vertical_len[s] > full * cell_len ? vertical_len[s] - full * cell_len : 0;
            std::memcpy(&surv[r * n0], h_vertical[s] + full * cell_len, std::min(avail, n0));
            in[r] = &surv[r * n0];
        }
        for (size_t r = 0; r < p.missing.size(); r++) out[r] = &rec[r * n0];
        const int rc = code_row(c, p.matrix.data(), p.aff.data(), in, k, out, p.missing.size(), n0);
        if (rc != HEC_OK) return rc;
        for (size_t r = 0; r < p.missing.size(); r++) {
            const size_t i = p.missing[r];
            std::memcpy(frow + i * cell_len, &rec[r * n0], cell_have(i));
        }
        return int(HEC_OK);
    });
}

// ---- Chunk checksums ------------------------------------

namespace {

// HEC_CHECKSUM_* (ChecksumTypeProto) -> crc::Kind; -1 for NULL / invalid
int crc_kind(int checksum_type) {
    switch (checksum_type) {
        case HEC_CHECKSUM_CRC32C: return hec::crc::kCrc32c;
        case HEC_CHECKSUM_CRC32: return hec::crc::kCksum;
        default: return -1;
    }
}

// One checksum launch over n_shards cells per stripe; cell (s, i) sits at
// s * n_total + sid[i] in the sums/flags layouts (sid == nullptr: identity).
int checksum_launch(hec_coder* c, int kind, const uint8_t* const* bases, const size_t* strides, const uint8_t* sid,
                    size_t n_shards, size_t n_total, size_t cell_len, size_t stripes, size_t bpc, uint8_t* out,
                    const uint8_t* expected, uint8_t* bad, hipStream_t stream,
                    const uint32_t* stripe_list = nullptr) {
    hec::CrcArgs a;
    std::memset(&a, 0, sizeof(a));
    a.stripe_list = stripe_list;
    for (size_t i = 0; i < n_shards; i++) {
        if (!bases[i]) return HEC_ERR_INVALID_ARG;
        a.base[i] = bases[i];
        a.stride[i] = strides[i];
        a.sid[i] = uint8_t(sid ? sid[i] : i);
    }
    a.n_total = uint32_t(n_total);
    a.out = out;
    a.expected = expected;
    a.bad = bad;
    a.kind = kind;
    a.n_shards = uint32_t(n_shards);
    a.cell_len = cell_len;
    a.stripes = stripes;
    a.bytes_per_checksum = bpc;
    const int rc = hec::launch_checksum(a, c->device, stream);
    return rc == 0 ? HEC_OK : to_status(rc);
}

int checksum_entry(hec_coder* c, int checksum_type, const uint8_t* const* d_bases, const size_t* strides,
                   size_t n_shards, size_t cell_len, size_t stripes, size_t bpc, uint8_t* d_out,
                   const uint8_t* d_expected, uint8_t* d_bad, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("checksum_entry");
    const int kind = crc_kind(checksum_type);
    if (!c || !d_bases || !strides || kind < 0 || n_shards == 0 || n_shards > size_t(hec::kCrcMaxShards) ||
        cell_len == 0 || bpc == 0 || (!d_out && !d_expected) || (d_expected && !d_bad))
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_shards; i++)
        if (!d_bases[i]) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    return guarded([&] {
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        return checksum_launch(c, kind, d_bases, strides, nullptr, n_shards, n_shards, cell_len, stripes, bpc, d_out,
                               d_expected, d_bad, static_cast<hipStream_t>(hip_stream));
    });
}

}  // namespace

int hec_crc32c_device(hec_coder_t* c, const uint8_t* const* d_bases, const size_t* strides, size_t n_shards,
                      size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint8_t* d_out, void* hip_stream) {
    if (!d_out) return HEC_ERR_INVALID_ARG;
    return checksum_entry(c, HEC_CHECKSUM_CRC32C, d_bases, strides, n_shards, cell_len, stripes, bytes_per_checksum,
                          d_out, nullptr, nullptr, hip_stream);
}

int hec_checksum_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_bases, const size_t* strides,
                        size_t n_shards, size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint8_t* d_out,
                        void* hip_stream) {
    if (!d_out) return HEC_ERR_INVALID_ARG;
    return checksum_entry(c, checksum_type, d_bases, strides, n_shards, cell_len, stripes, bytes_per_checksum, d_out,
                          nullptr, nullptr, hip_stream);
}

int hec_checksum_verify_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_bases,
                               const size_t* strides, size_t n_shards, size_t cell_len, size_t stripes,
                               size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                               void* hip_stream) {
    if (checksum_type == HEC_CHECKSUM_NULL) return c ? HEC_OK : HEC_ERR_INVALID_ARG;
    if (!d_expected || !d_bad) return HEC_ERR_INVALID_ARG;
    return checksum_entry(c, checksum_type, d_bases, strides, n_shards, cell_len, stripes, bytes_per_checksum,
                          nullptr, d_expected, d_bad, hip_stream);
}

// ---- Composite CRCs (crc_compose.hpp): cell, unit and group sums from chunk sums ----

int hec_crc_concat(int checksum_type, uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t* out) {
    const int kind = crc_kind(checksum_type);
    if (kind < 0 || !out) return HEC_ERR_INVALID_ARG;
    *out = kind == hec::crc::kCrc32c ? hec::crc::concat<hec::crc::kCrc32c>(crc_a, crc_b, len_b)
                                     : hec::crc::concat<hec::crc::kCksum>(crc_a, crc_b, len_b);
    return HEC_OK;
}

int hec_composite_crc(int checksum_type, const uint8_t* sums, size_t n_units, size_t data_units, size_t cell_len,
                      size_t stripes, size_t bytes_per_checksum, uint64_t data_len, uint8_t* cell_crcs,
                      uint8_t* unit_crcs, uint8_t* group_crc) {
    const int kind = crc_kind(checksum_type);
    hec::crc::Geometry g;
    if (kind < 0 || !sums ||
        !hec::crc::make_geometry(n_units, data_units, cell_len, stripes, bytes_per_checksum, data_len, &g))
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    return guarded([&] {
        if (kind == hec::crc::kCrc32c)
            hec::crc::composite_host<hec::crc::kCrc32c>(g, sums, cell_crcs, unit_crcs, group_crc);
        else
            hec::crc::composite_host<hec::crc::kCksum>(g, sums, cell_crcs, unit_crcs, group_crc);
        return int(HEC_OK);
    });
}

size_t hec_composite_crc_workspace_size(size_t n_units, size_t stripes) {
    if (n_units < 1 || n_units > hec::crc::kComposeMaxUnits) return 0;
    return size_t(hec::crc::compose_workspace_bytes(n_units, stripes));
}

int hec_composite_crc_device(hec_coder_t* c, int checksum_type, const uint8_t* d_sums, size_t n_units,
                             size_t data_units, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                             uint64_t data_len, uint8_t* d_cell_crcs, uint8_t* d_unit_crcs, uint8_t* d_group_crc,
                             void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_composite_crc_device");
    const int kind = crc_kind(checksum_type);
    hec::crc::Geometry g;
    const uintptr_t align = reinterpret_cast<uintptr_t>(d_sums) | reinterpret_cast<uintptr_t>(d_cell_crcs) |
                            reinterpret_cast<uintptr_t>(d_unit_crcs) | reinterpret_cast<uintptr_t>(d_group_crc);
    if (!c || !d_sums || kind < 0 || (align & 3u) ||
        !hec::crc::make_geometry(n_units, data_units, cell_len, stripes, bytes_per_checksum, data_len, &g))
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0 || (!d_cell_crcs && !d_unit_crcs && !d_group_crc)) return HEC_OK;
    if ((d_unit_crcs || d_group_crc) &&
        (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 3u) ||
         workspace_bytes < hec::crc::compose_workspace_bytes(n_units, stripes)))
        return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        DeviceGuard dg(c->device);
        if (!dg.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const int rc = hec::launch_composite_crc(kind, g, d_sums, d_cell_crcs, d_unit_crcs, d_group_crc, d_workspace,
                                                 c->device, static_cast<hipStream_t>(hip_stream));
        return rc == 0 ? int(HEC_OK) : to_status(rc);
    });
}

int hec_encode_crc_device(hec_coder_t* c, const uint8_t* const* d_data, const size_t* data_strides,
                          uint8_t* const* d_parity, const size_t* parity_strides, size_t cell_len, size_t stripes,
                          size_t bytes_per_checksum, uint8_t* d_sums, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_encode_crc_device");
    if (!c || !d_data || !data_strides || !d_parity || !parity_strides || !d_sums || cell_len == 0 ||
        bytes_per_checksum == 0)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    // Fused single pass when the shape allows it (k in {2,3,6,10}, m <= 4,
    // 512-B chunks, 16-B aligned cells); otherwise encode, then checksum.
    if (bytes_per_checksum == 512 && c->m <= size_t(hec::kMaxR) && !hec::tune_snapshot().crc_unfused) {
        const int rc = guarded([&] {
            DeviceGuard g(c->device);
            if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
            hec::MatmulArgs a;
            std::memset(&a, 0, sizeof(a));
            for (size_t i = 0; i < c->k; i++) {
                if (!d_data[i]) return int(HEC_ERR_INVALID_ARG);
                a.in[i] = d_data[i];
                a.in_stride[i] = data_strides[i];
            }
            for (size_t j = 0; j < c->m; j++) {
                if (!d_parity[j]) return int(HEC_ERR_INVALID_ARG);
                a.out[j] = d_parity[j];
                a.out_stride[j] = parity_strides[j];
                for (size_t i = 0; i < c->k; i++) a.coef[j * hec::kMaxK + i] = c->enc[(c->k + j) * c->k + i];
            }
            a.k = int32_t(c->k);
            a.r = int32_t(c->m);
            a.cell_len = cell_len;
            a.stripes = stripes;
            hec::FusedCrcArgs cs;
            std::memset(&cs, 0, sizeof(cs));
            cs.sums = d_sums;
            cs.n_total = uint32_t(c->k + c->m);
            cs.kind = hec::crc::kCrc32c;
            for (size_t i = 0; i < c->k + c->m; i++) cs.shard_id[i] = uint8_t(i);
            const int lrc = hec::launch_encode_crc(a, cs, c->device, static_cast<hipStream_t>(hip_stream));
            if (lrc == -1) return 1;  // shape not covered: fall through
            return lrc == 0 ? int(HEC_OK) : to_status(lrc);
        });
        if (rc != 1) return rc;
    }
    int rc = hec_encode_device(c, d_data, data_strides, d_parity, parity_strides, cell_len, stripes, hip_stream);
    if (rc != HEC_OK) return rc;
    const uint8_t* bases[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    size_t st[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    for (size_t i = 0; i < c->k; i++) {
        bases[i] = d_data[i];
        st[i] = data_strides[i];
    }
    for (size_t j = 0; j < c->m; j++) {
        bases[c->k + j] = d_parity[j];
        st[c->k + j] = parity_strides[j];
    }
    return hec_crc32c_device(c, bases, st, c->k + c->m, cell_len, stripes, bytes_per_checksum, d_sums, hip_stream);
}

// The verified striped read (block_reader.rs:480-525 -> ec_decode): phase 1
// verifies the batch plan's survivors of every stripe and rebuilds its
// missing data in one pass; phase 2 re-plans, one stripe at a time, the
// stripes where a survivor failed: drop it, take the next available shard
// (verifying it first, as read_slice starts the next parity reader), and
// rebuild every missing or failed data cell of that stripe.
// ---- plan-time specialisation of the fused decode + verify kernel (jit.hpp) ----

int hec_coder_prepare_decode(hec_coder_t* c, const uint8_t* present, int checksum_type, int* specialised) {
    if (specialised) *specialised = 0;
    if (!c || !present) return HEC_ERR_INVALID_ARG;
    const int kind = crc_kind(checksum_type);
    if (kind < 0) return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_coder_prepare_decode");
    return guarded([&]() -> int {
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;
        if (p.missing.empty() || p.missing.size() > size_t(hec::kMaxR)) return int(HEC_OK);  // no fused decode
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        hec::jit::VerifyKernel vk;
        const int e = int(p.missing.size());
        const hec::Tune tn = hec::tune_snapshot();
        const int slabs = (tn.fused_slabs == 4 || tn.fused_slabs == 8) ? tn.fused_slabs
                                                                        : hec::jit::default_slabs(int(c->k), e);
        const int pfd = hec::jit::pick_pfd(tn.jit_pfd, slabs, int(c->k), e);
        const int wpe = tn.fused_wpe == 3 && slabs == 4 ? 3 : 2;
        const int scheme = tn.crc_variant == 12 && kind == 0 ? 15 : 12;  // measurement: slicing-by-32 tail
        // the launch's choice (ec_fused.hip launch_fused; measurement: tune key 28)
        const bool wq = (hec::kExperimental && tn.fused_wq) ? tn.fused_wq == 1 : hec::jit::default_wq(int(c->k), e);
        const bool ok = hec::jit::verify_kernel(c->device, int(c->k), e, kind, slabs, wpe, pfd, p.matrix.data(), true,
                                                &vk, scheme, wq);
        if (specialised) *specialised = ok ? 1 : 0;
        return int(HEC_OK);
    });
}

int hec_jit_warm(size_t data_units, size_t parity_units, const uint8_t* present, int checksum_type) {
    if (!present || data_units == 0 || data_units > HEC_MAX_DATA_UNITS || parity_units == 0 ||
        parity_units > HEC_MAX_PARITY_UNITS)
        return HEC_ERR_INVALID_ARG;
    const int kind = crc_kind(checksum_type);
    if (kind < 0) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        size_t e = 0, surv[HEC_MAX_DATA_UNITS], miss[HEC_MAX_DATA_UNITS];
        uint8_t mat[HEC_MAX_DATA_UNITS * HEC_MAX_DATA_UNITS];
        const int rc = hec_decode_plan(data_units, parity_units, present, &e, surv, miss, mat);
        if (rc != HEC_OK) return rc;
        const size_t k = data_units;
        if (e == 0 || e > size_t(hec::kMaxR) || !(k == 2 || k == 3 || k == 6 || k == 10)) return int(HEC_ERR_INVALID_ARG);
        return hec::jit::warm(int(k), int(e), kind, hec::jit::default_slabs(int(k), int(e)), 2,
                              hec::jit::default_pfd(int(k), int(e)), mat, 12,
                              hec::jit::default_wq(int(k), int(e))) ? int(HEC_OK)
                                                         : fail(HEC_ERR_DEVICE, "hiprtc compile", hipErrorNotSupported);
    });
}

void hec_jit_stats(uint64_t* compiled, uint64_t* from_disk, uint64_t* failed, uint64_t* launches) {
    const hec::jit::Stats st = hec::jit::stats();
    if (compiled) *compiled = st.compiled;
    if (from_disk) *from_disk = st.from_disk;
    if (failed) *failed = st.failed;
    if (launches) *launches = st.launches;
}

int hec_decode_verify_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                             const size_t* shard_strides, uint8_t* const* d_out, const size_t* out_strides,
                             size_t cell_len, size_t stripes, size_t bytes_per_checksum, const uint8_t* d_sums,
                             uint8_t* d_bad, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_decode_verify_device");
    if (!c || !d_shards || !shard_strides || !d_out || !out_strides || cell_len == 0) return HEC_ERR_INVALID_ARG;
    if (checksum_type == HEC_CHECKSUM_NULL)
        return hec_decode_device(c, d_shards, shard_strides, d_out, out_strides, cell_len, stripes, hip_stream);
    const int kind = crc_kind(checksum_type);
    if (kind < 0 || bytes_per_checksum == 0 || !d_sums || !d_bad) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k; i++)
        if (!d_out[i]) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    return guarded([&]() -> int {
        const size_t k = c->k, n = c->k + c->m;
        const hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        uint8_t present[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        for (size_t i = 0; i < n; i++) present[i] = d_shards[i] != nullptr;
        const PlanRef p_ref = cached_plan(c, present);
        const DecodePlan& p = *p_ref;
        if (p.status != HEC_OK) return p.status;  // fewer than k available: nothing is read
        std::vector<size_t> surv = p.survivors;
        if (p.missing.empty())
            for (size_t i = 0; i < k; i++) surv.push_back(i);  // nothing to rebuild: the data cells are read
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        HEC_HIP(hipMemsetAsync(d_bad, 0, stripes * n, stream), HEC_ERR_DEVICE);

        // ---- phase 1: the whole batch under the batch plan
        const uint8_t* in[HEC_MAX_DATA_UNITS];
        size_t ist[HEC_MAX_DATA_UNITS];
        uint8_t sid[HEC_MAX_DATA_UNITS];
        for (size_t r = 0; r < k; r++) {
            in[r] = d_shards[surv[r]];
            ist[r] = shard_strides[surv[r]];
            sid[r] = uint8_t(surv[r]);
        }
        bool fused = false;
        if (!p.missing.empty() && p.missing.size() <= size_t(hec::kMaxR) && bytes_per_checksum == 512) {
            hec::MatmulArgs a;
            std::memset(&a, 0, sizeof(a));
            for (size_t r = 0; r < k; r++) {
                a.in[r] = in[r];
                a.in_stride[r] = ist[r];
            }
            for (size_t j = 0; j < p.missing.size(); j++) {
                a.out[j] = d_out[p.missing[j]];
                a.out_stride[j] = out_strides[p.missing[j]];
                for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = p.matrix[j * k + i];
            }
            a.k = int32_t(k);
            a.r = int32_t(p.missing.size());
            a.cell_len = cell_len;
            a.stripes = stripes;
            hec::FusedCrcArgs cs;
            std::memset(&cs, 0, sizeof(cs));
            cs.expected = d_sums;
            cs.bad = d_bad;
            cs.n_total = uint32_t(n);
            cs.kind = kind;
            for (size_t r = 0; r < k; r++) cs.shard_id[r] = sid[r];
            const int lrc = hec::launch_decode_verify(a, cs, c->device, stream);
            if (lrc > 0) return to_status(lrc);
            fused = lrc == 0;
        }
        if (!fused) {
            int rc = checksum_launch(c, kind, in, ist, sid, k, n, cell_len, stripes, bytes_per_checksum, nullptr,
                                     d_sums, d_bad, stream);
            if (rc != HEC_OK) return rc;
            if (!p.missing.empty()) {
                uint8_t* out[HEC_MAX_DATA_UNITS];
                size_t ost[HEC_MAX_DATA_UNITS];
                for (size_t j = 0; j < p.missing.size(); j++) {
                    out[j] = d_out[p.missing[j]];
                    ost[j] = out_strides[p.missing[j]];
                }
                rc = matmul_batch(c->device, p.matrix.data(), p.missing.size(), k, in, ist, out, ost, cell_len, stripes,
                                  stream);
                if (rc != HEC_OK) return rc;
            }
        }
        std::vector<uint8_t> bad(stripes * n);
        HEC_HIP(hipMemcpyAsync(bad.data(), d_bad, bad.size(), hipMemcpyDeviceToHost, stream), HEC_ERR_DEVICE);
        HEC_HIP(hipStreamSynchronize(stream), HEC_ERR_DEVICE);

        // ---- phase 2, batched over every stripe with a failed survivor.  A
        // round re-plans each such stripe on the host (drop what failed, take
        // the first k available shards), verifies every newly used cell of
        // every stripe with at most one checksum launch per shard index (a
        // stripe-list launch), and reads the flags back once.  At most m
        // rounds; then one mixed-pattern decode rebuilds every missing or
        // failed data cell of those stripes with its final plan.
        std::vector<uint32_t> F;  // stripes still being repaired
        for (size_t s = 0; s < stripes; s++) {
            bool any = false;
            for (size_t r = 0; r < k; r++) any |= bad[s * n + surv[r]] != 0;
            if (any) F.push_back(uint32_t(s));
        }
        if (F.empty()) return HEC_OK;
        // phase 2 uses the coder's shared device scratch (verify_ws): one
        // verifier at a time, and the stream drained before the lock is
        // released on every path (error returns included), so no queued
        // launch of ours still reads the scratch when another thread grows it
        std::lock_guard<std::mutex> vlk(c->verify_mu);
        struct DrainOnExit {
            hipStream_t s;
            ~DrainOnExit() {
                (void)hipStreamSynchronize(s);
                (void)hipGetLastError();
            }
        } drain_on_exit{stream};
        int status = HEC_OK;
        std::vector<uint8_t> ok(F.size() * n, 0);  // cell verified good
        for (size_t f = 0; f < F.size(); f++)
            for (size_t r = 0; r < k; r++) ok[f * n + surv[r]] = bad[F[f] * n + surv[r]] == 0;
        std::vector<uint8_t> active(F.size(), 1);
        const size_t nck = (cell_len + bytes_per_checksum - 1) / bytes_per_checksum;
        (void)nck;
        for (size_t round = 0; round <= c->m + 1; round++) {
            std::vector<std::vector<uint32_t>> lists(n);
            size_t todo_cells = 0;
            for (size_t f = 0; f < F.size(); f++) {
                if (!active[f]) continue;
                const uint8_t* row = &bad[F[f] * n];
                size_t picked = 0;
                for (size_t i = 0; i < n && picked < k; i++) {
                    if (!present[i] || row[i]) continue;
                    picked++;
                    if (!ok[f * n + i]) {
                        lists[i].push_back(F[f]);
                        todo_cells++;
                    }
                }
                if (picked < k) {  // fewer than k cells left that can verify
                    active[f] = 0;
                    status = HEC_ERR_NOT_ENOUGH_SHARDS;
                }
            }
            if (todo_cells == 0) break;
            // one upload of every list, one launch per shard index, one read-back
            std::vector<uint32_t> flat;
            std::vector<size_t> off(n, 0);
            for (size_t i = 0; i < n; i++) {
                off[i] = flat.size();
                flat.insert(flat.end(), lists[i].begin(), lists[i].end());
            }
            const size_t need = flat.size() * sizeof(uint32_t);
            if (c->verify_ws_bytes < need) {
                // stream-ordered: growing the scratch costs no device-wide sync
                if (c->verify_ws) (void)hipFreeAsync(c->verify_ws, stream);
                c->verify_ws = nullptr;
                c->verify_ws_bytes = 0;
                const size_t want = std::max(need, size_t(64) << 10);
                HEC_HIP(hipMallocAsync(reinterpret_cast<void**>(&c->verify_ws), want, stream), HEC_ERR_NO_MEMORY);
                c->verify_ws_bytes = want;
            }
            const uint32_t* d_lists = reinterpret_cast<const uint32_t*>(c->verify_ws);
            HEC_HIP(hipMemcpyAsync(c->verify_ws, flat.data(), need, hipMemcpyHostToDevice, stream), HEC_ERR_DEVICE);
            for (size_t i = 0; i < n; i++) {
                if (lists[i].empty()) continue;
                const uint8_t* tb[1] = {d_shards[i]};
                const size_t ts[1] = {shard_strides[i]};
                const uint8_t tid[1] = {uint8_t(i)};
                const int rc = checksum_launch(c, kind, tb, ts, tid, 1, n, cell_len, lists[i].size(), bytes_per_checksum,
                                               nullptr, d_sums, d_bad, stream, d_lists + off[i]);
                if (rc != HEC_OK) return rc;
            }
            HEC_HIP(hipMemcpyAsync(bad.data(), d_bad, bad.size(), hipMemcpyDeviceToHost, stream), HEC_ERR_DEVICE);
            HEC_HIP(hipStreamSynchronize(stream), HEC_ERR_DEVICE);  // also keeps `flat` alive through the upload
            for (size_t i = 0; i < n; i++)
                for (uint32_t s : lists[i]) {
                    const size_t f = size_t(std::lower_bound(F.begin(), F.end(), s) - F.begin());
                    ok[f * n + i] = bad[size_t(s) * n + i] == 0;
                }
        }
        // rebuild: final presence mask per repaired stripe, every other stripe
        // a no-op (nothing missing), one mixed-pattern decode launch
        const uint64_t all = n >= 64 ? ~uint64_t(0) : ((uint64_t(1) << n) - 1);
        std::vector<uint64_t> masks(stripes, all);
        bool any_rebuild = false;
        for (size_t f = 0; f < F.size(); f++) {
            if (!active[f]) continue;
            uint64_t mask = 0;
            for (size_t i = 0; i < n; i++)
                if (present[i] && !bad[size_t(F[f]) * n + i]) mask |= uint64_t(1) << i;
            masks[F[f]] = mask;
            any_rebuild = true;
        }
        if (any_rebuild) {
            const size_t ws_need = mixed_workspace(k, c->m, stripes);
            if (c->verify_ws_bytes < ws_need) {
                if (c->verify_ws) (void)hipFreeAsync(c->verify_ws, stream);
                c->verify_ws = nullptr;
                c->verify_ws_bytes = 0;
                HEC_HIP(hipMallocAsync(reinterpret_cast<void**>(&c->verify_ws), ws_need, stream), HEC_ERR_NO_MEMORY);
                c->verify_ws_bytes = ws_need;
            }
            // storage for shard indices no plan reads (absent for the whole batch)
            const uint8_t* shards_all[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
            for (size_t i = 0; i < n; i++) shards_all[i] = d_shards[i] ? d_shards[i] : d_out[0];
            const int rc = mixed_decode_impl(c, shards_all, shard_strides, d_out, out_strides, masks.data(), cell_len,
                                             stripes, c->verify_ws, c->verify_ws_bytes, hip_stream);
            if (rc != HEC_OK) return rc;
        }
        HEC_HIP(hipStreamSynchronize(stream), HEC_ERR_DEVICE);
        return status;
    });
}

// ---- verified reconstruction: chunk checksums in and out ---------------------
// hec_reconstruct_crc_device*: the reconstruct calls with the survivors' chunk
// sums verified and the rebuilt units' written in the same pass
// (ec_reconstruct_crc.hip), or as a composition of internal launches where
// the fused kernel does not take the shape.

}  // extern "C"

namespace {

// Where the storage of units comes from: d_shards or d_out with their strides.
template <typename P>
struct UnitTable {
    P const* base;
    const size_t* stride;
};

// What a verified call carries from its entry point to its launches; every
// entry point builds one behind its argument checks.  The encode calls: the
// shards are the data units, the outputs the parity units.
struct VerifiedCall {
    hec_coder* c;
    int kind;  // crc::Kind
    const uint8_t* const* d_shards;
    const size_t* shard_strides;
    uint8_t* const* d_out;  // null: the call writes no unit (sums only, scrub, read)
    const size_t* out_strides;
    size_t cell_len, bpc;
    const uint8_t* d_expected;  // null: nothing verified
    uint8_t* d_bad;
    uint8_t* d_sums;  // null: the call writes no sums (scrub, read)
    hipStream_t stream;
    size_t k() const { return c->k; }
    size_t n() const { return c->k + c->m; }
    UnitTable<const uint8_t*> shards() const { return {d_shards, shard_strides}; }
    UnitTable<uint8_t*> outs() const { return {d_out, out_strides}; }
};

// One group of stripes of a verified call that share a plan: its rows (null:
// a scrub group without an extra, sums only) and (mixed form) the device list
// of the group's stripes.
struct CrcGroupCall {
    const RowPlan* rp;
    size_t stripes;          // stripes of the group (entries of d_list)
    const uint32_t* d_list;  // null: stripes 0 .. stripes-1
    uint64_t mask = 0;       // the scrub calls: the units the group's stripes have; unused elsewhere
};

// The slots of an argument block to fill, from the first one on: the units'
// bases and strides (null: the block has none, as where only sums are
// computed) and their indices.
template <typename P, typename S>
struct UnitSlots {
    P* base;
    S* stride;
    uint8_t* id;
};

template <typename P, typename S>
UnitSlots<P, S> unit_slots(P* base, S* stride, uint8_t* id) {
    return {base, stride, id};
}

inline UnitSlots<uint8_t*, uint64_t> id_slots(uint8_t* id) { return {nullptr, nullptr, id}; }

// The units of a checksum launch (checksum_launch's bases, strides, sid).
struct UnitList {
    const uint8_t* base[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    size_t stride[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    uint8_t id[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    size_t cnt = 0;
    UnitSlots<const uint8_t*, size_t> slots() { return {base, stride, id}; }
};

template <typename T, typename P, typename S>
inline void fill_unit(size_t u, size_t slot, const UnitTable<T>& from, const UnitSlots<P, S>& to) {
    if (to.base) {
        to.base[slot] = from.base[u];
        to.stride[slot] = from.stride[u];
    }
    to.id[slot] = uint8_t(u);
}

// `count` units of a list, in its order, into the slots.
template <typename U, typename T, typename P, typename S>
void fill_units(const U* units, size_t count, const UnitTable<T>& from, const UnitSlots<P, S>& to) {
    for (size_t r = 0; r < count; r++) fill_unit(units[r], r, from, to);
}

// The k survivors of a plan into the slots.
template <typename T, typename P, typename S>
void fill_survivors(const RowPlan& rp, size_t k, const UnitTable<T>& from, const UnitSlots<P, S>& to) {
    fill_units(rp.plan->rec_survivors.data(), k, from, to);
}

// Rows j0 .. j0+rn-1 of a plan: row j0 + j's unit into slot j, its
// coefficients into coef[j*kMaxK + i].
template <typename T, typename P, typename S>
void fill_rows(const RowPlan& rp, size_t k, size_t j0, size_t rn, uint8_t* coef, const UnitTable<T>& from,
               const UnitSlots<P, S>& to) {
    const DecodePlan& p = *rp.plan;
    for (size_t j = 0; j < rn; j++) {
        const size_t row = rp.rows[j0 + j];
        fill_unit(p.lost[row], j, from, to);
        for (size_t i = 0; i < k; i++) coef[j * hec::kMaxK + i] = p.rec_matrix[row * k + i];
    }
}

// The units of a mask, ascending; returns how many.
size_t mask_units(uint64_t mask, uint8_t* units) {
    size_t cnt = 0;
    for (; mask; mask &= mask - 1) units[cnt++] = uint8_t(__builtin_ctzll(mask));
    return cnt;
}

// A fused launcher's return as the helpers pass it on: 0 ok, -1 refused
// (nothing launched), else HEC_*.
int fused_status(int rc) { return rc <= 0 ? rc : to_status(rc); }

// The byte route over `rows` rows, kMaxR per launch (one launch without a row
// where `even_empty`): fill(j0, rn) sets the rows' slots and, from the second
// launch on, clears what only the first launch does; launch() queues it.
template <typename Fill, typename Launch>
int byte_route_rows(size_t rows, bool even_empty, Fill&& fill, Launch&& launch) {
    for (size_t j0 = 0; j0 < rows || (even_empty && j0 == 0); j0 += size_t(hec::kMaxR)) {
        fill(j0, std::min(size_t(hec::kMaxR), rows - j0));
        const int rc = launch();
        if (rc != 0) return rc < 0 ? HEC_ERR_INVALID_ARG : to_status(rc);
    }
    return HEC_OK;
}

// What every entry point checks the same way, its buffers apart
// (recon_sums_buffers_check); kind < 0 = HEC_CHECKSUM_NULL, which only a call
// that can do without sums takes (`null_ok`).
int recon_crc_check(const hec_coder* c, int checksum_type, bool null_ok, size_t cell_len, size_t bpc, int* kind) {
    if (!c || cell_len == 0) return HEC_ERR_INVALID_ARG;
    *kind = -1;
    if (null_ok && checksum_type == HEC_CHECKSUM_NULL) return HEC_OK;
    *kind = crc_kind(checksum_type);
    return *kind < 0 || bpc == 0 ? HEC_ERR_INVALID_ARG : HEC_OK;
}

int recon_sums_buffers_check(const uint8_t* d_expected, const uint8_t* d_bad, const uint8_t* d_sums) {
    if (!d_sums || (reinterpret_cast<uintptr_t>(d_sums) & 3u) || (d_expected && !d_bad) ||
        (reinterpret_cast<uintptr_t>(d_expected) & 3u))
        return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// The shapes gf_reconstruct_crc takes (launch_reconstruct_crc checks the
// same): k, 512-B chunks, 16-B aligned cells.  The rows per plan and the
// units' bases are checked per group.
bool recon_crc_shape(const hec_coder* c, size_t cell_len, size_t bpc) {
    return register_kernel_k(c->k) && bpc == 512 && cell_len % 16 == 0;
}

// At most kMaxR rows, and 16-byte aligned survivors and (where the call
// writes them) targets.
bool recon_crc_group_aligned(const VerifiedCall& x, const CrcGroupCall& g) {
    if (g.rp->rows.size() > size_t(hec::kMaxR)) return false;
    uint64_t survivors = 0;
    for (size_t r = 0; r < x.k(); r++) survivors |= uint64_t(1) << g.rp->plan->rec_survivors[r];
    return aligned16(x.d_shards, x.shard_strides, survivors) &&
           (!x.d_out || aligned16(x.d_out, x.out_strides, g.rp->units()));
}

// The two argument blocks of a fused reconstruction launch over one group:
// the survivors in, the group's rows out (x.d_out == null: their sums only).
void recon_fused_args(const VerifiedCall& x, const CrcGroupCall& g, hec::MatmulArgs* a, hec::ReconCrcArgs* cs) {
    const size_t k = x.k(), r = g.rp->rows.size();
    std::memset(a, 0, sizeof(*a));
    std::memset(cs, 0, sizeof(*cs));
    fill_survivors(*g.rp, k, x.shards(), unit_slots(a->in, a->in_stride, cs->shard_id));
    fill_rows(*g.rp, k, 0, r, a->coef, x.outs(),
              x.d_out ? unit_slots(a->out, a->out_stride, cs->shard_id + k) : id_slots(cs->shard_id + k));
    a->k = int32_t(k);
    a->r = int32_t(r);
    a->cell_len = x.cell_len;
    a->stripes = g.stripes;
    cs->sums = x.d_sums;
    cs->expected = x.d_expected;
    cs->bad = x.d_bad;
    cs->n_total = uint32_t(x.n());
    cs->kind = x.kind;
    cs->stripe_list = g.d_list;
}

// The fused launch of one group.  0 ok, -1 refused by the launcher, else HEC_*.
int recon_crc_fused(const VerifiedCall& x, const CrcGroupCall& g) {
    hec::MatmulArgs a;
    hec::ReconCrcArgs cs;
    recon_fused_args(x, g, &a, &cs);
    return fused_status(hec::launch_reconstruct_crc(a, cs, x.c->device, x.stream));
}

// A checksum launch over units of a group's stripes: verified against
// x.d_expected (`verify`), or their sums written to x.d_sums.
int sums_launch(const VerifiedCall& x, const CrcGroupCall& g, bool verify, const UnitList& l) {
    return checksum_launch(x.c, x.kind, l.base, l.stride, l.id, l.cnt, x.n(), x.cell_len, g.stripes, x.bpc,
                           verify ? nullptr : x.d_sums, verify ? x.d_expected : nullptr, verify ? x.d_bad : nullptr,
                           x.stream, g.d_list);
}

// The survivors of a group verified by a checksum launch.
int verify_survivors(const VerifiedCall& x, const CrcGroupCall& g) {
    UnitList l;
    l.cnt = x.k();
    fill_survivors(*g.rp, l.cnt, x.shards(), l.slots());
    return sums_launch(x, g, true, l);
}

// Composition, last step: the rebuilt units of a group, read back from d_out,
// checksummed.
int recon_crc_sums_pass(const VerifiedCall& x, const CrcGroupCall& g) {
    UnitList l;
    for (l.cnt = 0; l.cnt < g.rp->rows.size(); l.cnt++) fill_unit(g.rp->unit(l.cnt), l.cnt, x.outs(), l.slots());
    return sums_launch(x, g, false, l);
}

}  // namespace

extern "C" {

int hec_reconstruct_crc_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                               const size_t* shard_strides, uint8_t* const* d_out, const size_t* out_strides,
                               const uint8_t* want, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                               const uint8_t* d_expected, uint8_t* d_bad, uint8_t* d_sums, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_crc_device");
    int kind;
    const int chk = recon_crc_check(c, checksum_type, true, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    if (kind < 0)
        return hec_reconstruct_device(c, d_shards, shard_strides, d_out, out_strides, want, cell_len, stripes,
                                      hip_stream);
    if (recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK || !d_shards || !shard_strides)
        return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        RowPlan rp;
        const int prc = resolve_reconstruct(c, d_shards, want, d_out, d_out && out_strides, stripes == 0, &rp);
        if (prc != HEC_OK || rp.rows.empty()) return prc;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, d_out, out_strides, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        const CrcGroupCall call{&rp, stripes, nullptr};
        if (recon_crc_shape(c, cell_len, bytes_per_checksum) && recon_crc_group_aligned(x, call)) {
            const int rc = recon_crc_fused(x, call);
            if (rc != -1) return rc;  // -1: refused, nothing launched
        }
        // the composition: verify the survivors, rebuild, checksum what was rebuilt
        if (d_expected) {
            const int rc = verify_survivors(x, call);
            if (rc != HEC_OK) return rc;
        }
        const int rc = hec_reconstruct_device(c, d_shards, shard_strides, d_out, out_strides, want, cell_len, stripes,
                                              hip_stream);
        if (rc != HEC_OK) return rc;
        return recon_crc_sums_pass(x, call);
    });
}

size_t hec_reconstruct_crc_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return recon_crc_workspace(c->k, c->m, stripes);
}

int hec_reconstruct_crc_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                     const size_t* shard_strides, uint8_t* const* d_out, const size_t* out_strides,
                                     const uint64_t* present, const uint64_t* want, size_t cell_len, size_t stripes,
                                     size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                                     uint8_t* d_sums, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_crc_device_mixed");
    int kind;
    const int chk = recon_crc_check(c, checksum_type, true, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    if (kind < 0)
        return hec_reconstruct_device_mixed(c, d_shards, shard_strides, d_out, out_strides, present, want, cell_len,
                                            stripes, d_workspace, workspace_bytes, hip_stream);
    if (recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK || !d_shards || !shard_strides || !present)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;  // every unit needs storage (present in some stripe)
    return guarded([&]() -> int {
        // 1. the distinct (present, want) pairs with a target, each with its
        // plan and the list of its stripes (host); fail before launching anything
        Batch batch;
        int rc = group_stripes(
            c, present, stripes, kNoPlanId, [&](size_t s, uint64_t mask) { return want ? want[s] : ~mask; },
            [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &batch);
        if (rc != HEC_OK) return rc;
        if (batch.plans.empty()) return HEC_OK;
        if (!d_out || !out_strides || any_null(d_out, batch.target_units)) return HEC_ERR_INVALID_ARG;
        // 2. the lists, flat, behind the plain mixed call's part of the workspace
        const size_t lists_pos = align_up(recon_workspace(c->k, c->m, stripes));
        std::vector<uint32_t> flat;
        std::vector<size_t> off;
        stripe_lists(batch, &flat, &off);
        const size_t lists_bytes = flat.size() * sizeof(uint32_t);
        if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 3u) || workspace_bytes < lists_pos + lists_bytes)
            return HEC_ERR_INVALID_ARG;
        uint8_t* d_lists = static_cast<uint8_t*>(d_workspace) + lists_pos;
        const VerifiedCall x{c, kind, d_shards, shard_strides, d_out, out_strides, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        std::vector<CrcGroupCall> calls(batch.plans.size());
        bool fused = recon_crc_shape(c, cell_len, bytes_per_checksum);
        for (size_t gi = 0; gi < calls.size(); gi++) {
            calls[gi] = CrcGroupCall{&batch.plans[gi], off[gi + 1] - off[gi],
                                     reinterpret_cast<const uint32_t*>(d_lists) + off[gi]};
            fused = fused && recon_crc_group_aligned(x, calls[gi]);
        }
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        rc = upload_pinned(c, lists_bytes, d_lists, x.stream,
                           [&](uint8_t* host) { std::memcpy(host, flat.data(), lists_bytes); });
        if (rc != HEC_OK) return rc;
        // 3. one launch per pair ...
        if (fused) {
            for (const CrcGroupCall& call : calls) {
                rc = recon_crc_fused(x, call);
                if (rc != HEC_OK) return rc == -1 ? HEC_ERR_INVALID_ARG : rc;
            }
            return HEC_OK;
        }
        // ... or the composition: verify per pair, one plain mixed call, sums per pair
        if (d_expected)
            for (const CrcGroupCall& call : calls) {
                rc = verify_survivors(x, call);
                if (rc != HEC_OK) return rc;
            }
        rc = mixed_reconstruct_impl(c, d_shards, shard_strides, d_out, out_strides, present, want, cell_len, stripes,
                                    d_workspace, lists_pos, hip_stream);
        if (rc != HEC_OK) return rc;
        for (const CrcGroupCall& call : calls) {
            rc = recon_crc_sums_pass(x, call);
            if (rc != HEC_OK) return rc;
        }
        return HEC_OK;
    });
}

// ---- checksum-only reconstruction ---------------------------------------------
// hec_reconstruct_sums_device*: the chunk sums of lost units from the
// survivors, nothing rebuilt written (ec_reconstruct_sums.hip).  Read-only
// over the cells; only the targets' live sums words and d_bad are written.

}  // extern "C"

namespace {

// Byte lengths of a group's units in its short last stripe; null = full cells.
struct SumsLens {
    const uint64_t* len = nullptr;  // [k + m]
    size_t stripe0 = 0;             // the stripe the lengths describe (the launch is that one stripe)
};

// The fused launch of one group of full stripes.  0 ok, -1 refused by the
// launcher (nothing launched), else HEC_*.
int recon_sums_fused(const VerifiedCall& x, const CrcGroupCall& g) {
    hec::MatmulArgs a;
    hec::ReconCrcArgs cs;
    recon_fused_args(x, g, &a, &cs);
    return fused_status(hec::launch_reconstruct_sums(a, cs, x.c->device, x.stream));
}

// The generic route of one group: gf_reconstruct_sums_bytes over the group's
// rows, four per launch.  Full cells (lens.len == nullptr): the survivors are
// verified by a checksum launch first.  A short last stripe: that one stripe,
// every unit at its own length, the survivors verified by the same kernel.
int recon_sums_generic(const VerifiedCall& x, const CrcGroupCall& g, const SumsLens& lens) {
    const size_t k = x.k();
    if (x.d_expected && !lens.len) {
        const int rc = verify_survivors(x, g);
        if (rc != HEC_OK) return rc;
    }
    hec::ReconSumsArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_survivors(*g.rp, k, x.shards(), unit_slots(a.in, a.in_stride, a.in_id));
    for (size_t r = 0; r < k; r++) a.in_len[r] = lens.len ? lens.len[a.in_id[r]] : x.cell_len;
    a.k = int32_t(k);
    a.sums = x.d_sums;
    a.n_total = uint32_t(x.n());
    a.kind = x.kind;
    a.stripe_list = g.d_list;
    a.stripe0 = lens.stripe0;
    a.stripes = g.stripes;
    a.bytes_per_checksum = x.bpc;
    a.nck = x.cell_len / x.bpc + (x.cell_len % x.bpc != 0);
    return byte_route_rows(
        g.rp->rows.size(), false,
        [&](size_t j0, size_t rn) {
            std::memset(a.coef, 0, sizeof(a.coef));
            fill_rows(*g.rp, k, j0, rn, a.coef, x.outs(), id_slots(a.out_id));
            for (size_t j = 0; j < rn; j++) a.out_len[j] = lens.len ? lens.len[a.out_id[j]] : x.cell_len;
            a.r = int32_t(rn);
            // a short stripe: the first launch also verifies
            a.expected = lens.len && j0 == 0 ? x.d_expected : nullptr;
            a.bad = lens.len && j0 == 0 ? x.d_bad : nullptr;
        },
        [&] { return hec::launch_reconstruct_sums_bytes(a, x.c->device, x.stream); });
}

// Full stripes of one group: the fused kernel where it takes the shape, else
// the generic route.
int recon_sums_group(const VerifiedCall& x, const CrcGroupCall& g) {
    if (g.stripes == 0) return HEC_OK;
    if (recon_crc_shape(x.c, x.cell_len, x.bpc) && recon_crc_group_aligned(x, g)) {
        const int rc = recon_sums_fused(x, g);
        if (rc != -1) return rc;  // -1: refused, nothing launched
    }
    return recon_sums_generic(x, g, SumsLens{});
}


}  // namespace

extern "C" {

int hec_reconstruct_sums_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                const size_t* shard_strides, const uint8_t* want, size_t cell_len, size_t stripes,
                                size_t bytes_per_checksum, uint64_t data_len, const uint8_t* d_expected,
                                uint8_t* d_bad, uint8_t* d_sums, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_sums_device");
    int kind;
    if (recon_crc_check(c, checksum_type, false, cell_len, bytes_per_checksum, &kind) != HEC_OK ||
        recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK)
        return HEC_ERR_INVALID_ARG;
    hec::crc::Geometry geo;
    if (!d_shards || !shard_strides ||
        !hec::crc::make_geometry(c->k + c->m, c->k, cell_len, stripes, bytes_per_checksum, data_len, &geo))
        return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        const size_t n = c->k + c->m;
        uint64_t mask = 0, want_mask = 0;
        for (size_t i = 0; i < n; i++)
            if (d_shards[i]) mask |= uint64_t(1) << i;
        for (size_t i = 0; want && i < n; i++)
            if (want[i]) want_mask |= uint64_t(1) << i;
        if (want_mask & mask) return HEC_ERR_INVALID_ARG;  // a present unit is not rebuilt
        RowPlan rp;
        rp.plan = plan_of_mask(c, mask);
        if (stripes != 0) rp.rows = target_rows(*rp.plan, want != nullptr, want_mask);
        if (rp.rows.empty()) return HEC_OK;
        if (rp.plan->rec_status != HEC_OK) return rp.plan->rec_status;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        // only the last stripe can be short: the others as one group of full cells
        const bool short_last = geo.last_len < uint64_t(c->k) * cell_len;
        const int rc = recon_sums_group(x, CrcGroupCall{&rp, short_last ? stripes - 1 : stripes, nullptr});
        if (rc != HEC_OK || !short_last) return rc;
        return recon_sums_generic(x, CrcGroupCall{&rp, 1, nullptr}, SumsLens{geo.len_last, stripes - 1});
    });
}

int hec_reconstruct_sums_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                      const size_t* shard_strides, const uint64_t* present, const uint64_t* want,
                                      size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                      const uint8_t* d_expected, uint8_t* d_bad, uint8_t* d_sums, void* d_workspace,
                                      size_t workspace_bytes, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_sums_device_mixed");
    int kind;
    if (recon_crc_check(c, checksum_type, false, cell_len, bytes_per_checksum, &kind) != HEC_OK ||
        recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK)
        return HEC_ERR_INVALID_ARG;
    if (!d_shards || !shard_strides || !present) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    // a unit without storage (the dead node's) is present in no stripe
    uint64_t ever_present = 0;
    for (size_t s = 0; s < stripes; s++) ever_present |= present[s];
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i] && ((ever_present >> i) & 1)) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        // the distinct (present, want) pairs with a target, each with its plan
        // and the list of its stripes (host); fail before launching anything
        Batch batch;
        int rc = group_stripes(
            c, present, stripes, kNoPlanId, [&](size_t s, uint64_t mask) { return want ? want[s] : ~mask; },
            [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &batch);
        if (rc != HEC_OK) return rc;
        if (batch.plans.empty()) return HEC_OK;
        // the lists where hec_reconstruct_crc_device_mixed keeps them: one
        // workspace, one size function, one rule for both calls
        const size_t lists_pos = align_up(recon_workspace(c->k, c->m, stripes));
        std::vector<uint32_t> flat;
        std::vector<size_t> off;
        stripe_lists(batch, &flat, &off);
        const size_t lists_bytes = flat.size() * sizeof(uint32_t);
        if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 3u) || workspace_bytes < lists_pos + lists_bytes)
            return HEC_ERR_INVALID_ARG;
        uint8_t* d_lists = static_cast<uint8_t*>(d_workspace) + lists_pos;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        rc = upload_pinned(c, lists_bytes, d_lists, x.stream,
                           [&](uint8_t* host) { std::memcpy(host, flat.data(), lists_bytes); });
        if (rc != HEC_OK) return rc;
        // one launch per pair (more where a pair has over four rows or runs the generic route)
        for (size_t gi = 0; gi < batch.plans.size(); gi++) {
            const CrcGroupCall call{&batch.plans[gi], off[gi + 1] - off[gi],
                                    reinterpret_cast<const uint32_t*>(d_lists) + off[gi]};
            rc = recon_sums_group(x, call);
            if (rc != HEC_OK) return rc;
        }
        return HEC_OK;
    });
}

// ---- verified reconstruction of short stripes ---------------------------------
// hec_reconstruct_crc_rows_device*: hec_reconstruct_crc_device* for stripes
// that hold fewer than k * cell_len logical bytes (ec_reconstruct_rows.hip).
// Full stripes go through the launches of hec_reconstruct_crc_device*.

}  // extern "C"

namespace {

// What needs no device and no buffer: the coder, the checksum (HEC_CHECKSUM_NULL
// has no call of this kind) and the sizes.
int recon_rows_check(const hec_coder* c, int checksum_type, size_t cell_len, size_t bpc, int* kind) {
    if (!c || cell_len == 0 || bpc == 0) return HEC_ERR_INVALID_ARG;
    *kind = crc_kind(checksum_type);
    if (*kind < 0 || cell_len > UINT64_MAX / c->k) return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// The short stripes of one group (g.stripes of them, g.d_list or lens.stripe0
// on): gf_reconstruct_crc_rows where `fused` and the launcher takes it, else
// gf_reconstruct_rows_bytes over the group's rows, four per launch, the first
// launch verifying the survivors.
int recon_rows_short(const VerifiedCall& x, const CrcGroupCall& g, const hec::ReconRowsLens& lens, bool fused) {
    if (g.stripes == 0) return HEC_OK;
    const size_t k = x.k();
    if (fused) {
        hec::MatmulArgs a;
        hec::ReconCrcArgs cs;
        recon_fused_args(x, g, &a, &cs);
        const int rc = fused_status(hec::launch_reconstruct_crc_rows(a, cs, lens, x.c->device, x.stream));
        if (rc != -1) return rc;  // -1: refused, nothing launched
    }
    hec::ReconRowsBytesArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_survivors(*g.rp, k, x.shards(), unit_slots(a.in, a.in_stride, a.in_id));
    a.k = int32_t(k);
    a.data_units = uint32_t(k);
    a.n_total = uint32_t(x.n());
    a.sums = x.d_sums;
    a.expected = x.d_expected;
    a.bad = x.d_bad;
    a.kind = x.kind;
    a.stripe_list = g.d_list;
    a.stripes = g.stripes;
    a.lens = lens;
    a.cell_len = x.cell_len;
    a.bytes_per_checksum = x.bpc;
    return byte_route_rows(
        g.rp->rows.size(), false,
        [&](size_t j0, size_t rn) {
            std::memset(a.coef, 0, sizeof(a.coef));
            fill_rows(*g.rp, k, j0, rn, a.coef, x.outs(), unit_slots(a.out, a.out_stride, a.out_id));
            a.r = int32_t(rn);
            if (j0 != 0) {  // the survivors are verified once
                a.expected = nullptr;
                a.bad = nullptr;
            }
        },
        [&] { return hec::launch_reconstruct_rows_bytes(a, x.c->device, x.stream); });
}


}  // namespace

extern "C" {

int hec_reconstruct_crc_rows_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                    const size_t* shard_strides, uint8_t* const* d_out, const size_t* out_strides,
                                    const uint8_t* want, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                    uint64_t data_len, const uint8_t* d_expected, uint8_t* d_bad, uint8_t* d_sums,
                                    void* hip_stream) {
    int kind;
    const int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    hec::crc::Geometry geo;
    if (!hec::crc::make_geometry(c->k + c->m, c->k, cell_len, stripes, bytes_per_checksum, data_len, &geo))
        return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_crc_rows_device");
    if (recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK) return HEC_ERR_INVALID_ARG;
    // every stripe full: the existing call, launch for launch
    if (stripes == 0 || geo.last_len == uint64_t(c->k) * cell_len)
        return hec_reconstruct_crc_device(c, checksum_type, d_shards, shard_strides, d_out, out_strides, want, cell_len,
                                          stripes, bytes_per_checksum, d_expected, d_bad, d_sums, hip_stream);
    if (!d_shards || !shard_strides || stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        RowPlan rp;
        const int prc = resolve_reconstruct(c, d_shards, want, d_out, d_out && out_strides, false, &rp);
        if (prc != HEC_OK || rp.rows.empty()) return prc;
        // one launch over the stripes - 1 full stripes, one over the last
        if (stripes > 1) {
            const int rc = hec_reconstruct_crc_device(c, checksum_type, d_shards, shard_strides, d_out, out_strides,
                                                      want, cell_len, stripes - 1, bytes_per_checksum, d_expected,
                                                      d_bad, d_sums, hip_stream);
            if (rc != HEC_OK) return rc;
        }
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, d_out, out_strides, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        const CrcGroupCall last{&rp, 1, nullptr};
        const bool fused = recon_crc_shape(c, cell_len, bytes_per_checksum) && recon_crc_group_aligned(x, last);
        return recon_rows_short(x, last, hec::ReconRowsLens{nullptr, geo.last_len, stripes - 1}, fused);
    });
}

size_t hec_reconstruct_crc_rows_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return recon_rows_workspace(c->k, c->m, stripes);
}

int hec_reconstruct_crc_rows_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                          const size_t* shard_strides, uint8_t* const* d_out,
                                          const size_t* out_strides, const uint64_t* present, const uint64_t* want,
                                          const uint64_t* stripe_bytes, size_t cell_len, size_t stripes,
                                          size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                                          uint8_t* d_sums, void* d_workspace, size_t workspace_bytes,
                                          void* hip_stream) {
    int kind;
    const int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    for (size_t s = 0; stripe_bytes && s < stripes; s++)
        if (stripe_bytes[s] > uint64_t(c->k) * cell_len) return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_reconstruct_crc_rows_device_mixed");
    if (recon_sums_buffers_check(d_expected, d_bad, d_sums) != HEC_OK) return HEC_ERR_INVALID_ARG;
    if (!d_shards || !shard_strides || !present) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;  // every unit needs storage (present in some stripe)
    return guarded([&]() -> int {
        // 1. the distinct (present, want) pairs with a target and their plans
        // (host); fail before anything is queued
        Batch batch;
        int rc = group_stripes(
            c, present, stripes, kNoPlanId, [&](size_t s, uint64_t mask) { return want ? want[s] : ~mask; },
            [&](uint64_t mask, uint64_t wmask, RowPlan* rp) { return reconstruct_rows(c, mask, wmask, rp); }, &batch);
        if (rc != HEC_OK) return rc;
        if (batch.plans.empty()) return HEC_OK;
        if (!d_out || !out_strides || any_null(d_out, batch.target_units)) return HEC_ERR_INVALID_ARG;
        // 2. every pair's full stripes and short stripes, the short ones' bytes
        RowsLists lists;
        rows_lists(batch, stripe_bytes, c->k, cell_len, &lists);
        const RowsLayout w = rows_layout(c->k, c->m, stripes, lists.full.size(), lists.shrt.size());
        if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 7u) || workspace_bytes < w.need)
            return HEC_ERR_INVALID_ARG;
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        const uint32_t* d_full = reinterpret_cast<const uint32_t*>(ws + w.full_pos);
        const uint32_t* d_short = reinterpret_cast<const uint32_t*>(ws + w.short_pos);
        const uint64_t* d_bytes = reinterpret_cast<const uint64_t*>(ws + w.bytes_pos);
        const size_t plans = batch.plans.size();
        const VerifiedCall x{c, kind, d_shards, shard_strides, d_out, out_strides, cell_len, bytes_per_checksum,
                             d_expected, d_bad, d_sums, static_cast<hipStream_t>(hip_stream)};
        std::vector<CrcGroupCall> full(plans), shrt(plans);
        bool fused = recon_crc_shape(c, cell_len, bytes_per_checksum);
        for (size_t gi = 0; gi < plans; gi++) {
            full[gi] = CrcGroupCall{&batch.plans[gi], lists.full_off[gi + 1] - lists.full_off[gi],
                                    d_full + lists.full_off[gi]};
            shrt[gi] = CrcGroupCall{&batch.plans[gi], lists.short_off[gi + 1] - lists.short_off[gi],
                                    d_short + lists.short_off[gi]};
            fused = fused && recon_crc_group_aligned(x, full[gi]);
        }
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        rc = upload_pinned(c, w.image_bytes, ws + w.full_pos, x.stream,
                           [&](uint8_t* host) { write_rows_image(host, lists, w); });
        if (rc != HEC_OK) return rc;
        // 3. the full stripes as hec_reconstruct_crc_device_mixed runs them:
        // one fused launch per pair ...
        if (fused) {
            for (const CrcGroupCall& call : full) {
                if (call.stripes == 0) continue;
                rc = recon_crc_fused(x, call);
                if (rc != HEC_OK) return rc == -1 ? HEC_ERR_INVALID_ARG : rc;
            }
        } else if (!lists.full.empty()) {
            // ... or the composition: verify per pair, one plain mixed call
            // (the short stripes with nothing wanted), sums per pair
            if (d_expected)
                for (const CrcGroupCall& call : full) {
                    if (call.stripes == 0) continue;
                    rc = verify_survivors(x, call);
                    if (rc != HEC_OK) return rc;
                }
            std::vector<uint64_t> want_full;
            if (!lists.shrt.empty()) {
                want_full.resize(stripes);
                for (size_t s = 0; s < stripes; s++)
                    want_full[s] = rows_short(stripe_bytes[s], c->k, cell_len) ? 0 : (want ? want[s] : ~present[s]);
            }
            rc = mixed_reconstruct_impl(c, d_shards, shard_strides, d_out, out_strides, present,
                                        want_full.empty() ? want : want_full.data(), cell_len, stripes, d_workspace,
                                        w.full_pos, hip_stream);
            if (rc != HEC_OK) return rc;
            for (const CrcGroupCall& call : full) {
                if (call.stripes == 0) continue;
                rc = recon_crc_sums_pass(x, call);
                if (rc != HEC_OK) return rc;
            }
        }
        // 4. one launch per pair over its short stripes
        for (size_t gi = 0; gi < plans; gi++) {
            rc = recon_rows_short(x, shrt[gi], hec::ReconRowsLens{d_bytes + lists.short_off[gi], 0, 0}, fused);
            if (rc != HEC_OK) return rc;
        }
        return HEC_OK;
    });
}

// ---- verified scrub: parity check and chunk checksums in one pass -------------
// hec_scrub_crc_device*: the scrub calls with the chunk sums of every present
// unit verified in the same pass (ec_scrub_crc.hip), or as a composition of
// internal launches where the fused kernel does not take the shape.

}  // extern "C"

namespace {

// [hec_scrub_device_mixed's workspace][stripe lists: u32 x stripes]
size_t scrub_crc_workspace(size_t k, size_t m, size_t stripes) {
    return align_up(scrub_workspace(k, m, stripes)) + align_up(stripes * sizeof(uint32_t));
}

// What both entry points check the same way, in two halves (every failure is
// HEC_ERR_INVALID_ARG): the units' storage and the results array ...
int scrub_crc_buffers_check(const hec_coder* c, const uint8_t* const* d_shards, const size_t* shard_strides,
                            size_t stripes, const hec_scrub_result_t* d_results) {
    if (!c || !d_shards || !shard_strides || !d_results || (reinterpret_cast<uintptr_t>(d_results) & 7u) != 0 ||
        stripes > SIZE_MAX / sizeof(hec_scrub_result_t))
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k + c->m; i++)
        if (!d_shards[i]) return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// ... and the sizes and the checksum; kind < 0 = HEC_CHECKSUM_NULL.
int scrub_crc_sums_check(int checksum_type, size_t cell_len, size_t bpc, const uint8_t* d_expected,
                         const uint8_t* d_bad, int* kind) {
    if (cell_len == 0 || bpc == 0) return HEC_ERR_INVALID_ARG;
    *kind = -1;
    if (checksum_type == HEC_CHECKSUM_NULL) return HEC_OK;
    *kind = crc_kind(checksum_type);
    if (*kind < 0 || !d_expected || !d_bad || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
        return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// The shapes gf_scrub_crc takes (launch_scrub_crc checks the same): k, 512-B
// chunks, 16-B aligned cells, tile indices in 32 bits (counted in its smaller
// block tile, 16 KiB).  The extras and row 0 of every plan are checked per plan.
bool scrub_crc_shape(const VerifiedCall& x, size_t stripes) {
    if (!register_kernel_k(x.k()) || x.bpc != 512 || x.cell_len % 16 != 0 || x.cell_len / 16 > 0xFFFFFFFFull ||
        stripes > 0xFFFFFFFFull)
        return false;
    const uint64_t tiles = (uint64_t(x.cell_len) + 16383) / 16384;
    if (tiles > 0xFFFFFFFFull / stripes) return false;
    return aligned16(x.d_shards, x.shard_strides, unit_bits(x.n()));
}

// At most kMaxR extras and no zero in row 0 of G (the minors divide by it).
bool scrub_crc_plan_fits(const hec_coder* c, const RowPlan& sp) {
    if (sp.rows.empty() || sp.rows.size() > size_t(hec::kMaxR)) return false;
    const uint8_t* row0 = &sp.plan->rec_matrix[sp.rows[0] * c->k];
    bool pivots = true;
    for (size_t i = 0; i < c->k; i++) pivots &= row0[i] != 0;
    return pivots;
}

// The fused launch of one group; with `lens`, of its short stripes
// (gf_scrub_crc_rows).  0 ok, -1 refused by the launcher, else HEC_*.
int scrub_crc_fused(const VerifiedCall& x, const CrcGroupCall& g, hec_scrub_result_t* d_results,
                    const hec::ReconRowsLens* lens = nullptr) {
    const size_t k = x.k(), r = g.rp->rows.size();
    hec::MatmulArgs a;
    std::memset(&a, 0, sizeof(a));
    hec::ScrubCrcArgs cs;
    std::memset(&cs, 0, sizeof(cs));
    fill_survivors(*g.rp, k, x.shards(), unit_slots(a.in, a.in_stride, cs.shard_id));
    fill_rows(*g.rp, k, 0, r, a.coef, x.shards(), unit_slots(a.in + k, a.in_stride + k, cs.shard_id + k));
    a.k = int32_t(k);
    a.r = int32_t(r);
    a.cell_len = x.cell_len;
    a.stripes = g.stripes;
    cs.expected = x.d_expected;
    cs.bad = x.d_bad;
    cs.results = reinterpret_cast<uint64_t*>(d_results);
    cs.missing = g.rp->missing;
    cs.n_total = uint32_t(x.n());
    cs.kind = x.kind;
    cs.stripe_list = g.d_list;
    return fused_status(lens ? hec::launch_scrub_crc_rows(a, cs, *lens, x.c->device, x.stream)
                             : hec::launch_scrub_crc(a, cs, x.c->device, x.stream));
}

// The present units of a group verified against their sums: the composition's
// first step, and all there is to do for a group with e == 0.
int scrub_crc_verify(const VerifiedCall& x, const CrcGroupCall& g) {
    uint8_t units[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    UnitList l;
    l.cnt = mask_units(g.mask & unit_bits(x.n()), units);
    if (l.cnt == 0) return HEC_OK;
    fill_units(units, l.cnt, x.shards(), l.slots());
    return sums_launch(x, g, true, l);
}


}  // namespace

extern "C" {

int hec_scrub_crc_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                         const size_t* shard_strides, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                         const uint8_t* d_expected, uint8_t* d_bad, hec_scrub_result_t* d_results, void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_crc_device");
    int kind;
    if (scrub_crc_buffers_check(c, d_shards, shard_strides, stripes, d_results) != HEC_OK ||
        scrub_crc_sums_check(checksum_type, cell_len, bytes_per_checksum, d_expected, d_bad, &kind) != HEC_OK)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (kind < 0) return hec_scrub_device(c, d_shards, shard_strides, cell_len, stripes, d_results, hip_stream);
    return guarded([&]() -> int {
        // every unit present: S = the data units, E = the parity units, G = P
        const uint64_t all = unit_bits(c->k + c->m);
        RowPlan sp;
        const int prc = scrub_rows(c, all, &sp);
        if (prc != HEC_OK) return prc;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        const CrcGroupCall call{&sp, stripes, nullptr, all};
        if (scrub_crc_plan_fits(c, sp) && scrub_crc_shape(x, stripes)) {
            // the kernel only ORs and adds into the words: zeroed here, in
            // stream order (a zeroing kernel node under capture)
            HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), x.stream), HEC_ERR_DEVICE);
            const int rc = scrub_crc_fused(x, call, d_results);
            if (rc != -1) return rc;  // -1: refused, no kernel launched
        }
        // the composition: verify every unit, then the plain scrub (which zeroes the results)
        const int rc = scrub_crc_verify(x, call);
        if (rc != HEC_OK) return rc;
        return hec_scrub_device(c, d_shards, shard_strides, cell_len, stripes, d_results, hip_stream);
    });
}

size_t hec_scrub_crc_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return scrub_crc_workspace(c->k, c->m, stripes);
}

int hec_scrub_crc_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                               const size_t* shard_strides, const uint64_t* present, size_t cell_len, size_t stripes,
                               size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                               hec_scrub_result_t* d_results, void* d_workspace, size_t workspace_bytes,
                               void* hip_stream) {
    if (c && c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_crc_device_mixed");
    int kind;
    if (scrub_crc_buffers_check(c, d_shards, shard_strides, stripes, d_results) != HEC_OK ||
        scrub_crc_sums_check(checksum_type, cell_len, bytes_per_checksum, d_expected, d_bad, &kind) != HEC_OK ||
        !present)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    if (kind < 0)
        return hec_scrub_device_mixed(c, d_shards, shard_strides, present, cell_len, stripes, d_results, d_workspace,
                                      workspace_bytes, hip_stream);
    return guarded([&]() -> int {
        const size_t k = c->k, m = c->m;
        const uint64_t all = unit_bits(k + m);
        // 1. plan per distinct mask with an extra (host), and the masks
        // without one that still have a unit to verify; fail before anything
        // is queued
        Batch batch;
        bool fits = true;  // every plan within the fused kernel's rows and pivots
        int rc = group_stripes(
            c, present, stripes, kNoPlanId, [](size_t, uint64_t) { return uint64_t(0); },
            [&](uint64_t mask, uint64_t, RowPlan* sp) {
                const int src = scrub_rows(c, mask, sp);
                if (src != HEC_OK || sp->rows.empty()) return src;
                fits = fits && scrub_crc_plan_fits(c, *sp);
                return int(HEC_OK);
            },
            &batch);
        if (rc != HEC_OK) return rc;
        std::map<uint64_t, std::vector<uint32_t>> bare;  // e == 0: mask -> its stripes, ascending
        for (size_t s = 0; s < stripes; s++)
            if (batch.stripe_plan[s] == kNoPlanId && (present[s] & all)) bare[present[s] & all].push_back(uint32_t(s));
        const bool idle = batch.plans.empty() && bare.empty();  // no stripe has a unit
        const size_t lists_pos = align_up(scrub_workspace(k, m, stripes));
        if (!idle && (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 15u) != 0 ||
                      workspace_bytes < scrub_crc_workspace(k, m, stripes)))
            return HEC_ERR_INVALID_ARG;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        const bool fused = fits && scrub_crc_shape(x, stripes);
        if (idle || fused)  // the composition's scrub call zeroes them itself
            HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), x.stream), HEC_ERR_DEVICE);
        if (idle) return HEC_OK;
        // 2. the lists, flat -- the plans' and then the bare masks' -- behind
        // the plain mixed call's part of the workspace
        std::vector<uint32_t> flat;
        std::vector<size_t> off;
        stripe_lists(batch, &flat, &off);
        for (const auto& b : bare) {
            flat.insert(flat.end(), b.second.begin(), b.second.end());
            off.push_back(flat.size());
        }
        const size_t lists_bytes = flat.size() * sizeof(uint32_t);
        uint8_t* d_lists = static_cast<uint8_t*>(d_workspace) + lists_pos;
        rc = upload_pinned(c, lists_bytes, d_lists, x.stream,
                           [&](uint8_t* host) { std::memcpy(host, flat.data(), lists_bytes); });
        if (rc != HEC_OK) return rc;
        std::vector<CrcGroupCall> groups;
        for (size_t gi = 0; gi < batch.plans.size(); gi++)
            groups.push_back(CrcGroupCall{&batch.plans[gi], off[gi + 1] - off[gi],
                                          reinterpret_cast<const uint32_t*>(d_lists) + off[gi],
                                          all & ~batch.plans[gi].missing});
        size_t gi = batch.plans.size();
        for (const auto& b : bare) {
            groups.push_back(CrcGroupCall{nullptr, off[gi + 1] - off[gi],
                                          reinterpret_cast<const uint32_t*>(d_lists) + off[gi], b.first});
            gi++;
        }
        // 3. one launch per mask: the fused kernel, or sums only where e == 0 ...
        if (fused) {
            for (const CrcGroupCall& grp : groups) {
                rc = grp.rp ? scrub_crc_fused(x, grp, d_results) : scrub_crc_verify(x, grp);
                if (rc != HEC_OK) return rc == -1 ? HEC_ERR_INVALID_ARG : rc;
            }
            return HEC_OK;
        }
        // ... or the composition: verify per mask, then the plain mixed scrub
        for (const CrcGroupCall& grp : groups) {
            rc = scrub_crc_verify(x, grp);
            if (rc != HEC_OK) return rc;
        }
        return hec_scrub_device_mixed(c, d_shards, shard_strides, present, cell_len, stripes, d_results, d_workspace,
                                      lists_pos, hip_stream);
    });
}

// ---- verified scrub of short stripes ------------------------------------------
// hec_scrub_crc_rows_device*: hec_scrub_crc_device* with the lengths of
// hec_reconstruct_crc_rows_device* -- a stripe of r < k * cell_len logical
// bytes is checked over its positions below n0 and every present unit is
// verified over its own bytes (ec_scrub_rows.hip).  Full stripes run as the
// existing calls run them, launch for launch.

}  // extern "C"

namespace {

// hec_scrub_crc_device_mixed's groups as one Batch, so that rows_lists splits
// every group's stripes into full and short: a plan per distinct mask with an
// extra, in the order the masks first appear, then an entry without rows (sums
// only; `missing` = the units the mask lacks) per distinct mask without an
// extra that still has a unit.  *fits: every check plan is within the fused
// kernel's rows and pivots.  Host only, nothing queued.
int scrub_rows_groups(hec_coder* c, const uint64_t* present, size_t stripes, Batch* b, bool* fits) {
    const uint64_t all = unit_bits(c->k + c->m);
    *fits = true;
    const int rc = group_stripes(
        c, present, stripes, kNoPlanId, [](size_t, uint64_t) { return uint64_t(0); },
        [&](uint64_t mask, uint64_t, RowPlan* sp) {
            const int src = scrub_rows(c, mask, sp);
            if (src != HEC_OK || sp->rows.empty()) return src;
            *fits = *fits && scrub_crc_plan_fits(c, *sp);
            return int(HEC_OK);
        },
        b);
    if (rc != HEC_OK) return rc;
    std::map<uint64_t, uint32_t> bare;  // e == 0: mask -> its entry
    for (size_t s = 0; s < stripes; s++) {
        const uint64_t mask = present[s] & all;
        if (b->stripe_plan[s] != kNoPlanId || !mask) continue;
        auto it = bare.find(mask);
        if (it == bare.end()) {
            RowPlan rp;
            rp.missing = ~mask & all;
            it = bare.emplace(mask, uint32_t(b->plans.size())).first;
            b->plans.push_back(std::move(rp));
        }
        b->stripe_plan[s] = it->second;
    }
    return HEC_OK;
}

// rows_layout behind hec_scrub_crc_device_mixed's workspace: the full
// stripes' lists where that call keeps its lists, then, behind its whole
// workspace, [short lists: u32][pad to kAlign][their bytes: u64].
RowsLayout scrub_rows_layout(size_t k, size_t m, size_t stripes, size_t n_full, size_t n_short) {
    RowsLayout w;
    w.full_pos = align_up(scrub_workspace(k, m, stripes));
    w.short_pos = align_up(scrub_crc_workspace(k, m, stripes));
    w.bytes_pos = w.short_pos + align_up(n_short * sizeof(uint32_t));
    w.need = n_short ? w.bytes_pos + n_short * sizeof(uint64_t) : w.full_pos + n_full * sizeof(uint32_t);
    w.image_bytes = w.need - w.full_pos;
    return w;
}

// The worst batch of `stripes`: every stripe short.
size_t scrub_rows_workspace(size_t k, size_t m, size_t stripes) {
    return scrub_rows_layout(k, m, stripes, 0, stripes).bytes_pos + stripes * sizeof(uint64_t);
}

// The shapes gf_scrub_crc_rows takes: gf_scrub_crc's, with lengths in 32 bits.
bool scrub_rows_shape(const VerifiedCall& x, size_t stripes) {
    return x.cell_len <= 0x7FFFFFFFull && scrub_crc_shape(x, stripes);
}

// The short stripes of one group (g.stripes of them, g.d_list or lens.stripe0
// on): gf_scrub_crc_rows where `fused`, the group has a check plan and the
// launcher takes it, else gf_scrub_rows_bytes (also all there is for a group
// with e == 0: the units' sums over their own bytes).
int scrub_rows_short(const VerifiedCall& x, const CrcGroupCall& g, const hec::ReconRowsLens& lens, bool fused,
                     hec_scrub_result_t* d_results) {
    if (g.stripes == 0) return HEC_OK;
    const size_t k = x.k();
    if (fused && g.rp) {
        const int rc = scrub_crc_fused(x, g, d_results, &lens);
        if (rc != -1) return rc;  // -1: refused, nothing launched
    }
    hec::ScrubRowsBytesArgs a;
    std::memset(&a, 0, sizeof(a));
    if (g.rp) {
        const size_t e = g.rp->rows.size();
        if (e > size_t(hec::kScrubRowsMaxE)) return HEC_ERR_INVALID_ARG;
        fill_survivors(*g.rp, k, x.shards(), unit_slots(a.in, a.in_stride, a.id));
        fill_rows(*g.rp, k, 0, e, a.coef, x.shards(), unit_slots(a.in + k, a.in_stride + k, a.id + k));
        a.ns = int32_t(k);
        a.e = int32_t(e);
        a.missing = g.rp->missing;
    } else {
        uint8_t units[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
        const size_t cnt = mask_units(g.mask & unit_bits(x.n()), units);
        if (cnt == 0) return HEC_OK;
        fill_units(units, cnt, x.shards(), unit_slots(a.in, a.in_stride, a.id));
        a.ns = int32_t(cnt);
    }
    a.data_units = uint32_t(k);
    a.n_total = uint32_t(x.n());
    a.expected = x.d_expected;
    a.bad = x.d_bad;
    a.results = reinterpret_cast<uint64_t*>(d_results);
    a.kind = x.kind;
    a.stripe_list = g.d_list;
    a.stripes = g.stripes;
    a.lens = lens;
    a.cell_len = x.cell_len;
    a.bytes_per_checksum = x.bpc;
    const int rc = hec::launch_scrub_rows_bytes(a, x.c->device, x.stream);
    if (rc != 0) return rc < 0 ? HEC_ERR_INVALID_ARG : to_status(rc);
    return HEC_OK;
}


}  // namespace

extern "C" {

int hec_scrub_crc_rows_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                              const size_t* shard_strides, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                              uint64_t data_len, const uint8_t* d_expected, uint8_t* d_bad,
                              hec_scrub_result_t* d_results, void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    hec::crc::Geometry geo;
    if (!hec::crc::make_geometry(c->k + c->m, c->k, cell_len, stripes, bytes_per_checksum, data_len, &geo))
        return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_crc_rows_device");
    if (scrub_crc_buffers_check(c, d_shards, shard_strides, stripes, d_results) != HEC_OK ||
        scrub_crc_sums_check(checksum_type, cell_len, bytes_per_checksum, d_expected, d_bad, &kind) != HEC_OK)
        return HEC_ERR_INVALID_ARG;
    // every stripe full: the existing call, launch for launch
    if (stripes == 0 || geo.last_len == uint64_t(c->k) * cell_len)
        return hec_scrub_crc_device(c, checksum_type, d_shards, shard_strides, cell_len, stripes, bytes_per_checksum,
                                    d_expected, d_bad, d_results, hip_stream);
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        const uint64_t all = unit_bits(c->k + c->m);
        RowPlan sp;
        const int prc = scrub_rows(c, all, &sp);
        if (prc != HEC_OK) return prc;
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        const RowPlan* plan = sp.rows.empty() ? nullptr : &sp;
        bool fused = plan && scrub_crc_plan_fits(c, sp) && scrub_rows_shape(x, stripes);
        // one launch over the stripes - 1 full stripes, one over the last;
        // the results are zeroed once, in stream order (a zeroing kernel node
        // under capture)
        if (fused) {
            HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), x.stream), HEC_ERR_DEVICE);
            if (stripes > 1) {
                const int rc = scrub_crc_fused(x, CrcGroupCall{plan, stripes - 1, nullptr, all}, d_results);
                if (rc == -1) fused = false;  // refused, no kernel launched
                else if (rc != HEC_OK) return rc;
            }
        }
        if (!fused) {
            // the composition zeroes its own stripes' results
            if (stripes > 1) {
                const int rc = hec_scrub_crc_device(c, checksum_type, d_shards, shard_strides, cell_len, stripes - 1,
                                                    bytes_per_checksum, d_expected, d_bad, d_results, hip_stream);
                if (rc != HEC_OK) return rc;
            }
            HEC_HIP(hec::zero_async(d_results + (stripes - 1), sizeof(hec_scrub_result_t), x.stream), HEC_ERR_DEVICE);
        }
        return scrub_rows_short(x, CrcGroupCall{plan, 1, nullptr, all},
                                hec::ReconRowsLens{nullptr, geo.last_len, stripes - 1}, fused, d_results);
    });
}

size_t hec_scrub_crc_rows_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return scrub_rows_workspace(c->k, c->m, stripes);
}

int hec_scrub_crc_rows_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                    const size_t* shard_strides, const uint64_t* present,
                                    const uint64_t* stripe_bytes, size_t cell_len, size_t stripes,
                                    size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                                    hec_scrub_result_t* d_results, void* d_workspace, size_t workspace_bytes,
                                    void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    bool any_short = false;
    for (size_t s = 0; stripe_bytes && s < stripes; s++) {
        if (stripe_bytes[s] > uint64_t(c->k) * cell_len) return HEC_ERR_INVALID_ARG;
        any_short = any_short || rows_short(stripe_bytes[s], c->k, cell_len);
    }
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_scrub_crc_rows_device_mixed");
    if (scrub_crc_buffers_check(c, d_shards, shard_strides, stripes, d_results) != HEC_OK ||
        scrub_crc_sums_check(checksum_type, cell_len, bytes_per_checksum, d_expected, d_bad, &kind) != HEC_OK ||
        !present)
        return HEC_ERR_INVALID_ARG;
    // every stripe full: the existing call, launch for launch
    if (stripes == 0 || !any_short)
        return hec_scrub_crc_device_mixed(c, checksum_type, d_shards, shard_strides, present, cell_len, stripes,
                                          bytes_per_checksum, d_expected, d_bad, d_results, d_workspace,
                                          workspace_bytes, hip_stream);
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        const size_t k = c->k, m = c->m;
        const uint64_t all = unit_bits(k + m);
        // 1. the groups and their plans (host); fail before anything is queued
        Batch batch;
        bool fits = true;
        int rc = scrub_rows_groups(c, present, stripes, &batch, &fits);
        if (rc != HEC_OK) return rc;
        const bool idle = batch.plans.empty();  // no stripe has a unit
        if (!idle && (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 15u) != 0 ||
                      workspace_bytes < scrub_rows_workspace(k, m, stripes)))
            return HEC_ERR_INVALID_ARG;
        // 2. every group's full stripes and short stripes, the short ones' bytes
        RowsLists lists;
        rows_lists(batch, stripe_bytes, k, cell_len, &lists);
        const RowsLayout w = scrub_rows_layout(k, m, stripes, lists.full.size(), lists.shrt.size());
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        const bool fused = fits && scrub_rows_shape(x, stripes);
        const bool composed = !fused && !lists.full.empty();  // the plain mixed scrub zeroes the results itself
        if (!composed)
            HEC_HIP(hec::zero_async(d_results, stripes * sizeof(hec_scrub_result_t), x.stream), HEC_ERR_DEVICE);
        if (idle) return HEC_OK;
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        rc = upload_pinned(c, w.image_bytes, ws + w.full_pos, x.stream,
                           [&](uint8_t* host) { write_rows_image(host, lists, w); });
        if (rc != HEC_OK) return rc;
        const uint32_t* d_full = reinterpret_cast<const uint32_t*>(ws + w.full_pos);
        const uint32_t* d_short = reinterpret_cast<const uint32_t*>(ws + w.short_pos);
        const uint64_t* d_bytes = reinterpret_cast<const uint64_t*>(ws + w.bytes_pos);
        const size_t groups = batch.plans.size();
        std::vector<CrcGroupCall> full(groups), shrt(groups);
        for (size_t gi = 0; gi < groups; gi++) {
            const RowPlan* sp = batch.plans[gi].rows.empty() ? nullptr : &batch.plans[gi];
            const uint64_t mask = all & ~batch.plans[gi].missing;
            full[gi] = CrcGroupCall{sp, lists.full_off[gi + 1] - lists.full_off[gi], d_full + lists.full_off[gi], mask};
            shrt[gi] =
                CrcGroupCall{sp, lists.short_off[gi + 1] - lists.short_off[gi], d_short + lists.short_off[gi], mask};
        }
        // 3. the full stripes as hec_scrub_crc_device_mixed runs them: one
        // launch per mask, the fused kernel or sums only where e == 0 ...
        if (fused) {
            for (const CrcGroupCall& grp : full) {
                if (grp.stripes == 0) continue;
                rc = grp.rp ? scrub_crc_fused(x, grp, d_results) : scrub_crc_verify(x, grp);
                if (rc != HEC_OK) return rc == -1 ? HEC_ERR_INVALID_ARG : rc;
            }
        } else if (composed) {
            // ... or the composition: verify per mask, then the plain mixed
            // scrub with the short stripes masked out (no unit: unchecked)
            for (const CrcGroupCall& grp : full) {
                if (grp.stripes == 0) continue;
                rc = scrub_crc_verify(x, grp);
                if (rc != HEC_OK) return rc;
            }
            std::vector<uint64_t> present_full(stripes);
            for (size_t s = 0; s < stripes; s++)
                present_full[s] = rows_short(stripe_bytes[s], k, cell_len) ? 0 : present[s];
            rc = hec_scrub_device_mixed(c, d_shards, shard_strides, present_full.data(), cell_len, stripes, d_results,
                                        d_workspace, w.full_pos, hip_stream);
            if (rc != HEC_OK) return rc;
        }
        // 4. one launch per mask over its short stripes
        for (size_t gi = 0; gi < groups; gi++) {
            rc = scrub_rows_short(x, shrt[gi], hec::ReconRowsLens{d_bytes + lists.short_off[gi], 0, 0}, fused,
                                  d_results);
            if (rc != HEC_OK) return rc;
        }
        return HEC_OK;
    });
}

// ---- encode with chunk sums of short stripes ----------------------------------
// hec_encode_crc_rows_device*: hec_encode_crc_device with a checksum type and
// the lengths of hec_reconstruct_crc_rows_device* -- a stripe of r < k *
// cell_len logical bytes gets its parity over [0, n0) and every unit the sums
// of its own bytes (ec_encode_rows.hip).  Full CRC32C stripes run as
// hec_encode_crc_device runs them, launch for launch.

}  // extern "C"

namespace {

// [the stripes' logical bytes: u64 x stripes], 0 rewritten to k * cell_len.
size_t encode_rows_workspace(size_t stripes) { return stripes * sizeof(uint64_t); }

// The lengths image of hec_encode_crc_rows_device_mixed: one u64 per stripe.
// Returns the bytes written.  Host only.
size_t write_encode_rows_image(uint8_t* host, const uint64_t* stripe_bytes, size_t stripes, size_t k,
                               size_t cell_len) {
    const uint64_t full = uint64_t(k) * cell_len;
    for (size_t s = 0; s < stripes; s++) {
        const uint64_t r = stripe_bytes[s] == 0 ? full : stripe_bytes[s];
        std::memcpy(host + s * sizeof(uint64_t), &r, sizeof(r));
    }
    return stripes * sizeof(uint64_t);
}

// The buffers of both entry points.
int encode_rows_buffers_check(const hec_coder* c, const uint8_t* const* d_data, const size_t* data_strides,
                              uint8_t* const* d_parity, const size_t* parity_strides, const uint8_t* d_sums) {
    if (!d_data || !data_strides || !d_parity || !parity_strides || !d_sums ||
        (reinterpret_cast<uintptr_t>(d_sums) & 3u))
        return HEC_ERR_INVALID_ARG;
    for (size_t i = 0; i < c->k; i++)
        if (!d_data[i]) return HEC_ERR_INVALID_ARG;
    for (size_t j = 0; j < c->m; j++)
        if (!d_parity[j]) return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// `stripes` stripes from batch stripe lens.stripe0 on, lengths in `lens`:
// gf_encode_crc_rows where the launcher takes the shape, else
// gf_encode_rows_bytes, four parity rows per launch, the first launch summing
// the data units.  The caller has checked the buffers.  The units are the
// call's own arrays in their order and the rows the coder's parity rows, so
// the slots are filled here, not from a plan.
int encode_rows_launch(const VerifiedCall& x, const hec::ReconRowsLens& lens, size_t stripes) {
    if (stripes == 0) return HEC_OK;
    const size_t k = x.k(), m = x.c->m;
    const uint8_t* enc = x.c->enc.data();
    if (x.bpc == 512 && m <= size_t(hec::kMaxR)) {
        hec::MatmulArgs a;
        std::memset(&a, 0, sizeof(a));
        for (size_t i = 0; i < k; i++) {
            a.in[i] = x.d_shards[i];
            a.in_stride[i] = x.shard_strides[i];
        }
        for (size_t j = 0; j < m; j++) {
            a.out[j] = x.d_out[j];
            a.out_stride[j] = x.out_strides[j];
            for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = enc[(k + j) * k + i];
        }
        a.k = int32_t(k);
        a.r = int32_t(m);
        a.cell_len = x.cell_len;
        a.stripes = stripes;
        hec::EncodeRowsCrcArgs cs;
        std::memset(&cs, 0, sizeof(cs));
        cs.sums = x.d_sums;
        cs.n_total = uint32_t(k + m);
        cs.kind = x.kind;
        const int rc = fused_status(hec::launch_encode_crc_rows(a, cs, lens, x.c->device, x.stream));
        if (rc != -1) return rc;  // -1: refused, nothing launched
    }
    hec::EncodeRowsBytesArgs a;
    std::memset(&a, 0, sizeof(a));
    for (size_t i = 0; i < k; i++) {
        a.in[i] = x.d_shards[i];
        a.in_stride[i] = x.shard_strides[i];
    }
    a.k = int32_t(k);
    a.n_total = uint32_t(k + m);
    a.sums = x.d_sums;
    a.kind = x.kind;
    a.stripes = stripes;
    a.lens = lens;
    a.cell_len = x.cell_len;
    a.bytes_per_checksum = x.bpc;
    return byte_route_rows(
        m, false,
        [&](size_t j0, size_t rn) {
            std::memset(a.coef, 0, sizeof(a.coef));
            for (size_t j = 0; j < rn; j++) {
                a.out[j] = x.d_out[j0 + j];
                a.out_stride[j] = x.out_strides[j0 + j];
                a.out_id[j] = uint8_t(k + j0 + j);
                for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = enc[(k + j0 + j) * k + i];
            }
            a.r = int32_t(rn);
            a.data_sums = j0 == 0;  // the data units are summed once
        },
        [&] { return hec::launch_encode_rows_bytes(a, x.c->device, x.stream); });
}

// `stripes` full stripes from stripe 0 on.  CRC32C: hec_encode_crc_device.
// CRC32: gf_encode_crc_rows with every stripe at k * cell_len where it takes
// the shape, else hec_encode_device, then hec_checksum_device.
int encode_rows_full(const VerifiedCall& x, int checksum_type, size_t stripes) {
    if (stripes == 0) return HEC_OK;
    hec_coder* c = x.c;
    if (x.kind == hec::crc::kCrc32c)
        return hec_encode_crc_device(c, x.d_shards, x.shard_strides, x.d_out, x.out_strides, x.cell_len, stripes, x.bpc,
                                     x.d_sums, x.stream);
    const size_t k = c->k, m = c->m;
    const bool one_pass = x.bpc == 512 && m <= size_t(hec::kMaxR) && x.cell_len % 16 == 0 &&
                          x.cell_len <= 0x7FFFFFFFull && stripes <= 0xFFFFFFFFull && register_kernel_k(k) &&
                          aligned16(x.d_shards, x.shard_strides, unit_bits(k)) &&
                          aligned16(x.d_out, x.out_strides, unit_bits(m));
    if (one_pass)
        return guarded([&]() -> int {
            DeviceGuard g(c->device);
            if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
            return encode_rows_launch(x, hec::ReconRowsLens{nullptr, uint64_t(k) * x.cell_len, 0}, stripes);
        });
    const int rc =
        hec_encode_device(c, x.d_shards, x.shard_strides, x.d_out, x.out_strides, x.cell_len, stripes, x.stream);
    if (rc != HEC_OK) return rc;
    const uint8_t* bases[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    size_t st[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
    for (size_t i = 0; i < k; i++) {
        bases[i] = x.d_shards[i];
        st[i] = x.shard_strides[i];
    }
    for (size_t j = 0; j < m; j++) {
        bases[k + j] = x.d_out[j];
        st[k + j] = x.out_strides[j];
    }
    return hec_checksum_device(c, checksum_type, bases, st, k + m, x.cell_len, stripes, x.bpc, x.d_sums, x.stream);
}


}  // namespace

extern "C" {

int hec_encode_crc_rows_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_data,
                               const size_t* data_strides, uint8_t* const* d_parity, const size_t* parity_strides,
                               size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint64_t data_len,
                               uint8_t* d_sums, void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    hec::crc::Geometry geo;
    if (!hec::crc::make_geometry(c->k + c->m, c->k, cell_len, stripes, bytes_per_checksum, data_len, &geo))
        return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_encode_crc_rows_device");
    chk = encode_rows_buffers_check(c, d_data, data_strides, d_parity, parity_strides, d_sums);
    if (chk != HEC_OK) return chk;
    if (stripes == 0) return HEC_OK;
    const VerifiedCall x{c, kind, d_data, data_strides, d_parity, parity_strides, cell_len, bytes_per_checksum,
                         nullptr, nullptr, d_sums, static_cast<hipStream_t>(hip_stream)};
    // every stripe full: one call over all of them
    if (geo.last_len == uint64_t(c->k) * cell_len) return encode_rows_full(x, checksum_type, stripes);
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    // the stripes - 1 full stripes, then one launch over the last
    const int rc = encode_rows_full(x, checksum_type, stripes - 1);
    if (rc != HEC_OK) return rc;
    return guarded([&]() -> int {
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        return encode_rows_launch(x, hec::ReconRowsLens{nullptr, geo.last_len, stripes - 1}, 1);
    });
}

size_t hec_encode_crc_rows_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c) return 0;
    return encode_rows_workspace(stripes);
}

int hec_encode_crc_rows_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_data,
                                     const size_t* data_strides, uint8_t* const* d_parity,
                                     const size_t* parity_strides, const uint64_t* stripe_bytes, size_t cell_len,
                                     size_t stripes, size_t bytes_per_checksum, uint8_t* d_sums, void* d_workspace,
                                     size_t workspace_bytes, void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    if (stripes > SIZE_MAX / sizeof(uint64_t)) return HEC_ERR_INVALID_ARG;
    bool any_short = false;
    for (size_t s = 0; stripe_bytes && s < stripes; s++) {
        if (stripe_bytes[s] > uint64_t(c->k) * cell_len) return HEC_ERR_INVALID_ARG;
        any_short = any_short || rows_short(stripe_bytes[s], c->k, cell_len);
    }
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_encode_crc_rows_device_mixed");
    chk = encode_rows_buffers_check(c, d_data, data_strides, d_parity, parity_strides, d_sums);
    if (chk != HEC_OK) return chk;
    if (any_short && (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 7u) ||
                      workspace_bytes < encode_rows_workspace(stripes)))
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    const VerifiedCall x{c, kind, d_data, data_strides, d_parity, parity_strides, cell_len, bytes_per_checksum,
                         nullptr, nullptr, d_sums, static_cast<hipStream_t>(hip_stream)};
    // no short entry: the uniform form with data_len == 0
    if (!any_short) return encode_rows_full(x, checksum_type, stripes);
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    // one launch over all stripes, full ones included, with the lengths on
    // the device
    return guarded([&]() -> int {
        DeviceGuard g(c->device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const int rc = upload_pinned(c, encode_rows_workspace(stripes), d_workspace, x.stream, [&](uint8_t* host) {
            write_encode_rows_image(host, stripe_bytes, stripes, c->k, cell_len);
        });
        if (rc != HEC_OK) return rc;
        return encode_rows_launch(x, hec::ReconRowsLens{static_cast<const uint64_t*>(d_workspace), 0, 0}, stripes);
    });
}

// ---- verified striped read into a file-order buffer ----------------------------
// hec_read_crc_rows_device*: the survivors verified over their own bytes, the
// lost data units rebuilt, all k data units of every stripe written at their
// file-order place, each for its own length (ec_read_rows.hip).  The mirror of
// hec_encode_crc_rows_device*.

}  // extern "C"

namespace {

// One present mask of a read and what its stripes run with: the survivors
// (the first k present units, so every present data unit is one) and the lost
// data units, both ascending.  `plan` holds the lost units' rows over the
// survivors (its first e rows); null when no data unit is lost.
struct ReadRowsGroup {
    uint64_t mask = 0;
    PlanRef plan;
    std::vector<uint8_t> survivors;  // k
    std::vector<uint8_t> lost;       // e
    size_t first = 0, count = 0;     // its stripes: list[first] .. list[first + count - 1]
};

// The groups of a batch in the order their masks first appear, every stripe
// once in `list` (by group, ascending within one) and its logical bytes beside
// it, 0 rewritten to k * cell_len.
struct ReadRowsPlan {
    std::vector<ReadRowsGroup> groups;
    std::vector<uint32_t> list;
    std::vector<uint64_t> bytes;
};

// Survivors and lost data units of one mask.  HEC_ERR_NOT_ENOUGH_SHARDS with
// fewer than k units present.  Host only.
int read_rows_group(hec_coder* c, uint64_t mask, ReadRowsGroup* g) {
    const size_t k = c->k;
    g->mask = mask;
    g->plan.reset();
    g->survivors.clear();
    g->lost.clear();
    if ((mask & unit_bits(k)) == unit_bits(k)) {  // e = 0: the data units, no parity unit touched
        for (size_t u = 0; u < k; u++) g->survivors.push_back(uint8_t(u));
        return HEC_OK;
    }
    RowPlan rp;
    const int rc = decode_rows(c, mask, &rp);
    if (rc != HEC_OK) return rc;
    g->plan = rp.plan;
    for (size_t u : rp.plan->survivors) g->survivors.push_back(uint8_t(u));
    for (size_t u : rp.plan->missing) g->lost.push_back(uint8_t(u));
    return HEC_OK;
}

// Groups the stripes of a batch by present[s] (bits k + m and above ignored).
// stripe_bytes = null: all full.  Nothing is queued; the first mask that has
// no plan ends the call with its status.  Host only.
int read_rows_plan(hec_coder* c, const uint64_t* present, const uint64_t* stripe_bytes, size_t stripes, size_t cell_len,
                   ReadRowsPlan* p) {
    const uint64_t all = unit_bits(c->k + c->m), full = uint64_t(c->k) * cell_len;
    std::unordered_map<uint64_t, uint32_t> ids;
    std::vector<uint32_t> group_of(stripes);
    for (size_t s = 0; s < stripes; s++) {
        const uint64_t mask = present[s] & all;
        auto it = ids.find(mask);
        if (it == ids.end()) {
            ReadRowsGroup g;
            const int rc = read_rows_group(c, mask, &g);
            if (rc != HEC_OK) return rc;
            it = ids.emplace(mask, uint32_t(p->groups.size())).first;
            p->groups.push_back(std::move(g));
        }
        group_of[s] = it->second;
        p->groups[it->second].count++;
    }
    size_t at = 0;
    for (ReadRowsGroup& g : p->groups) {
        g.first = at;
        at += g.count;
        g.count = 0;
    }
    p->list.resize(stripes);
    p->bytes.resize(stripes);
    for (size_t s = 0; s < stripes; s++) {
        ReadRowsGroup& g = p->groups[group_of[s]];
        const size_t i = g.first + g.count++;
        p->list[i] = uint32_t(s);
        p->bytes[i] = (!stripe_bytes || stripe_bytes[s] == 0) ? full : stripe_bytes[s];
    }
    return HEC_OK;
}

// The workspace: [stripe lists: u32 x stripes][pad to kAlign][their bytes: u64 x stripes].
struct ReadRowsLayout {
    size_t bytes_pos, need;
};

ReadRowsLayout read_rows_layout(size_t stripes) {
    ReadRowsLayout w;
    w.bytes_pos = align_up(stripes * sizeof(uint32_t));
    w.need = w.bytes_pos + stripes * sizeof(uint64_t);
    return w;
}

size_t read_rows_workspace(size_t stripes) { return read_rows_layout(stripes).need; }

// Writes every byte of the image (lists, zeroes in the pad, lengths).
void write_read_rows_image(uint8_t* host, const ReadRowsPlan& p, const ReadRowsLayout& w) {
    const size_t list_bytes = p.list.size() * sizeof(uint32_t);
    if (list_bytes) std::memcpy(host, p.list.data(), list_bytes);
    std::memset(host + list_bytes, 0, w.bytes_pos - list_bytes);
    if (!p.bytes.empty()) std::memcpy(host + w.bytes_pos, p.bytes.data(), p.bytes.size() * sizeof(uint64_t));
}

// What both entry points check before the coder's device is looked at, behind
// recon_rows_check and the lengths.
int read_rows_stride_check(const hec_coder* c, size_t cell_len, size_t file_stride) {
    return file_stride != 0 && file_stride < c->k * cell_len ? HEC_ERR_INVALID_ARG : HEC_OK;
}

// ... and behind it.
int read_rows_buffers_check(const uint8_t* const* d_shards, const size_t* shard_strides, const uint8_t* d_file,
                            const uint8_t* d_expected, const uint8_t* d_bad) {
    if (!d_shards || !shard_strides || !d_file || (d_expected && !d_bad) ||
        (reinterpret_cast<uintptr_t>(d_expected) & 3u))
        return HEC_ERR_INVALID_ARG;
    return HEC_OK;
}

// `stripes` stripes of one group (d_list, or lens.stripe0 on): gf_read_rows
// where the launcher takes the shape, else gf_read_rows_bytes over the lost
// data units, four per launch (one launch where none is lost), the first
// launch verifying every survivor and copying the present data units.  The
// rows are those of the decode plan (g.plan->matrix), so they are filled here.
int read_rows_launch(const VerifiedCall& x, const ReadRowsGroup& g, const uint32_t* d_list, size_t stripes,
                     const hec::ReconRowsLens& lens, uint8_t* d_file, size_t file_stride) {
    if (stripes == 0) return HEC_OK;
    const size_t k = x.k(), e = g.lost.size();
    if (x.bpc == 512 && e <= size_t(hec::kMaxR)) {
        hec::MatmulArgs a;
        std::memset(&a, 0, sizeof(a));
        hec::ReadRowsCrcArgs cs;
        std::memset(&cs, 0, sizeof(cs));
        fill_units(g.survivors.data(), k, x.shards(), unit_slots(a.in, a.in_stride, cs.shard_id));
        for (size_t j = 0; j < e; j++) {
            cs.shard_id[k + j] = g.lost[j];
            for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = g.plan->matrix[j * k + i];
        }
        a.k = int32_t(k);
        a.r = int32_t(e);
        a.cell_len = x.cell_len;
        a.stripes = stripes;
        cs.expected = x.d_expected;
        cs.bad = x.d_bad;
        cs.file = d_file;
        cs.file_stride = file_stride;
        cs.n_total = uint32_t(x.n());
        cs.kind = x.kind;
        cs.stripe_list = d_list;
        const int rc = fused_status(hec::launch_read_crc_rows(a, cs, lens, x.c->device, x.stream));
        if (rc != -1) return rc;  // -1: refused, nothing launched
    }
    hec::ReadRowsBytesArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_units(g.survivors.data(), k, x.shards(), unit_slots(a.in, a.in_stride, a.in_id));
    size_t data_in = 0;
    for (size_t i = 0; i < k; i++) data_in += g.survivors[i] < k;
    a.k = int32_t(k);
    a.n_total = uint32_t(x.n());
    a.file = d_file;
    a.file_stride = file_stride;
    a.expected = x.d_expected;
    a.bad = x.d_bad;
    a.kind = x.kind;
    a.stripe_list = d_list;
    a.stripes = stripes;
    a.lens = lens;
    a.cell_len = x.cell_len;
    a.bytes_per_checksum = x.bpc;
    a.parity_in = x.d_expected ? int32_t(k - data_in) : 0;
    return byte_route_rows(
        e, true,
        [&](size_t j0, size_t rn) {
            std::memset(a.coef, 0, sizeof(a.coef));
            std::memset(a.role, hec::kReadRowsSkip, sizeof(a.role));
            for (size_t i = 0; j0 == 0 && i < data_in; i++) a.role[g.survivors[i]] = uint8_t(i);
            for (size_t j = 0; j < rn; j++) {
                a.role[g.lost[j0 + j]] = uint8_t(hec::kReadRowsLost | j);
                for (size_t i = 0; i < k; i++) a.coef[j * hec::kMaxK + i] = g.plan->matrix[(j0 + j) * k + i];
            }
            a.r = int32_t(rn);
            if (j0 != 0) {  // the survivors are verified once
                a.expected = nullptr;
                a.bad = nullptr;
                a.parity_in = 0;
            }
        },
        [&] { return hec::launch_read_rows_bytes(a, x.c->device, x.stream); });
}


}  // namespace

extern "C" {

int hec_read_crc_rows_device(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                             const size_t* shard_strides, uint8_t* d_file, size_t file_stride, size_t cell_len,
                             size_t stripes, size_t bytes_per_checksum, uint64_t data_len, const uint8_t* d_expected,
                             uint8_t* d_bad, void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    hec::crc::Geometry geo;
    if (!hec::crc::make_geometry(c->k + c->m, c->k, cell_len, stripes, bytes_per_checksum, data_len, &geo))
        return HEC_ERR_INVALID_ARG;
    if (read_rows_stride_check(c, cell_len, file_stride) != HEC_OK) return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_read_crc_rows_device");
    chk = read_rows_buffers_check(d_shards, shard_strides, d_file, d_expected, d_bad);
    if (chk != HEC_OK) return chk;
    if (stripes == 0) return HEC_OK;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        uint64_t mask = 0;
        for (size_t i = 0; i < c->k + c->m; i++)
            if (d_shards[i]) mask |= uint64_t(1) << i;
        ReadRowsGroup g;
        int rc = read_rows_group(c, mask, &g);
        if (rc != HEC_OK) return rc;
        DeviceGuard dg(c->device);
        if (!dg.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        const uint64_t full = uint64_t(c->k) * cell_len;
        const size_t stride = file_stride ? file_stride : size_t(full);
        // one launch over the stripes - 1 full stripes and one over the last,
        // or one over all of them when the last is full too
        const size_t n_full = geo.last_len == full ? stripes : stripes - 1;
        rc = read_rows_launch(x, g, nullptr, n_full, hec::ReconRowsLens{nullptr, full, 0}, d_file, stride);
        if (rc != HEC_OK || n_full == stripes) return rc;
        return read_rows_launch(x, g, nullptr, 1, hec::ReconRowsLens{nullptr, geo.last_len, stripes - 1}, d_file,
                                stride);
    });
}

size_t hec_read_crc_rows_mixed_workspace_size(const hec_coder_t* c, size_t stripes) {
    if (!c || stripes > SIZE_MAX / 16) return 0;
    return read_rows_workspace(stripes);
}

int hec_read_crc_rows_device_mixed(hec_coder_t* c, int checksum_type, const uint8_t* const* d_shards,
                                   const size_t* shard_strides, uint8_t* d_file, size_t file_stride,
                                   const uint64_t* present, const uint64_t* stripe_bytes, size_t cell_len,
                                   size_t stripes, size_t bytes_per_checksum, const uint8_t* d_expected, uint8_t* d_bad,
                                   void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    int kind;
    int chk = recon_rows_check(c, checksum_type, cell_len, bytes_per_checksum, &kind);
    if (chk != HEC_OK) return chk;
    if (stripes > 0xFFFFFFFFull) return HEC_ERR_INVALID_ARG;
    for (size_t s = 0; stripe_bytes && s < stripes; s++)
        if (stripe_bytes[s] > uint64_t(c->k) * cell_len) return HEC_ERR_INVALID_ARG;
    if (read_rows_stride_check(c, cell_len, file_stride) != HEC_OK) return HEC_ERR_INVALID_ARG;
    if (c->device == HEC_DEVICE_HOST) return host_only("hec_read_crc_rows_device_mixed");
    chk = read_rows_buffers_check(d_shards, shard_strides, d_file, d_expected, d_bad);
    if (chk != HEC_OK) return chk;
    const ReadRowsLayout w = read_rows_layout(stripes);
    if (!present || !d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 7u) || workspace_bytes < w.need)
        return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    return guarded([&]() -> int {
        // 1. the distinct masks, their survivors and lost data units (host);
        // fail before anything is queued
        ReadRowsPlan plan;
        int rc = read_rows_plan(c, present, stripe_bytes, stripes, cell_len, &plan);
        if (rc != HEC_OK) return rc;
        for (const ReadRowsGroup& g : plan.groups)
            for (uint8_t u : g.survivors)
                if (!d_shards[u]) return HEC_ERR_INVALID_ARG;  // a survivor needs storage
        DeviceGuard dg(c->device);
        if (!dg.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const VerifiedCall x{c, kind, d_shards, shard_strides, nullptr, nullptr, cell_len, bytes_per_checksum,
                             d_expected, d_bad, nullptr, static_cast<hipStream_t>(hip_stream)};
        // 2. the lists and lengths, one copy
        uint8_t* ws = static_cast<uint8_t*>(d_workspace);
        rc = upload_pinned(c, w.need, ws, x.stream, [&](uint8_t* host) { write_read_rows_image(host, plan, w); });
        if (rc != HEC_OK) return rc;
        // 3. one launch per mask over its stripes, full and short together
        const uint32_t* d_list = reinterpret_cast<const uint32_t*>(ws);
        const uint64_t* d_bytes = reinterpret_cast<const uint64_t*>(ws + w.bytes_pos);
        const size_t stride = file_stride ? file_stride : c->k * cell_len;
        for (const ReadRowsGroup& g : plan.groups) {
            rc = read_rows_launch(x, g, d_list + g.first, g.count, hec::ReconRowsLens{d_bytes + g.first, 0, 0}, d_file,
                                  stride);
            if (rc != HEC_OK) return rc;
        }
        return HEC_OK;
    });
}

// ---- multi-GPU coder group -----------------------------------

}  // extern "C"

struct hec_group {
    std::vector<hec_coder_t*> coders;  // one per slot
};

namespace {

void group_range(size_t total, size_t n, size_t i, size_t* first, size_t* count) {
    const size_t base = total / n, extra = total % n;  // hdfs_native_ec.dist.shard_range
    *first = i * base + std::min(i, extra);
    *count = base + (i < extra ? 1 : 0);
}

// Runs body(slot) for every slot, slots 1.. on their own threads and slot 0 on
// the caller's; returns the lowest failing slot's status and copies its
// hec_last_error() text into the caller's thread.
template <class F>
int group_run(hec_group* g, F&& body) {
    const size_t n = g->coders.size();
    std::vector<int> rc(n, HEC_OK);
    std::vector<std::string> err(n);
    auto run = [&](size_t i) {
        rc[i] = body(i);
        if (rc[i] != HEC_OK) err[i] = g_last_error;
    };
    // Slots whose thread cannot be started run inline after slot 0; every
    // started thread is joined before returning (a joinable std::thread that
    // is destroyed would terminate the process across the ABI).
    std::vector<std::thread> th;
    std::vector<size_t> inline_slots;
    th.reserve(n);
    for (size_t i = 1; i < n; i++) {
        try {
            th.emplace_back(run, i);
        } catch (...) {
            inline_slots.push_back(i);
        }
    }
    run(0);
    for (size_t i : inline_slots) run(i);
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n; i++)
        if (rc[i] != HEC_OK) {
            std::snprintf(g_last_error, sizeof(g_last_error), "group slot %zu: %s", i, err[i].c_str());
            return rc[i];
        }
    return HEC_OK;
}

}  // namespace

extern "C" {

int hec_group_create(const char* codec, size_t data_units, size_t parity_units, const int* devices,
                     size_t n_devices, hec_group_t** out) {
    if (!out) return HEC_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || n_devices == 0 || n_devices > 64) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        auto* g = new hec_group();
        for (size_t i = 0; i < n_devices; i++) {
            hec_coder_t* c = nullptr;
            const int rc = hec_coder_create_codec(codec, data_units, parity_units, devices[i], &c);
            if (rc != HEC_OK) {
                hec_group_destroy(g);
                return rc;
            }
            g->coders.push_back(c);
        }
        *out = g;
        return HEC_OK;
    });
}

void hec_group_destroy(hec_group_t* g) {
    if (!g) return;
    for (auto* c : g->coders) hec_coder_destroy(c);
    delete g;
}

size_t hec_group_size(const hec_group_t* g) { return g ? g->coders.size() : 0; }

hec_coder_t* hec_group_coder(hec_group_t* g, size_t slot) {
    return (g && slot < g->coders.size()) ? g->coders[slot] : nullptr;
}

int hec_group_range(const hec_group_t* g, size_t total, size_t slot, size_t* first, size_t* count) {
    if (!g || !first || !count || slot >= g->coders.size()) return HEC_ERR_INVALID_ARG;
    group_range(total, g->coders.size(), slot, first, count);
    return HEC_OK;
}

int hec_group_encode_host_batch(hec_group_t* g, const uint8_t* h_data, uint8_t* h_parity, size_t cell_len,
                                size_t stripes, size_t chunk_stripes) {
    if (!g || !h_data || !h_parity || cell_len == 0 || chunk_stripes == 0) return HEC_ERR_INVALID_ARG;
    if (stripes == 0) return HEC_OK;
    return guarded([&] {
        return group_run(g, [&](size_t i) {
            hec_coder_t* c = g->coders[i];
            size_t first, count;
            group_range(stripes, g->coders.size(), i, &first, &count);
            if (count == 0) return int(HEC_OK);
            return hec_encode_host_batch(c, h_data + first * c->k * cell_len, h_parity + first * c->m * cell_len,
                                         cell_len, count, chunk_stripes);
        });
    });
}

int hec_group_decode_host_batch(hec_group_t* g, const uint8_t* const* h_vertical, size_t cell_len, size_t rows,
                                uint8_t* h_file, size_t chunk_rows) {
    if (!g || !h_vertical || !h_file || cell_len == 0 || chunk_rows == 0) return HEC_ERR_INVALID_ARG;
    if (rows == 0) return HEC_OK;
    return guarded([&] {
        return group_run(g, [&](size_t i) {
            hec_coder_t* c = g->coders[i];
            size_t first, count;
            group_range(rows, g->coders.size(), i, &first, &count);
            if (count == 0) return int(HEC_OK);
            const uint8_t* vert[HEC_MAX_DATA_UNITS + HEC_MAX_PARITY_UNITS];
            for (size_t s = 0; s < c->k + c->m; s++)
                vert[s] = h_vertical[s] ? h_vertical[s] + first * cell_len : nullptr;
            return hec_decode_host_batch(c, vert, cell_len, count, h_file + first * c->k * cell_len, chunk_rows);
        });
    });
}

}  // extern "C"

// Device-resident batches over the group: every slot's launch is enqueued
// from the calling thread (an enqueue is microseconds and asynchronous, so
// the GPUs run concurrently without host threads); every slot is tried, the
// lowest failing slot's status is returned.
namespace {
template <class F>
int group_enqueue(hec_group_t* g, F&& body) {
    int first_rc = HEC_OK;
    size_t first_slot = 0;
    std::string first_err;
    for (size_t i = 0; i < g->coders.size(); i++) {
        const int rc = body(i);
        if (rc != HEC_OK && first_rc == HEC_OK) {
            first_rc = rc;
            first_slot = i;
            first_err = g_last_error;
        }
    }
    if (first_rc != HEC_OK)
        std::snprintf(g_last_error, sizeof(g_last_error), "group slot %zu: %s", first_slot, first_err.c_str());
    return first_rc;
}
}  // namespace

extern "C" {

int hec_group_encode_device(hec_group_t* g, const uint8_t* const* d_data, const size_t* data_strides,
                            uint8_t* const* d_parity, const size_t* parity_strides, size_t cell_len,
                            const size_t* stripes, void* const* hip_streams) {
    if (!g || !d_data || !data_strides || !d_parity || !parity_strides || !stripes || cell_len == 0)
        return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        return group_enqueue(g, [&](size_t i) {
            hec_coder_t* c = g->coders[i];
            if (stripes[i] == 0) return int(HEC_OK);
            return hec_encode_device(c, d_data + i * c->k, data_strides + i * c->k, d_parity + i * c->m,
                                     parity_strides + i * c->m, cell_len, stripes[i],
                                     hip_streams ? hip_streams[i] : nullptr);
        });
    });
}

int hec_group_decode_device(hec_group_t* g, const uint8_t* const* d_shards, const size_t* shard_strides,
                            uint8_t* const* d_out, const size_t* out_strides, size_t cell_len,
                            const size_t* stripes, void* const* hip_streams) {
    if (!g || !d_shards || !shard_strides || !d_out || !out_strides || !stripes || cell_len == 0)
        return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        return group_enqueue(g, [&](size_t i) {
            hec_coder_t* c = g->coders[i];
            if (stripes[i] == 0) return int(HEC_OK);
            const size_t n = c->k + c->m;
            return hec_decode_device(c, d_shards + i * n, shard_strides + i * n, d_out + i * c->k,
                                     out_strides + i * c->k, cell_len, stripes[i],
                                     hip_streams ? hip_streams[i] : nullptr);
        });
    });
}

int hec_device_alloc(int device, size_t bytes, unsigned flags, void** out) {
    if (!out || bytes == 0 || (flags & ~unsigned(HEC_ALLOC_CONTIGUOUS))) return HEC_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const unsigned hf = (flags & HEC_ALLOC_CONTIGUOUS) ? hipDeviceMallocContiguous : hipDeviceMallocDefault;
        HEC_HIP(hipExtMallocWithFlags(out, bytes, hf), HEC_ERR_NO_MEMORY);
        return HEC_OK;
    });
}

int hec_device_free(int device, void* ptr) {
    if (!ptr) return HEC_OK;
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        HEC_HIP(hipFree(ptr), HEC_ERR_DEVICE);
        return HEC_OK;
    });
}

int hec_device_copy(int device, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return HEC_OK;
    if (!dst || !src) return HEC_ERR_INVALID_ARG;
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        HEC_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault), HEC_ERR_DEVICE);
        return HEC_OK;
    });
}

int hec_device_synchronize(int device, void* hip_stream) {
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        HEC_HIP(hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)), HEC_ERR_DEVICE);
        return HEC_OK;
    });
}

// ---- NUMA-placed pinned host buffers -------------------------------------

namespace {

std::mutex g_host_mu;
std::unordered_map<void*, size_t> g_host_allocs;  // ptr -> mapped bytes

int numa_node_of(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return -1;
    std::string id(bus);
    for (auto& ch : id) ch = char(std::tolower(static_cast<unsigned char>(ch)));
    std::ifstream f("/sys/bus/pci/devices/" + id + "/numa_node");
    int node = -1;
    if (!(f >> node)) return -1;
    return node;
}

}  // namespace

void hec_queue_stats(int device, uint64_t* streams, uint64_t* graph_sets, int* keyed_by_id) {
    if (streams) *streams = 0;
    if (graph_sets) *graph_sets = 0;
    if (keyed_by_id) *keyed_by_id = 0;
    try {
        int n = 0;
        if (device < 0 || hipGetDeviceCount(&n) != hipSuccess || device >= n) {
            (void)hipGetLastError();
            return;  // no such device: zeros, and no per-device state created
        }
        hec::queue_stats(device, streams, graph_sets);
        if (keyed_by_id) *keyed_by_id = hec::queue_keyed_by_id();
    } catch (...) {
        if (streams) *streams = 0;
        if (graph_sets) *graph_sets = 0;
    }
}

int hec_device_numa_node(int device) {
    try {
        return numa_node_of(device);
    } catch (...) {
        return -1;
    }
}

int hec_host_alloc(int device, size_t bytes, int numa_node, void** out) {
    if (!out || bytes == 0 || numa_node < -1 || numa_node >= 1024) return HEC_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded([&] {
        DeviceGuard g(device);
        if (!g.ok) return fail(HEC_ERR_DEVICE, "hipSetDevice", hipErrorInvalidDevice);
        const int node = numa_node >= 0 ? numa_node : numa_node_of(device);
        const size_t page = size_t(sysconf(_SC_PAGESIZE));
        const size_t len = (bytes + page - 1) / page * page;
        void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return int(HEC_ERR_NO_MEMORY);
        if (node >= 0) {
            // MPOL_BIND to the node before the pages exist: every page is
            // faulted in there by the touch below
            unsigned long mask[1024 / (8 * sizeof(unsigned long))] = {0};
            mask[node / (8 * sizeof(unsigned long))] |= 1ul << (node % (8 * sizeof(unsigned long)));
            const long MPOL_BIND_ = 2;
            if (syscall(SYS_mbind, p, len, MPOL_BIND_, mask, 1024ul, 0ul) != 0) {
                munmap(p, len);
                std::snprintf(g_last_error, sizeof(g_last_error), "mbind to NUMA node %d failed", node);
                return int(HEC_ERR_INVALID_ARG);
            }
        }
        std::memset(p, 0, len);
        const hipError_t e = hipHostRegister(p, len, hipHostRegisterDefault);
        if (e != hipSuccess) {
            munmap(p, len);
            (void)hipGetLastError();
            return fail(HEC_ERR_NO_MEMORY, "hipHostRegister", e);
        }
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_allocs[p] = len;
        *out = p;
        return int(HEC_OK);
    });
}

int hec_host_free(void* ptr) {
    if (!ptr) return HEC_OK;
    return guarded([&] {
        size_t len = 0;
        {
            std::lock_guard<std::mutex> lk(g_host_mu);
            auto it = g_host_allocs.find(ptr);
            if (it == g_host_allocs.end()) return int(HEC_ERR_INVALID_ARG);
            len = it->second;
            g_host_allocs.erase(it);
        }
        (void)hipHostUnregister(ptr);
        (void)hipGetLastError();
        munmap(ptr, len);
        return int(HEC_OK);
    });
}

#ifdef HEC_EXPERIMENTAL
// Measurement knobs (include/hdfs_ec_amd_exp.h): the HEC_EXPERIMENTAL build
// only.  The product library has no knobs and does not export this symbol.
int hec_tune_set(int key, int value) {
    const int rc = hec::tune_store(key, value);
    if (rc != HEC_OK)
        std::snprintf(g_last_error, sizeof(g_last_error), "hec_tune_set: key %d value %d unknown or out of range", key,
                      value);
    return rc;
}
#endif

}  // extern "C"
