/*
 * hdfs_ec_amd.h -- C ABI of the MI355X-native Reed-Solomon erasure-coding
 * engine that drops in behind hdfs-native's internal EC functions.
 *
 * Reference interface replaced (hdfs-native 0.14.1, Rust; public under the
 * `benchmark` feature, rust/src/lib.rs:49-52):
 *   hdfs_native::ec::gf256::Coder::new            rust/src/ec/gf256.rs:32-38
 *   hdfs_native::ec::gf256::Coder::gen_rs_matrix  rust/src/ec/gf256.rs:40-57
 *   hdfs_native::ec::gf256::Coder::encode         rust/src/ec/gf256.rs:61-80
 *   hdfs_native::ec::gf256::Coder::decode         rust/src/ec/gf256.rs:84-137
 *   Matrix::select_rows / Matrix::invert          rust/src/ec/matrix.rs:74-84, :101-162
 *   Mul<&[&[u8]]> for Matrix (the hot loop)       rust/src/ec/matrix.rs:204-231
 * Callers in the reference: CellBuffer::encode (rust/src/hdfs/block_writer.rs:838),
 * EcSchema::ec_decode (rust/src/ec/mod.rs:71-72), rust/benches/ec.rs.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every function returns an int status
 *    (HEC_OK == 0) and never aborts or throws across the ABI.
 *  - GF(2^8) modulo 0x11D, Hadoop Cauchy coding matrix: results are
 *    bit-identical to the reference Coder on the same inputs.
 *  - A coder is bound to one HIP device.  The host-buffer calls
 *    (hec_encode/hec_decode) are synchronous and serialised per coder by an
 *    internal lock (one coder may be shared by threads; use one coder per
 *    thread for concurrency).  The device calls are asynchronous: they only
 *    enqueue work on the caller's HIP stream (`hip_stream` is a hipStream_t
 *    passed as void*; NULL = the null stream).  Their only lock is the
 *    stream's work-queue counter-set lock, held from choosing the launch's
 *    counter set to enqueuing its kernel (see hec_queue_stats).
 */
#ifndef HDFS_EC_AMD_H
#define HDFS_EC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEC_ABI_VERSION 5

/* Status codes */
#define HEC_OK 0
#define HEC_ERR_INVALID_ARG (-1)       /* reference: assert!/panic (gf256.rs:62-65, matrix.rs:57) */
#define HEC_ERR_NOT_ENOUGH_SHARDS (-2) /* HdfsError::ErasureCodingError("Not enough valid shards") gf256.rs:107-111 */
#define HEC_ERR_UNSUPPORTED_CODEC (-3) /* HdfsError::UnsupportedErasureCodingPolicy mod.rs:74-78 */
#define HEC_ERR_DEVICE (-4)            /* HIP runtime / launch failure */
#define HEC_ERR_NO_MEMORY (-5)         /* host or device allocation failed */
#define HEC_ERR_SINGULAR (-6)          /* reference panics "Matrix is singular" matrix.rs:121-123 */
#define HEC_ERR_CHECKSUM (-7)          /* HdfsError::ChecksumError connection.rs:497-499 */

/* Chunk checksum types: ChecksumTypeProto values (rust/src/proto/hadoop.hdfs.rs:1363),
 * mapped to algorithms by ReadPacket::get_data (rust/src/hdfs/connection.rs:483-487). */
#define HEC_CHECKSUM_NULL 0   /* CHECKSUM_NULL: no verification */
#define HEC_CHECKSUM_CRC32 1  /* crc 3.4 CRC_32_CKSUM (connection.rs:37): MSB-first 0x04C11DB7, init 0, xorout ~0 */
#define HEC_CHECKSUM_CRC32C 2 /* crc 3.4 CRC_32_ISCSI (connection.rs:38): Castagnoli, reflected, init/xorout ~0 */

/* Limits of this engine (the reference has k+m <= 256 through `r as u8`). */
#define HEC_MAX_DATA_UNITS 32
#define HEC_MAX_PARITY_UNITS 16

typedef struct hec_coder hec_coder_t;

/* Human-readable text for a status code (static storage). */
const char *hec_strerror(int status);
int hec_abi_version(void);
/* Detail of the last failing HIP call made by this thread ("" if none). */
const char *hec_last_error(void);

/* ---- Field / matrix helpers (host only, no device needed) ------------- */

/* Coder::gen_rs_matrix (gf256.rs:40-57): writes the (k+m) x k coding matrix,
 * row-major, into out[(k+m)*k]. */
int hec_gen_rs_matrix(size_t data_units, size_t parity_units, uint8_t *out);

/* The same for a codec name as hec_coder_create_codec ("rs", "xor",
 * "rs-legacy"): the (k+m) x k matrix a coder of that codec encodes and
 * decodes with.  HEC_ERR_UNSUPPORTED_CODEC for other names. */
int hec_gen_codec_matrix(const char *codec, size_t data_units, size_t parity_units, uint8_t *out);

/* Matrix::invert (matrix.rs:101-162): in-place inverse of an n x n
 * row-major matrix over GF(2^8).  HEC_ERR_SINGULAR where the reference panics. */
int hec_matrix_invert(uint8_t *mat, size_t n);

/* The decode plan of Coder::decode (gf256.rs:84-126) for a presence mask.
 * present[k+m]: non-zero = shard available.  On HEC_OK:
 *   *n_missing   = e, the number of missing DATA shards (0 => nothing to do);
 *   survivors[k] = the first k present shard indices, ascending;
 *   missing[e]   = the missing data indices, ascending;
 *   matrix[e*k]  = rows of inverse(select_rows(encode_matrix, survivors))
 *                  for the missing indices (row-major).
 * Returns HEC_ERR_NOT_ENOUGH_SHARDS when e > 0 and fewer than k are present. */
int hec_decode_plan(size_t data_units, size_t parity_units, const uint8_t *present,
                    size_t *n_missing, size_t *survivors, size_t *missing, uint8_t *matrix);

/* ---- Coder lifecycle (Coder::new, gf256.rs:32-38) --------------------- */

/* `device` value of a host-only coder: no HIP call is made (creation cannot
 * fail for want of a GPU).  hec_encode / hec_decode and the host-batch calls
 * (hec_encode_host_batch, hec_decode_host_batch, hec_*_rows_host) run the
 * engine's host routine (hec_gf_matmul_host) whatever the host limit; the
 * device-resident calls return HEC_ERR_DEVICE.  This keeps the reference's
 * infallible Coder::new (gf256.rs:32-38) on a host without a visible GPU. */
#define HEC_DEVICE_HOST (-2)

/* Creates a coder for RS(data_units, parity_units) on HIP device `device`
 * (or HEC_DEVICE_HOST).
 * 1 <= data_units <= HEC_MAX_DATA_UNITS, 1 <= parity_units <= HEC_MAX_PARITY_UNITS. */
int hec_coder_create(size_t data_units, size_t parity_units, int device, hec_coder_t **out);
/* Same with a codec name: "rs" (the default above), "xor" (Hadoop XOR-k-1:
 * parity = XOR of the data units; parity_units must be 1) or "rs-legacy"
 * (Hadoop RSRawEncoderLegacy: systematic cyclic RS, generator roots 2^0 ..
 * 2^(m-1), data unit i at degree m+i; policy 3, RS-LEGACY-6-3-1024k).  The
 * reference resolves policies 3 and 4 (ec/mod.rs:118-131) but decodes only
 * "rs" (mod.rs:69-78); this engine codes all three on the same kernels.  Any
 * other name -> HEC_ERR_UNSUPPORTED_CODEC. */
int hec_coder_create_codec(const char *codec, size_t data_units, size_t parity_units, int device,
                           hec_coder_t **out);
void hec_coder_destroy(hec_coder_t *coder);
size_t hec_coder_data_units(const hec_coder_t *coder);
size_t hec_coder_parity_units(const hec_coder_t *coder);
int hec_coder_device(const hec_coder_t *coder);

/* Pooled coders for callers that build a Coder per row: the reference
 * constructs one per decoded row (ec/mod.rs:71-72, Coder::new gf256.rs:32-38)
 * and one per block writer (block_writer.rs:787).  hec_coder_acquire hands
 * out an idle coder of the same (codec, data_units, parity_units, device)
 * from a process-wide pool, or creates one; hec_coder_release returns it (at
 * most 64 idle per key are kept, the rest destroyed).  An acquired coder is
 * the caller's alone until released; steady state costs a mutex and a
 * vector pop -- no stream, event or buffer creation.  device -1 = any device
 * (round-robin over the visible ones; a host-only coder, HEC_DEVICE_HOST, when
 * no GPU is visible), HEC_DEVICE_HOST = host-only.  Release resets the coder's host
 * limit to the default (a setting never carries over to the next acquirer)
 * and ignores a second release of a coder that is already idle in the pool.
 * hec_coder_release on a coder from hec_coder_create destroys it.
 * hec_coder_pool_trim destroys every idle pooled coder and returns how many. */
int hec_coder_acquire(const char *codec, size_t data_units, size_t parity_units, int device, hec_coder_t **out);
void hec_coder_release(hec_coder_t *coder);
size_t hec_coder_pool_trim(void);

/* Routing of the host-buffer drop-ins below (hec_encode / hec_decode on
 * pageable buffers): rows of at most `max_shard_len` bytes per shard are coded
 * by the engine's host routine (hec_gf_matmul_host; rows of >= 256 KiB per
 * shard split over $HEC_HOST_THREADS threads, default 4), longer ones go
 * through the device (pinned bounce buffers, H2D, kernel, D2H).  Per coder;
 * default SIZE_MAX = every row on the host: measured per size, cold and hot,
 * the PCIe round trip of a pageable row never paid for itself;
 * 0 = always the device.  The batched and device-resident calls are not
 * affected. */
int hec_coder_set_host_limit(hec_coder_t *coder, size_t max_shard_len);
size_t hec_coder_host_limit(const hec_coder_t *coder);

/* ---- Host-buffer drop-ins (synchronous) -------------------------------- */

/* Coder::encode (gf256.rs:61-80).  data[k] host buffers of shard_len bytes
 * each; parity[m] caller-allocated host buffers of shard_len bytes, fully
 * overwritten.  shard_len == 0 -> HEC_ERR_INVALID_ARG (the reference panics,
 * matrix.rs:57).  Any shard_len >= 1 is accepted, including tails that are not
 * a multiple of 16. */
int hec_encode(hec_coder_t *coder, const uint8_t *const *data, size_t shard_len,
               uint8_t *const *parity);

/* Coder::decode (gf256.rs:84-137).  shards[k+m] host buffers of shard_len
 * bytes, NULL = missing.  For every missing DATA index i (< k) out[i] must
 * point to shard_len writable bytes and receives the reconstructed shard;
 * out[] entries for present shards and for parity indices are never touched
 * (missing parity is not regenerated, gf256.rs:96-97).  Survivors are the
 * first k present shards in index order.  Returns HEC_OK without writing when
 * no data shard is missing, HEC_ERR_NOT_ENOUGH_SHARDS when fewer than k
 * shards are present. */
int hec_decode(hec_coder_t *coder, const uint8_t *const *shards, size_t shard_len,
               uint8_t *const *out);

/* The hot loop Mul<&[&[u8]]> (matrix.rs:204-231) on the host, for rows too
 * small for the device: out[j] = sum_i matrix[j*cols + i] * in[i], len bytes
 * each, any length and alignment; AVX-512BW+GFNI affine transforms (one
 * vgf2p8affineqb per 64 bytes per coefficient), else AVX2 split-nibble
 * shuffles, else scalar tables (hec_host_isa names the one in use).
 * 1 <= cols <= HEC_MAX_DATA_UNITS.  Synchronous, thread-safe, no device. */
int hec_gf_matmul_host(const uint8_t *matrix, size_t rows, size_t cols, const uint8_t *const *in, uint8_t *const *out,
                       size_t len);
const char *hec_host_isa(void);

/* ---- Device-resident batched API (asynchronous, on hip_stream) --------- *
 * A batch is `stripes` independent stripes of cell_len-byte cells.  Shard i
 * of stripe s lives at  base[i] + s * stride[i]  (device pointers).  For the
 * [stripe][shard][cell] layout pass base[i] = buf + i*cell_len and
 * stride[i] = units*cell_len.  The fast path needs every base and stride
 * 16-byte aligned; other layouts run a byte-granular kernel (same results). */

/* Batched Coder::encode: parity[j] = sum_i C[k+j][i] * data[i]. */
int hec_encode_device(hec_coder_t *coder, const uint8_t *const *d_data, const size_t *data_strides,
                      uint8_t *const *d_parity, const size_t *parity_strides, size_t cell_len,
                      size_t stripes, void *hip_stream);

/* Batched Coder::decode with one erasure pattern for the whole batch.
 * d_shards[k+m] (NULL = missing) with shard_strides[k+m]; d_out[k] with
 * out_strides[k], used only for missing data indices.  The decode matrix is
 * computed on the host once per pattern and cached in the coder. */
int hec_decode_device(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                      uint8_t *const *d_out, const size_t *out_strides, size_t cell_len,
                      size_t stripes, void *hip_stream);

/* Batched Coder::decode where every stripe has its OWN erasure pattern, as a
 * striped read over many block groups sees (ec/mod.rs:71 decodes row by
 * row).  d_shards[k+m]/shard_strides[k+m]: storage of every shard index
 * (never NULL; slots a stripe lacks are not read).  present[stripes] (host):
 * bit i set = shard i of that stripe is available.  Reconstructed data shard
 * i of stripe s goes to d_out[i] + s*out_strides[i], only where it is
 * missing.  One plan per distinct pattern (first-k-present survivors, as
 * gf256.rs:84-126) is built on the host, cached in the coder and uploaded to
 * d_workspace (hec_decode_mixed_workspace_size bytes; keep it untouched
 * until the stream reaches the work: the launch also keeps its tile-queue
 * counters there, so calls in flight on different streams need different
 * workspaces).  If any stripe lacks data shards and
 * has fewer than k present, HEC_ERR_NOT_ENOUGH_SHARDS is returned and
 * nothing is launched. */
size_t hec_decode_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);
int hec_decode_device_mixed(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                            uint8_t *const *d_out, const size_t *out_strides, const uint64_t *present,
                            size_t cell_len, size_t stripes, void *d_workspace, size_t workspace_bytes,
                            void *hip_stream);

/* ---- Reconstruction: any lost unit of a stripe, parity included --------- *
 * What block-group repair needs (Hadoop RSRawDecoder.decode(inputs,
 * erasedIndexes, outputs)): when a DataNode dies, each block group it held
 * loses a different unit index, about m/(k+m) of them parity units.  The
 * reference's reader never rebuilds parity (gf256.rs:96-97), so these calls
 * have no counterpart there; the decode calls above are unchanged.
 * Survivors are the first k present units in index order, as hec_decode.  A
 * lost data unit t is rebuilt with row t of inverse(select_rows(C, survivors)),
 * a lost parity unit k+j with row  C[k+j] . inverse(select_rows(C, survivors)).
 * `want` (where taken) narrows the work to some of the lost units. */

/* The plan for a presence mask (host only, no device).  codec as
 * hec_coder_create_codec (NULL = "rs"); k+m <= 64.  present[k+m]: non-zero =
 * unit available.  want[k+m]: non-zero = rebuild this unit; NULL = every
 * missing unit; a want entry set on a present unit -> HEC_ERR_INVALID_ARG.
 * On HEC_OK:
 *   *n_targets   = t, the number of units to rebuild (0 => nothing to do, also
 *                  when fewer than k units are present);
 *   survivors[k] = the first k present unit indices, ascending;
 *   targets[t]   = the units to rebuild, ascending (t <= m);
 *   matrix[t*k]  = their rows over the survivors, row-major; for data units
 *                  byte-identical to hec_decode_plan's.
 * HEC_ERR_NOT_ENOUGH_SHARDS when t > 0 and fewer than k units are present
 * (*n_targets is still set; nothing else is written). */
int hec_reconstruct_plan(const char *codec, size_t data_units, size_t parity_units,
                         const uint8_t *present, const uint8_t *want,
                         size_t *n_targets, size_t *survivors, size_t *targets, uint8_t *matrix);

/* Host drop-in (synchronous).  shards[k+m] host buffers of shard_len bytes,
 * NULL = missing; want[k+m] as above (NULL = every missing unit).  out[k+m]:
 * for every target t, out[t] points to shard_len writable bytes and receives
 * the rebuilt unit (NULL there -> HEC_ERR_INVALID_ARG); the other entries are
 * never read or written.  Routed like hec_decode (hec_coder_set_host_limit;
 * a host-only coder always runs the host routine).  Any shard_len >= 1.
 * HEC_OK without writing when there is no target, HEC_ERR_NOT_ENOUGH_SHARDS
 * (nothing written) with a target and fewer than k units present. */
int hec_reconstruct(hec_coder_t *coder, const uint8_t *const *shards, size_t shard_len,
                    const uint8_t *want, uint8_t *const *out);

/* Device-resident batch with one pattern for the whole batch (asynchronous
 * on hip_stream).  d_shards[k+m] (NULL = missing) with shard_strides[k+m];
 * d_out[k+m] with out_strides[k+m], used only at target indices.  d_out[t]
 * may be the lost unit's own storage slot (repair in place); a NULL d_out at
 * a target -> HEC_ERR_INVALID_ARG, nothing launched.  Four rows per launch.  With every data unit present and all m parity units the targets,
 * the rows are the coding matrix's parity rows and the call runs the encode
 * kernels: the same bytes as hec_encode_device. */
int hec_reconstruct_device(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                           uint8_t *const *d_out, const size_t *out_strides, const uint8_t *want,
                           size_t cell_len, size_t stripes, void *hip_stream);

/* Device-resident batch where every stripe has its OWN pattern: the shape of
 * a repair batch after a node failure.  d_shards[k+m] / shard_strides[k+m]:
 * storage of every unit index (never NULL; slots a stripe lacks are not
 * read).  present[stripes] (host): bit i set = unit i of that stripe is
 * available.  want[stripes] (host): bit t set = rebuild unit t of that stripe;
 * NULL = everything the stripe lacks; a bit on a present unit ->
 * HEC_ERR_INVALID_ARG.  Rebuilt unit t of stripe s goes to d_out[t] +
 * s*out_strides[t]; d_out[t] is needed only for units that are a target in
 * some stripe and may alias d_shards[t].  One plan per distinct (present,
 * want) pair is uploaded to d_workspace (hec_reconstruct_mixed_workspace_size
 * bytes; keep it untouched until the stream reaches the work: the launch
 * keeps its tile counters there, so calls in flight at once need different
 * workspaces).  One kernel per 4 target rows for k in {2,3,6,10} with 16-B
 * aligned bases, strides and cell_len and plans that fit the kernel's LDS;
 * other shapes run one hec_reconstruct_device-style launch per run of
 * consecutive stripes sharing a plan (same results) and never touch the
 * workspace, which may then be NULL; its size is bounded by what the kernel's
 * LDS can hold, whatever the stripe count.  If any stripe has a
 * target and fewer than k units present, HEC_ERR_NOT_ENOUGH_SHARDS is
 * returned and nothing is launched. */
size_t hec_reconstruct_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);
int hec_reconstruct_device_mixed(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                                 uint8_t *const *d_out, const size_t *out_strides,
                                 const uint64_t *present, const uint64_t *want,
                                 size_t cell_len, size_t stripes, void *d_workspace, size_t workspace_bytes,
                                 void *hip_stream);

/* Verified reconstruction: the two device calls above with the chunk
 * checksums that surround a repair worker's bytes, in the same pass over the
 * cells.  The k survivors arrive from DataNodes with one sum per
 * bytes_per_checksum chunk and are verified before anything is trusted that
 * was rebuilt from them (HDFS-15759); the rebuilt units leave as packets that
 * need fresh chunk sums (WritePacket::calculate_checksum,
 * connection.rs:568-584).  Shards, outputs, want, present, survivors (the
 * first k present units), plans, in-place repair (d_out[t] may be the lost
 * slot) and status codes are exactly those of hec_reconstruct_device /
 * hec_reconstruct_device_mixed.
 *   d_sums, d_expected: [stripe][k+m][nck] big-endian u32, nck =
 *     ceil(cell_len / bytes_per_checksum); d_bad: [stripe][k+m] bytes -- the
 *     layouts of hec_encode_crc_device / hec_decode_verify_device; the sums
 *     buffers 4-byte aligned.
 *   d_sums (required) receives the chunk sums of every rebuilt unit at that
 *     unit's own slot; no other word of it is written.
 *   d_expected (optional; requires d_bad): the k survivors a stripe's plan
 *     reads are verified against it; a mismatch sets d_bad[s*(k+m) + unit] =
 *     1.  Flags are only ever set: the caller zeroes them, as for
 *     hec_checksum_verify_device.  Present units the plan does not read are
 *     not verified.  d_expected == d_sums is allowed (survivor slots are read,
 *     target slots written, and they are disjoint): a worker keeps one sums
 *     array per batch and the call fills in the holes.
 * Both calls are asynchronous on hip_stream: they never synchronise with the
 * device, never allocate device memory and never read the flags back.  A
 * stripe with a flagged survivor still gets its targets and their sums
 * written, with unspecified content: the caller reads d_bad, clears those
 * bits in `present`, may add the bad unit to `want`, and calls the mixed form
 * again for those stripes (want = 0 for every other stripe).
 * HEC_CHECKSUM_NULL runs the plain reconstruct call and ignores the three
 * checksum buffers; HEC_CHECKSUM_CRC32C and HEC_CHECKSUM_CRC32 are supported.
 * HEC_ERR_DEVICE on a host-only coder.  HEC_ERR_INVALID_ARG, nothing queued:
 * NULL coder, cell_len == 0, bytes_per_checksum == 0, NULL or misaligned
 * d_sums, d_expected without d_bad.  HEC_OK, nothing queued: stripes == 0 or
 * no target anywhere.
 * One fused kernel (reads k cells, writes t cells and their sums) for k in
 * {2,3,6,10}, at most 4 target rows per pattern, bytes_per_checksum == 512 and
 * 16-B aligned bases, strides and cell_len; everything else runs, in stream
 * order, a verify pass over the survivors (with d_expected), the plain
 * reconstruct call and a checksum pass over the rebuilt units read back from
 * d_out: the same results.
 * The mixed form takes one launch per distinct (present, want) pair, each
 * over a device list of that pair's stripes -- at most k+m launches after one
 * node failure.  The lists sit in d_workspace behind what
 * hec_reconstruct_device_mixed keeps there
 * (hec_reconstruct_crc_mixed_workspace_size bytes, 4-byte aligned, always
 * required; untouched until the stream reaches the work; calls in flight at
 * once need different workspaces). */
int hec_reconstruct_crc_device(hec_coder_t *coder, int checksum_type,
                               const uint8_t *const *d_shards, const size_t *shard_strides,
                               uint8_t *const *d_out, const size_t *out_strides, const uint8_t *want,
                               size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                               const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums, void *hip_stream);

size_t hec_reconstruct_crc_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);
int hec_reconstruct_crc_device_mixed(hec_coder_t *coder, int checksum_type,
                                     const uint8_t *const *d_shards, const size_t *shard_strides,
                                     uint8_t *const *d_out, const size_t *out_strides,
                                     const uint64_t *present, const uint64_t *want,
                                     size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                     const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums,
                                     void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Checksum-only reconstruction: the chunk sums of lost units, computed from
 * the survivors, with nothing rebuilt written to memory -- what
 * StripedBlockChecksumReconstructor does for the block (group) checksum of a
 * degraded group (HDFS-9833; COMPOSITE_CRC: HDFS-13056).  The two calls above
 * with d_out / out_strides removed: survivors (the first k present units),
 * plans, want, the layout and alignment of d_sums / d_expected / d_bad,
 * d_expected == d_sums, flags only ever set, asynchronous (no
 * synchronisation, no allocation, no read-back), HEC_ERR_NOT_ENOUGH_SHARDS
 * with nothing queued and HEC_ERR_DEVICE on a host-only coder are theirs.
 * What differs:
 *   Read-only over the cells: no byte of any unit slot is written, lost slots
 *     included.  Only the sums words of the target units' live chunks are
 *     written, plus d_bad on a mismatch.
 *   HEC_CHECKSUM_NULL is HEC_ERR_INVALID_ARG (nothing to compute, as for
 *     hec_checksum_device).
 *   data_len (uniform form) has the meaning and the range check of
 *     hec_composite_crc: 0 = every stripe full; otherwise the last stripe
 *     holds r = data_len - (stripes-1)*k*cell_len logical bytes, n0 =
 *     min(cell_len, r), and unit u has len(u) bytes there (data unit u: what
 *     is left of r past u*cell_len, at most cell_len; parity: n0).  In that
 *     stripe each present unit's slot holds its len(u) bytes followed by zeros
 *     up to n0 (CellReader::next_cell's padding); nothing at or past n0 is
 *     read from any slot.  A rebuilt unit t is computed over [0, n0); its sums
 *     are written for chunks c < ceil(len(t) / bytes_per_checksum), the last
 *     one over [c*bpc, len(t)); the slots past that -- all of them when len(t)
 *     == 0 -- are not written.  With d_expected a survivor is verified over
 *     its own len(u) bytes; a present unit of length 0 contributes zeros and
 *     none of its sums words is read.  These are the sums hec_composite_crc*
 *     expects, so a degraded group's block and group CRCs are this call and
 *     hec_composite_crc_device with the same data_len on one stream.
 *   Mixed form: full stripes only (a batch spans groups).  d_shards[i] may be
 *     NULL if no stripe's `present` has bit i -- the dead node's unit, for
 *     which the caller has no storage; a NULL slot some stripe has present is
 *     HEC_ERR_INVALID_ARG with nothing queued.  The workspace is the one of
 *     hec_reconstruct_crc_device_mixed (hec_reconstruct_crc_mixed_workspace_size,
 *     same rules); it holds the stripe lists.  One launch per distinct
 *     (present, want) pair; stripes without a target are skipped.
 * HEC_ERR_INVALID_ARG, nothing queued: NULL coder, HEC_CHECKSUM_NULL or an
 * unknown type, cell_len == 0, bytes_per_checksum == 0, NULL or misaligned
 * d_sums, d_expected without d_bad, data_len out of range, a workspace that is
 * too small, NULL or misaligned.  HEC_OK, nothing queued: stripes == 0 or no
 * target anywhere.
 * Full stripes run the kernel of hec_reconstruct_crc_device without its
 * output stores (reads k cells, writes the sums) for k in {2,3,6,10}, at most
 * 4 target rows per pattern, bytes_per_checksum == 512 and 16-B aligned
 * survivor bases, strides and cell_len.  Every other shape, and the short last
 * stripe, runs a byte-wise kernel (one lane per stripe, target and chunk)
 * behind a verify pass over the survivors: the same results.  The uniform
 * form queues kernels only and can be captured into a graph. */
int hec_reconstruct_sums_device(hec_coder_t *coder, int checksum_type,
                                const uint8_t *const *d_shards, const size_t *shard_strides,
                                const uint8_t *want, size_t cell_len, size_t stripes,
                                size_t bytes_per_checksum, uint64_t data_len,
                                const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums, void *hip_stream);

int hec_reconstruct_sums_device_mixed(hec_coder_t *coder, int checksum_type,
                                      const uint8_t *const *d_shards, const size_t *shard_strides,
                                      const uint64_t *present, const uint64_t *want,
                                      size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                      const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums,
                                      void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* ---- Verified reconstruction of short stripes ------------------------------ *
 * hec_reconstruct_crc_device / _mixed for stripes that hold fewer than
 * k * cell_len logical bytes: the last stripe of a block group (data_len, the
 * uniform form) or any stripe of a batch that spans groups or small files
 * (stripe_bytes, the mixed form).  Shards, outputs, want, present, the
 * survivors (the first k present units, whatever their length), plans,
 * in-place repair, the [stripe][k+m][nck] layout of d_sums / d_expected with
 * nck = ceil(cell_len / bytes_per_checksum), the [stripe][k+m] layout of d_bad,
 * d_expected == d_sums, flags only ever set, asynchronous (no synchronisation,
 * no allocation, no read-back), HEC_ERR_NOT_ENOUGH_SHARDS with nothing queued
 * and HEC_ERR_DEVICE on a host-only coder are theirs.
 *
 * A stripe of r logical bytes, 1 <= r <= k*cell_len, has n0 = min(cell_len, r),
 * data unit u < k of len(u) = min(cell_len, max(0, r - u*cell_len)) bytes and
 * every parity unit of n0 bytes (the geometry of hec_composite_crc and
 * hec_reconstruct_sums_device).
 *   data_len (uniform form) has the meaning and the range check of
 *     hec_composite_crc: 0 = every stripe full; otherwise only the last stripe
 *     is short, r = data_len - (stripes-1)*k*cell_len.
 *   stripe_bytes[stripes] (mixed form, host array, NULL = every stripe full):
 *     an entry of 0 or k*cell_len says the stripe is full, any other entry is
 *     the stripe's r; an entry above k*cell_len is HEC_ERR_INVALID_ARG.
 * In a short stripe:
 *   A present unit counts as zero from len(u) on: no slot byte at or past
 *     len(u) influences any output, a present unit of length 0 is not read at
 *     all and none of its sums words is read.  Nothing at or past cell_len of a
 *     slot is read; on the 16-B aligned route a read may reach the end of the
 *     16-byte block that holds byte n0-1, and no further.
 *   With d_expected each survivor the plan reads is verified over its own
 *     len(u) bytes: chunks c < ceil(len(u) / bytes_per_checksum), the last one
 *     short; sums slots past that are not read.
 *   A rebuilt unit t gets its len(t) computed bytes at [0, len(t)) and zeros at
 *     [len(t), n0): the slot is what CellReader::next_cell hands out, and
 *     hec_scrub_device with cell_len = n0 on that stripe sees a consistent
 *     stripe.  No byte at or past n0 of any slot is written.
 *   The sums of t are written for chunks c < ceil(len(t) / bytes_per_checksum),
 *     the last over [c*bpc, len(t)); the slots past that -- all of them when
 *     len(t) == 0 -- are not written.  These are the sums hec_composite_crc*
 *     expects: a repaired group's block and group CRCs are this call and
 *     hec_composite_crc_device with the same data_len, on one stream and one
 *     sums array.
 *   A stripe with a flagged survivor gets unspecified content in its targets'
 *     [0, n0) and in their live sums words; everything else holds.
 * HEC_CHECKSUM_NULL is HEC_ERR_INVALID_ARG: without sums a short stripe needs
 * no call of its own, because zero-padded slots through
 * hec_reconstruct_device[_mixed] give the same bytes.  The other
 * HEC_ERR_INVALID_ARG cases (nothing queued) are those of
 * hec_reconstruct_crc_device[_mixed], plus data_len out of range and a
 * stripe_bytes entry out of range; the coder, the checksum type, cell_len,
 * bytes_per_checksum, data_len and stripe_bytes are checked before the coder's
 * device.  HEC_OK, nothing queued: stripes == 0 or no target anywhere.
 * Full stripes make exactly the launches of hec_reconstruct_crc_device[_mixed]
 * (with data_len == 0 / stripe_bytes == NULL every output byte is theirs).
 * Short stripes run a one-pass kernel (k reads, t writes and their sums over
 * [0, n0)) for k in {2,3,6,10}, at most 4 target rows per pattern,
 * bytes_per_checksum == 512 and 16-B aligned bases, strides and cell_len -- the
 * lengths themselves may be any byte count -- and a byte-wise kernel with the
 * same results for every other shape.  Uniform form: one launch over the
 * stripes-1 full stripes, one over the last; kernels only, capturable into a
 * graph.  Mixed form: per distinct (present, want) pair one launch over its
 * full stripes and one over its short stripes.  Its workspace
 * (hec_reconstruct_crc_rows_mixed_workspace_size, never smaller than
 * hec_reconstruct_crc_mixed_workspace_size) is always required, 8-byte
 * aligned, and holds the short stripes' lists and lengths behind what
 * hec_reconstruct_crc_device_mixed keeps there; it stays untouched until the
 * stream reaches the work, and calls in flight at once need different
 * workspaces. */
int hec_reconstruct_crc_rows_device(hec_coder_t *coder, int checksum_type,
                                    const uint8_t *const *d_shards, const size_t *shard_strides,
                                    uint8_t *const *d_out, const size_t *out_strides, const uint8_t *want,
                                    size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint64_t data_len,
                                    const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums, void *hip_stream);

size_t hec_reconstruct_crc_rows_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);

int hec_reconstruct_crc_rows_device_mixed(hec_coder_t *coder, int checksum_type,
                                          const uint8_t *const *d_shards, const size_t *shard_strides,
                                          uint8_t *const *d_out, const size_t *out_strides,
                                          const uint64_t *present, const uint64_t *want, const uint64_t *stripe_bytes,
                                          size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                          const uint8_t *d_expected, uint8_t *d_bad, uint8_t *d_sums,
                                          void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* ---- Scrub: verify a stripe's parity and locate a corrupt unit ----------- *
 * What a block scanner or a repair worker asks before and after it rebuilds
 * (`hdfs debug verifyEC`; dfs.datanode.ec.reconstruct.validation, HDFS-15759):
 * are the k+m units of a stripe still consistent, and if not, which one is
 * wrong?  The reference's reader trusts the packet checksums
 * (connection.rs:477-504) and has no counterpart.  hec_scrub and
 * hec_scrub_device take stripes whose k+m units are all present; a stripe with
 * missing units (a dead DataNode) is scrubbed by hec_scrub_degraded and
 * hec_scrub_device_mixed, defined after them.
 *
 * With C the coder's (k+m) x k matrix (hec_gen_codec_matrix), P = C[k:] and
 * H = [P | I_m] (column t of H is P[:,t] for a data unit t < k and the unit
 * vector e_j for parity unit k+j), the syndrome of byte position b is
 *   s_j(b) = sum_i P[j][i] * u_i(b)  ^  u_{k+j}(b),   j < m.
 * Per stripe a scrub returns
 *   bad_bytes = the number of positions b < cell_len with some s_j(b) != 0;
 *   ruled_out = bit t (t < k+m) set iff some position's syndrome vector is not
 *               a GF(2^8) multiple of column t of H (some 2x2 minor
 *               s_i(b)*H[j][t] ^ s_j(b)*H[i][t] is non-zero).  Bits >= k+m are
 *               0; with m == 1 no bit is ever set (one parity cannot locate);
 *               a clean stripe gives (0, 0).
 * hec_scrub_verdict (host only) turns the pair into
 *   HEC_SCRUB_CLEAN     bad_bytes == 0;
 *   HEC_SCRUB_LOCATED   exactly one unit of 0..units-1 is not ruled out;
 *                       *unit (if not NULL) receives it -- written in no other case;
 *   HEC_SCRUB_MULTIPLE  every unit is ruled out: more than one unit is corrupt;
 *   HEC_SCRUB_AMBIGUOUS anything else (m == 1, or several candidates left);
 * units == 0 or > 64 -> HEC_ERR_INVALID_ARG.
 * What a verdict proves: one corrupt unit t leaves every syndrome vector a
 * multiple of column t, so it is never ruled out, and every other unit is
 * ruled out at each bad position (any two columns of H are independent for
 * m >= 2).  Explaining by a single unit a position where several units are
 * wrong needs an error of weight >= m there (every m columns of H are
 * independent: the codes are MDS), so with m >= 3 two corrupt units can never
 * pass for one and LOCATED is exact for up to m-1 corrupt units; with m == 2,
 * LOCATED assumes at most one corrupt unit.  CLEAN misses only corruption
 * that is itself a codeword (>= m+1 units wrong at a position, consistently).
 * The recipe for a repair worker -- scrub, turn each LOCATED unit into a
 * `present` mask, hec_reconstruct_device_mixed in place, scrub again -- is in
 * INTEGRATION.md. */
typedef struct {
    uint64_t ruled_out;
    uint64_t bad_bytes;
} hec_scrub_result_t;

#define HEC_SCRUB_CLEAN 0
#define HEC_SCRUB_LOCATED 1
#define HEC_SCRUB_AMBIGUOUS 2
#define HEC_SCRUB_MULTIPLE 3

int hec_scrub_verdict(uint64_t ruled_out, uint64_t bad_bytes, size_t units, int *unit);

/* Host drop-in (synchronous).  shards[k+m] host buffers of shard_len bytes,
 * none NULL; any shard_len >= 1.  Always the engine's host routine, whatever
 * the host limit (the answer is 16 bytes; a pageable row never pays for PCIe)
 * and on host-only coders: syndromes in blocks of 64 KiB per unit with the
 * AVX-512+GFNI / AVX2 / scalar multiply, a scalar locate over the non-zero
 * positions only, no allocation that grows with shard_len.  HEC_ERR_INVALID_ARG
 * for a NULL shard, shard_len == 0 or NULL out. */
int hec_scrub(hec_coder_t *coder, const uint8_t *const *shards, size_t shard_len, hec_scrub_result_t *out);

/* Device-resident batch (asynchronous on hip_stream), units laid out as for
 * hec_encode_device: d_shards[k+m] / shard_strides[k+m], none NULL.  Read-only
 * over the k+m cells of every stripe -- the bytes hec_encode_device moves --
 * with no scratch.  d_results[stripes] (device memory, 8-byte aligned) is
 * zeroed by the call itself (one hipMemsetAsync on the stream; a zeroing kernel
 * node under stream capture) and then receives each stripe's pair; clean stripes
 * cost no write.  k in {2,3,6,10} with m <= 4 and 16-B aligned bases, strides
 * and cell_len run the register kernel (a sibling of the encode kernel); other
 * shapes a byte-granular kernel with the same results.  stripes == 0 ->
 * HEC_OK, nothing queued.  HEC_ERR_INVALID_ARG (nothing queued) for a NULL
 * unit, cell_len == 0, NULL or misaligned d_results; HEC_ERR_DEVICE on a
 * host-only coder. */
int hec_scrub_device(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                     size_t cell_len, size_t stripes, hec_scrub_result_t *d_results, void *hip_stream);

/* Scrub correction: fix the unit a scrub LOCATED, in place, from the scrub's
 * own result -- no inverse, no plan, no workspace, no host round trip.  One
 * corrupt unit t with error e(b) leaves s_j(b) = H[j][t] * e(b) in every row,
 * so the error is one syndrome divided by one constant:
 *   e(b) = scale[t] * s_row[t](b),
 *   data unit t:     row[t] = the first j with P[j][t] != 0, scale[t] = 1 / P[j][t];
 *   parity unit k+j0: row = j0, scale = 1 (the cell is overwritten by row j0
 *                     of the encode).
 * The verdict is formed exactly as hec_scrub_verdict(ruled_out, bad_bytes,
 * k+m, &t) does: cand = ~ruled_out & ((1 << (k+m)) - 1); the stripe is LOCATED
 * iff bad_bytes != 0 and popcount(cand) == 1, and then t = ctz(cand).
 *   CLEAN (bad_bytes == 0):   unit = HEC_CORRECT_CLEAN; no cell is read or written;
 *   AMBIGUOUS or MULTIPLE (always so for m == 1):
 *                             unit = HEC_CORRECT_UNLOCATED; nothing is written;
 *   LOCATED unit t:           unit = t and u_t(b) ^= e(b) for every b < cell_len.
 * Only unit t's cell is written: bytes of it with e(b) == 0 keep their value
 * (whether or not they are stored again), no byte outside [0, cell_len) of
 * that cell changes, the other units are read-only.  One corrupt unit, with
 * m >= 2, comes back bit-exact.  What the verdict proves carries over from
 * hec_scrub_verdict word for word: with m >= 3, LOCATED is exact for up to m-1
 * corrupt units; with m == 2, LOCATED assumes at most one corrupt unit (two
 * corrupt units that pass for one are "corrected" to a consistent but wrong
 * stripe; chunk sums, hec_scrub_crc_device, tell).
 *
 * Out of scope: a _mixed form for degraded stripes (a stripe with missing
 * units goes through hec_reconstruct_device_mixed); a form that understands
 * the stripe lengths of the _rows scrubs; chunk sums -- the call does not
 * touch them: a unit whose bytes were wrong and whose sums were right verifies
 * again after the fix, which a second hec_scrub_crc_device shows.
 *
 * hec_scrub_correct (host, synchronous): runs the host routine of hec_scrub
 * over shards[k+m] (writable host buffers of shard_len bytes, none NULL),
 * stores the pair it found in *out if out is not NULL, and on LOCATED corrects
 * in place.  *unit receives t, HEC_CORRECT_CLEAN or HEC_CORRECT_UNLOCATED.
 * Always the host routine, also on host-only coders; no allocation grows with
 * shard_len.  HEC_ERR_INVALID_ARG for a NULL coder, shards, shard or unit, or
 * shard_len == 0.
 *
 * hec_scrub_correct_device (asynchronous on hip_stream), units laid out as for
 * hec_scrub_device.  The caller's contract: d_results[stripes] is what
 * hec_scrub_device or hec_scrub_crc_device wrote for these very cells (same
 * d_shards, strides, cell_len and stripes), earlier on the same stream, with
 * no write to the cells in between.  d_results is read on the device and is
 * read-only; d_units[stripes] (device memory, 4-byte aligned) is written for
 * every stripe by the call itself (no memset is queued; the caller need not
 * initialise it).  The call reads the k data cells and one parity cell of the
 * LOCATED stripes only.  It does not synchronise, does not allocate, takes no
 * workspace and leases no queue counters; under stream capture it is one kernel
 * node, so scrub -> correct -> scrub runs on one stream or in one graph with
 * one read-back of d_units and the final results ("Scrub,
 * correct, scrub"; stripes left at HEC_CORRECT_UNLOCATED go through the
 * reconstruct loop).  k in {2,3,6,10} with m <= 4 and 16-B aligned bases,
 * strides and cell_len run the register kernel; other shapes a byte-granular
 * kernel with the same results.  stripes == 0 -> HEC_OK, nothing queued.
 * HEC_ERR_INVALID_ARG (nothing queued) for a NULL coder, d_shards,
 * shard_strides, d_results or d_units, a NULL d_shards[i], cell_len == 0,
 * d_results not 8-byte aligned or d_units not 4-byte aligned; HEC_ERR_DEVICE
 * on a host-only coder. */
#define HEC_CORRECT_CLEAN (-1)     /* bad_bytes == 0: stripe untouched */
#define HEC_CORRECT_UNLOCATED (-2) /* AMBIGUOUS or MULTIPLE: stripe untouched */

int hec_scrub_correct(hec_coder_t *coder, uint8_t *const *shards, size_t shard_len,
                      hec_scrub_result_t *out /* may be NULL */, int *unit);
int hec_scrub_correct_device(hec_coder_t *coder, uint8_t *const *d_shards, const size_t *shard_strides,
                             size_t cell_len, size_t stripes, const hec_scrub_result_t *d_results,
                             int32_t *d_units, void *hip_stream);

/* Degraded scrub: a stripe with missing units.  Of its p present units, S is
 * the first k in ascending order (the survivors every reconstruction call
 * picks), E the other e = p - k (the extras, ascending), 0 <= e <= m.  With
 *   G = C[E] . inverse(select_rows(C, S))            (e x k)
 * -- the rows hec_reconstruct_plan returns for present = S only, want = E --
 * the syndrome of byte position b is
 *   s_j(b) = sum_i G[j][i] * u_{S_i}(b)  ^  u_{E_j}(b),   j < e,
 * and the parity-check matrix H' has one column per present unit: G[:, i] for
 * survivor S_i, the unit vector e_j for extra E_j.  With every unit present
 * S = 0..k-1, E = the parity units and G = P: the scrub above.  Per stripe
 *   bad_bytes = the number of positions with a non-zero syndrome vector;
 *   ruled_out = bit t set for a present unit t iff some position's vector is
 *               not a multiple of t's column of H' (2x2 minors, as above).
 *   Missing units: when bad_bytes != 0 the bit of every missing unit is set
 *               too -- a missing unit is never the culprit -- so
 *               hec_scrub_verdict(ruled_out, bad_bytes, k+m, &unit) works
 *               unchanged.  A clean stripe gives (0, 0).
 *   Unchecked stripes: e == 0 (exactly k units present, or fewer) leaves
 *               nothing to check against.  Such a stripe gives (0, 0), nothing
 *               of it is read and the call does not fail: one unrecoverable
 *               group must not fail a scanner's batch.  The caller knows e
 *               from its own mask (hec_scrub_plan returns it).
 * With e == 1 nothing can be located (AMBIGUOUS, as m == 1 above); what a
 * verdict proves is what is said above with e in the place of m.
 *
 * hec_scrub_plan (host only): the check plan of a presence mask present[k+m].
 * *n_checks = e; for e >= 1 survivors[k], extras[e] and matrix[e*k] (G,
 * row-major) are filled where not NULL; for e == 0 nothing else is written.
 * Codec names and their errors as hec_reconstruct_plan. */
int hec_scrub_plan(const char *codec, size_t data_units, size_t parity_units, const uint8_t *present,
                   size_t *n_checks, size_t *survivors, size_t *extras, uint8_t *matrix);

/* Host drop-in (synchronous): shards[k+m] host buffers of shard_len bytes,
 * NULL = missing (never read).  Always the host routine of hec_scrub, over
 * the stripe's [S..., E...] with G; no allocation that grows with shard_len;
 * works on host-only coders.  With no NULL the result is hec_scrub's.
 * HEC_ERR_INVALID_ARG for a NULL coder, shards or out, or shard_len == 0. */
int hec_scrub_degraded(hec_coder_t *coder, const uint8_t *const *shards, size_t shard_len,
                       hec_scrub_result_t *out);

/* Device-resident batch with one presence mask per stripe (asynchronous on
 * hip_stream), following hec_reconstruct_device_mixed: d_shards[k+m] /
 * shard_strides[k+m], none NULL (the slots a stripe lacks are not read);
 * present[stripes] host array, bit i = unit i present.  One plan per distinct
 * mask is built on the host and cached in the coder; the plans and the launch
 * counters sit in d_workspace (hec_scrub_mixed_workspace_size(coder, stripes)
 * bytes of device memory, 16-byte aligned, required whenever a stripe can be
 * checked), which must stay untouched until the stream reaches the work;
 * calls in flight at once need different workspaces.  As hec_scrub_device:
 * d_results[stripes] (8-byte aligned) is zeroed by the call itself on the
 * stream and then receives each stripe's pair; the pass is read-only over the
 * present units and clean stripes cost no write.
 * k in {2,3,6,10}, at most 4 extras in any stripe and 16-B aligned bases,
 * strides and cell_len run one register kernel with the plans resident in LDS;
 * a batch whose plans do not fit (RS(10,4) with hundreds of distinct masks)
 * runs that kernel once per run of consecutive stripes sharing a mask; other
 * shapes a byte-granular kernel.  The results are the same.
 * HEC_OK for stripes == 0 (nothing queued) and for a batch with no checkable
 * stripe (the results are still zeroed).  HEC_ERR_INVALID_ARG, nothing
 * queued: NULL coder, d_shards, shard_strides, present or d_results, a NULL
 * d_shards[i], cell_len == 0, misaligned d_results, and -- when a stripe can
 * be checked -- a NULL, misaligned or too small workspace.  HEC_ERR_DEVICE on
 * a host-only coder.  Capturing the call into a HIP graph is not supported. */
size_t hec_scrub_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);
int hec_scrub_device_mixed(hec_coder_t *coder, const uint8_t *const *d_shards, const size_t *shard_strides,
                           const uint64_t *present, size_t cell_len, size_t stripes,
                           hec_scrub_result_t *d_results, void *d_workspace, size_t workspace_bytes,
                           void *hip_stream);

/* Verified scrub: the two device calls above with the chunk checksums of every
 * present unit verified in the same pass over the cells.  A block scanner
 * exists to verify chunk sums, and the parity check exists to catch what sums
 * cannot -- a unit whose sums were computed from the wrong bytes (HDFS-15759)
 * -- so a scanner wants both answers for every stripe, and a repair worker
 * wants them for the units hec_reconstruct_crc_device_mixed has just rebuilt
 * and summed.  Shards, strides, present, survivors and extras, d_results, the
 * workspace rules and status codes are those of hec_scrub_device /
 * hec_scrub_device_mixed; the checksum buffers are those of
 * hec_reconstruct_crc_device:
 *   d_expected: [stripe][k+m][nck] big-endian u32, nck = ceil(cell_len /
 *     bytes_per_checksum), 4-byte aligned; d_bad: [stripe][k+m] bytes.  Both
 *     required with a checksum type other than HEC_CHECKSUM_NULL.
 *   Results: d_results[stripes] holds exactly what hec_scrub_device /
 *     hec_scrub_device_mixed return for the same cells and masks (missing-unit
 *     bits and the (0, 0) of unchecked stripes included), zeroed by the call
 *     itself on the stream (a zeroing kernel node under capture);
 *     hec_scrub_verdict works unchanged.
 *   Flags: every present unit of every stripe is verified against its
 *     expected sums -- also in stripes with e == 0 (exactly k units present,
 *     or fewer), whose parity result is (0, 0) but whose sums still have
 *     something to check against.  A mismatch sets d_bad[s*(k+m) + unit] = 1;
 *     flags are only ever set: the caller zeroes them, as for
 *     hec_checksum_verify_device, whose flags over the present units these
 *     are.  The cells and sums slots of missing units are never read.
 *   The two outputs are independent of each other, and neither call writes to
 *   the cells or to d_expected.  A flag does not always mean bad bytes: when
 *   the sum itself is corrupt the parity verdict with the unit included is
 *   CLEAN, and the caller may re-sum the unit instead of rebuilding it.
 * Both calls are asynchronous on hip_stream: they never synchronise with the
 * device, never allocate device memory and never read the flags back.
 * HEC_CHECKSUM_NULL runs the plain scrub call and ignores the two checksum
 * buffers; HEC_CHECKSUM_CRC32C and HEC_CHECKSUM_CRC32 are supported.
 * HEC_ERR_DEVICE on a host-only coder.  HEC_ERR_INVALID_ARG, nothing queued:
 * NULL coder, d_shards, shard_strides, d_results or (mixed form) present, a
 * NULL d_shards[i], cell_len == 0, bytes_per_checksum == 0, misaligned
 * d_results or d_expected, an unknown checksum type, NULL d_expected or d_bad
 * with a checksum type other than NULL, and -- mixed form, when some stripe has
 * a present unit -- a NULL, misaligned (16 B) or too small workspace.  HEC_OK,
 * nothing queued: stripes == 0.
 * One fused kernel (reads the k+e present cells of a stripe once) for k in
 * {2,3,6,10}, 1 <= e <= 4 in every checked stripe, bytes_per_checksum == 512,
 * 16-B aligned bases, strides and cell_len and plans whose first row has no
 * zero; everything else runs, in stream order, a verify pass over the present
 * units and the plain scrub call: the same results.
 * hec_scrub_crc_device can be captured into a HIP graph on one stream (one
 * zeroing node plus one kernel node, like hec_reconstruct_crc_device).
 * The mixed form takes one launch per distinct presence mask, each over a
 * device list of that mask's stripes (a mask with e == 0 and a present unit
 * gets a sums-only launch): at most k+m+1 launches after one node failure, but
 * a batch of many distinct masks pays a launch each.  The lists sit in
 * d_workspace behind what hec_scrub_device_mixed keeps there
 * (hec_scrub_crc_mixed_workspace_size bytes, 16-byte aligned; untouched until
 * the stream reaches the work; calls in flight at once need different
 * workspaces).  Capturing the mixed form into a HIP graph is not supported. */
int hec_scrub_crc_device(hec_coder_t *coder, int checksum_type,
                         const uint8_t *const *d_shards, const size_t *shard_strides,
                         size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                         const uint8_t *d_expected, uint8_t *d_bad,
                         hec_scrub_result_t *d_results, void *hip_stream);

size_t hec_scrub_crc_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);
int hec_scrub_crc_device_mixed(hec_coder_t *coder, int checksum_type,
                               const uint8_t *const *d_shards, const size_t *shard_strides,
                               const uint64_t *present, size_t cell_len, size_t stripes,
                               size_t bytes_per_checksum,
                               const uint8_t *d_expected, uint8_t *d_bad,
                               hec_scrub_result_t *d_results, void *d_workspace, size_t workspace_bytes,
                               void *hip_stream);

/* ---- Verified scrub of short stripes -------------------------------------- *
 * hec_scrub_crc_device / hec_scrub_crc_device_mixed with the lengths of
 * hec_reconstruct_crc_rows_device[_mixed]: the last stripe of a block group
 * (data_len) or every stripe of a batch of small files (stripe_bytes) holds
 * r < k*cell_len logical bytes.  A short group is repaired and checked with
 * hec_reconstruct_crc_rows_device* -> hec_scrub_crc_rows_device* ->
 * hec_composite_crc_device on one stream and one sums array, without padding
 * by the caller and without per-stripe calls.  Everything not said here is
 * what hec_scrub_crc_device[_mixed] does: shards, masks, survivors S and extras
 * E, d_results zeroed by the call on the stream (a zeroing kernel node under
 * capture), missing-unit bits and the (0, 0) of unchecked stripes, flags that
 * are only ever set, read-only over the cells and d_expected, asynchronous,
 * no allocation, no read-back, HEC_ERR_DEVICE on a host-only coder.
 * Geometry: a stripe holds r logical bytes, 1 <= r <= k*cell_len; n0 =
 * min(cell_len, r); data unit u holds len(u) = min(cell_len, max(0, r -
 * u*cell_len)) bytes and every parity unit n0 bytes.
 *   data_len (uniform form) has the meaning and the range check of
 *     hec_composite_crc: 0 = every stripe full; otherwise only the last stripe
 *     is short.
 *   stripe_bytes[stripes] (mixed form, host array, NULL = every stripe full):
 *     an entry of 0 or k*cell_len says the stripe is full; an entry above
 *     k*cell_len is HEC_ERR_INVALID_ARG.
 *   d_expected stays [stripe][k+m][nck], nck = ceil(cell_len /
 *     bytes_per_checksum); d_bad stays [stripe][k+m].
 * In a short stripe:
 *   d_results[s] is exactly what hec_scrub_degraded returns for that stripe
 *     with shard_len = n0 when every present unit is its own len(u) bytes
 *     followed by zeros up to n0 -- what hec_scrub_device[_mixed] returns with
 *     cell_len = n0 on zero-padded slots.  Only positions b < n0 are checked or
 *     counted; a position at or past len(u) does not additionally rule u out.
 *   A present unit counts as zero from len(u) on: no slot byte at or past
 *     len(u) influences a result or a flag, a present unit of length 0 is not
 *     read at all and none of its sums words is read.  Nothing at or past
 *     cell_len of a slot is read; on the 16-B aligned route a read may reach the
 *     end of the 16-byte block that holds byte n0-1, and no further.
 *   Every present unit with len(u) > 0 is verified over its own bytes: chunks
 *     c < ceil(len(u) / bytes_per_checksum), the last one over [c*bpc, len(u));
 *     sums slots past that are not read.  Also in stripes with e == 0.
 * HEC_CHECKSUM_NULL is HEC_ERR_INVALID_ARG: zero-padded slots through
 * hec_scrub_device[_mixed] already give those results.  The other
 * HEC_ERR_INVALID_ARG cases (nothing queued) are those of
 * hec_scrub_crc_device[_mixed], plus data_len or a stripe_bytes entry out of
 * range; every argument is checked before the coder's device is touched.
 * Full stripes make exactly the launches of hec_scrub_crc_device[_mixed] (with
 * data_len == 0 / stripe_bytes == NULL every result, flag byte and launch is
 * theirs).  Short stripes run a one-pass kernel (k + e reads over [0, n0)) for
 * k in {2,3,6,10}, 1 <= e <= 4, bytes_per_checksum == 512, 16-B aligned bases,
 * strides and cell_len (below 2^31) and plans whose first row has no zero --
 * the lengths themselves may be any byte count -- and a byte-wise kernel with
 * the same results for every other shape and for groups with e == 0.
 * Uniform form: the existing call over the first stripes-1 stripes, then one
 * short-stripe launch with r passed by value; kernels only, capturable into a
 * graph.  Mixed form: per distinct mask one launch over its full stripes and
 * one over its short stripes.  Its workspace
 * (hec_scrub_crc_rows_mixed_workspace_size, never smaller than
 * hec_scrub_crc_mixed_workspace_size; required in full whenever a stripe is
 * short and some stripe has a present unit) holds the short stripes' lists and
 * their u64 lengths behind what hec_scrub_crc_device_mixed keeps there;
 * alignment and lifetime rules are that call's. */
int hec_scrub_crc_rows_device(hec_coder_t *coder, int checksum_type,
                              const uint8_t *const *d_shards, const size_t *shard_strides,
                              size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint64_t data_len,
                              const uint8_t *d_expected, uint8_t *d_bad,
                              hec_scrub_result_t *d_results, void *hip_stream);

size_t hec_scrub_crc_rows_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);

int hec_scrub_crc_rows_device_mixed(hec_coder_t *coder, int checksum_type,
                                    const uint8_t *const *d_shards, const size_t *shard_strides,
                                    const uint64_t *present, const uint64_t *stripe_bytes,
                                    size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                    const uint8_t *d_expected, uint8_t *d_bad,
                                    hec_scrub_result_t *d_results, void *d_workspace, size_t workspace_bytes,
                                    void *hip_stream);

/* ---- Encode with chunk sums of short stripes ------------------------------ *
 * The writer's side of the two families above (CellBuffer::encode feeding
 * WritePacket::calculate_checksum): hec_encode_crc_device with a checksum type
 * and with the geometry of hec_reconstruct_crc_rows_device[_mixed] /
 * hec_scrub_crc_rows_device[_mixed] -- a stripe of r logical bytes, 1 <= r <=
 * k*cell_len, n0 = min(cell_len, r), data unit u of len(u) = min(cell_len,
 * max(0, r - u*cell_len)) bytes, every parity unit of n0 bytes; data_len
 * (uniform form) with the meaning and the range check of hec_composite_crc;
 * stripe_bytes[stripes] (mixed form, host array, NULL = every stripe full) with
 * 0 or k*cell_len = full and an entry above k*cell_len HEC_ERR_INVALID_ARG.  A
 * group whose last stripe is short, or a batch of small files, goes write ->
 * scrub -> composite on one stream and one sums array
 * (hec_encode_crc_rows_device* -> hec_scrub_crc_rows_device* ->
 * hec_composite_crc_device), with no padding by the caller.
 * d_data[k] / d_parity[m] and their strides as hec_encode_crc_device; d_sums is
 * [stripe][k+m][nck] big-endian u32, nck = ceil(cell_len /
 * bytes_per_checksum), data unit i at i and parity unit j at k + j.
 * In a short stripe:
 *   A data unit counts as zero from len(u) on: no slot byte at or past len(u)
 *     influences any output.  A data unit of length 0 is not read at all and
 *     none of its sums words is written.  Nothing at or past cell_len of a slot
 *     is read; on the 16-B aligned route a read of a non-empty unit's slot may
 *     reach the end of the 16-byte block that holds byte n0-1, and no further.
 *     A file-order buffer (base d + i*cell_len, stride k*cell_len, as
 *     hec_encode_rows_device takes it) is therefore usable directly, without a
 *     workspace and without zero-padding: the allocation must cover whole rows,
 *     the bytes past data_len may be anything.
 *   Parity unit j gets its n0 computed bytes at [0, n0); no byte at or past n0
 *     of a parity slot is written.  This is the rule of
 *     hec_reconstruct_crc_rows_device, not that of hec_encode_rows_device, which
 *     zeroes the rest of the row.
 *   Sums of data unit u: chunks c < ceil(len(u) / bytes_per_checksum), the last
 *     over [c*bpc, len(u)); of a parity unit: chunks c < ceil(n0 / bpc).  Sums
 *     slots past these are not written.  These are the sums
 *     hec_composite_crc*, hec_scrub_crc_rows_device* and
 *     hec_reconstruct_crc_rows_device* (as d_expected) expect.
 * checksum_type is HEC_CHECKSUM_CRC32C or HEC_CHECKSUM_CRC32, also on full
 * stripes; HEC_CHECKSUM_NULL and unknown types are HEC_ERR_INVALID_ARG
 * (hec_encode_rows_device is the call without sums).
 * Checks, in this order, nothing queued on any error: coder, type, cell_len,
 * bytes_per_checksum, data_len / stripe_bytes (HEC_ERR_INVALID_ARG); a
 * host-only coder (HEC_ERR_DEVICE); NULL arrays or entries, d_sums NULL or not
 * 4-byte aligned, the workspace (HEC_ERR_INVALID_ARG); stripes == 0 is HEC_OK.
 * Uniform form: with data_len == 0 or a full last stripe and CRC32C the call
 * is hec_encode_crc_device, launch for launch.  Otherwise the first stripes-1
 * stripes run so (CRC32: the short-stripe kernel with every stripe at
 * k*cell_len, or hec_encode_device + hec_checksum_device for shapes it does not
 * take) and one more launch covers the last stripe with r passed by value;
 * kernels only, capturable into a graph.
 * Mixed form: without a short entry, the uniform form with data_len == 0.  With
 * one, a single launch of the short-stripe kernel over all stripes, the full
 * ones included (a big file with one short stripe is the uniform form's case).
 * d_workspace (hec_encode_crc_rows_mixed_workspace_size: 8 bytes per stripe; 0
 * for a NULL coder) is needed only then: NULL, not 8-byte aligned or too small
 * is HEC_ERR_INVALID_ARG.  It receives the u64 lengths (0 rewritten to
 * k*cell_len) in one asynchronous copy and must stay untouched until the
 * stream has passed the call.
 * The one-pass kernel (k reads + m writes over [0, n0)) takes k in {2,3,6,10},
 * m <= 4, bytes_per_checksum == 512, 16-B aligned bases, strides and cell_len
 * (below 2^31); every other shape takes a byte-wise kernel with the same
 * results.  All codecs (rs, xor, rs-legacy). */
int hec_encode_crc_rows_device(hec_coder_t *coder, int checksum_type,
                               const uint8_t *const *d_data, const size_t *data_strides,
                               uint8_t *const *d_parity, const size_t *parity_strides,
                               size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint64_t data_len,
                               uint8_t *d_sums, void *hip_stream);

size_t hec_encode_crc_rows_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);

int hec_encode_crc_rows_device_mixed(hec_coder_t *coder, int checksum_type,
                                     const uint8_t *const *d_data, const size_t *data_strides,
                                     uint8_t *const *d_parity, const size_t *parity_strides,
                                     const uint64_t *stripe_bytes, size_t cell_len, size_t stripes,
                                     size_t bytes_per_checksum,
                                     uint8_t *d_sums, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* ---- Verified striped read into a file-order buffer ------------------------ *
 * The reader's side of hec_encode_crc_rows_device* (StripedBlockStream::
 * read_slice on the device): one pass that verifies the survivors' chunk sums,
 * rebuilds the lost data units and writes all k data units of every stripe at
 * their file-order place, each cut to its own length.  Write -> read works on
 * one file-order buffer and one sums array, with no padding on either side.
 * Geometry (r, n0, len(u)), data_len (uniform form), stripe_bytes (mixed form,
 * host array, NULL = every stripe full, 0 or k*cell_len = full, above that
 * HEC_ERR_INVALID_ARG), present (host array, bit i of present[s] = unit i of
 * stripe s is present), the [stripe][k+m][nck] layout of d_expected and the
 * [stripe][k+m] layout of d_bad are those of
 * hec_reconstruct_crc_rows_device[_mixed].  d_shards[k+m] / shard_strides as
 * there; in the uniform form a NULL entry is a unit lost for the whole batch, in
 * the mixed form every unit that is a survivor of some stripe needs storage.
 * The survivors of a stripe are its first k present units, so every present
 * data unit is a survivor; e = its lost data units.  With e == 0, the common
 * read, k units are read, verified and written and no parity unit is touched.
 * Reads: no slot byte at or past len(u) influences anything; a unit that is
 * empty in a stripe is not read; nothing at or past cell_len of a slot is read;
 * on the 16-B aligned route a read may reach the end of the 16-byte block that
 * holds byte n0-1, and no further.
 * Output: data unit u < k of stripe s goes to d_file + s*file_stride +
 * u*cell_len (file_stride == 0: k*cell_len) for exactly len(u) bytes, copied
 * where it is present and rebuilt where it is lost.  There is no zero fill: no
 * byte of row s at or past r(s) is written, and none between k*cell_len and
 * file_stride.  In the uniform form with the default stride a buffer of exactly
 * data_len bytes is enough (stripes*k*cell_len with data_len == 0).  Parity is
 * never written, no sums are written, d_expected and the shards are read-only.
 * d_file must not overlap any shard slot; this is not checked.
 * Verification: with d_expected every survivor is verified over its own len(u)
 * bytes and d_bad[s*(k+m) + u] = 1 is set on a mismatch (flags are only ever
 * set: zero them first).  A stripe with a flagged survivor has unspecified
 * bytes in its row's [0, r); everything else holds.  The caller clears the
 * flagged unit from that stripe's mask and calls the mixed form again; there is
 * no host re-plan inside.  d_expected == NULL (d_bad is then ignored) is the
 * plain read.  checksum_type is HEC_CHECKSUM_CRC32C or HEC_CHECKSUM_CRC32 in
 * either case; HEC_CHECKSUM_NULL and unknown types are HEC_ERR_INVALID_ARG.
 * Checks, in this order, nothing queued on any error: coder, type, cell_len,
 * bytes_per_checksum, data_len / stripe_bytes, a file_stride that is non-zero
 * and below k*cell_len (HEC_ERR_INVALID_ARG); a host-only coder
 * (HEC_ERR_DEVICE); NULL arrays, d_file NULL, d_expected without d_bad or not
 * 4-byte aligned, the workspace (HEC_ERR_INVALID_ARG); stripes == 0 is HEC_OK.
 * A pattern with fewer than k present units is HEC_ERR_NOT_ENOUGH_SHARDS.
 * The calls are asynchronous and neither allocate nor read back.
 * Uniform form: one launch over the stripes-1 full stripes and one over the
 * last stripe with its r by value; a single launch when data_len == 0 or the
 * last stripe is full.  Kernels only, capturable into a graph.
 * Mixed form: one launch per distinct present mask over that mask's stripes,
 * full and short together.  d_workspace
 * (hec_read_crc_rows_mixed_workspace_size; 0 for a NULL coder) is always
 * required: NULL, not 8-byte aligned or too small is HEC_ERR_INVALID_ARG.  It
 * receives the masks' stripe lists and the u64 lengths (0 rewritten to
 * k*cell_len) in one asynchronous copy and must stay untouched until the
 * stream has passed the call; calls in flight at once need different
 * workspaces.
 * The one-pass kernel (k reads + k writes of live bytes) takes k in
 * {2,3,6,10}, e <= 4, bytes_per_checksum == 512, 16-B aligned bases, strides,
 * d_file, file_stride and cell_len (below 2^31); every other shape takes a
 * byte-wise kernel with the same results.  All codecs (rs, xor, rs-legacy). */
int hec_read_crc_rows_device(hec_coder_t *coder, int checksum_type,
                             const uint8_t *const *d_shards, const size_t *shard_strides,
                             uint8_t *d_file, size_t file_stride,
                             size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint64_t data_len,
                             const uint8_t *d_expected, uint8_t *d_bad, void *hip_stream);

size_t hec_read_crc_rows_mixed_workspace_size(const hec_coder_t *coder, size_t stripes);

int hec_read_crc_rows_device_mixed(hec_coder_t *coder, int checksum_type,
                                   const uint8_t *const *d_shards, const size_t *shard_strides,
                                   uint8_t *d_file, size_t file_stride,
                                   const uint64_t *present, const uint64_t *stripe_bytes,
                                   size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                                   const uint8_t *d_expected, uint8_t *d_bad,
                                   void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The raw hot loop, Mul<&[&[u8]]> (matrix.rs:204-231), batched:
 * out[j] = sum_i matrix[j*cols + i] * in[i] for j < rows, i < cols.
 * Any rows >= 1 (launched 4 output rows at a time), 1 <= cols <=
 * HEC_MAX_DATA_UNITS.  Runs on the coder's device. */
int hec_gf_matmul_device(hec_coder_t *coder, const uint8_t *matrix, size_t rows, size_t cols,
                         const uint8_t *const *d_in, const size_t *in_strides, uint8_t *const *d_out,
                         const size_t *out_strides, size_t cell_len, size_t stripes, void *hip_stream);

/* ---- Chunk checksums -------------------------------- *
 * WritePacket::calculate_checksum (rust/src/hdfs/connection.rs:568-584) on
 * the device: for each of `n_shards` cells of `stripes` stripes (shard i of
 * stripe s at d_bases[i] + s*strides[i], cell_len bytes), one CRC32C
 * (Castagnoli / crc CRC_32_ISCSI, connection.rs:37-38) per
 * bytes_per_checksum chunk, the last one possibly short, written big-endian
 * (put_u32) to d_out + 4*((s*n_shards + i)*nchunks + c), nchunks =
 * ceil(cell_len / bytes_per_checksum).  Runs on the coder's device; the
 * fast path is bytes_per_checksum == 512 with 16-B aligned cells. */
int hec_crc32c_device(hec_coder_t *coder, const uint8_t *const *d_bases, const size_t *strides, size_t n_shards,
                      size_t cell_len, size_t stripes, size_t bytes_per_checksum, uint8_t *d_out,
                      void *hip_stream);

/* The same for either algorithm the read path accepts: `checksum_type` is
 * HEC_CHECKSUM_CRC32C or HEC_CHECKSUM_CRC32 (HEC_CHECKSUM_NULL is invalid
 * here: there is nothing to compute). */
int hec_checksum_device(hec_coder_t *coder, int checksum_type, const uint8_t *const *d_bases, const size_t *strides,
                        size_t n_shards, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                        uint8_t *d_out, void *hip_stream);

/* ReadPacket::get_data's check (connection.rs:477-504) over whole cells:
 * recomputes every chunk checksum and compares it with d_expected (same
 * layout as hec_checksum_device's output, big-endian as received).
 * d_bad[s*n_shards + i] is set to 1 when any chunk of cell (s, i)
 * mismatches (the reference's HdfsError::ChecksumError for that packet) and
 * is otherwise left untouched: zero it first.  HEC_CHECKSUM_NULL verifies
 * nothing and returns HEC_OK.  Asynchronous on hip_stream. */
int hec_checksum_verify_device(hec_coder_t *coder, int checksum_type, const uint8_t *const *d_bases,
                               const size_t *strides, size_t n_shards, size_t cell_len, size_t stripes,
                               size_t bytes_per_checksum, const uint8_t *d_expected, uint8_t *d_bad,
                               void *hip_stream);

/* ---- Composite CRCs: cell, block and block-group sums from chunk sums ---- *
 * HDFS reports no chunk sums outward: with COMPOSITE_CRC a DataNode answers
 * OpBlockChecksum / OpBlockGroupChecksum with the CRC of a whole internal
 * block (optionally one per cell, stripeLength = cellSize) and the client
 * folds the cell CRCs of a block group, in file order, into the CRC of the
 * logical bytes.  These calls fold the [stripe][n_units][nck] chunk sums the
 * calls above leave behind, nck = ceil(cell_len / bytes_per_checksum); they
 * never read a cell.
 *
 * hec_crc_concat: *out = crc(A || B) from crc_a = crc(A), crc_b = crc(B) and
 * len_b = |B|, with crc(A || B) = L(crc(A) ^ xorout ^ init) ^ crc(B) where L
 * appends len_b zero bytes to the register (a multiply by x^(8 len_b) mod P).
 * HEC_CHECKSUM_CRC32C or HEC_CHECKSUM_CRC32; others -> HEC_ERR_INVALID_ARG.
 *
 * Geometry of the composite calls: the first data_units of the n_units units
 * per stripe are data.  data_len is the logical length of the group: 0 means
 * stripes * data_units * cell_len, otherwise (stripes-1) * data_units *
 * cell_len < data_len <= stripes * data_units * cell_len and only the last
 * stripe is short: with r bytes in it, data unit u holds min(cell_len,
 * max(0, r - u * cell_len)) and every parity unit min(cell_len, r), the first
 * cell's length.  Chunk c of a cell covers its bytes [c * bpc, min((c+1) *
 * bpc, len)); slots past ceil(len / bpc) are never read.  Outputs, big-endian
 * u32 like the sums, each optional (NULL = not computed, not written):
 *   cell_crcs[stripe][n_units]  CRC of each cell (crc(empty) for length 0);
 *   unit_crcs[n_units]          CRC of cells (0,u) || (1,u) || ...: internal block u;
 *   group_crc[1]                CRC of the data cells in file order (stripe,
 *                               then unit 0 .. data_units-1): the data_len logical bytes.
 * Each output depends only on the slots of its own cells.
 *
 * hec_composite_crc runs on the host and needs no coder.  HEC_ERR_INVALID_ARG
 * for NULL sums, cell_len == 0, bytes_per_checksum == 0, n_units not in
 * 1..64, data_units not in 1..n_units, data_len out of range (with stripes ==
 * 0 only 0 is in range), HEC_CHECKSUM_NULL or an unknown type.  HEC_OK,
 * nothing written, for stripes == 0.
 *
 * hec_composite_crc_device does the same on the coder's device,
 * asynchronously on hip_stream: it never synchronises, allocates or reads
 * back, so it can be captured into a graph.  d_sums is only read; nothing but
 * the requested outputs and the workspace is written.  d_workspace
 * (hec_composite_crc_workspace_size(n_units, stripes) bytes, 4-byte aligned)
 * is needed only when d_unit_crcs or d_group_crc is asked for, is untouched
 * until the stream reaches the work, and must differ between calls in flight
 * at once.  HEC_ERR_DEVICE on a host-only coder.  HEC_ERR_INVALID_ARG,
 * nothing queued: the host call's cases, a NULL coder, d_sums or an output
 * not 4-byte aligned, a needed workspace that is NULL, misaligned or too
 * small.  HEC_OK, nothing queued: stripes == 0 or all three outputs NULL. */
int hec_crc_concat(int checksum_type, uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t *out);
int hec_composite_crc(int checksum_type, const uint8_t *sums, size_t n_units, size_t data_units, size_t cell_len,
                      size_t stripes, size_t bytes_per_checksum, uint64_t data_len, uint8_t *cell_crcs,
                      uint8_t *unit_crcs, uint8_t *group_crc);
size_t hec_composite_crc_workspace_size(size_t n_units, size_t stripes);
int hec_composite_crc_device(hec_coder_t *coder, int checksum_type, const uint8_t *d_sums, size_t n_units,
                             size_t data_units, size_t cell_len, size_t stripes, size_t bytes_per_checksum,
                             uint64_t data_len, uint8_t *d_cell_crcs, uint8_t *d_unit_crcs, uint8_t *d_group_crc,
                             void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The striped read of one batch of rows (block_reader.rs:480-525 feeding
 * EcSchema::ec_decode, ec/mod.rs:62-89) with every cell it consumes
 * checksum-verified.  d_shards[k+m] as hec_decode_device (NULL = shard not
 * available for the whole batch).  Per stripe the survivors are the first k
 * available shards whose chunk checksums verify against d_sums
 * ([stripe][k+m][nchunks] big-endian, the sums that arrived with the
 * packets); a shard that fails is skipped and the next available one is
 * read instead, as read_slice drops a failing cell reader and starts the
 * next parity reader.  Every data shard that is missing or failed is
 * rebuilt into d_out[i] (out_strides as hec_decode_device; all k slots
 * are required, and a present data shard's slot may be its own input
 * buffer, which then is repaired in place); present data shards that
 * verify are not copied.  d_bad[s*(k+m) + i] = 1 marks the
 * cells that failed (zeroed by the call; device memory).  When every stripe
 * verifies first time this is one fused pass over the survivors (k in
 * {2,3,6,10}, 512-B chunks, 16-B aligned).  Stripes with a failing cell
 * are re-planned on the host together: each round verifies every newly
 * used cell of all of them (one stripe-list checksum launch per shard
 * index, one flag read-back), and one mixed-pattern decode then rebuilds
 * them all (at most m rounds).  Synchronous (it must see the
 * verdicts).  Returns HEC_ERR_NOT_ENOUGH_SHARDS when some stripe has fewer
 * than k shards that verify (its d_bad flags say which; the other stripes
 * are still rebuilt).  HEC_CHECKSUM_NULL decodes without verifying. */
int hec_decode_verify_device(hec_coder_t *coder, int checksum_type, const uint8_t *const *d_shards,
                             const size_t *shard_strides, uint8_t *const *d_out, const size_t *out_strides,
                             size_t cell_len, size_t stripes, size_t bytes_per_checksum, const uint8_t *d_sums,
                             uint8_t *d_bad, void *hip_stream);

/* Plan-time specialisation of the fused decode + verify pass.
 * That pass rebuilds the missing data rows with the decode plan's matrix,
 * known only at run time, through v_perm product tables.  For a plan the
 * engine meets, it generates the matrix's bit-sliced XOR network and compiles
 * the same kernel with it (hiprtc, loaded with dlopen): about a third fewer
 * VALU ops for RS(6,3) with 3 rows lost.  By default the compile runs on a
 * background thread the first time a plan is launched, and launches use the
 * ahead-of-time kernel until it is ready (identical results).  Code objects
 * are cached per process and on disk ($HEC_JIT_CACHE, default
 * ~/.cache/hdfs_ec_amd/jit; "" = none).  HEC_JIT=0 disables it, HEC_JIT=sync
 * compiles on first use.
 *   hec_coder_prepare_decode: compile (or load) the specialised kernel for the
 *     presence mask present[k+m] and checksum type now, synchronously, on the
 *     coder's device; *specialised = 1 when it is ready (0: not available --
 *     no hiprtc, JIT off, no fused shape for this plan, or nothing missing).
 *   hec_jit_warm: the same into the caches only, no device needed (install-
 *     time warm-up).  HEC_ERR_INVALID_ARG for a plan without a fused kernel
 *     (k not in {2,3,6,10}, no or more than 4 data shards missing),
 *     HEC_ERR_DEVICE when hiprtc is absent or the compile fails.
 *   hec_jit_stats: kernels compiled, loaded from the disk cache, failed,
 *     and launches that ran a specialised kernel (process totals). */
int hec_coder_prepare_decode(hec_coder_t *coder, const uint8_t *present, int checksum_type, int *specialised);
int hec_jit_warm(size_t data_units, size_t parity_units, const uint8_t *present, int checksum_type);
void hec_jit_stats(uint64_t *compiled, uint64_t *from_disk, uint64_t *failed, uint64_t *launches);

/* ---- work-queue counter sets (diagnostic) -------------- *
 * The coding kernels deal their tiles from launch counters.  Every stream
 * that launched one has two counter sets it alternates between (each launch
 * zeroes the set of the stream's next launch); a launch into a capturing
 * stream gets a set of its own, zeroed by a kernel node in the graph.
 * hec_queue_stats: streams with sets and graph sets handed out on `device`
 * (process totals; past 4096 streams / 256 graph launches per device the
 * kernels fall back to their fixed tile order), and *keyed_by_id = 1 when
 * streams are told apart by hipStreamGetId (HIP >= 7.1 in the process), 0
 * when by handle.  Any pointer may be NULL; all zeros for a device that
 * does not exist. */
void hec_queue_stats(int device, uint64_t *streams, uint64_t *graph_sets, int *keyed_by_id);

/* Encode plus CRC32C of the k data and m parity cells (shard order
 * 0..k+m-1, same output layout as hec_crc32c_device): everything a striped
 * writer needs to emit its k+m packet streams.  One fused pass (the
 * checksums are taken from the registers/LDS the encode already holds) for
 * k in {2,3,6,10}, m <= 4, 512-B chunks and 16-B aligned cells; otherwise an
 * encode followed by hec_crc32c_device. */
int hec_encode_crc_device(hec_coder_t *coder, const uint8_t *const *d_data, const size_t *data_strides,
                          uint8_t *const *d_parity, const size_t *parity_strides, size_t cell_len, size_t stripes,
                          size_t bytes_per_checksum, uint8_t *d_sums, void *hip_stream);

/* ---- Pinned-host pipelined batch (PCIe-inclusive path) ----------------- *
 * Encodes a [stripe][k][cell] host batch into a [stripe][m][cell] host batch,
 * streaming chunks of `chunk_stripes` stripes H2D -> encode -> D2H with
 * copy/compute overlap on the coder's own streams (3 device slots; H2D,
 * compute and D2H of consecutive chunks run concurrently).  Host buffers should be
 * pinned (hipHostMalloc / registered) for full PCIe rate.  Synchronous. */
int hec_encode_host_batch(hec_coder_t *coder, const uint8_t *h_data, uint8_t *h_parity,
                          size_t cell_len, size_t stripes, size_t chunk_stripes);

/* The read side, fused with the cell split (ec/mod.rs:62-89): h_vertical[k+m]
 * are the per-shard "vertical" buffers a striped reader accumulates (shard i
 * = its cells of `rows` consecutive rows, rows*cell_len bytes; NULL =
 * missing).  Writes the k*cell_len*rows file bytes, in file (row) order, to
 * h_file: present data cells are copied, missing ones reconstructed
 * (first-k-present survivors).  The k survivors stream H2D through the same
 * 3-slot pipeline as the encode and only the rebuilt cells come back D2H;
 * the present data cells are copied host-side (up to 4 threads) while the
 * DMA runs.  HEC_ERR_NOT_ENOUGH_SHARDS when a data shard is missing and fewer
 * than k shards are present.  Synchronous. */
int hec_decode_host_batch(hec_coder_t *coder, const uint8_t *const *h_vertical, size_t cell_len, size_t rows,
                          uint8_t *h_file, size_t chunk_rows);

/* ---- Whole files: the last row may be short ------------------------------ *
 * A file of data_len bytes is rows of k cells in file order (CellBuffer::write,
 * block_writer.rs:791-805); the last row may hold L < k*cell_len bytes: cell
 * i of it has min(cell_len, max(0, L - i*cell_len)) bytes.  As
 * CellBuffer::encode (block_writer.rs:817-851) every cell of that row is
 * zero-padded to n0 = min(cell_len, L) and its m parity cells are n0 bytes
 * long; the engine writes them at their [row][m][cell_len] slots and zeroes
 * the slot bytes past n0.  Full rows run exactly as hec_encode_host_batch /
 * hec_encode_device. */
int hec_encode_rows_host(hec_coder_t *coder, const uint8_t *h_data, size_t data_len, uint8_t *h_parity,
                         size_t cell_len, size_t chunk_stripes);

/* The same on device memory (asynchronous on hip_stream): d_parity holds
 * ceil(data_len / (k*cell_len)) rows.  The short row's short cells are
 * zero-padded into d_workspace (hec_encode_rows_workspace_size bytes, untouched
 * until the stream reaches the work), so nothing is read past d_data +
 * data_len.  The workspace is checked before anything is queued, and is
 * needed (may be NULL otherwise) only when some cell of the short row holds
 * fewer than n0 bytes. */
size_t hec_encode_rows_workspace_size(const hec_coder_t *coder, size_t cell_len);
int hec_encode_rows_device(hec_coder_t *coder, const uint8_t *d_data, size_t data_len, uint8_t *d_parity,
                           size_t cell_len, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* hec_decode_host_batch over a whole file: h_vertical[i] holds vertical_len[i]
 * bytes of shard i (its block: max_offset(i), ec/mod.rs:40-60; NULL =
 * missing), and the file is file_len bytes.  Every cell shorter than cell_len
 * (or absent past the end of its shard) reads as zeros, as
 * CellReader::next_cell pads it (block_reader.rs:343-378); the short last row
 * is decoded like the others and trimmed to file_len (block_reader.rs:
 * 524-549).  HEC_ERR_INVALID_ARG if a present shard holds fewer than
 * full_rows * cell_len bytes. */
int hec_decode_rows_host(hec_coder_t *coder, const uint8_t *const *h_vertical, const size_t *vertical_len,
                         size_t cell_len, uint8_t *h_file, size_t file_len, size_t chunk_rows);

/* ---- Multi-GPU coder group --------------------------------- *
 * Stripes are independent, so a batch is split into contiguous stripe ranges,
 * one per device, and each range runs on its own device's coder from its own
 * host thread (own streams and 3-slot pipeline), with no collective and no
 * device-to-device traffic.  This is the in-process form of the stripe
 * sharding the bench does with one process per GPU.  Range of device slot i
 * for `total` stripes: sizes differ by at most one and tile [0, total) in slot
 * order (hec_group_range).  A device may appear more than once (several
 * coders on one GPU).  The group calls are synchronous; on failure they
 * return the status of the lowest failing slot (hec_last_error() of the
 * calling thread carries its detail) after every slot has finished. */
typedef struct hec_group hec_group_t;

/* codec "rs" or "xor" as hec_coder_create_codec; n_devices in 1..64. */
int hec_group_create(const char *codec, size_t data_units, size_t parity_units, const int *devices,
                     size_t n_devices, hec_group_t **out);
void hec_group_destroy(hec_group_t *group);
size_t hec_group_size(const hec_group_t *group);
/* Slot i's coder (owned by the group), for device-resident calls on that GPU. */
hec_coder_t *hec_group_coder(hec_group_t *group, size_t slot);
/* Slot i's contiguous share [*first, *first + *count) of `total` stripes. */
int hec_group_range(const hec_group_t *group, size_t total, size_t slot, size_t *first, size_t *count);

/* hec_encode_host_batch over the group: slot i encodes its stripe range of
 * the [stripe][k][cell] host batch into the same rows of h_parity. */
int hec_group_encode_host_batch(hec_group_t *group, const uint8_t *h_data, uint8_t *h_parity, size_t cell_len,
                                size_t stripes, size_t chunk_stripes);

/* hec_decode_host_batch over the group: slot i decodes its row range (its
 * part of every vertical buffer) into its rows of h_file. */
int hec_group_decode_host_batch(hec_group_t *group, const uint8_t *const *h_vertical, size_t cell_len,
                                size_t rows, uint8_t *h_file, size_t chunk_rows);

/* Device-resident batches over the group (the in-process form of the
 * bench's one-rank-per-GPU sharding; no host threads, no collective): slot i's
 * stripes live in ITS device's HBM.  Per-slot arrays, slot-major: d_data[i*k
 * + s] / data_strides[i*k + s] and d_parity[i*m + j] / parity_strides[i*m +
 * j] as hec_encode_device takes them; for decode d_shards[i*(k+m) + s]
 * (NULL = missing) / shard_strides[i*(k+m) + s] and d_out[i*k + s] /
 * out_strides[i*k + s] as hec_decode_device.  stripes[i] = slot i's stripe
 * count (0 = nothing), hip_streams[i] its stream on that device (NULL array =
 * default streams).  Asynchronous like the single-coder calls: every slot's
 * launch is enqueued from the calling thread, one device after another, and
 * the GPUs run concurrently; synchronise the streams before reading.
 * Returns the lowest failing slot's status; the other slots are still
 * enqueued.  Replaces the per-writer join_all fan-out of block_writer.rs:954
 * for device-resident stripes. */
int hec_group_encode_device(hec_group_t *group, const uint8_t *const *d_data, const size_t *data_strides,
                            uint8_t *const *d_parity, const size_t *parity_strides, size_t cell_len,
                            const size_t *stripes, void *const *hip_streams);
int hec_group_decode_device(hec_group_t *group, const uint8_t *const *d_shards, const size_t *shard_strides,
                            uint8_t *const *d_out, const size_t *out_strides, size_t cell_len,
                            const size_t *stripes, void *const *hip_streams);

/* ---- HBM buffers for the batched API ------------------------------------ *
 * Device memory for stripe batches on `device` (hipExtMallocWithFlags).
 * Checksum sum / flag buffers passed to the checksum calls must be 4-byte
 * aligned (they are read and written as u32).
 * HEC_ALLOC_CONTIGUOUS asks for physically contiguous HBM, which the GPU
 * maps with large page fragments: a batch of tens of GiB then needs far
 * fewer translation entries.  hec_device_free releases it
 * (synchronous, like hipFree). */
#define HEC_ALLOC_DEFAULT 0
#define HEC_ALLOC_CONTIGUOUS 1
int hec_device_alloc(int device, size_t bytes, unsigned flags, void **out);
int hec_device_free(int device, void *ptr);
/* hec_device_copy: `bytes` from src to dst, host or device memory either
 * side (unified addressing), synchronous; for callers without a HIP binding
 * of their own (the Rust shim's DeviceBuffer).  hec_device_synchronize: wait
 * for `hip_stream` on `device` (NULL = the device's default stream) -- the
 * device calls above only enqueue. */
int hec_device_copy(int device, void *dst, const void *src, size_t bytes);
int hec_device_synchronize(int device, void *hip_stream);

/* ---- NUMA-placed pinned host buffers (host-batch / group calls) -------- *
 * hec_host_alloc: `bytes` of page-locked host memory whose pages live on
 * NUMA node `numa_node` (-1 = the node of `device`'s PCIe root, read from
 * sysfs), registered with HIP for full-rate DMA: the buffers one group slot
 * streams to its GPU should sit next to that GPU's root complex.  Free with
 * hec_host_free.  hec_device_numa_node: that node, -1 if unknown. */
int hec_device_numa_node(int device);
int hec_host_alloc(int device, size_t bytes, int numa_node, void **out);
int hec_host_free(void *ptr);


#ifdef __cplusplus
}
#endif

#endif /* HDFS_EC_AMD_H */
