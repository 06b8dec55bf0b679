//! MI355X erasure-coding engine behind hdfs-native's internal EC functions.
//!
//! FFI to the C ABI in `include/hdfs_ec_amd.h` (library
//! `hdfs-native_amd/lib/libhdfs_ec_amd.so`), compiled only with the `mi355x`
//! cargo feature (see `rust/Cargo.toml.mi355x` and `rust/build_mi355x.rs`).
//! This file is written for hdfs-native 0.14.1's `rust/src/ec/` and is NOT
//! compiled in this repository's image (no cargo/rustc); `tests/cpp/
//! shim_replay.c` replays its exact C call sequence against the engine.
//!
//! It replaces, with the same contracts:
//!   * `Coder::new`     (`rust/src/ec/gf256.rs:32-38`)
//!   * `Coder::encode`  (`gf256.rs:61-80`): panics on a wrong shard count or
//!     unequal / zero lengths, like the reference's asserts (`gf256.rs:62-65`,
//!     `matrix.rs:57`); otherwise infallible;
//!   * `Coder::decode`  (`gf256.rs:84-137`): fills only missing DATA slots,
//!     first-k-present survivors, `Err(ErasureCodingError("Not enough valid
//!     shards"))` when fewer than k are present; parity slots are never
//!     touched.
//! and adds the batched forms the striped writer/reader can use instead of
//! one call per 1 MiB row.  `PooledCoder` is what `Coder::new` holds when the
//! `mi355x` feature forwards the reference's `Coder` (rust/patches/
//! ec_mi355x.patch): the reference builds a Coder per decoded row
//! (`ec/mod.rs:71`), so it takes an idle engine coder from the process-wide
//! pool (`hec_coder_acquire`) and gives it back on drop.  `Coder::new` stays
//! infallible: without a GPU the pool hands out an engine host-only coder,
//! and if even that fails the patched `Coder` keeps `None` and runs the
//! reference CPU path.  The striped writer and reader keep calling one row
//! at a time on pageable cells, which the engine codes with its host routine
//! (DESIGN.md §1 measures the device route at those call shapes: it loses).
//! `GpuCoder::encode_rows` / `decode_rows` are the pinned-memory batched
//! forms for callers that hold many rows at once (a reconstruct worker);
//! `GpuCoder::encode_device` / `decode_device` with `DeviceBuffer` the
//! device-resident forms (the patch's `mi355x` group of rust/benches/ec.rs).

use std::ffi::{c_char, c_int, c_void, CStr};

use bytes::{Bytes, BytesMut};

use crate::{HdfsError, Result};

#[repr(C)]
pub struct HecCoder {
    _private: [u8; 0],
}

#[repr(C)]
pub struct HecGroup {
    _private: [u8; 0],
}

const HEC_OK: c_int = 0;
const HEC_ERR_INVALID_ARG: c_int = -1;
const HEC_ERR_NOT_ENOUGH_SHARDS: c_int = -2;
const HEC_ERR_UNSUPPORTED_CODEC: c_int = -3;
const HEC_ERR_CHECKSUM: c_int = -7;
/// `device` of an engine host-only coder (include/hdfs_ec_amd.h).
const HEC_DEVICE_HOST: c_int = -2;

unsafe extern "C" {
    fn hec_abi_version() -> c_int;
    fn hec_strerror(rc: c_int) -> *const c_char;
    fn hec_last_error() -> *const c_char;
    fn hec_coder_create_codec(codec: *const c_char, k: usize, m: usize, device: c_int,
                              out: *mut *mut HecCoder) -> c_int;
    fn hec_coder_destroy(c: *mut HecCoder);
    fn hec_coder_acquire(codec: *const c_char, k: usize, m: usize, device: c_int, out: *mut *mut HecCoder) -> c_int;
    fn hec_coder_release(c: *mut HecCoder);
    fn hec_coder_device(c: *const HecCoder) -> c_int;
    fn hec_encode_rows_host(c: *mut HecCoder, h_data: *const u8, data_len: usize, h_parity: *mut u8,
                            cell_len: usize, chunk_stripes: usize) -> c_int;
    fn hec_decode_rows_host(c: *mut HecCoder, h_vertical: *const *const u8, vertical_len: *const usize,
                            cell_len: usize, h_file: *mut u8, file_len: usize, chunk_rows: usize) -> c_int;
    fn hec_encode(c: *mut HecCoder, data: *const *const u8, n: usize, parity: *const *mut u8) -> c_int;
    fn hec_decode(c: *mut HecCoder, shards: *const *const u8, n: usize, out: *const *mut u8) -> c_int;
    fn hec_encode_host_batch(c: *mut HecCoder, h_data: *const u8, h_parity: *mut u8, cell_len: usize,
                             stripes: usize, chunk_stripes: usize) -> c_int;
    fn hec_decode_host_batch(c: *mut HecCoder, h_vertical: *const *const u8, cell_len: usize, rows: usize,
                             h_file: *mut u8, chunk_rows: usize) -> c_int;
    fn hec_decode_verify_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                shard_strides: *const usize, d_out: *const *mut u8, out_strides: *const usize,
                                cell_len: usize, stripes: usize, bytes_per_checksum: usize, d_sums: *const u8,
                                d_bad: *mut u8, stream: *mut c_void) -> c_int;
    fn hec_encode_device(c: *mut HecCoder, d_data: *const *const u8, data_strides: *const usize,
                         d_parity: *const *mut u8, parity_strides: *const usize, cell_len: usize, stripes: usize,
                         stream: *mut c_void) -> c_int;
    fn hec_decode_device(c: *mut HecCoder, d_shards: *const *const u8, shard_strides: *const usize,
                         d_out: *const *mut u8, out_strides: *const usize, cell_len: usize, stripes: usize,
                         stream: *mut c_void) -> c_int;
    fn hec_reconstruct(c: *mut HecCoder, shards: *const *const u8, n: usize, want: *const u8,
                       out: *const *mut u8) -> c_int;
    fn hec_reconstruct_device(c: *mut HecCoder, d_shards: *const *const u8, shard_strides: *const usize,
                              d_out: *const *mut u8, out_strides: *const usize, want: *const u8, cell_len: usize,
                              stripes: usize, stream: *mut c_void) -> c_int;
    fn hec_reconstruct_plan(codec: *const c_char, k: usize, m: usize, present: *const u8, want: *const u8,
                            n_targets: *mut usize, survivors: *mut usize, targets: *mut usize,
                            matrix: *mut u8) -> c_int;
    fn hec_reconstruct_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_reconstruct_device_mixed(c: *mut HecCoder, d_shards: *const *const u8, shard_strides: *const usize,
                                    d_out: *const *mut u8, out_strides: *const usize, present: *const u64,
                                    want: *const u64, cell_len: usize, stripes: usize, d_workspace: *mut c_void,
                                    workspace_bytes: usize, stream: *mut c_void) -> c_int;
    fn hec_reconstruct_crc_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                  shard_strides: *const usize, d_out: *const *mut u8, out_strides: *const usize,
                                  want: *const u8, cell_len: usize, stripes: usize, bytes_per_checksum: usize,
                                  d_expected: *const u8, d_bad: *mut u8, d_sums: *mut u8,
                                  stream: *mut c_void) -> c_int;
    fn hec_reconstruct_crc_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_reconstruct_crc_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                        shard_strides: *const usize, d_out: *const *mut u8,
                                        out_strides: *const usize, present: *const u64, want: *const u64,
                                        cell_len: usize, stripes: usize, bytes_per_checksum: usize,
                                        d_expected: *const u8, d_bad: *mut u8, d_sums: *mut u8,
                                        d_workspace: *mut c_void, workspace_bytes: usize,
                                        stream: *mut c_void) -> c_int;
    fn hec_reconstruct_sums_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                   shard_strides: *const usize, want: *const u8, cell_len: usize, stripes: usize,
                                   bytes_per_checksum: usize, data_len: u64, d_expected: *const u8,
                                   d_bad: *mut u8, d_sums: *mut u8, stream: *mut c_void) -> c_int;
    fn hec_reconstruct_sums_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                         shard_strides: *const usize, present: *const u64, want: *const u64,
                                         cell_len: usize, stripes: usize, bytes_per_checksum: usize,
                                         d_expected: *const u8, d_bad: *mut u8, d_sums: *mut u8,
                                         d_workspace: *mut c_void, workspace_bytes: usize,
                                         stream: *mut c_void) -> c_int;
    fn hec_reconstruct_crc_rows_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                       shard_strides: *const usize, d_out: *const *mut u8,
                                       out_strides: *const usize, want: *const u8, cell_len: usize, stripes: usize,
                                       bytes_per_checksum: usize, data_len: u64, d_expected: *const u8,
                                       d_bad: *mut u8, d_sums: *mut u8, stream: *mut c_void) -> c_int;
    fn hec_reconstruct_crc_rows_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_reconstruct_crc_rows_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                             shard_strides: *const usize, d_out: *const *mut u8,
                                             out_strides: *const usize, present: *const u64, want: *const u64,
                                             stripe_bytes: *const u64, cell_len: usize, stripes: usize,
                                             bytes_per_checksum: usize, d_expected: *const u8, d_bad: *mut u8,
                                             d_sums: *mut u8, d_workspace: *mut c_void, workspace_bytes: usize,
                                             stream: *mut c_void) -> c_int;
    fn hec_scrub_verdict(ruled_out: u64, bad_bytes: u64, units: usize, unit: *mut c_int) -> c_int;
    fn hec_scrub(c: *mut HecCoder, shards: *const *const u8, shard_len: usize, out: *mut ScrubResult) -> c_int;
    fn hec_scrub_device(c: *mut HecCoder, d_shards: *const *const u8, shard_strides: *const usize, cell_len: usize,
                        stripes: usize, d_results: *mut ScrubResult, stream: *mut c_void) -> c_int;
    fn hec_scrub_correct_device(c: *mut HecCoder, d_shards: *const *mut u8, shard_strides: *const usize,
                                cell_len: usize, stripes: usize, d_results: *const ScrubResult, d_units: *mut i32,
                                stream: *mut c_void) -> c_int;
    fn hec_scrub_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_scrub_device_mixed(c: *mut HecCoder, d_shards: *const *const u8, shard_strides: *const usize,
                              present: *const u64, cell_len: usize, stripes: usize, d_results: *mut ScrubResult,
                              d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    fn hec_scrub_crc_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                            shard_strides: *const usize, cell_len: usize, stripes: usize,
                            bytes_per_checksum: usize, d_expected: *const u8, d_bad: *mut u8,
                            d_results: *mut ScrubResult, stream: *mut c_void) -> c_int;
    fn hec_scrub_crc_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_scrub_crc_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                  shard_strides: *const usize, present: *const u64, cell_len: usize,
                                  stripes: usize, bytes_per_checksum: usize, d_expected: *const u8,
                                  d_bad: *mut u8, d_results: *mut ScrubResult, d_workspace: *mut c_void,
                                  workspace_bytes: usize, stream: *mut c_void) -> c_int;
    fn hec_scrub_crc_rows_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                 shard_strides: *const usize, cell_len: usize, stripes: usize,
                                 bytes_per_checksum: usize, data_len: u64, d_expected: *const u8, d_bad: *mut u8,
                                 d_results: *mut ScrubResult, stream: *mut c_void) -> c_int;
    fn hec_scrub_crc_rows_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_scrub_crc_rows_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                       shard_strides: *const usize, present: *const u64, stripe_bytes: *const u64,
                                       cell_len: usize, stripes: usize, bytes_per_checksum: usize,
                                       d_expected: *const u8, d_bad: *mut u8, d_results: *mut ScrubResult,
                                       d_workspace: *mut c_void, workspace_bytes: usize,
                                       stream: *mut c_void) -> c_int;
    fn hec_encode_crc_rows_device(c: *mut HecCoder, checksum_type: c_int, d_data: *const *const u8,
                                  data_strides: *const usize, d_parity: *const *mut u8,
                                  parity_strides: *const usize, cell_len: usize, stripes: usize,
                                  bytes_per_checksum: usize, data_len: u64, d_sums: *mut u8,
                                  stream: *mut c_void) -> c_int;
    fn hec_encode_crc_rows_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_encode_crc_rows_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_data: *const *const u8,
                                        data_strides: *const usize, d_parity: *const *mut u8,
                                        parity_strides: *const usize, stripe_bytes: *const u64, cell_len: usize,
                                        stripes: usize, bytes_per_checksum: usize, d_sums: *mut u8,
                                        d_workspace: *mut c_void, workspace_bytes: usize,
                                        stream: *mut c_void) -> c_int;
    fn hec_read_crc_rows_device(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                shard_strides: *const usize, d_file: *mut u8, file_stride: usize, cell_len: usize,
                                stripes: usize, bytes_per_checksum: usize, data_len: u64, d_expected: *const u8,
                                d_bad: *mut u8, stream: *mut c_void) -> c_int;
    fn hec_read_crc_rows_mixed_workspace_size(c: *const HecCoder, stripes: usize) -> usize;
    fn hec_read_crc_rows_device_mixed(c: *mut HecCoder, checksum_type: c_int, d_shards: *const *const u8,
                                      shard_strides: *const usize, d_file: *mut u8, file_stride: usize,
                                      present: *const u64, stripe_bytes: *const u64, cell_len: usize, stripes: usize,
                                      bytes_per_checksum: usize, d_expected: *const u8, d_bad: *mut u8,
                                      d_workspace: *mut c_void, workspace_bytes: usize,
                                      stream: *mut c_void) -> c_int;
    fn hec_crc_concat(checksum_type: c_int, crc_a: u32, crc_b: u32, len_b: u64, out: *mut u32) -> c_int;
    fn hec_composite_crc(checksum_type: c_int, sums: *const u8, n_units: usize, data_units: usize, cell_len: usize,
                         stripes: usize, bytes_per_checksum: usize, data_len: u64, cell_crcs: *mut u8,
                         unit_crcs: *mut u8, group_crc: *mut u8) -> c_int;
    fn hec_composite_crc_workspace_size(n_units: usize, stripes: usize) -> usize;
    fn hec_composite_crc_device(c: *mut HecCoder, checksum_type: c_int, d_sums: *const u8, n_units: usize,
                                data_units: usize, cell_len: usize, stripes: usize, bytes_per_checksum: usize,
                                data_len: u64, d_cell_crcs: *mut u8, d_unit_crcs: *mut u8, d_group_crc: *mut u8,
                                d_workspace: *mut c_void, workspace_bytes: usize, stream: *mut c_void) -> c_int;
    fn hec_device_alloc(device: c_int, bytes: usize, flags: u32, out: *mut *mut c_void) -> c_int;
    fn hec_device_free(device: c_int, ptr: *mut c_void) -> c_int;
    fn hec_device_copy(device: c_int, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    fn hec_device_synchronize(device: c_int, stream: *mut c_void) -> c_int;
    fn hec_group_create(codec: *const c_char, k: usize, m: usize, devices: *const c_int, n_devices: usize,
                        out: *mut *mut HecGroup) -> c_int;
    fn hec_group_destroy(g: *mut HecGroup);
    fn hec_group_encode_host_batch(g: *mut HecGroup, h_data: *const u8, h_parity: *mut u8, cell_len: usize,
                                   stripes: usize, chunk_stripes: usize) -> c_int;
    fn hec_group_decode_host_batch(g: *mut HecGroup, h_vertical: *const *const u8, cell_len: usize,
                                   rows: usize, h_file: *mut u8, chunk_rows: usize) -> c_int;
}

/// One stripe's scrub result (`hec_scrub_result_t`): bit t of `ruled_out` is
/// set when some byte position's syndromes cannot come from unit t alone;
/// `bad_bytes` counts the positions whose syndromes are not all zero.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct ScrubResult {
    pub ruled_out: u64,
    pub bad_bytes: u64,
}

/// What a scrub result says about a stripe (`HEC_SCRUB_*`).  `Located` is
/// exact for up to m-1 corrupt units when m >= 3 and assumes at most one when
/// m == 2; with one parity unit the answer is never `Located`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ScrubVerdict {
    Clean,
    Located(usize),
    Ambiguous,
    Multiple,
}

/// `hec_scrub_verdict` (host only): the verdict for a stripe of `units` = k+m units.
pub fn scrub_verdict(result: ScrubResult, units: usize) -> Result<ScrubVerdict> {
    let mut unit: c_int = -1;
    match unsafe { hec_scrub_verdict(result.ruled_out, result.bad_bytes, units, &mut unit) } {
        0 => Ok(ScrubVerdict::Clean),
        1 => Ok(ScrubVerdict::Located(unit as usize)),
        2 => Ok(ScrubVerdict::Ambiguous),
        3 => Ok(ScrubVerdict::Multiple),
        rc => Err(err(rc)),
    }
}

/// The ABI revision this shim is written against (include/hdfs_ec_amd.h).
const ABI_VERSION: c_int = 5;

/// Status -> the reference's error kinds (rust/src/error.rs:32-39).
fn err(rc: c_int) -> HdfsError {
    match rc {
        HEC_ERR_NOT_ENOUGH_SHARDS => HdfsError::ErasureCodingError("Not enough valid shards".to_string()),
        HEC_ERR_UNSUPPORTED_CODEC => HdfsError::UnsupportedErasureCodingPolicy("engine codec".to_string()),
        HEC_ERR_CHECKSUM => HdfsError::ChecksumError,
        HEC_ERR_INVALID_ARG => HdfsError::InvalidArgument(status_text(rc)),
        _ => HdfsError::InternalError(format!("{}: {}", status_text(rc), last_error())),
    }
}

fn status_text(rc: c_int) -> String {
    unsafe { CStr::from_ptr(hec_strerror(rc)).to_string_lossy().into_owned() }
}

fn last_error() -> String {
    unsafe { CStr::from_ptr(hec_last_error()).to_string_lossy().into_owned() }
}

fn check(rc: c_int) -> Result<()> {
    if rc == HEC_OK { Ok(()) } else { Err(err(rc)) }
}

/// A coder bound to one MI355X (`hec_coder_t`).  The C ABI serialises the
/// host-buffer calls of one coder internally, so it may be shared.
pub struct GpuCoder {
    raw: *mut HecCoder,
    data_units: usize,
    parity_units: usize,
    device: i32,
}

unsafe impl Send for GpuCoder {}
unsafe impl Sync for GpuCoder {}

impl GpuCoder {
    /// `Coder::new` on device `device` for codec "rs" (or "xor", "rs-legacy").
    pub fn new(codec: &str, data_units: usize, parity_units: usize, device: i32) -> Result<Self> {
        assert_eq!(unsafe { hec_abi_version() }, ABI_VERSION, "libhdfs_ec_amd ABI mismatch");
        let name = std::ffi::CString::new(codec).map_err(|_| HdfsError::InvalidArgument(codec.to_string()))?;
        let mut raw = std::ptr::null_mut();
        check(unsafe { hec_coder_create_codec(name.as_ptr(), data_units, parity_units, device, &mut raw) })?;
        Ok(Self { raw, data_units, parity_units, device })
    }

    /// The coder's device ordinal.
    pub fn device(&self) -> i32 {
        self.device
    }

    /// Batched `Coder::encode` on stripes already in HBM (`hec_encode_device`):
    /// shard i of stripe s at `data[i] + s * data_strides[i]`, parity row j at
    /// `parity[j] + s * parity_strides[j]`; enqueued on `stream` (null = the
    /// device's default stream), complete after `synchronize`.
    ///
    /// # Safety
    /// Device pointers valid for `stripes` cells of `cell` bytes in that
    /// layout, on this coder's device; `stream` belongs to it.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn encode_device(&self, data: &[*const u8], data_strides: &[usize], parity: &[*mut u8],
                                parity_strides: &[usize], cell: usize, stripes: usize,
                                stream: *mut c_void) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(data.len() == k && data_strides.len() == k, "one slot per data shard");
        assert!(parity.len() == m && parity_strides.len() == m, "one slot per parity shard");
        check(unsafe {
            hec_encode_device(self.raw, data.as_ptr(), data_strides.as_ptr(), parity.as_ptr(),
                              parity_strides.as_ptr(), cell, stripes, stream)
        })
    }

    /// Batched `Coder::decode` on stripes already in HBM (`hec_decode_device`),
    /// one erasure pattern for the batch: `shards[k+m]` (null = missing),
    /// missing data shard i rebuilt into `out[i]` (the other `out` slots are
    /// never written; null is fine there).  `Err(ErasureCodingError)` when
    /// fewer than k shards are present.
    ///
    /// # Safety
    /// As `encode_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn decode_device(&self, shards: &[*const u8], shard_strides: &[usize], out: &[*mut u8],
                                out_strides: &[usize], cell: usize, stripes: usize,
                                stream: *mut c_void) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(shards.len() == k + m && shard_strides.len() == k + m, "one slot per shard");
        assert!(out.len() == k && out_strides.len() == k, "one output slot per data shard");
        check(unsafe {
            hec_decode_device(self.raw, shards.as_ptr(), shard_strides.as_ptr(), out.as_ptr(), out_strides.as_ptr(),
                              cell, stripes, stream)
        })
    }

    /// Batched reconstruction on stripes already in HBM
    /// (`hec_reconstruct_device`), one pattern for the batch: `shards[k+m]`
    /// (null = missing); every missing unit, data or parity, that `want`
    /// names (`None` = all of them) is rebuilt into `out[t]`, which may be the
    /// unit's own storage slot (the other `out` slots are never written; null
    /// is fine there).  What a repair worker calls; the reader never does.
    /// `Err(ErasureCodingError)` when fewer than k units are present.
    ///
    /// # Safety
    /// As `encode_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_device(&self, shards: &[*const u8], shard_strides: &[usize], out: &[*mut u8],
                                     out_strides: &[usize], want: Option<&[usize]>, cell: usize, stripes: usize,
                                     stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        let flags = want.map(|w| want_flags(n, w));
        check(unsafe {
            hec_reconstruct_device(self.raw, shards.as_ptr(), shard_strides.as_ptr(), out.as_ptr(),
                                   out_strides.as_ptr(), flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()),
                                   cell, stripes, stream)
        })
    }

    /// Device bytes `reconstruct_device_mixed` needs for `stripes` stripes.
    pub fn reconstruct_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_reconstruct_mixed_workspace_size(self.raw, stripes) }
    }

    /// A repair batch (`hec_reconstruct_device_mixed`): every stripe has its
    /// own loss pattern.  `shards[k+m]` is the storage of every unit (never
    /// null); `present[s]` bit i = unit i of stripe s is intact; `want[s]`
    /// (`None` = everything the stripe lacks) bit t = rebuild unit t.  Rebuilt
    /// unit t of stripe s goes to `out[t] + s * out_strides[t]`, which may be
    /// `shards[t]`'s slot (repair in place); `out[t]` may be null for units no
    /// stripe rebuilds.  `workspace` is device memory of
    /// `reconstruct_mixed_workspace_size(stripes)` bytes, untouched until
    /// `stream` has passed the call.
    ///
    /// # Safety
    /// As `encode_device`; `workspace` valid for `workspace_bytes` on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_device_mixed(&self, shards: &[*const u8], shard_strides: &[usize], out: &[*mut u8],
                                           out_strides: &[usize], present: &[u64], want: Option<&[u64]>,
                                           cell: usize, workspace: *mut c_void, workspace_bytes: usize,
                                           stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        assert!(want.map_or(true, |w| w.len() == present.len()), "one want mask per stripe");
        check(unsafe {
            hec_reconstruct_device_mixed(self.raw, shards.as_ptr(), shard_strides.as_ptr(), out.as_ptr(),
                                         out_strides.as_ptr(), present.as_ptr(),
                                         want.map_or(std::ptr::null(), |w| w.as_ptr()), cell, present.len(),
                                         workspace, workspace_bytes, stream)
        })
    }

    /// `reconstruct_device` with the chunk checksums that surround a repair
    /// worker's bytes, in the same pass (`hec_reconstruct_crc_device`).  `sums`
    /// (`[stripe][k+m][nck]` big-endian u32, 4-byte aligned) receives the chunk
    /// sums of every rebuilt unit at that unit's own slot and nothing else.
    /// With `expected` (same layout; may be `sums` itself) and `bad`
    /// (`[stripe][k+m]` bytes the caller zeroed) the k survivors the plan reads
    /// are verified and a mismatch sets `bad[s * (k+m) + unit] = 1`; pass null
    /// for both when the survivors' sums are already trusted.  `checksum_type`
    /// is a `ChecksumTypeProto` value (CRC32C or CRC32; NULL = plain
    /// `reconstruct_device`).  Never blocks: read `bad` back once `stream` has
    /// passed the call.
    ///
    /// # Safety
    /// As `encode_device`; the checksum buffers valid for their layouts on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_crc_device(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                         out: &[*mut u8], out_strides: &[usize], want: Option<&[usize]>,
                                         cell: usize, stripes: usize, bytes_per_checksum: usize,
                                         expected: *const u8, bad: *mut u8, sums: *mut u8,
                                         stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        let flags = want.map(|w| want_flags(n, w));
        check(unsafe {
            hec_reconstruct_crc_device(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(),
                                       out.as_ptr(), out_strides.as_ptr(),
                                       flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), cell, stripes,
                                       bytes_per_checksum, expected, bad, sums, stream)
        })
    }

    /// Device bytes `reconstruct_crc_device_mixed` needs for `stripes` stripes.
    pub fn reconstruct_crc_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_reconstruct_crc_mixed_workspace_size(self.raw, stripes) }
    }

    /// A repair batch with its checksums (`hec_reconstruct_crc_device_mixed`):
    /// `reconstruct_device_mixed` plus the checksum buffers of
    /// `reconstruct_crc_device`.  A stripe whose survivor is flagged in `bad`
    /// is repaired by a second call for those stripes alone: clear the bad
    /// unit's bit in `present`, add it to `want` if it should be rebuilt too,
    /// and pass `want = 0` for every other stripe.  `workspace` is device memory
    /// of `reconstruct_crc_mixed_workspace_size(stripes)` bytes, untouched until
    /// `stream` has passed the call.
    ///
    /// # Safety
    /// As `reconstruct_crc_device`; `workspace` valid for `workspace_bytes` on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_crc_device_mixed(&self, checksum_type: i32, shards: &[*const u8],
                                               shard_strides: &[usize], out: &[*mut u8], out_strides: &[usize],
                                               present: &[u64], want: Option<&[u64]>, cell: usize,
                                               bytes_per_checksum: usize, expected: *const u8, bad: *mut u8,
                                               sums: *mut u8, workspace: *mut c_void, workspace_bytes: usize,
                                               stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        assert!(want.map_or(true, |w| w.len() == present.len()), "one want mask per stripe");
        check(unsafe {
            hec_reconstruct_crc_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(),
                                             shard_strides.as_ptr(), out.as_ptr(), out_strides.as_ptr(),
                                             present.as_ptr(), want.map_or(std::ptr::null(), |w| w.as_ptr()), cell,
                                             present.len(), bytes_per_checksum, expected, bad, sums, workspace,
                                             workspace_bytes, stream)
        })
    }

    /// The chunk sums of the lost units of a block group, reconstructed from
    /// the survivors, with nothing rebuilt written to memory
    /// (`hec_reconstruct_sums_device`): what a degraded group's block (group)
    /// checksum needs.  `shards`, `want`, `expected`, `bad` and `sums` as for
    /// `reconstruct_crc_device`, but the cells are only read.  `data_len` as
    /// for `hec_composite_crc`: 0 = every stripe full, otherwise the last
    /// stripe is short and every sum covers the unit's true bytes, so
    /// `hec_composite_crc_device` with the same `data_len` on the same stream
    /// turns `sums` into the block and group CRCs.  `checksum_type` is CRC32C
    /// or CRC32.
    ///
    /// # Safety
    /// As `reconstruct_crc_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_sums_device(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                          want: Option<&[usize]>, cell: usize, stripes: usize,
                                          bytes_per_checksum: usize, data_len: u64, expected: *const u8,
                                          bad: *mut u8, sums: *mut u8, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        let flags = want.map(|w| want_flags(n, w));
        check(unsafe {
            hec_reconstruct_sums_device(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(),
                                        flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), cell, stripes,
                                        bytes_per_checksum, data_len, expected, bad, sums, stream)
        })
    }

    /// `reconstruct_sums_device` with one pattern per stripe, full stripes
    /// only (`hec_reconstruct_sums_device_mixed`).  `shards[i]` may be null for
    /// a unit no stripe has present: the dead node's.  `workspace` is device
    /// memory of `reconstruct_crc_mixed_workspace_size(stripes)` bytes,
    /// untouched until `stream` has passed the call.
    ///
    /// # Safety
    /// As `reconstruct_crc_device_mixed`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_sums_device_mixed(&self, checksum_type: i32, shards: &[*const u8],
                                                shard_strides: &[usize], present: &[u64], want: Option<&[u64]>,
                                                cell: usize, bytes_per_checksum: usize, expected: *const u8,
                                                bad: *mut u8, sums: *mut u8, workspace: *mut c_void,
                                                workspace_bytes: usize, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(want.map_or(true, |w| w.len() == present.len()), "one want mask per stripe");
        check(unsafe {
            hec_reconstruct_sums_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(),
                                              shard_strides.as_ptr(), present.as_ptr(),
                                              want.map_or(std::ptr::null(), |w| w.as_ptr()), cell, present.len(),
                                              bytes_per_checksum, expected, bad, sums, workspace, workspace_bytes,
                                              stream)
        })
    }

    /// `reconstruct_crc_device` for a block group whose last stripe is short
    /// (`hec_reconstruct_crc_rows_device`).  `data_len` as for
    /// `hec_composite_crc`: 0 = every stripe full, otherwise the last stripe
    /// holds the file's tail.  There every survivor counts as zero from its own
    /// length on and is verified over its own bytes, a rebuilt unit gets its
    /// bytes, zeros up to n0 = min(cell, tail) and the sums of its own bytes,
    /// and nothing at or past n0 is written: the slots are what
    /// `CellReader::next_cell` hands out and `sums` is what
    /// `hec_composite_crc_device` with the same `data_len` folds into the block
    /// and group CRCs.  `checksum_type` is CRC32C or CRC32.
    ///
    /// # Safety
    /// As `reconstruct_crc_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_crc_rows_device(&self, checksum_type: i32, shards: &[*const u8],
                                              shard_strides: &[usize], out: &[*mut u8], out_strides: &[usize],
                                              want: Option<&[usize]>, cell: usize, stripes: usize,
                                              bytes_per_checksum: usize, data_len: u64, expected: *const u8,
                                              bad: *mut u8, sums: *mut u8, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        let flags = want.map(|w| want_flags(n, w));
        check(unsafe {
            hec_reconstruct_crc_rows_device(self.raw, checksum_type as c_int, shards.as_ptr(),
                                            shard_strides.as_ptr(), out.as_ptr(), out_strides.as_ptr(),
                                            flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), cell, stripes,
                                            bytes_per_checksum, data_len, expected, bad, sums, stream)
        })
    }

    /// Device bytes `reconstruct_crc_rows_device_mixed` needs for `stripes` stripes.
    pub fn reconstruct_crc_rows_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_reconstruct_crc_rows_mixed_workspace_size(self.raw, stripes) }
    }

    /// A repair batch that spans block groups or small files
    /// (`hec_reconstruct_crc_rows_device_mixed`): `reconstruct_crc_device_mixed`
    /// with the logical bytes of every stripe.  `stripe_bytes[s]` of 0 or
    /// `k * cell` says stripe `s` is full (`None`: all of them); any other
    /// value is the stripe's length, handled as the last stripe of
    /// `reconstruct_crc_rows_device`.  `workspace` is device memory of
    /// `reconstruct_crc_rows_mixed_workspace_size(stripes)` bytes, 8-byte
    /// aligned, untouched until `stream` has passed the call.
    ///
    /// # Safety
    /// As `reconstruct_crc_device_mixed`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn reconstruct_crc_rows_device_mixed(&self, checksum_type: i32, shards: &[*const u8],
                                                    shard_strides: &[usize], out: &[*mut u8],
                                                    out_strides: &[usize], present: &[u64], want: Option<&[u64]>,
                                                    stripe_bytes: Option<&[u64]>, cell: usize,
                                                    bytes_per_checksum: usize, expected: *const u8, bad: *mut u8,
                                                    sums: *mut u8, workspace: *mut c_void, workspace_bytes: usize,
                                                    stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(out.len() == n && out_strides.len() == n, "one output slot per unit");
        assert!(want.map_or(true, |w| w.len() == present.len()), "one want mask per stripe");
        assert!(stripe_bytes.map_or(true, |b| b.len() == present.len()), "one length per stripe");
        check(unsafe {
            hec_reconstruct_crc_rows_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(),
                                                  shard_strides.as_ptr(), out.as_ptr(), out_strides.as_ptr(),
                                                  present.as_ptr(), want.map_or(std::ptr::null(), |w| w.as_ptr()),
                                                  stripe_bytes.map_or(std::ptr::null(), |b| b.as_ptr()), cell,
                                                  present.len(), bytes_per_checksum, expected, bad, sums, workspace,
                                                  workspace_bytes, stream)
        })
    }

    /// Scrubs a device-resident batch (`hec_scrub_device`): are the k+m units
    /// of every stripe consistent, and if not, which unit is wrong?  All
    /// `shards[k+m]` present (never null), laid out as for `encode_device`;
    /// read-only, no scratch.  `results` is device memory for `stripes`
    /// `ScrubResult`s (8-byte aligned); the call zeroes it on `stream` and the
    /// kernel fills it.  Copy it back once `stream` has passed the call and
    /// hand each entry to `scrub_verdict`; a `Located(t)` stripe is repaired by
    /// `reconstruct_device_mixed` with `present = all & !(1 << t)`, and a second
    /// scrub confirms it.
    ///
    /// # Safety
    /// As `encode_device`; `results` valid for `stripes * 16` bytes on this device.
    pub unsafe fn scrub_device(&self, shards: &[*const u8], shard_strides: &[usize], cell: usize, stripes: usize,
                               results: *mut ScrubResult, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_device(self.raw, shards.as_ptr(), shard_strides.as_ptr(), cell, stripes, results, stream)
        })
    }

    /// Fixes, in place, the unit a scrub located (`hec_scrub_correct_device`):
    /// `results` is what `scrub_device` or `scrub_crc_device` wrote for these
    /// very cells earlier on `stream`, with no write to them in between.  Per
    /// stripe the verdict of `scrub_verdict` is formed on the device;
    /// `units[s]` (device memory, `stripes` x `i32`, written for every stripe)
    /// receives the corrected unit, -1 (`HEC_CORRECT_CLEAN`) or -2
    /// (`HEC_CORRECT_UNLOCATED`, stripe untouched: repair it with `reconstruct_device_mixed`).  One
    /// kernel, no workspace, no synchronisation: scrub, correct, scrub run on
    /// one stream or in one captured graph.
    ///
    /// # Safety
    /// As `scrub_device`, with every `shards[i]` writable; `units` valid for
    /// `stripes * 4` bytes on this device.
    pub unsafe fn scrub_correct_device(&self, shards: &[*mut u8], shard_strides: &[usize], cell: usize,
                                       stripes: usize, results: *const ScrubResult, units: *mut i32,
                                       stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_correct_device(self.raw, shards.as_ptr(), shard_strides.as_ptr(), cell, stripes, results, units,
                                     stream)
        })
    }

    /// Device bytes `scrub_device_mixed` needs for `stripes` stripes.
    pub fn scrub_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_scrub_mixed_workspace_size(self.raw, stripes) }
    }

    /// Scrubs a batch of degraded stripes (`hec_scrub_device_mixed`):
    /// `present[s]` bit i = unit i of stripe s is there; the slots a stripe
    /// lacks are not read, but no `shards[i]` may be null.  Results as
    /// `scrub_device`, with the bits of a bad stripe's missing units set in
    /// `ruled_out`, so `scrub_verdict` works unchanged; a stripe with k units
    /// or fewer cannot be checked and gives (0, 0).  After a node loss: scrub
    /// with the masks, clear each `Located(t)` from its mask,
    /// `reconstruct_device_mixed` in place, scrub again.  `workspace` is device
    /// memory of `scrub_mixed_workspace_size(stripes)` bytes, untouched until
    /// `stream` has passed the call.
    ///
    /// # Safety
    /// As `scrub_device`; `workspace` valid for `workspace_bytes` on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn scrub_device_mixed(&self, shards: &[*const u8], shard_strides: &[usize], present: &[u64],
                                     cell: usize, results: *mut ScrubResult, workspace: *mut c_void,
                                     workspace_bytes: usize, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_device_mixed(self.raw, shards.as_ptr(), shard_strides.as_ptr(), present.as_ptr(), cell,
                                   present.len(), results, workspace, workspace_bytes, stream)
        })
    }

    /// `scrub_device` with the chunk checksums of every unit verified in the
    /// same pass (`hec_scrub_crc_device`): `expected` is `[stripe][k+m][nck]`
    /// big-endian u32 (4-byte aligned), `bad` is `[stripe][k+m]` flag bytes the
    /// caller zeroes; a unit that does not match its sums gets its flag set.
    /// `results` holds exactly what `scrub_device` returns; the two outputs are
    /// independent.  A flagged unit whose stripe scrubs clean with the unit
    /// included has a corrupt sum, not corrupt bytes.
    ///
    /// # Safety
    /// As `scrub_device`; `expected` and `bad` valid for their layouts on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn scrub_crc_device(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                   cell: usize, stripes: usize, bytes_per_checksum: usize, expected: *const u8,
                                   bad: *mut u8, results: *mut ScrubResult, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_crc_device(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(), cell,
                                 stripes, bytes_per_checksum, expected, bad, results, stream)
        })
    }

    /// Device bytes `scrub_crc_device_mixed` needs for `stripes` stripes.
    pub fn scrub_crc_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_scrub_crc_mixed_workspace_size(self.raw, stripes) }
    }

    /// `scrub_device_mixed` with the checksum buffers of `scrub_crc_device`
    /// (`hec_scrub_crc_device_mixed`): every present unit of every stripe is
    /// verified, also in stripes with k units or fewer; missing slots of the
    /// cells and of `expected` are never read.  `workspace` is device memory of
    /// `scrub_crc_mixed_workspace_size(stripes)` bytes (16-byte aligned),
    /// untouched until `stream` has passed the call.
    ///
    /// # Safety
    /// As `scrub_crc_device`; `workspace` valid for `workspace_bytes` on this device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn scrub_crc_device_mixed(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                         present: &[u64], cell: usize, bytes_per_checksum: usize,
                                         expected: *const u8, bad: *mut u8, results: *mut ScrubResult,
                                         workspace: *mut c_void, workspace_bytes: usize,
                                         stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_crc_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(),
                                       present.as_ptr(), cell, present.len(), bytes_per_checksum, expected, bad,
                                       results, workspace, workspace_bytes, stream)
        })
    }

    /// `scrub_crc_device` for a group whose last stripe is short
    /// (`hec_scrub_crc_rows_device`).  `data_len` as for
    /// `composite_crc_device` (0 = every stripe full): the last stripe is
    /// checked over its positions below n0 = min(cell, r) with every unit zero
    /// from its own length on, and every unit is verified over its own bytes;
    /// no slot byte at or past a unit's length is looked at.
    ///
    /// # Safety
    /// As `scrub_crc_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn scrub_crc_rows_device(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                        cell: usize, stripes: usize, bytes_per_checksum: usize, data_len: u64,
                                        expected: *const u8, bad: *mut u8, results: *mut ScrubResult,
                                        stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_scrub_crc_rows_device(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(), cell,
                                      stripes, bytes_per_checksum, data_len, expected, bad, results, stream)
        })
    }

    /// Device bytes `scrub_crc_rows_device_mixed` needs for `stripes` stripes.
    pub fn scrub_crc_rows_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_scrub_crc_rows_mixed_workspace_size(self.raw, stripes) }
    }

    /// `scrub_crc_device_mixed` with the logical bytes of every stripe
    /// (`hec_scrub_crc_rows_device_mixed`): `stripe_bytes` (`None` = every
    /// stripe full) has one entry per stripe, 0 or `k * cell` = that stripe is
    /// full.  `workspace` is device memory of
    /// `scrub_crc_rows_mixed_workspace_size(stripes)` bytes (16-byte aligned),
    /// untouched until `stream` has passed the call.
    ///
    /// # Safety
    /// As `scrub_crc_device_mixed`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn scrub_crc_rows_device_mixed(&self, checksum_type: i32, shards: &[*const u8],
                                              shard_strides: &[usize], present: &[u64], stripe_bytes: Option<&[u64]>,
                                              cell: usize, bytes_per_checksum: usize, expected: *const u8,
                                              bad: *mut u8, results: *mut ScrubResult, workspace: *mut c_void,
                                              workspace_bytes: usize, stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(stripe_bytes.map_or(true, |b| b.len() == present.len()), "one length per stripe");
        check(unsafe {
            hec_scrub_crc_rows_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(),
                                            present.as_ptr(), stripe_bytes.map_or(std::ptr::null(), |b| b.as_ptr()),
                                            cell, present.len(), bytes_per_checksum, expected, bad, results,
                                            workspace, workspace_bytes, stream)
        })
    }

    /// Parity and chunk sums of a group whose last stripe is short
    /// (`hec_encode_crc_rows_device`): `CellBuffer::encode` feeding
    /// `WritePacket::calculate_checksum` on the device.  `data_len` as for
    /// `composite_crc_device` (0 = every stripe full): the last stripe's
    /// parity units get their n0 = min(cell, r) bytes, nothing at or past n0
    /// is written, every unit gets the sums of its own bytes, and no data byte
    /// at or past a unit's length is looked at.
    ///
    /// # Safety
    /// `data[i] + s * data_strides[i]` (k units) and `parity[j] + s *
    /// parity_strides[j]` (m units) must be device memory of `cell` bytes for
    /// every stripe, `sums` device memory of `stripes * (k + m) * nck * 4`
    /// bytes, all valid until `stream` has passed the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn encode_crc_rows_device(&self, checksum_type: i32, data: &[*const u8], data_strides: &[usize],
                                         parity: &[*mut u8], parity_strides: &[usize], cell: usize, stripes: usize,
                                         bytes_per_checksum: usize, data_len: u64, sums: *mut u8,
                                         stream: *mut c_void) -> Result<()> {
        assert!(data.len() == self.data_units && data_strides.len() == self.data_units, "one slot per data unit");
        assert!(parity.len() == self.parity_units && parity_strides.len() == self.parity_units,
                "one slot per parity unit");
        check(unsafe {
            hec_encode_crc_rows_device(self.raw, checksum_type as c_int, data.as_ptr(), data_strides.as_ptr(),
                                       parity.as_ptr(), parity_strides.as_ptr(), cell, stripes, bytes_per_checksum,
                                       data_len, sums, stream)
        })
    }

    /// Device bytes `encode_crc_rows_device_mixed` needs for `stripes` stripes.
    pub fn encode_crc_rows_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_encode_crc_rows_mixed_workspace_size(self.raw, stripes) }
    }

    /// `encode_crc_rows_device` with the logical bytes of every stripe
    /// (`hec_encode_crc_rows_device_mixed`): `stripe_bytes` (`None` = every
    /// stripe full) has one entry per stripe, 0 or `k * cell` = that stripe is
    /// full.  `workspace` is device memory of
    /// `encode_crc_rows_mixed_workspace_size(stripes)` bytes (8-byte aligned),
    /// needed only when a stripe is short and untouched until `stream` has
    /// passed the call.
    ///
    /// # Safety
    /// As `encode_crc_rows_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn encode_crc_rows_device_mixed(&self, checksum_type: i32, data: &[*const u8],
                                               data_strides: &[usize], parity: &[*mut u8],
                                               parity_strides: &[usize], stripe_bytes: Option<&[u64]>, cell: usize,
                                               stripes: usize, bytes_per_checksum: usize, sums: *mut u8,
                                               workspace: *mut c_void, workspace_bytes: usize,
                                               stream: *mut c_void) -> Result<()> {
        assert!(data.len() == self.data_units && data_strides.len() == self.data_units, "one slot per data unit");
        assert!(parity.len() == self.parity_units && parity_strides.len() == self.parity_units,
                "one slot per parity unit");
        assert!(stripe_bytes.map_or(true, |b| b.len() == stripes), "one length per stripe");
        check(unsafe {
            hec_encode_crc_rows_device_mixed(self.raw, checksum_type as c_int, data.as_ptr(), data_strides.as_ptr(),
                                             parity.as_ptr(), parity_strides.as_ptr(),
                                             stripe_bytes.map_or(std::ptr::null(), |b| b.as_ptr()), cell, stripes,
                                             bytes_per_checksum, sums, workspace, workspace_bytes, stream)
        })
    }

    /// Verified striped read into a file-order buffer
    /// (`hec_read_crc_rows_device`): `StripedBlockStream::read_slice` on the
    /// device.  `shards[k + m]` (null = lost for the batch); the survivors are
    /// verified against `expected` (null = no verification) with flags set in
    /// `bad`, the lost data units rebuilt, and data unit u of stripe s written
    /// to `file + s * file_stride + u * cell` (`file_stride` 0 = `k * cell`)
    /// for its own length.  `data_len` as for `encode_crc_rows_device`; nothing
    /// at or past a stripe's logical end is written.
    ///
    /// # Safety
    /// `shards[i] + s * shard_strides[i]` must be device memory of `cell`
    /// bytes for every present unit and stripe, `file` device memory that
    /// covers every row's logical bytes and overlaps no shard slot,
    /// `expected` / `bad` device memory of `stripes * (k + m) * nck * 4` /
    /// `stripes * (k + m)` bytes, all valid until `stream` has passed the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn read_crc_rows_device(&self, checksum_type: i32, shards: &[*const u8], shard_strides: &[usize],
                                       file: *mut u8, file_stride: usize, cell: usize, stripes: usize,
                                       bytes_per_checksum: usize, data_len: u64, expected: *const u8, bad: *mut u8,
                                       stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        check(unsafe {
            hec_read_crc_rows_device(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(), file,
                                     file_stride, cell, stripes, bytes_per_checksum, data_len, expected, bad, stream)
        })
    }

    /// Device bytes `read_crc_rows_device_mixed` needs for `stripes` stripes.
    pub fn read_crc_rows_mixed_workspace_size(&self, stripes: usize) -> usize {
        unsafe { hec_read_crc_rows_mixed_workspace_size(self.raw, stripes) }
    }

    /// `read_crc_rows_device` with one presence mask and the logical bytes of
    /// every stripe (`hec_read_crc_rows_device_mixed`): bit i of `present[s]`
    /// = unit i of stripe s is present; `stripe_bytes` (`None` = every stripe
    /// full) has one entry per stripe, 0 or `k * cell` = that stripe is full.
    /// `workspace` is device memory of
    /// `read_crc_rows_mixed_workspace_size(stripes)` bytes (8-byte aligned),
    /// always needed and untouched until `stream` has passed the call.
    ///
    /// # Safety
    /// As `read_crc_rows_device`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn read_crc_rows_device_mixed(&self, checksum_type: i32, shards: &[*const u8],
                                             shard_strides: &[usize], file: *mut u8, file_stride: usize,
                                             present: &[u64], stripe_bytes: Option<&[u64]>, cell: usize,
                                             bytes_per_checksum: usize, expected: *const u8, bad: *mut u8,
                                             workspace: *mut c_void, workspace_bytes: usize,
                                             stream: *mut c_void) -> Result<()> {
        let n = self.data_units + self.parity_units;
        assert!(shards.len() == n && shard_strides.len() == n, "one slot per unit");
        assert!(stripe_bytes.map_or(true, |b| b.len() == present.len()), "one length per stripe");
        check(unsafe {
            hec_read_crc_rows_device_mixed(self.raw, checksum_type as c_int, shards.as_ptr(), shard_strides.as_ptr(),
                                           file, file_stride, present.as_ptr(),
                                           stripe_bytes.map_or(std::ptr::null(), |b| b.as_ptr()), cell, present.len(),
                                           bytes_per_checksum, expected, bad, workspace, workspace_bytes, stream)
        })
    }

    /// `hec_crc_concat`: crc(A || B) from crc(A), crc(B) and |B|.
    pub fn crc_concat(checksum_type: i32, crc_a: u32, crc_b: u32, len_b: u64) -> Result<u32> {
        let mut out = 0u32;
        check(unsafe { hec_crc_concat(checksum_type as c_int, crc_a, crc_b, len_b, &mut out) })?;
        Ok(out)
    }

    /// `hec_composite_crc` on the host: the CRC of every cell (`[stripes][n_units]`),
    /// of every internal block (`[n_units]`) and of the `data_len` logical
    /// bytes, from the `[stripes][n_units][nck]` big-endian chunk sums.
    /// `data_len == 0` means every stripe is full.
    #[allow(clippy::too_many_arguments)]
    pub fn composite_crc(checksum_type: i32, sums: &[u8], n_units: usize, data_units: usize, cell: usize,
                         stripes: usize, bytes_per_checksum: usize, data_len: u64)
                         -> Result<(Vec<u32>, Vec<u32>, u32)> {
        assert!(cell > 0 && bytes_per_checksum > 0, "cell and bytes_per_checksum must be positive");
        let nck = cell.div_ceil(bytes_per_checksum);
        assert!(sums.len() >= 4 * stripes * n_units * nck, "one u32 per chunk slot");
        let mut cells = vec![0u8; 4 * stripes * n_units];
        let mut units = vec![0u8; 4 * n_units];
        let mut group = [0u8; 4];
        check(unsafe {
            hec_composite_crc(checksum_type as c_int, sums.as_ptr(), n_units, data_units, cell, stripes,
                              bytes_per_checksum, data_len, cells.as_mut_ptr(), units.as_mut_ptr(),
                              group.as_mut_ptr())
        })?;
        let words = |b: &[u8]| b.chunks_exact(4).map(|w| u32::from_be_bytes([w[0], w[1], w[2], w[3]])).collect();
        Ok((words(&cells), words(&units), u32::from_be_bytes(group)))
    }

    /// Device bytes `composite_crc_device` needs for its unit and group outputs.
    pub fn composite_crc_workspace_size(n_units: usize, stripes: usize) -> usize {
        unsafe { hec_composite_crc_workspace_size(n_units, stripes) }
    }

    /// `hec_composite_crc_device`: the same fold on this coder's device,
    /// asynchronously on `stream`, over chunk sums already there (as the
    /// verified calls leave them).  Each output is optional (null = not
    /// computed); `workspace` is needed for `unit_crcs` and `group_crc`.
    ///
    /// # Safety
    /// `sums` valid for `stripes * n_units * ceil(cell / bytes_per_checksum)`
    /// u32, the outputs for `stripes * n_units`, `n_units` and one u32,
    /// `workspace` for `workspace_bytes`, all on this device and 4-byte aligned.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn composite_crc_device(&self, checksum_type: i32, sums: *const u8, n_units: usize,
                                       data_units: usize, cell: usize, stripes: usize, bytes_per_checksum: usize,
                                       data_len: u64, cell_crcs: *mut u8, unit_crcs: *mut u8, group_crc: *mut u8,
                                       workspace: *mut c_void, workspace_bytes: usize,
                                       stream: *mut c_void) -> Result<()> {
        check(unsafe {
            hec_composite_crc_device(self.raw, checksum_type as c_int, sums, n_units, data_units, cell, stripes,
                                     bytes_per_checksum, data_len, cell_crcs, unit_crcs, group_crc, workspace,
                                     workspace_bytes, stream)
        })
    }

    /// `hec_scrub` on host buffers: one stripe whose k+m units are all
    /// present, any length >= 1; always the engine's host routine.
    pub fn scrub(&self, units: &[Bytes]) -> Result<ScrubResult> {
        let n = self.data_units + self.parity_units;
        assert!(units.len() == n, "one buffer per unit");
        let len = units[0].len();
        assert!(units.iter().all(|u| u.len() == len), "equal unit lengths");
        let ptrs: Vec<*const u8> = units.iter().map(|u| u.as_ptr()).collect();
        let mut out = ScrubResult::default();
        check(unsafe { hec_scrub(self.raw, ptrs.as_ptr(), len, &mut out) })?;
        Ok(out)
    }

    /// Waits for `stream` (null = the default stream) on the coder's device.
    pub fn synchronize(&self, stream: *mut c_void) -> Result<()> {
        check(unsafe { hec_device_synchronize(self.device, stream) })
    }

    /// `Coder::encode` (gf256.rs:61-80): m freshly allocated parity shards.
    pub fn encode(&self, data: &[Bytes]) -> Vec<Bytes> {
        encode_raw(self.raw, self.data_units, self.parity_units, data)
    }

    /// `Coder::decode` (gf256.rs:84-137): rebuilds every missing data slot.
    pub fn decode(&self, data: &mut [Option<Bytes>]) -> Result<()> {
        decode_raw(self.raw, self.data_units, self.parity_units, data)
    }

    /// Hadoop's `RSRawDecoder.decode` (`hec_reconstruct`): rebuilds every
    /// missing slot, data or parity, that `want` names (`None` = all of
    /// them); the reference's `decode` above leaves parity `None`.
    pub fn reconstruct(&self, data: &mut [Option<Bytes>], want: Option<&[usize]>) -> Result<()> {
        reconstruct_raw(self.raw, self.data_units, self.parity_units, data, want)
    }

    /// A whole file in file order (rows of k cells, the last one possibly
    /// short: `CellBuffer::write` / `encode`, block_writer.rs:791-851) ->
    /// `parity` = ceil(len / (k*cell)) rows of m cells; the short row's parity
    /// cells hold len(cell 0) bytes, zero past them.
    pub fn encode_file(&self, data: &[u8], cell: usize, parity: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(cell > 0, "cell_len > 0");
        let rows = data.len().div_ceil(k * cell);
        assert!(parity.len() >= rows * m * cell, "parity holds ceil(len / row) * m cells");
        check(unsafe { hec_encode_rows_host(self.raw, data.as_ptr(), data.len(), parity.as_mut_ptr(), cell, 16) })
    }

    /// The blocks of one block group (`vertical[i]` = shard i's block, any
    /// length up to its `max_offset`; `None` = failed reader) -> the file's
    /// `file.len()` bytes, short and absent cells read as zeros
    /// (`CellReader::next_cell`, block_reader.rs:343-378).
    pub fn decode_file(&self, vertical: &[Option<&[u8]>], cell: usize, file: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert_eq!(vertical.len(), k + m, "one slot per shard");
        assert!(cell > 0, "cell_len > 0");
        let ptrs: Vec<*const u8> = vertical.iter().map(|v| v.map_or(std::ptr::null(), |b| b.as_ptr())).collect();
        let lens: Vec<usize> = vertical.iter().map(|v| v.map_or(0, <[u8]>::len)).collect();
        check(unsafe {
            hec_decode_rows_host(self.raw, ptrs.as_ptr(), lens.as_ptr(), cell, file.as_mut_ptr(), file.len(), 16)
        })
    }

    /// N full rows in file order (row r = `rows[r*k*cell ..]`) -> N x m
    /// parity cells, one pinned H2D / encode / D2H pipeline instead of N
    /// `CellBuffer::encode` calls (block_writer.rs:838).
    pub fn encode_rows(&self, rows: &[u8], cell: usize, parity: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(cell > 0 && rows.len() % (k * cell) == 0, "whole rows of k cells");
        let n = rows.len() / (k * cell);
        assert!(parity.len() >= n * m * cell, "parity holds n * m cells");
        check(unsafe { hec_encode_host_batch(self.raw, rows.as_ptr(), parity.as_mut_ptr(), cell, n, 16) })
    }

    /// Reader side: `vertical[i]` holds `n` consecutive cells of shard i
    /// (`None` = failed reader); `file` receives n rows of k cells in file
    /// order with lost cells rebuilt -- n `ec_decode` calls (ec/mod.rs:62-89).
    pub fn decode_rows(&self, vertical: &[Option<&[u8]>], cell: usize, n: usize, file: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert_eq!(vertical.len(), k + m, "one slot per shard");
        assert!(cell > 0, "cell_len > 0");
        assert!(vertical.iter().flatten().all(|v| v.len() >= n * cell), "every shard holds n cells");
        assert!(file.len() >= n * k * cell, "file holds n rows");
        let ptrs: Vec<*const u8> = vertical.iter().map(|v| v.map_or(std::ptr::null(), |b| b.as_ptr())).collect();
        check(unsafe { hec_decode_host_batch(self.raw, ptrs.as_ptr(), cell, n, file.as_mut_ptr(), 16) })
    }

    /// Verified striped read of `rows` rows already on the device
    /// (`block_reader.rs:480-525` + `ReadPacket::get_data`): shard i of row r
    /// at `shards[i] + r * strides[i]` (null = no reader); `sums` holds the
    /// packets' checksums `[row][k+m][chunk]` big-endian.  Missing or failed
    /// data cells are rebuilt into `out[i]` (may be `shards[i]` itself: in-
    /// place repair); `bad[r*(k+m)+i] = 1` marks the cells that failed.
    ///
    /// # Safety
    /// Every pointer is a device pointer valid for the layout above, and the
    /// stream belongs to the coder's device.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn decode_verified(&self, checksum_type: i32, shards: &[*const u8], strides: &[usize],
                                  out: &[*mut u8], out_strides: &[usize], cell: usize, rows: usize,
                                  bytes_per_checksum: usize, sums: *const u8, bad: *mut u8,
                                  stream: *mut c_void) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(shards.len() == k + m && strides.len() == k + m, "one slot per shard");
        assert!(out.len() == k && out_strides.len() == k, "one output slot per data shard");
        check(unsafe {
            hec_decode_verify_device(self.raw, checksum_type, shards.as_ptr(), strides.as_ptr(), out.as_ptr(),
                                     out_strides.as_ptr(), cell, rows, bytes_per_checksum, sums, bad, stream)
        })
    }
}

/// HBM on one device (`hec_device_alloc`), freed on drop: the stripe
/// buffers of `encode_device` / `decode_device` for a caller (the `mi355x`
/// Criterion group of rust/benches/ec.rs) with no HIP binding of its own.
pub struct DeviceBuffer {
    device: i32,
    ptr: *mut u8,
    len: usize,
}

unsafe impl Send for DeviceBuffer {}
unsafe impl Sync for DeviceBuffer {}

impl DeviceBuffer {
    pub fn new(device: i32, len: usize) -> Result<Self> {
        let mut p = std::ptr::null_mut();
        check(unsafe { hec_device_alloc(device, len, 0, &mut p) })?;
        Ok(Self { device, ptr: p.cast(), len })
    }

    /// A buffer holding a copy of `host`.
    pub fn upload(device: i32, host: &[u8]) -> Result<Self> {
        let b = Self::new(device, host.len())?;
        check(unsafe { hec_device_copy(device, b.ptr.cast(), host.as_ptr().cast(), host.len()) })?;
        Ok(b)
    }

    /// Copies the buffer into `host` (`host.len()` bytes from its start).
    pub fn download(&self, host: &mut [u8]) -> Result<()> {
        assert!(host.len() <= self.len, "read past the buffer");
        check(unsafe { hec_device_copy(self.device, host.as_mut_ptr().cast(), self.ptr.cast(), host.len()) })
    }

    /// Device address of byte `off`.
    pub fn at(&self, off: usize) -> *mut u8 {
        assert!(off <= self.len, "offset past the buffer");
        self.ptr.wrapping_add(off)
    }

    pub fn len(&self) -> usize {
        self.len
    }

    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
}

impl Drop for DeviceBuffer {
    fn drop(&mut self) {
        unsafe { hec_device_free(self.device, self.ptr.cast()) };
    }
}

impl Drop for GpuCoder {
    fn drop(&mut self) {
        unsafe { hec_coder_destroy(self.raw) }
    }
}

fn encode_raw(raw: *mut HecCoder, k: usize, m: usize, data: &[Bytes]) -> Vec<Bytes> {
    assert_eq!(data.len(), k, "data.len() == data_units (gf256.rs:62)");
    let n = data[0].len();
    assert!(n > 0, "shards must not be empty (matrix.rs:57)");
    assert!(data.iter().all(|s| s.len() == n), "equal shard lengths (gf256.rs:65)");
    let mut parity: Vec<BytesMut> = (0..m).map(|_| BytesMut::zeroed(n)).collect();
    let ins: Vec<*const u8> = data.iter().map(|d| d.as_ptr()).collect();
    let outs: Vec<*mut u8> = parity.iter_mut().map(|p| p.as_mut_ptr()).collect();
    let rc = unsafe { hec_encode(raw, ins.as_ptr(), n, outs.as_ptr()) };
    // the reference encode cannot fail; a device error here is a bug or a lost GPU
    assert_eq!(rc, HEC_OK, "hec_encode: {}", err(rc));
    parity.into_iter().map(BytesMut::freeze).collect()
}

fn decode_raw(raw: *mut HecCoder, k: usize, m: usize, data: &mut [Option<Bytes>]) -> Result<()> {
    assert_eq!(data.len(), k + m, "data.len() == data_units + parity_units");
    if data.iter().take(k).all(Option::is_some) {
        return Ok(()); // gf256.rs:102-105
    }
    let n = match data.iter().flatten().next() {
        Some(b) => b.len(),
        None => return Err(err(HEC_ERR_NOT_ENOUGH_SHARDS)),
    };
    // the engine reads n bytes from each of the first k present shards (the
    // survivors it decodes from): hold the reference's equal-length
    // precondition over exactly those (matrix.rs:212-216 asserts it over the
    // k selected rows only; a longer or shorter shard past them is not read)
    assert!(n > 0, "shards must not be empty (matrix.rs:57)");
    assert!(data.iter().flatten().take(k).all(|b| b.len() == n), "equal shard lengths (matrix.rs:215)");
    let ins: Vec<*const u8> = data.iter().map(|d| d.as_ref().map_or(std::ptr::null(), |b| b.as_ptr())).collect();
    let mut rec: Vec<Option<BytesMut>> =
        (0..k + m).map(|i| (i < k && data[i].is_none()).then(|| BytesMut::zeroed(n))).collect();
    // parity slots (and present data slots) pass null: never written
    let outs: Vec<*mut u8> =
        rec.iter_mut().map(|r| r.as_mut().map_or(std::ptr::null_mut(), |b| b.as_mut_ptr())).collect();
    check(unsafe { hec_decode(raw, ins.as_ptr(), n, outs.as_ptr()) })?;
    for (i, r) in rec.into_iter().enumerate() {
        if let Some(b) = r {
            data[i] = Some(b.freeze());
        }
    }
    Ok(())
}

fn want_flags(n: usize, want: &[usize]) -> Vec<u8> {
    let mut flags = vec![0u8; n];
    for &t in want {
        assert!(t < n, "want names unit {t} of {n}");
        flags[t] = 1;
    }
    flags
}

/// `hec_reconstruct_plan` (host only, no device): `(survivors, targets,
/// matrix)` for rebuilding the missing units of `present` that `want` names
/// (`None` = all of them); `matrix` holds one row of k coefficients per target.
pub fn reconstruct_plan(codec: &str, data_units: usize, parity_units: usize, present: &[bool],
                        want: Option<&[usize]>) -> Result<(Vec<usize>, Vec<usize>, Vec<u8>)> {
    let (k, n) = (data_units, data_units + parity_units);
    assert_eq!(present.len(), n, "present.len() == data_units + parity_units");
    let name = std::ffi::CString::new(codec).map_err(|_| HdfsError::InvalidArgument(codec.to_string()))?;
    let pres: Vec<u8> = present.iter().map(|&p| p as u8).collect();
    let flags = want.map(|w| want_flags(n, w));
    let (mut nt, mut surv, mut targets, mut matrix) = (0usize, vec![0usize; k], vec![0usize; n], vec![0u8; n * k]);
    check(unsafe {
        hec_reconstruct_plan(name.as_ptr(), data_units, parity_units, pres.as_ptr(),
                             flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), &mut nt, surv.as_mut_ptr(),
                             targets.as_mut_ptr(), matrix.as_mut_ptr())
    })?;
    if nt == 0 {
        surv.clear();
    }
    targets.truncate(nt);
    matrix.truncate(nt * k);
    Ok((surv, targets, matrix))
}

fn reconstruct_raw(raw: *mut HecCoder, k: usize, m: usize, data: &mut [Option<Bytes>],
                   want: Option<&[usize]>) -> Result<()> {
    assert_eq!(data.len(), k + m, "data.len() == data_units + parity_units");
    let flags = want.map(|w| want_flags(k + m, w));
    let target = |i: usize| data[i].is_none() && flags.as_ref().map_or(true, |f| f[i] != 0);
    if !(0..k + m).any(target) {
        // a want on a present unit is the engine's HEC_ERR_INVALID_ARG
        if let Some(f) = &flags {
            if (0..k + m).any(|i| f[i] != 0 && data[i].is_some()) {
                return Err(err(HEC_ERR_INVALID_ARG));
            }
        }
        return Ok(());
    }
    let n = match data.iter().flatten().next() {
        Some(b) => b.len(),
        None => return Err(err(HEC_ERR_NOT_ENOUGH_SHARDS)),
    };
    assert!(n > 0, "shards must not be empty (matrix.rs:57)");
    assert!(data.iter().flatten().take(k).all(|b| b.len() == n), "equal shard lengths (matrix.rs:215)");
    let ins: Vec<*const u8> = data.iter().map(|d| d.as_ref().map_or(std::ptr::null(), |b| b.as_ptr())).collect();
    let mut rec: Vec<Option<BytesMut>> = (0..k + m).map(|i| target(i).then(|| BytesMut::zeroed(n))).collect();
    let outs: Vec<*mut u8> =
        rec.iter_mut().map(|r| r.as_mut().map_or(std::ptr::null_mut(), |b| b.as_mut_ptr())).collect();
    check(unsafe {
        hec_reconstruct(raw, ins.as_ptr(), n, flags.as_ref().map_or(std::ptr::null(), |f| f.as_ptr()), outs.as_ptr())
    })?;
    for (i, r) in rec.into_iter().enumerate() {
        if let Some(b) = r {
            data[i] = Some(b.freeze());
        }
    }
    Ok(())
}

/// The engine coder behind the reference's `Coder` when the `mi355x` feature
/// forwards it (rust/patches/ec_mi355x.patch): `Coder::new` acquires one from
/// the process-wide pool, drop releases it.  `Coder::new` runs per decoded
/// row (ec/mod.rs:71) and per block writer (block_writer.rs:787), so a pool
/// hit costs a mutex and a vector pop -- no streams, events or buffers are
/// created (`tests/cpp/shim_replay.c` times 10,000 cycles).  The device is
/// `HDFS_EC_AMD_DEVICE` if set, else any (round-robin over the visible GPUs;
/// an engine host-only coder, `HEC_DEVICE_HOST`, when none is visible).  When
/// the device coder cannot be had (a bad `HDFS_EC_AMD_DEVICE`, device memory
/// exhausted) `acquire` falls back to a host-only coder, so only a library
/// that cannot allocate at all returns an error -- which the patched
/// `Coder::new` turns into its reference CPU path.
/// Rows below the coder's host limit are coded on the calling thread.
pub struct PooledCoder {
    raw: *mut HecCoder,
    data_units: usize,
    parity_units: usize,
}

unsafe impl Send for PooledCoder {}
unsafe impl Sync for PooledCoder {}

impl PooledCoder {
    pub fn acquire(codec: &str, data_units: usize, parity_units: usize) -> Result<Self> {
        assert_eq!(unsafe { hec_abi_version() }, ABI_VERSION, "libhdfs_ec_amd ABI mismatch");
        let device: i32 =
            std::env::var("HDFS_EC_AMD_DEVICE").ok().and_then(|v| v.parse().ok()).unwrap_or(-1);
        let name = std::ffi::CString::new(codec).map_err(|_| HdfsError::InvalidArgument(codec.to_string()))?;
        let mut raw = std::ptr::null_mut();
        let rc = unsafe { hec_coder_acquire(name.as_ptr(), data_units, parity_units, device, &mut raw) };
        if rc != HEC_OK {
            if rc == HEC_ERR_INVALID_ARG || rc == HEC_ERR_UNSUPPORTED_CODEC {
                return Err(err(rc));
            }
            log::warn!("MI355X EC engine: device coder unavailable ({}), host-only coder", err(rc));
            check(unsafe { hec_coder_acquire(name.as_ptr(), data_units, parity_units, HEC_DEVICE_HOST, &mut raw) })?;
        }
        Ok(Self { raw, data_units, parity_units })
    }

    /// True when this coder runs on the engine's host routine (no GPU).
    pub fn host_only(&self) -> bool {
        unsafe { hec_coder_device(self.raw) == HEC_DEVICE_HOST }
    }

    pub fn encode(&self, data: &[Bytes]) -> Vec<Bytes> {
        encode_raw(self.raw, self.data_units, self.parity_units, data)
    }

    pub fn decode(&self, data: &mut [Option<Bytes>]) -> Result<()> {
        decode_raw(self.raw, self.data_units, self.parity_units, data)
    }
}

impl Drop for PooledCoder {
    fn drop(&mut self) {
        unsafe { hec_coder_release(self.raw) }
    }
}

/// All GPUs of a node from one client process: a batch split into
/// contiguous stripe ranges, one device and host thread each, no collective
/// (stripes are independent).
pub struct GpuGroup {
    raw: *mut HecGroup,
    data_units: usize,
    parity_units: usize,
}

unsafe impl Send for GpuGroup {}
unsafe impl Sync for GpuGroup {}

impl GpuGroup {
    pub fn new(codec: &str, data_units: usize, parity_units: usize, devices: &[i32]) -> Result<Self> {
        assert_eq!(unsafe { hec_abi_version() }, ABI_VERSION, "libhdfs_ec_amd ABI mismatch");
        let name = std::ffi::CString::new(codec).map_err(|_| HdfsError::InvalidArgument(codec.to_string()))?;
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            hec_group_create(name.as_ptr(), data_units, parity_units, devices.as_ptr(), devices.len(), &mut raw)
        })?;
        Ok(Self { raw, data_units, parity_units })
    }

    /// `GpuCoder::encode_rows` across every GPU of the group.
    pub fn encode_rows(&self, rows: &[u8], cell: usize, parity: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert!(cell > 0 && rows.len() % (k * cell) == 0, "whole rows of k cells");
        let n = rows.len() / (k * cell);
        assert!(parity.len() >= n * m * cell, "parity holds n * m cells");
        check(unsafe { hec_group_encode_host_batch(self.raw, rows.as_ptr(), parity.as_mut_ptr(), cell, n, 16) })
    }

    /// `GpuCoder::decode_rows` across every GPU of the group.
    pub fn decode_rows(&self, vertical: &[Option<&[u8]>], cell: usize, n: usize, file: &mut [u8]) -> Result<()> {
        let (k, m) = (self.data_units, self.parity_units);
        assert_eq!(vertical.len(), k + m, "one slot per shard");
        assert!(vertical.iter().flatten().all(|v| v.len() >= n * cell), "every shard holds n cells");
        assert!(file.len() >= n * k * cell, "file holds n rows");
        let ptrs: Vec<*const u8> = vertical.iter().map(|v| v.map_or(std::ptr::null(), |b| b.as_ptr())).collect();
        check(unsafe { hec_group_decode_host_batch(self.raw, ptrs.as_ptr(), cell, n, file.as_mut_ptr(), 16) })
    }
}

impl Drop for GpuGroup {
    fn drop(&mut self) {
        unsafe { hec_group_destroy(self.raw) }
    }
}
