// CDNA4 (gfx950) kernels for the chunk data path.
//   K1/K2  crc_slices_kernel  : per-512B-slice CRC32 (big-endian .meta image) fused with the
//                               whole-block CRC (shift-combine tree, per-workgroup partials).
//   K3     same kernel in range/verify mode: recompute only touched slices and compare with
//          the HBM-resident .meta image (reference verify_partial_read, chunkserver.rs:296-351).
//   K1b    crc_scrub_kernel: one launch verifies every resident block against its .meta.
//   K4/K5  gf256_matmul_kernel: GF(2^8) matrix x shards (Reed-Solomon encode / reconstruct;
//          reference erasure.rs:7-49).
//   K4/K5 + K2  ec_fused_kernel: a whole RS stripe in one pass — the shards are landed (encode),
//          multiplied and checksummed from the registers they were loaded or computed in.
//   K4 + K2 of a resident block  ec_convert_kernel: the tiering conversion — the block's columns
//          are loaded at their byte shifts, zero-padded behind the block's end, and leave as k + m
//          stored and checksummed shards in the fused kernel's encode form.
//   K5 + range read  ec_read_kernel: a byte range of an RS-coded file whose data shards are partly
//          lost — only the lost columns inside the range are rebuilt, and the bytes go from the
//          registers over PCIe into the reader's registered buffer.
//   K7     sse_gcm_kernel: the AES-256-GCM of SSE-S3 over a body in registered host memory — CTR
//          keystream from a T-table in LDS, XOR in place, and the GHASH of the ciphertext as
//          per-workgroup partials that the host folds into the tag.
//   K7 read  sse_read_kernel: a GET of an SSE-S3 object in one pass over its stored blob in HBM —
//          the slices verified on the matrix cores, the ciphertext authenticated and decrypted in
//          registers, and only the plaintext stored over PCIe into the reader's registered buffer.
//   K7 range read  sse_read_range_kernel: a Range GET of an SSE-S3 object — every tile of the blob
//          verified and authenticated as above, the CTR keystream computed and the plaintext stored
//          only for the tiles that hold bytes of the range.
//   K7 write  sse_write_kernel: a PUT of an SSE-S3 object in one pass over the gateway's slot — the
//          plaintext loaded over PCIe, encrypted and authenticated in registers, the slices
//          checksummed on the matrix cores, and the blob stored to its HBM extent and back in place.
//   K7 copy  sse_rekey_kernel: a CopyObject of an SSE-S3 object in one pass from one HBM extent to
//          another — the source's slices verified and its ciphertext authenticated, both keystreams
//          XORed into it in registers, the new ciphertext authenticated, checksummed and stored.
//   K7 + K5 read  sse_ec_read_kernel: a GET of an SSE-S3 object held as RS(k, m) shards — the k
//          surviving shards loaded as the blob they spell (lost columns rebuilt in registers), the
//          ciphertext authenticated and decrypted there, and only the plaintext stored over PCIe.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcm_host.h"

namespace dfs {

constexpr int kCrcWgThreads = 256;
constexpr int kSlicesPerTile = 32;  // 4 waves x 8 slices x 512 B = 16 KiB per tile
constexpr int kMaxGridCrc = 768;  // 3 resident workgroups x 256 CUs (see crc_tile_mfma_kernel)
constexpr int kMaxShards = 32;
constexpr int kCrcBasisBytes = 16 * 64 * 16;  // MFMA basis (A fragments), stored after DevCrcTables
constexpr int kCrcChunkShiftBytes = 7 * 4 * 256 * 4;  // chunk -> slice shift tables, stored after the basis
// behind those: slice -> 4 KiB sub-tile shift tables (7) and the 16 KiB tile shift (wide kernel)
constexpr int kCrcWideExtraBytes = 8 * 4 * 256 * 4;
// behind those: the basis of the FP4 matrix-core form (8 A fragments of 16 B per lane)
constexpr int kCrcBasisFp4Bytes = 8 * 64 * 16;
constexpr int kCrcBasisFp4Offset = kCrcBasisBytes + kCrcChunkShiftBytes + kCrcWideExtraBytes;  // after DevCrcTables
// behind those: the AES tables of sse_gcm_kernel (Te0, 256 words, then the S-box, 256 bytes)
constexpr int kSseTablesOffset = kCrcBasisFp4Offset + kCrcBasisFp4Bytes;
constexpr int kSseTablesBytes = 256 * 4 + 256;

struct DevCrcTables {
  uint32_t slice16[16][256];
  uint32_t sh64[4][256], sh128[4][256], sh256[4][256];  // lane combine inside a slice
  uint32_t sh512[4][256], sh1k[4][256], sh2k[4][256];   // slice combine inside a wave
  uint32_t sh4k[4][256];                                 // wave combine inside a workgroup
  uint32_t tile_pow2[32][32];                            // GF(2) matrices: 16 KiB * 2^b
};

struct CrcLaunch {
  const uint8_t* data;
  uint64_t n;
  uint64_t s_full;      // number of full 512 B slices in the block
  uint64_t slice_lo;    // first full slice processed
  uint64_t slice_hi;    // one past last full slice processed
  uint64_t vfront;      // virtual leading zero slices (aligns block combine to tiles)
  uint64_t ntiles;      // virtual tiles covering [slice_lo - vfront, slice_hi)
  uint32_t full_init;   // S(512)
  uint32_t has_tail;    // process the short tail slice (index s_full)
  uint32_t tail_len;
  uint32_t tail_init;   // S(tail_len)
  uint32_t* meta_out;             // BE CRC per slice (nullable)
  const uint32_t* meta_expect;    // BE CRC per slice to verify against (nullable)
  uint32_t* part_crc;             // [grid] raw shifted partials for whole-block CRC (nullable)
  uint32_t* part_bad;             // [grid] min mismatching slice index, 0xFFFFFFFF = none
  // device view of host-visible memory that receives a copy of meta_out (nullable; honoured
  // only by the LDS kernel, see crc_meta_host_ok): the .meta image needs no readback copy
  uint32_t* meta_host;
};

// K1b: one launch verifies many resident blocks against their HBM .meta images. Blocks are
// laid out on a global tile axis (tile_start = prefix sum of ceil(s_full / 32)); each
// workgroup finds its block by binary search, so every tile of every block is one
// grid-stride step and the LDS table fill is paid once per workgroup per launch.
struct ScrubBlock {
  const uint8_t* data;
  const uint32_t* meta;  // BE CRC per slice (HBM-resident .meta image)
  uint64_t s_full;
  uint64_t tile_start;
  uint32_t tail_len;
  uint32_t tail_init;
};

struct ScrubLaunch {
  const ScrubBlock* blocks;  // device, sorted by tile_start
  uint32_t nblocks;
  uint64_t ntiles;
  uint32_t full_init;
  uint32_t* bad;  // [nblocks] min mismatching slice index, pre-set to 0xFFFFFFFF
};

struct GfLaunch {
  const uint8_t* in[kMaxShards];
  uint8_t* out[kMaxShards];
  uint64_t len;   // bytes per shard (buffers padded to 16 B)
  int k;          // inputs
  int rows;       // outputs
  const uint32_t* tables;  // device: [rows][k] x 8 dwords, split-nibble product tables (gf_nibble_tables)
};
// Host: split-nibble tables of a rows x k coefficient matrix (poly 0x11D): per (r, c) the
// 16 products of the low nibble, then the 16 of the high nibble, 32 bytes.
void gf_nibble_tables(const uint8_t* mat, int rows, int k, uint32_t* out);

// Upload tables once per device (LDS image followed by the MFMA basis). Returns device pointer.
// K1/K2/K1b use the matrix-core chunk CRC unless DFS_CRC_MFMA=0 (the LDS slicing-by-16 path).
bool crc_mfma_enabled();
void set_crc_mfma(bool on);  // benchmarks / tests: pick the K1 implementation
// K1/K2 blocks below this many MiB run the LDS-table kernel even with the matrix-core path
// enabled (size-based dispatch; DFS_CRC_LDS_MAX_MIB, 0 = always the matrix cores).
constexpr int kCrcLdsMaxMibDefault = 16;
void set_crc_lds_max_mib(int mib);
DevCrcTables* upload_crc_tables(hipStream_t s);
int crc_grid_for(uint64_t ntiles, uint32_t has_tail);
// Tile buffers per wave in the MFMA kernels' register ring (2..4; 2 = the 3-waves/SIMD
// kernels, 3..4 = the deep-ring kernels at 2 waves/SIMD). Measured (profiles/archive/r2_crc3): the
// K1b scrub gains ~19 % from 3 buffers; K1/K2 does not (its per-tile combine work, not load
// latency, is what the third wave hides), so it keeps 2. DFS_CRC_RING / DFS_CRC_TILE_RING
// override, set_crc_ring is the benches' A/B switch; K1/K2/K3 launches below
// kCrcRingMinTiles tiles (32 MiB) always use 2. Grid caps follow, never above kMaxGridCrc.
constexpr int kCrcRingDefault = 3;
constexpr int kCrcTileRingDefault = 2;
int crc_ring_buffers();       // K1b scrub
int crc_tile_ring_buffers();  // K1/K2/K3
void set_crc_ring(int scrub_buffers, int tile_buffers);
constexpr uint64_t kCrcRingMinTiles = 2048;
// K1/K2 on matrix cores with one 12-wave workgroup per CU (shared LDS image + MFMA basis, and
// a two-lookup combine per tile) from kCrcWideMinTiles tiles up; 0 = three 4-wave workgroups
// per CU everywhere. DFS_CRC_WIDE overrides, set_crc_wide is the benches' A/B switch.
constexpr int kCrcWideDefault = 1;
int crc_wide_mode();
void set_crc_wide(int mode);
// The wide K1/K2 kernel's chunk CRC on the FP4 matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4:
// 64 input bits per row per instruction at the cycles of the i8 form's 32) instead of i8.
// DFS_CRC_FP4 overrides, set_crc_fp4 is the benches' A/B switch.
constexpr int kCrcFp4Default = 1;
bool crc_fp4_enabled();
void set_crc_fp4(bool on);

// Benches: streaming read of n bytes (n % 16 == 0) on kStreamReadGrid x 256 threads; `out`
// holds 4 x kStreamReadGrid words.
constexpr int kStreamReadGrid = 2048;
hipError_t launch_stream_read(const uint8_t* d, uint64_t n, uint32_t* out, hipStream_t s);

hipError_t launch_crc(const CrcLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K3 fused verify + copy of a range read (crc_read_copy_kernel): `c` is the range plan
// (meta_expect set, part_* unused), `out` a device-visible pointer (registered host memory)
// that receives [off, off + len) with (out - off) % 16 == 0, `part_bad` [grid] device-visible
// words (min mismatching slice per workgroup, 0xFFFFFFFF = none). grid <= kMaxGridCrc.
struct ReadCopyLaunch {
  CrcLaunch c;
  uint8_t* out;
  uint64_t off, len;
  uint32_t* part_bad;
};
hipError_t launch_read_copy(const ReadCopyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K1/K2 fused with a write's host-to-device copy (crc_write_copy_kernel): `c` is a whole-block
// plan whose `data` is the device-visible view of registered host memory, `meta_out` the HBM
// .meta image and `part_crc` [grid] device-visible host words (whole-block partials);
// `dst` the HBM extent, `meta_host` a device-visible host copy of the .meta image. The data
// and dst must be 16 B aligned. grid <= kMaxGridCrc.
struct WriteCopyLaunch {
  CrcLaunch c;
  uint8_t* dst;
  uint32_t* meta_host;
  // optional second copy of the bytes into device-visible host memory (16 B aligned): a
  // pulled replica that the journal appends from the host, with no device-to-host copy
  uint8_t* dst_host = nullptr;
};
// True when launch_crc runs a block of `ntiles` tiles on the kernel that honours
// CrcLaunch::meta_host (the LDS kernel, below the MFMA size threshold).
bool crc_meta_host_ok(uint64_t ntiles);
hipError_t launch_write_copy(const WriteCopyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);
hipError_t launch_gf_matmul(const GfLaunch& a, hipStream_t s);

// K4/K5 fused with the shard checksums (ec_fused_kernel): one launch lands a whole RS stripe.
// Encode: `in` are device views of the k data shards in registered host memory, `dst` their HBM
// extents, `out` the `rows` parity shards; `meta` and the partials cover the k inputs, then the
// outputs. Reconstruct: `in` are verified HBM shards, `dst` is unused, `meta` and the partials
// cover the outputs only. Every pointer is 16 B aligned; shards are `len` bytes, and the plan
// fields are those of a whole-block CrcLaunch of `len` bytes, shared by every shard.
constexpr int kEcFusedMaxRows = 4;   // parity accumulators live in VGPRs
constexpr int kEcFusedMaxGrid = 512;  // one resident round at 2 workgroups per CU
struct EcFusedLaunch {
  const uint8_t* in[kMaxShards];
  uint8_t* dst[kMaxShards];
  uint8_t* out[kEcFusedMaxRows];
  uint32_t* meta[kMaxShards];  // HBM .meta image (BE CRC per slice) of each checksummed shard
  uint64_t s_full, vfront, ntiles;
  uint32_t full_init, tail_len, tail_init;
  int k, rows;
  bool encode;
  const uint32_t* tables;  // device-visible: [rows][k] x 8 dwords (gf_nibble_tables)
  uint32_t* part_crc;      // device-visible: [shard][kMaxGridCrc] raw shifted whole-shard partials
  uint32_t* tail_be;       // device-visible: [shard] BE .meta word of the short tail slice
};
// DFS_EC_FUSED=0 keeps the staged path (copies, K4/K5, one K2 launch per shard); set_ec_fused is
// the benches' A/B switch.
bool ec_fused_enabled();
void set_ec_fused(bool on);
int ec_fused_grid(uint64_t ntiles, uint32_t tail_len, int rows);
hipError_t launch_ec_fused(const EcFusedLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K4 + K2 of the tiering conversion (ec_convert_kernel): one launch turns the resident block `src`
// (HBM, 16 B aligned, n >= 1 bytes in an extent padded to 16 B) into the k + rows shards of
// RS(k, rows), sl = ceil(n / k) bytes each. Data shard c is block bytes [c * sl, c * sl + sl),
// zeros from n on: the columns sit at arbitrary byte shifts and the last ones are short or empty.
// `f` is the encode form of an EcFusedLaunch for shards of sl bytes — `dst` the k data shards,
// `out` the parity shards, `meta`, the plan, the tables, `part_crc` and `tail_be` as there — with
// `in` unused. Every pointer is 16 B aligned; rows <= kEcFusedMaxRows, k + rows <= kMaxShards.
struct EcConvertLaunch {
  EcFusedLaunch f;
  const uint8_t* src;
  uint64_t n, sl;
};
// DFS_EC_CONVERT_FUSED=0 keeps the staged conversion (one copy per column, K4, one K2 launch per
// shard); set_ec_convert_fused is the benches' A/B switch.
bool ec_convert_fused_enabled();
void set_ec_convert_fused(bool on);
int ec_convert_grid(uint64_t ntiles, uint32_t tail_len, int rows);
hipError_t launch_ec_convert(const EcConvertLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// Degraded range read of an RS(k, m) file (ec_read_kernel): bytes [from, from + want) of the
// original file — byte x is byte x % sl of data column x / sl — into `out`, the 16 B aligned
// device view of registered host memory, which receives exactly `want` bytes. `in` are any k
// surviving shards in HBM (16 B aligned, sl bytes in buffers padded to 16 B). A data column is
// either a survivor (surv_col[j] = c, copied with the byte shift between its place in the shard
// and its place in `out`) or, where it is lost and inside the range, the product of reconstruct
// row r with the survivors (row_col[r] = c; tables as gf_nibble_tables lays out [rows][k]).
// Lost columns outside the range are neither named nor computed. Limits: sl >= kEcReadMinShard,
// rows <= kEcFusedMaxRows, 0 < want, from + want <= k * sl.
constexpr uint64_t kEcReadMinShard = 1024;  // one wave step: 64 lanes x 16 B
constexpr int kEcReadMaxGrid = 1024;        // one resident round at 4 workgroups per CU
struct EcReadLaunch {
  const uint8_t* in[kMaxShards];
  int8_t surv_col[kMaxShards];       // data column that survivor j is, -1 for a parity shard
  int8_t row_col[kEcFusedMaxRows];   // data column that reconstruct row r rebuilds
  int k, rows;
  uint64_t sl, from, want;
  const uint32_t* tables;  // device-visible: [rows][k] x 8 dwords; unused when rows == 0
  uint8_t* out;
  // set by launch_ec_read: the (at most two) runs of wave steps that some column needs
  uint64_t seg_begin[2], seg_steps[2];
};
// DFS_EC_READ_FUSED=0 keeps the staged degraded read (ec_decode of whole shards into HBM, then one
// copy per column); set_ec_read_fused is the benches' A/B switch.
bool ec_read_fused_enabled();
void set_ec_read_fused(bool on);
hipError_t launch_ec_read(const EcReadLaunch& a, hipStream_t s);

// K7, AES-256-GCM of one message of n >= 1 bytes, no AAD (sse_gcm_kernel): dst = src XOR keystream
// and the GHASH of the ciphertext (dst when encrypting, src when decrypting) as one 128-bit partial
// per workgroup in `part`, which gcm::ghash_fold and gcm::finish_tag turn into the tag. `src` and
// `dst` are device views of registered host memory with src % 4 == 0 and (dst - src) % 16 == 0, equal
// (in place) or disjoint; only [dst, dst + n) is written, though the 16 B vectors that hold the
// message's first and last bytes are read whole. The plan is gcm::plan_for(n), the key schedule and
// the powers of H come from gcm::prepare for that plan, and `grid` is the plan's. The key material
// travels as kernel arguments (scalar registers), never through memory the store owns.
struct SseGcmLaunch {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t n, ntiles, vfront;
  uint32_t encrypt;
  uint32_t nonce[3];
  uint32_t rk[60];
  gcm::U128 h, hjump, tree[gcm::kGcmTreeSteps];
  gcm::U128* part;  // device-visible: [grid]
};
// DFS_SSE_FUSED=0 keeps OpenSSL on the calling thread. Bodies below sse_fused_min_bytes() stay there
// too: a call costs ~120 us before the first byte (key schedule and powers of H on the host, launch,
// synchronise, and a GHASH tree of 128-step multiplies per workgroup), which OpenSSL at 6.6 GB/s
// undercuts at 64 KiB (10 us) and at 1 MiB (155 against 162 us); 4 MiB is the smallest measured size
// the kernel wins (274 against 621 us, profiles/r10). DFS_SSE_FUSED_MIN_BYTES overrides; set_sse_fused is the benches' and tests' switch
// (min_bytes < 0 keeps the threshold).
constexpr uint64_t kSseFusedMinBytes = 4ull << 20;
bool sse_fused_enabled();
uint64_t sse_fused_min_bytes();
void set_sse_fused(bool on, int64_t min_bytes = -1);
hipError_t launch_sse_gcm(const SseGcmLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K7 read (sse_read_kernel): a stored SSE-S3 blob [nonce 12][ciphertext n][tag 16], resident in HBM
// at `src` (16 B aligned, readable up to the next 16 B boundary behind its end) with its .meta
// image `meta`, is verified slice by slice, decrypted and stored as n plaintext bytes at `out`, the
// 16 B aligned device view of registered host memory: only [out, out + n) is written. The kernel
// reads the nonce from the block; the host learns it, and the stored tag, from `nonce_tag`.
// `part_bad` takes the per-workgroup minimum bad slice (0xFFFFFFFF: none) and `part` the GHASH
// partials of the plan gcm::plan_for(kSseReadTileBytes * ntiles), ntiles = sse_read_tiles(n), whose
// grid is the launch's; gcm::prepare_keyed for that plan gives the key schedule and the powers of
// H, and gcm::tag_matches with the plan's zero blocks behind the message closes the tag. part,
// part_bad and nonce_tag are device-visible host words.
constexpr uint64_t kSseReadTileBytes = 16 << 10;
inline uint64_t sse_read_tiles(uint64_t n) { return (n + 28 + kSseReadTileBytes - 1) / kSseReadTileBytes; }
struct SseReadLaunch {
  const uint8_t* src;
  const uint32_t* meta;
  uint8_t* out;
  uint64_t n, ntiles;
  uint32_t full_init, tail_init;  // S(512), S((n + 28) % 512)
  uint32_t rk[60];
  gcm::U128 h, hjump, tree[gcm::kGcmTreeSteps];
  gcm::U128* part;     // [grid]
  uint32_t* part_bad;  // [grid]
  uint8_t* nonce_tag;  // [28]
};
// DFS_SSE_READ_FUSED=0 keeps the staged route (read_into, then sse_crypt where the blob lies), and
// blobs whose plaintext is below sse_read_fused_min_bytes() stay on it. DFS_SSE_READ_FUSED_MIN_BYTES
// overrides the floor; set_sse_read_fused is the benches' and tests' switch (min_bytes < 0 keeps it).
// A call costs ~128 us before the first byte (K7's fixed cost: key schedule, launch, synchronise,
// GHASH tree), which the staged route undercuts at 64 KiB with a mirror read and OpenSSL; 1 MiB is
// the smallest measured size the kernel wins (profiles/r11).
constexpr uint64_t kSseReadFusedMinBytes = 1ull << 20;
bool sse_read_fused_enabled();
uint64_t sse_read_fused_min_bytes();
void set_sse_read_fused(bool on, int64_t min_bytes = -1);
hipError_t launch_sse_read(const SseReadLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K7 range read (sse_read_range_kernel): plaintext [from, from + want) of the same blob, 0 < want and
// from + want <= r.n. Everything of SseReadLaunch holds as above (the whole blob is verified and
// authenticated: same plan, partials, verdicts and host half), except `r.out`: it is the device view
// of where plaintext byte `from` goes, with r.out % 16 == from % 16, and exactly [r.out, r.out + want)
// is written. Only the tiles that hold bytes of the range run AES. The floor is that of the whole
// read and applies to the blob's n, not to want: the pass covers the whole blob (profiles/r12).
struct SseReadRangeLaunch {
  SseReadLaunch r;
  uint64_t from, want;
};
hipError_t launch_sse_read_range(const SseReadRangeLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K7 write (sse_write_kernel): an SSE-S3 PUT in one pass. `buf` is the 16 B aligned device view of
// registered host memory of n + 28 bytes holding [12 unspecified][plaintext n][16 unspecified], n >= 1;
// `dst` a 16 B aligned HBM extent padded to 16 B and `meta` its .meta image. The kernel encrypts
// with the counter built from `nonce` (the argument, not the slot's bytes), stores
// [nonce][ciphertext][zeros] to dst and back to buf, writing nothing outside [buf, buf + n + 28), and
// leaves: the BE .meta words of the sse_write_body_slices(n) slices in front of the tag in `meta`
// and `meta_host`; in `part` the GHASH partials of the plan gcm::plan_for(kSseReadTileBytes * ntiles),
// ntiles = sse_read_tiles(n), whose grid is the launch's; and in `part_crc` the raw whole-block CRC
// partials of those slices followed by zeros to the end of the last tile (XOR them, then take the
// zeros out with crc_unshift). The key schedule and the powers of H are gcm::prepare's for that
// plan, except `hjump`: a chunk absorbs five elements, so a lane's step between its tiles is
// gcm::write_jump. The host closes the tag (gcm::unfold takes out the plan's zero blocks behind
// the message), writes it to both copies and checksums the slices that hold it. meta_host, part and
// part_crc are device-visible host words.
constexpr uint64_t sse_write_body_slices(uint64_t n) { return (n + 12) / 512; }
struct SseWriteLaunch {
  uint8_t* buf;
  uint8_t* dst;
  uint32_t* meta;
  uint32_t* meta_host;
  uint64_t n, ntiles;
  uint32_t full_init;  // S(512)
  uint32_t nonce[3];
  uint32_t rk[60];
  gcm::U128 h, hjump, tree[gcm::kGcmTreeSteps];
  gcm::U128* part;     // [grid]
  uint32_t* part_crc;  // [grid]
};
// The staged route is sse_crypt in place, then write. Measured (profiles/r13), the kernel wins from
// 4 MiB up on an hbm-ack store (320 against 381 us) and at no size on an nvme-sync store, where the
// durable copy can start only after the kernel while write() overlaps its data file with the GPU.
// So with nothing said the kernel takes bodies of sse_write_fused_min_bytes() and more on hbm-ack
// stores only; DFS_SSE_WRITE_FUSED=1 or set_sse_write_fused(true) turns it on in both modes, =0 or
// (false) off. DFS_SSE_WRITE_FUSED_MIN_BYTES overrides the floor; the setter is the benches' and
// tests' switch (min_bytes < 0 keeps the floor), and reset_sse_write_fused puts both back to what
// the environment and the defaults say, the "nothing said" state included.
constexpr uint64_t kSseWriteFusedMinBytes = 4ull << 20;
bool sse_write_fused_enabled(bool nvme_sync);
uint64_t sse_write_fused_min_bytes();
void set_sse_write_fused(bool on, int64_t min_bytes = -1);
void reset_sse_write_fused();
hipError_t launch_sse_write(const SseWriteLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K7 copy (sse_rekey_kernel): a CopyObject of an SSE-S3 object in one pass, HBM to HBM. `src` is a
// stored blob [nonce 12][ciphertext n][tag 16], n >= 1, resident at a 16 B aligned extent readable up
// to the next 16 B boundary behind its end, with its .meta image `src_meta`; `dst` another 16 B
// aligned extent padded to 16 B, disjoint from the first, and `meta` its .meta image. The kernel
// verifies every slice of the source against src_meta (`part_bad`: the per-workgroup minimum bad
// slice, 0xFFFFFFFF none), absorbs the old ciphertext under `from`, XORs the keystream of `from`
// with the nonce it reads from the blob and that of `to` with `nonce` into it, absorbs the new
// ciphertext under `to`, and stores [nonce][new ciphertext][zeros] to dst. It leaves what
// sse_read_kernel leaves for the source (from.part, part_bad, nonce_tag: gcm::tag_matches closes it)
// and what sse_write_kernel leaves for the destination (to.part, meta, meta_host, part_crc: the host
// closes the tag, writes it and checksums its slices). Both sides share the plan
// gcm::plan_for(kSseReadTileBytes * ntiles), ntiles = sse_read_tiles(n), whose grid is the launch's;
// `from` is gcm::prepare_keyed's and `to` gcm::prepare's for it, and either hjump is gcm::write_jump:
// a chunk absorbs five elements on both sides. The host must look at part_bad and the source's tag
// before anything names the destination's bytes. part, part_bad, part_crc, nonce_tag and meta_host
// are device-visible host words.
struct SseRekeySide {
  uint32_t rk[60];
  gcm::U128 h, hjump, tree[gcm::kGcmTreeSteps];
  gcm::U128* part;  // [grid]
};
struct SseRekeyLaunch {
  const uint8_t* src;
  const uint32_t* src_meta;
  uint8_t* dst;
  uint32_t* meta;
  uint32_t* meta_host;
  uint64_t n, ntiles;
  uint32_t full_init, tail_init;  // S(512), S((n + 28) % 512)
  uint32_t nonce[3];              // the destination's
  SseRekeySide from, to;
  uint32_t* part_bad;  // [grid]
  uint32_t* part_crc;  // [grid]
  uint8_t* nonce_tag;  // [28]: the source's
  // [kSseRekeyTailBytes]: the new blob from slice sse_write_body_slices(n) on, as whole 16 B vectors
  // (under 528 bytes of ciphertext and zeros), for the host's checksum of the slices that hold the tag
  uint8_t* tail_host;
};
constexpr uint64_t kSseRekeyTailBytes = 544;
// DFS_SSE_COPY_FUSED=0 keeps the staged route (sse_read into a temporary, sse_crypt under the new key,
// write), and blobs whose plaintext is below sse_copy_fused_min_bytes() stay on it.
// DFS_SSE_COPY_FUSED_MIN_BYTES overrides the floor; set_sse_copy_fused is the benches' and tests'
// switch (min_bytes < 0 keeps it). Measured (profiles/r14), a call costs ~300 us before the first byte
// (two key preparations, launch, synchronise, two GHASH trees, H_dst^-vback), which the staged route
// undercuts at 64 KiB (139 us); 1 MiB is the smallest measured size the kernel wins, on hbm-ack
// (322 against 569 us) and nvme-sync stores (443 against 598 us) alike, so nothing gates it by durability.
// That rests on one run of three repetitions per route, with no size between 64 KiB and 1 MiB taken.
constexpr uint64_t kSseCopyFusedMinBytes = 1ull << 20;
bool sse_copy_fused_enabled();
uint64_t sse_copy_fused_min_bytes();
void set_sse_copy_fused(bool on, int64_t min_bytes = -1);
hipError_t launch_sse_rekey(const SseRekeyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);

// K7 EC read (sse_ec_read_kernel): the stored blob [nonce 12][ciphertext n][tag 16], orig = n + 28
// bytes, is held as an RS(k, m) file with sl >= ceil(orig / k): blob byte x is byte x % sl of data
// column x / sl, zeros from orig on. `in` are k surviving shards in HBM (16 B aligned, sl bytes in
// buffers padded to 16 B), `surv_col`, `row_col` and `tables` as EcReadLaunch carries them, and every
// data column is either a survivor or named by a reconstruct row. The n plaintext bytes go to `out`,
// the 16 B aligned device view of registered host memory: exactly [out, out + n) is written. The
// rest is SseReadLaunch's without the checksum fields: the plan gcm::plan_for(kSseReadTileBytes *
// ntiles), ntiles = sse_read_tiles(n), whose grid is the launch's, gcm::prepare_keyed's key schedule
// and powers of H, `part` for gcm::ghash_fold and `nonce_tag` for gcm::tag_matches (device-visible
// host words, like `tables`). The shards are not checksummed here: the caller hands over verified
// shards, and the tag authenticates what was rebuilt and decrypted.
// The minimum shard length is one wave's span of the axis (64 lanes x 64 B): then a wave's blocks lie in
// at most two columns, which bounds the load stage's passes and lets the second one reuse the first
// one's registers. Shorter shards (blobs under 4 KiB * k) take the staged route.
constexpr uint64_t kSseEcReadMinShard = 4096;
static_assert(kSseEcReadMinShard >= kEcReadMinShard && kSseEcReadMinShard <= kSseReadTileBytes, "between the two");
struct SseEcReadLaunch {
  const uint8_t* in[kMaxShards];
  int8_t surv_col[kMaxShards];      // data column that survivor j is, -1 for a parity shard
  int8_t row_col[kEcFusedMaxRows];  // data column that reconstruct row r rebuilds
  int k, rows;
  uint64_t sl;
  const uint32_t* tables;  // [rows][k] x 8 dwords; unused when rows == 0
  uint8_t* out;
  uint64_t n, ntiles;
  uint32_t rk[60];
  gcm::U128 h, hjump, tree[gcm::kGcmTreeSteps];
  gcm::U128* part;     // [grid]
  uint8_t* nonce_tag;  // [28]
};
// DFS_SSE_EC_READ_FUSED=0 keeps the staged route (ec_read_range of the blob into a temporary, then
// sse_crypt or OpenSSL there), and blobs whose plaintext is below sse_ec_read_fused_min_bytes() stay
// on it. DFS_SSE_EC_READ_FUSED_MIN_BYTES overrides the floor; set_sse_ec_read_fused is the benches'
// and tests' switch (min_bytes < 0 keeps it). Measured (profiles/r15/README.md, RS(6,3), against
// ec_read_range of the blob into the slot followed by sse_crypt there), a call costs ~129 us at 64 KiB,
// which the staged pair undercuts (32 us: OpenSSL under sse_crypt's floor); 1 MiB is the smallest
// measured size the kernel wins (151 against 202 us, spreads under 2 us), with 0 and with 1 lost data
// column alike. No size between 64 KiB and 1 MiB was taken.
constexpr uint64_t kSseEcReadFusedMinBytes = 1ull << 20;
bool sse_ec_read_fused_enabled();
uint64_t sse_ec_read_fused_min_bytes();
void set_sse_ec_read_fused(bool on, int64_t min_bytes = -1);
hipError_t launch_sse_ec_read(const SseEcReadLaunch& a, const DevCrcTables* t, int grid, hipStream_t s);
hipError_t launch_scrub(const ScrubLaunch& a, const DevCrcTables* t, hipStream_t s);

}  // namespace dfs
