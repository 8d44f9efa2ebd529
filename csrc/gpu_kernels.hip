// CDNA4 kernels for the chunk data path. Design notes:
//  * 64-lane waves: 8 lanes x 64 B cover one 512 B slice, so a wave checksums 8 slices
//    (4 KiB) and a 256-thread workgroup a 16 KiB tile. Each lane runs a slicing-by-16
//    chain over its 64 B (16 independent LDS lookups per 16 B, state carried between
//    chunks), then the wave combines lane/slice partials with a butterfly over
//    __shfl_xor and "shift by 2^k bytes" byte tables — all tables live in LDS (48 KiB).
//  * Whole-block CRC (K2) comes out of the same pass: slices are combined into a tile
//    value, and each tile is shifted to its final position with GF(2) matrices applied
//    lane-parallel (lane i owns column i, 5 xor-shuffles), so the host only XORs
//    `grid` partials. Leading zero slices do not change a raw CRC, which lets the tiling
//    be aligned at the block END (virtual front padding) without any inverse operator.
//  * Grid = min(tiles, 1024) with a grid-stride loop: the LDS table fill (48 KiB from
//    L2) is paid once per workgroup, not per tile.
#include "gpu_kernels.h"

#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crc32.h"
#include "gf256.h"

namespace dfs {

namespace {

__device__ __forceinline__ uint32_t tab4(const uint32_t (*t)[256], uint32_t v) {
  return t[0][v & 0xff] ^ t[1][(v >> 8) & 0xff] ^ t[2][(v >> 16) & 0xff] ^ t[3][v >> 24];
}

__device__ __forceinline__ uint32_t chunk16(const uint32_t (*T)[256], uint32_t c, uint4 w) {
  uint32_t w0 = w.x ^ c;
  return T[15][w0 & 0xff] ^ T[14][(w0 >> 8) & 0xff] ^ T[13][(w0 >> 16) & 0xff] ^
         T[12][w0 >> 24] ^ T[11][w.y & 0xff] ^ T[10][(w.y >> 8) & 0xff] ^
         T[9][(w.y >> 16) & 0xff] ^ T[8][w.y >> 24] ^ T[7][w.z & 0xff] ^
         T[6][(w.z >> 8) & 0xff] ^ T[5][(w.z >> 16) & 0xff] ^ T[4][w.z >> 24] ^
         T[3][w.w & 0xff] ^ T[2][(w.w >> 8) & 0xff] ^ T[1][(w.w >> 16) & 0xff] ^ T[0][w.w >> 24];
}

// Value of lane `lane ^ m` without LDS traffic: DPP for m <= 8 (xor 4 = half-row mirror of
// the xor-3 quad permutation; xor 8 = rotate the 16-lane row by 8, either direction), the
// CDNA4 permlane swaps for 16 and 32 (swapping v with itself leaves the even half-rows /
// half-waves in r[0] and the odd ones in r[1]).
template <int kCtrl>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t x) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), kCtrl, 0xF, 0xF, false));
}

template <int m>
__device__ __forceinline__ uint32_t xchg(uint32_t v, int lane) {
  if constexpr (m == 1) return dpp_mov<0xB1>(v);  // quad_perm [1,0,3,2]
  else if constexpr (m == 2) return dpp_mov<0x4E>(v);  // quad_perm [2,3,0,1]
  else if constexpr (m == 4) return dpp_mov<0x141>(dpp_mov<0x1B>(v));  // quad_perm [3,2,1,0], then half-row mirror
  else if constexpr (m == 8) return dpp_mov<0x128>(v);  // row_ror:8
  else if constexpr (m == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane & 16) ? r[0] : r[1];
  } else {
    static_assert(m == 32, "xchg: 1, 2, 4, 8, 16 or 32");
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (lane & 32) ? r[0] : r[1];
  }
}

// Butterfly step: lanes with (lane & m) == 0 hold the earlier bytes.
template <int m>
__device__ __forceinline__ uint32_t combine(uint32_t r, int lane, const uint32_t (*t)[256]) {
  uint32_t p = xchg<m>(r, lane);
  bool right = lane & m;
  uint32_t left = right ? p : r;
  uint32_t rgt = right ? r : p;
  return tab4(t, left) ^ rgt;
}

// XOR all-reduce steps inside the wave without LDS traffic (ds_bpermute plus its address
// arithmetic is what __shfl_xor compiles to). Applied smallest group first: xr4 / xr8 pair
// lanes by mirroring a half-row / row (DPP), which equals the xor-4 / xor-8 partner's value
// once the quads / 8-lane groups are already uniform; xr16 / xr32 use the CDNA4 permlane
// swaps (a swap of v with itself leaves the two halves' values in the two results).
template <int kCtrl>
__device__ __forceinline__ uint32_t xr_dpp(uint32_t v) {
  return v ^ static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), kCtrl, 0xF, 0xF, false));
}
__device__ __forceinline__ uint32_t xr1(uint32_t v) { return xr_dpp<0xB1>(v); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ uint32_t xr2(uint32_t v) { return xr_dpp<0x4E>(v); }   // quad_perm [2,3,0,1]
__device__ __forceinline__ uint32_t xr4(uint32_t v) { return xr_dpp<0x141>(v); }  // row_half_mirror
__device__ __forceinline__ uint32_t xr8(uint32_t v) { return xr_dpp<0x140>(v); }  // row_mirror
__device__ __forceinline__ uint32_t xr16(uint32_t v) {
  const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  return r[0] ^ r[1];
}
__device__ __forceinline__ uint32_t xr32(uint32_t v) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return r[0] ^ r[1];
}

// Lane-parallel GF(2) matrix apply: v uniform across the wave, lanes 0..31 own columns.
__device__ __forceinline__ uint32_t mat_apply(const uint32_t* col, uint32_t v, int lane) {
  int i = lane & 31;
  uint32_t x = ((v >> i) & 1u) ? col[i] : 0u;
  return xr16(xr8(xr4(xr2(xr1(x)))));
}

__device__ __forceinline__ void load_tables(const DevCrcTables* __restrict__ gt, DevCrcTables* lt) {
  const uint4* src = reinterpret_cast<const uint4*>(gt);
  uint4* dst = reinterpret_cast<uint4*>(lt);
  constexpr int n16 = sizeof(DevCrcTables) / 16;
  for (int i = threadIdx.x; i < n16; i += kCrcWgThreads) dst[i] = src[i];
}

// One 512 B slice per 8 lanes: lane `sl` hashes bytes [sl*64, sl*64+64), then the three
// butterflies leave the slice CRC (raw, before the init term) in lane sl == 0.
__device__ __forceinline__ uint32_t slice_crc(const DevCrcTables& lt, const uint8_t* slice, int sl, int lane,
                                              bool valid) {
  uint32_t r = 0;
  if (valid) {
    const uint4* p = reinterpret_cast<const uint4*>(slice + sl * 64);
    uint4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3];
    r = chunk16(lt.slice16, 0, c0);
    r = chunk16(lt.slice16, r, c1);
    r = chunk16(lt.slice16, r, c2);
    r = chunk16(lt.slice16, r, c3);
  }
  r = combine<1>(r, lane, lt.sh64);
  r = combine<2>(r, lane, lt.sh128);
  return combine<4>(r, lane, lt.sh256);
}

// ---------------------------------------------------------------------------------------
// Matrix-core chunk CRC. The raw CRC of a 64-byte chunk is a GF(2)-linear map of its 512
// bits: R(chunk) = XOR over set bits (byte b, bit p) of V[b][p], V[b][p] = R(e_{b,p}).
// That is a 32 x 512 binary matrix times the chunk's bit vector — an integer GEMM whose
// result only needs its parity. One v_mfma_i32_32x32x32_i8 multiplies A (32 CRC bits x 32
// K-bits of the basis) by B (32 K-bits x 32 chunks); 16 of them cover the 512 bits of 32
// chunks (2 KiB), two passes the wave's 4 KiB.
//  * B (data): lane (n = l&31, h = l>>5) loads bytes [32h, 32h+32) of chunk n. K-step s
//    uses dword s>>1 and bit planes 4(s&1)..4(s&1)+3: fragment dword q is the dword ANDed
//    with 0x01010101 << p (one VALU op; the planes are not shifted down).
//  * A (basis, in 64 VGPRs for the whole kernel): element (s, h, j) is 2^(7-p) where bit i
//    of V[byte][p] is set, so every product of a set data bit is 2^7 (mod 2^8) and bit 7 of
//    the int32 accumulator is the parity — the GF(2) sum — for any K order, as long as A
//    and B agree on it (the host builds A in upload_crc_tables with the same mapping).
//  * D: lane (n, h) holds CRC bits i = (r&3) + 8(r>>2) + 4h of chunk n in register r; the
//    two half-waves OR their 16 bits together with one shuffle.
// 64 LDS table lookups per lane per 64 B become 32 MFMAs per 4 KiB per wave.
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

__device__ __forceinline__ void load_basis(const i32x4* __restrict__ basis, int lane, i32x4 (&A)[16]) {
#pragma unroll
  for (int s = 0; s < 16; ++s) A[s] = basis[s * 64 + lane];
}

// The 64 B this lane feeds to the two MFMA passes over the wave's 8 slices starting at slice
// i0 (two halves of chunk n in pass 0 and pass 1); slices outside [lo, hi) read as zeros.
struct WaveData {
  uint4 v[4];
};

__device__ __forceinline__ WaveData load_wave(const uint8_t* __restrict__ data, int64_t i0, int64_t lo, int64_t hi,
                                              int lane) {
  const int n = lane & 31, h = lane >> 5;
  WaveData d;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = it * 32 + n;
    const int64_t i = i0 + (c >> 3);
    d.v[2 * it] = d.v[2 * it + 1] = make_uint4(0, 0, 0, 0);
    if (i >= lo && i < hi) {
      // streamed once: non-temporal, so checksum passes do not evict hot lines from L2
      using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
      const u32x4* p = reinterpret_cast<const u32x4*>(data + static_cast<uint64_t>(i) * 512 + (c & 7) * 64 + h * 32);
      u32x4 x = __builtin_nontemporal_load(p), y = __builtin_nontemporal_load(p + 1);
      d.v[2 * it] = make_uint4(x[0], x[1], x[2], x[3]);
      d.v[2 * it + 1] = make_uint4(y[0], y[1], y[2], y[3]);
    }
  }
  return d;
}

// Ring form of load_wave for the pipelined kernels: the loads are unconditional (slices
// outside [lo, hi) read slice lo instead; requires lo < hi) and the consumer zeroes the
// CHUNK CRCs of those slices (one select per lane instead of 16 on the data; the raw CRC of
// zeros is zero, so it is the same as zeroed data). A conditional load into a zeroed
// register is a VALU write to a register the ring may still have a load pending on, and the
// compiler resolves that with a vmcnt(0) that drains the whole ring.
__device__ __forceinline__ WaveData load_wave_ring(const uint8_t* __restrict__ data, int64_t i0, int64_t lo,
                                                   int64_t hi, int lane) {
  const int n = lane & 31, h = lane >> 5;
  WaveData d;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = it * 32 + n;
    int64_t i = i0 + (c >> 3);
    i = (i >= lo && i < hi) ? i : lo;
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
    const u32x4* p = reinterpret_cast<const u32x4*>(data + static_cast<uint64_t>(i) * 512 + (c & 7) * 64 + h * 32);
    u32x4 x = __builtin_nontemporal_load(p), y = __builtin_nontemporal_load(p + 1);
    d.v[2 * it] = make_uint4(x[0], x[1], x[2], x[3]);
    d.v[2 * it + 1] = make_uint4(y[0], y[1], y[2], y[3]);
  }
  return d;
}

// Raw CRC of the 64-byte chunk `lane` of the wave's 4 KiB (wave-wide: all 64 lanes together).
// Every product in the accumulators is 0 or +-2^7, so an accumulator's low byte is 0x80 or 0
// (its parity, nothing below): three byte permutes gather the low bytes of four accumulators
// into one dword (acc[4k + q] -> byte k), four such dwords shifted by q land in distinct bits,
// and the half-waves interleave by 4. The basis rows are laid out so that this gather IS the
// CRC bit order (row R of the MFMA carries CRC bit R ^ 7, see upload_crc_tables): 17 VALU
// per pass instead of one extract-and-insert pair per accumulator.
__device__ __forceinline__ uint32_t wave_chunk_crcs(const i32x4 (&A)[16], const WaveData& d, int lane) {
  const int h = lane >> 5;
  uint32_t mine = 0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint4 w0 = d.v[2 * it], w1 = d.v[2 * it + 1];
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const uint32_t x = w[s >> 1];
      const uint32_t m = 0x01010101u << (4 * (s & 1));
      i32x4 b;
      b.x = static_cast<int>(x & m);
      b.y = static_cast<int>(x & (m << 1));
      b.z = static_cast<int>(x & (m << 2));
      b.w = static_cast<int>(x & (m << 3));
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s], b, acc, 0, 0, 0);
    }
    uint32_t part = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t lo = __builtin_amdgcn_perm(static_cast<uint32_t>(acc[4 + q]), static_cast<uint32_t>(acc[q]), 0x0c0c0400u);
      const uint32_t hi = __builtin_amdgcn_perm(static_cast<uint32_t>(acc[12 + q]), static_cast<uint32_t>(acc[8 + q]),
                                                0x0c0c0400u);
      part |= __builtin_amdgcn_perm(hi, lo, 0x05040100u) >> q;  // bit 7 + 8k - q: acc[4k + q]
    }
    part >>= 4 * h;
    part = xr32(part);  // the half-waves' bits are disjoint: XOR = OR
    if (it == h) mine = part;  // lane L keeps chunk L: it comes out of pass L >> 5
  }
  return mine;
}

// The same chunk CRCs on the FP4 matrix cores. v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1
// operands (unit block scales) takes 64 K per instruction at the cycles of the i8 32x32x32, so a
// 64 B chunk is 8 instructions instead of 16 and the basis 32 VGPRs instead of 64:
//  * B: one data dword x gives the whole 32-element fragment: x & 0x11111111 (each nibble 0 or
//    0b0001 = 0.5), x & 0x22222222 (0 or 1.0), x & 0x44444444 (0 or 2.0) and
//    (x >> 1) & 0x44444444 (bit 3 of each nibble; 0 or 2.0; bit 3 itself is the sign).
//  * A: 2.0 / 1.0 / 0.5 / 0.5 where the basis bit is set, so every product of two set bits is
//    exactly 1.0 and the f32 accumulator counts them (at most 512 per pass: exact).
//  * The accumulators start at 65536 = 2^16: in [2^16, 2^17) one ulp is 2^-7, so the count's
//    bit 0 — the parity — is bit 7 of the float's encoding and bits 0..6 are 0. The low byte is
//    0x80 or 0, exactly what the i8 form's gather expects.
using i32x8 = __attribute__((ext_vector_type(8))) int;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ uint32_t wave_chunk_crcs_fp4(const i32x4 (&A)[8], const WaveData& d, int lane) {
  const int h = lane >> 5;
  uint32_t mine = 0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint4 w0 = d.v[2 * it], w1 = d.v[2 * it + 1];
    const uint32_t w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 65536.0f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const uint32_t x = w[s];
      const i32x8 b = {static_cast<int>(x & 0x11111111u), static_cast<int>(x & 0x22222222u),
                       static_cast<int>(x & 0x44444444u), static_cast<int>((x >> 1) & 0x44444444u), 0, 0, 0, 0};
      const i32x8 a = {A[s].x, A[s].y, A[s].z, A[s].w, 0, 0, 0, 0};
      acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 4, 4, 0, 127, 0, 127);
    }
    uint32_t part = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t lo = __builtin_amdgcn_perm(__float_as_uint(acc[4 + q]), __float_as_uint(acc[q]), 0x0c0c0400u);
      const uint32_t hi = __builtin_amdgcn_perm(__float_as_uint(acc[12 + q]), __float_as_uint(acc[8 + q]), 0x0c0c0400u);
      part |= __builtin_amdgcn_perm(hi, lo, 0x05040100u) >> q;
    }
    part >>= 4 * h;
    part = xr32(part);
    if (it == h) mine = part;
  }
  return mine;
}

// The basis of either form in VGPRs, loaded from the uploaded image (kernels that keep no LDS copy).
template <bool kFp4>
struct ChunkBasis {
  static constexpr int kFrags = kFp4 ? 8 : 16;
  i32x4 A[kFrags];
  __device__ __forceinline__ void load(const DevCrcTables* __restrict__ gt, int lane) {
    const i32x4* p = reinterpret_cast<const i32x4*>(reinterpret_cast<const uint8_t*>(gt + 1) +
                                                    (kFp4 ? kCrcBasisFp4Offset : 0));
#pragma unroll
    for (int s = 0; s < kFrags; ++s) A[s] = p[s * 64 + lane];
  }
  __device__ __forceinline__ uint32_t crcs(const WaveData& d, int lane) const {
    if constexpr (kFp4) return wave_chunk_crcs_fp4(A, d, lane);
    else return wave_chunk_crcs(A, d, lane);
  }
};

// Chunk CRCs -> slice CRC in one lookup round: lane sl of a slice's 8-lane group moves its
// chunk CRC past the 64 * (7 - sl) bytes that follow the chunk in the slice (one tab4 into
// its own shift table; sl == 7 needs none) and three xor-shuffles fold the group, since the
// raw CRC of a concatenation is the XOR of the shifted parts. Every lane of the group ends
// with the slice CRC. (The butterfly it replaces did three dependent tab4 rounds — 12 LDS
// lookups per lane, the kernels' only bank conflicts — for the same result.)
template <class L>
__device__ __forceinline__ uint32_t slice_from_chunks(const L& lt, uint32_t r, int lane) {
  const int sl = lane & 7;
  uint32_t v = sl < 7 ? tab4(lt.cs[sl], r) : r;
  return xr4(xr2(xr1(v)));
}

// LDS images of the matrix-core kernels: only the GF(2) shift tables they look up (the
// slicing-by-16 tables of the table kernels are not needed: short tail slices go through
// the MFMA path front-padded with zeros). `cs` comes from the chunk-shift tables stored
// behind the MFMA basis, the tile part is the suffix of DevCrcTables from sh512 on.
struct MfmaSliceLds {  // K1b, fused K3: chunk -> slice combine (28 KiB)
  uint32_t cs[7][4][256];
};
struct MfmaTileLds {  // K1/K2/K3: + slice -> sub-tile combine and the tile shifts (48 KiB)
  uint32_t cs[7][4][256];
  uint32_t sh512[4][256], sh1k[4][256], sh2k[4][256];
  uint32_t sh4k[4][256];
  uint32_t tile_pow2[32][32];
};
static_assert(sizeof(MfmaSliceLds) == kCrcChunkShiftBytes, "chunk-shift image");
static_assert(sizeof(MfmaTileLds) - sizeof(MfmaSliceLds) == sizeof(DevCrcTables) - offsetof(DevCrcTables, sh512),
              "LDS image layout");

template <int kThreads = kCrcWgThreads>
__device__ __forceinline__ void copy16(const void* __restrict__ from, void* to, int bytes) {
  const uint4* src = reinterpret_cast<const uint4*>(from);
  uint4* dst = reinterpret_cast<uint4*>(to);
  const int n16 = bytes / 16;
#pragma unroll 4
  for (int i = threadIdx.x; i < n16; i += kThreads) dst[i] = src[i];
}

// The same copy by LDS-DMA (global_load_lds_dwordx4: each wave instruction moves 1 KiB straight
// into LDS, no VGPRs, no wait before the next one), so a kernel's whole LDS image is in flight at
// once instead of one register round trip per pass. The destination of one instruction is
// wave-uniform base + 16 x lane, which a linear copy is. bytes % 16 == 0; completes at the next
// __syncthreads() (its vmcnt(0)).
template <int kThreads>
__device__ __forceinline__ void dma16(const void* __restrict__ from, void* to, int bytes) {
  using LdsPtr = __attribute__((address_space(3))) void*;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(from);
  uint8_t* dst = reinterpret_cast<uint8_t*>(to);
  for (int base = wave * 1024; base < bytes; base += kThreads * 16)
    if (base + lane * 16 < bytes)
      __builtin_amdgcn_global_load_lds(src + base + lane * 16, (LdsPtr)(dst + base), 16, 0, 0);
}

template <class L, int kThreads = kCrcWgThreads>
__device__ __forceinline__ void load_lds_image(const DevCrcTables* __restrict__ gt, L* lt) {
  const uint8_t* cs = reinterpret_cast<const uint8_t*>(gt + 1) + kCrcBasisBytes;
  copy16<kThreads>(cs, lt, kCrcChunkShiftBytes);
  if constexpr (sizeof(L) > kCrcChunkShiftBytes)
    copy16<kThreads>(&gt->sh512, reinterpret_cast<uint8_t*>(lt) + kCrcChunkShiftBytes,
                     static_cast<int>(sizeof(L)) - kCrcChunkShiftBytes);
}

// The short tail slice (len < 512 bytes at `base`) as slice 0 of a wave's 4 KiB, front-padded
// with zeros to 512 B (the raw CRC ignores leading zeros); every other slice reads as zeros.
// Byte loads: it runs once per block. Only base[0, valid) is read; the bytes behind it count
// as zeros (a column of a block that ends inside the slice, see ec_convert_kernel).
__device__ __forceinline__ WaveData load_tail_wave(const uint8_t* __restrict__ base, uint32_t len, int lane,
                                                   int valid) {
  const int n = lane & 31, h = lane >> 5;
  WaveData d;
#pragma unroll
  for (int k = 0; k < 4; ++k) d.v[k] = make_uint4(0, 0, 0, 0);
  if (n < 8) {
    const int pad = 512 - static_cast<int>(len);
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint32_t v = 0;
      for (int b = 0; b < 4; ++b) {
        const int pos = n * 64 + h * 32 + q * 4 + b;
        v |= (pos >= pad && pos - pad < valid ? static_cast<uint32_t>(base[pos - pad]) : 0u) << (8 * b);
      }
      w[q] = v;
    }
    d.v[0] = make_uint4(w[0], w[1], w[2], w[3]);
    d.v[1] = make_uint4(w[4], w[5], w[6], w[7]);
  }
  return d;
}

__device__ __forceinline__ WaveData load_tail_wave(const uint8_t* __restrict__ base, uint32_t len, int lane) {
  return load_tail_wave(base, len, lane, static_cast<int>(len));
}

// Short slice of `len` bytes, front-padded with zeros to 512 B (wave-wide call, lanes 0..7 work).
__device__ __forceinline__ uint32_t tail_crc(const DevCrcTables& lt, const uint8_t* base, uint32_t len, int lane) {
  const int sw = lane >> 3, sl = lane & 7;
  const uint32_t pad = 512u - len;
  uint32_t r = 0;
  if (sw == 0) {
    uint32_t words[16];
    for (int q = 0; q < 16; ++q) {
      uint32_t w = 0;
      for (int b = 0; b < 4; ++b) {
        uint32_t pos = sl * 64 + q * 4 + b;
        uint32_t byte = pos >= pad ? base[pos - pad] : 0u;
        w |= byte << (8 * b);
      }
      words[q] = w;
    }
    for (int q = 0; q < 4; ++q)
      r = chunk16(lt.slice16, r, make_uint4(words[4 * q], words[4 * q + 1], words[4 * q + 2], words[4 * q + 3]));
  }
  r = combine<1>(r, lane, lt.sh64);
  r = combine<2>(r, lane, lt.sh128);
  return combine<4>(r, lane, lt.sh256);
}

// Contiguous, balanced tile runs: workgroup b owns [b*T/G, (b+1)*T/G), so every workgroup
// gets floor or ceil of T/G tiles. (A ceil-sized split gave 64 MiB = 4096 tiles over 768
// workgroups as 683 runs of 6 — some CUs 18 tiles, others 12 — and left 85 slots idle.)
__device__ __forceinline__ uint64_t tile_run_begin(uint64_t ntiles, uint64_t b) {
  return b * ntiles / gridDim.x;
}

// LDS slicing-by-16 implementation (DFS_CRC_MFMA=0; the A/B baseline of crc_bench).
__global__ __launch_bounds__(kCrcWgThreads) void crc_slices_kernel(CrcLaunch a,
                                                                   const DevCrcTables* __restrict__ gt) {
  __shared__ DevCrcTables lt;
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t wg_bad;
  load_tables(gt, &lt);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sw = lane >> 3;   // slice within wave
  const int sl = lane & 7;    // 64 B sub-chunk within slice
  uint32_t acc = 0;
  uint32_t bad = 0xFFFFFFFFu;

  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    int64_t v = static_cast<int64_t>(t * kSlicesPerTile + wave * 8 + sw);
    int64_t i = static_cast<int64_t>(a.slice_lo) + v - static_cast<int64_t>(a.vfront);
    bool valid = i >= static_cast<int64_t>(a.slice_lo) && i < static_cast<int64_t>(a.slice_hi);
    uint32_t r = slice_crc(lt, a.data + (valid ? static_cast<uint64_t>(i) * 512 : 0), sl, lane, valid);
    if (valid && sl == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.full_init);
      if (a.meta_out) a.meta_out[i] = be;
      if (a.meta_host) a.meta_host[i] = be;
      if (a.meta_expect && a.meta_expect[i] != be) bad = min(bad, static_cast<uint32_t>(i));
    }
    if (a.part_crc) {
      r = combine<8>(r, lane, lt.sh512);
      r = combine<16>(r, lane, lt.sh1k);
      r = combine<32>(r, lane, lt.sh2k);
      if (lane == 0) wsum[wave] = r;
      __syncthreads();
      if (wave == 0) {
        uint32_t tv = wsum[0];
        tv = tab4(lt.sh4k, tv) ^ wsum[1];
        tv = tab4(lt.sh4k, tv) ^ wsum[2];
        tv = tab4(lt.sh4k, tv) ^ wsum[3];
        uint64_t e = a.ntiles - 1 - t;  // tiles that follow this one
        for (int b = 0; e; ++b, e >>= 1)
          if (e & 1) tv = mat_apply(lt.tile_pow2[b], tv, lane);
        acc ^= tv;
      }
      __syncthreads();
    }
  }

  // Short tail slice: front-pad the window with zeros (raw CRC is invariant to them).
  if (a.has_tail && blockIdx.x == 0 && wave == 0) {
    uint32_t r = tail_crc(lt, a.data + a.s_full * 512, a.tail_len, lane);
    if (lane == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.tail_init);
      if (a.meta_out) a.meta_out[a.s_full] = be;
      if (a.meta_host) a.meta_host[a.s_full] = be;
      if (a.meta_expect && a.meta_expect[a.s_full] != be) bad = min(bad, static_cast<uint32_t>(a.s_full));
    }
  }

  if (a.part_bad && bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.part_crc) a.part_crc[blockIdx.x] = acc;
    if (a.part_bad) a.part_bad[blockIdx.x] = wg_bad;
  }
}

// ---------------------------------------------------------------------------------------
// K1b: batched scrub over many blocks in one launch (see ScrubLaunch).
__global__ __launch_bounds__(kCrcWgThreads) void crc_scrub_kernel(ScrubLaunch a, const DevCrcTables* __restrict__ gt) {
  __shared__ DevCrcTables lt;
  load_tables(gt, &lt);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sw = lane >> 3, sl = lane & 7;
  for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    // last block whose tile range starts at or before t (workgroup-uniform)
    uint32_t lo = 0, hi = a.nblocks;
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (a.blocks[mid].tile_start <= t) lo = mid;
      else hi = mid;
    }
    const ScrubBlock& b = a.blocks[lo];
    uint64_t i = (t - b.tile_start) * kSlicesPerTile + wave * 8 + sw;
    bool valid = i < b.s_full;
    uint32_t r = slice_crc(lt, b.data + (valid ? i * 512 : 0), sl, lane, valid);
    if (valid && sl == 0 && b.meta[i] != __builtin_bswap32(r ^ a.full_init))
      atomicMin(&a.bad[lo], static_cast<uint32_t>(i));
  }
  // short tail slices: one wave per block
  const int waves = kCrcWgThreads / 64;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * waves + wave; k < a.nblocks;
       k += static_cast<uint64_t>(gridDim.x) * waves) {
    const ScrubBlock& b = a.blocks[k];
    if (!b.tail_len) continue;
    uint32_t r = tail_crc(lt, b.data + b.s_full * 512, b.tail_len, lane);
    if (lane == 0 && b.meta[b.s_full] != __builtin_bswap32(r ^ b.tail_init))
      atomicMin(&a.bad[k], static_cast<uint32_t>(b.s_full));
  }
}

// ---------------------------------------------------------------------------------------
// K1/K2/K3 on the matrix cores (default). Each workgroup owns a CONTIGUOUS run of 16 KiB
// tiles; each wave owns one 4 KiB sub-tile per tile and runs its own Horner accumulator for
// the whole-block CRC (consecutive sub-tiles of a wave are exactly one tile apart, so one
// lane-parallel GF(2) shift per tile) — no barrier inside the tile loop. The next tile's
// data is loaded while the current one is on the matrix cores, and the first tile's loads
// are issued before the LDS table fill, so a 1 MiB block costs one memory round trip.
// 3 waves/SIMD (168 VGPRs: the 64-VGPR basis + double-buffered data, no spills) x 4 SIMDs =
// 3 workgroups per CU, which their 32 KiB LDS images allow; the grid is sized to exactly one
// resident round (kMaxGridCrc = 3 x 256 CUs), so no second, partly empty round.
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void crc_tile_mfma_kernel(CrcLaunch a,
                                                                      const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaTileLds lt;
  __shared__ uint32_t wacc[4];
  __shared__ uint32_t wg_bad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  const int64_t lo = static_cast<int64_t>(a.slice_lo), hi = static_cast<int64_t>(a.slice_hi);
  auto first_slice = [&](uint64_t t) {
    return lo + static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(a.vfront);
  };
  WaveData cur;
  if (t_begin < t_end) cur = load_wave(a.data, first_slice(t_begin), lo, hi, lane);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  __syncthreads();

  uint32_t acc = 0;
  uint32_t bad = 0xFFFFFFFFu;
  for (uint64_t t = t_begin; t < t_end; ++t) {
    WaveData nxt;
    if (t + 1 < t_end) nxt = load_wave(a.data, first_slice(t + 1), lo, hi, lane);
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, cur, lane), lane);
    const int64_t i = first_slice(t) + sw;
    if (i >= lo && i < hi && sl == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.full_init);
      if (a.meta_out) a.meta_out[i] = be;
      if (a.meta_expect && a.meta_expect[i] != be) bad = min(bad, static_cast<uint32_t>(i));
    }
    if (a.part_crc) {
      r = combine<8>(r, lane, lt.sh512);
      r = combine<16>(r, lane, lt.sh1k);
      r = combine<32>(r, lane, lt.sh2k);  // wave-uniform: the 4 KiB sub-tile's raw CRC
      acc = mat_apply(lt.tile_pow2[0], acc, lane) ^ r;
    }
    if (t + 1 < t_end) cur = nxt;
  }

  if (a.has_tail && blockIdx.x == 0 && wave == 0) {
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(a.data + a.s_full * 512, a.tail_len, lane),
                                                       lane), lane);
    if (lane == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.tail_init);
      if (a.meta_out) a.meta_out[a.s_full] = be;
      if (a.meta_expect && a.meta_expect[a.s_full] != be) bad = min(bad, static_cast<uint32_t>(a.s_full));
    }
  }
  if (a.part_crc) {
    // place this wave's accumulator in the block: (3 - wave) sub-tiles of its last tile
    // and (ntiles - t_end) whole tiles follow it
    for (int k = wave; k < 3; ++k) acc = tab4(lt.sh4k, acc);
    uint64_t e = t_begin < t_end ? a.ntiles - t_end : 0;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) acc = mat_apply(lt.tile_pow2[b], acc, lane);
    if (lane == 0) wacc[wave] = acc;
  }
  if (a.part_bad && bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.part_crc) a.part_crc[blockIdx.x] = wacc[0] ^ wacc[1] ^ wacc[2] ^ wacc[3];
    if (a.part_bad) a.part_bad[blockIdx.x] = wg_bad;
  }
}

// K1/K2 with one workgroup per CU: kGroups groups of 4 waves share one LDS image and one
// LDS copy of the MFMA basis. Each group is a "virtual workgroup" of the kernel above (its own
// balanced tile run, partial word and verdict: part_crc/part_bad are indexed by
// blockIdx.x * kGroups + group, so the host sees the same `grid` words). The per-tile combine
// is two dependent table rounds instead of five: every lane of a slice group moves its slice
// CRC to the end of the wave's 4 KiB with one lookup in its own shift table (ss[sw], the
// slice-level twin of slice_from_chunks) and three xor-shuffles fold the sub-tile; the Horner
// step is one lookup in the 16 KiB shift table (all lanes the same value: an LDS broadcast)
// instead of a lane-parallel matrix apply with five shuffles. The image (68 KiB) only fits
// one workgroup per CU, which is what this kernel is.
struct MfmaWideLds {
  uint32_t cs[7][4][256];  // chunk -> slice (64 B * (7 - sl))
  uint32_t ss[7][4][256];  // slice -> sub-tile (512 B * (7 - sw))
  uint32_t sh16k[4][256];  // one tile
  uint32_t sh4k[4][256];   // one sub-tile (epilogue)
  uint32_t tile_pow2[32][32];
};
static_assert(offsetof(MfmaWideLds, sh4k) == kCrcChunkShiftBytes + kCrcWideExtraBytes, "wide image: contiguous head");
static_assert(sizeof(MfmaWideLds) - offsetof(MfmaWideLds, sh4k) == sizeof(DevCrcTables) - offsetof(DevCrcTables, sh4k),
              "wide image: DevCrcTables tail");

// kWrite: the K1/K2 write form (slice words out, whole-block partials, nothing to verify),
// with those checks resolved at compile time so the loop body has no uniform branches.
// kFp4: the chunk CRCs on the FP4 matrix cores (wave_chunk_crcs_fp4), else i8.
template <int kGroups, bool kWrite, bool kFp4 = false>
__global__ __launch_bounds__(kCrcWgThreads * kGroups) __attribute__((amdgpu_waves_per_eu(kGroups, kGroups)))
void crc_tile_wide_kernel(CrcLaunch a, const DevCrcTables* __restrict__ gt) {
  constexpr int kThreads = kCrcWgThreads * kGroups;
  constexpr int kFrags = kFp4 ? 8 : 16;  // A fragments per lane
  __shared__ __attribute__((aligned(16))) MfmaWideLds lt;
  __shared__ i32x4 lbasis[kFrags * 64];
  __shared__ uint32_t wacc[4 * kGroups];
  __shared__ uint32_t wg_bad[kGroups];
  const int lane = threadIdx.x & 63, gw = threadIdx.x >> 6, wave = gw & 3, grp = gw >> 2, sw = lane >> 3,
            sl = lane & 7;
  const uint64_t vb = static_cast<uint64_t>(blockIdx.x) * kGroups + grp, vg = static_cast<uint64_t>(gridDim.x) * kGroups;
  const uint64_t t_begin = vb * a.ntiles / vg, t_end = (vb + 1) * a.ntiles / vg;
  const int64_t lo = static_cast<int64_t>(a.slice_lo), hi = static_cast<int64_t>(a.slice_hi);
  auto first_slice = [&](uint64_t t) {
    return lo + static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(a.vfront);
  };
  // unconditional loads (load_wave_ring: out-of-block slices re-read slice lo, and their chunk
  // CRCs are zeroed below), so no exec-masked branches around the loads in the loop
  WaveData cur;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(gt + 1);
  if constexpr (kFp4) {
    // the LDS image and basis by LDS-DMA, all in flight together with the first tile's loads
    dma16<kThreads>(img + kCrcBasisFp4Offset, lbasis, kCrcBasisFp4Bytes);
    dma16<kThreads>(img + kCrcBasisBytes, &lt, kCrcChunkShiftBytes + kCrcWideExtraBytes);
    dma16<kThreads>(&gt->sh4k, &lt.sh4k, static_cast<int>(sizeof(DevCrcTables) - offsetof(DevCrcTables, sh4k)));
    if (t_begin < t_end) cur = load_wave_ring(a.data, first_slice(t_begin), lo, hi, lane);
  } else {
    if (t_begin < t_end) cur = load_wave_ring(a.data, first_slice(t_begin), lo, hi, lane);
    copy16<kThreads>(img, lbasis, kCrcBasisBytes);
    copy16<kThreads>(img + kCrcBasisBytes, &lt, kCrcChunkShiftBytes + kCrcWideExtraBytes);
    copy16<kThreads>(&gt->sh4k, &lt.sh4k, static_cast<int>(sizeof(DevCrcTables) - offsetof(DevCrcTables, sh4k)));
  }
  if (threadIdx.x < kGroups) wg_bad[threadIdx.x] = 0xFFFFFFFFu;
  __syncthreads();
  i32x4 A[kFrags];
#pragma unroll
  for (int s = 0; s < kFrags; ++s) A[s] = lbasis[s * 64 + lane];
  auto chunk_crcs = [&](const WaveData& d) {
    if constexpr (kFp4) return wave_chunk_crcs_fp4(A, d, lane);
    else return wave_chunk_crcs(A, d, lane);
  };

  uint32_t acc = 0;
  uint32_t bad = 0xFFFFFFFFu;
  // tile t's combine (table lookups and shuffles: a latency chain) is issued after tile t+1's
  // matrix-core work, so each wave has independent MFMAs to issue while its lookups are out
  auto finish = [&](uint32_t c, uint64_t t) {
    const int64_t i = first_slice(t) + sw;
    const bool valid = i >= lo && i < hi;
    uint32_t r = slice_from_chunks(lt, valid ? c : 0u, lane);
    if (valid && sl == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.full_init);
      if (kWrite || a.meta_out) a.meta_out[i] = be;
      if (!kWrite && a.meta_expect && a.meta_expect[i] != be) bad = min(bad, static_cast<uint32_t>(i));
    }
    if (kWrite || a.part_crc) {
      uint32_t v = sw < 7 ? tab4(lt.ss[sw], r) : r;
      v = xr32(xr16(xr8(v)));  // wave-uniform: the 4 KiB sub-tile's raw CRC
      acc = tab4(lt.sh16k, acc) ^ v;
    }
  };
  uint32_t cprev = 0;
  for (uint64_t t = t_begin; t < t_end; ++t) {
    WaveData nxt;
    if (t + 1 < t_end) nxt = load_wave_ring(a.data, first_slice(t + 1), lo, hi, lane);
    const uint32_t c = chunk_crcs(cur);
    if (t > t_begin) finish(cprev, t - 1);
    cprev = c;
    if (t + 1 < t_end) cur = nxt;
  }
  if (t_begin < t_end) finish(cprev, t_end - 1);

  if (a.has_tail && vb == 0 && wave == 0) {
    uint32_t r = slice_from_chunks(lt, chunk_crcs(load_tail_wave(a.data + a.s_full * 512, a.tail_len, lane)), lane);
    if (lane == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.tail_init);
      if (a.meta_out) a.meta_out[a.s_full] = be;
      if (a.meta_expect && a.meta_expect[a.s_full] != be) bad = min(bad, static_cast<uint32_t>(a.s_full));
    }
  }
  if (a.part_crc) {
    for (int k = wave; k < 3; ++k) acc = tab4(lt.sh4k, acc);
    uint64_t e = t_begin < t_end ? a.ntiles - t_end : 0;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) acc = mat_apply(lt.tile_pow2[b], acc, lane);
    if (lane == 0) wacc[gw] = acc;
  }
  if (a.part_bad && bad != 0xFFFFFFFFu) atomicMin(&wg_bad[grp], bad);
  __syncthreads();
  if (threadIdx.x < kGroups) {
    const int g = threadIdx.x;
    const uint64_t v = static_cast<uint64_t>(blockIdx.x) * kGroups + g;
    if (a.part_crc) a.part_crc[v] = wacc[4 * g] ^ wacc[4 * g + 1] ^ wacc[4 * g + 2] ^ wacc[4 * g + 3];
    if (a.part_bad) a.part_bad[v] = wg_bad[g];
  }
}

// K3 fused: verify AND deliver a read in one pass over HBM. The data the MFMA chunk CRC
// already holds in registers is stored straight to the reader's buffer — host memory that
// the store registered (the client's shared-memory slot), so the stores cross PCIe from the
// CUs — instead of a verify kernel followed by an SDMA copy that reads the same bytes from
// HBM again, plus a second small copy for the verdict. Only bytes inside [off, off + len)
// are stored; the verdict per workgroup goes to host-visible memory too, so one kernel and
// one stream sync make the whole read. The host guarantees (out - off) % 16 == 0.
// Bytes of lane segment `q` (0..7, dwords of the lane's 32 B) of iteration `it`.
__device__ __forceinline__ uint32_t seg_dword(const WaveData& d, int it, int q) {
  const uint4 v = d.v[2 * it + (q >> 2)];
  const int k = q & 3;
  return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
}

__device__ __forceinline__ void store_wave(const ReadCopyLaunch& a, int64_t i0, const WaveData& d, int lane) {
  const int n = lane & 31, h = lane >> 5;
  const int64_t lo = static_cast<int64_t>(a.c.slice_lo), hi = static_cast<int64_t>(a.c.slice_hi);
  const uint64_t end = a.off + a.len;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = it * 32 + n;
    const int64_t i = i0 + (c >> 3);
    if (i < lo || i >= hi) continue;
    const uint64_t pos = static_cast<uint64_t>(i) * 512 + (c & 7) * 64 + h * 32;
    if (pos >= a.off && pos + 32 <= end) {
      uint4* dst = reinterpret_cast<uint4*>(a.out + (pos - a.off));
      dst[0] = d.v[2 * it];
      dst[1] = d.v[2 * it + 1];
    } else if (pos + 32 > a.off && pos < end) {  // the range's first / last 32 B
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const uint32_t w = seg_dword(d, it, q);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint64_t p = pos + 4 * q + b;
          if (p >= a.off && p < end) a.out[p - a.off] = static_cast<uint8_t>(w >> (8 * b));
        }
      }
    }
  }
}

__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void crc_read_copy_kernel(
    ReadCopyLaunch a, const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaSliceLds lt;
  __shared__ uint32_t wg_bad;
  const CrcLaunch& c = a.c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(c.ntiles, blockIdx.x), t_end = tile_run_begin(c.ntiles, blockIdx.x + 1);
  const int64_t lo = static_cast<int64_t>(c.slice_lo), hi = static_cast<int64_t>(c.slice_hi);
  auto first_slice = [&](uint64_t t) { return lo + static_cast<int64_t>(t * kSlicesPerTile + wave * 8); };
  WaveData cur;
  if (t_begin < t_end) cur = load_wave(c.data, first_slice(t_begin), lo, hi, lane);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  __syncthreads();

  uint32_t bad = 0xFFFFFFFFu;
  for (uint64_t t = t_begin; t < t_end; ++t) {
    WaveData nxt;
    if (t + 1 < t_end) nxt = load_wave(c.data, first_slice(t + 1), lo, hi, lane);
    const int64_t i0 = first_slice(t);
    store_wave(a, i0, cur, lane);
    const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, cur, lane), lane);
    const int64_t i = i0 + sw;
    if (i >= lo && i < hi && sl == 0 && c.meta_expect[i] != __builtin_bswap32(r ^ c.full_init))
      bad = min(bad, static_cast<uint32_t>(i));
    if (t + 1 < t_end) cur = nxt;
  }

  if (c.has_tail && blockIdx.x == 0 && wave == 0) {
    const uint8_t* base = c.data + c.s_full * 512;
    const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(base, c.tail_len, lane), lane), lane);
    if (lane == 0 && c.meta_expect[c.s_full] != __builtin_bswap32(r ^ c.tail_init))
      bad = min(bad, static_cast<uint32_t>(c.s_full));
    const uint64_t p0 = c.s_full * 512, end = a.off + a.len;
    for (uint32_t k = lane; k < c.tail_len; k += 64) {
      const uint64_t p = p0 + k;
      if (p >= a.off && p < end) a.out[p - a.off] = base[k];
    }
  }
  if (bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) a.part_bad[blockIdx.x] = wg_bad;
}

// K1/K2 fused with the host-to-device copy of a write (the mirror of crc_read_copy_kernel):
// the waves load the block straight from the writer's registered host slot over PCIe, store
// it into the HBM extent, checksum the registers they already hold on the matrix cores, and
// write the .meta image both next to the block in HBM and into host-visible memory together
// with the whole-block partials — one kernel and one stream sync instead of an SDMA copy,
// the checksum kernel and two device-to-host copies (the .meta image and the partials).
__device__ __forceinline__ void store_wave_dst(uint8_t* __restrict__ dst, int64_t i0, int64_t lo, int64_t hi,
                                               const WaveData& d, int lane) {
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = it * 32 + n;
    const int64_t i = i0 + (c >> 3);
    if (i < lo || i >= hi) continue;
    uint4* p = reinterpret_cast<uint4*>(dst + static_cast<uint64_t>(i) * 512 + (c & 7) * 64 + h * 32);
    p[0] = d.v[2 * it];
    p[1] = d.v[2 * it + 1];
  }
}

__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void crc_write_copy_kernel(
    WriteCopyLaunch a, const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaTileLds lt;
  __shared__ uint32_t wacc[4];
  const CrcLaunch& c = a.c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(c.ntiles, blockIdx.x), t_end = tile_run_begin(c.ntiles, blockIdx.x + 1);
  const int64_t lo = static_cast<int64_t>(c.slice_lo), hi = static_cast<int64_t>(c.slice_hi);
  auto first_slice = [&](uint64_t t) {
    return lo + static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(c.vfront);
  };
  WaveData cur;
  if (t_begin < t_end) cur = load_wave(c.data, first_slice(t_begin), lo, hi, lane);  // PCIe latency first
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  __syncthreads();

  uint32_t acc = 0;
  for (uint64_t t = t_begin; t < t_end; ++t) {
    WaveData nxt;
    if (t + 1 < t_end) nxt = load_wave(c.data, first_slice(t + 1), lo, hi, lane);
    const int64_t i0 = first_slice(t);
    store_wave_dst(a.dst, i0, lo, hi, cur, lane);
    if (a.dst_host) store_wave_dst(a.dst_host, i0, lo, hi, cur, lane);
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, cur, lane), lane);
    const int64_t i = i0 + sw;
    if (i >= lo && i < hi && sl == 0) {
      const uint32_t be = __builtin_bswap32(r ^ c.full_init);
      c.meta_out[i] = be;
      a.meta_host[i] = be;
    }
    r = combine<8>(r, lane, lt.sh512);
    r = combine<16>(r, lane, lt.sh1k);
    r = combine<32>(r, lane, lt.sh2k);
    acc = mat_apply(lt.tile_pow2[0], acc, lane) ^ r;
    if (t + 1 < t_end) cur = nxt;
  }

  if (c.has_tail && blockIdx.x == 0 && wave == 0) {
    const uint8_t* base = c.data + c.s_full * 512;
    const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(base, c.tail_len, lane), lane), lane);
    if (lane == 0) {
      const uint32_t be = __builtin_bswap32(r ^ c.tail_init);
      c.meta_out[c.s_full] = be;
      a.meta_host[c.s_full] = be;
    }
    uint8_t* out = a.dst + c.s_full * 512;
    uint8_t* hout = a.dst_host ? a.dst_host + c.s_full * 512 : nullptr;
    for (uint32_t k = lane; k < c.tail_len; k += 64) {
      out[k] = base[k];
      if (hout) hout[k] = base[k];
    }
  }
  for (int k = wave; k < 3; ++k) acc = tab4(lt.sh4k, acc);
  uint64_t e = t_begin < t_end ? c.ntiles - t_end : 0;
  for (int b = 0; e; ++b, e >>= 1)
    if (e & 1) acc = mat_apply(lt.tile_pow2[b], acc, lane);
  if (lane == 0) wacc[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) c.part_crc[blockIdx.x] = wacc[0] ^ wacc[1] ^ wacc[2] ^ wacc[3];
}

// K1b on the matrix cores: contiguous tile runs per workgroup, so the tile -> block lookup is
// one binary search per workgroup and then a forward walk, and the next tile's data (and its
// block) are fetched while the current tile computes.
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void crc_scrub_mfma_kernel(ScrubLaunch a,
                                                                       const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaSliceLds lt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  uint32_t blk = 0;
  if (t_begin < t_end) {
    uint32_t l = 0, h = a.nblocks;
    while (h - l > 1) {
      uint32_t mid = (l + h) >> 1;
      if (a.blocks[mid].tile_start <= t_begin) l = mid;
      else h = mid;
    }
    blk = l;
  }
  auto advance = [&](uint64_t t, uint32_t b) {
    while (b + 1 < a.nblocks && a.blocks[b + 1].tile_start <= t) ++b;
    return b;
  };
  auto first_slice = [&](uint64_t t, uint32_t b) {
    return static_cast<int64_t>((t - a.blocks[b].tile_start) * kSlicesPerTile + wave * 8);
  };
  WaveData cur;
  if (t_begin < t_end)
    cur = load_wave(a.blocks[blk].data, first_slice(t_begin, blk), 0, static_cast<int64_t>(a.blocks[blk].s_full), lane);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  __syncthreads();
  for (uint64_t t = t_begin; t < t_end; ++t) {
    WaveData nxt;
    uint32_t nb = blk;
    if (t + 1 < t_end) {
      nb = advance(t + 1, blk);
      nxt = load_wave(a.blocks[nb].data, first_slice(t + 1, nb), 0, static_cast<int64_t>(a.blocks[nb].s_full), lane);
    }
    const ScrubBlock& b = a.blocks[blk];
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, cur, lane), lane);
    const int64_t i = first_slice(t, blk) + sw;
    if (sl == 0 && i < static_cast<int64_t>(b.s_full) && b.meta[i] != __builtin_bswap32(r ^ a.full_init))
      atomicMin(&a.bad[blk], static_cast<uint32_t>(i));
    if (t + 1 < t_end) {
      cur = nxt;
      blk = nb;
    }
  }
  const int waves = kCrcWgThreads / 64;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * waves + wave; k < a.nblocks;
       k += static_cast<uint64_t>(gridDim.x) * waves) {
    const ScrubBlock& b = a.blocks[k];
    if (!b.tail_len) continue;
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(b.data + b.s_full * 512, b.tail_len, lane),
                                                       lane), lane);
    if (lane == 0 && b.meta[b.s_full] != __builtin_bswap32(r ^ b.tail_init))
      atomicMin(&a.bad[k], static_cast<uint32_t>(b.s_full));
  }
}



// ---------------------------------------------------------------------------------------
// Deep-ring variants of the two MFMA kernels (R = 3..4 buffers: crc_ring_buffers() for the
// scrub, crc_tile_ring_buffers() for K1/K2/K3, see gpu_kernels.h for the defaults; deeper
// rings spill at the 256-VGPR budget of 2 waves/SIMD).
// The kernels stream every byte once, so what bounds them is the data in flight per CU, not
// the matrix cores (32 MFMAs per 4 KiB per wave ≈ 9.8 TB/s at full rate): the kernels above
// keep one tile in flight per wave at 3 waves/SIMD. Here each wave keeps R-1 tiles in flight
// in a register ring (16 VGPRs per buffer) at 2 waves/SIMD (grid 512 = one resident round).
// For the compiler to wait with a counted vmcnt(N) instead of draining the ring:
//  * the ring loads are unconditional (tiles past the run re-read its last tile, slices
//    outside the block read slice lo and their chunk CRCs are zeroed), and the loop
//    runs whole groups of R tiles with the remainder (already loaded) after it;
//  * nothing else in the loop is a global load whose result is used: the expected .meta word
//    of a lane's slice is loaded with its data, and the scrub's block table is read through
//    the constant address space (scalar loads; the table is read-only for the launch, and
//    the atomics on `bad` would otherwise make the compiler treat it as clobbered).
template <int R>
struct Ring {
  WaveData b[R];
  uint32_t expect[R];
};

template <int R>
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void crc_tile_ring_kernel(CrcLaunch a, const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaTileLds lt;
  __shared__ uint32_t wacc[4];
  __shared__ uint32_t wg_bad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  const int64_t lo = static_cast<int64_t>(a.slice_lo), hi = static_cast<int64_t>(a.slice_hi);
  auto first_slice = [&](uint64_t t) {
    return lo + static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(a.vfront);
  };
  Ring<R> ring;
  auto load = [&](int slot, uint64_t t) {
    t = t < t_end ? t : t_end - 1;
    const int64_t i0 = first_slice(t), i = i0 + sw;
    ring.b[slot] = load_wave_ring(a.data, i0, lo, hi, lane);
    ring.expect[slot] = a.meta_expect ? a.meta_expect[(i >= lo && i < hi) ? i : lo] : 0u;
  };
  const bool work = t_begin < t_end;  // workgroup-uniform
  if (work) {
#pragma unroll
    for (int k = 0; k < R - 1; ++k) load(k, t_begin + k);
  }
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  __syncthreads();

  uint32_t acc = 0;
  uint32_t bad = 0xFFFFFFFFu;
  auto step = [&](int slot, uint64_t t) {
    const int64_t i = first_slice(t) + sw;
    const bool valid = i >= lo && i < hi;
    const uint32_t c = wave_chunk_crcs(A, ring.b[slot], lane);
    uint32_t r = slice_from_chunks(lt, valid ? c : 0u, lane);
    if (valid && sl == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.full_init);
      if (a.meta_out) a.meta_out[i] = be;
      if (a.meta_expect && ring.expect[slot] != be) bad = min(bad, static_cast<uint32_t>(i));
    }
    if (a.part_crc) {
      r = combine<8>(r, lane, lt.sh512);
      r = combine<16>(r, lane, lt.sh1k);
      r = combine<32>(r, lane, lt.sh2k);  // wave-uniform: the 4 KiB sub-tile's raw CRC
      acc = mat_apply(lt.tile_pow2[0], acc, lane) ^ r;
    }
  };
  uint64_t t0 = t_begin;
  if (work) {
    for (; t0 + R <= t_end; t0 += R) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        load((k + R - 1) % R, t0 + k + R - 1);
        step(k, t0 + k);
      }
    }
#pragma unroll
    for (int k = 0; k < R - 1; ++k)
      if (t0 + k < t_end) step(k, t0 + k);  // loaded by the last group (or the prologue)
  }

  if (a.has_tail && blockIdx.x == 0 && wave == 0) {
    uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(a.data + a.s_full * 512, a.tail_len, lane),
                                                       lane), lane);
    if (lane == 0) {
      uint32_t be = __builtin_bswap32(r ^ a.tail_init);
      if (a.meta_out) a.meta_out[a.s_full] = be;
      if (a.meta_expect && a.meta_expect[a.s_full] != be) bad = min(bad, static_cast<uint32_t>(a.s_full));
    }
  }
  if (a.part_crc) {
    for (int k = wave; k < 3; ++k) acc = tab4(lt.sh4k, acc);
    uint64_t e = work ? a.ntiles - t_end : 0;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) acc = mat_apply(lt.tile_pow2[b], acc, lane);
    if (lane == 0) wacc[wave] = acc;
  }
  if (a.part_bad && bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.part_crc) a.part_crc[blockIdx.x] = wacc[0] ^ wacc[1] ^ wacc[2] ^ wacc[3];
    if (a.part_bad) a.part_bad[blockIdx.x] = wg_bad;
  }
}

using ConstScrubBlock = const __attribute__((address_space(4))) ScrubBlock;

template <int R, bool kFp4 = false>
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
void crc_scrub_ring_kernel(ScrubLaunch a, const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaSliceLds lt;
  ConstScrubBlock* blocks = (ConstScrubBlock*)a.blocks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  const bool work = t_begin < t_end;  // workgroup-uniform
  uint32_t blk = 0;
  if (work) {
    uint32_t l = 0, h = a.nblocks;
    while (h - l > 1) {
      uint32_t mid = (l + h) >> 1;
      if (blocks[mid].tile_start <= t_begin) l = mid;
      else h = mid;
    }
    blk = l;
  }
  auto advance = [&](uint64_t t, uint32_t b) {
    while (b + 1 < a.nblocks && blocks[b + 1].tile_start <= t) ++b;
    return b;
  };
  Ring<R> ring;
  uint32_t lblk = blk;  // block of the next tile to load (non-decreasing: clamped tiles are too)
  auto load = [&](int slot, uint64_t t) {
    t = t < t_end ? t : t_end - 1;
    lblk = advance(t, lblk);
    const uint8_t* data = blocks[lblk].data;
    const uint32_t* meta = blocks[lblk].meta;
    const int64_t i0 = static_cast<int64_t>((t - blocks[lblk].tile_start) * kSlicesPerTile + wave * 8);
    const int64_t hi = static_cast<int64_t>(blocks[lblk].s_full);
    ring.b[slot] = load_wave_ring(data, i0, 0, hi, lane);
    ring.expect[slot] = meta[i0 + sw < hi ? i0 + sw : 0];
  };
  if (work) {
#pragma unroll
    for (int k = 0; k < R - 1; ++k) load(k, t_begin + k);
  }
  ChunkBasis<kFp4> basis;
  basis.load(gt, lane);
  load_lds_image(gt, &lt);
  __syncthreads();
  auto step = [&](int slot, uint64_t t) {
    blk = advance(t, blk);
    const int64_t i0 = static_cast<int64_t>((t - blocks[blk].tile_start) * kSlicesPerTile + wave * 8);
    const int64_t hi = static_cast<int64_t>(blocks[blk].s_full);
    // slices past the block end are never compared, so their (re-read) data needs no masking
    uint32_t r = slice_from_chunks(lt, basis.crcs(ring.b[slot], lane), lane);
    const int64_t i = i0 + sw;
    if (sl == 0 && i < hi && ring.expect[slot] != __builtin_bswap32(r ^ a.full_init))
      atomicMin(&a.bad[blk], static_cast<uint32_t>(i));
  };
  if (work) {
    uint64_t t0 = t_begin;
    for (; t0 + R <= t_end; t0 += R) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        load((k + R - 1) % R, t0 + k + R - 1);
        step(k, t0 + k);
      }
    }
#pragma unroll
    for (int k = 0; k < R - 1; ++k)
      if (t0 + k < t_end) step(k, t0 + k);
  }
  const int waves = kCrcWgThreads / 64;
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * waves + wave; k < a.nblocks;
       k += static_cast<uint64_t>(gridDim.x) * waves) {
    ConstScrubBlock& b = blocks[k];
    if (!b.tail_len) continue;
    uint32_t r = slice_from_chunks(lt, basis.crcs(load_tail_wave(b.data + b.s_full * 512, b.tail_len, lane), lane), lane);
    if (lane == 0 && b.meta[b.s_full] != __builtin_bswap32(r ^ b.tail_init))
      atomicMin(&a.bad[k], static_cast<uint32_t>(b.s_full));
  }
}

// ---------------------------------------------------------------------------------------
// Roofline probe for the benches: a plain streaming read of n bytes (16 B per lane, four
// loads in flight per lane, non-temporal like the CRC kernels) XOR-folded into one word per
// workgroup. Its TB/s on the same box is what "fraction of achievable HBM" divides by.
__global__ __launch_bounds__(256) void stream_read_kernel(const uint4* __restrict__ p, uint64_t nvec, uint32_t* out) {
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  uint32_t x = 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    u32x4 a = __builtin_nontemporal_load(q + i), b = __builtin_nontemporal_load(q + i + stride);
    u32x4 c = __builtin_nontemporal_load(q + i + 2 * stride), d = __builtin_nontemporal_load(q + i + 3 * stride);
    a ^= b ^ c ^ d;
    x ^= a[0] ^ a[1] ^ a[2] ^ a[3];
  }
  for (; i < nvec; i += stride) {
    u32x4 a = __builtin_nontemporal_load(q + i);
    x ^= a[0] ^ a[1] ^ a[2] ^ a[3];
  }
  for (int m = 32; m; m >>= 1) x ^= __shfl_xor(x, m);
  if ((threadIdx.x & 63) == 0) out[blockIdx.x * 4 + (threadIdx.x >> 6)] = x;
}

// ---------------------------------------------------------------------------------------
// GF(2^8) shard matrix multiply (K4 encode / K5 reconstruct): out[r] = XOR_c mat[r][c] * in[c].
// Branch-free split-nibble form (ISA-L style): c * x = T_lo[x & 15] ^ T_hi[x >> 4], with the
// two 16-byte tables per coefficient looked up four bytes at a time by v_perm_b32 (a byte
// shuffle over an 8-byte table pair; bit 3 of the nibble picks the half through v_bfi_b32).
// Per input dword the nibble selectors are prepared once and reused for every output row;
// the tables of one (row, input) pair are wave-uniform and sit in scalar registers. No LDS,
// no data-dependent branches: ~8 VALU ops per input byte for RS(6,3), far under the VALU
// rate needed to keep up with HBM.
struct NibbleSel {
  uint32_t lo7, lo_m, hi7, hi_m;
};

__device__ __forceinline__ NibbleSel nibble_sel(uint32_t x) {
  NibbleSel n;
  n.lo7 = x & 0x07070707u;
  n.hi7 = (x >> 4) & 0x07070707u;
  // bit 3 of each nibble -> 0x00 / 0xFF per byte (perm selector 12 = 0x00, 13 = 0xFF)
  n.lo_m = __builtin_amdgcn_perm(0u, 0u, ((x >> 3) & 0x01010101u) | 0x0C0C0C0Cu);
  n.hi_m = __builtin_amdgcn_perm(0u, 0u, ((x >> 7) & 0x01010101u) | 0x0C0C0C0Cu);
  return n;
}

// t[0..3]: low-nibble table bytes 0..15, t[4..7]: high-nibble table.
__device__ __forceinline__ uint32_t gf_mul4(const uint32_t* __restrict__ t, const NibbleSel& n) {
  uint32_t a = __builtin_amdgcn_perm(t[1], t[0], n.lo7), b = __builtin_amdgcn_perm(t[3], t[2], n.lo7);
  uint32_t c = __builtin_amdgcn_perm(t[5], t[4], n.hi7), d = __builtin_amdgcn_perm(t[7], t[6], n.hi7);
  return ((a & ~n.lo_m) | (b & n.lo_m)) ^ ((c & ~n.hi_m) | (d & n.hi_m));
}

constexpr int kGfRowBlock = 4;

__global__ __launch_bounds__(256) void gf256_matmul_kernel(GfLaunch a) {
  const uint64_t nvec = (a.len + 15) / 16;
  for (uint64_t vi = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; vi < nvec;
       vi += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    for (int r0 = 0; r0 < a.rows; r0 += kGfRowBlock) {
      uint32_t acc[kGfRowBlock][4] = {};
      for (int c = 0; c < a.k; ++c) {
        const uint4 w = reinterpret_cast<const uint4*>(a.in[c])[vi];
        const NibbleSel ns[4] = {nibble_sel(w.x), nibble_sel(w.y), nibble_sel(w.z), nibble_sel(w.w)};
#pragma unroll
        for (int rr = 0; rr < kGfRowBlock; ++rr) {
          const int r = r0 + rr;
          if (r >= a.rows) break;
          const uint32_t* t = a.tables + (r * a.k + c) * 8;  // uniform: scalar loads
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[rr][q] ^= gf_mul4(t, ns[q]);
        }
      }
      for (int rr = 0; rr < kGfRowBlock; ++rr) {
        int r = r0 + rr;
        if (r >= a.rows) break;
        reinterpret_cast<uint4*>(a.out[r])[vi] = make_uint4(acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// K4/K5 fused with K2: one pass over an RS stripe. The tile axis is the shard-relative 16 KiB
// tile of a whole-block checksum plan (virtual front padding, balanced contiguous runs per
// workgroup), and the same run is walked for every shard of the stripe. Per tile a wave loads
// its 4 KiB of input c (encode: over PCIe from the writer's registered slot, prefetching the
// next input or tile behind the current one's arithmetic), stores it into the shard's HBM
// extent, checksums it on the matrix cores from the registers it sits in and multiplies it into
// R parity accumulators that stay in VGPRs; after input k-1 the accumulators are stored and
// checksummed the same way, so no shard byte is read twice and parity is never read at all.
//  * Each wave keeps a running whole-shard partial per shard. Up to 32 of them are indexed by a
//    loop variable, so they live in LDS (one word per wave and shard; the wave's own lanes are
//    the only readers and writers inside the loop), not in a register array.
//  * The GF split-nibble tables are read once per workgroup through the device view of the
//    lane's pinned scratch into LDS (no table copy on the stream); the wave-uniform tables of
//    one (row, input) pair are LDS broadcasts.
//  * Short tail slice: byte-wise GF products keep the zero front padding of load_tail_wave, so
//    the parity tail is the XOR of the products in that layout, checksummed like a data tail and
//    stored byte-wise at the unpadded positions.
//  * Reconstruct mode (kEncode = false): inputs are verified HBM shards — no input stores or
//    checksums, only the R outputs.
// Register budget: FP4 basis 32 VGPRs (the i8 form's 64 buy nothing here: encode is bound by
// PCIe, reconstruct by the v_perm_b32 rate) + two WaveData 32 + R WaveData of parity + R x 8 table
// dwords + the 16 MFMA accumulators + one 16 B group's 16 selector registers: ~200 at R = 4
// before addresses and temporaries. That is over the 168 of 3 waves/SIMD for every R, so
// R <= 3 runs at 2 waves/SIMD (256 registers, two workgroups per CU) and R = 4, which does not
// fit 256 without scratch, at 1 wave/SIMD (one workgroup per CU; the overflow sits in AGPRs).
// The next input's loads are in flight behind the arithmetic either way. LDS: 48 KiB image +
// R KiB tables + 512 B partials. The compiler's report (-Rpass-analysis=kernel-resource-usage,
// gfx950; VGPRs + AGPRs / LDS bytes / waves per SIMD; scratch is 0 in all eight):
//   R  reconstruct             encode
//   1  203      / 50688 / 2    210      / 50688 / 2
//   2  195      / 51712 / 2    210      / 51712 / 2
//   3  237      / 52736 / 2    252      / 52736 / 2
//   4  256 + 62 / 53760 / 1    256 + 86 / 53760 / 1
template <int R>
__device__ __forceinline__ void gf_accumulate(const uint32_t* __restrict__ t, int k, int c, const WaveData& d,
                                              WaveData (&pacc)[R]) {
  uint32_t tb[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < 8; ++j) tb[r][j] = t[(r * k + c) * 8 + j];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    // the selectors of an input dword are prepared once and reused for every row
    const NibbleSel n0 = nibble_sel(d.v[v].x), n1 = nibble_sel(d.v[v].y), n2 = nibble_sel(d.v[v].z),
                    n3 = nibble_sel(d.v[v].w);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      pacc[r].v[v].x ^= gf_mul4(tb[r], n0);
      pacc[r].v[v].y ^= gf_mul4(tb[r], n1);
      pacc[r].v[v].z ^= gf_mul4(tb[r], n2);
      pacc[r].v[v].w ^= gf_mul4(tb[r], n3);
    }
    // one 16 B group at a time: interleaving the four groups keeps 64 selector registers live
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Mirror of load_tail_wave: the bytes of the front-padded slice back to their unpadded places.
__device__ __forceinline__ void store_tail_wave(uint8_t* __restrict__ base, uint32_t len, const WaveData& d, int lane) {
  const int n = lane & 31, h = lane >> 5;
  if (n >= 8) return;
  const int pad = 512 - static_cast<int>(len);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint32_t w = seg_dword(d, 0, q);
    for (int b = 0; b < 4; ++b) {
      const int pos = n * 64 + h * 32 + q * 4 + b;
      if (pos >= pad) base[pos - pad] = static_cast<uint8_t>(w >> (8 * b));
    }
  }
}

// The checksum side of the stripe kernels (ec_fused_kernel, ec_convert_kernel) works on the LDS
// image, the FP4 basis in VGPRs and one running whole-shard partial per wave and shard.
using StripeParts = uint32_t[4][kMaxShards];

// slice CRCs of the wave's 4 KiB of shard s -> its .meta words and the wave's running partial
__device__ __forceinline__ void checksum(const EcFusedLaunch& a, const MfmaTileLds& lt, StripeParts& part,
                                         const ChunkBasis<true>& basis, int s, int64_t i0, const WaveData& d, int lane) {
  const int wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const int64_t hi = static_cast<int64_t>(a.s_full);
  uint32_t r = slice_from_chunks(lt, basis.crcs(d, lane), lane);
  const int64_t i = i0 + sw;
  if (i >= 0 && i < hi && sl == 0) a.meta[s][i] = __builtin_bswap32(r ^ a.full_init);
  r = combine<8>(r, lane, lt.sh512);
  r = combine<16>(r, lane, lt.sh1k);
  r = combine<32>(r, lane, lt.sh2k);
  const uint32_t acc = mat_apply(lt.tile_pow2[0], part[wave][s], lane) ^ r;
  if (lane == 0) part[wave][s] = acc;
}

// the short tail slice of shard s, front-padded in `d`: its .meta word, and the bytes into `shard`
__device__ __forceinline__ void checksum_tail(const EcFusedLaunch& a, const MfmaTileLds& lt,
                                              const ChunkBasis<true>& basis, int s, uint8_t* __restrict__ shard,
                                              const WaveData& d, int lane) {
  const uint32_t r = slice_from_chunks(lt, basis.crcs(d, lane), lane);
  if (lane == 0) {
    const uint32_t be = __builtin_bswap32(r ^ a.tail_init);
    a.meta[s][a.s_full] = be;
    a.tail_be[s] = be;
  }
  store_tail_wave(shard + a.s_full * 512, a.tail_len, d, lane);
}

// place the partials in the shard: (3 - wave) sub-tiles of the wave's last tile follow its
// accumulator (lane s shifts shard s), then — the shifts are linear, so once for the XOR of
// the four waves — the (ntiles - t_end) whole tiles behind the workgroup's run
__device__ __forceinline__ void place_partials(const EcFusedLaunch& a, const MfmaTileLds& lt, StripeParts& part, int nsh,
                                               uint64_t t_begin, uint64_t t_end, int lane) {
  const int wave = threadIdx.x >> 6;
  if (lane < nsh) {
    uint32_t v = part[wave][lane];
    for (int j = wave; j < 3; ++j) v = tab4(lt.sh4k, v);
    part[wave][lane] = v;
  }
  __syncthreads();
  for (int s = wave; s < nsh; s += 4) {
    uint32_t v = part[0][s] ^ part[1][s] ^ part[2][s] ^ part[3][s];
    uint64_t e = t_begin < t_end ? a.ntiles - t_end : 0;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) v = mat_apply(lt.tile_pow2[b], v, lane);
    if (lane == 0) a.part_crc[s * kMaxGridCrc + blockIdx.x] = v;
  }
}

template <int R, bool kEncode>
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(R < 4 ? 2 : 1, R < 4 ? 2 : 1)))
void ec_fused_kernel(EcFusedLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(R >= 1 && R <= kEcFusedMaxRows, "parity accumulators in VGPRs");
  __shared__ MfmaTileLds lt;
  __shared__ StripeParts part;
  __shared__ uint32_t gft[R * kMaxShards * 8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = a.k, first_out = kEncode ? k : 0, nsh = first_out + R;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  const int64_t hi = static_cast<int64_t>(a.s_full);
  auto first_slice = [&](uint64_t t) {
    return static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(a.vfront);
  };
  WaveData cur;
  if (t_begin < t_end) cur = load_wave(a.in[0], first_slice(t_begin), 0, hi, lane);  // PCIe latency first
  ChunkBasis<true> basis;
  basis.load(gt, lane);
  load_lds_image(gt, &lt);
  for (int i = threadIdx.x; i < R * k * 8; i += kCrcWgThreads) gft[i] = a.tables[i];
  if (threadIdx.x < 4 * kMaxShards) (&part[0][0])[threadIdx.x] = 0;
  __syncthreads();

  for (uint64_t t = t_begin; t < t_end; ++t) {
    const int64_t i0 = first_slice(t);
    WaveData pacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) pacc[r].v[v] = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < k; ++c) {
      const bool more = c + 1 < k || t + 1 < t_end;
      WaveData nxt;
      if (more) nxt = load_wave(a.in[c + 1 < k ? c + 1 : 0], c + 1 < k ? i0 : first_slice(t + 1), 0, hi, lane);
      if constexpr (kEncode) {
        store_wave_dst(a.dst[c], i0, 0, hi, cur, lane);
        checksum(a, lt, part, basis, c, i0, cur, lane);
      }
      gf_accumulate<R>(gft, k, c, cur, pacc);
      if (more) cur = nxt;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      store_wave_dst(a.out[r], i0, 0, hi, pacc[r], lane);
      checksum(a, lt, part, basis, first_out + r, i0, pacc[r], lane);
    }
  }

  if (a.tail_len && blockIdx.x == 0 && wave == 0) {
    const uint64_t off = a.s_full * 512;
    WaveData pacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) pacc[r].v[v] = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < k; ++c) {
      const WaveData d = load_tail_wave(a.in[c] + off, a.tail_len, lane);
      if constexpr (kEncode) checksum_tail(a, lt, basis, c, a.dst[c], d, lane);
      gf_accumulate<R>(gft, k, c, d, pacc);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) checksum_tail(a, lt, basis, first_out + r, a.out[r], pacc[r], lane);
  }
  place_partials(a, lt, part, nsh, t_begin, t_end, lane);
}

// ---------------------------------------------------------------------------------------
// K4 + K2 for the tiering conversion: one resident, verified block -> the k + R shards of
// RS(k, R), in ec_fused_kernel's encode form (same tile axis and runs, same stores, checksums,
// accumulators and partials; the helpers are shared). What differs is where a data shard's bytes
// come from: column c of the block starts at byte c * sl, an arbitrary byte shift against the
// 16 B vectors, and the block ends at n, inside or before the last columns.
//  * Shifted load. The shift (c * sl) & 15 is uniform per column, a scalar. A lane's 32 B of a
//    pass are covered by three aligned 16 B vectors of the block (two at shift 0), loaded
//    non-temporal; v_alignbyte_b32 funnels dwords w .. w + 8 of them (w = shift / 4, a uniform
//    switch) by shift % 4 bytes into the same 32 B that load_wave gives for an aligned shard. The
//    third vector is the first of the lane's upper neighbour: a line the wave pulls anyway.
//  * End of the block. A vector at or behind n is not loaded and reads as zeros (nothing at or
//    beyond align_up(n, 16) is ever touched); the one vector that straddles n is masked
//    byte-wise after the wait, only in waves whose 4 KiB reach n (a uniform test). A column at
//    or behind n is all zeros and still stored, checksummed and multiplied: the zero padding is
//    part of the shards and of their CRCs.
//  * Pipeline. The next column's (or tile's) raw vectors are in flight behind the current
//    column's funnel, stores, checksum and GF arithmetic: 24 VGPRs per buffer instead of the fused
//    kernel's 16. R = 3 does not have them at 2 waves/SIMD: it spills 88 B per lane to scratch,
//    and still 24 B with the prefetch dropped (loads at the top of the column step). So R = 3 runs
//    like R = 4, at 1 wave/SIMD with the overflow in AGPRs and the prefetch kept, and both take
//    half the grid (ec_convert_grid): one workgroup per CU.
//  * Tail slice: byte loads as load_tail_wave does them, limited to the column's bytes below n.
// The compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs + AGPRs / LDS bytes
// / waves per SIMD; scratch is 0 in all four):
//   R  convert
//   1  255       / 50688 / 2
//   2  256       / 51712 / 2
//   3  256 + 68  / 52736 / 1
//   4  256 + 110 / 53760 / 1
struct ShiftedWave {
  uint4 v[6];  // per MFMA pass the aligned vectors 0, 16 and 32 B from the lane's bytes, rounded down
};

struct ConvertCol {
  const uint8_t* base;  // the aligned vector that holds the column's first byte
  int64_t left;         // block bytes from base on (<= 0: the column starts behind the block)
  uint32_t shift;       // of the column's first byte inside that vector
};

__device__ __forceinline__ ConvertCol convert_col(const EcConvertLaunch& a, int c) {
  const uint64_t b = static_cast<uint64_t>(c) * a.sl, b16 = b & ~15ull;
  return {a.src + b16, static_cast<int64_t>(a.n) - static_cast<int64_t>(b16),
          static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(b & 15)))};
}

__device__ __forceinline__ ShiftedWave load_wave_shifted(const ConvertCol& col, int64_t i0, int64_t hi, int lane) {
  const int n = lane & 31, h = lane >> 5;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  ShiftedWave d;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = it * 32 + n;
    const int64_t i = i0 + (c >> 3), off = i * 512 + (c & 7) * 64 + h * 32;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      d.v[3 * it + j] = make_uint4(0, 0, 0, 0);
      if (i >= 0 && i < hi && off + 16 * j < col.left && (j < 2 || col.shift)) {
        const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col.base + off) + j);
        d.v[3 * it + j] = make_uint4(x[0], x[1], x[2], x[3]);
      }
    }
  }
  return d;
}

// keep the low `keep` bytes (any int; <= 0 none, >= 16 all) of a vector
__device__ __forceinline__ uint4 keep_bytes(const uint4& v, int64_t keep) {
  const int r = static_cast<int>(keep < 0 ? 0 : keep > 16 ? 16 : keep);
  auto m = [&](int q) {
    const int b = r - 4 * q;
    return b >= 4 ? ~0u : b <= 0 ? 0u : (1u << (8 * b)) - 1u;
  };
  return make_uint4(v.x & m(0), v.y & m(1), v.z & m(2), v.w & m(3));
}

template <int W>
__device__ __forceinline__ void funnel_at(const uint32_t (&e)[12], uint32_t b, uint4& lo, uint4& hi) {
  lo = make_uint4(__builtin_amdgcn_alignbyte(e[W + 1], e[W], b), __builtin_amdgcn_alignbyte(e[W + 2], e[W + 1], b),
                  __builtin_amdgcn_alignbyte(e[W + 3], e[W + 2], b), __builtin_amdgcn_alignbyte(e[W + 4], e[W + 3], b));
  hi = make_uint4(__builtin_amdgcn_alignbyte(e[W + 5], e[W + 4], b), __builtin_amdgcn_alignbyte(e[W + 6], e[W + 5], b),
                  __builtin_amdgcn_alignbyte(e[W + 7], e[W + 6], b), __builtin_amdgcn_alignbyte(e[W + 8], e[W + 7], b));
}

// The loaded vectors -> the wave's 4 KiB of the column in load_wave's layout: zeros behind the
// block's end, then bytes [shift, shift + 32) of each pass's three vectors.
__device__ __forceinline__ WaveData shape_wave(const ConvertCol& col, int64_t i0, ShiftedWave r, int lane) {
  const int n = lane & 31, h = lane >> 5;
  if (col.left < (i0 + 8) * 512 + 16) {  // uniform: this wave's vectors reach the end of the block
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c = it * 32 + n;
      const int64_t off = (i0 + (c >> 3)) * 512 + (c & 7) * 64 + h * 32;
#pragma unroll
      for (int j = 0; j < 3; ++j) r.v[3 * it + j] = keep_bytes(r.v[3 * it + j], col.left - off - 16 * j);
    }
  }
  WaveData d;
  const uint32_t b = col.shift & 3u;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const uint4 &x = r.v[3 * it], &y = r.v[3 * it + 1], &z = r.v[3 * it + 2];
    const uint32_t e[12] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, z.x, z.y, z.z, z.w};
    switch (col.shift >> 2) {  // uniform
      case 0: funnel_at<0>(e, b, d.v[2 * it], d.v[2 * it + 1]); break;  // shift 0: the first two vectors as they are
      case 1: funnel_at<1>(e, b, d.v[2 * it], d.v[2 * it + 1]); break;
      case 2: funnel_at<2>(e, b, d.v[2 * it], d.v[2 * it + 1]); break;
      default: funnel_at<3>(e, b, d.v[2 * it], d.v[2 * it + 1]); break;
    }
  }
  return d;
}

template <int R>
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(R < 3 ? 2 : 1, R < 3 ? 2 : 1)))
void ec_convert_kernel(EcConvertLaunch cv, const DevCrcTables* __restrict__ gt) {
  static_assert(R >= 1 && R <= kEcFusedMaxRows, "parity accumulators in VGPRs");
  __shared__ MfmaTileLds lt;
  __shared__ StripeParts part;
  __shared__ uint32_t gft[R * kMaxShards * 8];
  const EcFusedLaunch& a = cv.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = a.k, nsh = k + R;
  const uint64_t t_begin = tile_run_begin(a.ntiles, blockIdx.x), t_end = tile_run_begin(a.ntiles, blockIdx.x + 1);
  const int64_t hi = static_cast<int64_t>(a.s_full);
  auto first_slice = [&](uint64_t t) {
    return static_cast<int64_t>(t * kSlicesPerTile + wave * 8) - static_cast<int64_t>(a.vfront);
  };
  ShiftedWave cur;
  if (t_begin < t_end) cur = load_wave_shifted(convert_col(cv, 0), first_slice(t_begin), hi, lane);
  ChunkBasis<true> basis;
  basis.load(gt, lane);
  load_lds_image(gt, &lt);
  for (int i = threadIdx.x; i < R * k * 8; i += kCrcWgThreads) gft[i] = a.tables[i];
  if (threadIdx.x < 4 * kMaxShards) (&part[0][0])[threadIdx.x] = 0;
  __syncthreads();

  for (uint64_t t = t_begin; t < t_end; ++t) {
    const int64_t i0 = first_slice(t);
    WaveData pacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) pacc[r].v[v] = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < k; ++c) {
      const ConvertCol col = convert_col(cv, c);
      const bool more = c + 1 < k || t + 1 < t_end;
      ShiftedWave nxt;
      if (more)
        nxt = load_wave_shifted(convert_col(cv, c + 1 < k ? c + 1 : 0), c + 1 < k ? i0 : first_slice(t + 1), hi, lane);
      const WaveData d = shape_wave(col, i0, cur, lane);
      store_wave_dst(a.dst[c], i0, 0, hi, d, lane);
      checksum(a, lt, part, basis, c, i0, d, lane);
      gf_accumulate<R>(gft, k, c, d, pacc);
      if (more) cur = nxt;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      store_wave_dst(a.out[r], i0, 0, hi, pacc[r], lane);
      checksum(a, lt, part, basis, k + r, i0, pacc[r], lane);
    }
  }

  if (a.tail_len && blockIdx.x == 0 && wave == 0) {
    const int64_t off = static_cast<int64_t>(a.s_full * 512);
    WaveData pacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v) pacc[r].v[v] = make_uint4(0, 0, 0, 0);
    for (int c = 0; c < k; ++c) {
      // byte loads at the column's own offset: what is left of the block behind the tail's start
      const int64_t at = static_cast<int64_t>(c * cv.sl) + off, left = static_cast<int64_t>(cv.n) - at;
      const WaveData d = load_tail_wave(cv.src + at, a.tail_len, lane,
                                        static_cast<int>(left < 0 ? 0 : left > 512 ? 512 : left));
      checksum_tail(a, lt, basis, c, a.dst[c], d, lane);
      gf_accumulate<R>(gft, k, c, d, pacc);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) checksum_tail(a, lt, basis, k + r, a.out[r], pacc[r], lane);
  }
  place_partials(a, lt, part, nsh, t_begin, t_end, lane);
}

// ---------------------------------------------------------------------------------------
// K5 for a degraded range read: bytes [from, from + want) of an RS-coded file go from the
// surviving shards in HBM straight into the reader's registered buffer. The kernel walks the
// SOURCE axis: every shard shares the shard-relative position p, data column c wants the
// positions [lo_c, hi_c) that the range cuts out of it, and a wave step is the 64 aligned 16 B
// vectors (1 KiB) at p = 1024 * step. Which columns want a step is wave-uniform (scalar
// compares); the steps that some column wants form at most two runs (launch_ec_read), and each
// wave takes a balanced contiguous piece of them, as tile_run_begin splits tiles.
//  * Loads. At a step survivor j is loaded once if it is a data column that wants the step, or
//    if any lost column wants it; the next survivor's load is issued before the current one's
//    arithmetic. A copied column and the rebuild share the registers of that one load.
//  * Arithmetic. The vector is multiplied into the R accumulators with the split-nibble
//    v_perm_b32 form of K4/K5 (selectors once per input dword, reused for every row); the
//    tables come through the device view of the lane's pinned scratch into LDS once per
//    workgroup and are LDS broadcasts after that.
//  * Shift. Column c's byte at p lands at out + c * sl - from + p, so with p % 16 == 0 the
//    source and destination vectors differ by the byte shift (c * sl - from) % 16: uniform per
//    column, a scalar. Each lane builds ONE destination-aligned vector from its own source vector
//    and its lower neighbour's (v_mov_b32_dpp wave_shr:1, then v_alignbyte_b32 by the scalar
//    shift). Lane 0's neighbour is the previous step's lane 63: a copied column reloads that one
//    vector; a rebuilt column carries it in scalar registers from the wave's previous step, or,
//    at the start of a run, rebuilds that single vector (one broadcast load per survivor).
//  * Stores. A destination vector that lies inside the column's window of `out` is one aligned
//    16 B store, wave-contiguous; the at most two vectors per column that straddle the window's
//    edges are stored byte-wise under the window test, so nothing outside [out, out + want) is
//    written and the zero padding behind the file's end is never emitted.
// No checksums (the survivors were verified where they were gathered, the bytes go to the
// client), no HBM output, no matrix cores. The compiler's report
// (-Rpass-analysis=kernel-resource-usage, gfx950; scratch is 0 in all five):
//   R  VGPRs  SGPRs  LDS bytes  waves per SIMD
//   0   40     82          0  8
//   1   67     98       1024  7
//   2   98    106       2048  4
//   3  118    106       3072  4
//   4  137    106       4096  3
struct EcReadCol {
  uint64_t lo, hi;  // shard-relative positions inside the range (lo == hi: none)
  // wave steps that hold a source vector of the column's destination vectors: the vector behind
  // the last byte supplies the lower neighbour of the last, shifted, destination vector
  __host__ __device__ uint64_t first_step() const { return lo / 1024; }
  __host__ __device__ uint64_t last_step() const { return ((hi - 1) / 16 + 1) / 64; }
};

__host__ __device__ inline EcReadCol ec_read_col(uint64_t sl, uint64_t from, uint64_t want, uint64_t c) {
  const uint64_t b = c * sl, lo = from > b ? from : b, hi = from + want < b + sl ? from + want : b + sl;
  return lo < hi ? EcReadCol{lo - b, hi - b} : EcReadCol{0, 0};
}

template <int R>
__device__ __forceinline__ void gf_accumulate16(const uint32_t* __restrict__ t, int k, int j, const uint4& d,
                                                uint4 (&acc)[R]) {
  uint32_t tb[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int q = 0; q < 8; ++q) tb[r][q] = t[(r * k + j) * 8 + q];
  const NibbleSel n0 = nibble_sel(d.x), n1 = nibble_sel(d.y), n2 = nibble_sel(d.z), n3 = nibble_sel(d.w);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    acc[r].x ^= gf_mul4(tb[r], n0);
    acc[r].y ^= gf_mul4(tb[r], n1);
    acc[r].z ^= gf_mul4(tb[r], n2);
    acc[r].w ^= gf_mul4(tb[r], n3);
  }
}

// Lane L takes lane L - 1's x; lane 0, which has no lower neighbour, keeps `first`.
__device__ __forceinline__ uint32_t lane_below(uint32_t x, uint32_t first) {
  return static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(static_cast<int>(first), static_cast<int>(x), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// One column's share of a wave step: `cur` is the lane's source vector v of the column, `first`
// the vector v0 - 1 below lane 0's. Destination vector q = v + floor(delta / 16) takes its low
// `shift` bytes from the top of vector v - 1 and the rest from the bottom of vector v.
__device__ __forceinline__ void shift_store(uint8_t* __restrict__ out, int64_t delta, int64_t dlo, int64_t dhi, int64_t v,
                                            const uint4& cur, const uint4& first) {
  const uint32_t shift = static_cast<uint32_t>(delta) & 15u;
  uint4 val = cur;
  if (shift) {  // uniform
    const uint4 prev = make_uint4(lane_below(cur.x, first.x), lane_below(cur.y, first.y), lane_below(cur.z, first.z),
                                  lane_below(cur.w, first.w));
    // bytes [16 - shift, 32 - shift) of prev:cur; dword w, byte b of it
    const uint32_t w = (16u - shift) >> 2, b = (16u - shift) & 3u;
    uint32_t e0, e1, e2, e3, e4;
    switch (w) {
      case 0: e0 = prev.x; e1 = prev.y; e2 = prev.z; e3 = prev.w; e4 = cur.x; break;
      case 1: e0 = prev.y; e1 = prev.z; e2 = prev.w; e3 = cur.x; e4 = cur.y; break;
      case 2: e0 = prev.z; e1 = prev.w; e2 = cur.x; e3 = cur.y; e4 = cur.z; break;
      default: e0 = prev.w; e1 = cur.x; e2 = cur.y; e3 = cur.z; e4 = cur.w; break;
    }
    val = make_uint4(__builtin_amdgcn_alignbyte(e1, e0, b), __builtin_amdgcn_alignbyte(e2, e1, b),
                     __builtin_amdgcn_alignbyte(e3, e2, b), __builtin_amdgcn_alignbyte(e4, e3, b));
  }
  const int64_t pos = ((delta >> 4) + v) * 16;  // of the destination vector in `out`
  if (pos >= dlo && pos + 16 <= dhi) {
    *reinterpret_cast<uint4*>(out + pos) = val;
  } else if (pos + 16 > dlo && pos < dhi) {  // a window edge: at most two vectors per column
    const uint32_t word[4] = {val.x, val.y, val.z, val.w};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (pos + i >= dlo && pos + i < dhi) out[pos + i] = static_cast<uint8_t>(word[i >> 2] >> (8 * (i & 3)));
  }
}

template <int R>
__global__ __launch_bounds__(kCrcWgThreads) void ec_read_kernel(EcReadLaunch a) {
  static_assert(R >= 0 && R <= kEcFusedMaxRows, "accumulators in VGPRs");
  constexpr int RR = R ? R : 1;
  __shared__ uint32_t gft[RR * kMaxShards * 8];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), k = a.k;
  if constexpr (R > 0) {
    for (int i = threadIdx.x; i < R * k * 8; i += kCrcWgThreads) gft[i] = a.tables[i];
    __syncthreads();
  }
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const uint64_t sl = a.sl, from = a.from, want = a.want, nvec = (sl + 15) / 16;
  const int c0 = static_cast<int>(from / sl), c1 = static_cast<int>((from + want - 1) / sl);
  const EcReadCol first = ec_read_col(sl, from, want, c0), last = ec_read_col(sl, from, want, c1);
  const uint64_t f0 = first.first_step(), l0 = first.last_step(), f1 = last.first_step(), l1 = last.last_step();
  // does data column c want wave step s (the columns between c0 and c1 want every step there is)
  auto wants = [&](int c, uint64_t s) {
    return c >= c0 && c <= c1 && (c != c0 || (s >= f0 && s <= l0)) && (c != c1 || (s >= f1 && s <= l1));
  };
  auto load = [&](int j, uint64_t v) {
    uint4 d = make_uint4(0, 0, 0, 0);
    if (v < nvec) {
      const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.in[j]) + v);
      d = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return d;
  };
  auto store = [&](int c, uint64_t v, const uint4& cur, const uint4& below) {
    const EcReadCol cr = ec_read_col(sl, from, want, c);
    const int64_t delta = static_cast<int64_t>(c * sl) - static_cast<int64_t>(from);
    shift_store(a.out, delta, delta + static_cast<int64_t>(cr.lo), delta + static_cast<int64_t>(cr.hi),
                static_cast<int64_t>(v), cur, below);
  };
  bool carried_shift = false;  // does a rebuilt column sit at a byte shift (its lane 0 needs the vector below)
#pragma unroll
  for (int r = 0; r < R; ++r) carried_shift = carried_shift || ((a.row_col[r] * sl - from) & 15) != 0;

  const uint64_t total = a.seg_steps[0] + a.seg_steps[1], nwaves = gridDim.x * 4ull, gw = blockIdx.x * 4ull + wave;
  const uint64_t i_begin = gw * total / nwaves, i_end = (gw + 1) * total / nwaves;
  uint4 carry[RR];  // lane 63's rebuilt vectors of step carry_step: wave-uniform
#pragma unroll
  for (int r = 0; r < RR; ++r) carry[r] = make_uint4(0, 0, 0, 0);
  uint64_t carry_step = ~0ull - 1;
  for (uint64_t i = i_begin; i < i_end; ++i) {
    const uint64_t s = i < a.seg_steps[0] ? a.seg_begin[0] + i : a.seg_begin[1] + (i - a.seg_steps[0]);
    uint32_t copy_mask = 0, row_mask = 0;
    for (int j = 0; j < k; ++j)
      if (wants(a.surv_col[j], s)) copy_mask |= 1u << j;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (wants(a.row_col[r], s)) row_mask |= 1u << r;
    uint32_t rest = row_mask ? (k >= 32 ? ~0u : (1u << k) - 1u) : copy_mask;
    if (!rest) continue;
    const uint64_t v0 = s * 64, v = v0 + lane;

    uint4 acc[RR];
    if constexpr (R > 0) {
      if (row_mask && carried_shift && v0 > 0 && carry_step + 1 != s) {
        // start of a run: rebuild the one vector below lane 0 (every lane loads the same 16 B)
#pragma unroll
        for (int r = 0; r < R; ++r) carry[r] = make_uint4(0, 0, 0, 0);
        for (int j = 0; j < k; ++j) gf_accumulate16<R>(gft, k, j, load(j, v0 - 1), carry);
#pragma unroll
        for (int r = 0; r < R; ++r)
          carry[r] = make_uint4(__builtin_amdgcn_readfirstlane(carry[r].x), __builtin_amdgcn_readfirstlane(carry[r].y),
                                __builtin_amdgcn_readfirstlane(carry[r].z), __builtin_amdgcn_readfirstlane(carry[r].w));
      }
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = make_uint4(0, 0, 0, 0);
    }

    int j = __builtin_ctz(rest);
    rest &= rest - 1;
    // the vector below lane 0's, for a copied column at a byte shift: one extra load in one lane
    auto load_below = [&](int jj) {
      return lane == 0 && v0 > 0 && ((copy_mask >> jj) & 1u) ? load(jj, v0 - 1) : make_uint4(0, 0, 0, 0);
    };
    uint4 cur = load(j, v), below = load_below(j);
    for (;;) {
      const int jn = rest ? __builtin_ctz(rest) : -1;
      uint4 nxt, nxt_below;
      if (jn >= 0) {
        nxt = load(jn, v);
        nxt_below = load_below(jn);
      }
      if ((copy_mask >> j) & 1u) store(a.surv_col[j], v, cur, below);
      if constexpr (R > 0)
        if (row_mask) gf_accumulate16<R>(gft, k, j, cur, acc);
      if (jn < 0) break;
      rest &= rest - 1;
      j = jn;
      cur = nxt;
      below = nxt_below;
    }
    if constexpr (R > 0) {
      if (row_mask) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((row_mask >> r) & 1u) store(a.row_col[r], v, acc[r], carry[r]);
          carry[r] = make_uint4(__builtin_amdgcn_readlane(acc[r].x, 63), __builtin_amdgcn_readlane(acc[r].y, 63),
                                __builtin_amdgcn_readlane(acc[r].z, 63), __builtin_amdgcn_readlane(acc[r].w, 63));
        }
        carry_step = s;
      }
    }
  }
}

// ---- K7: AES-256-GCM of a body in registered host memory (SSE-S3) ----
//
// Work split. The tile axis is the message's 16 B block axis, right-aligned (gcm_host.h): tile T,
// thread t owns blocks T * 1024 + 4t - vfront .. + 3, and a block below 0 does not exist. Workgroups
// stride over tiles; the next tile's vectors are loaded before the current one is encrypted.
//
// Alignment. The message starts Q dwords into a 16 B vector (Q = (src & 15) / 4, a template
// argument, so every funnel below indexes registers statically). All global traffic is on the
// aligned vector grid: a thread loads its four vectors, takes the Q dwords that its last block
// still lacks from the thread above (lane 63 loads that one vector itself), and after the XOR
// hands its last Q dwords up the same way, so that vectors leave whole. Only a wave's first vector
// (its low Q dwords belong to the wave below, which stores them) and the vectors holding the
// message's first and last bytes leave as dwords or bytes: nothing outside [dst, dst + n) is
// written. In place is safe because no thread uses bytes that another one writes: lane 63's load of
// the vector above does overlap dwords Q..3 of it, which the next wave's lane 0 stores, but it uses
// only dwords 0..Q-1, which it alone writes, and lane 0 in turn ignores those.
//
// AES. Te0 (1 KiB) and the S-box (256 B) sit in LDS; the other three tables are rotates. Four
// blocks go through each round together. The round keys are kernel arguments: scalar loads.
//
// GHASH. A thread keeps one accumulator for all its tiles: (acc ^ C) * H per block, and
// * H^(1024 * grid - 4) between its tiles, so every block costs one multiply. After the last tile
// the accumulators combine in a log tree with H^(4 * 2^s) (shuffles inside a wave, LDS across the
// four waves) into the workgroup's partial. Multiplies are shift-and-XOR in VGPRs with the
// wave-uniform power of H as the operand whose bits are tested.
__device__ __forceinline__ gcm::U128 shuffle_down(const gcm::U128& v, int by) {
  const uint32_t a = __shfl_down(static_cast<uint32_t>(v.hi >> 32), by), b = __shfl_down(static_cast<uint32_t>(v.hi), by),
                 c = __shfl_down(static_cast<uint32_t>(v.lo >> 32), by), d = __shfl_down(static_cast<uint32_t>(v.lo), by);
  return gcm::U128{static_cast<uint64_t>(a) << 32 | b, static_cast<uint64_t>(c) << 32 | d};
}

// Dwords [lo, hi) of the 16 B vector whose first byte is message byte `pos` (pos % 4 == 0, may
// be negative), clipped to the message [0, n).
__device__ __forceinline__ void sse_store(uint8_t* dst, int64_t pos, int64_t n, const uint32_t (&w)[4], int lo,
                                          int hi) {
  if (lo == 0 && hi == 4 && pos >= 0 && pos + 16 <= n) {
    *reinterpret_cast<uint4*>(dst + pos) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t p = pos + 4 * k;
    if (k < lo || k >= hi || p < 0 || p >= n) continue;
    if (p + 4 <= n) {
      *reinterpret_cast<uint32_t*>(dst + p) = w[k];
    } else {
      for (int i = 0; p + i < n; ++i) dst[p + i] = static_cast<uint8_t>(w[k] >> (8 * i));
    }
  }
}

// sse_gcm_kernel's AES and GHASH steps as functions, for sse_read_kernel.
// Te0 and the S-box from the uploaded image into LDS (256 threads, one entry each; sync after).
__device__ __forceinline__ void sse_load_tables(const DevCrcTables* __restrict__ gt, uint32_t (&te0)[256],
                                                uint8_t (&sbox)[256]) {
  const uint8_t* img = reinterpret_cast<const uint8_t*>(gt) + sizeof(DevCrcTables) + kSseTablesOffset;
  te0[threadIdx.x] = reinterpret_cast<const uint32_t*>(img)[threadIdx.x];
  sbox[threadIdx.x] = img[1024 + threadIdx.x];
}

// CTR keystream of message blocks j0 .. j0 + 3: E_K(nonce || 2 + j).
template <class RK>
__device__ __forceinline__ void sse_keystream(const uint32_t (&te0)[256], const uint8_t (&sbox)[256], const RK& rk,
                                              uint32_t n0, uint32_t n1, uint32_t n2, int64_t j0, uint32_t (&ks)[4][4]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    ks[b][0] = n0;
    ks[b][1] = n1;
    ks[b][2] = n2;
    ks[b][3] = gcm::bswap32(2u + static_cast<uint32_t>(j0 + b));
  }
  gcm::aes256_encrypt_words<4>(te0, sbox, rk, ks);
}

// Mask of the bytes of a dword that has `left` message bytes at and behind its first one.
__device__ __forceinline__ uint32_t sse_keep(int64_t left) {
  return left >= 4 ? ~0u : left <= 0 ? 0u : (1u << (8 * left)) - 1u;
}

// One GHASH step: (acc ^ C) * H for the ciphertext block c (little-endian dwords).
__device__ __forceinline__ gcm::U128 ghash_absorb(const gcm::U128& acc, const gcm::U128& h, const uint32_t (&c)[4]) {
  const gcm::U128 e = gcm::ghash_element(c[0], c[1], c[2], c[3]);
  return gcm::gf128_mul(h, gcm::U128{acc.hi ^ e.hi, acc.lo ^ e.lo});
}

// The lanes' accumulators, each standing at the end of its four blocks in the workgroup's last
// tile, into the workgroup's partial: a log tree inside each wave, then the four waves in order.
__device__ __forceinline__ void ghash_wg_partial(gcm::U128 acc, const gcm::U128 (&tree)[gcm::kGcmTreeSteps],
                                                 gcm::U128 (&wave_part)[4], gcm::U128* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int s = 0; s < 6; ++s) {
    const gcm::U128 right = shuffle_down(acc, 1 << s), left = gcm::gf128_mul(tree[s], acc);
    acc = gcm::U128{left.hi ^ right.hi, left.lo ^ right.lo};
  }
  if (lane == 0) wave_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    gcm::U128 y = wave_part[0];
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
      y = gcm::gf128_mul(tree[6], y);
      y = gcm::U128{y.hi ^ wave_part[w].hi, y.lo ^ wave_part[w].lo};
    }
    part[blockIdx.x] = y;
  }
}

// sse_gcm_kernel keeps these steps written out in its body: calling the functions above cost it
// 30 VGPRs (140 -> 170 in the compiler's table) and with them its third wave per SIMD.
template <int Q>
__global__ __launch_bounds__(kCrcWgThreads) void sse_gcm_kernel(SseGcmLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(Q >= 0 && Q < 4 && kCrcWgThreads == 256 && gcm::kGcmTileBlocks == 4 * kCrcWgThreads, "tile shape");
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part[4];
  {
    const uint8_t* img = reinterpret_cast<const uint8_t*>(gt) + sizeof(DevCrcTables) + kSseTablesOffset;
    te0[threadIdx.x] = reinterpret_cast<const uint32_t*>(img)[threadIdx.x];
    sbox[threadIdx.x] = img[1024 + threadIdx.x];
  }
  __syncthreads();
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = static_cast<int64_t>(a.n), nvec = (n + 4 * Q + 15) / 16;
  // vector v of the aligned grid holds message bytes [16v - 4Q, 16v - 4Q + 16)
  const u32x4* src = reinterpret_cast<const u32x4*>(a.src - 4 * Q);  // may alias dst: no __restrict__
  uint8_t* dst = a.dst;
  auto first_block = [&](uint64_t tile) {
    return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x) - static_cast<int64_t>(a.vfront);
  };
  auto load = [&](int64_t v) {
    uint4 d = make_uint4(0, 0, 0, 0);
    if (v >= 0 && v < nvec) {
      const u32x4 x = __builtin_nontemporal_load(src + v);
      d = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return d;
  };
  // a thread's four vectors and, in lane 63, the one above them
  auto fetch = [&](uint64_t tile, uint4 (&v)[4], uint4& above) {
    const int64_t j0 = first_block(tile);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = load(j0 + i);
    above = Q > 0 && lane == 63 ? load(j0 + 4) : make_uint4(0, 0, 0, 0);
  };

  gcm::U128 acc{0, 0};
  uint4 cur[4], cur_above;
  fetch(blockIdx.x, cur, cur_above);
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    uint4 nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    uint4 nxt_above = make_uint4(0, 0, 0, 0);
    if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x, nxt, nxt_above);
    const int64_t j0 = first_block(tile);

    // the message dwords of the thread's four blocks: own dwords from Q on, then Q from above
    const uint32_t d[16] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                            cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};
    const uint32_t ab[4] = {cur_above.x, cur_above.y, cur_above.z, cur_above.w};
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + Q < 16) {
        m[i] = d[i + Q];
      } else {
        const uint32_t up = __shfl_down(d[i + Q - 16], 1);
        m[i] = lane == 63 ? ab[i + Q - 16] : up;
      }
    }

    uint32_t ks[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      ks[b][0] = a.nonce[0];
      ks[b][1] = a.nonce[1];
      ks[b][2] = a.nonce[2];
      ks[b][3] = gcm::bswap32(2u + static_cast<uint32_t>(j0 + b));
    }
    gcm::aes256_encrypt_words<4>(te0, sbox, a.rk, ks);

    uint32_t o[16];
    if (tile != blockIdx.x) acc = gcm::gf128_mul(a.hjump, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      uint32_t c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[4 * b + k] = m[4 * b + k] ^ ks[b][k];
        // the ciphertext, zero where the block lies outside the message (its short end included)
        const int64_t left = j0 + b < 0 ? 0 : n - 16 * (j0 + b) - 4 * k;
        const uint32_t keep = left >= 4 ? ~0u : left <= 0 ? 0u : (1u << (8 * left)) - 1u;
        c[k] = (a.encrypt ? o[4 * b + k] : m[4 * b + k]) & keep;
      }
      const gcm::U128 e = gcm::ghash_element(c[0], c[1], c[2], c[3]);
      acc = gcm::gf128_mul(a.h, gcm::U128{acc.hi ^ e.hi, acc.lo ^ e.lo});
    }

    // back onto the vector grid: vector j0 + i takes dwords [4i - Q, 4i - Q + 4) of the output,
    // the first Q of them from the thread below
    uint32_t below[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < Q; ++i) below[i] = __shfl_up(o[16 - Q + i], 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = 4 * i + k < Q ? below[(4 * i + k) & 3] : o[(4 * i + k - Q) & 15];
      sse_store(dst, 16 * (j0 + i) - 4 * Q, n, w, i == 0 && lane == 0 ? Q : 0, 4);
    }
    if (Q > 0 && lane == 63) {  // the low Q dwords of the vector above the wave's span
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < Q; ++k) w[k] = o[16 - Q + k];
      sse_store(dst, 16 * (j0 + 4) - 4 * Q, n, w, 0, Q);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
    cur_above = nxt_above;
  }

  // a thread's accumulator stands at the end of its four blocks in the workgroup's last tile
#pragma unroll 1
  for (int s = 0; s < 6; ++s) {
    const gcm::U128 right = shuffle_down(acc, 1 << s), left = gcm::gf128_mul(a.tree[s], acc);
    acc = gcm::U128{left.hi ^ right.hi, left.lo ^ right.lo};
  }
  if (lane == 0) wave_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    gcm::U128 y = wave_part[0];
#pragma unroll 1
    for (int w = 1; w < 4; ++w) {
      y = gcm::gf128_mul(a.tree[6], y);
      y = gcm::U128{y.hi ^ wave_part[w].hi, y.lo ^ wave_part[w].lo};
    }
    a.part[blockIdx.x] = y;
  }
}

// ---- K7 read: verify, authenticate, decrypt and deliver a stored SSE-S3 blob in one pass ----
//
// The block in HBM is [nonce 12][ciphertext n][tag 16]. One launch checks every 512 B slice of it
// against the .meta image (as crc_read_copy_kernel does), decrypts the ciphertext with K7's CTR
// keystream, accumulates K7's GHASH of it, and stores the plaintext, and nothing else, into the
// reader's registered buffer: the ciphertext crosses no link at all.
//
// The two axes. CRC slices, chunks and tiles count from block byte 0; AES blocks from byte 12. The
// kernel lives on the CRC axis: tile T is block bytes [16 KiB * T, 16 KiB * (T + 1)), thread t of
// its workgroup owns the 64 B chunk at vectors g = 1024 T + 4t .. g + 3, and workgroups stride
// over tiles as in K7. AES block i is dword 3 of vector i and dwords 0..2 of vector i + 1, so the
// thread that owns vector i owns block i: counter, GHASH position and output offset 16i all follow
// from the vector index, and the 12 bytes between the axes are one fixed 3-dword funnel on the load
// side (a lane takes three dwords from the lane above; lane 63 loads the vector above its wave,
// which at wave 3 is the first vector of the next tile). The plaintext block then lies on the
// aligned grid of `out` and leaves as one 16 B store.
//   On the GHASH side this is gcm::plan_for of the tiles' whole span, 16 KiB * ntiles: no virtual
// blocks in front, and `vback` zero blocks behind the message (the tag, the bytes behind the block
// and the rest of the last tile are masked to zero). Zero blocks at the end do count: the fold
// comes out as the message's sum times H^vback, which gcm::tag_matches takes into account on the
// host, where multiplying the other side of the comparison costs less than a right-aligned axis
// would here (every lane's chunk off the CRC's 64 B grid).
//
// CRC. A lane holds chunk `lane` of its wave's 4 KiB whole, the MFMA wants lane (n, h) to hold half
// h of chunk n and of chunk 32 + n: exchanging dwords k and 8 + k between the half-waves (eight
// v_permlane32_swap) makes exactly that WaveData, and wave_chunk_crcs returns chunk `lane`'s CRC to
// the lane that decrypts it. The short tail slice is checked by workgroup 0 from byte loads.
//
// Registers: 64 for the CRC basis, 40 for two tiles' vectors, 16 + 16 for states and message, the
// MFMA accumulators and the GHASH operands do not fit three waves per SIMD; two do, without scratch.
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sse_read_kernel(
    SseReadLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(kCrcWgThreads == 256 && gcm::kGcmTileBlocks * 16 == kSlicesPerTile * 512, "a CRC tile is a GCM tile");
  __shared__ MfmaSliceLds lt;
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part[4];
  __shared__ uint32_t wg_bad;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const int64_t n = static_cast<int64_t>(a.n), size = n + 28, nvec = (size + 15) / 16, s_full = size / 512;
  const u32x4* src = reinterpret_cast<const u32x4*>(a.src);
  auto load = [&](int64_t v) {
    uint4 d = make_uint4(0, 0, 0, 0);
    if (v < nvec) {  // the vector behind the block's end is never loaded
      const u32x4 x = __builtin_nontemporal_load(src + v);
      d = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return d;
  };
  auto first_vector = [&](uint64_t tile) { return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x); };
  auto fetch = [&](uint64_t tile, uint4 (&v)[4], uint4& above) {
    const int64_t g = first_vector(tile);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = load(g + i);
    above = lane == 63 ? load(g + 4) : make_uint4(0, 0, 0, 0);
  };

  uint4 cur[4], cur_above;
  fetch(blockIdx.x, cur, cur_above);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  sse_load_tables(gt, te0, sbox);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  // the nonce: the block's first three dwords, the same for every lane
  const uint32_t* head = reinterpret_cast<const uint32_t*>(a.src);
  const uint32_t n0 = head[0], n1 = head[1], n2 = head[2];
  if (blockIdx.x == 0 && threadIdx.x < 28)  // nonce and stored tag for the host: block bytes [0, 12) and [12 + n, 28 + n)
    a.nonce_tag[threadIdx.x] = a.src[threadIdx.x < 12 ? threadIdx.x : n + threadIdx.x];
  __syncthreads();

  gcm::U128 acc{0, 0};
  uint32_t bad = 0xFFFFFFFFu;
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    uint4 nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    uint4 nxt_above = make_uint4(0, 0, 0, 0);
    if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x, nxt, nxt_above);
    const int64_t g = first_vector(tile);
    const uint32_t d[16] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                            cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};

    // verify: the lane's chunk, halves exchanged across the half-waves into the MFMA's operand
    {
      uint32_t p0[8], p1[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const auto r = __builtin_amdgcn_permlane32_swap(d[k], d[8 + k], false, false);
        p0[k] = r[0];  // lanes 0..31: own dword k; lanes 32..63: dword 8 + k of lane - 32
        p1[k] = r[1];  // lanes 0..31: dword k of lane + 32; lanes 32..63: own dword 8 + k
      }
      WaveData w;
      w.v[0] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
      w.v[1] = make_uint4(p0[4], p0[5], p0[6], p0[7]);
      w.v[2] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
      w.v[3] = make_uint4(p1[4], p1[5], p1[6], p1[7]);
      const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, w, lane), lane);
      const int64_t i = static_cast<int64_t>(tile) * kSlicesPerTile + wave * 8 + sw;
      if (i < s_full && sl == 0 && a.meta[i] != __builtin_bswap32(r ^ a.full_init)) bad = min(bad, static_cast<uint32_t>(i));
    }

    // the ciphertext of blocks g .. g + 3: the lane's dwords from 3 on, then three from above
    const uint32_t ab[3] = {cur_above.x, cur_above.y, cur_above.z};
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + 3 < 16) {
        m[i] = d[i + 3];
      } else {
        const uint32_t up = __shfl_down(d[i + 3 - 16], 1);
        m[i] = lane == 63 ? ab[i + 3 - 16] : up;
      }
    }

    uint32_t ks[4][4];
    sse_keystream(te0, sbox, a.rk, n0, n1, n2, g, ks);

    if (tile != blockIdx.x) acc = gcm::gf128_mul(a.hjump, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t pos = 16 * (g + b);  // of the block in the message and in `out`
      uint32_t c[4], o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = m[4 * b + k] & sse_keep(n - pos - 4 * k);
        o[k] = m[4 * b + k] ^ ks[b][k];
      }
      acc = ghash_absorb(acc, a.h, c);
      if (pos + 16 <= n) {
        *reinterpret_cast<uint4*>(a.out + pos) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        for (int64_t p = pos; p < n; ++p) a.out[p] = static_cast<uint8_t>(o[(p - pos) >> 2] >> (8 * ((p - pos) & 3)));
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
    cur_above = nxt_above;
  }

  if (size % 512 && blockIdx.x == 0 && wave == 0) {
    const uint32_t tail_len = static_cast<uint32_t>(size % 512);
    const uint32_t r =
        slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(a.src + s_full * 512, tail_len, lane), lane), lane);
    if (lane == 0 && a.meta[s_full] != __builtin_bswap32(r ^ a.tail_init)) bad = min(bad, static_cast<uint32_t>(s_full));
  }
  if (bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  ghash_wg_partial(acc, a.tree, wave_part, a.part);  // its barrier orders wg_bad too
  if (threadIdx.x == 0) a.part_bad[blockIdx.x] = wg_bad;
}

// ---- K7 range read: authenticate the whole stored blob, decrypt and deliver only a byte range ----
//
// sse_read_kernel's axes, loads, CRC and GHASH plan, tile for tile: GCM's tag covers the whole
// ciphertext and .meta every slice, so every tile of the blob is verified and absorbed, from HBM.
// CTR's keystream is random access (block i is E_K(nonce || i + 2)), so AES runs only where
// plaintext leaves, and only plaintext [from, from + want) crosses the link, to out[0, want).
//
// A tile holds message bytes [16 KiB * T, 16 KiB * (T + 1)). Against the range it is, for the whole
// workgroup alike,
//   outside: CRC and GHASH, then on to the next tile: no keystream, no store;
//   inside:  every lane's four blocks decrypted and stored whole, as in sse_read_kernel;
//   edge:    (the range's first or last byte lies in it) a lane whose 64 B miss the range skips the
//            keystream; of the others' blocks those wholly in range leave as 16 B stores, and the
//            blocks holding byte `from` and byte `from + want - 1` as byte stores clipped to it.
// With out % 16 == from % 16, block `pos` goes to out + (pos - from) on out's 16 B grid, so the load
// side's funnel is the fixed one. In-range tiles are contiguous and workgroups stride over tiles,
// so the keystream work spreads over min(tiles in range, grid) workgroups without a schedule.
//
// The GHASH of a tile is done before its keystream: the accumulate needs the ciphertext alone, and
// the four AES states are then live only with the message, not with the multiply's operands.
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sse_read_range_kernel(
    SseReadRangeLaunch ar, const DevCrcTables* __restrict__ gt) {
  __shared__ MfmaSliceLds lt;
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part[4];
  __shared__ uint32_t wg_bad;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const SseReadLaunch& a = ar.r;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const int64_t n = static_cast<int64_t>(a.n), size = n + 28, nvec = (size + 15) / 16, s_full = size / 512;
  const int64_t from = static_cast<int64_t>(ar.from), to = from + static_cast<int64_t>(ar.want);
  const u32x4* src = reinterpret_cast<const u32x4*>(a.src);
  auto load = [&](int64_t v) {
    uint4 d = make_uint4(0, 0, 0, 0);
    if (v < nvec) {  // the vector behind the block's end is never loaded
      const u32x4 x = __builtin_nontemporal_load(src + v);
      d = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return d;
  };
  auto first_vector = [&](uint64_t tile) { return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x); };
  auto fetch = [&](uint64_t tile, uint4 (&v)[4], uint4& above) {
    const int64_t g = first_vector(tile);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = load(g + i);
    above = lane == 63 ? load(g + 4) : make_uint4(0, 0, 0, 0);
  };

  uint4 cur[4], cur_above;
  fetch(blockIdx.x, cur, cur_above);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  sse_load_tables(gt, te0, sbox);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  const uint32_t* head = reinterpret_cast<const uint32_t*>(a.src);
  const uint32_t n0 = head[0], n1 = head[1], n2 = head[2];
  if (blockIdx.x == 0 && threadIdx.x < 28) a.nonce_tag[threadIdx.x] = a.src[threadIdx.x < 12 ? threadIdx.x : n + threadIdx.x];
  __syncthreads();

  gcm::U128 acc{0, 0};
  uint32_t bad = 0xFFFFFFFFu;
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    uint4 nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    uint4 nxt_above = make_uint4(0, 0, 0, 0);
    if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x, nxt, nxt_above);
    const int64_t g = first_vector(tile);
    const uint32_t d[16] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                            cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};

    // verify, as sse_read_kernel
    {
      uint32_t p0[8], p1[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const auto r = __builtin_amdgcn_permlane32_swap(d[k], d[8 + k], false, false);
        p0[k] = r[0];
        p1[k] = r[1];
      }
      WaveData w;
      w.v[0] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
      w.v[1] = make_uint4(p0[4], p0[5], p0[6], p0[7]);
      w.v[2] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
      w.v[3] = make_uint4(p1[4], p1[5], p1[6], p1[7]);
      const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, w, lane), lane);
      const int64_t i = static_cast<int64_t>(tile) * kSlicesPerTile + wave * 8 + sw;
      if (i < s_full && sl == 0 && a.meta[i] != __builtin_bswap32(r ^ a.full_init)) bad = min(bad, static_cast<uint32_t>(i));
    }

    // the ciphertext of blocks g .. g + 3: the lane's dwords from 3 on, then three from above
    const uint32_t ab[3] = {cur_above.x, cur_above.y, cur_above.z};
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i + 3 < 16) {
        m[i] = d[i + 3];
      } else {
        const uint32_t up = __shfl_down(d[i + 3 - 16], 1);
        m[i] = lane == 63 ? ab[i + 3 - 16] : up;
      }
    }

    // authenticate: every tile, whatever its class
    if (tile != blockIdx.x) acc = gcm::gf128_mul(a.hjump, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      uint32_t c[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) c[k] = m[4 * b + k] & sse_keep(n - 16 * (g + b) - 4 * k);
      acc = ghash_absorb(acc, a.h, c);
    }

    // decrypt and deliver: by the tile's class, the same for the whole workgroup
    const int64_t t_lo = static_cast<int64_t>(tile * kSseReadTileBytes), t_hi = t_lo + static_cast<int64_t>(kSseReadTileBytes);
    const bool outside = t_hi <= from || t_lo >= to, inside = t_lo >= from && t_hi <= to;
    if (!outside && (inside || (16 * g < to && 16 * (g + 4) > from))) {
      uint32_t ks[4][4];
      sse_keystream(te0, sbox, a.rk, n0, n1, n2, g, ks);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t pos = 16 * (g + b);  // of the block in the message; out holds byte `from` first
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = m[4 * b + k] ^ ks[b][k];
        uint8_t* dst = a.out + (pos - from);
        if (inside || (pos >= from && pos + 16 <= to)) {
          *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        } else if (pos < to && pos + 16 > from) {  // the block of the range's first or last byte
#pragma unroll
          for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int64_t p = pos + 4 * k + i;
              if (p >= from && p < to) dst[4 * k + i] = static_cast<uint8_t>(o[k] >> (8 * i));
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
    cur_above = nxt_above;
  }

  if (size % 512 && blockIdx.x == 0 && wave == 0) {
    const uint32_t tail_len = static_cast<uint32_t>(size % 512);
    const uint32_t r =
        slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(a.src + s_full * 512, tail_len, lane), lane), lane);
    if (lane == 0 && a.meta[s_full] != __builtin_bswap32(r ^ a.tail_init)) bad = min(bad, static_cast<uint32_t>(s_full));
  }
  if (bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  ghash_wg_partial(acc, a.tree, wave_part, a.part);  // its barrier orders wg_bad too
  if (threadIdx.x == 0) a.part_bad[blockIdx.x] = wg_bad;
}

// ---- K7 write: encrypt, authenticate, checksum and land an SSE-S3 PUT in one pass ----
//
// The mirror of sse_read_kernel, on the same axis: the slot holds [nonce 12][plaintext n][16 free],
// tile T is blob bytes [16 KiB * T, 16 KiB * (T + 1)), thread t owns the 64 B chunk at vectors
// g = 1024 T + 4t .. g + 3. Both the slot and the extent are 16 B aligned, so vector v is loaded
// from buf + 16v and its ciphertext stored to dst + 16v and back to buf + 16v, unshifted.
//
// Nothing crosses a lane. A chunk touches five AES blocks: dwords 1..3 of block g - 1 (the chunk's
// first three dwords), blocks g .. g + 2 whole, and dword 0 of block g + 3 (its last). The lane
// computes all five counters' keystream (the fifth block rides in the rounds of the other four) and
// so holds its whole ciphertext chunk: the CRC's operand, and what it stores. Because a lane reads
// and writes its own four vectors only, encrypting in place has no ordering to respect.
//   GHASH is linear in the block, so the two split blocks are absorbed as two elements each, one by
// either owner, zero where the other's dwords stand: five absorbs per chunk (tail of block g - 1,
// three whole blocks, head of block g + 3), and the step between a lane's tiles is
// H^(1024 * grid - 5). The lane again stands at the end of block g + 3, so the tree, the partials
// and gcm::ghash_fold are those of sse_read_kernel. The nonce (vector 0, dwords 0..2) is stored from
// the arguments and is no part of any element; every byte from 12 + n on counts as zero whatever the slot
// holds there, so the tag's room and the padding are stored as zeros and the host, which alone can
// close the tag, writes it afterwards.
//
// CRC. The ciphertext chunk goes through the permlane32 route of sse_read_kernel into the MFMA
// operand. Slices that lie wholly in front of the tag (s < (n + 12) / 512) get their .meta word
// here, in HBM and in the host image; the one or two behind them hold tag bytes and are the host's.
// The same slices feed the whole-block CRC: sub-tile CRCs, a Horner step of `grid` tiles between a
// workgroup's tiles, and the partial moved to the end of the tile axis as crc_write_copy_kernel
// does. The zeros behind the last such slice are part of that value; the host takes them out again
// (the shift by zero bytes is invertible: x has an inverse modulo the CRC polynomial).
//
// Registers as sse_read_kernel: two waves per SIMD, no scratch.
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sse_write_kernel(
    SseWriteLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(kCrcWgThreads == 256 && gcm::kGcmTileBlocks * 16 == kSlicesPerTile * 512, "a CRC tile is a GCM tile");
  __shared__ MfmaTileLds lt;
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part[4];
  __shared__ uint32_t wacc[4];
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const int64_t n = static_cast<int64_t>(a.n), size = n + 28, nvec = (size + 15) / 16;
  const int64_t s_body = static_cast<int64_t>(sse_write_body_slices(a.n));
  const u32x4* src = reinterpret_cast<const u32x4*>(a.buf);  // aliases the stores back: no __restrict__
  auto first_vector = [&](uint64_t tile) { return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x); };
  auto fetch = [&](uint64_t tile, uint4 (&v)[4]) {
    const int64_t g = first_vector(tile);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = make_uint4(0, 0, 0, 0);
      if (g + i < nvec) {  // the vector behind the slot's end is never loaded
        const u32x4 x = __builtin_nontemporal_load(src + g + i);
        v[i] = make_uint4(x[0], x[1], x[2], x[3]);
      }
    }
  };

  uint4 cur[4];
  fetch(blockIdx.x, cur);  // the link's latency first
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  sse_load_tables(gt, te0, sbox);
  __syncthreads();

  gcm::U128 acc{0, 0};
  uint32_t crc = 0;
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    uint4 nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x, nxt);
    const int64_t g = first_vector(tile);
    const uint32_t d[16] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                            cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};

    // the keystream of blocks g - 1 .. g + 3; chunk dword i takes dword (i + 1) % 4 of block g - 1 + (i + 1) / 4
    uint32_t ks[5][4];
#pragma unroll
    for (int b = 0; b < 5; ++b) {
      ks[b][0] = a.nonce[0];
      ks[b][1] = a.nonce[1];
      ks[b][2] = a.nonce[2];
      ks[b][3] = gcm::bswap32(1u + static_cast<uint32_t>(g + b));
    }
    gcm::aes256_encrypt_words<5>(te0, sbox, a.rk, ks);
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t p = 16 * g + 4 * i;  // the dword's first byte in the blob
      c[i] = p < 12 ? a.nonce[i & 3] : (d[i] ^ ks[(i + 1) >> 2][(i + 1) & 3]) & sse_keep(12 + n - p);
    }

    // land: the extent is padded to 16 B, the slot ends where the blob does
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t pos = 16 * (g + i);
      if (pos >= size) continue;
      const uint4 v = make_uint4(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
      *reinterpret_cast<uint4*>(a.dst + pos) = v;
      if (pos + 16 <= size) {
        *reinterpret_cast<uint4*>(a.buf + pos) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (pos + j < size) a.buf[pos + j] = static_cast<uint8_t>(c[4 * i + (j >> 2)] >> (8 * (j & 3)));
      }
    }

    // checksum: the chunk, halves exchanged across the half-waves into the MFMA's operand
    {
      uint32_t p0[8], p1[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const auto r = __builtin_amdgcn_permlane32_swap(c[k], c[8 + k], false, false);
        p0[k] = r[0];
        p1[k] = r[1];
      }
      WaveData w;
      w.v[0] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
      w.v[1] = make_uint4(p0[4], p0[5], p0[6], p0[7]);
      w.v[2] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
      w.v[3] = make_uint4(p1[4], p1[5], p1[6], p1[7]);
      uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, w, lane), lane);
      const int64_t i = static_cast<int64_t>(tile) * kSlicesPerTile + wave * 8 + sw;
      if (i >= s_body) {
        r = 0;  // the host's slices, and zeros to the whole-block CRC
      } else if (sl == 0) {
        const uint32_t be = __builtin_bswap32(r ^ a.full_init);
        a.meta[i] = be;
        a.meta_host[i] = be;
      }
      r = combine<8>(r, lane, lt.sh512);
      r = combine<16>(r, lane, lt.sh1k);
      r = combine<32>(r, lane, lt.sh2k);  // wave-uniform: the 4 KiB sub-tile's raw CRC
      if (tile != blockIdx.x) {
        uint32_t e = gridDim.x;
        for (int b = 0; e; ++b, e >>= 1)
          if (e & 1) crc = mat_apply(lt.tile_pow2[b], crc, lane);
      }
      crc ^= r;
    }

    // authenticate: the tail of block g - 1, blocks g .. g + 2, the head of block g + 3
    if (tile != blockIdx.x) acc = gcm::gf128_mul(a.hjump, acc);
    {
      const bool head = g == 0;  // the nonce stands where block -1's tail would
      const uint32_t e0[4] = {0, head ? 0 : c[0], head ? 0 : c[1], head ? 0 : c[2]};
      acc = ghash_absorb(acc, a.h, e0);
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const uint32_t e[4] = {c[4 * b + 3], c[4 * b + 4], c[4 * b + 5], c[4 * b + 6]};
        acc = ghash_absorb(acc, a.h, e);
      }
      const uint32_t e4[4] = {c[15], 0, 0, 0};
      acc = ghash_absorb(acc, a.h, e4);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
  }

  // the wave's CRC stands at the end of its sub-tile in the workgroup's last tile: to the axis's end
  {
    for (int k = wave; k < 3; ++k) crc = tab4(lt.sh4k, crc);
    const uint64_t last = blockIdx.x + (a.ntiles - 1 - blockIdx.x) / gridDim.x * gridDim.x;
    uint64_t e = a.ntiles - 1 - last;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) crc = mat_apply(lt.tile_pow2[b], crc, lane);
    if (lane == 0) wacc[wave] = crc;
  }
  ghash_wg_partial(acc, a.tree, wave_part, a.part);  // its barrier orders wacc too
  if (threadIdx.x == 0) a.part_crc[blockIdx.x] = wacc[0] ^ wacc[1] ^ wacc[2] ^ wacc[3];
}

// ---- K7 copy: verify, authenticate, re-key, authenticate, checksum and land a CopyObject in one pass ----
//
// Source and destination blobs are both [nonce 12][ciphertext n][tag 16] in HBM extents, 16 B aligned,
// so ciphertext byte i sits at blob byte 12 + i on either side and the new ciphertext is
// old ^ keystream(K_src, nonce_src) ^ keystream(K_dst, nonce_dst) at the same offset: vector v is
// loaded from src + 16v and stored to dst + 16v. The plaintext exists between two XORs, in registers.
//
// Which axis the AES runs on: sse_write_kernel's. A lane keeps its own 64 B chunk of the CRC axis
// (tile T is blob bytes [16 KiB * T, 16 KiB * (T + 1)), thread t owns vectors g = 1024 T + 4t .. g + 3)
// and computes, per key, the keystream of the five AES blocks g - 1 .. g + 3 that the chunk touches.
// sse_read_kernel's 3-dword funnel would save two of the ten blocks, but here the bytes must come
// back to the CRC axis for the second checksum and the aligned store, so it would take a funnel in
// (16 shuffles and lane 63's extra load) and a funnel out (3 more shuffles, and the wave's first three
// dwords stored by the wave below): lane exchanges both ways and stores that are no longer whole
// vectors, against two AES blocks that ride in the rounds of the other four. With the chunk kept
// where it is, the first CRC reads the loaded registers, the second the re-keyed ones, and no lane
// reads another's bytes.
//   GHASH, twice. The old ciphertext is absorbed under H_src and the new one under H_dst, each as
// sse_write_kernel does: the tail of block g - 1, blocks g .. g + 2, the head of block g + 3, five
// elements per chunk by linearity, a lane's step between its tiles gcm::write_jump for that key. The
// nonce dwords and every byte from 12 + n on count as zero on both sides, so the source's partials
// fold to what sse_read_kernel's would (gcm::tag_matches on the host) and the destination's to what
// sse_write_kernel's would (gcm::unfold, gcm::finish_tag). The source's nonce is read from its first
// three dwords; the host learns it, and the stored tag, from `nonce_tag`.
//
// CRC, twice, on the matrix cores through the permlane32 route. The loaded chunk is compared with the
// source's .meta image (minimum bad slice per workgroup; the short tail slice by workgroup 0 from
// byte loads, as sse_read_kernel). The re-keyed chunk gives the .meta words of the slices in front
// of the tag, to HBM and to the host image, and the raw whole-block partials, as sse_write_kernel.
// The slices behind them hold the tag, which only the host can close: their bytes (under 528, with
// zeros for the tag) are stored a second time into `tail_host`, so the host checksums them without a
// copy back; they are all of the payload that crosses the link.
//   The kernel stores before it can know that the source verifies: the host looks at part_bad and
// the source's tag first, and releases the extent unless both hold, so no block ever names those
// bytes.
//
// Scalar registers. Two key schedules are 120 words, and two sets of H, jump and tree powers 72 more:
// they do not fit the scalar file. All of it stays in the kernel-argument segment. The AES round
// loop is not unrolled and indexes the schedule by the round, so the compiler loads the four words
// of a round from the segment as the round begins (one scalar load of four dwords, for either key),
// and H, the jump and the tree steps are loaded where they are used; only one schedule's round and
// one power of H are live at a time. The two keystreams run one after the other over the same 20
// state registers. Two waves per SIMD as the read and write kernels (the CRC basis alone is 64
// registers), no scratch: see the resource report in profiles/r14.
__device__ __forceinline__ WaveData chunk_operand(const uint32_t (&c)[16]) {
  uint32_t p0[8], p1[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const auto r = __builtin_amdgcn_permlane32_swap(c[k], c[8 + k], false, false);
    p0[k] = r[0];  // lanes 0..31: own dword k; lanes 32..63: dword 8 + k of lane - 32
    p1[k] = r[1];  // lanes 0..31: dword k of lane + 32; lanes 32..63: own dword 8 + k
  }
  WaveData w;
  w.v[0] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
  w.v[1] = make_uint4(p0[4], p0[5], p0[6], p0[7]);
  w.v[2] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
  w.v[3] = make_uint4(p1[4], p1[5], p1[6], p1[7]);
  return w;
}

// The five elements of a chunk on the CRC axis (its dwords c, zero where no ciphertext stands).
__device__ __forceinline__ gcm::U128 ghash_absorb_chunk(gcm::U128 acc, const gcm::U128& h, const uint32_t (&c)[16]) {
  const uint32_t e0[4] = {0, c[0], c[1], c[2]};
  acc = ghash_absorb(acc, h, e0);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const uint32_t e[4] = {c[4 * b + 3], c[4 * b + 4], c[4 * b + 5], c[4 * b + 6]};
    acc = ghash_absorb(acc, h, e);
  }
  const uint32_t e4[4] = {c[15], 0, 0, 0};
  return ghash_absorb(acc, h, e4);
}

__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sse_rekey_kernel(
    SseRekeyLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(kCrcWgThreads == 256 && gcm::kGcmTileBlocks * 16 == kSlicesPerTile * 512, "a CRC tile is a GCM tile");
  __shared__ MfmaTileLds lt;
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part_src[4], wave_part_dst[4];
  __shared__ uint32_t wacc[4];
  __shared__ uint32_t wg_bad;
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sw = lane >> 3, sl = lane & 7;
  const int64_t n = static_cast<int64_t>(a.n), size = n + 28, nvec = (size + 15) / 16, s_full = size / 512;
  const int64_t s_body = static_cast<int64_t>(sse_write_body_slices(a.n));
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.src);
  auto first_vector = [&](uint64_t tile) { return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x); };
  auto fetch = [&](uint64_t tile, uint4 (&v)[4]) {
    const int64_t g = first_vector(tile);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = make_uint4(0, 0, 0, 0);
      if (g + i < nvec) {  // the vector behind the block's end is never loaded
        const u32x4 x = __builtin_nontemporal_load(src + g + i);
        v[i] = make_uint4(x[0], x[1], x[2], x[3]);
      }
    }
  };

  // Zero where no ciphertext stands: the nonce's dwords in the blob's first chunk, and every byte from
  // 12 + n on. Only those few chunks take the branch, so no mask is live through the AES rounds.
  auto mask = [&](int64_t g, uint32_t (&c)[16]) {
    if (g != 0 && 16 * g + 64 <= 12 + n) return;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t p = 16 * g + 4 * i;  // the dword's first byte in the blob
      c[i] = p < 12 ? 0u : c[i] & sse_keep(12 + n - p);
    }
  };

  uint4 cur[4];
  fetch(blockIdx.x, cur);
  i32x4 A[16];
  load_basis(reinterpret_cast<const i32x4*>(gt + 1), lane, A);
  load_lds_image(gt, &lt);
  sse_load_tables(gt, te0, sbox);
  if (threadIdx.x == 0) wg_bad = 0xFFFFFFFFu;
  // the source's nonce: the block's first three dwords, the same for every lane
  const uint32_t* head = reinterpret_cast<const uint32_t*>(a.src);
  const uint32_t s0 = head[0], s1 = head[1], s2 = head[2];
  if (blockIdx.x == 0 && threadIdx.x < 28)  // nonce and stored tag for the host: block bytes [0, 12) and [12 + n, 28 + n)
    a.nonce_tag[threadIdx.x] = a.src[threadIdx.x < 12 ? threadIdx.x : n + threadIdx.x];
  __syncthreads();

  gcm::U128 acc_src{0, 0}, acc_dst{0, 0};
  uint32_t bad = 0xFFFFFFFFu, crc = 0;
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    uint4 nxt[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x, nxt);
    const int64_t g = first_vector(tile);
    const int64_t slice = static_cast<int64_t>(tile) * kSlicesPerTile + wave * 8 + sw;
    uint32_t c[16] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                      cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};

    // verify the source: the chunk as loaded
    {
      const uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, chunk_operand(c), lane), lane);
      if (slice < s_full && sl == 0 && a.src_meta[slice] != __builtin_bswap32(r ^ a.full_init))
        bad = min(bad, static_cast<uint32_t>(slice));
    }

    // authenticate the source: its ciphertext alone, zero where the nonce, the tag and the rest stand
    mask(g, c);
    if (tile != blockIdx.x) acc_src = gcm::gf128_mul(a.from.hjump, acc_src);
    acc_src = ghash_absorb_chunk(acc_src, a.from.h, c);

    // re-key: the keystreams of blocks g - 1 .. g + 3 under either key, one after the other; chunk
    // dword i takes dword (i + 1) % 4 of block g - 1 + (i + 1) / 4
    {
      uint32_t ks[5][4];
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        ks[b][0] = s0;
        ks[b][1] = s1;
        ks[b][2] = s2;
        ks[b][3] = gcm::bswap32(1u + static_cast<uint32_t>(g + b));
      }
      gcm::aes256_encrypt_words<5>(te0, sbox, a.from.rk, ks);
#pragma unroll
      for (int i = 0; i < 16; ++i) c[i] ^= ks[(i + 1) >> 2][(i + 1) & 3];
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        ks[b][0] = a.nonce[0];
        ks[b][1] = a.nonce[1];
        ks[b][2] = a.nonce[2];
        ks[b][3] = gcm::bswap32(1u + static_cast<uint32_t>(g + b));
      }
      gcm::aes256_encrypt_words<5>(te0, sbox, a.to.rk, ks);
#pragma unroll
      for (int i = 0; i < 16; ++i) c[i] ^= ks[(i + 1) >> 2][(i + 1) & 3];
    }
    mask(g, c);

    // authenticate the destination, then put its nonce where it belongs: no part of any element
    if (tile != blockIdx.x) acc_dst = gcm::gf128_mul(a.to.hjump, acc_dst);
    acc_dst = ghash_absorb_chunk(acc_dst, a.to.h, c);
    if (g == 0) {
      c[0] = a.nonce[0];
      c[1] = a.nonce[1];
      c[2] = a.nonce[2];
    }

    // land: the extent is padded to 16 B; zeros where the tag goes and behind it
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t pos = 16 * (g + i);
      if (pos >= size) continue;
      const uint4 v = make_uint4(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
      *reinterpret_cast<uint4*>(a.dst + pos) = v;
      // the host's slices (at most 512 + 15 bytes and the pad) also where it can checksum them
      if (pos >= s_body * 512) *reinterpret_cast<uint4*>(a.tail_host + (pos - s_body * 512)) = v;
    }

    // checksum the destination: the slices in front of the tag, and the whole-block partial
    {
      uint32_t r = slice_from_chunks(lt, wave_chunk_crcs(A, chunk_operand(c), lane), lane);
      if (slice >= s_body) {
        r = 0;  // the host's slices, and zeros to the whole-block CRC
      } else if (sl == 0) {
        const uint32_t be = __builtin_bswap32(r ^ a.full_init);
        a.meta[slice] = be;
        a.meta_host[slice] = be;
      }
      r = combine<8>(r, lane, lt.sh512);
      r = combine<16>(r, lane, lt.sh1k);
      r = combine<32>(r, lane, lt.sh2k);  // wave-uniform: the 4 KiB sub-tile's raw CRC
      if (tile != blockIdx.x) {
        uint32_t e = gridDim.x;
        for (int b = 0; e; ++b, e >>= 1)
          if (e & 1) crc = mat_apply(lt.tile_pow2[b], crc, lane);
      }
      crc ^= r;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
  }

  if (size % 512 && blockIdx.x == 0 && wave == 0) {  // the source's short tail slice
    const uint32_t tail_len = static_cast<uint32_t>(size % 512);
    const uint32_t r =
        slice_from_chunks(lt, wave_chunk_crcs(A, load_tail_wave(a.src + s_full * 512, tail_len, lane), lane), lane);
    if (lane == 0 && a.src_meta[s_full] != __builtin_bswap32(r ^ a.tail_init)) bad = min(bad, static_cast<uint32_t>(s_full));
  }
  if (bad != 0xFFFFFFFFu) atomicMin(&wg_bad, bad);
  // the wave's CRC stands at the end of its sub-tile in the workgroup's last tile: to the axis's end
  {
    for (int k = wave; k < 3; ++k) crc = tab4(lt.sh4k, crc);
    const uint64_t last = blockIdx.x + (a.ntiles - 1 - blockIdx.x) / gridDim.x * gridDim.x;
    uint64_t e = a.ntiles - 1 - last;
    for (int b = 0; e; ++b, e >>= 1)
      if (e & 1) crc = mat_apply(lt.tile_pow2[b], crc, lane);
    if (lane == 0) wacc[wave] = crc;
  }
  ghash_wg_partial(acc_src, a.from.tree, wave_part_src, a.from.part);  // its barrier orders wg_bad and wacc too
  ghash_wg_partial(acc_dst, a.to.tree, wave_part_dst, a.to.part);
  if (threadIdx.x == 0) {
    a.part_bad[blockIdx.x] = wg_bad;
    a.part_crc[blockIdx.x] = wacc[0] ^ wacc[1] ^ wacc[2] ^ wacc[3];
  }
}

// ---- K7 EC read: a GET of an SSE-S3 object held as RS(k, m) shards, in one pass ----
//
// The stored blob [nonce 12][ciphertext n][tag 16] is not in HBM as one extent: blob byte x is byte
// x % sl of data column x / sl, and a column is either a surviving shard or the GF(2^8) product of
// the k survivors. The kernel treats the shards as the blob: it has sse_read_kernel's tiles (16 KiB
// of the axis per workgroup step, thread t owns AES blocks 1024 T + 4t .. + 3, the plan
// gcm::plan_for(16 KiB * ntiles)), its AES, its GHASH and its stores, and in front of them a load
// stage that builds a thread's four ciphertext blocks out of shard vectors.
//
// Virtual-blob load. AES block q is blob bytes [16q + 12, 16q + 28). Byte p of column c is blob byte
// c * sl + p, so on the AES axis the column starts at delta = c * sl - 12, and with q and the
// shard's vector index v both on 16 B grids the only per-column quantity is the byte shift
// delta & 15: block q takes its low `shift` bytes from the top of shard vector v - 1 and the rest
// from the bottom of v, v = q - (delta >> 4). The 12 bytes between the blob's vector grid and the
// AES blocks are part of that shift, not a second funnel. A wave (64 threads, 4 KiB of the axis) walks
// the columns that its span touches with a wave-uniform c, shard pointer and shift: a thread loads
// its four aligned vectors of the shard, takes vector v - 1 from the lane below (lane_below; lane 0
// loads that one vector itself) and funnels with v_alignbyte_b32. The bytes that fall outside the
// column's window [delta, delta + sl) are masked off and the passes ORed, which is how a thread, or
// a block, that straddles a column boundary merges its two columns. The shard pointers are only
// ever indexed with the wave-uniform column (scalar loads from the kernel arguments).
//   With sl >= kSseEcReadMinShard = 4 KiB a wave's span touches at most two columns; the first one's
// vectors for the workgroup's next tile are loaded before the current tile is decrypted.
//
// Lost columns. A pass over a lost column builds the same five vectors as the product of reconstruct
// row r with the k survivors' vectors at the same indices (split-nibble v_perm_b32 form, the row's
// tables broadcast from LDS, the next survivor's loads issued before the current one's arithmetic).
// Because the axis is the blob's, a span never needs two rebuilt columns at the same shard position,
// so one set of accumulators (five vectors, the fifth live in lane 0 only) serves any number of lost
// columns: the template argument only says whether the rebuild exists. Parity survivors are only
// ever multiplied. Every column is rebuilt, the tag covers the whole blob.
//
// Nonce and tag. The nonce is vector 0 of column 0: a scalar load where that column survives, else
// k uniform 16 B loads and one product, which every thread of the workgroup does alike (the loads are
// of one and the same vector, and nothing has to be shared through LDS). The stored tag is AES-axis bytes [n, n + 16):
// the threads whose blocks hold them store them to `nonce_tag` from the merged registers, so it may
// lie in a rebuilt column or across a boundary.
//
// No CRC stage: as with ec_read_kernel the caller hands over verified shards (the gather scrubs the
// local one, peers' shards are checksummed as they land), and the GCM tag authenticates the result.
// The compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950):
//   rebuild  VGPRs  SGPRs  SGPR spills           scratch  LDS bytes  waves per SIMD
//   no        137    106    15 (to VGPR lanes)      0       1376     2
//   yes       231    105     0                      0       5472     2
struct ColVecs {
  uint4 v[4];
  uint4 below;  // lane 0: the vector under v[0]
};

// Block bytes [16v - shift, 16v - shift + 16) of a shard: the top `shift` bytes of vector v - 1 under
// the low 16 - shift of vector v. `shift` is wave-uniform.
__device__ __forceinline__ uint4 shift_up(const uint4& prev, const uint4& cur, uint32_t shift) {
  if (!shift) return cur;
  const uint32_t w = (16u - shift) >> 2, b = (16u - shift) & 3u;
  uint32_t e0, e1, e2, e3, e4;
  switch (w) {
    case 0: e0 = prev.x; e1 = prev.y; e2 = prev.z; e3 = prev.w; e4 = cur.x; break;
    case 1: e0 = prev.y; e1 = prev.z; e2 = prev.w; e3 = cur.x; e4 = cur.y; break;
    case 2: e0 = prev.z; e1 = prev.w; e2 = cur.x; e3 = cur.y; e4 = cur.z; break;
    default: e0 = prev.w; e1 = cur.x; e2 = cur.y; e3 = cur.z; e4 = cur.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(e1, e0, b), __builtin_amdgcn_alignbyte(e2, e1, b),
                    __builtin_amdgcn_alignbyte(e3, e2, b), __builtin_amdgcn_alignbyte(e4, e3, b));
}

__device__ __forceinline__ void gf_mul_add(const uint32_t (&tb)[8], const uint4& d, uint4& acc) {
  acc.x ^= gf_mul4(tb, nibble_sel(d.x));
  acc.y ^= gf_mul4(tb, nibble_sel(d.y));
  acc.z ^= gf_mul4(tb, nibble_sel(d.z));
  acc.w ^= gf_mul4(tb, nibble_sel(d.w));
}

constexpr int kColNone = -128;  // col_src: a column that nothing supplies (the launch refuses it)

template <bool kRebuild>
__global__ __launch_bounds__(kCrcWgThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void sse_ec_read_kernel(
    SseEcReadLaunch a, const DevCrcTables* __restrict__ gt) {
  static_assert(kCrcWgThreads == 256 && gcm::kGcmTileBlocks * 16 == kSseReadTileBytes, "sse_read_kernel's tiles");
  static_assert(kSseEcReadMinShard >= 16 * gcm::kGcmWaveBlocks, "a wave's span touches at most two columns");
  __shared__ uint32_t te0[256];
  __shared__ uint8_t sbox[256];
  __shared__ gcm::U128 wave_part[4];
  __shared__ int8_t col_src[kMaxShards];  // column c: survivor j >= 0, or -1 - r for reconstruct row r
  __shared__ uint32_t gft[kRebuild ? kEcFusedMaxRows * kMaxShards * 8 : 1];
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), k = a.k;
  const int64_t n = static_cast<int64_t>(a.n), sl = static_cast<int64_t>(a.sl), nvec = (sl + 15) / 16;

  sse_load_tables(gt, te0, sbox);
  if (threadIdx.x < static_cast<unsigned>(k)) {
    int src = kColNone;
    for (int j = 0; j < k; ++j)
      if (a.surv_col[j] == static_cast<int>(threadIdx.x)) src = j;
    for (int r = 0; r < a.rows; ++r)
      if (a.row_col[r] == static_cast<int>(threadIdx.x)) src = -1 - r;
    col_src[threadIdx.x] = static_cast<int8_t>(src);
  }
  if constexpr (kRebuild)
    for (int i = threadIdx.x; i < a.rows * k * 8; i += kCrcWgThreads) gft[i] = a.tables[i];
  __syncthreads();

  auto load = [&](const u32x4* base, int64_t v) {
    uint4 d = make_uint4(0, 0, 0, 0);
    if (v >= 0 && v < nvec) {  // inside the shard's padded buffer
      const u32x4 x = __builtin_nontemporal_load(base + v);
      d = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return d;
  };
  // survivor j's vectors v0 .. v0 + 3 and, in lane 0, v0 - 1
  auto fetch = [&](int j, int64_t v0, ColVecs& r) {
    const u32x4* base = reinterpret_cast<const u32x4*>(a.in[j]);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = load(base, v0 + i);
    r.below = lane == 0 ? load(base, v0 - 1) : make_uint4(0, 0, 0, 0);
  };
  auto zero = [](ColVecs& r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = make_uint4(0, 0, 0, 0);
    r.below = make_uint4(0, 0, 0, 0);
  };
  auto source_of = [&](int c) { return __builtin_amdgcn_readfirstlane(static_cast<int>(col_src[c])); };
  auto first_block = [&](uint64_t tile) { return static_cast<int64_t>(tile * gcm::kGcmTileBlocks + 4 * threadIdx.x); };
  // the columns that the wave's 4 KiB of tile `tile` touch: blob bytes [x0, x0 + 4096)
  auto span = [&](uint64_t tile, int& c_lo, int& c_hi) {
    const int64_t x0 = static_cast<int64_t>(tile * kSseReadTileBytes) + 16 * gcm::kGcmWaveBlocks * wave + 12;
    c_lo = static_cast<int>(min(x0 / sl, static_cast<int64_t>(k)));
    c_hi = static_cast<int>(min((x0 + 16 * gcm::kGcmWaveBlocks - 1) / sl, static_cast<int64_t>(k - 1)));
  };
  // the thread's first shard vector of column c
  auto first_vector = [&](uint64_t tile, int c) { return first_block(tile) - ((c * sl - 12) >> 4); };
  // the vectors of the wave's first column of a tile, where a survivor holds it
  auto prefetch = [&](uint64_t tile, ColVecs& r) {
    zero(r);
    int c_lo, c_hi;
    span(tile, c_lo, c_hi);
    if (c_lo > c_hi) return;
    const int src = source_of(c_lo);
    if (src >= 0) fetch(src, first_vector(tile, c_lo), r);
  };

  // the nonce: blob bytes [0, 12), the head of column 0
  uint32_t n0 = 0, n1 = 0, n2 = 0;
  {
    const int src = source_of(0);
    if (src >= 0) {
      const uint32_t* head = reinterpret_cast<const uint32_t*>(a.in[src]);
      n0 = head[0];
      n1 = head[1];
      n2 = head[2];
    } else if constexpr (kRebuild) {
      if (src != kColNone) {
        uint4 acc = make_uint4(0, 0, 0, 0);
        for (int j = 0; j < k; ++j) {
          uint32_t tb[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) tb[q] = gft[((-1 - src) * k + j) * 8 + q];
          gf_mul_add(tb, load(reinterpret_cast<const u32x4*>(a.in[j]), 0), acc);
        }
        n0 = __builtin_amdgcn_readfirstlane(acc.x);
        n1 = __builtin_amdgcn_readfirstlane(acc.y);
        n2 = __builtin_amdgcn_readfirstlane(acc.z);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 12) {
    const uint32_t w = threadIdx.x < 4 ? n0 : threadIdx.x < 8 ? n1 : n2;
    a.nonce_tag[threadIdx.x] = static_cast<uint8_t>(w >> (8 * (threadIdx.x & 3)));
  }

  gcm::U128 acc{0, 0};
  ColVecs cur;
  prefetch(blockIdx.x, cur);
  for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    ColVecs nxt;
    zero(nxt);
    if (tile + gridDim.x < a.ntiles) prefetch(tile + gridDim.x, nxt);
    const int64_t g = first_block(tile);

    // the ciphertext of blocks g .. g + 3, column by column
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = 0;
    int c_lo, c_hi;
    span(tile, c_lo, c_hi);
    for (int c = c_lo; c <= c_hi; ++c) {
      const int src = source_of(c);
      const int64_t delta = c * sl - 12, v0 = first_vector(tile, c);
      ColVecs x;
      if (src >= 0) {
        if (c == c_lo) x = cur;
        else fetch(src, v0, x);
      } else {
        zero(x);
        if constexpr (kRebuild) {
          if (src != kColNone) {
            const uint32_t* row = gft + (-1 - src) * k * 8;
            ColVecs d;
            fetch(0, v0, d);
            for (int j = 0; j < k; ++j) {
              ColVecs dn;
              if (j + 1 < k) fetch(j + 1, v0, dn);
              uint32_t tb[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) tb[q] = row[j * 8 + q];
#pragma unroll
              for (int i = 0; i < 4; ++i) gf_mul_add(tb, d.v[i], x.v[i]);
              gf_mul_add(tb, d.below, x.below);
              if (j + 1 < k) d = dn;
            }
          }
        }
      }
      const uint32_t shift = static_cast<uint32_t>(delta) & 15u;
      uint4 blk[4];
      {
        const uint4 under = make_uint4(lane_below(x.v[3].x, x.below.x), lane_below(x.v[3].y, x.below.y),
                                       lane_below(x.v[3].z, x.below.z), lane_below(x.v[3].w, x.below.w));
        blk[0] = shift_up(under, x.v[0], shift);
#pragma unroll
        for (int i = 1; i < 4; ++i) blk[i] = shift_up(x.v[i - 1], x.v[i], shift);
      }
      const uint32_t w[16] = {blk[0].x, blk[0].y, blk[0].z, blk[0].w, blk[1].x, blk[1].y, blk[1].z, blk[1].w,
                              blk[2].x, blk[2].y, blk[2].z, blk[2].w, blk[3].x, blk[3].y, blk[3].z, blk[3].w};
      // the column's window on the AES axis is [delta, delta + sl)
      const int64_t y = 16 * g;
      if (y >= delta && y + 64 <= delta + sl) {
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = w[i];
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          m[i] |= w[i] & sse_keep(delta + sl - y - 4 * i) & ~sse_keep(delta - y - 4 * i);
      }
    }

    // the stored tag, AES-axis bytes [n, n + 16), for the host
    if (16 * g + 64 > n && 16 * g < n + 16) {
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const int64_t y = 16 * g + i;
        if (y >= n && y < n + 16) a.nonce_tag[12 + (y - n)] = static_cast<uint8_t>(m[i >> 2] >> (8 * (i & 3)));
      }
    }

    uint32_t ks[4][4];
    sse_keystream(te0, sbox, a.rk, n0, n1, n2, g, ks);

    if (tile != blockIdx.x) acc = gcm::gf128_mul(a.hjump, acc);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t pos = 16 * (g + b);  // of the block in the message and in `out`
      uint32_t c[4], o[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        c[kk] = m[4 * b + kk] & sse_keep(n - pos - 4 * kk);
        o[kk] = m[4 * b + kk] ^ ks[b][kk];
      }
      acc = ghash_absorb(acc, a.h, c);
      if (pos + 16 <= n) {
        *reinterpret_cast<uint4*>(a.out + pos) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        for (int64_t p = pos; p < n; ++p) a.out[p] = static_cast<uint8_t>(o[(p - pos) >> 2] >> (8 * ((p - pos) & 3)));
      }
    }
    cur = nxt;
  }
  ghash_wg_partial(acc, a.tree, wave_part, a.part);
}

}  // namespace

// Raw CRC (zero init, no xorout) of a 64-byte message whose only set bit is bit p of byte b.
static uint32_t chunk_basis_crc(int b, int p) {
  uint32_t r = 0;
  for (int i = 0; i < 64; ++i) {
    r ^= i == b ? (1u << p) : 0u;
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1u) ? kCrcPoly : 0u);
  }
  return r;
}

static std::atomic<int> g_crc_mfma{-1};

bool crc_mfma_enabled() {
  int v = g_crc_mfma.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = std::getenv("DFS_CRC_MFMA");
    v = (e && e[0] == '0') ? 0 : 1;
    g_crc_mfma.store(v);
  }
  return v == 1;
}

void set_crc_mfma(bool on) { g_crc_mfma.store(on ? 1 : 0); }

static std::atomic<int> g_crc_ring{0}, g_crc_tile_ring{0};

static int ring_env(const char* name, int dflt) {
  const char* e = std::getenv(name);
  int v = e ? std::atoi(e) : dflt;
  return v < 2 ? 2 : (v > 4 ? 4 : v);
}

int crc_ring_buffers() {
  int v = g_crc_ring.load(std::memory_order_relaxed);
  if (v == 0) g_crc_ring.store(v = ring_env("DFS_CRC_RING", kCrcRingDefault));
  return v;
}

int crc_tile_ring_buffers() {
  int v = g_crc_tile_ring.load(std::memory_order_relaxed);
  if (v == 0) g_crc_tile_ring.store(v = ring_env("DFS_CRC_TILE_RING", kCrcTileRingDefault));
  return v;
}

void set_crc_ring(int scrub_buffers, int tile_buffers) {
  g_crc_ring.store(scrub_buffers < 2 ? 2 : (scrub_buffers > 4 ? 4 : scrub_buffers));
  g_crc_tile_ring.store(tile_buffers < 2 ? 2 : (tile_buffers > 4 ? 4 : tile_buffers));
}

// Ring depth of a K1/K2/K3 launch over `ntiles` tiles: a deep ring only pays once workgroups
// have several tiles each (below kCrcRingMinTiles its longer prologue costs ~0.3 us per
// launch, e.g. on 1 MiB blocks).
// Size-based K1/K2 dispatch: below DFS_CRC_LDS_MAX_MIB (default 16 MiB) the LDS-table kernel
// wins (its per-workgroup setup is smaller: 1 MiB 6.02 vs 6.47 us, 8 MiB 7.39 vs 8.89 us in
// profiles/archive/r2_crc4/crc_default.json); from 64 MiB up the matrix-core kernel is 1.3-1.9x faster.
static std::atomic<int64_t> g_lds_max_mib{-1};

void set_crc_lds_max_mib(int mib) { g_lds_max_mib.store(mib < 0 ? 0 : mib); }

static uint64_t lds_max_tiles() {
  int64_t mib = g_lds_max_mib.load(std::memory_order_relaxed);
  if (mib < 0) {
    const char* e = std::getenv("DFS_CRC_LDS_MAX_MIB");
    long v = e ? std::atol(e) : kCrcLdsMaxMibDefault;
    g_lds_max_mib.store(mib = v > 0 ? v : 0);
  }
  return static_cast<uint64_t>(mib) * (1ull << 20) / (kSlicesPerTile * 512ull);
}

static int ring_for(uint64_t ntiles) {
  if (!crc_mfma_enabled() || ntiles < lds_max_tiles()) return 0;
  return ntiles >= kCrcRingMinTiles ? crc_tile_ring_buffers() : 2;
}

// One resident round: 3 workgroups per CU at 3 waves/SIMD (R = 2), 2 at 2 waves/SIMD.
static uint64_t crc_grid_cap(int ring) { return ring > 2 ? 2 * 256 : kMaxGridCrc; }

// K1/K2 as crc_tile_wide_kernel (one workgroup of G x 4 waves per CU): 0 = off, 1 = G = 3
// (3 waves/SIMD), 2 = G = 2 (2 waves/SIMD). DFS_CRC_WIDE overrides the default.
// Why G = 2 can win although it halves the waves: the loop is matrix-pipe + VALU bound, so a
// tile-iteration of a group costs ~G units on a CU, and a block of T tiles takes
// ceil(T / (256 G)) iterations: 64 MiB = 4096 tiles is 6 x 3 = 18 units at G = 3 (runs of 5 or
// 6: the CUs with 6 set the time) but 8 x 2 = 16 at G = 2 (every run exactly 8); every
// power-of-two size divides evenly at G = 2.
static std::atomic<int> g_crc_wide{-1};

void set_crc_wide(int mode) { g_crc_wide.store(mode <= 0 ? 0 : (mode >= 2 ? 2 : 1)); }

int crc_wide_mode() {
  int v = g_crc_wide.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = std::getenv("DFS_CRC_WIDE");
    v = e ? std::atoi(e) : kCrcWideDefault;
    g_crc_wide.store(v = v <= 0 ? 0 : (v >= 2 ? 2 : 1));
  }
  return v;
}

static int crc_wide_groups() { return crc_wide_mode() == 2 ? 2 : kMaxGridCrc / 256; }

static std::atomic<int> g_crc_fp4{-1};

void set_crc_fp4(bool on) { g_crc_fp4.store(on ? 1 : 0); }

bool crc_fp4_enabled() {
  int v = g_crc_fp4.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = std::getenv("DFS_CRC_FP4");
    g_crc_fp4.store(v = (e ? std::atoi(e) : kCrcFp4Default) ? 1 : 0);
  }
  return v != 0;
}

DevCrcTables* upload_crc_tables(hipStream_t s) {
  static_assert(sizeof(DevCrcTables) % 16 == 0, "table image must be uint4-copyable");
  std::vector<uint8_t> host(sizeof(DevCrcTables));
  auto* t = reinterpret_cast<DevCrcTables*>(host.data());
  std::memcpy(t->slice16, crc_tables().slice16, sizeof(t->slice16));
  shift_table(64, t->sh64);
  shift_table(128, t->sh128);
  shift_table(256, t->sh256);
  shift_table(512, t->sh512);
  shift_table(1024, t->sh1k);
  shift_table(2048, t->sh2k);
  shift_table(4096, t->sh4k);
  for (int b = 0; b < 32; ++b) {
    const Gf2Mat& m = shift_pow2_bytes(14 + b);  // 16 KiB * 2^b
    std::memcpy(t->tile_pow2[b], m.col, sizeof(m.col));
  }
  // MFMA basis right behind the LDS image (never copied to LDS): fragment [s][lane] of A,
  // element j = byte j of the 16 B: CRC bit i = lane & 31 of V[32h + 4(s>>1) + (j&3)][4(s&1) + (j>>2)],
  // scaled by 2^(7-p) (see wave_chunk_crcs)
  host.resize(sizeof(DevCrcTables) + kSseTablesOffset + kSseTablesBytes);
  static_assert(sizeof(gcm::AesTables) == kSseTablesBytes && kSseTablesOffset % 16 == 0, "AES tables end the image");
  std::memcpy(host.data() + sizeof(DevCrcTables) + kSseTablesOffset, &gcm::aes_tables(), kSseTablesBytes);
  static_assert(kCrcBasisFp4Offset == kCrcBasisBytes + kCrcChunkShiftBytes + kCrcWideExtraBytes, "image order");
  // chunk-shift tables behind the basis: cs[sl] moves a 64 B chunk's CRC past 64 * (7 - sl) bytes;
  // then ss[sw] (a slice's CRC past 512 * (7 - sw) bytes) and the 16 KiB tile shift
  auto* cs = reinterpret_cast<uint32_t(*)[4][256]>(host.data() + sizeof(DevCrcTables) + kCrcBasisBytes);
  for (int sl = 0; sl < 7; ++sl) shift_table(64 * (7 - sl), cs[sl]);
  for (int sw = 0; sw < 7; ++sw) shift_table(512 * (7 - sw), cs[7 + sw]);
  shift_table(16384, cs[14]);
  int8_t* basis = reinterpret_cast<int8_t*>(host.data() + sizeof(DevCrcTables));
  for (int st = 0; st < 16; ++st)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 16; ++j) {
        // row R = lane & 31 of A carries CRC bit R ^ 7 (the order wave_chunk_crcs gathers in)
        const int h = lane >> 5, bit = (lane & 31) ^ 7;
        const int byte = 32 * h + 4 * (st >> 1) + (j & 3), p = 4 * (st & 1) + (j >> 2);
        const uint32_t v = chunk_basis_crc(byte, p);
        basis[(st * 64 + lane) * 16 + j] = ((v >> bit) & 1u) ? static_cast<int8_t>(static_cast<uint8_t>(1u << (7 - p))) : 0;
      }
  // FP4 basis (wave_chunk_crcs_fp4): fragment [s][lane], dword r, nibble q is the element that
  // B takes from bit 4(q & 1) + r of byte (q >> 1) of data dword s of the lane's 32 B half;
  // value 2.0 / 1.0 / 0.5 / 0.5 (e2m1 0b0100 / 0b0010 / 0b0001) for planes r = 0..3 where
  // the basis bit is set, so the product with B's 0.5 / 1.0 / 2.0 / 2.0 is 1.0
  uint8_t* b4 = host.data() + sizeof(DevCrcTables) + kCrcBasisFp4Offset;
  std::memset(b4, 0, kCrcBasisFp4Bytes);
  static const uint8_t kFp4Code[4] = {0x4, 0x2, 0x1, 0x1};
  for (int st = 0; st < 8; ++st)
    for (int lane = 0; lane < 64; ++lane)
      for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 8; ++q) {
          const int h = lane >> 5, bit = (lane & 31) ^ 7;
          const uint32_t v = chunk_basis_crc(32 * h + 4 * st + (q >> 1), 4 * (q & 1) + r);
          if ((v >> bit) & 1u) b4[(st * 64 + lane) * 16 + 4 * r + (q >> 1)] |= kFp4Code[r] << (4 * (q & 1));
        }
  t = reinterpret_cast<DevCrcTables*>(host.data());
  DevCrcTables* d = nullptr;
  if (hipMalloc(&d, host.size()) != hipSuccess) return nullptr;
  if (hipMemcpyAsync(d, host.data(), host.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  return d;
}


int crc_grid_for(uint64_t ntiles, uint32_t has_tail) {
  // small blocks: at least `per` tiles per workgroup, so the per-workgroup fixed cost (the
  // 16 KiB basis per wave and the LDS image, both from L2) is amortised over more data
  static const uint64_t per = [] {
    const char* e = std::getenv("DFS_CRC_MIN_TILES_PER_WG");
    long v = e ? std::atol(e) : 1;
    return static_cast<uint64_t>(v > 0 ? v : 1);
  }();
  uint64_t g = (ntiles + per - 1) / per;
  const int ring = ring_for(ntiles);
  uint64_t cap = crc_grid_cap(ring);
  const uint64_t G = crc_wide_groups();
  if (ring == 2 && crc_wide_mode()) cap = 256 * G;  // one resident round of the wide kernel
  g = g < cap ? g : cap;
  // the wide kernel runs G virtual workgroups per launched one (empty runs leave a zero
  // partial and no verdict)
  if (ring == 2 && crc_wide_mode() && g) g = (g + G - 1) / G * G;
  if (g == 0 && has_tail) g = 1;
  return static_cast<int>(g);
}

bool crc_meta_host_ok(uint64_t ntiles) { return ring_for(ntiles) == 0; }

hipError_t launch_crc(const CrcLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  if (grid <= 0) return hipSuccess;
  if (a.meta_host && ring_for(a.ntiles) != 0) return hipErrorInvalidValue;  // only the LDS kernel mirrors it
  switch (ring_for(a.ntiles)) {
    case 0: hipLaunchKernelGGL(crc_slices_kernel, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t); break;
    case 2:
      if (crc_wide_mode() && grid % crc_wide_groups() == 0) {
        const int G = crc_wide_groups();
        const dim3 g(grid / G), b(kCrcWgThreads * G);
        const bool w = a.meta_out && !a.meta_expect && a.part_crc;
        constexpr int G3 = kMaxGridCrc / 256;
        const int v = (G == 2 ? 0 : 4) | (w ? 2 : 0) | (crc_fp4_enabled() ? 1 : 0);
        switch (v) {
          case 0: hipLaunchKernelGGL((crc_tile_wide_kernel<2, false, false>), g, b, 0, s, a, t); break;
          case 1: hipLaunchKernelGGL((crc_tile_wide_kernel<2, false, true>), g, b, 0, s, a, t); break;
          case 2: hipLaunchKernelGGL((crc_tile_wide_kernel<2, true, false>), g, b, 0, s, a, t); break;
          case 3: hipLaunchKernelGGL((crc_tile_wide_kernel<2, true, true>), g, b, 0, s, a, t); break;
          case 4: hipLaunchKernelGGL((crc_tile_wide_kernel<G3, false, false>), g, b, 0, s, a, t); break;
          case 5: hipLaunchKernelGGL((crc_tile_wide_kernel<G3, false, true>), g, b, 0, s, a, t); break;
          case 6: hipLaunchKernelGGL((crc_tile_wide_kernel<G3, true, false>), g, b, 0, s, a, t); break;
          default: hipLaunchKernelGGL((crc_tile_wide_kernel<G3, true, true>), g, b, 0, s, a, t); break;
        }
      } else {
        hipLaunchKernelGGL(crc_tile_mfma_kernel, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t);
      }
      break;
    case 3: hipLaunchKernelGGL(crc_tile_ring_kernel<3>, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t); break;
    default: hipLaunchKernelGGL(crc_tile_ring_kernel<4>, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t); break;
  }
  return hipGetLastError();
}

hipError_t launch_read_copy(const ReadCopyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  if (grid <= 0) return hipSuccess;
  if (grid > kMaxGridCrc) return hipErrorInvalidValue;  // part_bad holds kMaxGridCrc words
  hipLaunchKernelGGL(crc_read_copy_kernel, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

hipError_t launch_write_copy(const WriteCopyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  if (grid <= 0) return hipSuccess;
  // part_crc holds kMaxGridCrc words; the plan must be a whole block (K1/K2, no verify)
  if (grid > kMaxGridCrc || a.c.slice_lo != 0 || a.c.slice_hi != a.c.s_full || !a.c.meta_out || !a.meta_host ||
      !a.c.part_crc || !a.dst ||
      (reinterpret_cast<uintptr_t>(a.c.data) | reinterpret_cast<uintptr_t>(a.dst) | reinterpret_cast<uintptr_t>(a.dst_host)) % 16)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(crc_write_copy_kernel, dim3(grid), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

hipError_t launch_scrub(const ScrubLaunch& a, const DevCrcTables* t, hipStream_t s) {
  if (a.nblocks == 0) return hipSuccess;
  const int ring = crc_mfma_enabled() ? crc_ring_buffers() : 0;
  const uint64_t cap = ring ? crc_grid_cap(ring) : 2048;
  uint64_t g = a.ntiles < cap ? a.ntiles : cap;
  uint64_t tail_waves = (a.nblocks + 3) / 4;
  if (g < tail_waves) g = tail_waves < cap ? tail_waves : cap;
  if (g == 0) g = 1;
  const dim3 grid(static_cast<unsigned>(g));
  switch (ring) {
    case 0: hipLaunchKernelGGL(crc_scrub_kernel, grid, dim3(kCrcWgThreads), 0, s, a, t); break;
    case 2: hipLaunchKernelGGL(crc_scrub_mfma_kernel, grid, dim3(kCrcWgThreads), 0, s, a, t); break;
    case 3:
      if (crc_fp4_enabled()) hipLaunchKernelGGL((crc_scrub_ring_kernel<3, true>), grid, dim3(kCrcWgThreads), 0, s, a, t);
      else hipLaunchKernelGGL((crc_scrub_ring_kernel<3, false>), grid, dim3(kCrcWgThreads), 0, s, a, t);
      break;
    default:
      if (crc_fp4_enabled()) hipLaunchKernelGGL((crc_scrub_ring_kernel<4, true>), grid, dim3(kCrcWgThreads), 0, s, a, t);
      else hipLaunchKernelGGL((crc_scrub_ring_kernel<4, false>), grid, dim3(kCrcWgThreads), 0, s, a, t);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_stream_read(const uint8_t* d, uint64_t n, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(stream_read_kernel, dim3(kStreamReadGrid), dim3(256), 0, s, reinterpret_cast<const uint4*>(d), n / 16,
                     out);
  return hipGetLastError();
}

void gf_nibble_tables(const uint8_t* mat, int rows, int k, uint32_t* out) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < k; ++c) {
      uint8_t coef = mat[r * k + c];
      uint8_t lo[16], hi[16];
      for (int v = 0; v < 16; ++v) {
        lo[v] = gf::mul(coef, static_cast<uint8_t>(v));
        hi[v] = gf::mul(coef, static_cast<uint8_t>(v << 4));
      }
      uint32_t* t = out + (r * k + c) * 8;
      std::memcpy(t, lo, 16);
      std::memcpy(t + 4, hi, 16);
    }
}

hipError_t launch_gf_matmul(const GfLaunch& a, hipStream_t s) {
  if (a.len == 0 || a.rows == 0) return hipSuccess;
  uint64_t nvec = (a.len + 15) / 16;
  uint64_t blocks = (nvec + 255) / 256;
  int grid = static_cast<int>(blocks < 2048 ? blocks : 2048);
  hipLaunchKernelGGL(gf256_matmul_kernel, dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

static std::atomic<int> g_ec_fused{-1};

void set_ec_fused(bool on) { g_ec_fused.store(on ? 1 : 0); }

bool ec_fused_enabled() {
  int v = g_ec_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_EC_FUSED");
    g_ec_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

int ec_fused_grid(uint64_t ntiles, uint32_t tail_len, int rows) {
  // one resident round: two workgroups per CU, one with four accumulator rows
  const uint64_t cap = rows < 4 ? kEcFusedMaxGrid : kEcFusedMaxGrid / 2;
  const uint64_t g = ntiles < cap ? ntiles : cap;
  return static_cast<int>(g == 0 && tail_len ? 1 : g);
}

hipError_t launch_ec_fused(const EcFusedLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  if (grid <= 0) return hipSuccess;
  static_assert(kEcFusedMaxGrid <= kMaxGridCrc, "part_crc holds kMaxGridCrc words per shard");
  const int nsh = (a.encode ? a.k : 0) + a.rows;
  if (grid > kMaxGridCrc || a.k <= 0 || a.k > kMaxShards || a.rows <= 0 || a.rows > kEcFusedMaxRows ||
      nsh > kMaxShards || !a.tables || !a.part_crc || !a.tail_be)
    return hipErrorInvalidValue;
  uintptr_t bits = reinterpret_cast<uintptr_t>(a.tables) | reinterpret_cast<uintptr_t>(a.part_crc) |
                   reinterpret_cast<uintptr_t>(a.tail_be);
  for (int c = 0; c < a.k; ++c) {
    if (!a.in[c] || (a.encode && !a.dst[c])) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(a.in[c]) | (a.encode ? reinterpret_cast<uintptr_t>(a.dst[c]) : 0);
  }
  for (int r = 0; r < a.rows; ++r) {
    if (!a.out[r]) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(a.out[r]);
  }
  for (int i = 0; i < nsh; ++i) {
    if (!a.meta[i]) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(a.meta[i]);
  }
  if (bits % 16) return hipErrorInvalidValue;
  const dim3 g(grid), b(kCrcWgThreads);
  switch (a.rows * 2 + (a.encode ? 1 : 0)) {
    case 2: hipLaunchKernelGGL((ec_fused_kernel<1, false>), g, b, 0, s, a, t); break;
    case 3: hipLaunchKernelGGL((ec_fused_kernel<1, true>), g, b, 0, s, a, t); break;
    case 4: hipLaunchKernelGGL((ec_fused_kernel<2, false>), g, b, 0, s, a, t); break;
    case 5: hipLaunchKernelGGL((ec_fused_kernel<2, true>), g, b, 0, s, a, t); break;
    case 6: hipLaunchKernelGGL((ec_fused_kernel<3, false>), g, b, 0, s, a, t); break;
    case 7: hipLaunchKernelGGL((ec_fused_kernel<3, true>), g, b, 0, s, a, t); break;
    case 8: hipLaunchKernelGGL((ec_fused_kernel<4, false>), g, b, 0, s, a, t); break;
    default: hipLaunchKernelGGL((ec_fused_kernel<4, true>), g, b, 0, s, a, t); break;
  }
  return hipGetLastError();
}

static std::atomic<int> g_ec_convert_fused{-1};

void set_ec_convert_fused(bool on) { g_ec_convert_fused.store(on ? 1 : 0); }

bool ec_convert_fused_enabled() {
  int v = g_ec_convert_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_EC_CONVERT_FUSED");
    g_ec_convert_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

int ec_convert_grid(uint64_t ntiles, uint32_t tail_len, int rows) {
  // one resident round: two workgroups per CU, one from three accumulator rows up
  const uint64_t cap = rows < 3 ? kEcFusedMaxGrid : kEcFusedMaxGrid / 2;
  const uint64_t g = ntiles < cap ? ntiles : cap;
  return static_cast<int>(g == 0 && tail_len ? 1 : g);
}

hipError_t launch_ec_convert(const EcConvertLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const EcFusedLaunch& f = a.f;
  if (grid <= 0 || grid > kMaxGridCrc || f.k <= 0 || f.rows <= 0 || f.rows > kEcFusedMaxRows ||
      f.k + f.rows > kMaxShards || a.n < 1 || a.sl != (a.n + f.k - 1) / f.k || !a.src || !f.tables || !f.part_crc ||
      !f.tail_be)
    return hipErrorInvalidValue;
  uintptr_t bits = reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(f.tables) |
                   reinterpret_cast<uintptr_t>(f.part_crc) | reinterpret_cast<uintptr_t>(f.tail_be);
  for (int c = 0; c < f.k; ++c) {
    if (!f.dst[c]) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(f.dst[c]);
  }
  for (int r = 0; r < f.rows; ++r) {
    if (!f.out[r]) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(f.out[r]);
  }
  for (int i = 0; i < f.k + f.rows; ++i) {
    if (!f.meta[i]) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(f.meta[i]);
  }
  if (bits % 16) return hipErrorInvalidValue;
  const dim3 g(grid), b(kCrcWgThreads);
  switch (f.rows) {
    case 1: hipLaunchKernelGGL((ec_convert_kernel<1>), g, b, 0, s, a, t); break;
    case 2: hipLaunchKernelGGL((ec_convert_kernel<2>), g, b, 0, s, a, t); break;
    case 3: hipLaunchKernelGGL((ec_convert_kernel<3>), g, b, 0, s, a, t); break;
    default: hipLaunchKernelGGL((ec_convert_kernel<4>), g, b, 0, s, a, t); break;
  }
  return hipGetLastError();
}

static std::atomic<int> g_ec_read_fused{-1};

void set_ec_read_fused(bool on) { g_ec_read_fused.store(on ? 1 : 0); }

bool ec_read_fused_enabled() {
  int v = g_ec_read_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_EC_READ_FUSED");
    g_ec_read_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

hipError_t launch_ec_read(const EcReadLaunch& in, hipStream_t s) {
  EcReadLaunch a = in;
  if (a.k <= 0 || a.k > kMaxShards || a.rows < 0 || a.rows > kEcFusedMaxRows || a.sl < kEcReadMinShard || a.want == 0 ||
      a.from + a.want > a.sl * a.k || !a.out || (a.rows && !a.tables))
    return hipErrorInvalidValue;
  uintptr_t bits = reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.tables);
  for (int j = 0; j < a.k; ++j) {
    if (!a.in[j] || a.surv_col[j] >= a.k) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(a.in[j]);
  }
  for (int r = 0; r < a.rows; ++r)
    if (a.row_col[r] < 0 || a.row_col[r] >= a.k) return hipErrorInvalidValue;
  if (bits % 16) return hipErrorInvalidValue;
  // The steps some column wants. Three or more columns: the middle ones want the whole shard.
  // Two: the tail of the first and the head of the second, which may leave a gap. One: its own.
  const uint64_t c0 = a.from / a.sl, c1 = (a.from + a.want - 1) / a.sl;
  const EcReadCol first = ec_read_col(a.sl, a.from, a.want, c0), last = ec_read_col(a.sl, a.from, a.want, c1);
  a.seg_begin[0] = a.seg_begin[1] = a.seg_steps[0] = a.seg_steps[1] = 0;
  if (c1 == c0 + 1 && last.last_step() + 1 < first.first_step()) {
    a.seg_steps[0] = last.last_step() + 1;
    a.seg_begin[1] = first.first_step();
    a.seg_steps[1] = first.last_step() + 1 - first.first_step();
  } else {
    a.seg_begin[0] = c1 > c0 ? 0 : first.first_step();
    a.seg_steps[0] = first.last_step() + 1 - a.seg_begin[0];  // the first column reaches the shard's end, or is the only one
  }
  // at least two steps per wave: a run's first step of a rebuilt column pays for the vector below it
  const uint64_t total = a.seg_steps[0] + a.seg_steps[1], want_wg = (total + 7) / 8;
  const dim3 g(static_cast<unsigned>(want_wg < static_cast<uint64_t>(kEcReadMaxGrid) ? want_wg : kEcReadMaxGrid)),
      b(kCrcWgThreads);
  switch (a.rows) {
    case 0: hipLaunchKernelGGL(ec_read_kernel<0>, g, b, 0, s, a); break;
    case 1: hipLaunchKernelGGL(ec_read_kernel<1>, g, b, 0, s, a); break;
    case 2: hipLaunchKernelGGL(ec_read_kernel<2>, g, b, 0, s, a); break;
    case 3: hipLaunchKernelGGL(ec_read_kernel<3>, g, b, 0, s, a); break;
    default: hipLaunchKernelGGL(ec_read_kernel<4>, g, b, 0, s, a); break;
  }
  return hipGetLastError();
}

static std::atomic<int> g_sse_fused{-1};

static std::atomic<int64_t> g_sse_min_bytes{-1};

void set_sse_fused(bool on, int64_t min_bytes) {
  g_sse_fused.store(on ? 1 : 0);
  if (min_bytes >= 0) g_sse_min_bytes.store(min_bytes);
}

uint64_t sse_fused_min_bytes() {
  int64_t v = g_sse_min_bytes.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_FUSED_MIN_BYTES");
    g_sse_min_bytes.store(v = e && std::atoll(e) >= 0 ? std::atoll(e) : static_cast<int64_t>(kSseFusedMinBytes));
  }
  return static_cast<uint64_t>(v);
}

bool sse_fused_enabled() {
  int v = g_sse_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_FUSED");
    g_sse_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

hipError_t launch_sse_gcm(const SseGcmLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const gcm::Plan p = gcm::plan_for(a.n);
  const uintptr_t src = reinterpret_cast<uintptr_t>(a.src), dst = reinterpret_cast<uintptr_t>(a.dst);
  if (!t || !a.src || !a.dst || !a.part || a.n == 0 || p.nblocks > 0xFFFFFFFEull || src % 4 || (dst - src) % 16 ||
      reinterpret_cast<uintptr_t>(a.part) % 16 || a.ntiles != p.ntiles || a.vfront != p.vfront || grid != p.grid)
    return hipErrorInvalidValue;
  if (src != dst && src < dst + a.n && dst < src + a.n) return hipErrorInvalidValue;  // in place or disjoint
  const dim3 g(static_cast<unsigned>(grid)), b(kCrcWgThreads);
  switch ((src & 15) >> 2) {
    case 0: hipLaunchKernelGGL(sse_gcm_kernel<0>, g, b, 0, s, a, t); break;
    case 1: hipLaunchKernelGGL(sse_gcm_kernel<1>, g, b, 0, s, a, t); break;
    case 2: hipLaunchKernelGGL(sse_gcm_kernel<2>, g, b, 0, s, a, t); break;
    default: hipLaunchKernelGGL(sse_gcm_kernel<3>, g, b, 0, s, a, t); break;
  }
  return hipGetLastError();
}

static std::atomic<int> g_sse_read_fused{-1};

static std::atomic<int64_t> g_sse_read_min_bytes{-1};

void set_sse_read_fused(bool on, int64_t min_bytes) {
  g_sse_read_fused.store(on ? 1 : 0);
  if (min_bytes >= 0) g_sse_read_min_bytes.store(min_bytes);
}

uint64_t sse_read_fused_min_bytes() {
  int64_t v = g_sse_read_min_bytes.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_READ_FUSED_MIN_BYTES");
    g_sse_read_min_bytes.store(v = e && std::atoll(e) >= 0 ? std::atoll(e) : static_cast<int64_t>(kSseReadFusedMinBytes));
  }
  return static_cast<uint64_t>(v);
}

bool sse_read_fused_enabled() {
  int v = g_sse_read_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_READ_FUSED");
    g_sse_read_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

hipError_t launch_sse_read(const SseReadLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const gcm::Plan p = gcm::plan_for(kSseReadTileBytes * sse_read_tiles(a.n));
  if (!t || !a.src || !a.meta || !a.out || !a.part || !a.part_bad || !a.nonce_tag || a.n == 0 ||
      p.nblocks > 0xFFFFFFFEull || reinterpret_cast<uintptr_t>(a.src) % 16 || reinterpret_cast<uintptr_t>(a.out) % 16 ||
      reinterpret_cast<uintptr_t>(a.part) % 16 || a.ntiles != p.ntiles || p.vfront != 0 || grid != p.grid)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sse_read_kernel, dim3(static_cast<unsigned>(grid)), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

hipError_t launch_sse_read_range(const SseReadRangeLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const SseReadLaunch& r = a.r;
  const gcm::Plan p = gcm::plan_for(kSseReadTileBytes * sse_read_tiles(r.n));
  if (!t || !r.src || !r.meta || !r.out || !r.part || !r.part_bad || !r.nonce_tag || r.n == 0 || a.want == 0 ||
      a.from > r.n || a.want > r.n - a.from || p.nblocks > 0xFFFFFFFEull || reinterpret_cast<uintptr_t>(r.src) % 16 ||
      (reinterpret_cast<uintptr_t>(r.out) - a.from) % 16 || reinterpret_cast<uintptr_t>(r.part) % 16 ||
      r.ntiles != p.ntiles || p.vfront != 0 || grid != p.grid)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sse_read_range_kernel, dim3(static_cast<unsigned>(grid)), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

static std::atomic<int> g_sse_write_fused{-1};
// -1 = DFS_SSE_WRITE_FUSED_MIN_BYTES, else kSseWriteFusedMinBytes
static std::atomic<int64_t> g_sse_write_min_bytes{-1};

void set_sse_write_fused(bool on, int64_t min_bytes) {
  g_sse_write_fused.store(on ? 1 : 0);
  if (min_bytes >= 0) g_sse_write_min_bytes.store(min_bytes);
}

void reset_sse_write_fused() {
  g_sse_write_fused.store(-1);
  g_sse_write_min_bytes.store(-1);
}

uint64_t sse_write_fused_min_bytes() {
  int64_t v = g_sse_write_min_bytes.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_WRITE_FUSED_MIN_BYTES");
    g_sse_write_min_bytes.store(v = e && std::atoll(e) >= 0 ? std::atoll(e) : static_cast<int64_t>(kSseWriteFusedMinBytes));
  }
  return static_cast<uint64_t>(v);
}

bool sse_write_fused_enabled(bool nvme_sync) {
  int v = g_sse_write_fused.load();
  if (v < 0) {  // 0 off, 1 on, 2 (nothing said): on where it measured faster
    const char* e = std::getenv("DFS_SSE_WRITE_FUSED");
    g_sse_write_fused.store(v = !e ? 2 : std::atoi(e) == 0 ? 0 : 1);
  }
  return v == 1 || (v == 2 && !nvme_sync);
}

hipError_t launch_sse_write(const SseWriteLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const gcm::Plan p = gcm::plan_for(kSseReadTileBytes * sse_read_tiles(a.n));
  if (!t || !a.buf || !a.dst || !a.meta || !a.meta_host || !a.part || !a.part_crc || a.n == 0 ||
      p.nblocks > 0xFFFFFFFEull || reinterpret_cast<uintptr_t>(a.buf) % 16 || reinterpret_cast<uintptr_t>(a.dst) % 16 ||
      reinterpret_cast<uintptr_t>(a.part) % 16 || a.ntiles != p.ntiles || p.vfront != 0 || grid != p.grid)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sse_write_kernel, dim3(static_cast<unsigned>(grid)), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

static std::atomic<int> g_sse_copy_fused{-1};
// -1 = DFS_SSE_COPY_FUSED_MIN_BYTES, else kSseCopyFusedMinBytes
static std::atomic<int64_t> g_sse_copy_min_bytes{-1};

void set_sse_copy_fused(bool on, int64_t min_bytes) {
  g_sse_copy_fused.store(on ? 1 : 0);
  if (min_bytes >= 0) g_sse_copy_min_bytes.store(min_bytes);
}

uint64_t sse_copy_fused_min_bytes() {
  int64_t v = g_sse_copy_min_bytes.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_COPY_FUSED_MIN_BYTES");
    g_sse_copy_min_bytes.store(v = e && std::atoll(e) >= 0 ? std::atoll(e) : static_cast<int64_t>(kSseCopyFusedMinBytes));
  }
  return static_cast<uint64_t>(v);
}

bool sse_copy_fused_enabled() {
  int v = g_sse_copy_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_COPY_FUSED");
    g_sse_copy_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

hipError_t launch_sse_rekey(const SseRekeyLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const gcm::Plan p = gcm::plan_for(kSseReadTileBytes * sse_read_tiles(a.n));
  const uintptr_t src = reinterpret_cast<uintptr_t>(a.src), dst = reinterpret_cast<uintptr_t>(a.dst);
  const uint64_t span = (a.n + 28 + 15) / 16 * 16;
  if (!t || !a.src || !a.src_meta || !a.dst || !a.meta || !a.meta_host || !a.from.part || !a.to.part || !a.part_bad ||
      !a.part_crc || !a.nonce_tag || !a.tail_host || reinterpret_cast<uintptr_t>(a.tail_host) % 16 || a.n == 0 || p.nblocks > 0xFFFFFFFEull || src % 16 || dst % 16 ||
      reinterpret_cast<uintptr_t>(a.from.part) % 16 || reinterpret_cast<uintptr_t>(a.to.part) % 16 ||
      a.ntiles != p.ntiles || p.vfront != 0 || grid != p.grid)
    return hipErrorInvalidValue;
  if (src < dst + span && dst < src + span) return hipErrorInvalidValue;  // two extents, never one in place
  hipLaunchKernelGGL(sse_rekey_kernel, dim3(static_cast<unsigned>(grid)), dim3(kCrcWgThreads), 0, s, a, t);
  return hipGetLastError();
}

static std::atomic<int> g_sse_ec_read_fused{-1};
// -1 = DFS_SSE_EC_READ_FUSED_MIN_BYTES, else kSseEcReadFusedMinBytes
static std::atomic<int64_t> g_sse_ec_read_min_bytes{-1};

void set_sse_ec_read_fused(bool on, int64_t min_bytes) {
  g_sse_ec_read_fused.store(on ? 1 : 0);
  if (min_bytes >= 0) g_sse_ec_read_min_bytes.store(min_bytes);
}

uint64_t sse_ec_read_fused_min_bytes() {
  int64_t v = g_sse_ec_read_min_bytes.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_EC_READ_FUSED_MIN_BYTES");
    g_sse_ec_read_min_bytes.store(v = e && std::atoll(e) >= 0 ? std::atoll(e) : static_cast<int64_t>(kSseEcReadFusedMinBytes));
  }
  return static_cast<uint64_t>(v);
}

bool sse_ec_read_fused_enabled() {
  int v = g_sse_ec_read_fused.load();
  if (v < 0) {
    const char* e = std::getenv("DFS_SSE_EC_READ_FUSED");
    g_sse_ec_read_fused.store(v = (e && std::atoi(e) == 0) ? 0 : 1);
  }
  return v != 0;
}

hipError_t launch_sse_ec_read(const SseEcReadLaunch& a, const DevCrcTables* t, int grid, hipStream_t s) {
  const gcm::Plan p = gcm::plan_for(kSseReadTileBytes * sse_read_tiles(a.n));
  if (!t || !a.out || !a.part || !a.nonce_tag || a.n == 0 || a.k <= 0 || a.k > kMaxShards || a.rows < 0 ||
      a.rows > kEcFusedMaxRows || a.sl < kSseEcReadMinShard || a.n + 28 > a.sl * a.k || (a.rows && !a.tables) ||
      p.nblocks > 0xFFFFFFFEull || a.ntiles != p.ntiles || p.vfront != 0 || grid != p.grid)
    return hipErrorInvalidValue;
  uintptr_t bits = reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.part) | reinterpret_cast<uintptr_t>(a.tables);
  uint32_t covered = 0;  // every data column is a survivor or a reconstruct row's, once
  for (int j = 0; j < a.k; ++j) {
    if (!a.in[j] || a.surv_col[j] >= a.k) return hipErrorInvalidValue;
    bits |= reinterpret_cast<uintptr_t>(a.in[j]);
    if (a.surv_col[j] >= 0) covered ^= 1u << a.surv_col[j];
  }
  for (int r = 0; r < a.rows; ++r) {
    if (a.row_col[r] < 0 || a.row_col[r] >= a.k) return hipErrorInvalidValue;
    covered ^= 1u << a.row_col[r];
  }
  if (bits % 16 || covered != (a.k >= 32 ? ~0u : (1u << a.k) - 1u)) return hipErrorInvalidValue;
  const dim3 g(static_cast<unsigned>(grid)), b(kCrcWgThreads);
  if (a.rows) hipLaunchKernelGGL(sse_ec_read_kernel<true>, g, b, 0, s, a, t);
  else hipLaunchKernelGGL(sse_ec_read_kernel<false>, g, b, 0, s, a, t);
  return hipGetLastError();
}

}  // namespace dfs
