// AES-256-GCM pieces shared by the host and the SSE kernel (sse_gcm_kernel): the arithmetic
// that both sides must agree on is written once, as inline host/device functions, and
// everything the kernel needs prepared or finished lives in gcm_host.cpp.
//
// Conventions. AES state and round keys are four little-endian column words (byte r of word c
// is state row r, column c), so the keystream XORs straight onto little-endian data dwords;
// Te0[x] = 2S | S << 8 | S << 16 | 3S << 24 and the other three tables are byte rotates of it.
// A GHASH element is GCM's bit-reflected polynomial (SP 800-38D 6.3) held as two big-endian
// 64-bit halves: bit 63 of `hi` is the coefficient of x^0, R = 0xE1 || 0^120.
//
// The kernel's tile axis. A tile is kGcmTileBlocks 16 B blocks, a lane owns kGcmLaneBlocks
// consecutive ones. The message is right-aligned on the axis: `vfront` virtual zero blocks stand
// in front of it so that the last tile ends where the message does, which costs nothing (a zero
// block adds nothing to GHASH) and makes every workgroup partial an exact power of H away from
// the message's end. Workgroup w takes tiles w, w + grid, ...; its partial is
// sum C_i * H^(end of its last tile - i).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GCM_HD __host__ __device__ inline
#else
#define GCM_HD inline
#endif

namespace dfs::gcm {

constexpr int kGcmLaneBlocks = 4;                     // 64 B per lane
constexpr int kGcmWaveBlocks = 64 * kGcmLaneBlocks;   // 4 KiB per wave
constexpr int kGcmTileBlocks = 4 * kGcmWaveBlocks;    // 16 KiB per 256-thread workgroup
constexpr int kGcmMaxGrid = 512;                      // one resident round at 2 workgroups per CU
constexpr int kGcmTreeSteps = 7;                      // H^(4 * 2^s): 6 steps inside a wave, 1 wave span

struct U128 {
  uint64_t hi, lo;
};

GCM_HD uint32_t bswap32(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
GCM_HD uint32_t rotl32(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// A block's four little-endian dwords as a GHASH element.
GCM_HD U128 ghash_element(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
  return U128{(static_cast<uint64_t>(bswap32(d0)) << 32) | bswap32(d1),
              (static_cast<uint64_t>(bswap32(d2)) << 32) | bswap32(d3)};
}

// x * y in GF(2^128). x's bits are walked from x^0 up while y is multiplied by x each step; on the
// GPU the callers pass the wave-uniform power of H as `x`, so the test is a scalar branch.
GCM_HD U128 gf128_mul(U128 x, U128 y) {
  U128 z{0, 0};
  for (int half = 0; half < 2; ++half) {
    const uint64_t bits = half ? x.lo : x.hi;
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {
      if ((bits >> i) & 1u) {
        z.hi ^= y.hi;
        z.lo ^= y.lo;
      }
      const uint64_t carry = y.lo & 1u;
      y.lo = (y.lo >> 1) | (y.hi << 63);
      y.hi = (y.hi >> 1) ^ (carry ? 0xE100000000000000ull : 0ull);
    }
  }
  return z;
}

// NB AES-256 block encryptions (14 rounds), round by round so that the blocks' table lookups are
// in flight together. `te0` 256 words, `sbox` 256 bytes, `rk` the 60 round-key words; `s` holds the
// states, in and out.
template <int NB, class TE, class SB, class RK>
GCM_HD void aes256_encrypt_words(const TE& te0, const SB& sbox, const RK& rk, uint32_t (&s)[NB][4]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c) s[b][c] ^= rk[c];
#pragma unroll 1
  for (int r = 1; r < 14; ++r) {
    const uint32_t k0 = rk[4 * r], k1 = rk[4 * r + 1], k2 = rk[4 * r + 2], k3 = rk[4 * r + 3];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const uint32_t a0 = s[b][0], a1 = s[b][1], a2 = s[b][2], a3 = s[b][3];
      s[b][0] = te0[a0 & 255] ^ rotl32(te0[(a1 >> 8) & 255], 8) ^ rotl32(te0[(a2 >> 16) & 255], 16) ^
                rotl32(te0[a3 >> 24], 24) ^ k0;
      s[b][1] = te0[a1 & 255] ^ rotl32(te0[(a2 >> 8) & 255], 8) ^ rotl32(te0[(a3 >> 16) & 255], 16) ^
                rotl32(te0[a0 >> 24], 24) ^ k1;
      s[b][2] = te0[a2 & 255] ^ rotl32(te0[(a3 >> 8) & 255], 8) ^ rotl32(te0[(a0 >> 16) & 255], 16) ^
                rotl32(te0[a1 >> 24], 24) ^ k2;
      s[b][3] = te0[a3 & 255] ^ rotl32(te0[(a0 >> 8) & 255], 8) ^ rotl32(te0[(a1 >> 16) & 255], 16) ^
                rotl32(te0[a2 >> 24], 24) ^ k3;
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const uint32_t a[4] = {s[b][0], s[b][1], s[b][2], s[b][3]};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      s[b][c] = (static_cast<uint32_t>(sbox[a[c] & 255]) | static_cast<uint32_t>(sbox[(a[(c + 1) & 3] >> 8) & 255]) << 8 |
                 static_cast<uint32_t>(sbox[(a[(c + 2) & 3] >> 16) & 255]) << 16 |
                 static_cast<uint32_t>(sbox[a[(c + 3) & 3] >> 24]) << 24) ^ rk[56 + c];
  }
}

// The tables the kernel keeps in LDS, generated once (GF(2^8) inverse + affine map, FIPS 197 5.1.1).
struct AesTables {
  uint32_t te0[256];
  uint8_t sbox[256];
};
const AesTables& aes_tables();

// What one message needs on the device, and what finishes it on the host. Key material: wipe it.
struct Keys {
  uint32_t rk[60];             // AES-256 key schedule
  uint32_t nonce[3];           // counter block words 0..2; word 3 is bswap32(2 + block index)
  U128 h;                      // hash subkey E_K(0^128)
  U128 tree[kGcmTreeSteps];    // H^(kGcmLaneBlocks * 2^s)
  U128 htile;                  // H^kGcmTileBlocks: the host fold's step
  U128 hjump;                  // H^(kGcmTileBlocks * grid - kGcmLaneBlocks): a lane's step to its next tile
  uint8_t ekj0[16];            // E_K(nonce || 00000001)
};

struct Plan {
  uint64_t nblocks, ntiles, vfront;
  int grid;
};
// grid_cap 0: the kernel's (kGcmMaxGrid).
Plan plan_for(uint64_t n, int grid_cap = 0);

void aes256_expand_key(const uint8_t key[32], uint32_t rk[60]);
U128 gf128_pow(U128 h, uint64_t e);
// Everything in Keys. Single block encryptions go through OpenSSL; false if it refuses.
bool prepare(const uint8_t key[32], const uint8_t nonce[12], const Plan& p, Keys* k);
// For a message whose nonce the host learns only after the kernel ran (sse_read_kernel reads it
// from the stored blob): everything in Keys that needs the key alone; `nonce` and `ekj0` stay zero
// until set_nonce fills them.
bool prepare_keyed(const uint8_t key[32], const Plan& p, Keys* k);
bool set_nonce(const uint8_t key[32], const uint8_t nonce[12], Keys* k);
// Whether `tag` authenticates an n-byte message whose blocks were folded with `vback` zero blocks
// behind them, so that `folded` is the message's sum times H^vback. Zero blocks at the end do
// change GHASH and H has no cheap inverse, so the comparison is made one multiply further on, where
// both sides can be computed: folded * H == ((tag ^ E_K(J0)) ^ len * H) * H^vback. Constant time.
bool tag_matches(const Keys& k, U128 folded, uint64_t n, uint64_t vback, const uint8_t tag[16]);
// For a kernel that folds with `vback` zero blocks behind the message and must produce the tag
// (sse_write_kernel): unfold_factor is H^-vback, by Fermat H^(2^128 - 1 - vback), one square-and-
// multiply over a 128-bit exponent (some 250 multiplies, ~150 us measured, needing only the key: the caller
// computes it while the kernel runs), and unfold(folded, factor) the message's own sum, which
// finish_tag closes. vback == 0 costs nothing.
U128 unfold_factor(const Keys& k, uint64_t vback);
inline U128 unfold(U128 folded, U128 factor) { return gf128_mul(factor, folded); }
// sse_write_kernel's step between a lane's tiles: its chunk absorbs five elements, not four.
U128 write_jump(const Keys& k, const Plan& p);
// The workgroup partials as the kernel leaves them, computed on the host: [p.grid].
void ghash_partials(const Keys& k, const Plan& p, const uint8_t* data, uint64_t n, U128* part);
// Fold per-workgroup partials into sum C_i * H^(nblocks - i), close with the length block
// (no AAD, n bytes) and XOR E_K(J0): the tag.
U128 ghash_fold(const Keys& k, const Plan& p, const U128* part);
void finish_tag(const Keys& k, U128 folded, uint64_t n, uint8_t tag[16]);
// GHASH_H(data || pad || len block), H from `key`, through the tile cut and the fold above.
bool ghash(const uint8_t key[32], const uint8_t* data, uint64_t n, int grid_cap, uint8_t out[16]);
// Wipes without the compiler's leave to skip it.
void wipe(void* p, size_t n);

}  // namespace dfs::gcm
