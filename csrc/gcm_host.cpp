#include "gcm_host.h"

#include <openssl/crypto.h>
#include <openssl/evp.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace dfs::gcm {

namespace {
constexpr U128 kOne{0x8000000000000000ull, 0};  // x^0

uint8_t rotl8(uint8_t x, int s) { return static_cast<uint8_t>((x << s) | (x >> (8 - s))); }

AesTables make_tables() {
  AesTables t{};
  uint8_t p = 1, q = 1;  // p walks the multiplicative group by 3, q is its inverse
  do {
    p = static_cast<uint8_t>(p ^ (p << 1) ^ ((p & 0x80) ? 0x1B : 0));
    q ^= static_cast<uint8_t>(q << 1);
    q ^= static_cast<uint8_t>(q << 2);
    q ^= static_cast<uint8_t>(q << 4);
    if (q & 0x80) q ^= 0x09;
    t.sbox[p] = static_cast<uint8_t>(q ^ rotl8(q, 1) ^ rotl8(q, 2) ^ rotl8(q, 3) ^ rotl8(q, 4) ^ 0x63);
  } while (p != 1);
  t.sbox[0] = 0x63;
  for (int x = 0; x < 256; ++x) {
    const uint32_t s = t.sbox[x], s2 = ((s << 1) ^ ((s & 0x80) ? 0x11B : 0)) & 0xFF;
    t.te0[x] = s2 | s << 8 | s << 16 | (s2 ^ s) << 24;
  }
  return t;
}

uint32_t sub_word(uint32_t w) {
  const uint8_t* s = aes_tables().sbox;
  return static_cast<uint32_t>(s[w & 255]) | static_cast<uint32_t>(s[(w >> 8) & 255]) << 8 |
         static_cast<uint32_t>(s[(w >> 16) & 255]) << 16 | static_cast<uint32_t>(s[w >> 24]) << 24;
}

bool aes256_ecb_block(const uint8_t key[32], const uint8_t in[16], uint8_t out[16]) {
  EVP_CIPHER_CTX* c = EVP_CIPHER_CTX_new();
  int len = 0;
  const bool ok = c && EVP_EncryptInit_ex(c, EVP_aes_256_ecb(), nullptr, key, nullptr) &&
                  EVP_CIPHER_CTX_set_padding(c, 0) && EVP_EncryptUpdate(c, out, &len, in, 16) && len == 16;
  EVP_CIPHER_CTX_free(c);
  return ok;
}

U128 from_bytes(const uint8_t b[16]) {
  U128 v{0, 0};
  for (int i = 0; i < 8; ++i) {
    v.hi = v.hi << 8 | b[i];
    v.lo = v.lo << 8 | b[8 + i];
  }
  return v;
}

void to_bytes(U128 v, uint8_t b[16]) {
  for (int i = 0; i < 8; ++i) {
    b[i] = static_cast<uint8_t>(v.hi >> (56 - 8 * i));
    b[8 + i] = static_cast<uint8_t>(v.lo >> (56 - 8 * i));
  }
}

// Block `u` of the tile axis: zero in front of the message, zero-padded at its end.
U128 axis_block(const Plan& p, const uint8_t* data, uint64_t n, uint64_t u) {
  if (u < p.vfront) return U128{0, 0};
  const uint64_t off = (u - p.vfront) * 16;
  uint8_t b[16] = {0};
  std::memcpy(b, data + off, static_cast<size_t>(std::min<uint64_t>(16, n - off)));
  return from_bytes(b);
}

U128 close_ghash(const Keys& k, U128 folded, uint64_t n) {
  folded.lo ^= n * 8;  // len(A) = 0 || len(C) in bits
  return gf128_mul(k.h, folded);
}
}  // namespace

const AesTables& aes_tables() {
  static const AesTables t = make_tables();
  return t;
}

void wipe(void* p, size_t n) { OPENSSL_cleanse(p, n); }

Plan plan_for(uint64_t n, int grid_cap) {
  Plan p{};
  p.nblocks = (n + 15) / 16;
  p.ntiles = (p.nblocks + kGcmTileBlocks - 1) / kGcmTileBlocks;
  p.vfront = p.ntiles * kGcmTileBlocks - p.nblocks;
  const uint64_t cap = grid_cap > 0 ? static_cast<uint64_t>(grid_cap) : kGcmMaxGrid;
  p.grid = static_cast<int>(std::min(p.ntiles, cap));
  return p;
}

void aes256_expand_key(const uint8_t key[32], uint32_t rk[60]) {
  std::memcpy(rk, key, 32);  // little-endian words
  uint32_t rcon = 1;
  for (int i = 8; i < 60; ++i) {
    uint32_t t = rk[i - 1];
    if (i % 8 == 0) {
      t = sub_word((t >> 8) | (t << 24)) ^ rcon;
      rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x11B : 0)) & 0xFF;
    } else if (i % 8 == 4) {
      t = sub_word(t);
    }
    rk[i] = rk[i - 8] ^ t;
  }
}

U128 gf128_pow(U128 h, uint64_t e) {
  U128 r = kOne;
  for (; e; e >>= 1) {
    if (e & 1) r = gf128_mul(h, r);
    h = gf128_mul(h, h);
  }
  return r;
}

bool prepare(const uint8_t key[32], const uint8_t nonce[12], const Plan& p, Keys* k) {
  aes256_expand_key(key, k->rk);
  std::memcpy(k->nonce, nonce, 12);
  uint8_t blk[16] = {0}, out[16];
  if (!aes256_ecb_block(key, blk, out)) return false;
  k->h = from_bytes(out);
  std::memcpy(blk, nonce, 12);
  blk[15] = 1;
  if (!aes256_ecb_block(key, blk, k->ekj0)) return false;
  U128 t = gf128_pow(k->h, kGcmLaneBlocks);
  for (int s = 0; s < kGcmTreeSteps; ++s) {
    k->tree[s] = t;
    t = gf128_mul(t, t);
  }
  static_assert(kGcmTileBlocks == kGcmLaneBlocks << (kGcmTreeSteps + 1), "a tile is two more doublings of the tree");
  k->htile = gf128_mul(t, t);
  k->hjump = gf128_pow(k->h, static_cast<uint64_t>(kGcmTileBlocks) * std::max(p.grid, 1) - kGcmLaneBlocks);
  wipe(out, sizeof(out));
  return true;
}

bool prepare_keyed(const uint8_t key[32], const Plan& p, Keys* k) {
  const uint8_t none[12] = {0};
  if (!prepare(key, none, p, k)) return false;
  wipe(k->ekj0, sizeof(k->ekj0));  // of the zero nonce: nobody's
  return true;
}

bool set_nonce(const uint8_t key[32], const uint8_t nonce[12], Keys* k) {
  uint8_t blk[16] = {0};
  std::memcpy(k->nonce, nonce, 12);
  std::memcpy(blk, nonce, 12);
  blk[15] = 1;
  return aes256_ecb_block(key, blk, k->ekj0);
}

bool tag_matches(const Keys& k, U128 folded, uint64_t n, uint64_t vback, const uint8_t tag[16]) {
  uint8_t g[16];
  for (int i = 0; i < 16; ++i) g[i] = tag[i] ^ k.ekj0[i];
  const U128 want = from_bytes(g), len = gf128_mul(k.h, U128{0, n * 8});
  const U128 lhs = gf128_mul(k.h, folded);
  const U128 rhs = gf128_mul(gf128_pow(k.h, vback), U128{want.hi ^ len.hi, want.lo ^ len.lo});
  const bool ok = CRYPTO_memcmp(&lhs, &rhs, sizeof(lhs)) == 0;
  wipe(g, sizeof(g));
  return ok;
}

U128 unfold_factor(const Keys& k, uint64_t vback) {
  if (vback == 0) return kOne;
  // the exponent 2^128 - 1 - vback is the complement of vback: its high 64 bits are all ones
  U128 r = kOne, h = k.h;
  for (int i = 0; i < 128; ++i) {
    if (i >= 64 || ((~vback >> i) & 1)) r = gf128_mul(h, r);
    h = gf128_mul(h, h);
  }
  wipe(&h, sizeof(h));
  return r;
}

U128 write_jump(const Keys& k, const Plan& p) {
  return gf128_pow(k.h, static_cast<uint64_t>(kGcmTileBlocks) * std::max(p.grid, 1) - (kGcmLaneBlocks + 1));
}

void ghash_partials(const Keys& k, const Plan& p, const uint8_t* data, uint64_t n, U128* part) {
  constexpr int kLanes = kGcmTileBlocks / kGcmLaneBlocks;
  std::vector<U128> acc(kLanes);
  for (int w = 0; w < p.grid; ++w) {
    std::fill(acc.begin(), acc.end(), U128{0, 0});
    for (uint64_t tile = w; tile < p.ntiles; tile += p.grid)
      for (int t = 0; t < kLanes; ++t) {
        U128 a = tile == static_cast<uint64_t>(w) ? acc[t] : gf128_mul(k.hjump, acc[t]);
        for (int i = 0; i < kGcmLaneBlocks; ++i) {
          const U128 c = axis_block(p, data, n, tile * kGcmTileBlocks + t * kGcmLaneBlocks + i);
          a = gf128_mul(k.h, U128{a.hi ^ c.hi, a.lo ^ c.lo});
        }
        acc[t] = a;
      }
    // the log tree: inside a wave (64 lanes), then the four waves in order
    for (int s = 0; s < 6; ++s)
      for (int t = 0; t < kLanes; t += 2 << s) {
        const U128 l = gf128_mul(k.tree[s], acc[t]), r = acc[t + (1 << s)];
        acc[t] = U128{l.hi ^ r.hi, l.lo ^ r.lo};
      }
    U128 y = acc[0];
    for (int wave = 1; wave < 4; ++wave) {
      y = gf128_mul(k.tree[6], y);
      y = U128{y.hi ^ acc[wave * 64].hi, y.lo ^ acc[wave * 64].lo};
    }
    part[w] = y;
  }
}

U128 ghash_fold(const Keys& k, const Plan& p, const U128* part) {
  // the last `grid` tiles are the last tiles of `grid` different workgroups, in tile order
  U128 y{0, 0};
  for (uint64_t tile = p.ntiles - p.grid; tile < p.ntiles; ++tile) {
    y = gf128_mul(k.htile, y);
    const U128& w = part[tile % p.grid];
    y = U128{y.hi ^ w.hi, y.lo ^ w.lo};
  }
  return y;
}

void finish_tag(const Keys& k, U128 folded, uint64_t n, uint8_t tag[16]) {
  to_bytes(close_ghash(k, folded, n), tag);
  for (int i = 0; i < 16; ++i) tag[i] ^= k.ekj0[i];
}

bool ghash(const uint8_t key[32], const uint8_t* data, uint64_t n, int grid_cap, uint8_t out[16]) {
  const Plan p = plan_for(n, grid_cap);
  const uint8_t nonce[12] = {0};
  Keys k;
  if (!prepare(key, nonce, p, &k)) return false;
  std::vector<U128> part(static_cast<size_t>(p.grid));
  ghash_partials(k, p, data, n, part.data());
  to_bytes(close_ghash(k, p.grid ? ghash_fold(k, p, part.data()) : U128{0, 0}, n), out);
  wipe(&k, sizeof(k));
  return true;
}

}  // namespace dfs::gcm
