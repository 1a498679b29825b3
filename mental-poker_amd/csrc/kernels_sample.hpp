// Secrets drawn on the device from seeds: masking factors with the permutation of a shuffle, or a player's secret key
// [REF examples/round.rs:265-266, examples/parameter_selection.rs:38-39, barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:123-130:
// `Fr::rand(rng)` / `sample_vector(rng, N)`, then `Permutation::new(rng, N)`].
// "mpshuffle secret stream v1" (include/mpshuffle.h), for seed[32], S scalars and a permutation of length P:
//   key  = BLAKE2s-256("mpshuffle secret stream v1" || seed)
//   rng  = ChaCha20Rng::from_seed(key)                       the word stream of hash.hpp, block counter from 0
//   s_k  = Fr::rand(rng), k = 0 .. S-1                       candidates of 8 words on FrStream's half-block grid
//   perm = [0 .. P-1]; for i = P-1 down to 1: j = rng.next_u64() % (i + 1); swap(perm[i], perm[j])
// The u64 draws follow directly behind the last candidate, low word first: they start at word 0 or at word 8 of a block.
// One lane = one seed.  The lane keeps its permutation in its own output row in HBM while it swaps: a row belongs to one lane (program
// order is all the ordering it needs), it is the only place that holds 4 096 entries for each of 64 lanes of a wave (16 KB a lane:
// the LDS of a CU holds ten such rows), and it is one code path for every length.  The 3 P scattered dword accesses of a 52-card row
// stay in L2 and are nothing against the ~60 ChaCha20 blocks of the lane, let alone the ~6.6 10^4 point operations of its proof.
#pragma once
#include "kernels_proto.hpp"

namespace mp {

constexpr char SAMPLE_TAG[] = "mpshuffle secret stream v1\0";      // 26 bytes (+ 2 of padding: word 6 is completed by the seed)
constexpr uint32_t SAMPLE_TAG_BYTES = 26;
static_assert(sizeof(SAMPLE_TAG) == SAMPLE_TAG_BYTES + 2, "the tag is 26 bytes");
constexpr uint32_t sample_tag_word(int i) {
  return (uint32_t)(uint8_t)SAMPLE_TAG[4 * i] | (uint32_t)(uint8_t)SAMPLE_TAG[4 * i + 1] << 8 | (uint32_t)(uint8_t)SAMPLE_TAG[4 * i + 2] << 16 |
         (uint32_t)(uint8_t)SAMPLE_TAG[4 * i + 3] << 24;
}
// key = BLAKE2s-256(tag || seed): 58 bytes, one block; the seed starts two bytes into word 6
MP_HD void sample_stream_key(const uint8_t* seed, uint32_t key[8]) {
  constexpr uint32_t T0 = sample_tag_word(0), T1 = sample_tag_word(1), T2 = sample_tag_word(2), T3 = sample_tag_word(3), T4 = sample_tag_word(4),
                     T5 = sample_tag_word(5), T6 = sample_tag_word(6);
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(seed);      // (4-byte aligned: API contract)
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = sw[i];
  uint32_t m[16];
  m[0] = T0; m[1] = T1; m[2] = T2; m[3] = T3; m[4] = T4; m[5] = T5;
  m[6] = T6 | (w[0] << 16);
#pragma unroll
  for (int i = 0; i < 7; ++i) m[7 + i] = (w[i] >> 16) | (w[i + 1] << 16);
  m[14] = w[7] >> 16;
  m[15] = 0;
  Blake2sState s;
  blake2s_init(s);
  blake2s_compress(s, m, SAMPLE_TAG_BYTES + 32, true);
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = s.h[i];
}

// (hi 2^32 + lo) % d for 1 <= d <= 4 096, the full 64-bit remainder in 32-bit steps: a remainder is below 2^12, so with 16 more bits
// behind it it is below 2^28
MP_HD uint32_t sample_mod_u64(uint32_t lo, uint32_t hi, uint32_t d) {
  uint32_t r = hi % d;
  r = ((r << 16) | (lo >> 16)) % d;
  return ((r << 16) | (lo & 0xFFFFu)) % d;
}

struct SampleArgs {
  const uint8_t* seeds;   // [lanes][32]
  uint8_t* scalars;       // [lanes][S] wire scalars (nullptr if S = 0)
  uint32_t* perms;        // [lanes][P] (nullptr if P = 0)
  uint32_t S, P;
};
template <class C>
MP_HD void body_sample_secrets(const SampleArgs& a, uint32_t b, uint32_t y) {
  typedef typename C::FrP R;
  uint32_t key[8];
  sample_stream_key(a.seeds + (size_t)b * 32, key);
  FrStream st;
  frstream_init(st, key);
  // the candidate loop of body_prove_init: a lane whose candidate is rejected keeps its index, so that no lane waits for the unluckiest
  // one of its wave at every scalar
  uint8_t* out = a.scalars + (size_t)b * a.S * 32;
  uint32_t got = 0;
  while (got < a.S) {
    Fe<R> v;
    if (frstream_try<R>(st, v)) {
      fe_to_wire<R>(v, out + (size_t)got * 32);
      ++got;
    }
  }
  if (a.P == 0) return;
  uint32_t* row = a.perms + (size_t)b * a.P;
  for (uint32_t i = 0; i < a.P; ++i) row[i] = i;
  // Fisher-Yates, a block of eight u64 at a time (no dynamic index into the block): `first` = the first u64 of the block in hand that
  // no candidate has taken -- 4 when the last candidate was the first half of its block, 8 (none) otherwise and before any block
  uint32_t first = st.half < 2 ? 4u * st.half : 8u;
  uint32_t i = a.P - 1;
  while (i >= 1) {
    if (first >= 8) {
      chacha20_block(st.key, st.counter, st.blk);
      st.counter++;
      first = 0;
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      if (k >= first && i >= 1) {
        const uint32_t j = sample_mod_u64(st.blk[2 * k], st.blk[2 * k + 1], i + 1);
        const uint32_t vi = row[i], vj = row[j];
        row[i] = vj;
        row[j] = vi;
        --i;
      }
    }
    first = 8;
  }
}
MP_KERNEL(k_sample_secrets, SampleArgs, body_sample_secrets)

// ---- key generation: the statement of a player's Schnorr proof, g = G (the public key is computed into slot a); the secret key comes
// from the sampler's output through k_load_scalars
struct KeygenStmtArgs {
  uint32_t* P;
  const uint32_t* fbpts;
  uint32_t g_slot, Bpad, g_base;
};
template <class C>
MP_HD void body_keygen_stmt(const KeygenStmtArgs& a, uint32_t b, uint32_t y) {
  st_aff<C>(a.P + p_off<C>(a.g_slot, a.Bpad, b), ld_aff<C>(a.fbpts + (size_t)a.g_base * Geo<C>::PW));
}
MP_KERNEL(k_keygen_stmt, KeygenStmtArgs, body_keygen_stmt)

}  // namespace mp
