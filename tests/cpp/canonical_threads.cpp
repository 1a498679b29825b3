// The device conversions between wire v1 and canonical bytes (include/mpshuffle.h "canonical serialisation") from two host threads on
// ONE context, under ThreadSanitizer on the development emulator (kernel bodies as plain CPU loops, compiled WITHOUT OpenMP here so
// that every access is one the sanitizer follows; "device" memory is host memory there).
//   thread A serialises proofs (mp_proof_serialize_dev) -- of the shape (2, 3) and, every other round, wire bytes of the shape (3, 4), so
//            that the context's element table is rebuilt between the other thread's calls;
//   thread B deserialises proofs (mp_proof_deserialize_dev, every other round through mp_proofs_deserialize_batch).
// The library serialises the calls on the context's lock: every round gives the bytes and status words of the single-threaded run.
// Built and run by tests/test_canonical_dev_emu.py; exit code 0 and no "WARNING: ThreadSanitizer" on stderr = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "mpshuffle.h"

static const uint32_t M = 2, N_ = 3, B = 6, ROUNDS = 4;
#define CHECK(x)                                                                   \
  do {                                                                             \
    if (!(x)) {                                                                    \
      fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, mp_last_error()); \
      std::abort();                                                                \
    }                                                                              \
  } while (0)

struct Converted {
  std::vector<uint8_t> bytes;
  std::vector<int32_t> status;
  bool operator==(const Converted& o) const { return bytes == o.bytes && status == o.status; }
};

static Converted serialize(mp_ctx* ctx, uint32_t m, uint32_t n, const std::vector<uint8_t>& wire) {
  Converted r{std::vector<uint8_t>(B * mp_serialized_proof_size(MP_CURVE_STARK, m, n), 0x5A), std::vector<int32_t>(B, 0x5A5A5A5A)};
  CHECK(wire.size() == B * mp_proof_size_curve(MP_CURVE_STARK, m, n));
  CHECK(mp_proof_serialize_dev(ctx, m, n, B, wire.data(), r.bytes.data(), r.status.data()) == 0);
  CHECK(mp_sync(ctx) == 0);
  return r;
}
static Converted deserialize(mp_ctx* ctx, const std::vector<uint8_t>& canon, bool host_form) {
  Converted r{std::vector<uint8_t>(B * mp_proof_size_curve(MP_CURVE_STARK, M, N_), 0x5A), std::vector<int32_t>(B, 0x5A5A5A5A)};
  if (host_form) {
    CHECK(mp_proofs_deserialize_batch(ctx, M, N_, B, canon.data(), r.bytes.data(), r.status.data()) == 0);
  } else {
    CHECK(mp_proof_deserialize_dev(ctx, M, N_, B, canon.data(), r.bytes.data(), r.status.data()) == 0);
    CHECK(mp_sync(ctx) == 0);
  }
  return r;
}

int main() {
  mp_ctx* ctx = nullptr;
  mp_table* t = nullptr;
  CHECK(mp_ctx_create(MP_CURVE_STARK, 0, &ctx) == 0);
  const uint32_t cards = M * N_;
  std::vector<uint8_t> params(mp_params_size(N_)), more(mp_params_size(2 * cards * B));
  uint8_t seed[32];
  memset(seed, 7, 32);
  CHECK(mp_setup(ctx, M, N_, seed, params.data()) == 0);
  memset(seed, 9, 32);
  CHECK(mp_setup(ctx, M, 2 * cards * B, seed, more.data()) == 0);      // (2 cards B + 3 points: one key, the decks)
  CHECK(mp_table_create(ctx, M, N_, params.data(), more.data(), &t) == 0);
  std::vector<uint8_t> rho((size_t)B * cards * 32), seeds((size_t)B * 32);
  for (size_t i = 0; i < rho.size(); ++i) rho[i] = (uint8_t)((i * 37 + 11) & 0xFF);
  for (size_t i = 31; i < rho.size(); i += 32) rho[i] &= 3;
  for (size_t i = 0; i < seeds.size(); ++i) seeds[i] = (uint8_t)(i * 13 + 5);
  std::vector<uint32_t> perm((size_t)B * cards);
  for (uint32_t b = 0; b < B; ++b)
    for (uint32_t i = 0; i < cards; ++i) perm[b * cards + i] = (i * 5 + b) % cards;      // (5 and 6 coprime)
  const size_t psz = mp_proof_size(M, N_);
  std::vector<uint8_t> decks((size_t)B * cards * 128), proofs(B * psz);
  std::vector<int32_t> st(B, 55);
  CHECK(mp_shuffle_and_remask_batch(t, B, more.data() + 64, rho.data(), perm.data(), seeds.data(), decks.data(), proofs.data(), st.data()) == 0);
  for (int32_t v : st) CHECK(v == 0);

  // single-threaded: the device forms against the host forms, then the references of the threaded rounds
  const Converted canon = serialize(ctx, M, N_, proofs);
  const size_t csz = mp_serialized_proof_size(MP_CURVE_STARK, M, N_);
  for (uint32_t b = 0; b < B; ++b) {
    std::vector<uint8_t> one(csz), back(psz);
    CHECK(mp_proof_serialize(MP_CURVE_STARK, M, N_, proofs.data() + b * psz, one.data()) == 0);
    CHECK(memcmp(one.data(), canon.bytes.data() + b * csz, csz) == 0 && canon.status[b] == 0);
    CHECK(mp_proof_deserialize(MP_CURVE_STARK, M, N_, one.data(), csz, back.data()) == 0);
    CHECK(memcmp(back.data(), proofs.data() + b * psz, psz) == 0);
  }
  std::vector<uint8_t> damaged = canon.bytes;
  damaged[2 * csz] ^= 1;                                              // proof 2: the first Vec length
  const Converted wire = deserialize(ctx, damaged, false);
  for (uint32_t b = 0; b < B; ++b) CHECK(wire.status[b] == (b == 2 ? MP_ERR_BAD_ENCODING : 0));
  CHECK(wire.bytes == proofs);                                        // (a wrong length zeroes nothing)
  CHECK(deserialize(ctx, damaged, true) == wire);
  std::vector<uint8_t> other(B * mp_proof_size_curve(MP_CURVE_STARK, 3, 4));      // wire bytes of another shape: small coordinates, in range
  for (size_t i = 0; i < other.size(); ++i) other[i] = (i % 32) < 30 ? (uint8_t)(i * 29 + 3) : 0;
  const Converted other_canon = serialize(ctx, 3, 4, other);
  for (int32_t v : other_canon.status) CHECK(v == 0);

  std::thread a([&] {
    for (uint32_t r = 0; r < ROUNDS; ++r) {
      CHECK(serialize(ctx, M, N_, proofs) == canon);
      if (r & 1) CHECK(serialize(ctx, 3, 4, other) == other_canon);
    }
  });
  std::thread b([&] {
    for (uint32_t r = 0; r < ROUNDS; ++r) CHECK(deserialize(ctx, damaged, (r & 1) != 0) == wire);
  });
  a.join();
  b.join();
  mp_table_destroy(t);
  mp_ctx_destroy(ctx);
  printf("canonical threads ok\n");
  return 0;
}
