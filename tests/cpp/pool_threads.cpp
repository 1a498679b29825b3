// The device pool (mp_pool_*, include/mpshuffle.h): batches cut into contiguous blocks over several contexts.
//   pool_threads tsan     STARK m = 2, n = 3 on the development emulator under ThreadSanitizer (tests/test_pool_tsan.py)
//   pool_threads gpu      the same scenario against libmpshuffle.so (tests/test_gpu_pool.py)
// Pool {0, 0, 0} (three lanes of device 0), 8-bit tables.  B = 7, 3, 2 and 1, with the table's key and with a key per proof on a keyless
// pool table: bytes and status words equal the same call on one mp_table, a tampered proof, a non-permutation and an off-curve card
// included; members used and blocks as documented; one fixed-base build for the three lanes.  Two caller threads on the pool while a third
// calls a borrowed member table directly, a setter and the stats getters.  Pools created and destroyed in a loop; a member build that
// fails (m = 1) and the argument errors of mp_pool_create give their codes and name the member.  include/barnett_smart.hpp with a device
// list gives the bytes and status words of the same members on one context.
// Exit code 0 and "pool ok" on stdout = pass.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "barnett_smart.hpp"
#include "mpshuffle.h"

#define CHECK(x)                                                                            \
  do {                                                                                      \
    if (!(x)) {                                                                             \
      fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, mp_last_error()); \
      std::abort();                                                                         \
    }                                                                                       \
  } while (0)

static const uint32_t M = 2, N_ = 3, N = M * N_, R = 7;
static const size_t DSZ = (size_t)N * 128;

struct Case {
  size_t psz;
  std::vector<uint8_t> params, keys, decks, rho, seeds, pkeys;     // keys: 4 points (key 0 = the keyed tables'); pkeys: key 1 + r % 3 per request
  std::vector<uint32_t> perm;
};

static Case make_case(mp_ctx* ctx) {
  Case c;
  c.psz = mp_proof_size(M, N_);
  c.params.resize(mp_params_size(N_));
  uint8_t seed[32];
  memset(seed, 7, 32);
  CHECK(mp_setup(ctx, M, N_, seed, c.params.data()) == 0);
  // 4 keys and R decks of independent points
  const uint32_t pts = 4 + 2 * N * R;
  std::vector<uint8_t> more(mp_params_size(pts - 3));
  memset(seed, 9, 32);
  CHECK(mp_setup(ctx, M, pts - 3, seed, more.data()) == 0);
  c.keys.assign(more.begin(), more.begin() + 4 * 64);
  c.decks.assign(more.begin() + 4 * 64, more.begin() + 4 * 64 + R * DSZ);
  c.rho.resize((size_t)R * N * 32);
  for (size_t i = 0; i < c.rho.size(); ++i) c.rho[i] = (uint8_t)((i * 37 + 11 + i / 4096) & 0xFF);
  for (size_t i = 31; i < c.rho.size(); i += 32) c.rho[i] &= 3;
  c.perm.resize((size_t)R * N);
  for (uint32_t r = 0; r < R; ++r)
    for (uint32_t i = 0; i < N; ++i) c.perm[(size_t)r * N + i] = (r & 1 ? N - 1 - (i + r) % N : (i + r) % N);
  c.seeds.resize((size_t)R * 32);
  for (size_t i = 0; i < c.seeds.size(); ++i) c.seeds[i] = (uint8_t)(i * 13 + 5 + i / 251);
  c.pkeys.resize((size_t)R * 64);
  for (uint32_t r = 0; r < R; ++r) memcpy(&c.pkeys[r * 64], &c.keys[(1 + r % 3) * 64], 64);
  return c;
}

struct Out {
  std::vector<uint8_t> d, p;
  std::vector<int32_t> st;
  int rc = 0;
  explicit Out(const Case& c, size_t B) : d(B * DSZ, 0xAB), p(B * c.psz, 0xCD), st(B, 55) {}
  bool operator==(const Out& o) const { return rc == o.rc && d == o.d && p == o.p && st == o.st; }
};

// prove B requests on one table (t) or through the pool (pt); keys: per-proof keys or NULL
static Out prove(const Case& c, mp_table* t, mp_pool_table* pt, size_t B, const uint8_t* keys, const uint8_t* decks = nullptr,
                 const uint32_t* perm = nullptr) {
  Out o(c, B);
  if (!decks) decks = c.decks.data();
  if (!perm) perm = c.perm.data();
  if (pt)
    o.rc = mp_pool_shuffle_and_remask_batch(pt, B, keys, decks, c.rho.data(), perm, c.seeds.data(), o.d.data(), o.p.data(), o.st.data());
  else if (keys)
    o.rc = mp_shuffle_and_remask_batch_keys(t, B, keys, decks, c.rho.data(), perm, c.seeds.data(), o.d.data(), o.p.data(), o.st.data());
  else
    o.rc = mp_shuffle_and_remask_batch(t, B, decks, c.rho.data(), perm, c.seeds.data(), o.d.data(), o.p.data(), o.st.data());
  return o;
}
static std::vector<int32_t> verify(const Case& c, mp_table* t, mp_pool_table* pt, size_t B, const uint8_t* keys, const uint8_t* shuf,
                                   const uint8_t* proofs) {
  std::vector<int32_t> st(B, 55);
  int rc;
  if (pt)
    rc = mp_pool_verify_shuffle_batch(pt, B, keys, c.decks.data(), shuf, proofs, st.data());
  else if (keys)
    rc = mp_verify_shuffle_batch_keys(t, B, keys, c.decks.data(), shuf, proofs, st.data());
  else
    rc = mp_verify_shuffle_batch(t, B, c.decks.data(), shuf, proofs, st.data());
  CHECK(rc == 0);
  return st;
}

static int run(bool gpu) {
  const int lanes[3] = {0, 0, 0};
  uint64_t v[8], mv[4];
  // ---- argument errors of mp_pool_create: nothing is created, the member is named
  mp_pool* p = nullptr;
  CHECK(mp_pool_create(MP_CURVE_STARK, 0, lanes, &p) == MP_ERR_BAD_ARGUMENT && !p);
  CHECK(mp_pool_create(MP_CURVE_STARK, 65, nullptr, &p) == MP_ERR_BAD_ARGUMENT && !p);
  const int nodev[2] = {0, 99};
  CHECK(mp_pool_create(MP_CURVE_STARK, 2, nodev, &p) == MP_ERR_NO_DEVICE && !p);
  CHECK(strstr(mp_last_error(), "member 1 (device 99)"));
  // ---- create and destroy in a loop (with and without tables)
  for (int it = 0; it < 3; ++it) {
    CHECK(mp_pool_create(MP_CURVE_STARK, 3, lanes, &p) == 0 && mp_pool_size(p) == 3);
    CHECK(mp_pool_member_ctx(p, 2) && !mp_pool_member_ctx(p, 3));
    if (it == 1) {
      const Case c0 = make_case(mp_pool_member_ctx(p, 1));
      mp_pool_table* x = nullptr;
      CHECK(mp_pool_table_create(p, M, N_, c0.params.data(), nullptr, 8, &x) == 0);
      mp_pool_table_destroy(x);
    }
    mp_pool_destroy(p);
    p = nullptr;
  }

  CHECK(mp_pool_create(MP_CURVE_STARK, 3, lanes, &p) == 0);
  mp_ctx* ctx = nullptr;
  CHECK(mp_ctx_create(MP_CURVE_STARK, 0, &ctx) == 0);
  const Case c = make_case(ctx);
  mp_table *t = nullptr, *tp = nullptr;
  CHECK(mp_table_create_ex(ctx, M, N_, c.params.data(), c.keys.data(), 8, &t) == 0);
  CHECK(mp_table_create_params(ctx, M, N_, c.params.data(), 8, &tp) == 0);
  // ---- a member build that fails leaves nothing behind: the call's code and the member's name, no handle
  mp_pool_table* pt = nullptr;
  CHECK(mp_pool_table_create(p, 1, N_, c.params.data(), c.keys.data(), 8, &pt) == MP_ERR_BAD_ARGUMENT && !pt);
  CHECK(strstr(mp_last_error(), "member 0 (device 0)"));
  std::vector<uint8_t> badparams(c.params);
  badparams[64 + 32] ^= 1;      // ck_0 off the curve
  CHECK(mp_pool_table_create(p, M, N_, badparams.data(), c.keys.data(), 8, &pt) == MP_ERR_BAD_ENCODING && !pt);
  mp_pool_table* ptl = nullptr;
  CHECK(mp_pool_table_create(p, M, N_, c.params.data(), c.keys.data(), 8, &pt) == 0);
  CHECK(mp_pool_table_create(p, M, N_, c.params.data(), nullptr, 8, &ptl) == 0);
  CHECK(mp_pool_stats(pt, v) == 0 && v[0] == 0 && v[3] == 1 && v[4] == 3 && v[5] == 0 && v[6] == 0 && v[7] == 0);
  for (size_t i = 0; i < 3; ++i) CHECK(mp_pool_table_member(pt, i) && mp_table_window_bits(mp_pool_table_member(pt, i)) == 8);
  CHECK(!mp_pool_table_member(pt, 3));

  // ---- B = 7, 3, 2, 1: bytes and status words of the single-table call, with the table's key and with a key per proof
  const size_t used[4] = {3, 3, 2, 1}, sizes[4] = {7, 3, 2, 1};
  Out full(c, R), fullk(c, R);
  for (int k = 0; k < 4; ++k) {
    const size_t B = sizes[k];
    const Out a = prove(c, t, nullptr, B, nullptr), b = prove(c, nullptr, pt, B, nullptr);
    CHECK(a.rc == 0 && a == b);
    for (int32_t s : b.st) CHECK(s == 0);
    CHECK(mp_pool_stats(pt, v) == 0 && v[2] == used[k]);
    const Out ak = prove(c, tp, nullptr, B, c.pkeys.data()), bk = prove(c, nullptr, ptl, B, c.pkeys.data());
    CHECK(ak.rc == 0 && ak == bk);
    CHECK(mp_pool_stats(ptl, v) == 0 && v[2] == used[k]);
    CHECK(verify(c, t, nullptr, B, nullptr, a.d.data(), a.p.data()) == verify(c, nullptr, pt, B, nullptr, b.d.data(), b.p.data()));
    CHECK(verify(c, nullptr, ptl, B, c.pkeys.data(), bk.d.data(), bk.p.data()) == std::vector<int32_t>(B, 0));
    if (B == R) full = a, fullk = ak;
  }
  CHECK(mp_pool_stats(pt, v) == 0 && v[0] == 8 && v[1] == 2 * 13);
  CHECK(mp_pool_member_stats(pt, 0, mv) == 0 && mv[0] == 0 && mv[1] == 8 && mv[2] == 2 * (3 + 1 + 1 + 1));      // blocks 3/2/2, 1/1/1, 1/1, 1
  CHECK(mp_pool_member_stats(pt, 2, mv) == 0 && mv[1] == 4 && mv[2] == 2 * (2 + 1));
  CHECK(mp_pool_member_stats(pt, 3, mv) == MP_ERR_BAD_ARGUMENT);
  // min_shard: blocks of at least 3 proofs -> 7 proofs take 2 members; same bytes
  CHECK(mp_pool_set_min_shard(pt, 3) == 0 && mp_pool_set_min_shard(pt, 0) == MP_ERR_BAD_ARGUMENT);
  CHECK(prove(c, nullptr, pt, R, nullptr) == full);
  CHECK(mp_pool_stats(pt, v) == 0 && v[2] == 2);
  CHECK(mp_pool_set_min_shard(pt, 1) == 0);
  // ---- status words: a tampered proof, a swapped deck and the wrong key in a verify call; a non-permutation and an off-curve card in a
  // prove call -- at the first and last proof of blocks 3/2/2
  {
    std::vector<uint8_t> shuf(full.d), proofs(full.p);
    proofs[2 * c.psz + c.psz - 31] ^= 2;                                        // proof 2: a response scalar
    memcpy(&shuf[3 * DSZ], &full.d[4 * DSZ], DSZ);                              // proof 3: another proof's deck
    proofs[6 * c.psz + 32] ^= 1;                                                // proof 6: y of its first point
    const std::vector<int32_t> a = verify(c, t, nullptr, R, nullptr, shuf.data(), proofs.data());
    CHECK(a == verify(c, nullptr, pt, R, nullptr, shuf.data(), proofs.data()));
    CHECK(a[0] == 0 && a[1] == 0 && a[2] > 0 && a[3] > 0 && a[4] == 0 && a[5] == 0 && a[6] < 0);
    CHECK(verify(c, tp, nullptr, R, c.pkeys.data(), full.d.data(), full.p.data()) ==
          verify(c, nullptr, ptl, R, c.pkeys.data(), full.d.data(), full.p.data()));      // (made under key 0: every one rejected)
    std::vector<uint32_t> perm(c.perm);
    perm[4 * N + 1] = perm[4 * N];                                              // proof 4: not a permutation
    std::vector<uint8_t> decks(c.decks);
    decks[5 * DSZ + 128 + 32] ^= 1;                                             // proof 5: card 1 off the curve
    const Out pa = prove(c, t, nullptr, R, nullptr, decks.data(), perm.data()), pb = prove(c, nullptr, pt, R, nullptr, decks.data(), perm.data());
    CHECK(pa.rc == 0 && pa == pb && pa.st[4] == MP_ERR_BAD_PERMUTATION && pa.st[5] == MP_ERR_BAD_ENCODING && pa.st[3] == 0 && pa.st[6] == 0);
  }
  // ---- call-level errors: the single-table call's code, before anything is dispatched
  {
    Out o(c, R);
    CHECK(mp_pool_stats(pt, v) == 0);
    const uint64_t calls = v[0];
    const int a = mp_shuffle_and_remask_batch(t, R, nullptr, c.rho.data(), c.perm.data(), c.seeds.data(), o.d.data(), o.p.data(), o.st.data());
    const std::string ta = mp_last_error();
    CHECK(a < 0 && mp_pool_shuffle_and_remask_batch(pt, R, nullptr, nullptr, c.rho.data(), c.perm.data(), c.seeds.data(), o.d.data(), o.p.data(), o.st.data()) == a);
    CHECK(ta == mp_last_error());
    const int b = mp_shuffle_and_remask_batch(tp, R, c.decks.data(), c.rho.data(), c.perm.data(), c.seeds.data(), o.d.data(), o.p.data(), o.st.data());
    CHECK(b < 0 && mp_pool_shuffle_and_remask_batch(ptl, R, nullptr, c.decks.data(), c.rho.data(), c.perm.data(), c.seeds.data(), o.d.data(), o.p.data(), o.st.data()) == b);
    const int d = mp_verify_shuffle_batch(tp, R, c.decks.data(), full.d.data(), full.p.data(), o.st.data());
    CHECK(d < 0 && mp_pool_verify_shuffle_batch(ptl, R, nullptr, c.decks.data(), full.d.data(), full.p.data(), o.st.data()) == d);
    CHECK(mp_pool_verify_shuffle_batch(pt, 0, nullptr, c.decks.data(), full.d.data(), full.p.data(), o.st.data()) ==
          mp_verify_shuffle_batch(t, 0, c.decks.data(), full.d.data(), full.p.data(), o.st.data()));
    CHECK(mp_pool_stats(pt, v) == 0 && v[0] == calls);
  }
  // ---- two caller threads on the pool; a third on a borrowed member table, a setter and the stats getters
  {
    const int iters = gpu ? 6 : 2;
    std::atomic<int> running{2};
    auto caller = [&](bool keyed) {
      for (int it = 0; it < iters; ++it) {
        const Out o = prove(c, nullptr, keyed ? ptl : pt, R, keyed ? c.pkeys.data() : nullptr);
        CHECK(o == (keyed ? fullk : full));
        const Out o2 = prove(c, nullptr, pt, 3, nullptr);
        CHECK(o2.rc == 0 && memcmp(o2.d.data(), full.d.data(), 3 * DSZ) == 0 && memcmp(o2.p.data(), full.p.data(), 3 * c.psz) == 0);
        CHECK(verify(c, nullptr, pt, R, nullptr, full.d.data(), full.p.data()) == std::vector<int32_t>(R, 0));
      }
      --running;
    };
    std::thread a(caller, false), b(caller, true);
    std::thread direct([&] {
      uint64_t w[8], mw[4];
      mp_table* m1 = mp_pool_table_member(pt, 1);
      do {
        const Out o = prove(c, m1, nullptr, 2, nullptr);
        CHECK(o.rc == 0 && memcmp(o.d.data(), full.d.data(), 2 * DSZ) == 0 && memcmp(o.p.data(), full.p.data(), 2 * c.psz) == 0);
        CHECK(mp_set_io_chunk(m1, 0) == 0);
        CHECK(mp_pool_stats(pt, w) == 0 && mp_pool_stats(ptl, w) == 0 && mp_pool_member_stats(pt, 1, mw) == 0 && mw[0] == 0);
      } while (running.load() > 0);
    });
    a.join();
    b.join();
    direct.join();
  }
  // ---- include/barnett_smart.hpp: the device-list constructor routes the batch members through a pool; same bytes, same status words
  {
    namespace bs = barnett_smart;
    bs::DLCards one(MP_CURVE_STARK, 0), two(MP_CURVE_STARK, std::vector<int>{0, 0});
    bs::Parameters pp;
    pp.m = M, pp.n = N_, pp.raw = c.params;
    bs::PublicKey pk;
    memcpy(pk.data(), c.keys.data(), 64);
    const size_t B = 3;
    std::vector<std::array<uint8_t, 32>> seeds(B);
    std::vector<std::vector<bs::MaskedCard>> decks(B, std::vector<bs::MaskedCard>(N));
    std::vector<std::vector<bs::Scalar>> rho(B, std::vector<bs::Scalar>(N));
    std::vector<bs::Permutation> perms(B);
    for (size_t b = 0; b < B; ++b) {
      memcpy(seeds[b].data(), &c.seeds[b * 32], 32);
      memcpy(decks[b][0].data(), &c.decks[b * DSZ], DSZ);
      memcpy(rho[b][0].data(), &c.rho[b * N * 32], N * 32);
      perms[b].mapping.assign(c.perm.begin() + b * N, c.perm.begin() + (b + 1) * N);
    }
    const auto a = one.shuffle_and_remask_batch(seeds, pp, pk, decks, rho, perms), b = two.shuffle_and_remask_batch(seeds, pp, pk, decks, rho, perms);
    CHECK(two.pool_table() && !one.pool_table() && a.decks == b.decks && a.proofs == b.proofs && a.status == b.status);
    CHECK(memcmp(b.proofs[2].data(), &full.p[2 * c.psz], c.psz) == 0 && memcmp(b.decks[2][0].data(), &full.d[2 * DSZ], DSZ) == 0);
    std::vector<bs::ZKProofShuffle> pf(b.proofs);
    pf[1][c.psz - 31] ^= 2;
    const std::vector<int32_t> va = one.verify_shuffle_batch(pp, pk, decks, a.decks, pf), vb = two.verify_shuffle_batch(pp, pk, decks, b.decks, pf);
    CHECK(va == vb && va[0] == 0 && va[1] > 0 && va[2] == 0);
    two.verify_shuffle(pp, pk, decks[0], b.decks[0], b.proofs[0]);      // a single-proof member: member 0's table
    CHECK(mp_pool_stats(two.pool_table(), v) == 0 && v[0] == 2 && v[2] == 2);
  }
  mp_pool_table_destroy(ptl);
  mp_pool_table_destroy(pt);
  mp_pool_destroy(p);
  mp_table_destroy(tp);
  mp_table_destroy(t);
  mp_ctx_destroy(ctx);
  printf("pool ok\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "tsan";
  if (mode == "tsan") return run(false);
  if (mode == "gpu") return run(true);
  fprintf(stderr, "usage: pool_threads tsan | gpu\n");
  return 2;
}
