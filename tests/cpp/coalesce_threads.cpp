// Coalescing of the single-proof entry points (mp_set_coalesce, include/mpshuffle.h) from many host threads.
//   coalesce_threads tsan             STARK m = 2, n = 3 on the development emulator under ThreadSanitizer (tests/test_coalesce_tsan.py):
//                                     8 threads released by one barrier on one table -- same bytes as the single-threaded uncoalesced run,
//                                     at most 2 batched calls per queue; a tampered proof and two malformed prove requests inside batches
//                                     get exactly their own uncoalesced results; keyed calls on a keyless table; a lone caller; settings
//                                     changed while calls are queued; a third thread calling setters and getters throughout.
//   coalesce_threads gpu T ROUNDS [m n]   T threads, each ROUNDS x (mp_shuffle_and_remask + mp_verify_shuffle) on one table with
//                                     coalescing (max_batch = T, 1 000 us): bytes equal the batched call's; prints one JSON line with the
//                                     rate (proofs proved and verified per second) and the coalescing counters (tests/test_gpu_coalesce.py,
//                                     tools/coalesce_rate.py).
// Exit code 0 and "coalesce ok" on stdout = pass.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mpshuffle.h"

#define CHECK(x)                                                                            \
  do {                                                                                      \
    if (!(x)) {                                                                             \
      fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #x, mp_last_error()); \
      std::abort();                                                                         \
    }                                                                                       \
  } while (0)

struct Barrier {
  std::mutex mu;
  std::condition_variable cv;
  size_t n, waiting = 0, gen = 0;
  explicit Barrier(size_t k) : n(k) {}
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    const size_t g = gen;
    if (++waiting == n) {
      waiting = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
};

struct Case {
  uint32_t m, n, N, R;               // R requests
  size_t dsz, psz;
  std::vector<uint8_t> params, keys, decks, rho, seeds;     // keys: 4 points (key 0 = the keyed table's)
  std::vector<uint32_t> perm;
  const uint8_t* key(int k) const { return keys.data() + (size_t)k * 64; }
  const uint8_t* deck(int r) const { return decks.data() + (size_t)r * dsz; }
  const uint8_t* rh(int r) const { return rho.data() + (size_t)r * N * 32; }
  const uint32_t* pm(int r) const { return perm.data() + (size_t)r * N; }
  const uint8_t* seed(int r) const { return seeds.data() + (size_t)r * 32; }
};

static Case make_case(mp_ctx* ctx, uint32_t m, uint32_t n, uint32_t R) {
  Case c;
  c.m = m, c.n = n, c.N = m * n, c.R = R;
  c.dsz = (size_t)c.N * 128;
  c.psz = mp_proof_size(m, n);
  c.params.resize(mp_params_size(n));
  uint8_t seed[32];
  memset(seed, 7, 32);
  CHECK(mp_setup(ctx, m, n, seed, c.params.data()) == 0);
  // 4 keys and D distinct decks from independent points; request r takes deck r % D
  const uint32_t D = R < 8 ? R : 8;
  std::vector<uint8_t> more(mp_params_size(4 + 2 * c.N * D - 3));
  memset(seed, 9, 32);
  CHECK(mp_setup(ctx, m, 4 + 2 * c.N * D - 3, seed, more.data()) == 0);
  c.keys.assign(more.begin(), more.begin() + 4 * 64);
  c.decks.resize((size_t)R * c.dsz);
  for (uint32_t r = 0; r < R; ++r) memcpy(c.decks.data() + (size_t)r * c.dsz, more.data() + 4 * 64 + (size_t)(r % D) * c.dsz, c.dsz);
  c.rho.resize((size_t)R * c.N * 32);
  for (size_t i = 0; i < c.rho.size(); ++i) c.rho[i] = (uint8_t)((i * 37 + 11 + i / 4096) & 0xFF);
  for (size_t i = 31; i < c.rho.size(); i += 32) c.rho[i] &= 3;
  c.perm.resize((size_t)R * c.N);
  for (uint32_t r = 0; r < R; ++r)                                  // a rotation composed with a reflection, different per request
    for (uint32_t i = 0; i < c.N; ++i) c.perm[(size_t)r * c.N + i] = (r & 1 ? c.N - 1 - (i + r) % c.N : (i + r) % c.N);
  c.seeds.resize((size_t)R * 32);
  for (size_t i = 0; i < c.seeds.size(); ++i) c.seeds[i] = (uint8_t)(i * 13 + 5 + i / 251);
  return c;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void stats(const mp_table* t, uint64_t v[8]) { CHECK(mp_coalesce_stats(t, v) == 0); }

// ---------------------------------------------------------------------------------------------------------------------------------------
static int run_tsan() {
  const uint32_t T = 8;
  mp_ctx* ctx = nullptr;
  CHECK(mp_ctx_create(MP_CURVE_STARK, 0, &ctx) == 0);
  const Case c = make_case(ctx, 2, 3, T);
  mp_table *t = nullptr, *tp = nullptr;
  CHECK(mp_table_create_ex(ctx, c.m, c.n, c.params.data(), c.key(0), 8, &t) == 0);
  CHECK(mp_table_create_params(ctx, c.m, c.n, c.params.data(), 8, &tp) == 0);
  mp_table* tk[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; ++k) CHECK(mp_table_create_ex(ctx, c.m, c.n, c.params.data(), c.key(1 + k), 8, &tk[k]) == 0);

  // single-threaded, uncoalesced references
  std::vector<uint8_t> ref_d(T * c.dsz), ref_p(T * c.psz), key_d(T * c.dsz), key_p(T * c.psz);
  for (uint32_t r = 0; r < T; ++r) {
    CHECK(mp_shuffle_and_remask(t, c.deck(r), c.rh(r), c.pm(r), c.seed(r), &ref_d[r * c.dsz], &ref_p[r * c.psz]) == 0);
    CHECK(mp_verify_shuffle(t, c.deck(r), &ref_d[r * c.dsz], &ref_p[r * c.psz], c.psz) == 0);
    CHECK(mp_shuffle_and_remask(tk[r % 3], c.deck(r), c.rh(r), c.pm(r), c.seed(r), &key_d[r * c.dsz], &key_p[r * c.psz]) == 0);
  }
  std::vector<uint8_t> bad_p(ref_p.begin() + 3 * c.psz, ref_p.begin() + 4 * c.psz);
  bad_p[c.psz - 31] ^= 2;
  const int bad_code = mp_verify_shuffle(t, c.deck(3), &ref_d[3 * c.dsz], bad_p.data(), c.psz);
  CHECK(bad_code > 0);
  std::vector<uint32_t> nonperm(c.pm(2), c.pm(2) + c.N);
  nonperm[1] = nonperm[0];
  std::vector<uint8_t> offcurve(c.deck(5), c.deck(5) + c.dsz);
  offcurve[128 + 32] ^= 1;                                          // y of card 1's first point
  std::vector<uint8_t> od(c.dsz), op(c.psz);
  CHECK(mp_shuffle_and_remask(t, c.deck(2), c.rh(2), nonperm.data(), c.seed(2), od.data(), op.data()) == MP_ERR_BAD_PERMUTATION);
  const std::string err_perm = mp_last_error();
  CHECK(mp_shuffle_and_remask(t, offcurve.data(), c.rh(5), c.pm(5), c.seed(5), od.data(), op.data()) == MP_ERR_BAD_ENCODING);
  const std::string err_enc = mp_last_error();
  CHECK(err_perm != err_enc);

  std::atomic<bool> stop{false};
  std::thread poker([&] {      // setters and the locked getters, throughout
    uint64_t v[8];
    for (int i = 0; !stop.load(); ++i) {
      CHECK(mp_set_work_split(t, i % 3 == 0 ? 0 : -1) == 0);
      CHECK(mp_set_group_adapt(t, i % 2) == 0);
      CHECK(mp_set_io_chunk(tp, 0) == 0);
      (void)mp_reverified_count(t);
      (void)mp_group_size(t, 4096);
      (void)mp_chain_group_size(t, 64, 4, 0);
      (void)mp_chain_last_slice(t);
      CHECK(mp_table_window_bits(tp) == 8);
      stats(t, v);
      stats(tp, v);
      std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
  });

  Barrier bar(T);
  auto threads = [&](auto fn) {
    std::vector<std::thread> th;
    for (uint32_t r = 0; r < T; ++r) th.emplace_back([&, r] { fn(r); });
    for (auto& x : th) x.join();
  };
  uint64_t v[8];
  // (a) 8 threads, one barrier: prove, then verify; each gets the uncoalesced bytes
  CHECK(mp_set_coalesce(t, 8, 500000) == 0);
  std::vector<uint64_t> after_prove(8);
  threads([&](uint32_t r) {
    std::vector<uint8_t> d(c.dsz), p(c.psz);
    bar.wait();
    CHECK(mp_shuffle_and_remask(t, c.deck(r), c.rh(r), c.pm(r), c.seed(r), d.data(), p.data()) == 0);
    CHECK(memcmp(d.data(), &ref_d[r * c.dsz], c.dsz) == 0 && memcmp(p.data(), &ref_p[r * c.psz], c.psz) == 0);
    bar.wait();
    if (r == 0) stats(t, after_prove.data());
    bar.wait();
    CHECK(mp_verify_shuffle(t, c.deck(r), d.data(), p.data(), c.psz) == 0);
  });
  stats(t, v);
  printf("(a) prove: served %llu in %llu calls; + verify: served %llu in %llu calls, largest %llu\n", (unsigned long long)after_prove[0],
         (unsigned long long)after_prove[1], (unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2]);
  CHECK(after_prove[0] == T && after_prove[1] >= 1 && after_prove[1] <= 2);
  CHECK(v[0] == 2 * T && v[1] - after_prove[1] <= 2 && v[5] == 0);
  // (b) one tampered proof in a verify batch: its own check code; everybody else 0
  CHECK(mp_set_coalesce(t, 8, 500000) == 0);
  threads([&](uint32_t r) {
    bar.wait();
    const int rc = mp_verify_shuffle(t, c.deck(r), &ref_d[r * c.dsz], r == 3 ? bad_p.data() : &ref_p[r * c.psz], c.psz);
    CHECK(rc == (r == 3 ? bad_code : 0));
  });
  stats(t, v);
  CHECK(v[0] == T && v[1] <= 2);
  // (c) a non-permutation and an off-curve card in one prove batch: their own error codes and texts; the others' bytes unchanged
  CHECK(mp_set_coalesce(t, 8, 500000) == 0);
  threads([&](uint32_t r) {
    std::vector<uint8_t> d(c.dsz), p(c.psz);
    bar.wait();
    const int rc = mp_shuffle_and_remask(t, r == 5 ? offcurve.data() : c.deck(r), c.rh(r), r == 2 ? nonperm.data() : c.pm(r), c.seed(r),
                                         d.data(), p.data());
    if (r == 2) {
      CHECK(rc == MP_ERR_BAD_PERMUTATION && err_perm == mp_last_error());
    } else if (r == 5) {
      CHECK(rc == MP_ERR_BAD_ENCODING && err_enc == mp_last_error());
    } else {
      CHECK(rc == 0);
      CHECK(memcmp(d.data(), &ref_d[r * c.dsz], c.dsz) == 0 && memcmp(p.data(), &ref_p[r * c.psz], c.psz) == 0);
    }
  });
  stats(t, v);
  CHECK(v[0] == T && v[1] <= 2 && v[5] == 0);
  // (d) keyed calls with 3 distinct keys on a keyless table: the bytes of tables created with those keys
  CHECK(mp_set_coalesce(tp, 8, 500000) == 0);
  threads([&](uint32_t r) {
    std::vector<uint8_t> d(c.dsz), p(c.psz);
    bar.wait();
    CHECK(mp_shuffle_and_remask_keyed(tp, c.key(1 + r % 3), c.deck(r), c.rh(r), c.pm(r), c.seed(r), d.data(), p.data()) == 0);
    CHECK(memcmp(d.data(), &key_d[r * c.dsz], c.dsz) == 0 && memcmp(p.data(), &key_p[r * c.psz], c.psz) == 0);
    CHECK(mp_verify_shuffle_keyed(tp, c.key(1 + r % 3), c.deck(r), d.data(), p.data(), c.psz) == 0);
    CHECK(mp_verify_shuffle_keyed(tp, c.key(1 + (r + 1) % 3), c.deck(r), d.data(), p.data(), c.psz) > 0);      // the wrong key
    CHECK(mp_shuffle_and_remask(tp, c.deck(r), c.rh(r), c.pm(r), c.seed(r), d.data(), p.data()) == MP_ERR_BAD_ARGUMENT);   // keyless
  });
  stats(tp, v);
  CHECK(v[0] == 3 * T && v[5] == 0);
  // keyed calls without coalescing: a batch of one
  CHECK(mp_set_coalesce(tp, 0, 0) == 0);
  CHECK(mp_shuffle_and_remask_keyed(tp, c.key(2), c.deck(1), c.rh(1), c.pm(1), c.seed(1), od.data(), op.data()) == 0);
  CHECK(memcmp(od.data(), &key_d[1 * c.dsz], c.dsz) == 0 && memcmp(op.data(), &key_p[1 * c.psz], c.psz) == 0);
  stats(tp, v);
  CHECK(v[0] == 0);
  // (e) a lone caller with max_batch = 256, max_wait_us = 2000: nothing waits for requests that never come
  CHECK(mp_set_coalesce(t, 256, 2000) == 0);
  const double t0 = now_s();
  CHECK(mp_shuffle_and_remask(t, c.deck(4), c.rh(4), c.pm(4), c.seed(4), od.data(), op.data()) == 0);
  const double lone = now_s() - t0;
  CHECK(memcmp(od.data(), &ref_d[4 * c.dsz], c.dsz) == 0 && memcmp(op.data(), &ref_p[4 * c.psz], c.psz) == 0);
  stats(t, v);
  CHECK(v[0] == 1 && v[1] == 1 && v[4] == 1);
  printf("(e) lone caller: %.1f ms\n", lone * 1e3);
  // (f) coalescing switched on and off while calls are queued: same bytes, same verdicts
  std::atomic<bool> stop_f{false};
  std::thread toggler([&] {
    for (int i = 0; !stop_f.load(); ++i) {
      CHECK(mp_set_coalesce(t, i % 3 == 2 ? 0 : 3 + i % 5, i % 2 ? 0 : 300) == 0);
      std::this_thread::sleep_for(std::chrono::microseconds(300));
    }
  });
  threads([&](uint32_t r) {
    std::vector<uint8_t> d(c.dsz), p(c.psz);
    for (int it = 0; it < 3; ++it) {
      CHECK(mp_shuffle_and_remask(t, c.deck(r), c.rh(r), c.pm(r), c.seed(r), d.data(), p.data()) == 0);
      CHECK(memcmp(d.data(), &ref_d[r * c.dsz], c.dsz) == 0 && memcmp(p.data(), &ref_p[r * c.psz], c.psz) == 0);
      CHECK(mp_verify_shuffle(t, c.deck(r), d.data(), r == 3 ? bad_p.data() : p.data(), c.psz) == (r == 3 ? bad_code : 0));
    }
  });
  stop_f = true;
  toggler.join();
  stop = true;
  poker.join();
  for (int k = 0; k < 3; ++k) mp_table_destroy(tk[k]);
  mp_table_destroy(tp);
  mp_table_destroy(t);
  mp_ctx_destroy(ctx);
  printf("coalesce ok\n");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
static int run_gpu(uint32_t T, uint32_t rounds, uint32_t m, uint32_t n) {
  mp_ctx* ctx = nullptr;
  CHECK(mp_ctx_create(MP_CURVE_STARK, 0, &ctx) == 0);
  const Case c = make_case(ctx, m, n, T);
  mp_table* t = nullptr;
  CHECK(mp_table_create_ex(ctx, c.m, c.n, c.params.data(), c.key(0), 16, &t) == 0);
  std::vector<uint8_t> ref_d(T * c.dsz), ref_p(T * c.psz);
  std::vector<int32_t> st(T, 55);
  CHECK(mp_shuffle_and_remask_batch(t, T, c.decks.data(), c.rho.data(), c.perm.data(), c.seeds.data(), ref_d.data(), ref_p.data(), st.data()) == 0);
  for (int32_t s : st) CHECK(s == 0);
  CHECK(mp_set_coalesce(t, T, 1000) == 0);
  Barrier bar(T);
  std::vector<std::thread> th;
  double t0 = 0;
  for (uint32_t r = 0; r < T; ++r)
    th.emplace_back([&, r] {
      std::vector<uint8_t> d(c.dsz), p(c.psz);
      bar.wait();
      if (r == 0) t0 = now_s();
      for (uint32_t it = 0; it < rounds; ++it) {
        CHECK(mp_shuffle_and_remask(t, c.deck(r), c.rh(r), c.pm(r), c.seed(r), d.data(), p.data()) == 0);
        CHECK(memcmp(d.data(), &ref_d[r * c.dsz], c.dsz) == 0 && memcmp(p.data(), &ref_p[r * c.psz], c.psz) == 0);
        CHECK(mp_verify_shuffle(t, c.deck(r), d.data(), p.data(), c.psz) == 0);
      }
    });
  for (auto& x : th) x.join();
  const double secs = now_s() - t0;
  uint64_t v[8];
  stats(t, v);
  CHECK(v[0] == 2ull * T * rounds && v[5] == 0);
  printf("{\"threads\": %u, \"m\": %u, \"n\": %u, \"proofs\": %llu, \"seconds\": %.4f, \"proofs_per_s\": %.1f, \"served\": %llu, \"batches\": %llu, "
         "\"largest\": %llu, \"closed_full\": %llu, \"closed_time\": %llu, \"rerun\": %llu, \"wait_us\": %llu}\n",
         T, m, n, (unsigned long long)T * rounds, secs, (double)T * rounds / secs, (unsigned long long)v[0], (unsigned long long)v[1],
         (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], (unsigned long long)v[5], (unsigned long long)v[6]);
  mp_table_destroy(t);
  mp_ctx_destroy(ctx);
  printf("coalesce ok\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "tsan";
  if (mode == "tsan") return run_tsan();
  if (mode == "gpu" && argc >= 4) {
    const uint32_t T = (uint32_t)atoi(argv[2]), rounds = (uint32_t)atoi(argv[3]);
    const uint32_t m = argc > 5 ? (uint32_t)atoi(argv[4]) : 2, n = argc > 5 ? (uint32_t)atoi(argv[5]) : 26;
    if (T < 1 || T > 4096 || rounds < 1 || m < 2 || n < 2 || m * n > 4096) return 2;
    return run_gpu(T, rounds, m, n);
  }
  fprintf(stderr, "usage: coalesce_threads tsan | gpu THREADS ROUNDS [m n]\n");
  return 2;
}
