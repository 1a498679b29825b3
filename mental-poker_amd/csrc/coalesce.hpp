#pragma once
// coalesce.hpp -- request coalescing of the single-proof host-buffer entry points (mp_set_coalesce, include/mpshuffle.h).
//
// A caller of the reference's trait makes one proof per call [REF src/lib.rs:181-197]; at B = 1 the engine runs at a few hundred proofs per
// second however many host threads call it, because the context's lock runs their calls one after the other.  With coalescing on, the
// concurrent single-proof calls of a table are gathered into batches and each batch is ONE prove_batch_host / verify_batch_host call:
//
//   - four queues per table (prove / verify, each with and without a per-request key): a batch never mixes them;
//   - a caller reserves a slot in the open batch of its queue (under the queue's mutex) and copies its inputs into that slot of the
//     batch's page-locked staging itself (without the mutex), so packing is spread over the callers; the first caller into an empty
//     batch is its leader;
//   - the batch closes when it holds max_batch requests, or when its leader holds the context's lock and max_wait_us have passed since it
//     opened -- while an earlier batch holds the lock (it runs on the GPU), the next one fills by itself;
//   - the leader runs the batched call, every caller copies its own outputs back and takes its own status word.  Two staging sets per
//     queue: one fills while the other runs; a set is reused only after all its callers have copied out;
//   - lock order: the context's lock, then a queue's mutex -- never the other way round;
//   - a call-level failure of the batched call makes the leader run every request of the batch on its own, so each caller gets exactly
//     what its uncoalesced call would have returned (status word, return code, mp_last_error text on its own thread).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "engine_base.hpp"

namespace mp {

enum CoKind { CO_PROVE = 0, CO_PROVE_KEYED = 1, CO_VERIFY = 2, CO_VERIFY_KEYED = 3 };
using CoClock = std::chrono::steady_clock;

// one caller's buffers (its own host memory)
struct CoRequest {
  const uint8_t* key = nullptr;      // keyed queues
  const uint8_t* deck = nullptr;
  const uint8_t* rho = nullptr;      // prove
  const uint32_t* perm = nullptr;
  const uint8_t* seed = nullptr;
  uint8_t* out_deck = nullptr;
  uint8_t* out_proof = nullptr;
  const uint8_t* shuf = nullptr;     // verify
  const uint8_t* proof = nullptr;
};

// bytes per request of each array of a queue's staging
struct CoGeom {
  size_t pb = 0, dsz = 0, psz = 0, N = 0;
  bool prove = false, keyed = false;
};

// one staging set: page-locked arrays of `cap` requests back to back (the layout of the batched entry points' arguments)
struct CoSet {
  enum State { FREE, OPEN, CLOSED, DONE } state = FREE;
  uint8_t* mem = nullptr;
  size_t cap = 0;
  uint8_t *keys = nullptr, *decks = nullptr, *rho = nullptr, *seeds = nullptr, *out_decks = nullptr, *out_proofs = nullptr;
  uint8_t *shuf = nullptr, *proofs = nullptr;
  uint32_t* perm = nullptr;
  int32_t* status = nullptr;
  size_t limit = 0;                  // max_batch of this batch (the setting when it opened)
  uint32_t wait_us = 0;              // max_wait_us of this batch
  size_t count = 0, filled = 0, left = 0;     // slots reserved / inputs copied in / callers still to copy out
  CoClock::time_point opened;
  std::vector<CoClock::time_point> arrived;
  std::vector<int> rc;               // call-level return code per request (MP_OK unless the request failed on its own)
  std::vector<std::string> err;      // mp_last_error text of a failed request
  std::condition_variable cv;        // leader: the batch closed / every slot is filled; callers: the batch is DONE

  // (re)size for `n` requests; called under the queue's mutex while the set is FREE
  void reserve(const CoGeom& g, size_t n) {
    if (n <= cap) return;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t kb = g.keyed ? up(n * g.pb) : 0, db = up(n * g.dsz), pbb = up(n * g.psz), sb = up(n * 4);
    const size_t bytes = g.prove ? kb + 2 * db + up(n * g.N * 32) + up(n * g.N * 4) + up(n * 32) + pbb + sb : kb + 2 * db + pbb + sb;
    uint8_t* p = (uint8_t*)rt::host_alloc(bytes);
    if (mem) rt::host_free(mem);
    mem = p;
    cap = n;
    uint8_t* o = p;
    auto take = [&](size_t b) {
      uint8_t* r = o;
      o += b;
      return r;
    };
    keys = g.keyed ? take(kb) : nullptr;
    decks = take(db);
    if (g.prove) {
      rho = take(up(n * g.N * 32));
      perm = (uint32_t*)take(up(n * g.N * 4));
      seeds = take(up(n * 32));
      out_decks = take(db);
      out_proofs = take(pbb);
    } else {
      shuf = take(db);
      proofs = take(pbb);
    }
    status = (int32_t*)take(sb);
    arrived.resize(n);
    rc.resize(n);
    err.resize(n);
  }
  void pack(const CoGeom& g, size_t i, const CoRequest& r) {
    if (g.keyed) memcpy(keys + i * g.pb, r.key, g.pb);
    memcpy(decks + i * g.dsz, r.deck, g.dsz);
    if (g.prove) {
      memcpy(rho + i * g.N * 32, r.rho, g.N * 32);
      memcpy(perm + i * g.N, r.perm, g.N * 4);
      memcpy(seeds + i * 32, r.seed, 32);
    } else {
      memcpy(shuf + i * g.dsz, r.shuf, g.dsz);
      memcpy(proofs + i * g.psz, r.proof, g.psz);
    }
  }
  void unpack(const CoGeom& g, size_t i, const CoRequest& r) const {
    if (!g.prove) return;
    memcpy(r.out_deck, out_decks + i * g.dsz, g.dsz);
    memcpy(r.out_proof, out_proofs + i * g.psz, g.psz);
  }
};

struct CoQueue {
  std::mutex mu;
  std::condition_variable free_cv;   // a staging set became FREE
  CoSet set[2];
  int open = -1;                     // the set that takes new requests (-1: none open)
  // counters since mp_set_coalesce (mp_coalesce_stats)
  uint64_t served = 0, calls = 0, largest = 0, closed_full = 0, closed_time = 0, rerun = 0, wait_us = 0;
  void reset() { served = calls = largest = closed_full = closed_time = rerun = wait_us = 0; }
};

// runs requests [first, first + count) of a set as one batched call; returns the call-level code (< 0: fail() has set the text)
using CoRun = std::function<int(CoSet& s, size_t first, size_t count)>;

}  // namespace mp

struct mp_coalescer {
  std::atomic<size_t> max_batch{0};  // 0 = off
  std::atomic<uint32_t> max_wait_us{0};
  mp::CoQueue q[4];
  ~mp_coalescer() {
    for (auto& qq : q)
      for (auto& s : qq.set)
        if (s.mem) mp::rt::host_free(s.mem);
  }
};

namespace mp {

inline bool co_on(const mp_table* t) { return t->co && t->co->max_batch.load(std::memory_order_relaxed) != 0; }

inline CoGeom co_geom(const mp_table* t, int kind) {
  CoGeom g;
  g.pb = t->point_bytes;
  g.N = t->N;
  g.dsz = (size_t)2 * t->N * t->point_bytes;
  g.psz = proof_size_bytes(t->m, t->n, t->point_bytes);
  g.prove = kind == CO_PROVE || kind == CO_PROVE_KEYED;
  g.keyed = kind == CO_PROVE_KEYED || kind == CO_VERIFY_KEYED;
  return g;
}

// One request through queue `kind`.  Returns 1 if coalescing was off when the request arrived (the caller runs it uncoalesced), else the
// request's call-level code: MP_OK with *status = its status word, or < 0 with mp_last_error set on this thread.
inline int co_submit(mp_table* t, int kind, const CoRequest& r, const CoRun& run, int32_t* status) {
  mp_coalescer& co = *t->co;
  CoQueue& q = co.q[kind];
  const CoGeom g = co_geom(t, kind);
  std::unique_lock<std::mutex> lk(q.mu);
  CoSet* s = nullptr;
  bool leader = false;
  while (!s) {
    if (q.open >= 0) {
      s = &q.set[q.open];
    } else if (q.set[0].state == CoSet::FREE || q.set[1].state == CoSet::FREE) {
      // open a batch with the settings of now (mp_set_coalesce affects the batches opened after it)
      const size_t limit = co.max_batch.load();
      if (!limit) return 1;
      const int f = q.set[0].state == CoSet::FREE ? 0 : 1;
      CoSet& ns = q.set[f];
      ns.reserve(g, limit);
      ns.state = CoSet::OPEN;
      ns.limit = limit;
      ns.wait_us = co.max_wait_us.load();
      ns.count = ns.filled = ns.left = 0;
      ns.opened = CoClock::now();
      q.open = f;
      s = &ns;
      leader = true;
    } else {
      q.free_cv.wait(lk);      // both sets busy: one runs, the other is full or being copied out
    }
  }
  const size_t i = s->count++;
  s->arrived[i] = CoClock::now();
  s->rc[i] = MP_OK;
  if (s->count == s->limit) {      // closed full
    s->state = CoSet::CLOSED;
    q.open = -1;
    q.closed_full++;
    s->cv.notify_all();
  }
  lk.unlock();
  s->pack(g, i, r);
  lk.lock();
  if (++s->filled == s->count) s->cv.notify_all();
  if (leader) {
    lk.unlock();
    std::unique_lock<std::recursive_mutex> ctx_lk(t->ctx->mu);      // (context first, then the queue)
    lk.lock();
    if (s->state == CoSet::OPEN) {
      // (the deadline on the steady clock, each wait on the system clock: a steady-clock wait_until is pthread_cond_clockwait, which
      // ThreadSanitizer does not follow; a jump of the system clock only cuts a slice short or long, and the loop looks again)
      const CoClock::time_point deadline = s->opened + std::chrono::microseconds(s->wait_us);
      for (CoClock::time_point now = CoClock::now(); s->state == CoSet::OPEN && now < deadline; now = CoClock::now())
        s->cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::duration_cast<std::chrono::system_clock::duration>(deadline - now));
      if (s->state == CoSet::OPEN) {      // closed by time
        s->state = CoSet::CLOSED;
        q.open = -1;
        q.closed_time++;
      }
    }
    s->cv.wait(lk, [&] { return s->filled == s->count; });
    const size_t B = s->count;
    const CoClock::time_point start = CoClock::now();
    q.calls++;
    q.served += B;
    q.largest = std::max<uint64_t>(q.largest, B);
    for (size_t k = 0; k < B; ++k) q.wait_us += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(start - s->arrived[k]).count();
    lk.unlock();
    // the set is CLOSED and every slot filled: nobody else touches its arrays until DONE
    if (run(*s, 0, B) < 0) {
      // a call-level failure: every request on its own, so that each caller gets what its uncoalesced call returns
      for (size_t k = 0; k < B; ++k) {
        s->rc[k] = run(*s, k, 1);
        if (s->rc[k] < 0) s->err[k] = last_error();
      }
      lk.lock();
      q.rerun += B;
    } else {
      lk.lock();
    }
    s->state = CoSet::DONE;
    s->left = B;
    s->cv.notify_all();
    lk.unlock();
    ctx_lk.unlock();
    lk.lock();
  } else {
    s->cv.wait(lk, [&] { return s->state == CoSet::DONE; });
  }
  const int rc = s->rc[i];
  const std::string err = rc < 0 ? s->err[i] : std::string();
  const int32_t st = s->status[i];
  lk.unlock();
  if (rc == MP_OK) s->unpack(g, i, r);
  lk.lock();
  if (--s->left == 0) {
    s->state = CoSet::FREE;
    q.free_cv.notify_all();
  }
  lk.unlock();
  if (rc < 0) return fail(rc, err);
  *status = st;
  return MP_OK;
}

}  // namespace mp
