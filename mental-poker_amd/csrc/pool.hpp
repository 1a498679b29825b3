#pragma once
// pool.hpp -- an in-process pool of contexts behind one handle (mp_pool_*, include/mpshuffle.h).
//
// The per-player proofs of a round are independent [REF examples/round.rs:263-350] and deterministic in their seeds, and contexts share
// nothing (engine_base.hpp mp_ctx::mu), so a batch can be cut into contiguous blocks that run on several contexts at once and come back as
// exactly the bytes and status words of the uncut call:
//
//   - a member is one mp_ctx on one device plus one persistent worker thread; members on one device are lanes that run side by side on
//     that chip, members on different devices are the multi-GPU case;
//   - a pool table is one mp_table per member.  The first member of every distinct device builds the fixed-base window tables (the devices
//     build in parallel, each on its worker; nothing is copied between devices); the other members of that device hold a read-only view of
//     them (DevBuf::borrow) -- at production widths the tables are tens of gigabytes -- and are created after the owner's build has been
//     synchronised.  Borrowers are destroyed before their owner;
//   - a batched call cuts [0, B) by the rule of bench.py's shard_range -- base, rem = divmod(B, K), the first rem blocks one longer -- over
//     the first K = min(members, max(1, B / min_shard)) members; every worker calls the ordinary mp_*_batch[_keys] entry point on its slice
//     of every buffer, and the calling thread waits for all of them;
//   - lock order: the pool's lock, then (on the workers) a context's lock.  A thread that calls a borrowed member table directly takes the
//     context's lock only, so it simply takes its turn with that member's shard;
//   - mp_last_error is per thread: a worker hands the text of a failed call back with its return code.
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_base.hpp"

namespace mp {

// one persistent thread that runs the jobs posted to it in order
struct PoolWorker {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::function<void()>> jobs;
  bool stop = false;
  std::thread th;
  PoolWorker() {
    th = std::thread([this] {
      for (;;) {
        std::function<void()> job;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return stop || !jobs.empty(); });
          if (jobs.empty()) return;      // (stop: what was posted before it still runs)
          job = std::move(jobs.front());
          jobs.pop_front();
        }
        job();
      }
    });
  }
  PoolWorker(const PoolWorker&) = delete;
  PoolWorker& operator=(const PoolWorker&) = delete;
  ~PoolWorker() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    th.join();
  }
  void post(std::function<void()> job) {
    {
      std::lock_guard<std::mutex> lk(mu);
      jobs.push_back(std::move(job));
    }
    cv.notify_one();
  }
};

// what a worker hands back from one job: the call-level code, the text behind a failure and the host time the call took
struct PoolResult {
  int rc = MP_OK;
  std::string err;
  uint64_t busy_us = 0;
};

// the calling thread's side of a dispatch: counts the jobs still out
struct PoolLatch {
  std::mutex mu;
  std::condition_variable cv;
  size_t left = 0;
  void done() {
    std::lock_guard<std::mutex> lk(mu);      // (notified under the mutex: the waiter owns the latch and may destroy it as soon as it wakes)
    if (--left == 0) cv.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return left == 0; });
  }
};

// contiguous blocks of [0, B) over K members: base, rem = divmod(B, K), the first rem blocks get one more (bench.py shard_range)
inline void pool_block(size_t B, size_t K, size_t i, size_t* first, size_t* count) {
  const size_t base = B / K, rem = B % K;
  *first = i * base + std::min(i, rem);
  *count = base + (i < rem ? 1 : 0);
}

}  // namespace mp

struct mp_pool {
  struct Member {
    mp_ctx* ctx = nullptr;
    int device = 0;
    std::unique_ptr<mp::PoolWorker> worker;
  };
  std::mutex mu;      // pool calls from several host threads run one after the other; the stats getters take it too
  int curve = 0;
  std::vector<Member> members;
  ~mp_pool() {
    for (Member& m : members) m.worker.reset();      // (joins: no job is left when the contexts go)
    for (Member& m : members)
      if (m.ctx) mp_ctx_destroy(m.ctx);
  }
  // runs job(i) for every i < K on member i's worker and waits for all of them; out[i] = what job(i) returned
  void run(size_t K, const std::function<int(size_t)>& job, std::vector<mp::PoolResult>& out) {
    out.assign(K, mp::PoolResult());
    mp::PoolLatch latch;
    latch.left = K;
    for (size_t i = 0; i < K; ++i)
      members[i].worker->post([&, i] {
        const auto t0 = std::chrono::steady_clock::now();
        mp::PoolResult& r = out[i];
        r.rc = job(i);
        if (r.rc < 0) r.err = mp::last_error();
        r.busy_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        latch.done();
      });
    latch.wait();
  }
};

struct mp_pool_table {
  mp_pool* pool = nullptr;
  std::vector<mp_table*> tables;      // one per member
  std::vector<int> owner;             // the member whose fixed-base tables member i reads (i itself: it built them)
  size_t min_shard = 1;
  uint64_t calls = 0, proofs = 0, last_members = 0, builds = 0;
  struct MemberStats {
    uint64_t calls = 0, proofs = 0, busy_us = 0;
  };
  std::vector<MemberStats> stats;
};

namespace mp {

// "member 2 (device 0): ..." -- how a pool call names the member behind an error
inline std::string pool_member_text(const mp_pool* p, size_t i, const std::string& text) {
  return "member " + std::to_string(i) + " (device " + std::to_string(p->members[i].device) + "): " + text;
}

// One batched call through the pool: `call(member, first, count)` is the single-table entry point on that slice.  Returns MP_OK, or the
// code of the lowest member whose call failed as a whole (its text, prefixed, on this thread); the other members' shards are complete.
inline int pool_dispatch(mp_pool_table* pt, size_t B, const std::function<int(size_t, size_t, size_t)>& call) {
  mp_pool* p = pt->pool;
  std::lock_guard<std::mutex> lk(p->mu);
  const size_t K = std::min(pt->tables.size(), std::max<size_t>(1, B / std::max<size_t>(1, pt->min_shard)));
  std::vector<PoolResult> res;
  p->run(K, [&](size_t i) {
    size_t first = 0, count = 0;
    pool_block(B, K, i, &first, &count);
    return call(i, first, count);
  }, res);
  pt->calls++;
  pt->proofs += B;
  pt->last_members = K;
  int rc = MP_OK;
  for (size_t i = K; i-- > 0;) {
    size_t first = 0, count = 0;
    pool_block(B, K, i, &first, &count);
    pt->stats[i].calls++;
    pt->stats[i].proofs += count;
    pt->stats[i].busy_us += res[i].busy_us;
    if (res[i].rc < 0) rc = fail(res[i].rc, pool_member_text(p, i, res[i].err));
  }
  return rc;
}

}  // namespace mp
