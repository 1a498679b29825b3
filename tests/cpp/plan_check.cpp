// Host check of the static job tables of layout.hpp: whatever the work split, every phase of the prover's and the verifier's plans must
// evaluate the same formal sums, without a slot hazard and inside its arenas.  Includes layout.hpp only: no field arithmetic, no GPU.
// Built and run by tests/test_plan_check.py
//   g++ -O2 -std=c++17 -include tools/hostemu/rt.hpp -Itools/hostemu -Imental-poker_amd/csrc tests/cpp/plan_check.cpp
//
// Evaluation model.  A phase is evaluated over formal sums of leaves (S slot | ONE, point, window range | none) in the launch order of
// engine_core.hpp run_msms: fjobs, vjobs (with window lanes job c writes its range sums to out .. out + vsplit), wcjobs, wjobs (fold),
// bjobs, cjobs0, cjobs, cjobs2.  The jobs of one launch do not see each other's outputs.  Digit and table slots are mapped back to S and P
// slots through `recode` and `tables`; a combine term with AFF_FLAG is the leaf (ONE, P slot), NEG_FLAG negates; a combine term that
// names a final slot (below the layout's first partial) which the phase has not written is an external leaf (ONE, J slot): the result
// of another phase, or jkey + k of a keyed plan.
//
// Modes:
//   plan_check                                                    the grid below, the Karatsuba check, the anchor to describe_verify
//   plan_check --features m n fixed var lanes bucket_min keyed toom   the structural branches that plan takes, per phase, and its counts
//   plan_check --plan m n fixed var lanes bucket_min keyed toom       the job tables of that plan (to read a failing configuration)
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "layout.hpp"

using namespace mp;

// ---- configurations ---------------------------------------------------------------------------------------------------------------
struct Split {
  uint32_t fch, vch, lanes;
};
struct Cfg {
  uint32_t m, n;
  Split sp;
  uint32_t bmin;
  bool keyed, toom;
};
static const uint32_t BWIN = 32;          // windows of a bucket job (8-bit windows of a 256-bit scalar); any value serves the checks
static const uint32_t UNSPLIT = 1u << 20; // terms per job of the unsplit plan: larger than any MSM of the grid

static std::string cfg_str(const Cfg& c) {
  char buf[200];
  snprintf(buf, sizeof buf, "m=%u n=%u split(fixed=%u var=%u lanes=%u bucket_min=%u) keyed=%d toom=%d", c.m, c.n, c.sp.fch, c.sp.vch, c.sp.lanes,
           c.bmin, (int)c.keyed, (int)c.toom);
  return buf;
}
static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
  char buf[400];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}
struct Failure {
  std::string msg;
};
[[noreturn]] static void fail(const std::string& m) { throw Failure{m}; }

static ProvePlan prove_plan(const Cfg& c) {
  return make_prove_plan(c.m, c.n, c.sp.fch, c.sp.vch, 64, c.keyed, c.bmin, BWIN, c.toom, c.sp.lanes, 8);
}
static VerifyPlan verify_plan(const Cfg& c) { return make_verify_plan(c.m, c.n, c.sp.fch, c.sp.vch, 64, c.keyed, c.bmin, BWIN, c.sp.lanes, 8); }

// ---- formal sums ------------------------------------------------------------------------------------------------------------------
typedef uint64_t Leaf;
enum { K_P = 0, K_BASE = 1, K_J = 2 };
static const uint32_t ONE = 0xFFFFFFu;      // "scalar 1": above every S slot (checked: nS < ONE)
static const uint32_t NORANGE = 63;
static Leaf leaf(uint32_t s, uint32_t kind, uint32_t p, uint32_t range = NORANGE) {
  return (uint64_t)s << 32 | (uint64_t)kind << 30 | (uint64_t)p << 6 | range;
}
static uint32_t leaf_s(Leaf l) { return (uint32_t)(l >> 32); }
static uint32_t leaf_kind(Leaf l) { return (uint32_t)(l >> 30) & 3u; }
static uint32_t leaf_p(Leaf l) { return (uint32_t)(l >> 6) & 0xFFFFFFu; }
static uint32_t leaf_range(Leaf l) { return (uint32_t)l & 63u; }
static std::string leaf_str(Leaf l) {
  static const char* kinds[] = {"P", "base", "J"};
  std::string s = leaf_s(l) == ONE ? std::string("1") : fmt("S%u", leaf_s(l));
  s += fmt(" * %s%u", kinds[leaf_kind(l)], leaf_p(l));
  if (leaf_range(l) != NORANGE) s += fmt(" [window range %u]", leaf_range(l));
  return s;
}
typedef std::vector<std::pair<Leaf, int32_t>> Sum;      // sorted by leaf, no zero coefficient
static void normalise(Sum& s) {
  std::sort(s.begin(), s.end());
  size_t w = 0;
  for (size_t i = 0; i < s.size();) {
    size_t j = i;
    int64_t c = 0;
    while (j < s.size() && s[j].first == s[i].first) c += s[j++].second;
    if (c) s[w++] = {s[i].first, (int32_t)c};
    i = j;
  }
  s.resize(w);
}
static void add_into(Sum& acc, const Sum& v, int sign) {
  for (auto& t : v) acc.push_back({t.first, sign * t.second});
}
static std::string sum_diff(const Sum& got, const Sum& want) {
  Sum d;
  add_into(d, got, 1);
  add_into(d, want, -1);
  normalise(d);
  std::string s = fmt("%zu leaves differ:", d.size());
  for (size_t i = 0; i < d.size() && i < 4; ++i) s += fmt(" %+d x (%s);", d[i].second, leaf_str(d[i].first).c_str());
  return s;
}

// ---- one phase --------------------------------------------------------------------------------------------------------------------
struct Arena {
  uint32_t nS, nP, nJ, first_partial, nbases;      // first_partial: J slots below it are the layout's final slots
};
typedef std::map<uint32_t, Sum> Finals;            // final slot -> what the phase left there
static const size_t MAXP = 128;                    // PhaseBuilder::end: sub-jobs per MSM and kind

struct Val {
  Sum s;
  uint32_t nf = 0, nv = 0;      // fixed / variable sub-jobs under this value
  int stage = 0;                // launch that wrote it (6 = cjobs)
  bool opaque = false;          // a per-window result of a bucket job: nobody may read it
};

static void eval_phase(const Phase& ph, const Arena& A, Finals& fin) {
  if (A.nS >= ONE || A.nP >= ONE || A.nJ >= ONE) fail("arena too large for the checker's leaves");
  // digit and table slots: each produced exactly once, from a slot inside its arena
  std::vector<uint32_t> d2s(ph.n_dslots, NO_SLOT), t2p(ph.n_tslots, NO_SLOT);
  for (const Term& t : ph.recode) {
    if (t.b >= ph.n_dslots) fail(fmt("recode: digit slot %u >= n_dslots %u", t.b, ph.n_dslots));
    if (t.s >= A.nS) fail(fmt("recode: S slot %u >= nS %u", t.s, A.nS));
    if (d2s[t.b] != NO_SLOT) fail(fmt("recode: digit slot %u produced twice", t.b));
    d2s[t.b] = t.s;
  }
  for (const Term& t : ph.tables) {
    if (t.b >= ph.n_tslots) fail(fmt("tables: table slot %u >= n_tslots %u", t.b, ph.n_tslots));
    if (t.s >= A.nP) fail(fmt("tables: P slot %u >= nP %u", t.s, A.nP));
    if (t2p[t.b] != NO_SLOT) fail(fmt("tables: table slot %u produced twice", t.b));
    t2p[t.b] = t.s;
  }
  for (uint32_t d = 0; d < ph.n_dslots; ++d)
    if (d2s[d] == NO_SLOT) fail(fmt("digit slot %u is never produced", d));
  for (uint32_t t = 0; t < ph.n_tslots; ++t)
    if (t2p[t] == NO_SLOT) fail(fmt("table slot %u is never produced", t));
  if (ph.vsplit < 1 || ph.vsplit > VSPLIT_MAX) fail(fmt("vsplit %u", ph.vsplit));

  std::vector<int32_t> where(A.nJ, -1);
  std::vector<Val> vals;
  std::set<uint32_t> ext_read;
  std::vector<std::pair<uint32_t, Val>> pending;      // the outputs of the launch being evaluated
  auto write = [&](uint32_t slot, Val&& v) {
    if (slot >= A.nJ) fail(fmt("J slot %u written, nJ = %u", slot, A.nJ));
    pending.emplace_back(slot, std::move(v));
  };
  auto launch_done = [&](int stage) {
    for (auto& w : pending) {
      if (where[w.first] != -1) fail(fmt("J slot %u is written twice", w.first));
      if (ext_read.count(w.first)) fail(fmt("J slot %u is written after a combine read it as another phase's result", w.first));
      where[w.first] = (int32_t)vals.size();
      w.second.stage = stage;
      vals.push_back(std::move(w.second));
    }
    pending.clear();
  };
  auto in_range = [&](const char* what, size_t j, uint32_t begin, uint32_t count, size_t size) {
    if (!count) fail(fmt("%s %zu has no terms", what, j));
    if ((uint64_t)begin + count > size) fail(fmt("%s %zu: terms [%u, %u + %u) outside its term vector of %zu", what, j, begin, begin, count, size));
  };

  // 1. fixed-base jobs
  for (size_t j = 0; j < ph.fjobs.size(); ++j) {
    const Job& jb = ph.fjobs[j];
    in_range("fixed job", j, jb.begin, jb.count, ph.fterms.size());
    Val v;
    v.nf = 1;
    for (uint32_t i = 0; i < jb.count; ++i) {
      const Term& t = ph.fterms[jb.begin + i];
      if (t.s >= A.nS) fail(fmt("fixed job %zu: S slot %u >= nS %u", j, t.s, A.nS));
      if (t.b >= A.nbases) fail(fmt("fixed job %zu: base %u >= %u", j, t.b, A.nbases));
      v.s.push_back({leaf(t.s, K_BASE, t.b), 1});
    }
    normalise(v.s);
    write(jb.out, std::move(v));
  }
  launch_done(0);
  // 2. variable-base (Straus) jobs: with window lanes, range r of job c goes to out + r
  for (size_t j = 0; j < ph.vjobs.size(); ++j) {
    const Job& jb = ph.vjobs[j];
    in_range("variable job", j, jb.begin, jb.count, ph.vterms.size());
    for (uint32_t r = 0; r < ph.vsplit; ++r) {
      Val v;
      v.nv = 1;
      for (uint32_t i = 0; i < jb.count; ++i) {
        const Term& t = ph.vterms[jb.begin + i];
        if (t.s >= ph.n_dslots) fail(fmt("variable job %zu: digit slot %u >= n_dslots %u", j, t.s, ph.n_dslots));
        if (t.b >= ph.n_tslots) fail(fmt("variable job %zu: table slot %u >= n_tslots %u", j, t.b, ph.n_tslots));
        v.s.push_back({leaf(d2s[t.s], K_P, t2p[t.b], ph.vsplit > 1 ? r : NORANGE), 1});
      }
      normalise(v.s);
      write(jb.out + r, std::move(v));
    }
  }
  launch_done(1);
  // combine launches
  auto combine = [&](const char* what, const std::vector<Job>& jobs, const std::vector<Term>& terms, int stage) {
    for (size_t j = 0; j < jobs.size(); ++j) {
      const Job& jb = jobs[j];
      in_range(what, j, jb.begin, jb.count, terms.size());
      Val v;
      for (uint32_t i = 0; i < jb.count; ++i) {
        const uint32_t raw = terms[jb.begin + i].s, slot = raw & SLOT_MASK;
        const int sign = (raw & NEG_FLAG) ? -1 : 1;
        if (raw & AFF_FLAG) {
          if (slot >= A.nP) fail(fmt("%s %zu: P slot %u >= nP %u", what, j, slot, A.nP));
          v.s.push_back({leaf(ONE, K_P, slot), sign});
          continue;
        }
        if (slot >= A.nJ) fail(fmt("%s %zu reads J slot %u, nJ = %u", what, j, slot, A.nJ));
        if (where[slot] >= 0) {
          const Val& src = vals[(size_t)where[slot]];
          if (src.opaque) fail(fmt("%s %zu reads J slot %u, a per-window result of a bucket job", what, j, slot));
          add_into(v.s, src.s, sign);
          // (a late combine adds up the results of other MSMs, which nothing tells from variable-base sub-jobs of its own: only the
          // outputs of fixed-base jobs count as its sub-jobs; the MSMs it consumes are counted where they are written)
          if (stage != 7 || src.stage == 0) {
            v.nf += src.nf;
            v.nv += src.nv;
          }
        } else if (slot < A.first_partial) {
          ext_read.insert(slot);
          v.s.push_back({leaf(ONE, K_J, slot), sign});
        } else {
          fail(fmt("%s %zu reads partial slot %u, which no earlier launch of the phase wrote", what, j, slot));
        }
      }
      normalise(v.s);
      write(jb.out, std::move(v));
    }
    launch_done(stage);
  };
  // 3. the range sums of an MSM's window-split sub-jobs, range by range
  combine("range combine", ph.wcjobs, ph.wcterms, 2);
  // 4. folds
  for (size_t j = 0; j < ph.wjobs.size(); ++j) {
    const BJob& jb = ph.wjobs[j];
    if (jb.count != ph.vsplit) fail(fmt("fold %zu consumes %u ranges, the phase has %u window lanes", j, jb.count, ph.vsplit));
    Val v;
    for (uint32_t r = 0; r < jb.count; ++r) {
      const uint32_t slot = jb.win_first + r;
      if (slot >= A.nJ) fail(fmt("fold %zu reads J slot %u, nJ = %u", j, slot, A.nJ));
      if (where[slot] < 0) fail(fmt("fold %zu reads partial slot %u, which no earlier launch of the phase wrote", j, slot));
      const Val& src = vals[(size_t)where[slot]];
      if (src.opaque) fail(fmt("fold %zu reads J slot %u, a per-window result of a bucket job", j, slot));
      Sum flat;
      for (auto& t : src.s) {
        if (leaf_range(t.first) != r) fail(fmt("fold %zu: slot %u, range %u of the fold, holds %s", j, slot, r, leaf_str(t.first).c_str()));
        flat.push_back({leaf(leaf_s(t.first), leaf_kind(t.first), leaf_p(t.first)), t.second});
      }
      normalise(flat);
      if (r == 0) {
        v.s = flat;
        v.nf = src.nf;
        v.nv = src.nv;
      } else if (flat != v.s) {
        fail(fmt("fold %zu: range %u does not hold the terms of range 0: %s", j, r, sum_diff(flat, v.s).c_str()));
      }
    }
    if (v.s.empty()) fail(fmt("fold %zu folds nothing", j));
    write(jb.out, std::move(v));
  }
  launch_done(3);
  // 5. bucket jobs
  {
    if (ph.bpos.size() != ph.bterms.size()) fail(fmt("bpos has %zu entries for %zu bucket terms", ph.bpos.size(), ph.bterms.size()));
    std::vector<std::pair<uint32_t, uint32_t>> dig;      // [first digit, end)
    uint32_t kmax = 0;
    for (size_t j = 0; j < ph.bjobs.size(); ++j) {
      const BJob& jb = ph.bjobs[j];
      in_range("bucket job", j, jb.begin, jb.count, ph.bterms.size());
      if (jb.count > BUCKET_TERMS_MAX) fail(fmt("bucket job %zu has %u terms", j, jb.count));
      if (jb.kpad != (jb.count + 63) / 64 * 64) fail(fmt("bucket job %zu: kpad %u for %u terms", j, jb.kpad, jb.count));
      kmax = std::max(kmax, jb.kpad);
      dig.push_back({jb.dig_off, jb.dig_off + BWIN * jb.kpad});
      Val v;
      v.nv = 1;
      for (uint32_t i = 0; i < jb.count; ++i) {
        const Term& t = ph.bterms[jb.begin + i];
        if (t.s >= A.nS) fail(fmt("bucket job %zu: S slot %u >= nS %u", j, t.s, A.nS));
        if (t.b >= A.nP) fail(fmt("bucket job %zu: P slot %u >= nP %u", j, t.b, A.nP));
        const BTermPos& bp = ph.bpos[jb.begin + i];
        if (bp.pos != jb.dig_off + i || bp.kpad != jb.kpad)
          fail(fmt("bucket job %zu, term %u: bpos (%u, %u), the job says (%u, %u)", j, i, bp.pos, bp.kpad, jb.dig_off + i, jb.kpad));
        v.s.push_back({leaf(t.s, K_P, t.b), 1});
      }
      normalise(v.s);
      write(jb.out, std::move(v));
      for (uint32_t w = 0; w < BWIN; ++w) {      // the per-window results: disjoint from every other slot the phase writes
        Val o;
        o.opaque = true;
        write(jb.win_first + w, std::move(o));
      }
    }
    std::sort(dig.begin(), dig.end());
    uint32_t at = 0;
    for (auto& d : dig) {
      if (d.first != at) fail(fmt("bucket digits: a job's range starts at %u, the ranges before it end at %u", d.first, at));
      at = d.second;
    }
    if (at != ph.b_dig_bytes) fail(fmt("bucket digits: the jobs' ranges end at %u, b_dig_bytes = %u", at, ph.b_dig_bytes));
    if (kmax != ph.b_kpad_max) fail(fmt("b_kpad_max = %u, the largest kpad is %u", ph.b_kpad_max, kmax));
  }
  launch_done(4);
  combine("group combine", ph.cjobs0, ph.cterms0, 5);
  combine("combine", ph.cjobs, ph.cterms, 6);
  combine("late combine", ph.cjobs2, ph.cterms2, 7);

  for (uint32_t slot = 0; slot < A.nJ; ++slot) {
    if (where[slot] < 0) continue;
    const Val& v = vals[(size_t)where[slot]];
    if (v.nf > MAXP || v.nv > MAXP) fail(fmt("the MSM in J slot %u has %u fixed and %u variable sub-jobs", slot, v.nf, v.nv));
    if (slot >= A.first_partial) continue;
    if (v.opaque) fail(fmt("final slot %u holds a per-window result of a bucket job", slot));
    for (auto& t : v.s)
      if (leaf_range(t.first) != NORANGE) fail(fmt("final slot %u holds an unfolded range: %s", slot, leaf_str(t.first).c_str()));
    fin[slot] = v.s;
  }
}

// ---- one configuration: every phase of both plans -----------------------------------------------------------------------------------
static const int N_PHASES = 8;
static const char* PHASE_NAMES[N_PHASES] = {"prove.A",  "prove.B", "prove.C", "prove.D", "prove.A2", "prove.B2", "verify.per-equation",
                                            "verify.merged"};
struct Evaluated {
  Finals fin[N_PHASES];
  ProvePlan pp;
  VerifyPlan vp;
};
static Arena prove_arena(const ProvePlan& p, bool keyed) {
  if (keyed != (p.jkey != NO_SLOT)) fail("jkey does not follow `keyed`");
  if (keyed && p.jkey != p.lay.nP) fail(fmt("jkey = %u, nP = %u", p.jkey, p.lay.nP));
  return Arena{p.lay.nS, p.lay.nP, p.nJ, p.lay.nP + (keyed ? 2 * p.lay.m : 0u), FixedBases{p.lay.n}.count()};
}
static Arena verify_arena(const VerifyPlan& v) {
  return Arena{v.lay.nS, v.lay.nP, v.nJ, v.lay.chk_first + v.lay.n_chk, FixedBases{v.lay.n}.count()};
}
static const Phase& phase_of(const Evaluated& e, int i) { return i < 6 ? e.pp.ph[i] : (i == 6 ? e.vp.ph : e.vp.mph); }

static void check_merge_jobs(const Evaluated& e, bool keyed);

// builds and evaluates; a failure names the configuration and the phase
static void evaluate(const Cfg& c, Evaluated& e) {
  const char* where = "plan construction";
  try {
    try {
      e.pp = prove_plan(c);
      e.vp = verify_plan(c);
    } catch (const std::exception& ex) {
      fail(std::string("throws: ") + ex.what());
    }
    const Arena pa = prove_arena(e.pp, c.keyed), va = verify_arena(e.vp);
    for (int i = 0; i < N_PHASES; ++i) {
      where = PHASE_NAMES[i];
      eval_phase(phase_of(e, i), i < 6 ? pa : va, e.fin[i]);
    }
    where = PHASE_NAMES[7];
    check_merge_jobs(e, c.keyed);
  } catch (Failure& f) {
    fail(cfg_str(c) + " phase " + where + ": " + f.msg);
  }
}
static void compare(const Cfg& c, const Evaluated& e, const Evaluated& ref) {
  for (int i = 0; i < N_PHASES; ++i) {
    const std::string tag = cfg_str(c) + " phase " + PHASE_NAMES[i] + ": ";
    for (auto& kv : ref.fin[i]) {
      auto it = e.fin[i].find(kv.first);
      if (it == e.fin[i].end()) fail(tag + fmt("final slot %u of the unsplit plan is not written", kv.first));
      if (it->second != kv.second) fail(tag + fmt("final slot %u differs from the unsplit plan's: ", kv.first) + sum_diff(it->second, kv.second));
    }
    for (auto& kv : e.fin[i])
      if (!ref.fin[i].count(kv.first)) fail(tag + fmt("final slot %u is written, the unsplit plan does not write it", kv.first));
  }
}

// ---- anchor to the specification: describe_verify, fed to a recording sink ----------------------------------------------------------
struct RecSink {
  int cur = -1;
  std::vector<int> opened;
  std::map<int, Sum> eq;                                         // check -> (coefficient slot, point / base)
  void begin(int id) {
    cur = id;
    opened.push_back(id);
  }
  void var(uint32_t coef, uint32_t pslot) { eq[cur].push_back({leaf(coef, K_P, pslot), 1}); }
  void fixed(uint32_t coef, uint32_t base) { eq[cur].push_back({leaf(coef, K_BASE, base), 1}); }
  void end() { normalise(eq[cur]); }
};
// the merged phase, each merged scalar expanded through mjobs / mpairs: every described (check, coefficient, point) exactly once under
// the weight slot mr + check, and nothing else
static void check_merge_jobs(const Evaluated& e, bool keyed) {
  const VerifyLay& l = e.vp.lay;
  RecSink rec;
  describe_verify(l, e.vp.cm, rec, keyed);
  const Finals& fin = e.fin[7];
  if (fin.size() != 1 || !fin.count(l.chk_merged)) fail(fmt("writes %zu final slots, expected the merged check slot %u alone", fin.size(), l.chk_merged));
  std::map<uint32_t, const MergeJob*> by_dst;
  for (const MergeJob& j : e.vp.mjobs) {
    if ((uint64_t)j.begin + j.count > e.vp.mpairs.size()) fail(fmt("merge job for S slot %u: pairs outside mpairs", j.dst));
    if (j.dst >= l.nS) fail(fmt("merge job writes S slot %u >= nS", j.dst));
    if (!by_dst.insert({j.dst, &j}).second) fail(fmt("two merge jobs write S slot %u", j.dst));
  }
  std::map<int, Sum> got;
  size_t used = 0;
  for (auto& t : fin.at(l.chk_merged)) {
    const uint32_t s = leaf_s(t.first), kind = leaf_kind(t.first), p = leaf_p(t.first);
    if (t.second != 1) fail(fmt("merged term %s has coefficient %d", leaf_str(t.first).c_str(), t.second));
    if (kind == K_J || s != (kind == K_P ? l.mvar : l.mfix) + p) fail(fmt("merged term %s does not use the merged scalar of its point", leaf_str(t.first).c_str()));
    auto it = by_dst.find(s);
    if (it == by_dst.end()) fail(fmt("merged term %s: no merge job computes its scalar", leaf_str(t.first).c_str()));
    ++used;
    for (uint32_t i = 0; i < it->second->count; ++i) {
      const MergePair& mp_ = e.vp.mpairs[it->second->begin + i];
      if (mp_.r < l.mr || mp_.r >= l.mr + VC_COUNT) fail(fmt("merge pair of S slot %u: weight slot %u outside mr", s, mp_.r));
      got[(int)(mp_.r - l.mr)].push_back({leaf(mp_.coef, kind, p), 1});
    }
  }
  if (used != e.vp.mjobs.size()) fail(fmt("%zu merge jobs, %zu feed a term of the merged equation", e.vp.mjobs.size(), used));
  for (auto& kv : got) normalise(kv.second);
  for (int id : rec.opened)
    if (got[id] != rec.eq[id]) fail(fmt("check %d under weight slot mr + %d: ", id, id) + sum_diff(got[id], rec.eq[id]));
  for (auto& kv : got)
    if (!rec.eq.count(kv.first)) fail(fmt("terms under weight slot mr + %d, a check the description does not open", kv.first));
}
// the unsplit per-equation phase: for every check the description opens, exactly the described terms in chk_first + id
static void check_per_equation(const Cfg& c, const Evaluated& e) {
  const VerifyLay& l = e.vp.lay;
  RecSink rec;
  describe_verify(l, e.vp.cm, rec, c.keyed);
  const std::string tag = cfg_str(c) + " phase " + PHASE_NAMES[6] + ": ";
  for (int id : rec.opened) {
    if (!vcheck_is_msm(id)) fail(tag + fmt("the description opens check %d, which vcheck_is_msm calls direct", id));
    auto it = e.fin[6].find(l.chk_first + (uint32_t)id);
    if (it == e.fin[6].end()) fail(tag + fmt("check %d is described, slot %u is not written", id, l.chk_first + id));
    if (it->second != rec.eq[id]) fail(tag + fmt("check %d: ", id) + sum_diff(it->second, rec.eq[id]));
  }
  if (e.fin[6].size() != rec.opened.size()) fail(tag + fmt("%zu final slots written for %zu described checks", e.fin[6].size(), rec.opened.size()));
}

// ---- Karatsuba: the 2m diagonals are the schoolbook bilinear form --------------------------------------------------------------------
// Index convention (make_prove_plan and oracle/py/mp_oracle.py mexp_prove): a_0 is the prover's random vector (S slots mea0 + t), a_j for
// 1 <= j <= m is row j of b (S slots b + (j - 1) n + t); ciphertext row i, 1 <= i <= m, is row i - 1 of the shuffled deck (P slots
// shuf + 2 ((i - 1) n + t) + c for component c).  E_k = E(b_k gen; tau_k) + sum over 1 <= i <= m with j = k - m + i in [0, m] of
// <a_j, row i>, every pair with the integer coefficient 1.  The fixed part: tau_k G in component 0; b_k gen + tau_k pk in component 1
// (tau_k pk is the external J slot jkey + k in a keyed plan).
static void check_karatsuba(const Cfg& c, const Evaluated& e) {
  const ProveLay& l = e.pp.lay;
  const uint32_t m = l.m, n = l.n;
  const std::string tag = cfg_str(c) + " phase prove.B (Karatsuba): ";
  if (e.pp.toom.E || l.toom) fail(tag + "not a Karatsuba plan");
  if (!e.pp.lin_coef.empty()) fail(tag + "lin_coef is not empty");
  std::map<uint32_t, Sum> svec;      // S slot -> sum of original S slots (as leaves (slot, base 0))
  for (const LinJob& lj : e.pp.lin) {
    if ((uint64_t)lj.begin + lj.count > e.pp.lin_src.size()) fail(tag + "a LinJob's sources lie outside lin_src");
    if (lj.dst + n > l.nS) fail(tag + fmt("LinJob writes S slots up to %u, nS = %u", lj.dst + n, l.nS));
    for (uint32_t t = 0; t < n; ++t) {
      Sum& s = svec[lj.dst + t];
      if (!s.empty()) fail(tag + fmt("S slot %u is written by two LinJobs", lj.dst + t));
      for (uint32_t i = 0; i < lj.count; ++i) s.push_back({(Leaf)(e.pp.lin_src[lj.begin + i] + t), 1});
    }
  }
  const FixedBases fb{n};
  for (uint32_t k = 0; k < 2 * m; ++k)
    for (uint32_t comp = 0; comp < 2; ++comp) {
      const uint32_t slot = l.meE + 2 * k + comp;
      auto it = e.fin[1].find(slot);
      if (it == e.fin[1].end()) fail(tag + fmt("E_%u component %u (slot %u) is not written", k, comp, slot));
      Sum got, want;
      for (auto& t : it->second) {
        const uint32_t s = leaf_s(t.first), p = leaf_p(t.first);
        if (leaf_kind(t.first) != K_P || s == ONE) {
          got.push_back(t);
          continue;
        }
        Sum one_s{{(Leaf)s, 1}}, one_p{{leaf(ONE, K_P, p), 1}};
        const Sum& ss = svec.count(s) ? svec[s] : one_s;
        const Sum& ps = e.fin[4].count(p) ? e.fin[4].at(p) : one_p;
        for (auto& a : ss)
          for (auto& b : ps) {
            if (leaf_s(b.first) != ONE || leaf_kind(b.first) != K_P) fail(tag + "an operand row of phase A2 is not a sum of points");
            got.push_back({leaf((uint32_t)a.first, K_P, leaf_p(b.first)), t.second * a.second * b.second});
          }
      }
      normalise(got);
      for (uint32_t i = 1; i <= m; ++i) {
        const int64_t j = (int64_t)k - m + i;
        if (j < 0 || j > (int64_t)m) continue;
        const uint32_t vec = j == 0 ? l.mea0 : l.b + (uint32_t)(j - 1) * n;
        for (uint32_t t = 0; t < n; ++t) want.push_back({leaf(vec + t, K_P, l.shuf + 2 * ((i - 1) * n + t) + comp), 1});
      }
      if (comp == 0) {
        want.push_back({leaf(l.metau + k, K_BASE, fb.G()), 1});
      } else {
        want.push_back({leaf(l.meb + k, K_BASE, fb.gen()), 1});
        want.push_back({c.keyed ? leaf(ONE, K_J, e.pp.jkey + k) : leaf(l.metau + k, K_BASE, fb.pk()), 1});
      }
      normalise(want);
      if (got != want) fail(tag + fmt("E_%u component %u is not the schoolbook form: ", k, comp) + sum_diff(got, want));
    }
}

// ---- the grid -------------------------------------------------------------------------------------------------------------------
// (tests/test_plan_check.py computes the number of configurations from its own copy of these lists)
static const uint32_t SMALL_N[] = {2, 3, 8, 9}, LARGE_N[] = {63, 64, 65, 128, 129};      // the large n at m = 2 only
static const uint32_t M_FIRST = 2, M_LAST = 18;
// the six default PlanParams of engine_core.hpp (fixed, variable, window lanes) with both tiny_v variants, and the six of
// tests/shuffle_edge_cases.py PLAN_PARAMS
static const Split NAMED[] = {{8, 64, 1}, {1, 16, 16}, {4, 32, 4}, {1, 1, 1}, {1, 2, 1}, {4, 64, 16}, {1, 8, 8},
                              {4, 16, 3}, {8, 64, 16}, {1, 2, 5}, {1, 1, 2}, {4, 64, 7}, {1, 1, 4}};
static const uint32_t CHUNKS[][2] = {{1, 1}, {2, 2}, {3, 3}, {4, 4}, {8, 8}, {16, 16}, {32, 32}, {64, 64}, {1, 64}, {64, 1}, {2, 3}, {3, 2}};
static const uint32_t CHUNKS_LARGE[][2] = {{1, 1}, {3, 3}, {64, 64}, {1, 64}};
static const uint32_t LANES[] = {1, 2, 3, 5, 16}, LANES_LARGE[] = {1, 3, 16};
static const Split BUCKET_SPLITS[] = {{1, 1, 1}, {4, 16, 3}, {8, 64, 16}};      // x bucket_min = largest MSM - 1, the same, + 1
static const uint32_t BUCKET_FIXED[] = {2, 64};                                // x the first two of BUCKET_SPLITS

template <class T, size_t K>
static size_t len(const T (&)[K]) { return K; }

static uint32_t largest_msm(const Evaluated& unsplit) {      // variable-base terms of the largest MSM: one job each in the unsplit plan
  uint32_t k = 0;
  for (int i = 0; i < N_PHASES; ++i)
    for (const Job& j : phase_of(unsplit, i).vjobs) k = std::max(k, j.count);
  return k;
}
static std::vector<std::pair<Split, uint32_t>> splits_of(bool large, uint32_t kmax) {
  std::vector<std::pair<Split, uint32_t>> v;
  for (const Split& s : NAMED) v.push_back({s, 0});
  if (large) {
    for (auto& ch : CHUNKS_LARGE)
      for (uint32_t ln : LANES_LARGE) v.push_back({Split{ch[0], ch[1], ln}, 0});
  } else {
    for (auto& ch : CHUNKS)
      for (uint32_t ln : LANES) v.push_back({Split{ch[0], ch[1], ln}, 0});
  }
  for (const Split& s : BUCKET_SPLITS)
    for (int d = -1; d <= 1; ++d) v.push_back({s, (uint32_t)((int)kmax + d)});
  for (uint32_t b : BUCKET_FIXED)
    for (int i = 0; i < 2; ++i) v.push_back({BUCKET_SPLITS[i], b});
  return v;
}

static size_t run_shape(uint32_t m, uint32_t n, bool large) {
  size_t count = 0;
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int toom = 0; toom < 2; ++toom) {
      const Cfg base{m, n, Split{UNSPLIT, UNSPLIT, 1}, 0, keyed != 0, toom != 0};
      Evaluated ref;
      evaluate(base, ref);
      check_per_equation(base, ref);
      if (m >= 3 && !ref.pp.toom.E) check_karatsuba(base, ref);
      for (int i = 0; i < N_PHASES; ++i) {      // the unsplit plan is unsplit: no window lanes, no bucket job (a combine tree it can have: addends are pieces)
        const Phase& ph = phase_of(ref, i);
        if (!ph.wjobs.empty() || !ph.bjobs.empty()) fail(cfg_str(base) + " phase " + PHASE_NAMES[i] + ": the unsplit plan is split");
      }
      for (auto& sb : splits_of(large, largest_msm(ref))) {
        const Cfg c{m, n, sb.first, sb.second, keyed != 0, toom != 0};
        Evaluated e;
        evaluate(c, e);
        compare(c, e, ref);
        ++count;
      }
    }
  return count;
}

static int run_grid() {
  const auto t0 = std::chrono::steady_clock::now();
  size_t configs = 0, kshapes = 0;
  for (uint32_t m = M_FIRST; m <= M_LAST; ++m)
    for (uint32_t n : SMALL_N) configs += run_shape(m, n, false);
  for (uint32_t n : LARGE_N) configs += run_shape(2, n, true);
  // Karatsuba for m = 3 .. 40 at n = 2 (Toom-Cook off), keyed and not: construction does not throw, the diagonals are the schoolbook
  // form, and two fine splits evaluate the unsplit plan's sums
  for (uint32_t m = 3; m <= 40; ++m)
    for (int keyed = 0; keyed < 2; ++keyed) {
      const Cfg base{m, 2, Split{UNSPLIT, UNSPLIT, 1}, 0, keyed != 0, false};
      Evaluated ref;
      evaluate(base, ref);
      check_per_equation(base, ref);
      check_karatsuba(base, ref);
      for (const Split& s : {Split{1, 1, 2}, Split{4, 16, 3}}) {
        const Cfg c{m, 2, s, 0, keyed != 0, false};
        Evaluated e;
        evaluate(c, e);
        compare(c, e, ref);
        check_karatsuba(c, e);
      }
      ++kshapes;
    }
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("configurations %zu\nkaratsuba_plans %zu\nseconds %.1f\n", configs, kshapes, sec);
  return 0;
}

// ---- --features / --plan --------------------------------------------------------------------------------------------------------
static std::string join(const std::set<std::string>& s) {
  std::string r;
  for (auto& x : s) r += (r.empty() ? "" : ",") + x;
  return r.empty() ? "-" : r;
}
static void features(const Cfg& c, const Evaluated& e) {
  uint64_t st[3][8] = {};
  for (int i = 0; i < N_PHASES; ++i) {
    const Phase& ph = phase_of(e, i);
    const uint32_t first_partial = (i < 6 ? prove_arena(e.pp, c.keyed) : verify_arena(e.vp)).first_partial;
    uint64_t* o = st[i < 6 ? 0 : i - 5];
    o[0] += ph.fterms.size(); o[1] += ph.vterms.size(); o[2] += ph.fjobs.size(); o[3] += ph.vjobs.size(); o[4] += ph.tables.size();
    o[5] += ph.cterms.size() + ph.cterms2.size() + ph.cterms0.size(); o[6] += ph.bterms.size(); o[7] += ph.bjobs.size();
    if (ph.fjobs.empty() && ph.vjobs.empty() && ph.bjobs.empty() && ph.cjobs.empty() && ph.cjobs2.empty()) continue;
    size_t direct = 0, capf = 0, capv = 0, wmulti = 0;
    for (const Job& j : ph.fjobs) direct += j.out < first_partial, capf += j.count > c.sp.fch;
    for (const Job& j : ph.vjobs) direct += ph.vsplit == 1 && j.out < first_partial, capv += j.count > c.sp.vch;
    for (const BJob& j : ph.bjobs) direct += j.out < first_partial;
    std::set<uint32_t> wc_out, c0_out;
    std::map<uint32_t, uint32_t> c0_count;
    for (const Job& j : ph.wcjobs) wc_out.insert(j.out);
    for (const Job& j : ph.cjobs0) c0_count[j.out] = j.count;
    for (const BJob& j : ph.wjobs) direct += j.out < first_partial, wmulti += wc_out.count(j.win_first);
    std::set<std::string> flat, tree, buckets;
    for (const Job& j : ph.cjobs) {
      uint32_t pieces = 0, group = 0;
      for (uint32_t k = 0; k < j.count; ++k) {
        auto it = c0_count.find(ph.cterms[j.begin + k].s);
        if (it == c0_count.end()) break;
        pieces += it->second;
        group = std::max(group, it->second);
      }
      if (pieces) tree.insert(fmt("%u/%u", pieces, group)); else flat.insert(fmt("%u", j.count));
    }
    for (const BJob& j : ph.bjobs) buckets.insert(fmt("%u", j.count));
    printf("phase %s direct=%zu cap_fixed=%zu cap_var=%zu flat=%s tree=%s wsplit_single=%zu wsplit_multi=%zu lanes=%u bucket=%s late=%zu\n", PHASE_NAMES[i],
           direct, capf, capv, join(flat).c_str(), join(tree).c_str(), ph.wjobs.size() - wmulti, wmulti, ph.vsplit, join(buckets).c_str(),
           ph.cjobs2.size());
  }
  static const char* names[3] = {"prove", "verify.per-equation", "verify.merged"};
  for (int k = 0; k < 3; ++k)
    printf("stats %s fixed_terms=%llu var_terms=%llu fixed_jobs=%llu var_jobs=%llu table_bases=%llu combine_terms=%llu bucket_terms=%llu bucket_jobs=%llu\n",
           names[k], (unsigned long long)st[k][0], (unsigned long long)st[k][1], (unsigned long long)st[k][2], (unsigned long long)st[k][3],
           (unsigned long long)st[k][4], (unsigned long long)st[k][5], (unsigned long long)st[k][6], (unsigned long long)st[k][7]);
  Evaluated ref;
  evaluate(Cfg{c.m, c.n, Split{UNSPLIT, UNSPLIT, 1}, 0, c.keyed, c.toom}, ref);
  printf("largest_msm %u\n", largest_msm(ref));      // variable-base terms of the largest MSM of the shape (the merged equation)
}
static void dump(const Evaluated& e) {
  auto jobs = [](const char* what, const std::vector<Job>& js, const std::vector<Term>& ts, bool comb) {
    for (const Job& j : js) {
      printf("  %s out=%u:", what, j.out);
      for (uint32_t i = 0; i < j.count && j.begin + i < ts.size(); ++i) {
        const Term& t = ts[j.begin + i];
        if (comb) printf(" %s%s%u", (t.s & NEG_FLAG) ? "-" : "+", (t.s & AFF_FLAG) ? "P" : "J", t.s & SLOT_MASK); else printf(" (%u,%u)", t.s, t.b);
      }
      printf("\n");
    }
  };
  for (int i = 0; i < N_PHASES; ++i) {
    const Phase& ph = phase_of(e, i);
    printf("phase %s lanes=%u digit_slots=%u table_slots=%u\n", PHASE_NAMES[i], ph.vsplit, ph.n_dslots, ph.n_tslots);
    jobs("fixed", ph.fjobs, ph.fterms, false);
    jobs("var", ph.vjobs, ph.vterms, false);
    jobs("range-combine", ph.wcjobs, ph.wcterms, true);
    for (const BJob& j : ph.wjobs) printf("  fold out=%u ranges=[%u, +%u)\n", j.out, j.win_first, j.count);
    for (const BJob& j : ph.bjobs) printf("  bucket out=%u windows=[%u, +%u) terms=[%u, +%u) kpad=%u dig_off=%u\n", j.out, j.win_first, BWIN, j.begin, j.count, j.kpad, j.dig_off);
    jobs("group-combine", ph.cjobs0, ph.cterms0, true);
    jobs("combine", ph.cjobs, ph.cterms, true);
    jobs("late-combine", ph.cjobs2, ph.cterms2, true);
  }
}

int main(int argc, char** argv) {
  try {
    if (argc == 10 && (!strcmp(argv[1], "--features") || !strcmp(argv[1], "--plan"))) {
      uint32_t a[8];
      for (int i = 0; i < 8; ++i) a[i] = (uint32_t)strtoul(argv[2 + i], nullptr, 10);
      const Cfg c{a[0], a[1], Split{a[2], a[3], a[4]}, a[5], a[6] != 0, a[7] != 0};
      Evaluated e;
      if (!strcmp(argv[1], "--plan")) {      // print first: this mode is for plans that do not evaluate
        e.pp = prove_plan(c);
        e.vp = verify_plan(c);
        dump(e);
        return 0;
      }
      evaluate(c, e);
      features(c, e);
      return 0;
    }
    if (argc != 1) {
      fprintf(stderr, "usage: plan_check [--features|--plan m n fixed var lanes bucket_min keyed toom]\n");
      return 2;
    }
    return run_grid();
  } catch (Failure& f) {
    printf("FAIL %s\n", f.msg.c_str());
    return 1;
  }
}
