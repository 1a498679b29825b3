// engine_core.hpp -- the per-curve engine: batch workspace, plans on the device, prove / verify pipelines.
// Included by one translation unit per curve (curve_*.hip).
#pragma once
#include "engine_base.hpp"
#include "kernels_bucket.hpp"
#include "kernels_canonical.hpp"
#include "kernels_sigma.hpp"
#include "kernels_open.hpp"
#include "kernels_deal.hpp"
#include "kernels_sample.hpp"
#include "kernels_screen.hpp"
#include "kernels_chain_pieces.hpp"
#include "kernels_keyset.hpp"
#include "serialize_host.hpp"
#include "setup_host.hpp"

namespace mp {

static const uint32_t FCHUNK = 8;     // fixed-base terms per sub-job (8 x 13..32 mixed additions, by window width)
static const uint32_t VCHUNK = 64;    // variable-base terms per sub-job: the terms of a job share one 250-doubling chain
static const uint32_t NORM_CHUNK = 64;   // points per Fermat inversion in k_normalize
static const uint32_t BUCKET_MIN = 2048; // variable-base terms from which an MSM runs on the bucket kernel (kernels_bucket.hpp)
static const uint32_t BUCKET_MIN_SMALL_BATCH = 512;   // ... in the finest split (latency, not throughput): the merged equation of a 300-card proof (1 239 terms), not that of a 52-card one (239: Straus verifies one proof in 1.4 ms, the rebuilt bucket kernel in 1.6; profiles/r05d_latency.txt)

struct PhaseDev {
  DevBuf<Term> recode, tables, fterms, vterms, cterms, cterms2, cterms0;
  DevBuf<Job> fjobs, vjobs, cjobs, cjobs2, cjobs0;
  DevBuf<BJob> bjobs;
  DevBuf<Term> bterms;
  DevBuf<BTermPos> bpos;
  DevBuf<Job> wcjobs;       // window-split Straus jobs (layout.hpp Phase::vsplit): range sums over an MSM's sub-jobs,
  DevBuf<Term> wcterms;
  DevBuf<BJob> wjobs;       // and the fold of an MSM's range sums
  uint32_t vsplit = 1, n_wc = 0, n_w = 0;
  uint32_t n_b = 0, n_bterms = 0, b_dig_bytes = 0, b_kpad_max = 0, b_bits = 8;
  uint32_t n_recode = 0, n_tables = 0, n_f = 0, n_v = 0, n_c = 0, n_c2 = 0, n_c0 = 0, n_tslots = 0, n_dslots = 0;
  std::vector<std::pair<uint32_t, uint32_t>> normalize;
  void upload(const Phase& ph, rt::Stream s) {
    recode.upload(ph.recode, s);
    tables.upload(ph.tables, s);
    fterms.upload(ph.fterms, s);
    vterms.upload(ph.vterms, s);
    cterms.upload(ph.cterms, s);
    fjobs.upload(ph.fjobs, s);
    vjobs.upload(ph.vjobs, s);
    cjobs.upload(ph.cjobs, s);
    cterms2.upload(ph.cterms2, s);
    cjobs2.upload(ph.cjobs2, s);
    n_c2 = (uint32_t)ph.cjobs2.size();
    cterms0.upload(ph.cterms0, s);
    cjobs0.upload(ph.cjobs0, s);
    n_c0 = (uint32_t)ph.cjobs0.size();
    wcjobs.upload(ph.wcjobs, s);
    wcterms.upload(ph.wcterms, s);
    wjobs.upload(ph.wjobs, s);
    vsplit = ph.vsplit;
    n_wc = (uint32_t)ph.wcjobs.size();
    n_w = (uint32_t)ph.wjobs.size();
    bjobs.upload(ph.bjobs, s);
    bterms.upload(ph.bterms, s);
    bpos.upload(ph.bpos, s);
    n_b = (uint32_t)ph.bjobs.size();
    n_bterms = (uint32_t)ph.bterms.size();
    b_dig_bytes = ph.b_dig_bytes;
    b_kpad_max = ph.b_kpad_max;
    b_bits = ph.b_bits;
    n_recode = (uint32_t)ph.recode.size();
    n_tables = (uint32_t)ph.tables.size();
    n_f = (uint32_t)ph.fjobs.size();
    n_v = (uint32_t)ph.vjobs.size();
    n_c = (uint32_t)ph.cjobs.size();
    n_tslots = ph.n_tslots;
    n_dslots = ph.n_dslots;
    normalize = ph.normalize;
  }
};

// per-batch arenas
struct Workspace {
  uint32_t fw = 8;      // words of a base-field element (Geo<C>::FW of the owning table: 8, or 12 on BLS12-377)
  uint32_t Bpad = 0;
  uint32_t nS = 0, nP = 0, nJ = 0, nD = 0, nT = 0, nwin = 0, stage_words = 0;
  DevBuf<uint32_t> S, P, J, T, NS, NS2, stage, seed, direct;      // NS2: inversion scratch of the main stream while `side` has NS (prove_dev: m points per proof, allocated by reserve_ws for batches that fork)
  DevBuf<uint32_t> W;       // wire words of the loaded decks, [slot][word][Bpad] (what the transcript hashes; LoadPointsArgs::W)
  DevBuf<int8_t> D;
  DevBuf<int16_t> D16;      // bucket-method digits, proof-major: [b][d8_bytes] (d8_bytes counts digits)
  uint32_t d8_bytes = 0;
  // scratch rows of the bucket kernel's persistent waves (kernels_bucket.hpp): the sorted point references of the window a wave is
  // working on, and its parked bucket sums -- at most 2 048 x (128 KB + 64 KB), whatever the batch
  DevBuf<uint32_t> bk_sorted, bk_park, bk_counter, bk_timing, bk_quarters;
  DevBuf<uint16_t> bk_offs;           // the split pipeline's bucket offsets per (item, chunk)
  void ensure_bucket(uint32_t nslots, uint32_t kpad_max, uint32_t bits, uint32_t xw, rt::Stream s) {
    bk_sorted.alloc((size_t)nslots * kpad_max, s, false);
    bk_park.alloc((size_t)nslots * bk_buckets(bits) * xw, s, false);
    bk_counter.alloc(8, s);
  }
  DevBuf<int32_t> status;
  // The arenas are slot-major with the lane stride Bpad.  Bpad follows the batch (B rounded up to a wave), whatever the arenas were
  // allocated for (`cap` lanes): a 1 024-proof batch laid out with the stride of an earlier 262 144-proof one touches 32 KB out of
  // every 8 MB -- a TLB miss per slot -- and ran at 100 k proofs/s instead of 160 k (round 4).  Lanes [B, Bpad) of the J arena are
  // read by the flat normalisation kernels and must hold zeros (Z = 0: skipped), so a change of stride clears the part in use.
  uint32_t cap = 0;
  void ensure(uint32_t B, uint32_t nS_, uint32_t nP_, uint32_t nJ_, uint32_t nD_, uint32_t nT_, uint32_t nwin_,
              uint32_t stage_words_, rt::Stream s, uint32_t d8_bytes_ = 0) {
    const uint32_t need = (B + 63u) & ~63u;
    const bool grow = !(need <= cap && nS_ <= nS && nP_ <= nP && nJ_ <= nJ && nD_ <= nD && nT_ <= nT && stage_words_ <= stage_words &&
                        d8_bytes_ <= d8_bytes);
    if (grow) {
      cap = std::max(cap, need);
      nS = std::max(nS, nS_); nP = std::max(nP, nP_); nJ = std::max(nJ, nJ_); nD = std::max(nD, nD_); nT = std::max(nT, nT_);
      nwin = nwin_;
      stage_words = std::max(stage_words, stage_words_);
      // re-allocate everything (capacity grows monotonically); zero-filled so padding lanes hold valid data
      S.n = P.n = J.n = T.n = NS.n = stage.n = seed.n = direct.n = 0;
      D.n = 0;
      D16.n = 0;
      d8_bytes = std::max(d8_bytes, d8_bytes_);
      D16.alloc((size_t)std::max(d8_bytes, 4u) * cap, s);      // zero-filled: the padding digits of an MSM stay zero
      status.n = 0;
      S.alloc((size_t)nS * cap * 8, s);
      P.alloc((size_t)nP * cap * 2 * fw, s);
      J.alloc((size_t)nJ * cap * 3 * fw, s);
      D.alloc((size_t)std::max(nD, 1u) * nwin * cap, s);
      T.alloc((size_t)std::max(nT, 1u) * VB_ENTRIES * cap * 2 * fw, s);
      size_t norm_max = std::max((size_t)nT * 8, (size_t)nJ) * cap;   // k_table prefix products (8 per base), k_normalize ranges
      NS.alloc(norm_max * fw, s);
      stage.alloc((size_t)stage_words * cap, s);
      seed.alloc((size_t)8 * cap, s);
      direct.alloc((size_t)2 * cap, s);
      status.alloc(cap, s);
      Bpad = need;
      return;
    }
    if (Bpad != need) {
      Bpad = need;
      rt::dzero(J.p, (size_t)nJ * Bpad * 3 * fw * sizeof(uint32_t), s);      // (the bucket digits D16 are proof-major: no stride in them)
    }
  }
};

template <class C>
struct Table : mp_table {
  typedef typename C::FqP F;
  typedef typename C::FrP R;
  typedef Geo<C> G_;      // element sizes of this curve (words in the arenas, bytes on the wire)

  // One static plan per work split (below): the same results from sub-jobs of different sizes.
  struct PlanSet {
    ProvePlan pplan;
    VerifyPlan vplan;
    PhaseDev pph[6], vph, vmph;      // vmph: the merged verification plan (one MSM for all equations)
    DevBuf<MergeJob> mjobs;
    DevBuf<MergePair> mpairs;
    DevBuf<uint32_t> draws, lin_src, lin_coef, consts;      // consts: Fr constants of the Toom-Cook plan (8 words each)
    DevBuf<LinJob> lin;
    DevBuf<ProofElem> pwire, vwire;
    uint32_t table_group = TABLE_GROUP;
    uint32_t norm_chunk = NORM_CHUNK;
  };
  // Six static work splits per table, identical results.  Sub-job sizes (PlanParams below): fixed-base / variable-base terms per lane,
  // bases per table lane, points per shared inversion, and -- since round 4 -- lanes per variable-base sub-job (window split,
  // layout.hpp vsplit_lo: the windows of a sub-job dealt to k lanes, one fold per MSM).  Measured on an MI355X, 52 cards, proofs/s with
  // the verify calls pipelined (profiles/r04_plan_sweep.txt):
  //   [3] finest      1 / 1 / 2 / 4 / 1     up to ~128 proofs in flight (plus the bucket kernel for the merged verifier equation)
  //   [5] small       1 / 8 / 2 / 4 / 8     up to ~768      (256: 83 k against 55 k on the finest split, 512: 137 k against 90 k)
  //   [1] latency     1 / 16 / 4 / 8 / 16   up to ~2 560    (1 024: 168 k serial, 200 k pipelined; 2 048: 253 k; round 4's 2 / 16 / 4 / 8 / 8: 240 k at 2 048)
  //   [2] medium      4 / 32 / 8 / 16 / 4   up to ~6 144    (4 096: 338 k; round 3's 4 / 16 / 16 / 32 / 1: 242-255 k)
  //   [4] wide        4 / 64 / 16 / 32 / 16 up to ~49 152   (16 384: 462 k, 32 768: 483 k; round 3's 4 / 32 / 16 / 32 / 1: 402 k, 440 k)
  //   [0] throughput  8 / 64 / 64 / 64 / 1  beyond: fewest operations
  // Window lanes instead of ever smaller sub-jobs: a sub-job of T terms costs 250 doublings + 51 T additions whatever T is, so cutting
  // 64-term jobs into 4-term jobs for 16x the lanes multiplied the doublings by 16; dealing the 51 windows to 16 lanes gives the same
  // lanes for one extra fold (< 250 doublings) per MSM output.
  static const int N_PLANS = 6;
  struct PlanParams {
    uint32_t fch, vch, grp, nch, vsp;
  };
  PlanParams pprm[N_PLANS];
  void default_plan_params() {
    // ([3] on decks of up to 128 cards: one variable-base term per lane and two bases per table lane -- the partial sums go through
    // the two-level combine; measured on one MI355X: one 52-card proof 6.6 -> 6.1 ms against 2 terms / 4 bases, same or better up
    // to 256 proofs.  A single 300-card proof already brings more lanes than the chip holds: there the finer split only adds work,
    // BLS12-377 (30,10) 90 -> 117 ms.)
    const uint32_t tiny_v = N <= 128 ? 1u : 2u, tiny_g = N <= 128 ? 2u : 4u;
    pprm[0] = PlanParams{FCHUNK, VCHUNK, TABLE_GROUP, NORM_CHUNK, 1};
    pprm[1] = PlanParams{1, 16, 4, 8, 16};      // (round 5 re-sweep, profiles/r05k_plan_sweep_small.txt: 2 048 proofs 240 k -> 253 k/s against 2 / 16 / 4 / 8 / 8, 1 024 unchanged)
    pprm[2] = PlanParams{4, 32, 8, 16, 4};
    pprm[3] = PlanParams{1, tiny_v, tiny_g, 4, 1};
    pprm[4] = PlanParams{4, 64, 16, 32, 16};
    pprm[5] = PlanParams{1, 8, 2, 4, 8};
  }
  int set_plan_params(int plan, uint32_t fch, uint32_t vch, uint32_t grp, uint32_t nch, uint32_t vsp) override {
    if (plan < 0 || plan >= N_PLANS || !fch || !vch || !grp || grp > TABLE_GROUP || !nch || !vsp || vsp > VSPLIT_MAX) return MP_ERR_BAD_ARGUMENT;
    pprm[plan] = PlanParams{fch, vch, grp, nch, vsp};
    flush();
    rt::stream_sync(ctx->stream);
    build_plans(ps, false);
    psk_ready = false;
    chain.L = 0;
    gplans.clear();
    rt::stream_sync(ctx->stream);
    return MP_OK;
  }
  void set_plan_thresholds(size_t tiny, size_t small, size_t latency, size_t medium, size_t wide) override {
    auto cap = [](size_t v) { return (uint32_t)std::min<size_t>(v, 0x40000000u); };
    tiny_batch = cap(tiny); small_batch = cap(small); latency_batch = cap(latency); medium_batch = cap(medium); wide_batch = cap(wide);
  }
  PlanSet ps[N_PLANS];        // plans with the table's own aggregate key as a fixed base
  PlanSet psk[N_PLANS];       // plans for keyed batches (per-proof aggregate key): built on first use
  bool psk_ready = false;
  DevBuf<Term> key_recode, key_tables;          // static job lists of the per-proof key tables
  uint32_t key_d_first = 0, key_t_first = 0;     // first digit slot (rho_0) / table slot (window 0) of the key machinery
  // crossovers on 52-card decks (round 4, with window lanes; round 3 had 600 / 3 840 / 12 288 / 49 152 for its four finer splits)
  uint32_t tiny_batch = 128;                     // up to this size the finest split,
  uint32_t small_batch = 768;                    // the small split,
  uint32_t latency_batch = 2560;                 // the latency plan (mp_set_latency_batch scales all of them),
  uint32_t medium_batch = 6144;                  // the medium plan,
  uint32_t wide_batch = 49152;                   // the wide plan; larger batches: throughput
  int plan_of(uint32_t B) const {
    if (forced_split >= 0 && forced_split < N_PLANS) return forced_split;
    return B <= tiny_batch ? 3 : (B <= small_batch ? 5 : (B <= latency_batch ? 1 : (B <= medium_batch ? 2 : (B <= wide_batch ? 4 : 0))));
  }
  PlanSet& pick(uint32_t B, bool keyed = false) { return (keyed ? psk : ps)[plan_of(B)]; }
  void set_latency_batch(size_t b) override {
    latency_batch = (uint32_t)std::min<size_t>(b, 0x02000000u);
    tiny_batch = latency_batch / 20;
    small_batch = (uint32_t)((uint64_t)latency_batch * 3 / 10);
    medium_batch = (uint32_t)((uint64_t)latency_batch * 12 / 5);
    wide_batch = (uint32_t)((uint64_t)latency_batch * 96 / 5);
  }
  uint32_t bucket_min = BUCKET_MIN;              // MSMs of at least this many variable-base terms use the bucket kernel (0 = never)
  bool toom_cook = true;        // 3 <= m <= 16: Toom-Cook instead of Karatsuba for the multi-exponentiation diagonals
  void set_toom_cook(bool on) override {
    if (on == toom_cook) return;
    toom_cook = on;
    flush();
    rt::stream_sync(ctx->stream);
    build_plans(ps, false);
    psk_ready = false;
    rt::stream_sync(ctx->stream);
  }
  // Fr constants of a Toom-Cook plan: powers x_e^j of the evaluation points and the inverse Vandermonde matrix W (host)
  std::vector<uint32_t> toom_constants(const ToomPlan& T) {
    std::vector<uint32_t> out((size_t)std::max<uint32_t>(T.n_consts, 1) * 8, 0u);
    if (!T.E) return out;
    const uint32_t E = T.E, mm = E / 2;
    auto put = [&](uint32_t idx, const Fe<R>& v) { fe_pack<R>(v, &out[(size_t)idx * 8]); };
    std::vector<Fe<R>> X(E);
    auto powers = [&](const Fe<R>& x, uint32_t cnt) {                 // x^0 .. x^(cnt-1)
      std::vector<Fe<R>> p(cnt);
      p[0] = fe_one<R>();
      for (uint32_t k = 1; k < cnt; ++k) p[k] = fe_mul<R>(p[k - 1], x);
      return p;
    };
    for (uint32_t e = 2; e < E; ++e) {
      const int32_t x = T.x_of(e);
      X[e] = x >= 0 ? fe_from_u32<R>((uint32_t)x) : fe_neg<R>(fe_from_u32<R>((uint32_t)(-x)));
    }
    // scalar operand of point e: sum_j coef_j a_j with coef_j = x^j, or x^(m - j) for a reversed point
    for (uint32_t e = 2; e < E; ++e) {
      const std::vector<Fe<R>> pw = powers(X[e], mm + 1);
      for (uint32_t j = 0; j <= mm; ++j) put(e * (mm + 1) + j, T.rev_of(e) ? pw[mm - j] : pw[j]);
    }
    // V[e][k]: the product at point e is sum_k V[e][k] E_k -- x^k, or x^(2m - 1 - k) for a reversed point (reversed operands of
    // degrees m and m - 1); e = 0: (1, 0, ...), e = 1 (infinity): (0, ..., 0, 1).  W = V^-1 by Gauss-Jordan
    std::vector<Fe<R>> V((size_t)E * E, fe_zero<R>()), W((size_t)E * E, fe_zero<R>());
    for (uint32_t e = 0; e < E; ++e) {
      W[(size_t)e * E + e] = fe_one<R>();
      if (e == 0) {
        V[0] = fe_one<R>();
        continue;
      }
      if (e == 1) {
        V[(size_t)e * E + (E - 1)] = fe_one<R>();
        continue;
      }
      const std::vector<Fe<R>> pw = powers(X[e], E);
      for (uint32_t k = 0; k < E; ++k) V[(size_t)e * E + k] = T.rev_of(e) ? pw[E - 1 - k] : pw[k];
    }
    for (uint32_t col = 0; col < E; ++col) {
      uint32_t piv = col;
      while (piv < E && fe_is_zero(V[(size_t)piv * E + col])) ++piv;
      if (piv == E) throw std::logic_error("Toom-Cook: singular Vandermonde matrix");
      for (uint32_t k = 0; k < E; ++k) {
        std::swap(V[(size_t)piv * E + k], V[(size_t)col * E + k]);
        std::swap(W[(size_t)piv * E + k], W[(size_t)col * E + k]);
      }
      const Fe<R> inv = fe_inv<R>(V[(size_t)col * E + col]);
      for (uint32_t k = 0; k < E; ++k) {
        V[(size_t)col * E + k] = fe_mul<R>(V[(size_t)col * E + k], inv);
        W[(size_t)col * E + k] = fe_mul<R>(W[(size_t)col * E + k], inv);
      }
      for (uint32_t r = 0; r < E; ++r) {
        if (r == col) continue;
        const Fe<R> f = V[(size_t)r * E + col];
        if (fe_is_zero(f)) continue;
        for (uint32_t k = 0; k < E; ++k) {
          V[(size_t)r * E + k] = fe_sub<R>(V[(size_t)r * E + k], fe_mul<R>(f, V[(size_t)col * E + k]));
          W[(size_t)r * E + k] = fe_sub<R>(W[(size_t)r * E + k], fe_mul<R>(f, W[(size_t)col * E + k]));
        }
      }
    }
    // W now maps the products (index e) to the coefficients (index k): E_k = sum_e W[k][e] P_e
    for (uint32_t k = 0; k < E; ++k)
      for (uint32_t e = 0; e < E; ++e) put(T.w_const_first + k * E + e, W[(size_t)k * E + e]);
    return out;
  }
  void set_bucket_min(uint32_t terms) override {
    if (terms == bucket_min) return;
    bucket_min = terms;
    flush();
    rt::stream_sync(ctx->stream);
    build_plans(ps, false);          // the split between Straus sub-jobs and bucket jobs is part of the static plans
    psk_ready = false;
    rt::stream_sync(ctx->stream);
  }
  void set_bucket_bits(uint32_t bits) override {
    if (bits == bucket_bits) return;
    bucket_bits = bits;
    flush();
    rt::stream_sync(ctx->stream);
    build_plans(ps, false);
    psk_ready = false;
    chain.L = 0;                     // (the chain and group equations are rebuilt with the new width on their next use)
    gplans.clear();
    rt::stream_sync(ctx->stream);
  }
  uint32_t cur_table_group = TABLE_GROUP;
  uint32_t cur_norm_chunk = NORM_CHUNK;          // points per inversion in k_normalize: a property of the plan in use
  DevBuf<uint32_t> fbpts;    // (n+5) affine base points
  DevBuf<uint32_t> FB;       // fixed-base window tables (a view of another table's on the lanes of a pool: init)
  const DevBuf<uint32_t>& fixed_tables() const override { return FB; }
  Workspace ws;
  bool merged_verify = true;   // verify_dev screens the batch with the merged equation first (mp_set_merged_verify)
  void set_merged_verify(bool on) override { merged_verify = on; }
  // curves with a cofactor: every wire point of a call is tested for [q]P == O (kernels_msm.hpp k_subgroup_check)
  bool subgroup_check = !Cofactor<C>::ONE;
  void set_subgroup_check(bool on) override { subgroup_check = on && !Cofactor<C>::ONE; }
  void check_subgroup(Workspace& w, uint32_t B, uint32_t first, uint32_t count) {
    if (!subgroup_check || !count) return;
    SubgroupArgs a{w.P.p, w.status.p, w.Bpad, first};
    MP_RUN(k_subgroup_check, C, B, count, a);
  }
  // The wire points of a verify call: input deck, shuffled deck, the proof's points [, the proof's key] -- the P slots [0, pk (+ 1)).
  // What the caller has validated already (mp_set_validated: a deck that came through mp_deck_deserialize_dev or mp_deck_validate_dev,
  // as the reference's typed points came through CanonicalDeserialize [REF examples/parameter_selection.rs:78-91]) is not tested again:
  // a deck that passes along a chain of shuffles used to be tested in every call that touched it (round 6).
  void check_verify_inputs(Workspace& w, uint32_t B, const VerifyLay& l, bool keyed) {
    if (!validated) {
      check_subgroup(w, B, 0, l.pk + (keyed ? 1u : 0u));
      return;
    }
    if (!(validated & MP_VALIDATED_DECKS)) check_subgroup(w, B, l.deck, 2 * N);
    if (!(validated & MP_VALIDATED_SHUFFLED)) check_subgroup(w, B, l.shuf, 2 * N);
    const uint32_t rest = std::max(l.deck, l.shuf) + 2 * N;      // (decks first, then the proof's points up to pk)
    if (!(validated & MP_VALIDATED_PROOFS)) check_subgroup(w, B, rest, l.pk - rest);
    if (keyed) check_subgroup(w, B, l.pk, 1);
  }
  // wire-v1 decks in HBM -> one status word per deck: 0, or MP_ERR_BAD_ENCODING if some point is not canonical, not on the curve or
  // (curves with a cofactor) outside the prime-order subgroup -- whatever mp_set_subgroup_check says: this IS the validation
  Workspace dws;
  void validate_decks_dev(size_t count, const uint8_t* decks, int32_t* status) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)count;
    Workspace& w = dws;
    w.fw = G_::FW;
    w.ensure(B, 1, 2 * N, 8, 0, 0, nwin, 4, s, 0);
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    LoadPointsArgs a{decks, w.P.p, w.status.p, w.Bpad, 2 * N, 0};
    MP_RUN(k_load_points, C, B, 2 * N, a);
    if (!Cofactor<C>::ONE) {
      SubgroupArgs sa{w.P.p, w.status.p, w.Bpad, 0};
      MP_RUN(k_subgroup_check, C, B, 2 * N, sa);
    }
    rt::d2d(status, w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
  }
  DevBuf<uint32_t> vflag;      // [2] "some proof of the batch needs a closer look" (word 0: the caller's lane, word 1: the verify lane)
  uint32_t* flag_word(bool vlane, rt::Stream s) {
    if (!vflag.n) vflag.alloc(2, s);
    rt::dzero(vflag.p + (vlane ? 1 : 0), 4, s);
    return vflag.p + (vlane ? 1 : 0);
  }
  bool read_flag(bool vlane) {
    uint32_t flag = 0;
    rt::d2h(&flag, vflag.p + (vlane ? 1 : 0), 4, ctx->stream);
    rt::stream_sync(ctx->stream);
    return flag != 0;
  }
  uint32_t nwin = 0;
  FbGeom fbg{8, 32, 255};
  uint32_t init_seed[8];
  // staging for the host-buffer API
  DevBuf<uint8_t> io_a, io_b, io_c, io_d, io_e, io_f;
  DevBuf<int32_t> io_status;

  // ---------------------------------------------------------------- construction
  static bool wire_point_host(const uint8_t* p, Aff<C>& out) {
    // host-side use of the same MP_HD conversion (alignment: copy to an aligned temp)
    alignas(8) uint8_t tmp[G_::PB];
    memcpy(tmp, p, G_::PB);
    return wire_to_aff<C>(tmp, out);
  }

  void build_plans(PlanSet* set, bool keyed) {
    rt::Stream s = ctx->stream;
    for (int k = 0; k < N_PLANS; ++k) {
      PlanSet& q = set[k];
      const PlanParams& pp = pprm[k];
      // the finest split serves batches too small to fill the chip with one lane per Straus job: there the bucket kernel
      // (windows x 64 lanes per MSM) pays from ~500 terms on -- the merged equation of a 300-card proof (1 239 terms), no longer that of a
      // 52-card one (239: since the quad-lane Straus chains of round 3 and the kernel's rebuild in round 4, Straus verifies one proof in 1.4 ms,
      // the bucket kernel in 1.6, 64 proofs in 1.7 against 2.1; profiles/r05d_latency.txt).  The latency split had it too until the end of round 3: from ~1 000
      // proofs on the fixed 14-addition reduction per window is 3x the work of Straus (2 048 proofs: 164 k -> 184 k/s without it)
      const uint32_t bmin = (bucket_min && k == 3) ? std::min(bucket_min, BUCKET_MIN_SMALL_BATCH) : bucket_min;
      // Toom-Cook adds two dependent stages (operand evaluation, interpolation): a win when the batch fills the chip (throughput and
      // medium plans), a loss for a handful of proofs, where the small-batch plans keep Karatsuba (BLS12-377 (6,50), one proof: 78 vs 94 ms)
      const uint32_t pbits = bucket_bits_of(4 * N + 11 * m + 9);      // (the merged equation: the largest MSM a proof brings)
      q.pplan = make_prove_plan(m, n, pp.fch, pp.vch, G_::PB, keyed, bmin, bk_windows(R::BITS, pbits), toom_cook && (k == 0 || k == 2 || k == 4), pp.vsp, pbits);
      q.vplan = make_verify_plan(m, n, pp.fch, pp.vch, G_::PB, keyed, bmin, bk_windows(R::BITS, pbits), pp.vsp, pbits);
      q.table_group = pp.grp;
      q.norm_chunk = pp.nch;       // fewer points per serial inversion chain when lanes are idle
      for (int i = 0; i < 6; ++i) q.pph[i].upload(q.pplan.ph[i], s);
      q.vph.upload(q.vplan.ph, s);
      q.vmph.upload(q.vplan.mph, s);
      q.mjobs.upload(q.vplan.mjobs, s);
      q.mpairs.upload(q.vplan.mpairs, s);
      q.draws.upload(q.pplan.draws, s);
      q.lin.upload(q.pplan.lin, s);
      q.lin_src.upload(q.pplan.lin_src, s);
      q.lin_coef.upload(q.pplan.lin_coef, s);
      q.consts.upload(toom_constants(q.pplan.toom), s);
      q.pwire.upload(q.pplan.wire, s);
      q.vwire.upload(q.vplan.wire, s);
    }
  }
  // keyed batches: plans + the static lists that turn a proof's key into window tables (recode rho, tables of 2^(5w) pk)
  void ensure_keyed() {
    if (psk_ready) return;
    build_plans(psk, true);
    const ProveLay& l = psk[0].pplan.lay;
    // the key's digit / table slots live behind those of every phase of either plan
    key_d_first = key_t_first = 0;
    for (int k = 0; k < N_PLANS; ++k)
      for (int i = 0; i < 6; ++i) {
        key_d_first = std::max(key_d_first, psk[k].pplan.ph[i].n_dslots);
        key_t_first = std::max(key_t_first, psk[k].pplan.ph[i].n_tslots);
      }
    std::vector<Term> rec, tab;
    for (uint32_t i = 0; i < N; ++i) rec.push_back(Term{l.rho + i, key_d_first + i});
    for (uint32_t w = 0; w < nwin; ++w) tab.push_back(Term{l.kw + w, key_t_first + w});
    key_recode.upload(rec, ctx->stream);
    key_tables.upload(tab, ctx->stream);
    psk_ready = true;
  }

  // fb_from: a table of the same parameters, key and window width on the same device, already built and synchronised, whose fixed-base
  // tables this one reads instead of building its own (the lanes of a pool: pool.hpp); it must outlive this table
  int init(mp_ctx* c, uint32_t m_, uint32_t n_, const uint8_t* params, const uint8_t* pk, uint32_t fb_bits, const mp_table* fb_from = nullptr) {
    ctx = c;
    if (fb_bits != 8 && fb_bits != 16 && fb_bits != 20 && fb_bits != 21)
      return fail(MP_ERR_BAD_ARGUMENT, "fixed-base window width must be 8, 16, 20 or 21 bits");
    // windows cover the scalar field's bit length (252 bits on the STARK curve: 12 windows of 21 bits instead of 13 of 20)
    fbg = FbGeom{fb_bits, ((uint32_t)R::BITS + fb_bits - 1u) / fb_bits, (1u << fb_bits) - 1u};
    this->fb_bits = fb_bits;
    m = m_; n = n_; N = m * n;
    point_bytes = G_::PB;
    if (G_::FW > 8) bucket_split_bits = 11;      // (BLS12-377: the one-wave-per-window kernel spills on the 14-limb field, the split pipeline's hot loop does not)
    // plan thresholds count lanes, and a proof of N cards brings ~N/52 times the lanes of a 52-card proof
    set_latency_batch(std::max<size_t>(40, (size_t)2560 * 52 / N));
    nwin = (uint32_t)vb_windows(R::BITS);
    default_plan_params();
    FixedBases fb{n};
    std::vector<Aff<C>> bases(fb.count());
    bool ok = true;
    Aff<C> G, H, gen, pkp;
    ok &= wire_point_host(params, G);
    for (uint32_t j = 0; j < n; ++j) ok &= wire_point_host(params + G_::PB * (1 + j), bases[fb.ck(j)]);
    ok &= wire_point_host(params + G_::PB * (1 + n), H);
    ok &= wire_point_host(params + G_::PB * (2 + n), gen);
    ok &= wire_point_host(pk, pkp);
    if (!ok) return fail(MP_ERR_BAD_ENCODING, "parameters / shared key: bad point encoding");
    ok = aff_in_subgroup_host<C>(G) && aff_in_subgroup_host<C>(H) && aff_in_subgroup_host<C>(gen) && aff_in_subgroup_host<C>(pkp);
    for (uint32_t j = 0; j < n; ++j) ok = ok && aff_in_subgroup_host<C>(bases[fb.ck(j)]);
    if (!ok) return fail(MP_ERR_BAD_ENCODING, "parameters / shared key: a point is not in the prime-order subgroup");
    bases[fb.H()] = H; bases[fb.G()] = G; bases[fb.pk()] = pkp; bases[fb.gen()] = gen;
    Jac<C> gs = jac_inf<C>();
    for (uint32_t j = 0; j < n; ++j) gs = jac_madd<C>(gs, bases[fb.ck(j)]);
    if (jac_is_inf<C>(gs)) {
      bases[fb.gsum()] = aff_inf<C>();
    } else {
      bases[fb.gsum()] = jac_to_aff_with_zinv<C>(gs, fe_inv<F>(gs.Z));
    }
    for (uint32_t i = 0; i < fb.count(); ++i)
      if (i != fb.gsum() && aff_is_inf<C>(bases[i])) return fail(MP_ERR_BAD_ENCODING, "parameters: a base is the point at infinity");

    rt::Stream s = ctx->stream;
    std::vector<uint32_t> flat(fb.count() * G_::PW);
    for (uint32_t i = 0; i < fb.count(); ++i) {
      fe_pack<F>(bases[i].x, &flat[i * G_::PW]);
      fe_pack<F>(bases[i].y, &flat[i * G_::PW + G_::FW]);
    }
    fbpts.upload(flat, s);
    if (fb_from) {
      if (fb_from->fb_bits != fb_bits || fb_from->n != n || fb_from->point_bytes != point_bytes || fb_from->ctx->device != ctx->device)
        return fail(MP_ERR_INTERNAL, "shared fixed-base tables: geometry or device mismatch");
      FB.borrow(fb_from->fixed_tables());
    } else {
      build_fixed_tables(fb.count());
    }

    build_plans(ps, false);
    // Blake2s("Shuffle Proof")  [REF mod.rs:84]
    {
      Blake2sState st;
      blake2s_init(st);
      uint32_t mblk[16] = {0};
      memcpy(mblk, "Shuffle Proof", 13);
      blake2s_compress(st, mblk, 13, true);
      memcpy(init_seed, st.h, 32);
    }
    rt::stream_sync(s);
    return MP_OK;
  }

  void normalize_flat(const uint32_t* src, uint32_t* dst, uint32_t* scratch, size_t count) {
    if (!count) return;
    const uint32_t ch = cur_norm_chunk;
    NormArgs a{src, dst, scratch, (uint32_t)count, (uint32_t)((count + ch - 1) / ch), ch};
    MP_RUN(k_normalize, C, a.nthreads, 1, a);
  }

  // tables with narrow windows, built by chains: out[base][gh.windows][gh.entries] affine (window widths alternate gh.bits / h2)
  void build_narrow_tables(const uint32_t* pts, uint32_t nb, const FbGeom& gh, uint32_t h2, uint32_t* out) {
    rt::Stream s = ctx->stream;
    DevBuf<uint32_t> WJ, W, EJ, scratch;
    const size_t nwinpts = (size_t)nb * gh.windows, nent = nwinpts * gh.entries;
    WJ.alloc(nwinpts * G_::JW, s);
    W.alloc(nwinpts * G_::PW, s);
    EJ.alloc(nent * G_::JW, s);
    scratch.alloc(nent * G_::FW, s);
    enqueue_narrow_tables(pts, nb, gh, h2, out, WJ.p, W.p, EJ.p, scratch.p);
    rt::stream_sync(s);
  }
  // the passes alone, on buffers of the caller's: [nb * windows] Jacobian and affine window bases, [nb * windows * entries] Jacobian
  // entries and as many field elements of inversion scratch.  Nothing is allocated or waited for
  void enqueue_narrow_tables(const uint32_t* pts, uint32_t nb, const FbGeom& gh, uint32_t h2, uint32_t* out, uint32_t* WJ, uint32_t* W,
                             uint32_t* EJ, uint32_t* scratch) {
    const size_t nwinpts = (size_t)nb * gh.windows, nent = nwinpts * gh.entries;
    FbWinArgs wa{pts, WJ, gh, h2};
    MP_RUN(k_fb_windows, C, nb, 1, wa);
    normalize_flat(WJ, W, scratch, nwinpts);
    FbFillArgs fa{W, EJ, gh};
    MP_RUN(k_fb_fill, C, (uint32_t)nwinpts, 1, fa);
    normalize_flat(EJ, out, scratch, nent);
  }
  void build_fixed_tables(uint32_t nb) {
    rt::Stream s = ctx->stream;
    // narrow table first (h-bit windows: h = 8 for 8- and 16-bit tables, 10 for 20-bit tables)
    // (a 21-bit window splits 11 + 10: the narrow windows alternate between the two widths, all of them with 2^h - 1 entries)
    const uint32_t h = fbg.bits == 8 ? 8u : (fbg.bits + 1u) / 2u, h2 = fbg.bits == 8 ? 8u : fbg.bits - h;
    const FbGeom gh{h, fbg.bits == 8 ? fbg.windows : 2u * fbg.windows, (1u << h) - 1u};
    DevBuf<uint32_t> Th;
    Th.alloc((size_t)nb * gh.windows * gh.entries * G_::PW, s);
    build_narrow_tables(fbpts.p, nb, gh, h2, Th.p);
    if (fbg.bits == h) {
      std::swap(FB.p, Th.p);
      std::swap(FB.n, Th.n);
      return;
    }
    // widen: windows of 2h bits; every entry is one affine + affine addition of two narrow entries
    // (16-bit: 2 GB at n = 26; 20-bit: 27 GB -- sized for a 288 GB part)
    const size_t nentw = (size_t)nb * fbg.windows * fbg.entries;
    if (nentw >= ((size_t)1 << 32)) throw std::runtime_error("fixed-base table too large for one launch: use narrower windows");
    DevBuf<uint32_t> EJw, scratchw;
    EJw.alloc(nentw * G_::JW, s, false);
    scratchw.alloc(nentw * G_::FW, s, false);
    FB.alloc(nentw * G_::PW, s, false);
    FbWidenArgs ww{Th.p, EJw.p, gh, fbg};
    MP_RUN(k_fb_widen, C, (uint32_t)nentw, 1, ww);
    const size_t per = (size_t)1 << 26;                     // normalise in slices of 64 M points
    for (size_t off = 0; off < nentw; off += per) {
      const size_t cnt = std::min(per, nentw - off);
      normalize_flat(EJw.p + off * G_::JW, FB.p + off * G_::PW, scratchw.p + off * G_::FW, cnt);
    }
    rt::stream_sync(s);
  }

  // ---- key sets: 8-bit fixed-base tables of K aggregate keys (32 windows x 255 entries = 8 160 points per key: 0.5 MB on the
  // 256-bit curves), built in slices of 2 048 keys so that the Jacobian intermediates stay below 2 GB
  int keyset_build(mp_keyset& ks, size_t K, const uint8_t* keys_host) override {
    rt::Stream s = ctx->stream;
    const FbGeom g8{8u, ((uint32_t)R::BITS + 7u) / 8u, 255u};
    if (K == 0 || K * (size_t)g8.windows * g8.entries >= ((size_t)1 << 32)) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_create: 1 .. 500 000 keys");
    std::vector<uint32_t> flat(K * G_::PW), wire(K * (G_::PB / 4));
    for (size_t i = 0; i < K; ++i) {
      Aff<C> p;
      if (!wire_point_host(keys_host + i * G_::PB, p) || aff_is_inf<C>(p) || !aff_in_subgroup_host<C>(p))
        return fail(MP_ERR_BAD_ENCODING, "mp_keyset_create: key " + std::to_string(i) + " is not a point of the prime-order group");
      fe_pack<F>(p.x, &flat[i * G_::PW]);
      fe_pack<F>(p.y, &flat[i * G_::PW + G_::FW]);
    }
    memcpy(wire.data(), keys_host, K * G_::PB);
    DevBuf<uint32_t> pts;
    pts.upload(flat, s);
    ks.wire.upload(wire, s);
    ks.K = K;
    ks.bits = g8.bits; ks.windows = g8.windows; ks.entries = g8.entries;
    const size_t per_key = (size_t)g8.windows * g8.entries * G_::PW;
    ks.FB.alloc(K * per_key, s, false);
    const std::vector<uint32_t> all_live(K, 1u);
    ks.live.upload(all_live, s);      // (the stream is waited for below)
    const size_t slice = 2048;
    for (size_t k0 = 0; k0 < K; k0 += slice) {
      const uint32_t kc = (uint32_t)std::min(slice, K - k0);
      build_narrow_tables(pts.p + k0 * G_::PW, kc, g8, 8u, ks.FB.p + k0 * per_key);
    }
    rt::stream_sync(s);
    return MP_OK;
  }
  // ---- slots that change (kernels_keyset.hpp).  An update builds the tables of ITS keys only, in slices of KEYSET_UPDATE_SLICE keys
  // whose staging the set keeps: 1 024 keys are 0.5 GB of tables, 0.8 GB of Jacobian entries and 0.27 GB of inversion scratch on the
  // 256-bit curves, and 32 768 lanes for k_fb_fill.  Nothing here waits for the stream once the staging is as large as the call needs.
#ifdef MP_EXP_KS_SLICE      // the emulator's second library (tools/hostemu: make KS_SLICE=4): an update of slice + 1 keys in seconds
  static constexpr size_t KEYSET_UPDATE_SLICE = MP_EXP_KS_SLICE;
#else
  static constexpr size_t KEYSET_UPDATE_SLICE = 1024;
#endif
  int keyset_build_empty(mp_keyset& ks, size_t K) override {
    rt::Stream s = ctx->stream;
    const FbGeom g8{8u, ((uint32_t)R::BITS + 7u) / 8u, 255u};
    if (K == 0 || K * (size_t)g8.windows * g8.entries >= ((size_t)1 << 32)) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_create_empty: 1 .. 500 000 slots");
    ks.K = K;
    ks.bits = g8.bits; ks.windows = g8.windows; ks.entries = g8.entries;
    // zero words are the identity, as wire key and as table entry: what slot 0 lends to a proof that names no key is defined
    ks.wire.alloc(K * (G_::PB / 4), s);
    ks.FB.alloc(K * (size_t)g8.windows * g8.entries * G_::PW, s);
    ks.live.alloc(K, s);
    rt::stream_sync(s);
    return MP_OK;
  }
  void keyset_update(mp_keyset& ks, size_t count, const uint32_t* d_slots, const uint8_t* d_keys, int32_t* d_status) override {
    // a pipelined verify call whose verdict is still unexamined holds a pointer to the set, and its second pass would read the new keys:
    // complete those first.  That also waits for the verify lane; the prove lane IS the stream the update is enqueued on
    flush();
    rt::Stream s = ctx->stream;
    const FbGeom g8{ks.bits, ks.windows, ks.entries};
    const size_t per_key = (size_t)g8.windows * g8.entries * G_::PW;
    if (d_keys) {
      const size_t kc = std::min(count, KEYSET_UPDATE_SLICE), nwinpts = kc * g8.windows, nent = nwinpts * g8.entries;
      ks.up_pts.alloc(kc * G_::PW, s, false);
      ks.up_WJ.alloc(nwinpts * G_::JW, s, false);
      ks.up_W.alloc(nwinpts * G_::PW, s, false);
      ks.up_EJ.alloc(nent * G_::JW, s, false);
      ks.up_scratch.alloc(nent * G_::FW, s, false);
      ks.up_tab.alloc(kc * per_key, s, false);
    }
    for (size_t k0 = 0; k0 < count; k0 += KEYSET_UPDATE_SLICE) {
      const uint32_t kc = (uint32_t)std::min(KEYSET_UPDATE_SLICE, count - k0);
      KeysetSlotsArgs sa{d_keys ? d_keys + k0 * G_::PB : nullptr, d_slots + k0, ks.wire.p, ks.live.p, ks.up_pts.p,
                         d_keys ? d_status + k0 : nullptr};
      MP_RUN(k_keyset_slots, C, kc, 1, sa);
      if (!d_keys) continue;
      enqueue_narrow_tables(ks.up_pts.p, kc, g8, 8u, ks.up_tab.p, ks.up_WJ.p, ks.up_W.p, ks.up_EJ.p, ks.up_scratch.p);
      KeysetScatterArgs ca{reinterpret_cast<const uint4*>(ks.up_tab.p), reinterpret_cast<uint4*>(ks.FB.p), d_slots + k0, ks.live.p,
                           (uint32_t)(per_key / 4)};
      MP_RUN(k_keyset_scatter, C, ca.words, kc, ca);
    }
  }
  void keyset_chain_keys(const mp_keyset& ks, size_t tables, const uint32_t* d_kidx, const uint32_t* d_off, uint8_t* d_keys) override {
    KeysetChainKeysArgs a{ks.wire.p, ks.live.p, d_kidx, d_off, reinterpret_cast<uint32_t*>(d_keys), (uint32_t)ks.K};
    MP_RUN(k_keyset_chain_keys, C, (uint32_t)tables, G_::PB / 4, a);
  }
  void keyset_chain_status(const mp_keyset& ks, size_t tables, const uint32_t* d_kidx, const uint32_t* d_off, int32_t* d_status) override {
    KeysetChainStatusArgs a{ks.live.p, d_kidx, d_off, d_status, (uint32_t)ks.K};
    MP_RUN(k_keyset_chain_status, C, (uint32_t)tables, 1, a);
  }
  DevBuf<uint32_t> ks_keys_main, ks_keys_vlane;      // the wire keys of a batch, gathered from a key set (one buffer per lane)
  const uint8_t* gather_keys(uint32_t B, const mp_keyset* ks, const uint32_t* kidx, int32_t* status, bool vlane = false) {
    DevBuf<uint32_t>& ks_keys = vlane ? ks_keys_vlane : ks_keys_main;
    ks_keys.alloc((size_t)B * (G_::PB / 4), ctx->stream, false);
    GatherKeysArgs ga{ks->wire.p, kidx, ks_keys.p, status, (uint32_t)ks->K, ks->live.p};
    MP_RUN(k_gather_keys, C, B, G_::PB / 4, ga);
    return reinterpret_cast<const uint8_t*>(ks_keys.p);
  }

  uint32_t stage_words_needed() const {
    const size_t tb = G_::PB + 1;     // ark ToBytes of a point: x || y || flag
    size_t bytes = (size_t)(3 + n + 1 + 4 * N) * tb + 16 + 32;
    bytes = std::max(bytes, (size_t)(1 + 6 * m) * tb + 32);
    return (uint32_t)(bytes / 4 + 4);
  }

  void reserve(size_t B) override { reserve_for(B, false); }
  void reserve_for(size_t B, bool keyed) { reserve_ws(ws, B, keyed); }
  void reserve_ws(Workspace& ws, size_t B, bool keyed) {
    if (keyed) ensure_keyed();
    PlanSet& q = pick((uint32_t)B, keyed);
    uint32_t nS = std::max(q.pplan.lay.nS, q.vplan.lay.nS), nP = std::max(q.pplan.lay.nP, q.vplan.lay.nP);
    uint32_t nJ = std::max(q.pplan.nJ, q.vplan.nJ), nD = std::max(q.vph.n_dslots, q.vmph.n_dslots),
             nT = std::max(q.vph.n_tslots, q.vmph.n_tslots);
    uint32_t d8 = std::max(q.vph.b_dig_bytes, q.vmph.b_dig_bytes);
    for (int i = 0; i < 6; ++i) {
      nD = std::max(nD, q.pph[i].n_dslots);
      nT = std::max(nT, q.pph[i].n_tslots);
      d8 = std::max(d8, q.pph[i].b_dig_bytes);
    }
    if (keyed) {
      nD = std::max(nD, key_d_first + N);
      nT = std::max(nT, key_t_first + nwin);
    }
    ws.fw = G_::FW;
    // NS2 = the main stream's inversion scratch while `side` has NS (prove_dev: only c_A's m points are normalised there, and only
    // batches up to overlap_max fork); the verify lane's, chain and ad-hoc workspaces never need it
    ws.ensure((uint32_t)B, nS, nP, nJ, nD, nT, nwin, stage_words_needed(), ctx->stream, d8);
    if (&ws == &this->ws && overlap_max && B <= overlap_max) ws.NS2.alloc((size_t)m * ws.Bpad * G_::FW, ctx->stream, false);
  }

  // ---------------------------------------------------------------- one dependency level of group work
  // parts: which of (recode, window tables, MSMs + combines, normalisations) to run; norm_only / norm_skip: the normalisation range
  // that starts at this slot alone / every range but it; scratch: the inversion scratch to use (default: w.NS)
  enum : uint32_t { PH_RECODE = 1, PH_TABLES = 2, PH_MSM = 4, PH_NORM = 8, PH_ALL = 15 };
  void run_phase(PhaseDev& ph, Workspace& w, uint32_t B, uint32_t parts = PH_ALL, uint32_t norm_only = NO_SLOT, uint32_t norm_skip = NO_SLOT,
                 uint32_t* scratch = nullptr) {
    if (!scratch) scratch = w.NS.p;
    if (parts & PH_TABLES) run_tables(ph, w, B, scratch);
    if (parts & PH_RECODE) run_recode(ph, w, B);
    if (parts & PH_MSM) run_msms(ph, w, B);
    if (parts & PH_NORM) run_normalize(ph, w, B, norm_only, norm_skip, scratch);
  }
  // kernels_quad.hpp: up to this many lanes' worth of (proof, job) pairs run their group operations on four lanes each
#ifdef MP_EXP_QUAD_MAX      // experiment hook (tools/ab_build.py): 0 = never
  uint32_t quad_max_lanes = MP_EXP_QUAD_MAX;
#else
  uint32_t quad_max_lanes = 65536;       // (per launch; 262 144 was tried: the many short chains of a 4 096-proof batch -- combines, fixed-base sums -- then go four lanes wide too: 239 k -> 161 k/s)
#endif
  // (the quad kernels index their items -- (proof, job) pairs -- with 32 bits: a forced mp_set_group_lanes(t, 4) on a launch with more
  // items than that falls back to one lane per chain)
  bool quad_ops(uint32_t B, uint32_t njobs) const {
    const uint64_t items = (uint64_t)B * njobs;
    if (items > 0xFFFFFFF0ull) return false;
    return group_lanes == 4 || (group_lanes == 0 && items * 4u <= quad_max_lanes);
  }
  static uint32_t quad_waves(uint32_t B, uint32_t njobs) { return (uint32_t)(((uint64_t)B * njobs + 15u) / 16u); }
  void run_combine(const CombineArgs& a, uint32_t B, uint32_t njobs) {
    if (quad_ops(B, njobs)) {
      CombineQuadArgs qa{a, B, njobs};
      MP_WAVE_RUN(k_combine_q, C, quad_waves(B, njobs), 0, qa);
    } else {
      MP_RUN(k_combine, C, B, njobs, a);
    }
  }
  void run_recode(PhaseDev& ph, Workspace& w, uint32_t B) {
    if (ph.n_recode) {
      RecodeArgs a{w.S.p, w.D.p, ph.recode.p, w.Bpad, nwin};
      MP_RUN(k_recode, C, B, ph.n_recode, a);
    }
  }
  void run_tables(PhaseDev& ph, Workspace& w, uint32_t B, uint32_t* scratch) {
    if (ph.n_tables) {
      TableArgs a{w.P.p, w.T.p, scratch, ph.tables.p, w.Bpad, ph.n_tables, cur_table_group};
      MP_RUN(k_table, C, B, (ph.n_tables + cur_table_group - 1) / cur_table_group, a);
    }
  }

  // the bucket method over a phase's large MSMs: digits, the persistent wave kernel (one wave per (equation, MSM, window) at a time),
  // the fold of the window results.  `count` equations -- proofs, or chain / group equations -- whose scalars lie in S with lane stride
  // sstride and whose digits go to D (dstride per equation)
  uint32_t bk_pass_eqs = 0;           // the split pipeline's equations per pass and what they were sized for (run_bucket)
  size_t bk_pass_bytes = 0;
  uint32_t bucket_slots() {
    if (!ctx->bk_slots) ctx->bk_slots = BK_WAVES_PER_CU * rt::cu_count();
    return ctx->bk_slots;
  }
  // tile / tile_K: group verification -- the points of equation e as one contiguous run (k_group_tile), terms carry their index in it
  void run_bucket(Workspace& w, PhaseDev& ph, const uint32_t* S, uint32_t sstride, int16_t* D, size_t dstride, uint32_t count,
                  uint32_t link_stride, const char* too_large, const uint32_t* tile = nullptr, uint32_t tile_K = 0) {
    rt::Stream s = ctx->stream;
    const uint32_t c = ph.b_bits, bw = bk_windows(R::BITS, c);
    // (the item counter runs past the last item by one draw per persistent wave)
    if ((uint64_t)count * ph.n_bterms >= ((uint64_t)1 << 32) || (uint64_t)count * ph.n_b * bw + 8ull * bucket_slots() >= ((uint64_t)1 << 32)) throw std::runtime_error(too_large);
    BRecodeArgs ra{S, D, ph.bterms.p, ph.bpos.p, sstride, bw, ph.n_bterms, dstride, c};
    MP_RUN(k_bucket_recode, C, count * ph.n_bterms, 1, ra);
    if (c >= bucket_split_bits) {
      // windows of 12 bits and more: sort / additions / reduction as three kernels (kernels_bucket.hpp, round 6).  Their scratch
      // (sorted runs, offsets, parked sums: ~1.7 MB per (equation, window) at 13 bits and 243 712 points) holds all items of a PASS of
      // equations: as many as fit a quarter of the free memory, 12 GB at the most
      const uint32_t NBK = bk_buckets(c), XW = XyzzWords<C>::N, gmax = bk_chunks(ph.b_kpad_max), units = bk_units(c);
      if (gmax > BK_CHUNKS_MAX) throw std::runtime_error("bucket method: more than 589 824 terms in one multi-scalar multiplication with windows of 12 bits or more");
      const size_t per_item = ((size_t)ph.b_kpad_max + (size_t)NBK * XW) * 4 + (size_t)gmax * bk_offs_row(c) * 2, per_eq = per_item * ph.n_b * bw;
      if (!bk_pass_eqs || bk_pass_bytes != per_eq) {
        size_t free_b = 0, total_b = 0;
        rt::mem_info(&free_b, &total_b);
        // (what the scratch already holds counts as free; the emulator reports no memory: one gigabyte)
        const size_t have = (w.bk_sorted.n + w.bk_park.n) * 4 + w.bk_offs.n * 2;
        const size_t budget = total_b ? std::min<size_t>((size_t)12 << 30, (free_b + have) / 4) : (size_t)1 << 30;
        bk_pass_eqs = (uint32_t)std::max<size_t>(1, std::min<size_t>(budget / per_eq, 0x7FFFFFFFu));
        bk_pass_bytes = per_eq;
      }
      const uint32_t pass = std::min(count, std::max(bk_pass_eqs, 1u));
      const size_t items_max = (size_t)pass * ph.n_b * bw;
      if (items_max * units >= ((uint64_t)1 << 32)) throw std::runtime_error(too_large);
      w.bk_sorted.alloc(items_max * ph.b_kpad_max, s, false);
      w.bk_offs.alloc(items_max * gmax * bk_offs_row(c), s, false);
      w.bk_park.alloc(items_max * NBK * XW, s, false);
      w.bk_quarters.alloc(items_max * 8 * XW, s, false);
      for (uint32_t e0 = 0; e0 < count; e0 += pass) {
        const uint32_t ne = std::min(pass, count - e0), items = ne * ph.n_b * bw;
        const uint32_t acc_lds = bk_acc_lds_words(c, gmax, XW, G_::PW), wpb = rt::waves_per_block(acc_lds), wgs = (items * units + wpb - 1) / wpb;
        BSplitArgs sa{D, w.P.p, w.J.p, ph.bjobs.p, ph.bterms.p, w.Bpad, bw, ph.n_b, dstride, link_stride, c, e0, ne, tile, tile_K,
                      w.bk_sorted.p, w.bk_offs.p, w.bk_park.p, ph.b_kpad_max, gmax, units, wpb, wgs, w.bk_quarters.p};
        ctx->prof.begin("k_bucket_sort", s, (uint64_t)items * gmax);
        MP_BLOCK_LAUNCH(k_bucket_sort, C, s, items * gmax, bk_sort_lds_words(c), sa);
        ctx->prof.end(s);
        MP_WAVE_RUN(k_bucket_acc, C, (wgs + 7u) / 8u * 8u * wpb, acc_lds, sa);      // (8 XCDs x their share of the workgroups: bk_unit_of_wave)
        MP_WAVE_RUN(k_bucket_list, C, (wgs + 7u) / 8u * 8u * wpb, acc_lds, sa);     // (the windows whose digits crowd into a few buckets: nothing to do for the others)
        MP_WAVE_RUN(k_bucket_reduce, C, items * 4u, 64u * XW, sa);
        MP_RUN(k_bucket_final, C, items, 1, sa);
      }
      BFoldArgs fa{w.J.p, ph.bjobs.p, w.Bpad, bw, 0u, c};
      if (quad_ops(count, ph.n_b)) {
        BFoldQuadArgs qa{fa, count, ph.n_b};
        MP_WAVE_RUN(k_bucket_fold_q, C, quad_waves(count, ph.n_b), 0, qa);
      } else {
        MP_RUN(k_bucket_fold, C, count, ph.n_b, fa);
      }
      return;
    }
    const uint32_t nitems = count * ph.n_b * bw, nslots = std::min(nitems, bucket_slots());
    w.ensure_bucket(bucket_slots(), ph.b_kpad_max, c, XyzzWords<C>::N, s);
    rt::dzero(w.bk_counter.p, 8 * 4, s);
    BucketArgs ba{D, w.P.p, w.J.p, ph.bjobs.p, ph.bterms.p, w.Bpad, bw, ph.n_b, dstride, link_stride, c, nitems, nslots, w.bk_counter.p,
                  count, bk_xcd_affine && count >= 8u ? 8u : 1u, tile, tile_K, bk_stage ? 1u : 0u,
                  w.bk_sorted.p, w.bk_park.p, ph.b_kpad_max, nullptr};
#ifdef MP_EXP_BK_TIMING
    w.bk_timing.alloc((size_t)bucket_slots() * 8, s);
    ba.timing = w.bk_timing.p;
#endif
    ctx->prof.begin("k_bucket_msm", s, nitems);
    MP_WAVE_LAUNCH(k_bucket_msm, C, s, nslots, bk_lds_words(c, XyzzWords<C>::N), ba);
    ctx->prof.end(s);
#ifdef MP_EXP_BK_TIMING     // experiment (tools/ab_build.py --units=curve_stark_msm.hip,curve_stark.hip): mean cycles per phase and wave
    {
      std::vector<unsigned long long> tm((size_t)nslots * 4);
      rt::d2h(tm.data(), w.bk_timing.p, tm.size() * 8, s);
      rt::stream_sync(s);
      double sum[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < tm.size(); ++i) sum[i & 3] += (double)tm[i];
      fprintf(stderr, "k_bucket_msm items %u slots %u bits %u kpad %u: cycles/wave sort %.0f ranks %.0f additions %.0f reduction %.0f\n", nitems, nslots, c,
              ph.b_kpad_max, sum[0] / nslots, sum[1] / nslots, sum[2] / nslots, sum[3] / nslots);
    }
#endif
    BFoldArgs fa{w.J.p, ph.bjobs.p, w.Bpad, bw, 0u, c};
    if (quad_ops(count, ph.n_b)) {          // few equations: the fold's ~256 dependent doublings on four lanes each
      BFoldQuadArgs qa{fa, count, ph.n_b};
      MP_WAVE_RUN(k_bucket_fold_q, C, quad_waves(count, ph.n_b), 0, qa);
    } else {
      MP_RUN(k_bucket_fold, C, count, ph.n_b, fa);
    }
  }
  void run_msms(PhaseDev& ph, Workspace& w, uint32_t B) {
    if (ph.n_f) {
      FixedArgs a{w.S.p, w.J.p, FB.p, ph.fjobs.p, ph.fterms.p, w.Bpad, fbg, w.Bpad};
      if (quad_ops(B, ph.n_f)) {
        FixedQuadArgs qa{a, B, ph.n_f};
        MP_WAVE_RUN(k_fixed_msm_q, C, quad_waves(B, ph.n_f), 0, qa);
      } else {
        MP_RUN(k_fixed_msm, C, B, ph.n_f, a);
      }
    }
    if (ph.n_v) {
      VarArgs a{w.D.p, w.T.p, w.J.p, ph.vjobs.p, ph.vterms.p, w.Bpad, nwin, ph.vsplit};
      const uint32_t nvl = ph.n_v * ph.vsplit;      // lanes per proof: (job, window range) pairs
#ifdef MP_EXP_VAR_LDS      // experiment hook (tools/ab_build.py): unused dynamic LDS per workgroup caps the waves per SIMD of k_var_msm
      ctx->prof.begin("k_var_msm", ctx->stream);
      hipLaunchKernelGGL((k_var_msm<C>), dim3((B + 255u) / 256u, nvl), dim3(256), MP_EXP_VAR_LDS, ctx->stream, a, (uint32_t)B);
      ctx->prof.end(ctx->stream);
#else
      if (quad_ops(B, nvl)) {      // a handful of proofs: four lanes per group operation, 3-4 products deep instead of 10
        VarQuadArgs qa{a, B, nvl};
        MP_WAVE_RUN(k_var_msm_q, C, quad_waves(B, nvl), 0, qa);
      } else {
        MP_RUN(k_var_msm, C, B, nvl, a);
      }
#endif
      if (ph.n_wc) {      // window-split jobs: the range sums of an MSM's sub-jobs, range by range ...
        CombineArgs ca{w.J.p, w.P.p, ph.wcjobs.p, ph.wcterms.p, w.Bpad};
        run_combine(ca, B, ph.n_wc);
      }
      if (ph.n_w) {       // ... and the fold R = sum_r 2^(5 lo(r)) S_r, once per MSM
        BFoldArgs fa{w.J.p, ph.wjobs.p, w.Bpad, 0u, nwin, 0u};
        if (quad_ops(B, ph.n_w)) {
          BFoldQuadArgs qa{fa, B, ph.n_w};
          ctx->prof.begin("k_wfold_q", ctx->stream);
          MP_WAVE_LAUNCH(k_bucket_fold_q, C, ctx->stream, quad_waves(B, ph.n_w), 0, qa);
          ctx->prof.end(ctx->stream);
        } else {
          ctx->prof.begin("k_wfold", ctx->stream);
          MP_LAUNCH(k_bucket_fold, C, ctx->stream, B, ph.n_w, fa);
          ctx->prof.end(ctx->stream);
        }
      }
    }
    if (ph.n_b) run_bucket(w, ph, w.S.p, w.Bpad, w.D16.p, (size_t)w.d8_bytes, B, 0u, "bucket recode: batch too large for one launch");
    if (ph.n_c0) {   // group sums of MSMs with many partials
      CombineArgs a{w.J.p, w.P.p, ph.cjobs0.p, ph.cterms0.p, w.Bpad};
      run_combine(a, B, ph.n_c0);
    }
    if (ph.n_c) {
      CombineArgs a{w.J.p, w.P.p, ph.cjobs.p, ph.cterms.p, w.Bpad};
      run_combine(a, B, ph.n_c);
    }
    if (ph.n_c2) {   // second stage: consumers of first-stage combine outputs
      CombineArgs a{w.J.p, w.P.p, ph.cjobs2.p, ph.cterms2.p, w.Bpad};
      run_combine(a, B, ph.n_c2);
    }
  }
  void run_normalize(PhaseDev& ph, Workspace& w, uint32_t B, uint32_t norm_only, uint32_t norm_skip, uint32_t* scratch) {
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    for (auto& r : ph.normalize)
      if ((norm_only == NO_SLOT || r.first == norm_only) && r.first != norm_skip) ranges.push_back(r);
    // the ranges of a phase in as few launches as possible (NORM_MAX_RANGES per launch; element offsets must fit 32 bits)
    for (size_t i = 0; i < ranges.size();) {
      const size_t nr = std::min<size_t>(NORM_MAX_RANGES, ranges.size() - i);
      size_t last_elem = 0;
      for (size_t k = 0; k < nr; ++k)
        last_elem = std::max(last_elem, ((size_t)ranges[i + k].first + ranges[i + k].second) * w.Bpad);
      if (nr == 1 || last_elem >= ((size_t)1 << 32)) {
        auto& r = ranges[i];
        normalize_flat(w.J.p + j_off<C>(r.first, w.Bpad, 0), w.P.p + p_off<C>(r.first, w.Bpad, 0), scratch, (size_t)r.second * w.Bpad);
        ++i;
        continue;
      }
      NormMultiArgs a{};
      a.J = w.J.p; a.P = w.P.p; a.scratch = scratch;
      a.nr = (uint32_t)nr; a.chunk = cur_norm_chunk;
      uint32_t threads = 0, selem = 0;
      for (size_t k = 0; k < nr; ++k) {
        auto& r = ranges[i + k];
        const uint32_t cnt = r.second * w.Bpad;
        a.first[k] = r.first * w.Bpad;
        a.count[k] = cnt;
        a.tstart[k] = threads;
        a.sstart[k] = selem;
        threads += (cnt + cur_norm_chunk - 1) / cur_norm_chunk;
        selem += cnt;
      }
      a.tstart[nr] = threads;
      MP_RUN(k_normalize_multi, C, threads, 1, a);
      i += nr;
    }
  }

  FsStatementArgs statement_args(Workspace& w, uint32_t p_deck, uint32_t p_shuf, uint32_t p_cA, uint32_t s_x, uint32_t p_pk = NO_SLOT) {
    FsStatementArgs a{};
    a.f = FsDev{w.stage.p, w.seed.p, w.Bpad};
    a.S = w.S.p;
    a.P = w.P.p;
    a.fbpts = fbpts.p;
    memcpy(a.init_seed, init_seed, 32);
    a.m = m; a.n = n; a.N = N;
    a.p_deck = p_deck; a.p_shuf = p_shuf; a.p_cA = p_cA; a.s_x = s_x;
    a.p_pk = p_pk;
    a.W = nullptr;
    a.w_deck = a.w_shuf = NO_SLOT;
    return a;
  }
  // The transcript kernels: one lane per proof, or four lanes per hash (k_fsq_*: the lanes of a wave dealt to 64 / lpp proofs)
  // for batches that would leave the chip to a few hundred lone lanes.  Crossover: a lone wave issues every 8-10 cycles, four
  // waves per SIMD every ~4.3, and the quad kernels run ~2.7x fewer instructions per hash on 16x more waves.
  FsqGeom fsq_geom(uint32_t B) const {
    uint32_t lpp = 64;
    while (lpp > 4 && (uint64_t)B * lpp > 65536u) lpp >>= 1;
    return FsqGeom{lpp, B};
  }
  static uint32_t fsq_waves(const FsqGeom& g) { return (g.B + 64u / g.lpp - 1) / (64u / g.lpp); }
  bool fs_quad(uint32_t B) const { return fs_lanes == 4 || (fs_lanes == 0 && B <= FSQ_MAX_BATCH); }
  void run_fs_round1(const FsStatementArgs& a, uint32_t B) {
    if (fs_quad(B)) {
      FsqStatementArgs q{a, fsq_geom(B)};
      MP_WAVE_RUN(k_fsq_round1, C, fsq_waves(q.g), 0, q);
    } else {
      MP_RUN(k_fs_round1, C, B, 1, a);
    }
  }
  void run_fs_round(const FsRoundArgs& a, uint32_t B) {
    if (fs_quad(B)) {
      FsqRoundArgs q{a, fsq_geom(B)};
      MP_WAVE_RUN(k_fsq_round, C, fsq_waves(q.g), 0, q);
    } else {
      MP_RUN(k_fs_round, C, B, 1, a);
    }
  }
  void run_verify_fs(const VerifyFsArgs& a, uint32_t B) {
    if (fs_quad(B)) {
      FsqVerifyArgs q{a, fsq_geom(B)};
      MP_WAVE_RUN(k_fsq_verify, C, fsq_waves(q.g), 0, q);
    } else {
      MP_RUN(k_verify_fs, C, B, 1, a);
    }
  }
  // room for the wire words of `decks` decks per proof (their transcript bytes, kept by k_load_points) -- for the small-batch
  // plans only: there the transcript lane is what a proof waits for (a 300-card BLS12-377 verification: 24 -> 19 ms, a 52-card one
  // 3.5 -> 3.3 ms), while a full batch hides that lane behind thousands of others and would only pay for the extra 64 bytes
  // written per point (-0.3 % on the default bench, A/B)
  uint32_t* wire_words(Workspace& w, uint32_t B, uint32_t decks) {
    const int plan = plan_of(B);
    if (plan != 1 && plan != 3 && plan != 5) return nullptr;
    w.W.alloc((size_t)decks * 2 * N * (G_::PB / 4) * w.Bpad, ctx->stream, false);
    return w.W.p;
  }

  void prove_init(const ProveInitArgs& ia, uint32_t B) {
    if (B <= PROVE_INIT_WAVE_MAX)      // a wave per proof: 64 ChaCha20 blocks at a time instead of one lane's ~300 in a row
      MP_WAVE_RUN(k_prove_init_w, C, B, N, ia);
    else
      MP_RUN(k_prove_init, C, B, 1, ia);
  }
  // the challenge-independent group work behind the re-encryption (after the shuffled deck is normalised): operand sums of its
  // rows (m = 2 Toom-Cook / Karatsuba), their Toom-Cook evaluations (3 <= m <= 16); with_tables: also the window tables of level B
#ifdef MP_EXP_OVERLAP_MAX      // experiment hook (tools/ab_build.py): 0 = never
  uint32_t overlap_max = MP_EXP_OVERLAP_MAX;
#else
  uint32_t overlap_max = OVERLAP_MAX_BATCH;
#endif
  // work forked onto ctx->side: until the main stream has been made to wait for it (joined = true), an exception on the way out
  // must not leave kernels of this batch running on the shared arenas behind the caller's back
  struct SideGuard {
    mp_ctx* c;
    bool joined = false;
    ~SideGuard() {
      if (!joined) {
        try {
          rt::stream_sync(c->side);
        } catch (...) {
        }
      }
    }
  };
  // forks `side` off the context's stream; while it lives, kernel launches (which take their stream from the context) go to `side`
  struct SideFork {
    mp_ctx* c;
    rt::Stream keep;
    explicit SideFork(mp_ctx* ctx) : c(ctx), keep(ctx->stream) {
      rt::event_record(c->ev_fork, keep);
      c->stream = c->side;
      rt::stream_wait(c->side, c->ev_fork);
    }
    ~SideFork() { c->stream = keep; }
    SideFork(const SideFork&) = delete;
    SideFork& operator=(const SideFork&) = delete;
  };
  void prove_side_work(PlanSet& q, Workspace& w, uint32_t B, bool with_tables) {
    const ProveLay& l = q.pplan.lay;
    run_phase(q.pph[4], w, B);      // Toom-Cook (m = 2) / Karatsuba operand sums (empty when unused)
    const ToomPlan& tk = q.pplan.toom;
    if (tk.E) {                   // Toom-Cook, 3 <= m <= 16: the ciphertext polynomial at +-1 .. +-(m-1)
      ToomPointsArgs ta{w.P.p, w.J.p, w.Bpad, m, n, l.shuf, tk.cv_first};
      MP_RUN(k_toom_points, C, B, 2 * n, ta);
      normalize_flat(w.J.p + j_off<C>(tk.cv_first, w.Bpad, 0), w.P.p + p_off<C>(tk.cv_first, w.Bpad, 0), w.NS.p,
                     (size_t)(tk.E - 2) * 2 * n * w.Bpad);
    }
    if (with_tables) run_phase(q.pph[1], w, B, PH_TABLES);
  }

  // ---------------------------------------------------------------- prove
  // keys != nullptr: keyed batch -- proof b is made under the aggregate key keys[b] (one wire point each) instead of the
  // table's own key [REF mod.rs:380-418 takes shared_key per call; tables of different card tables differ in nothing else]
  void prove_dev(size_t B_, const uint8_t* decks, const uint8_t* rho, const uint32_t* perm, const uint8_t* seeds,
                 uint8_t* out_decks, uint8_t* out_proofs, int32_t* status, const uint8_t* keys, const mp_keyset* kset,
                 const uint32_t* kidx) override {
    const uint32_t B = (uint32_t)B_;
    const bool keyed = keys != nullptr || kset != nullptr;
    reserve_for(B, keyed);
    Workspace& w = ws;
    PlanSet& q = pick(B, keyed);
    cur_table_group = q.table_group;
    cur_norm_chunk = q.norm_chunk;
    const ProveLay& l = q.pplan.lay;
    PhaseDev* pph = q.pph;
    rt::Stream s = ctx->stream;
    FixedBases fb{n};
    const bool overlap = overlap_max && B <= overlap_max;      // two streams for the stretch before the first challenge
    SideGuard side_guard{ctx, !overlap};
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    {
      uint32_t* const ww = wire_words(w, B, 1);
      LoadPointsArgs a{decks, w.P.p, w.status.p, w.Bpad, 2 * N, l.deck, ww, 0};
      MP_RUN(k_load_points, C, B, 2 * N, a);
      LoadScalarsArgs sa{rho, w.S.p, w.status.p, w.Bpad, N, l.rho};
      MP_RUN(k_load_scalars, C, B, N, sa);
      ProveInitArgs ia{w.S.p, w.status.p, perm, seeds, q.draws.p, l, w.Bpad};
      if (!overlap) prove_init(ia, B);
      RemaskArgs ra{w.S.p, w.P.p, w.J.p, FB.p, perm, w.Bpad, N, l.rho, l.deck, l.shuf, fb.G(), fb.pk(), fbg,
                    0, w.D.p, w.T.p, key_d_first, key_t_first, nwin, nullptr, nullptr, FbGeom{8, 32, 255}, 0};
      if (!(validated & MP_VALIDATED_DECKS)) check_subgroup(w, B, l.deck, 2 * N);
      if (kset) {
        // the proof's key is a member of a key set: its multiples come from the set's tables, the key itself (transcript, its
        // own terms in the argument) from the set's copy of the wire bytes (validated when the set was built)
        keys = gather_keys(B, kset, kidx, w.status.p);
        LoadPointsArgs ka{keys, w.P.p, w.status.p, w.Bpad, 1, l.pk};
        MP_RUN(k_load_points, C, B, 1, ka);
        ra.keyed = 2;
        ra.KFB = kset->FB.p;
        ra.kidx = kidx;
        ra.kg = FbGeom{kset->bits, kset->windows, kset->entries};
        ra.nkeys = (uint32_t)kset->K;
        ra.live = kset->live.p;
      } else if (keyed) {
        // the proof's key -> window bases 2^(5w) pk -> their 16-entry tables; signed digits of the masking factors
        LoadPointsArgs ka{keys, w.P.p, w.status.p, w.Bpad, 1, l.pk};
        MP_RUN(k_load_points, C, B, 1, ka);
        check_subgroup(w, B, l.pk, 1);
        KeyWinArgs kw{w.P.p, w.J.p, w.Bpad, l.pk, l.kw, nwin};
        MP_RUN(k_key_windows, C, B, 1, kw);
        normalize_flat(w.J.p + j_off<C>(l.kw, w.Bpad, 0), w.P.p + p_off<C>(l.kw, w.Bpad, 0), w.NS.p, (size_t)nwin * w.Bpad);
        RecodeArgs rc{w.S.p, w.D.p, key_recode.p, w.Bpad, nwin};
        MP_RUN(k_recode, C, B, N, rc);
        TableArgs ta{w.P.p, w.T.p, w.NS.p, key_tables.p, w.Bpad, nwin, cur_table_group};
        MP_RUN(k_table, C, B, (nwin + cur_table_group - 1) / cur_table_group, ta);
        ra.keyed = 1;
      }
      // Everything up to the first challenge falls into two independent halves.  On `side`: the re-encryption, the shuffled deck
      // in affine form, the operand sums / Toom-Cook evaluations of its rows and the window tables of all of them -- none of it
      // depends on the prover's randomness or on a challenge.  On the main stream: the randomness, c_A, then (once the shuffled
      // deck is there) the statement hash and the scalar program behind it.  A batch that fills the chip gains nothing from
      // running them side by side; a small one hides its transcript lanes and ChaCha draws behind the group work, or the other way.
      if (overlap) {
        SideFork on_side(ctx);
        MP_RUN(k_remask, C, B, 2 * N, ra);
        run_phase(pph[0], w, B, PH_NORM, l.shuf);
        rt::event_record(ctx->ev_shuf, ctx->side);
        prove_side_work(q, w, B, true);
        rt::event_record(ctx->ev_tab, ctx->side);
      } else {
        MP_RUN(k_remask, C, B, 2 * N, ra);
      }
      if (overlap) {
        prove_init(ia, B);
        run_phase(pph[0], w, B, PH_ALL, NO_SLOT, l.shuf, w.NS2.p);
        rt::stream_wait(s, ctx->ev_shuf);
      } else {
        run_phase(pph[0], w, B);
        prove_side_work(q, w, B, false);
      }
    }
    const ToomPlan& tk = q.pplan.toom;
    {
      FsStatementArgs a = statement_args(w, l.deck, l.shuf, l.cA, l.x, keyed ? l.pk : NO_SLOT);
      a.W = wire_words(w, B, 1);
      a.w_deck = 0;             // the input deck as it came; the shuffled deck was computed here and is taken from its P slots
      run_fs_round1(a, B);
    }
    ProveScalArgs sc{w.S.p, perm, l, w.Bpad, q.lin.p, q.lin_src.p, tk.E ? 0u : (uint32_t)q.pplan.lin.size()};
    MP_RUN(k_prove_scal1, C, B, N, sc);
    MP_RUN(k_prove_scal1b, C, B, n + sc.n_lin * n, sc);
    MP_RUN(k_prove_scal1c, C, B, 1, sc);
    if (tk.E) {                   // the scalar polynomial at the same points; the interpolation matrix as MSM scalars
      LinCombArgs la{w.S.p, q.lin.p, q.lin_src.p, q.lin_coef.p, q.consts.p, w.Bpad, n};
      MP_RUN(k_lin_comb, C, B, (uint32_t)q.pplan.lin.size() * n, la);
      FillConstArgs fa{w.S.p, q.consts.p, w.Bpad, tk.w_first, tk.w_const_first};
      MP_RUN(k_fill_consts, C, B, tk.E * tk.E, fa);
    }
    if (keyed) {      // tau_k pk, k < 2m, from the key's own tables (the proof's, or its key set's): finished partial sums of the E_k
      KeyTermsArgs ka{w.S.p, w.J.p, w.Bpad, l.metau, q.pplan.jkey, kset ? 2u : 1u, w.T.p, key_t_first, nwin,
                      kset ? kset->FB.p : nullptr, kidx, kset ? FbGeom{kset->bits, kset->windows, kset->entries} : FbGeom{8, 32, 255},
                      kset ? (uint32_t)kset->K : 0u, kset ? kset->live.p : nullptr};
      MP_RUN(k_key_terms, C, B, 2 * m, ka);
    }
    if (overlap) {
      rt::stream_wait(s, ctx->ev_tab);
      side_guard.joined = true;
      run_phase(pph[1], w, B, PH_ALL & ~PH_TABLES);
    } else {
      run_phase(pph[1], w, B);
    }
    run_phase(pph[5], w, B);      // Toom-Cook interpolation: the diagonals E_k from the 2m products (empty otherwise)
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    {
      FsRoundArgs a{};
      a.f = f; a.S = w.S.p; a.P = w.P.p;
      a.step[0] = FsStep{l.cB, m, 0, 0, l.y, l.z};
      a.nsteps = 1;
      a.copy_from = NO_SLOT; a.copy_to = NO_SLOT;
      run_fs_round(a, B);
    }
    MP_RUN(k_prove_scal2, C, B, n + 1, sc);
    MP_RUN(k_prove_scal2b, C, B, n, sc);
    run_phase(pph[2], w, B);
    {
      FsRoundArgs a{};
      a.f = f; a.S = w.S.p; a.P = w.P.p;
      a.copy_from = l.cb; a.copy_to = l.hB + m - 1;
      a.step[0] = FsStep{l.cb, 1, 0, 0, NO_SLOT, NO_SLOT};
      a.step[1] = FsStep{l.hB, m, 0, 0, l.hx, l.hy};
      a.nsteps = 2;
      run_fs_round(a, B);
    }
    MP_RUN(k_prove_scal3, C, B, n + 1, sc);
    {      // small batches: the d_k as partial sums over column ranges first (kernels_proto.hpp; 0.1 -> 0.03 ms of a single proof)
      ProveScalArgs sd = sc;
      sd.d_parts = B <= SCAL3D_SPLIT_MAX_BATCH ? scal3d_parts(m, n) : 0u;
      if (sd.d_parts >= 2) {
        MP_RUN(k_prove_scal3d_part, C, B, (2 * m + 1) * sd.d_parts, sd);
      } else {
        sd.d_parts = 0;
      }
      MP_RUN(k_prove_scal3d, C, B, 2 * m + 1, sd);
    }
    run_phase(pph[3], w, B);
    {
      FsRoundArgs a{};
      a.f = f; a.S = w.S.p; a.P = w.P.p;
      a.copy_from = NO_SLOT; a.copy_to = NO_SLOT;
      a.step[0] = FsStep{l.zcA0, 2 + 2 * m + 1, 0, 0, l.zx, NO_SLOT};
      a.step[1] = FsStep{l.svcd, 3, 0, 0, l.svx, NO_SLOT};
      a.step[2] = FsStep{l.mecA0, 1 + 6 * m, 0, 0, l.mx, NO_SLOT};
      a.nsteps = 3;
      run_fs_round(a, B);
    }
    MP_RUN(k_prove_scal4, C, B, n + 3, sc);
    {
      StorePointsArgs a{out_decks, w.P.p, w.Bpad, 2 * N, l.shuf};
      MP_RUN(k_store_points, C, B, 2 * N, a);
      ProofIoArgs pa{out_proofs, w.S.p, w.P.p, w.status.p, q.pwire.p, w.Bpad, (uint32_t)proof_size_bytes(m, n, G_::PB)};
      MP_RUN(k_store_proof, C, B, (uint32_t)q.pplan.wire.size(), pa);
    }
    rt::d2d(status, w.status.p, (size_t)B * 4, s);
  }

  // ---------------------------------------------------------------- verify
  // Two passes.  (1) Screening: all group equations merged with random weights into ONE multi-scalar multiplication
  // (n + 5 fixed-base terms instead of one per equation and base, a quarter of the doubling chains) -- every honest batch
  // ends here.  (2) Only if some proof failed the screen: the equations one by one, to report the FIRST failing check by
  // name as the reference does [REF tests.rs:223-225].  A proof that passes (1) satisfies every equation except with
  // probability ~2^-250 over weights that depend on the whole proof.
  struct VArgs {
    uint32_t B;
    const uint8_t *decks, *shuf, *proofs;
    int32_t* status;
    const uint8_t* keys;
    const mp_keyset* kset;
    const uint32_t* kidx;
  };
  // a pipelined verify call whose screening verdict has not been looked at yet: k_verdict_merged writes the flag straight into a
  // page-locked host word (zero-copy; no copy call on the lane, which would make the runtime wait); it is valid once `ev` has passed
  struct Pending {
    VArgs v{};
    uint32_t* h_flag = nullptr;      // host address
    uint32_t* d_flag = nullptr;      // the same word as the device sees it
    rt::Event ev = nullptr;
    uint32_t gl = 0;                 // > 0: the screen was the equation of groups of gl proofs; their verdicts:
    uint32_t *h_gbad = nullptr, *d_gbad = nullptr;      // [gbad_cap] page-locked words the device writes directly (k_chain_verdict)
    size_t gbad_cap = 0;
  };
  std::deque<Pending> pend;          // oldest first; at most `pipeline` of them stay unexamined when a verify call returns
  std::vector<Pending> pend_pool;    // flag words and events for reuse
  Workspace vws;                     // the verify lane's arenas (pipelined mode: a prove call uses `ws` at the same time)
  static void release(Pending& p_) {
    if (p_.ev) rt::event_destroy(p_.ev);
    rt::host_free(p_.h_flag);
    rt::host_free(p_.h_gbad);
  }
  ~Table() {
    for (auto& p_ : pend_pool) release(p_);
    for (auto& p_ : pend) release(p_);
  }
  // ---- the stages the three screening passes (verify_pass, verify_group_pass, verify_chain_dev) are built from, on the context's
  // CURRENT lane.  Wire points of batch v -> P slots, proof scalars -> S slots: input deck, shuffled deck, proof [, the proof's key];
  // `wire`: the decks' wire words are kept for the transcript (wire_words: the small-batch plans of the per-proof passes)
  void load_verify_inputs(Workspace& w, PlanSet& q, const VArgs& v, bool vlane, bool wire) {
    const uint32_t B = v.B;
    const bool keyed = v.keys != nullptr || v.kset != nullptr;
    const VerifyLay& l = q.vplan.lay;
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, ctx->stream);
    uint32_t* const ww = wire ? wire_words(w, B, 2) : nullptr;
    LoadPointsArgs a{v.decks, w.P.p, w.status.p, w.Bpad, 2 * N, l.deck, ww, 0};
    MP_RUN(k_load_points, C, B, 2 * N, a);
    LoadPointsArgs b{v.shuf, w.P.p, w.status.p, w.Bpad, 2 * N, l.shuf, ww, wire ? 2 * N : 0};
    MP_RUN(k_load_points, C, B, 2 * N, b);
    ProofIoArgs pa{const_cast<uint8_t*>(v.proofs), w.S.p, w.P.p, w.status.p, q.vwire.p, w.Bpad, (uint32_t)proof_size_bytes(m, n, G_::PB)};
    MP_RUN(k_load_proof, C, B, (uint32_t)q.vplan.wire.size(), pa);
    if (keyed) {
      LoadPointsArgs ka{v.kset ? gather_keys(B, v.kset, v.kidx, w.status.p, vlane) : v.keys, w.P.p, w.status.p, w.Bpad, 1, l.pk};
      MP_RUN(k_load_points, C, B, 1, ka);
    }
    // decks and proof points are the P slots [0, pk); the key follows
    check_verify_inputs(w, B, l, keyed);
  }
  // the transcripts of the batch: challenges and (merge) the weights of the merged equation
  void run_transcripts(Workspace& w, PlanSet& q, uint32_t B, bool keyed, bool merged, bool wire) {
    const VerifyLay& l = q.vplan.lay;
    VerifyFsArgs a{};
    a.st = statement_args(w, l.deck, l.shuf, l.cA, l.x, keyed ? l.pk : NO_SLOT);
    if (wire) {
      a.st.W = wire_words(w, B, 2);
      a.st.w_deck = 0;
      a.st.w_shuf = 2 * N;
    }
    a.l = l;
    a.merge = merged ? 1u : 0u;
    run_verify_fs(a, B);
  }
  // the scalars of every proof's equations [, merged into those of its one equation]
  void run_verify_scalars(Workspace& w, PlanSet& q, uint32_t B, bool merged) {
    VerifyScalArgs sa{w.S.p, w.P.p, w.direct.p, q.vplan.lay, q.vplan.cm, w.Bpad};
    MP_RUN(k_verify_scal, C, B, n + 2, sa);
    if (merged) {
      VerifyMergeArgs ma{w.S.p, q.mjobs.p, q.mpairs.p, w.Bpad};
      MP_RUN(k_verify_merge, C, B, (uint32_t)q.vplan.mjobs.size(), ma);
    }
  }
  // one pass over a batch on the context's CURRENT lane: merged = the screening equation, else equation by equation
  void verify_pass(Workspace& w, const VArgs& v, bool merged, bool vlane, uint32_t* host_flag = nullptr) {
    const uint32_t B = v.B;
    const bool keyed = v.keys != nullptr || v.kset != nullptr;
    PlanSet& q = pick(B, keyed);
    cur_table_group = q.table_group;
    cur_norm_chunk = q.norm_chunk;
    const VerifyLay& l = q.vplan.lay;
    rt::Stream s = ctx->stream;
    load_verify_inputs(w, q, v, vlane, true);
    // The window tables of the verifier's bases need the loaded points and nothing else: batches that do not fill the chip build
    // them on `side` while the main stream hashes the transcript and derives the scalars (the table kernel leans on HBM, the
    // transcript lanes on latency: they do not compete)
    PhaseDev& ph = merged ? q.vmph : q.vph;
    const bool vtab_forked = overlap_max && B <= overlap_max && ph.n_tables != 0;
    SideGuard vguard{ctx, !vtab_forked};
    if (vtab_forked) {
      SideFork on_side(ctx);
      run_tables(ph, w, B, w.NS.p);
      rt::event_record(ctx->ev_tab, ctx->side);
    }
    run_transcripts(w, q, B, keyed, merged, true);
    run_verify_scalars(w, q, B, merged);
    if (vtab_forked) {
      rt::stream_wait(s, ctx->ev_tab);
      vguard.joined = true;
    }
    run_phase(ph, w, B, vtab_forked ? (PH_ALL & ~PH_TABLES) : PH_ALL);
    if (merged) {
      uint32_t* fl = host_flag;      // (already zero)
      if (!fl) fl = flag_word(vlane, s);
      VerdictMergedArgs a{w.J.p, w.direct.p, w.status.p, fl, w.Bpad, l.chk_merged};
      MP_RUN(k_verdict_merged, C, B, 1, a);
    } else {
      VerdictArgs a{w.J.p, w.direct.p, w.status.p, w.Bpad, l.chk_first};
      MP_RUN(k_verdict, C, B, 1, a);
    }
    rt::d2d(v.status, w.status.p, (size_t)B * 4, s);
  }
  // whether a batch of this size is screened with the merged equation first: small batches (the two finest splits) go straight to
  // the per-equation pass -- with an idle chip the merged MSM is one long dependency chain and its flag read-back a round trip; it
  // pays from the medium plan on (+3 % there, measured) -- unless the merged equation runs on the bucket kernel, which spreads ONE
  // MSM over windows x 64 lanes
  bool screens(uint32_t B, bool keyed) {
    const int plan = plan_of(B);
    return merged_verify && (plan != 3 || pick(B, keyed).vmph.n_b);
  }
  // ---- round 5: a failing screen costs what the rejected proofs cost, not what the batch costs.  Every screen says WHICH proofs it
  // could not clear -- k_verdict_merged marks them 1, k_chain_verdict writes one word per group / chain --, their inputs are gathered
  // into a contiguous sub-batch (k_gather_rows), the sub-batch takes the next finer pass and its status words are scattered back:
  //   level 0  the suspects of failing groups: equations of sub-groups an eighth the size (16 proofs of a 52-card deck) when there are
  //            enough of them to fill the bucket kernel (>= 128 sub-groups), else straight to level 1;
  //   level 1  equation by equation: the FIRST failing check by name, exactly as the reference reports it [REF tests.rs:223-225].
  // Everybody else's verdict stands.  One tampered proof among 262 144 re-verifies 128 proofs, not 262 144.
  struct SubBatch {
    DevBuf<uint32_t> decks, shuf, proofs, keys, kidx, idx;
    DevBuf<int32_t> status;
  };
  SubBatch sub[2][3];                 // [lane][depth of the refinement]
  Workspace rws[2];                   // [lane] arenas of the per-equation passes over sub-batches (sized by the sub-batch, not by the batch)
  DevBuf<uint32_t> gbad[2];           // per-group verdicts of a group / chain pass on the caller's lane, on the verify lane
  uint32_t refine_points = 0;         // points per sub-group equation (mp_set_group_refine; 0 = an eighth of the group equation's)
  uint32_t refine_min = 128;          // fewer sub-groups than this: straight to the per-equation pass
  uint64_t n_reverified = 0;          // proofs that went through a per-equation pass because a screen could not clear them
  void set_group_refine(uint32_t points, uint32_t min_groups) override {
    refine_points = points;
    refine_min = min_groups ? min_groups : 128u;
  }
  uint64_t reverified() const override { return n_reverified; }
  // proofs per sub-group for the nsub suspects a screen with groups of l1 proofs left (l1 = 0: no groups above, e.g. a chain)
  // `crowded`: (nearly) every group of the screen above failed -- the rate of bad proofs is beyond what an eighth of such a group could
  // clear (round 6: 1 % of bad proofs fails every group of 1 024 and three in four of 128): a sixty-fourth instead
  uint32_t subgroup_size(size_t nsub, bool keyed, uint32_t l1, bool crowded = false) const {
    const uint32_t per = 4 * N + 11 * m + 8 + (keyed ? 1u : 0u);
    if (!group_points || !merged_verify) return 0;
    // (a sub-group equation costs 0.55 us per proof at 32 proofs, 0.73 at 16, 0.85 at 8, 1.1 at 4 -- the per-equation pass 1.2: an eighth
    // of a group of fewer than 64 proofs is not worth an equation of its own; profiles/r05h_rejection_strategies.txt)
    if (!refine_points && l1 && l1 < 64) return 0;
    const uint32_t pts = refine_points ? refine_points : (l1 ? l1 * per : group_points) / (crowded && l1 >= 512 ? 64u : 8u);
    const uint32_t want = (uint32_t)std::min<uint64_t>((pts + per / 2) / per, 1023u);
    if (want < 2 || (l1 && want >= l1) || (uint64_t)want * per + n + 5 > BUCKET_TERMS_MAX || nsub < (uint64_t)refine_min * want) return 0;
    return want;
  }
  void gather_rows(const void* src, DevBuf<uint32_t>& dst, const uint32_t* d_idx, size_t rows, size_t row_bytes) {
    const uint32_t words = (uint32_t)(row_bytes / 4);
    dst.alloc(rows * words, ctx->stream, false);
    const size_t slice = std::max<size_t>(1, ((size_t)1 << 30) / words);      // (thread index: 32 bits)
    for (size_t r0 = 0; r0 < rows; r0 += slice) {
      const size_t rc = std::min(slice, rows - r0);
      GatherRowsArgs ga{reinterpret_cast<const uint32_t*>(src), dst.p + r0 * words, d_idx + r0, words};
      MP_RUN(k_gather_rows, C, (uint32_t)(rc * words), 1, ga);
    }
  }
  // the positions of the non-zero words among `count` device (or mapped host) words, on the context's current lane
  void read_words(const void* d_words, size_t count, std::vector<uint32_t>& host) {
    host.resize(count);
    rt::d2h(host.data(), d_words, count * 4, ctx->stream);
    rt::stream_sync(ctx->stream);
  }
  // members of the failing groups (lane of (member j, group t) = j T + t)
  static void group_members(const uint32_t* bad, uint32_t T, uint32_t L, std::vector<uint32_t>& idx) {
    idx.clear();
    for (uint32_t t = 0; t < T; ++t)
      if (bad[t])
        for (uint32_t j = 0; j < L; ++j) idx.push_back(j * T + t);
    std::sort(idx.begin(), idx.end());
  }
  // what a screen of T equations of L proofs each could not clear: the members of the failing equations through the finer passes
  // (verify_subset: level, l1, own_arenas, depth), nobody else.  `bad`: one verdict word per equation -- device words, or (mapped) the
  // page-locked words a pipelined screen wrote, valid already.  note: the group sizes adapt to what this screen saw.  Returns the suspects
  std::vector<uint32_t> refine_groups(const VArgs& v, const uint32_t* bad, bool mapped, uint32_t T, uint32_t L, bool vlane, bool note,
                                      int level, uint32_t l1, bool own_arenas = true, uint32_t depth = 0) {
    std::vector<uint32_t> words, idx;
    if (!mapped) {
      read_words(bad, T, words);
      bad = words.data();
    }
    group_members(bad, T, L, idx);
    if (note) note_group_verdicts(T, (uint32_t)(idx.size() / L), L);
    verify_subset(v, idx, level, vlane, l1, own_arenas, depth);
    return idx;
  }
  // the proofs idx[] of batch v (ascending) through the finer passes; their status words replace the screen's marks
  // own_arenas: the caller's arenas (ws) are laid out for batch v (verify_dev); a chain call's are not (its lean workspace is cws)
  // depth: how many sub-batches lie above this one (each has gather buffers of its own: sub[lane][depth])
  void verify_subset(const VArgs& v, std::vector<uint32_t>& idx, int level, bool vlane, uint32_t l1 = 0, bool own_arenas = true, uint32_t depth = 0,
                     int crowd = -1) {
    if (depth >= 2) level = 1;
    // (the suspects are whole groups of l1: if they are nearly the whole batch, nearly every group failed -- judged before any slicing)
    const bool crowded = crowd >= 0 ? crowd != 0 : (l1 != 0 && idx.size() * 20 >= (size_t)v.B * 19);
    if (idx.empty()) return;
    const bool keyed = v.keys != nullptr || v.kset != nullptr;
    rt::Stream s = ctx->stream;
    // Bounded memory whatever the number of suspects (one bad link per chain equation sends all T x L links of a call here):
    // at most 131 072 52-card proofs' worth of them are gathered and looked at at a time (2.6 GB of decks and proofs, arenas of the passes
    // below for that many lanes); the slices are sub-batches of their own, any partition of the suspects gives the same status words
    const size_t sub_max = std::max<size_t>(4096, ((size_t)131072 * 52u / N) & ~(size_t)1023);
    if (!(level == 1 && idx.size() == v.B && (vlane || own_arenas)) && idx.size() > sub_max) {
      for (size_t o = 0; o < idx.size(); o += sub_max) {
        std::vector<uint32_t> part(idx.begin() + o, idx.begin() + std::min(idx.size(), o + sub_max));
        verify_subset(v, part, level, vlane, l1, own_arenas, depth, crowded ? 1 : 0);
      }
      return;
    }
    const uint32_t L2 = level == 0 ? subgroup_size(idx.size(), keyed, l1, crowded) : 0u;
    if (!L2) level = 1;
    // The equations of a sub-batch run on arenas of their OWN (rws), in slices of at most 32 768 52-card proofs: the work split follows
    // the size of the sub-batch (128 suspects take the finest split), and a split with more table / digit slots per proof than the
    // caller's must not grow the caller's arenas -- those are laid out for 262 144 lanes, and re-allocating them cost the first rejected
    // proof of a session 3.5 s (measured).  Bounded memory (~20 GB at the most), cost proportional to the suspects.
    auto per_equation = [&](const VArgs& a) {
      Workspace& w = rws[vlane ? 1 : 0];
      const uint32_t slice = std::max<uint32_t>(64u, (uint32_t)(((uint64_t)32768 * 52u / N) & ~63ull));
      const size_t dsz = (size_t)2 * N * G_::PB, psz = proof_size_bytes(m, n, G_::PB);
      n_reverified += a.B;
      for (uint32_t s0 = 0; s0 < a.B; s0 += slice) {
        const uint32_t sc = std::min(slice, a.B - s0);
        const VArgs ss{sc, a.decks + (size_t)s0 * dsz, a.shuf + (size_t)s0 * dsz, a.proofs + (size_t)s0 * psz, a.status + s0,
                       a.keys ? a.keys + (size_t)s0 * G_::PB : nullptr, a.kset, a.kidx ? a.kidx + s0 : nullptr};
        reserve_ws(w, sc, keyed);
        verify_pass(w, ss, false, vlane);
      }
    };
    if (level == 1 && idx.size() == v.B) {      // (everybody: no gather)
      if (vlane || !own_arenas) {               // (no arenas of the batch's size for the equations on the verify lane or under a chain call: slices)
        per_equation(v);
      } else {                                  // (the caller's arenas are laid out for this batch and its work split already)
        reserve_ws(ws, v.B, keyed);
        n_reverified += v.B;
        verify_pass(ws, v, false, false);
      }
      return;
    }
    const uint32_t distinct = (uint32_t)idx.size();
    if (L2)
      while (idx.size() % L2) idx.push_back(idx[0]);      // (a suspect twice: the same verdict written twice)
    const uint32_t nsub = (uint32_t)idx.size();
    SubBatch& sb = sub[vlane ? 1 : 0][depth];
    sb.idx.upload(idx, s);
    gather_rows(v.decks, sb.decks, sb.idx.p, nsub, (size_t)2 * N * G_::PB);
    gather_rows(v.shuf, sb.shuf, sb.idx.p, nsub, (size_t)2 * N * G_::PB);
    gather_rows(v.proofs, sb.proofs, sb.idx.p, nsub, proof_size_bytes(m, n, G_::PB));
    if (v.kset) gather_rows(v.kidx, sb.kidx, sb.idx.p, nsub, 4);
    else if (v.keys) gather_rows(v.keys, sb.keys, sb.idx.p, nsub, G_::PB);
    sb.status.alloc(nsub, s, false);
    const VArgs sv{nsub, reinterpret_cast<const uint8_t*>(sb.decks.p), reinterpret_cast<const uint8_t*>(sb.shuf.p),
                   reinterpret_cast<const uint8_t*>(sb.proofs.p), sb.status.p,
                   v.keys && !v.kset ? reinterpret_cast<const uint8_t*>(sb.keys.p) : nullptr, v.kset, v.kset ? sb.kidx.p : nullptr};
    if (L2) {
      const uint32_t T2 = nsub / L2;
      DevBuf<uint32_t>& gb = gbad[vlane ? 1 : 0];
      gb.alloc(T2, s, false);
      verify_group_pass(sv, L2, vlane, nullptr, gb.p);
      if (read_flag(vlane)) {
        // (the members of the failing sub-groups: through sub-groups an eighth the size once more if there are enough of them -- 1 024 ->
        // 128 -> 16 --, else equation by equation)
        for (uint32_t i2 : refine_groups(sv, gb.p, false, T2, L2, vlane, false, L2 >= 64 ? 0 : 1, L2, true, depth + 1))
          if (i2 >= distinct) n_reverified -= 1;          // (mp_reverified_count counts proofs, not the copies that fill the last sub-group)
      }
    } else {
      per_equation(sv);
    }
    ScatterStatusArgs sa{sb.status.p, v.status, sb.idx.p};
    MP_RUN(k_scatter_status, C, nsub, 1, sa);
    rt::stream_sync(s);      // (idx[] was uploaded from pageable memory and sb is reused by the next failing batch)
  }
  // the proofs a per-proof screen marked (status word 1) through the per-equation pass
  void refine_marked(const VArgs& v, bool vlane) {
    std::vector<uint32_t> st, idx;
    read_words(v.status, v.B, st);
    for (uint32_t b = 0; b < v.B; ++b)
      if ((int32_t)st[b] == 1) idx.push_back(b);
    verify_subset(v, idx, 1, vlane);
  }
  void verify_dev(size_t B_, const uint8_t* decks, const uint8_t* shuf, const uint8_t* proofs, int32_t* status,
                  const uint8_t* keys, const mp_keyset* kset, const uint32_t* kidx) override {
    const VArgs v{(uint32_t)B_, decks, shuf, proofs, status, keys, kset, kidx};
    const bool keyed = keys != nullptr || kset != nullptr;
    if (keyed) ensure_keyed();
    const uint32_t gl = group_size(v.B, keyed);      // > 0: the screen is one equation per group of gl proofs (bucket kernel)
    if (pipeline) {
      // Pipelined mode: the call runs on the verify lane with arenas of its own and does NOT wait for its screening verdict, so the
      // caller's next prove call overlaps it on the chip.  The verdict of call k is looked at when call k + 1 comes in (or at
      // mp_sync); only then -- and only for the proofs the screen could not clear -- do the finer passes run.
      resolve_pending((size_t)pipeline - 1);      // this call makes it `pipeline` unexamined ones
      rt::event_record(ctx->ev_vin, ctx->stream);
      LaneSwap lane(ctx);
      rt::stream_wait(ctx->stream, ctx->ev_vin);
      // (the verify lane's arenas are sized ON the verify lane: a zero-fill of theirs must queue behind the verify work in flight)
      if (!gl) reserve_ws(vws, v.B, keyed);
      if (!gl && !screens(v.B, keyed)) {
        verify_pass(vws, v, false, true);
        return;
      }
      Pending pn;
      if (!pend_pool.empty()) {
        pn = pend_pool.back();
        pend_pool.pop_back();
      } else {
        void* dp = nullptr;
        pn.h_flag = (uint32_t*)rt::host_alloc_mapped(4, &dp);
        pn.d_flag = (uint32_t*)dp;
        pn.ev = rt::event_create();
      }
      pn.v = v;
      pn.gl = gl;
      *pn.h_flag = 0;
      if (gl && pn.gbad_cap < v.B / gl) {
        rt::host_free(pn.h_gbad);
        pn.h_gbad = nullptr;
        pn.gbad_cap = 0;
        void* dp = nullptr;
        pn.h_gbad = (uint32_t*)rt::host_alloc_mapped((size_t)(v.B / gl) * 4, &dp);
        pn.d_gbad = (uint32_t*)dp;
        pn.gbad_cap = v.B / gl;
      }
      pend.push_back(pn);                   // (before the launches: an exception on the way still leaves the slot owned)
      if (gl) verify_group_pass(v, gl, true, pn.d_flag, pn.d_gbad);
      else verify_pass(vws, v, true, true, pn.d_flag);
      rt::event_record(pn.ev, ctx->stream);
      return;
    }
    if (gl) {
      const uint32_t T = v.B / gl;
      gbad[0].alloc(T, ctx->stream, false);
      verify_group_pass(v, gl, false, nullptr, gbad[0].p);
      if (!read_flag(false)) {              // every group's equation holds
        note_group_verdicts(T, 0, gl);
        return;
      }
      refine_groups(v, gbad[0].p, false, T, gl, false, true, 0, gl);
      return;
    }
    reserve_for(v.B, keyed);
    // Two passes.  (1) Screening; every honest batch ends here.  (2) The proofs the screen marked, equation by equation
    if (!screens(v.B, keyed)) {
      verify_pass(ws, v, false, false);
      return;
    }
    verify_pass(ws, v, true, false);
    if (read_flag(false)) refine_marked(v, false);
  }
  // look at the screening verdicts of all but the `keep` most recent pipelined verify calls
  void resolve_pending(size_t keep) {
    while (pend.size() > keep) {
      Pending pn = pend.front();
      pend.pop_front();
      pend_pool.push_back(pn);
      rt::event_sync(pn.ev);
      if (!*pn.h_flag) {
        if (pn.gl) note_group_verdicts(pn.v.B / pn.gl, 0, pn.gl);
        continue;
      }
      LaneSwap lane(ctx);
      if (pn.gl) {
        refine_groups(pn.v, pn.h_gbad, true, pn.v.B / pn.gl, pn.gl, true, true, 0, pn.gl);
      } else {
        refine_marked(pn.v, true);          // the proofs the screen marked: the first failing check of each
      }
      rt::stream_sync(ctx->stream);
    }
  }
  void flush() override {
    resolve_pending(0);
    if (ctx->vstream) rt::stream_sync(ctx->vstream);
  }


  // ---------------------------------------------------------------- chain verification
  // The L shuffles of one card table form a chain (deck_{j+1} = output of link j [REF examples/round.rs:268-350]) and every one of
  // them is verified.  Checked one by one, each of the L - 1 inner decks is a base in TWO verifier equations (as the shuffled deck
  // of link j - 1 and as the input deck of link j).  Here the merged equations of all links of a table are added up with weights
  // rho_j that depend on every proof of the chain: every distinct point appears ONCE -- (L + 1) 2N deck points + L (11m + 8) proof
  // points instead of L (4N + 11m + 8) -- the n + 5 fixed bases appear once per table instead of once per link, and the resulting
  // MSM (4 424 terms for 32 links of a 52-card deck) is long enough for the bucket kernel.  A table whose chain fails is re-verified
  // link by link, so the per-link status words are exactly those of verify_dev.  T tables, lane of (link j, table t) = j T + t.
  struct ChainPlan {
    uint32_t L = 0, G = 0;
    bool keyed = false;
    Phase ph;
    PhaseDev dev;
    std::vector<ChainTerm> cterms;
    DevBuf<ChainTerm> dterms;
    uint32_t K = 0, nfix = 0, nJ = 0;
    std::vector<uint32_t> tile_src;     // chain equations (round 6): slot | link << 20 of term i -- where k_chain_tile finds the point of entry i of the equation's run
    DevBuf<uint32_t> dtile_src;
  };
  ChainPlan chain;
  Workspace cws;                      // lean workspace of chain verification: no window tables, no digit planes
  DevBuf<uint32_t> chain_cw, chain_cs, chain_dig, chain_part;
  // the verdicts of T chain / group equations of L links (kernels_proto.hpp: per link, per equation, then the caller's status words)
  void run_chain_verdict(ChainVerdictArgs va) {
    chain_part.alloc(va.T, ctx->stream, false);
    rt::dzero(chain_part.p, (size_t)va.T * 4, ctx->stream);
    va.part = chain_part.p;
    MP_RUN(k_chain_check, C, va.T * va.L, 1, va);
    MP_RUN(k_chain_verdict, C, va.T, 1, va);
    if (va.out) MP_RUN(k_chain_mark, C, va.T * va.L, 1, va);
  }
  // the weights of T chain / group equations of L links each (kernels_proto.hpp: block digests, then table key, block key, 64 weights per lane)
  void run_chain_weights(Workspace& w, uint32_t Tpad, uint32_t T, uint32_t L) {
    const uint32_t nb = (L + CW_BLOCK - 1) / CW_BLOCK;
    chain_dig.alloc((size_t)nb * 8 * Tpad, ctx->stream, false);
    ChainWeightsArgs wa{w.seed.p, chain_cw.p, chain_dig.p, w.Bpad, Tpad, T, L};
    MP_RUN(k_chain_digest, C, T, nb, wa);
    MP_RUN(k_chain_weights, C, T, nb, wa);
  }
  DevBuf<int16_t> chain_d8;
  // Tables per chain equation (round 5).  One table's chain is 4 424 points for 32 links of a 52-card deck: 8-bit windows (32 per
  // scalar) and a wave-wide reduction per window that is a sixth of its additions.  The chains of G tables added up with the same kind
  // of weights (they depend on every proof of every member) are ONE equation of G x 4 424 points: 10-bit windows (26 per scalar), the
  // reduction spread over G times the terms, the fixed bases once per G tables -- what group verification does for independent proofs.
  // Member g of equation e is table g (T / G) + e, so that link j of member g is lane (j G + g)(T / G) + e: the plan below is the
  // chain plan with "links" j G + g and a chain's consecutive links G apart; kernels and lane formula are unchanged.  A failing
  // equation sends ITS G x L links through the per-link verifier.  G = the divisor of T that brings the equation nearest to the
  // group equation's size (mp_set_group_verify), with enough equations left to keep the persistent waves busy; 1 = a table on its own.
  // members per equation: the divisor of `total` nearest to `want` (between half and twice it) whose equation -- `per` points a member
  // and the n + 5 fixed bases -- fits one bucket job (65 535 points) and passes `fits`; 0 = there is none
  template <class Fits>
  uint32_t nearest_divisor(uint32_t total, uint32_t want, uint32_t per, Fits fits) const {
    for (uint32_t d = 0; d <= want; ++d)
      for (int sgn = 1; sgn >= -1; sgn -= 2) {
        const int64_t L = (int64_t)want + sgn * (int64_t)d;
        if (L < 2 || 2 * L < (int64_t)want || L > 2 * (int64_t)want || (uint64_t)L * per + n + 5 > BUCKET_TERMS_MAX || !fits((uint32_t)L)) continue;
        if (total % (uint32_t)L == 0) return (uint32_t)L;
      }
    return 0;
  }
  uint32_t chain_points_per_table(uint32_t L, bool keyed) const { return (L + 1) * 2 * N + L * (11 * m + 8) + (keyed ? 1u : 0u); }
  uint32_t chain_group_of(uint32_t T, uint32_t L, bool keyed) const {
    // (an explicit mp_set_chain_group is honoured whatever mp_set_group_verify says; the automatic rule follows the group equations')
    if (chain_group == 1 || (!chain_group && !group_points && !group_points_wg)) return 1;
    const uint32_t per = chain_points_per_table(L, keyed);
    uint32_t want = chain_group;
    if (!want) {
      const uint32_t eq_min = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)group_min_batch * 2u) / 13u));
      want = std::min<uint32_t>((group_points + per / 2) / per, T / eq_min);
      // (round 6, as group_size: equations for the split pipeline if at least min_batch / 48 of them, of at least 50 000 points, are left
      // -- 64 tables x 4 392 points for 32 links of a 52-card deck)
      const uint32_t want_wg = std::min<uint32_t>((group_points_wg + per / 2) / per, T / std::max<uint32_t>(1u, group_min_batch / 512u));
      if (group_points_wg && (uint64_t)want_wg * per >= GROUP_WG_POINTS_MIN) want = std::max(want, want_wg);
    }
    if (want < 2) return 1;
    // (12 bits of link in a term's tile source: k_chain_tile)
    const uint32_t G = nearest_divisor(T, want, per, [&](uint32_t g) { return (uint64_t)g * (L + 1) <= 4094; });
    return G ? G : 1;
  }
  // The plan of an equation over `links` lanes: ONE bucket MSM over K distinct points + the fixed-base part.  `terms(var)` enumerates the
  // K variable terms -- var(term, point): where chains and groups differ --; shared: the window width from K, the fixed bases (the scalar of
  // one is a sum over the equation's links, one lane adding them up in k_chain_scalars: in runs of at most 64 -- a base then appears
  // ceil(links / 64) times in the fixed-base part -- so that no lane of that kernel runs 1 024 products in a row), counts and uploads
  template <class Terms>
  void build_equation_plan(ChainPlan& p, const VerifyLay& l, uint32_t L, uint32_t G, bool keyed, uint32_t K, uint32_t links, Terms terms) {
    p.ph = Phase();
    p.cterms.clear();
    p.tile_src.clear();
    p.L = L;
    p.G = G;
    p.keyed = keyed;
    uint32_t next_partial = 1;                  // J slot 0 = the equation's value
    const uint32_t bits = bucket_bits_of(K);
    PhaseBuilder pb(p.ph, next_partial, FCHUNK, VCHUNK, 1u, bk_windows(R::BITS, bits), 1u, bits);
    pb.begin(0);
    terms([&](ChainTerm ct, uint32_t point) {
      pb.var((uint32_t)p.cterms.size(), point);
      p.cterms.push_back(ct);
    });
    p.K = (uint32_t)p.cterms.size();
    FixedBases fb{n};
    for (uint32_t f = 0; f < fb.count(); ++f) {
      if (keyed && f == fb.pk()) continue;
      for (uint32_t j0 = 0; j0 < links; j0 += 64u) {
        pb.fixed((uint32_t)p.cterms.size(), f);
        p.cterms.push_back(ChainTerm{l.mfix + f, j0, std::min(64u, links - j0), NO_SLOT, 1});
      }
    }
    p.nfix = (uint32_t)p.cterms.size() - p.K;
    pb.end();
    p.nJ = next_partial;
    p.dev.upload(p.ph, ctx->stream);
    p.dterms.upload(p.cterms, ctx->stream);
  }
  void build_chain_plan(uint32_t L, bool keyed, uint32_t G = 1) {
    if (chain.L == L && chain.keyed == keyed && chain.G == G) return;
    if (keyed) ensure_keyed();
    const VerifyLay& l = (keyed ? psk : ps)[0].vplan.lay;
    build_equation_plan(chain, l, L, G, keyed, G * ((L + 1) * 2 * N + L * (l.pk - l.cA) + (keyed ? 1u : 0u)), L * G, [&](auto term) {
      // (a term's point: its index in the equation's contiguous run -- k_chain_tile copies it there from slot | link << 20)
      auto var = [&](ChainTerm ct, uint32_t pslot, uint32_t link) {
        chain.tile_src.push_back(pslot | (link << 20));
        term(ct, (uint32_t)chain.cterms.size());
      };
      // ("link" j G + g of the equation = link j of member g)
      for (uint32_t g = 0; g < G; ++g)
        for (uint32_t j = 0; j <= L; ++j)
          for (uint32_t i = 0; i < 2 * N; ++i) {
            if (j == 0) var(ChainTerm{l.mvar + l.deck + i, g, 1, NO_SLOT, G}, l.deck + i, g);
            else if (j < L) var(ChainTerm{l.mvar + l.deck + i, j * G + g, 1, l.mvar + l.shuf + i, G}, l.deck + i, j * G + g);
            else var(ChainTerm{l.mvar + l.shuf + i, (L - 1) * G + g, 1, NO_SLOT, G}, l.shuf + i, (L - 1) * G + g);
          }
      for (uint32_t j = 0; j < L * G; ++j)
        for (uint32_t slot = l.cA; slot < l.pk; ++slot) var(ChainTerm{l.mvar + slot, j, 1, NO_SLOT, 1}, slot, j);
      if (keyed)
        for (uint32_t g = 0; g < G; ++g) var(ChainTerm{l.mvar + l.pk, g, L, NO_SLOT, G}, l.pk, g);      // one key term per member
    });
    chain.dtile_src.upload(chain.tile_src, ctx->stream);
  }
  size_t chain_lane_bytes(uint32_t, bool keyed) override {
    if (keyed) ensure_keyed();
    const VerifyLay& l = (keyed ? psk : ps)[0].vplan.lay;
    // J slots of a chain plan: the equation's value, the bucket job's result and one partial sum per window (at most 33 of 8 bits), the
    // fixed-base part -- whatever the number of links or of tables per equation (build_chain_plan; Workspace::ensure takes at least 8)
    const size_t fwb = (size_t)G_::FW * 4, nJ = 4 + bk_windows(R::BITS, 8);
    // (Workspace::ensure: S, P, J, one window-table row and digit plane it always keeps, inversion scratch, stage, seed, direct, status, digits)
    return (size_t)l.nS * 32 + (size_t)l.nP * 2 * fwb + nJ * 3 * fwb + nwin + (size_t)VB_ENTRIES * 2 * fwb + nJ * fwb + (size_t)stage_words_needed() * 4 + 32 + 8 + 4 + 8;
  }
  size_t chain_lanes_held() const override { return cws.cap; }
  uint32_t chain_group_size(size_t T, uint32_t L, bool keyed) const override { return T < 0x7FFFFFFFu ? chain_group_of((uint32_t)T, L, keyed) : 1u; }
  // ---- the equation stages of a chain / group pass: T equations of L links each over plan p, lane of (link j, equation t) = j T + t.
  // Room for the weights, the scalars of the terms and their bucket digits (before the weights are drawn)
  void size_equations(const ChainPlan& p, uint32_t T, uint32_t L) {
    const uint32_t Tpad = (T + 63u) & ~63u;
    chain_cw.alloc((size_t)L * Tpad * 8, ctx->stream, false);
    chain_cs.alloc((size_t)(p.K + p.nfix) * Tpad * 8, ctx->stream);
    chain_d8.alloc((size_t)p.dev.b_dig_bytes * Tpad, ctx->stream);
  }
  // what the equations of a chain pass and of a group pass do not share
  struct EquationArgs {
    uint32_t T, L;
    bool vlane;
    const char* too_many;      // (what run_bucket says when T is beyond one launch)
    uint32_t pk, G;            // ChainVerdictArgs: the key's P slot (chains whose links share it), tables per equation
    uint32_t* flag;            // raised if some equation fails (null: the lane's flag word)
    uint32_t* gbad;            // [T] which (null: the lane's gbad[] words, sized here)
    int32_t* status;           // the caller's status words
  };
  // With weights (run_chain_weights) and the proofs' merged scalars in place: one scalar per distinct point / fixed base, the points as one
  // contiguous run per equation (tile(run): k_chain_tile / k_group_tile; tiled = false: the bucket kernel takes them from their P slots),
  // ONE bucket MSM + fixed-base part per equation, the verdicts: flag, gbad[t], and in e.status 0 for every link of an equation that holds
  // (final), MP_ERR_INTERNAL for those of the others until the finer passes have given each its own word
  // the value of T equations into J slot 0 of the lanes 0 .. T - 1 of w: scalars cs [terms][Tpad], ONE bucket MSM + fixed-base part each
  // (shared by the equations of chains and groups and by those of the sigma screen)
  void run_equation_msm(Workspace& w, PhaseDev& ph, const uint32_t* cs, int16_t* d8, uint32_t T, const char* too_many, const uint32_t* run, uint32_t K) {
    const uint32_t Tpad = (T + 63u) & ~63u;
    run_bucket(w, ph, cs, Tpad, d8, (size_t)ph.b_dig_bytes, T, T, too_many, run, K);
    FixedArgs fx{cs, w.J.p, FB.p, ph.fjobs.p, ph.fterms.p, w.Bpad, fbg, Tpad};
    MP_RUN(k_fixed_msm, C, T, ph.n_f, fx);
    if (ph.n_c0) {
      CombineArgs cb0{w.J.p, w.P.p, ph.cjobs0.p, ph.cterms0.p, w.Bpad};
      MP_RUN(k_combine, C, T, ph.n_c0, cb0);
    }
    CombineArgs cb{w.J.p, w.P.p, ph.cjobs.p, ph.cterms.p, w.Bpad};
    MP_RUN(k_combine, C, T, ph.n_c, cb);
  }
  template <class Tile>
  void run_equations(Workspace& w, ChainPlan& p, const EquationArgs& e, bool tiled, Tile tile) {
    const uint32_t T = e.T, Tpad = (T + 63u) & ~63u, nterms = p.K + p.nfix;
    rt::Stream s = ctx->stream;
    ChainScalArgs ca{w.S.p, chain_cw.p, chain_cs.p, p.dterms.p, w.Bpad, Tpad, T};
    MP_RUN(k_chain_scalars, C, T, nterms, ca);
    PhaseDev& ph = p.dev;
    const uint32_t* run = nullptr;
    if (tiled) {
      DevBuf<uint32_t>& gt = gtile[e.vlane ? 1 : 0];
      gt.alloc((size_t)T * p.K * G_::PW, s, false);
      tile(gt.p);
      run = gt.p;
    }
    run_equation_msm(w, ph, chain_cs.p, chain_d8.p, T, e.too_many, run, p.K);
    uint32_t* gb = e.gbad;
    if (!gb) {
      gbad[e.vlane ? 1 : 0].alloc(T, s, false);
      gb = gbad[e.vlane ? 1 : 0].p;
    }
    ChainVerdictArgs va{w.J.p, w.direct.p, w.status.p, e.flag ? e.flag : flag_word(e.vlane, s), gb, w.Bpad, T, e.L, 0u, w.P.p, e.pk, e.G, e.status, nullptr};
    run_chain_verdict(va);
  }
  void verify_chain_dev(size_t T_, uint32_t L, const uint8_t* decks, const uint8_t* proofs, int32_t* status, const uint8_t* keys) override {
    const uint32_t T = (uint32_t)T_, B = T * L;
    const bool keyed = keys != nullptr;
    // G tables per equation: Tq equations of Lq "links" each, lane of (link, equation) = link Tq + equation as before
    const uint32_t G = chain_group_of(T, L, keyed), Tq = T / G, Lq = L * G;
    build_chain_plan(L, keyed, G);
    PlanSet& q = (keyed ? psk : ps)[0];
    const VerifyLay& l = q.vplan.lay;
    Workspace& w = cws;
    w.fw = G_::FW;
    w.ensure(B, l.nS, l.nP, std::max(chain.nJ, 8u), 0, 0, nwin, stage_words_needed(), ctx->stream, 0);
    // (link j of table t: deck row j T + t, shuffled deck row (j + 1) T + t -- the same index into the array one deck further on)
    const VArgs cv{B, decks, decks + (size_t)T * 2 * N * G_::PB, proofs, status, keys, nullptr, nullptr};
    load_verify_inputs(w, q, cv, false, false);
    run_transcripts(w, q, B, keyed, true, false);
    run_verify_scalars(w, q, B, true);
    // the chain equation: weights, one scalar per distinct point / fixed base, ONE bucket MSM + fixed-base part per table
    size_equations(chain, Tq, Lq);
    run_chain_weights(w, (Tq + 63u) & ~63u, Tq, Lq);
    const EquationArgs e{Tq, Lq, false, "chain verification: too many tables for one launch", keyed ? l.pk : NO_SLOT, G, nullptr, nullptr, status};
    run_equations(w, chain, e, true, [&](uint32_t* run) {
      ChainTileArgs ta{w.P.p, run, chain.dtile_src.p, w.Bpad, Tq, chain.K};
      if ((uint64_t)Tq * chain.K >= ((uint64_t)1 << 32)) throw std::runtime_error("chain verification: too many tables for one launch");
      MP_RUN(k_chain_tile, C, Tq * chain.K, 1, ta);
    });
    if (!read_flag(false)) return;
    // some equation failed: the per-link verifier gives every link of ITS tables its exact status; the other tables' verdicts stand
    refine_groups(cv, gbad[0].p, false, Tq, Lq, false, false, 0, 0, false);
  }
  // chains of different lengths (kernels_chain_pieces.hpp): the G pieces of l links of one pass from the caller's table-major arrays into
  // the link-major staging, in one launch; and the words of all passes back into the caller's table-major status array
  size_t chain_piece_gather(const uint64_t* desc, size_t G, uint32_t l, const uint8_t* decks, const uint8_t* proofs, const uint8_t* keys,
                            uint8_t* sdecks, uint8_t* sproofs, uint8_t* skeys) override {
    const uint32_t dw = 2 * N * G_::PB / 16, pw = (uint32_t)(proof_size_bytes(m, n, G_::PB) / 16), kw = keys ? G_::PB / 16 : 0;
    ChainPieceGatherArgs ga{desc, (const uint4*)decks, (const uint4*)proofs, (const uint4*)keys, (uint4*)sdecks, (uint4*)sproofs, (uint4*)skeys,
                            (uint64_t)(l + 1) * G * dw, (uint64_t)l * G * pw, (uint64_t)l * G * kw, (uint32_t)G, dw, pw, kw};
    const uint64_t W = ga.wd + ga.wp + ga.wk, ny = (W + CP_X_SPAN - 1) / CP_X_SPAN;
    if (ny > 65535) throw std::runtime_error("chain verification: too many bytes in one pass for one launch");
    MP_RUN(k_chain_piece_gather, C, (uint32_t)std::min<uint64_t>(W, CP_X_SPAN), (uint32_t)ny, ga);
    return (size_t)W * 16;
  }
  void chain_piece_scatter(const uint64_t* desc, const uint64_t* pass, uint32_t passes, const int32_t* words, size_t total, int32_t* status) override {
    ChainPieceScatterArgs sa{desc, pass, words, status, passes};
    MP_RUN(k_chain_piece_scatter, C, (uint32_t)total, 1, sa);
  }

  // ---------------------------------------------------------------- group verification (round 4)
  // The screening pass of a LARGE batch, one level up from the merged equation of one proof: the merged equations of L independent proofs
  // are added up with weights rho_j that depend on every proof of the group (the machinery of chain verification, without its shared
  // decks), and the resulting multi-scalar multiplication -- L (4N + 11m + 8) points, 7 616 for 32 proofs of a 52-card deck -- runs on
  // the bucket-method kernel: 33 additions per term and window-sorted, wave-reduced buckets instead of 51 additions, 15 window-table
  // entries and a share of four 250-doubling chains per term on the Straus path; the n + 5 fixed bases appear once per GROUP.  The
  // verifier's half of a 52-card step is the north star's kernel from here on (Pippenger: LDS-staged digits, counting sort by wavefront
  // prefix sum).  Soundness as for the merged equation (weights = Fr::rand of ChaCha20(Blake2s(final transcript states of the group's
  // proofs)): an error in one proof cannot cancel against another's except with probability ~2^-250).  A batch in which some group
  // fails is re-verified equation by equation, so the status words are exactly those of the other paths.  Lane of (member j, group t)
  // = j T + t with T = B / L groups: the members of a group are T proofs apart.
  // round 5, the bucket kernel's memory side (kernels_bucket.hpp): contiguous point runs per group, XCD-affine items, LDS-staged points
  // (A/B hooks of round 5, compile-time like the others -- tools/ab_build.py -DMP_EXP_BK_TILE=0 ...; the product library reads no
  // environment variable.  profiles/r05b_bucket_ab.txt has what each bought)
#ifndef MP_EXP_BK_TILE
#define MP_EXP_BK_TILE 1
#endif
#ifndef MP_EXP_BK_XCD
#define MP_EXP_BK_XCD 1
#endif
#ifndef MP_EXP_BK_STAGE
#define MP_EXP_BK_STAGE 1
#endif
  static constexpr bool bk_tile = MP_EXP_BK_TILE != 0, bk_xcd_affine = MP_EXP_BK_XCD != 0, bk_stage = MP_EXP_BK_STAGE != 0;
  DevBuf<uint32_t> gtile[2];          // [lane] the group equations' point runs: T x K x 64 bytes (4 GB at 262 144 proofs of 52 cards)
  std::map<std::pair<uint32_t, bool>, std::unique_ptr<ChainPlan>> gplans;      // by (proofs per group, keyed): a failing batch alternates between two sizes
  Workspace gws;                      // lean workspace of the pipelined group pass: no window tables, no digit planes (68 KB per proof)
  // Group size: the wave-wide reduction of a window costs ~40 additions whatever the equation holds, and 10-bit windows (26 per scalar
  // instead of 32) want ~60 terms per bucket -- ~30 000 points per equation when the batch is large
  // (128 proofs of a 52-card deck, 8 of a 1 024-card one); but the kernel's 2 048 persistent waves want a dozen (equation, window) items
  // each, so a smaller batch takes smaller groups: no fewer than 2/13 of the minimum batch (945 at the default 6 144: 12 x 2 048 / 26).
  // window width of the bucket method for an MSM of K terms (mp_set_bucket_bits; 0 = by size)
  uint32_t bucket_bits_of(uint32_t K) const { return bucket_bits ? bucket_bits : bk_bits_for(K); }
  // (BLS12-377: the bucket kernel's additions over a 377-bit field spill ~200 registers at two waves per SIMD and only draw level with the
  // Straus screen -- 13.1 k against 13.1 k proofs/s at (10,30) --, so groups are off there unless mp_set_group_verify asks for them)
  // Round 6: two sizes.  group_points (30 464: 128 proofs of a 52-card deck, 10-bit windows on one wave per window, 26 additions per
  // point) is what a batch of fewer than 16 384 proofs takes under the rule below; a larger one takes equations of up to group_points_wg
  // points (243 712: 1 024 proofs of a 52-card deck) instead -- 14-bit windows on the split pipeline (kernels_bucket.hpp k_bucket_sort /
  // _acc / _reduce: 18 additions per point; 12-bit ones, 21, from 50 000 points on).
  // BLS12-377: the one-wave-per-window kernel spills 200 registers on the 14-limb field and only drew level with the Straus screen
  // (round 4), so group_points stays 0 there; the split pipeline's hot loop is spill-free (213 registers, no scratch), takes 11-bit
  // windows too on this curve (mp_set_bucket_split 11) and equations from 40 000 points on: 32 proofs of a 300-card deck at 4 096 in
  // flight, 13.3 -> 14.5 k pairs/s with the subgroup test of every point still in the call (profiles/r06o_bls_groups.txt).
  static const uint32_t GROUP_POINTS_WAVE = 30464u, GROUP_POINTS_WG = 243712u, GROUP_WG_POINTS_MIN = G_::FW > 8 ? 40000u : 50000u;
  uint32_t group_points = G_::FW > 8 ? 0u : GROUP_POINTS_WAVE;      // points per group equation aimed at (mp_set_group_verify; 0 = off)
  uint32_t group_points_wg = GROUP_POINTS_WG;                       // ... by the batches large enough for the split pipeline (0 = never)
  uint32_t group_min_batch = 6144;    // smaller batches (in 52-card proofs: x 52 / N) keep the per-proof screen
  void set_group_verify(uint32_t points, size_t min_batch) override {
    // (one knob: up to 65 535 points = equations of that size at the most, under the rule of rounds 4-5; more = the split pipeline's
    // equations for the batches large enough, the default size below them)
    group_points = std::min(points, points > 65535u ? GROUP_POINTS_WAVE : 65535u);
    group_points_wg = points > 65535u ? points : 0u;
    group_min_batch = (uint32_t)std::min<size_t>(min_batch, 0x7FFFFFFFu);
  }
  // proofs per group for a batch of B (nearest_divisor of the wanted size); 0 = this batch takes the per-proof screen
  uint32_t group_size_of(size_t B) const override { return B < 0x7FFFFFFFu ? group_size((uint32_t)B, false) : 0; }
  uint32_t group_size(uint32_t B, bool keyed) const {
    const uint32_t per = 4 * N + 11 * m + 8 + (keyed ? 1u : 0u);
    // (the minimum counts lanes like the work-split thresholds: a proof of N cards brings N / 52 times the points of a 52-card one)
    if ((!group_points && !group_points_wg) || !merged_verify || (uint64_t)B * N < (uint64_t)group_min_batch * 52u) return 0;
    // as many proofs per group as bring its equation nearest to group_points points, but no fewer groups than keep the persistent
    // waves busy
    const uint32_t groups_min = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)group_min_batch * 2u) / 13u));
    uint32_t want = std::min<uint32_t>((group_points + per / 2) / per, B / groups_min);
    // (batches of 8/3 min_batch -- 16 384 -- 52-card proofs and more: the split pipeline's equations, if at least min_batch / 512 (12)
    // of at least GROUP_WG_POINTS_MIN points are left.  Its units are a thirty-second of a window, so sixteen equations of 1 024 proofs
    // keep the chip busy: 482 -> 504 k proofs/s at 16 384 in flight, 550 -> 586 k at 32 768, 610 -> 661 k at 65 536, 644 -> 702 k at
    // 131 072 (profiles/r06v_mid_batches.txt); below that the equations of rounds 4-5 or the per-proof screen are as fast or faster)
    const uint32_t want_wg = std::min<uint32_t>((group_points_wg + per / 2) / per, B / std::max<uint32_t>(1u, group_min_batch / 512u));
    if (group_points_wg && (uint64_t)want_wg * per >= GROUP_WG_POINTS_MIN && (uint64_t)B * N * 3u >= (uint64_t)group_min_batch * 52u * 8u)
      want = std::max(want, want_wg);
    // (under sustained rejection the groups shrink: note_group_verdicts below)
    if (want >= 4) want = std::max<uint32_t>(want >> adapt_shift, 4u);
    if (want < 2) return 0;
    // (without the contiguous run of k_group_tile a sorted entry names member and slot: 10 bits of link -- kernels_bucket.hpp)
    return nearest_divisor(B, want, per, [](uint32_t L) { return bk_tile || L <= 1023; });
  }
  // Groups that adapt to the rejection rate (round 5).  A group of L proofs fails if ANY member does: with a fraction p of bad proofs
  // spread over the batch, 1 - (1 - p)^L of the groups fail -- 72 % of the groups of 128 at p = 1 % -- and every member of a failing group
  // pays a finer pass (0.55-0.85 us per proof for a sub-group equation, 1.2 us equation by equation: profiles/r05h_rejection_strategies.txt)
  // on top of the screen that told it nothing.  So the table remembers what the last screens saw: if more than a fifth of the groups of a
  // call fail, the next call takes groups of half the size (down to 8: the screen of groups of 16 costs 0.16 us per proof more than that of
  // 128, and 15 % of them fail at p = 1 %); if fewer than 4 % fail, the size goes back up, one step per call.  Honest traffic never
  // leaves the default; under sustained 1 % rejection the step settles at ~0.8 x the honest rate instead of ~0.68 x.  Only calls with at
  // least 64 groups count (a fraction of three groups says nothing).  mp_set_group_adapt(t, 0) pins the default size.
  uint32_t adapt_shift = 0;
  bool group_adapt = true;
  void set_group_adapt(bool on) override {
    group_adapt = on;
    adapt_shift = 0;
  }
  void note_group_verdicts(uint32_t T, uint32_t failing, uint32_t L) {
    // (a fraction of three groups says nothing -- but sixteen equations of 1 024 proofs that ALL fail do: from eight groups on, and a
    // step down only on the evidence of at least four failing groups)
    if (!group_adapt || T < 8) return;
    if (T < 64 && failing > 0 && failing < 4) return;
    // (round 6: the default group is 1 024 proofs -- seven halvings down to 8.  When nineteen groups in twenty fail, the rate is far
    // beyond what the next size could clear: three halvings at once; and a call in which no group fails at all grows back two steps)
    if ((uint64_t)failing * 5 > T) {
      const uint32_t by = (uint64_t)failing * 20 >= (uint64_t)T * 19 && L >= 128 ? 3u : 1u;
      if (L >= 16) adapt_shift = std::min<uint32_t>(7u, adapt_shift + by);
    } else if ((uint64_t)failing * 25 < T && adapt_shift > 0) {
      adapt_shift -= failing == 0 && adapt_shift >= 2 ? 2u : 1u;
    }
  }
  ChainPlan& build_group_plan(uint32_t L, bool keyed) {
    const std::pair<uint32_t, bool> key(L, keyed);
    auto it = gplans.find(key);
    if (it != gplans.end()) return *it->second;
    if (gplans.size() >= 8) {      // (sizes come and go with the batch size: keep a handful)
      rt::stream_sync(ctx->stream);
      if (ctx->vstream) rt::stream_sync(ctx->vstream);
      gplans.clear();
    }
    std::unique_ptr<ChainPlan>& fresh = gplans[key];
    fresh.reset(new ChainPlan());
    if (keyed) ensure_keyed();
    const VerifyLay& l = (keyed ? psk : ps)[0].vplan.lay;
    const uint32_t per = l.pk + (keyed ? 1u : 0u);      // decks, proof points [, the proof's own key]
    build_equation_plan(*fresh, l, L, 1, keyed, L * per, L, [&](auto term) {
      for (uint32_t j = 0; j < L; ++j)
        for (uint32_t slot = 0; slot < per; ++slot)
          // (a term's point: its index in the group's contiguous run, or the P slot | member whose lane holds it)
          term(ChainTerm{l.mvar + slot, j, 1, NO_SLOT, 1}, bk_tile ? j * per + slot : (slot | (j << 20)));
    });
    return *fresh;
  }
  // the group pass on the context's CURRENT lane; the flag word (host_flag, or vflag) is raised if some group needs a closer look
  // and gbad_out[t] says which
  void verify_group_pass(const VArgs& v, uint32_t L, bool vlane, uint32_t* host_flag, uint32_t* gbad_out) {
    const uint32_t B = v.B, T = B / L;
    const bool keyed = v.keys != nullptr || v.kset != nullptr;
    ChainPlan& gplan = build_group_plan(L, keyed);
    PlanSet& q = (keyed ? psk : ps)[0];
    const VerifyLay& l = q.vplan.lay;
    rt::Stream s = ctx->stream;
    // (on the caller's stream the pass borrows the prover's arenas, as the per-proof screen does: nothing of a prove call outlives it;
    // the verify lane has lean arenas of its own)
    Workspace& w = vlane ? gws : ws;
    w.fw = G_::FW;
    w.ensure(B, l.nS, l.nP, std::max(gplan.nJ, 8u), 0, 0, nwin, stage_words_needed(), s, 0);
    load_verify_inputs(w, q, v, vlane, false);
    run_transcripts(w, q, B, keyed, true, false);
    size_equations(gplan, T, L);
    {
      // the group weights need the transcripts' final states and nothing else, and one lane per GROUP hashes them (2 048 lanes, 64
      // BLAKE2s blocks in a row: 2.5 ms of latency at 262 144 proofs): on `side`, beside the coefficient programs of the proofs
      SideGuard wguard{ctx, false};
      {
        SideFork on_side(ctx);
        run_chain_weights(w, (T + 63u) & ~63u, T, L);
        rt::event_record(ctx->ev_tab, ctx->side);
      }
      run_verify_scalars(w, q, B, true);
      rt::stream_wait(s, ctx->ev_tab);
      wguard.joined = true;
    }
    const uint32_t per = l.pk + (keyed ? 1u : 0u);
    const EquationArgs e{T, L, vlane, "group verification: too many groups for one launch", NO_SLOT, 1u, host_flag, gbad_out, v.status};
    run_equations(w, gplan, e, bk_tile, [&](uint32_t* run) {
      GroupTileArgs ta{w.P.p, run, w.Bpad, T, per, gplan.K};
      MP_RUN(k_group_tile, C, B, per, ta);
    });
  }

  // ---------------------------------------------------------------- building blocks (ad-hoc plans)
  struct Adhoc {
    Phase ph;
    PhaseDev dev;
    Workspace w;
  };
  void run_adhoc(Adhoc& ad, uint32_t B, uint32_t nS, uint32_t nP, uint32_t nJ) {
    ad.dev.upload(ad.ph, ctx->stream);
    ad.w.fw = G_::FW;
    ad.w.ensure(B, nS, nP, nJ, ad.ph.n_dslots, ad.ph.n_tslots, nwin, 4, ctx->stream, ad.ph.b_dig_bytes);
  }

  void remask_host(size_t count, const uint8_t* cards, const uint8_t* rho, uint8_t* out) override {
    // `count` cards = `count` batch lanes with N = 1
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)count;
    Adhoc ad;
    run_adhoc(ad, B, 1, 4, 4);
    Workspace& w = ad.w;
    DevBuf<uint8_t> din, drho, dout;
    din.alloc(count * 2 * G_::PB, s, false); drho.alloc(count * 32, s, false); dout.alloc(count * 2 * G_::PB, s, false);
    rt::h2d(din.p, cards, count * 2 * G_::PB, s);
    rt::h2d(drho.p, rho, count * 32, s);
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    FixedBases fb{n};
    LoadPointsArgs a{din.p, w.P.p, w.status.p, w.Bpad, 2, 0};
    MP_RUN(k_load_points, C, B, 2, a);
    LoadScalarsArgs sa{drho.p, w.S.p, w.status.p, w.Bpad, 1, 0};
    MP_RUN(k_load_scalars, C, B, 1, sa);
    RemaskArgs ra{w.S.p, w.P.p, w.J.p, FB.p, nullptr, w.Bpad, 1, 0, 0, 2, fb.G(), fb.pk(), fbg, 0, nullptr, nullptr, 0, 0, 0};
    MP_RUN(k_remask, C, B, 2, ra);
    normalize_flat(w.J.p + j_off<C>(2, w.Bpad, 0), w.P.p + p_off<C>(2, w.Bpad, 0), w.NS.p, (size_t)2 * w.Bpad);
    StorePointsArgs st{dout.p, w.P.p, w.Bpad, 2, 2};
    MP_RUN(k_store_points, C, B, 2, st);
    std::vector<int32_t> hs(B);
    rt::d2h(out, dout.p, count * 2 * G_::PB, s);
    rt::d2h(hs.data(), w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
    for (auto v : hs)
      if (v < 0) throw std::invalid_argument("remask: bad encoding in input");
  }

  void msm_host(size_t n_msm, size_t k, const uint8_t* scalars, const uint8_t* points, uint8_t* out) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)n_msm, K = (uint32_t)k;
    Adhoc ad;
    uint32_t next_partial = K + 1;
    {
      const uint32_t abits = bucket_bits_of(K);
      PhaseBuilder pb(ad.ph, next_partial, FCHUNK, VCHUNK, bucket_min, bk_windows(R::BITS, abits), 1u, abits);
      pb.begin(K);
      for (uint32_t t = 0; t < K; ++t) pb.var(t, t);
      pb.end();
      pb.normalize(K, 1);
    }
    run_adhoc(ad, B, K, K + 1, next_partial);
    Workspace& w = ad.w;
    DevBuf<uint8_t> dsc, dpt, dout;
    dsc.alloc(n_msm * k * 32, s, false); dpt.alloc(n_msm * k * G_::PB, s, false); dout.alloc(n_msm * G_::PB, s, false);
    rt::h2d(dsc.p, scalars, n_msm * k * 32, s);
    rt::h2d(dpt.p, points, n_msm * k * G_::PB, s);
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    LoadPointsArgs la{dpt.p, w.P.p, w.status.p, w.Bpad, K, 0};
    MP_RUN(k_load_points, C, B, K, la);
    LoadScalarsArgs sa{dsc.p, w.S.p, w.status.p, w.Bpad, K, 0};
    MP_RUN(k_load_scalars, C, B, K, sa);
    run_phase(ad.dev, w, B);
    StorePointsArgs so{dout.p, w.P.p, w.Bpad, 1, K};
    MP_RUN(k_store_points, C, B, 1, so);
    std::vector<int32_t> hs(B);
    rt::d2h(out, dout.p, n_msm * G_::PB, s);
    rt::d2h(hs.data(), w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
    for (auto v : hs)
      if (v < 0) throw std::invalid_argument("msm: bad encoding in input");
  }

  void commit_host(size_t count, size_t len, const uint8_t* values, const uint8_t* r, uint8_t* out) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)count, L = (uint32_t)len;
    FixedBases fb{n};
    Adhoc ad;
    uint32_t next_partial = 1;
    {
      PhaseBuilder pb(ad.ph, next_partial, FCHUNK, VCHUNK);
      pb.begin(0);
      for (uint32_t t = 0; t < L; ++t) pb.fixed(t, fb.ck(t));
      pb.fixed(L, fb.H());
      pb.end();
      pb.normalize(0, 1);
    }
    run_adhoc(ad, B, L + 1, 1, next_partial);
    Workspace& w = ad.w;
    DevBuf<uint8_t> dv, dr, dout;
    dv.alloc(std::max<size_t>(count * len * 32, 4), s, false); dr.alloc(count * 32, s, false); dout.alloc(count * G_::PB, s, false);
    if (len) rt::h2d(dv.p, values, count * len * 32, s);
    rt::h2d(dr.p, r, count * 32, s);
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    if (L) {
      LoadScalarsArgs sa{dv.p, w.S.p, w.status.p, w.Bpad, L, 0};
      MP_RUN(k_load_scalars, C, B, L, sa);
    }
    LoadScalarsArgs sr{dr.p, w.S.p, w.status.p, w.Bpad, 1, L};
    MP_RUN(k_load_scalars, C, B, 1, sr);
    run_phase(ad.dev, w, B);
    StorePointsArgs so{dout.p, w.P.p, w.Bpad, 1, 0};
    MP_RUN(k_store_points, C, B, 1, so);
    std::vector<int32_t> hs(B);
    rt::d2h(out, dout.p, count * G_::PB, s);
    rt::d2h(hs.data(), w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
    for (auto v : hs)
      if (v < 0) throw std::invalid_argument("commit: bad encoding in input");
  }

  void plan_stats(uint64_t out[16]) override {
    for (int i = 0; i < 16; ++i) out[i] = 0;
    uint64_t bucket_terms = 0, bucket_jobs = 0;
    auto add = [&](const Phase& ph, uint64_t* o) {
      o[0] += ph.fterms.size(); o[1] += ph.vterms.size(); o[2] += ph.fjobs.size(); o[3] += ph.vjobs.size();
      o[4] += ph.tables.size(); o[5] += ph.cterms.size() + ph.cterms2.size() + ph.cterms0.size();
      bucket_terms += ph.bterms.size();
      bucket_jobs += ph.bjobs.size();
    };
    for (int i = 0; i < 6; ++i) add(ps[0].pplan.ph[i], out);
    add(merged_verify ? ps[0].vplan.mph : ps[0].vplan.ph, out + 6);    // what an honest batch executes
    out[12] = nwin; out[13] = fbg.windows;
    out[14] = N | ((uint64_t)(ps[0].pplan.toom.E ? m : 0u) << 32);      // high word: m if k_toom_points runs in this plan
    out[15] = bucket_terms | (bucket_jobs << 32);      // variable-base terms / MSMs on the bucket kernel (prove + verify)
  }
  // ---------------------------------------------------------------- sigma screening (kernels_screen.hpp; mp_set_sigma_screen)
  // Opt-in: the Chaum-Pedersen / Schnorr verifiers behind opening, dealing and seating check every proof on a Straus plan of its own
  // (~3 x (51 + 15) additions and ~500 doublings a lane).  With the screen on, the checks z g_i - c a_i - A_i = O of g consecutive lanes
  // are added up, each with a weight of its own, into ONE equation: 3 nb points a lane (one fewer where a base is the table's G, which
  // collapses into one fixed-base term per 64 lanes), ~18-33 additions a point on the bucket pipeline.  A group whose equation fails, or
  // that holds a lane whose status word is set already, goes through the verifier's own per-proof phase -- its lanes only --, so every
  // status word is the one the unscreened call gives.  Weights: Fr::rand of ChaCha20(Blake2s(...)) over the lane digests of the whole
  // group (k_screen_digest: transcript state AND response), through k_chain_digest / k_chain_weights.
  struct SigmaScreen {
    uint32_t lanes = 0;               // 0 = off, MP_SIGMA_SCREEN_AUTO = by points, else lanes per group
    uint32_t min_lanes = 0;
    uint64_t stats[4] = {0, 0, 0, 0};
    // the plan of one group equation, cached by (nbases, which base is G, lanes per group, window width)
    uint32_t nb = 0, g = 0, bits = 0, per = 0;
    int gi = -2;
    ChainPlan plan;
    std::vector<ScreenTerm> terms;
    DevBuf<ScreenTerm> dterms;
    uint32_t pslot[8];
    Workspace w;                      // lean: the equations' J slots and the bucket kernels' scratch
    Workspace rw;                     // the lanes of failing groups, compacted: what the verifier's phase needs
    DevBuf<uint32_t> seeds, dig, cw, cs, tile, part, gbad, flag, idx;
    DevBuf<int16_t> d16;
  } scr;
  static const uint32_t SCREEN_POINTS_PER_LANE_MAX = 6;      // Chaum-Pedersen, neither base the table's G
  int set_sigma_screen(uint32_t lanes, size_t min_lanes) override {
    if (lanes != MP_SIGMA_SCREEN_AUTO && (uint64_t)lanes * SCREEN_POINTS_PER_LANE_MAX > BUCKET_TERMS_MAX) return MP_ERR_BAD_ARGUMENT;
    scr.lanes = lanes;
    scr.min_lanes = (uint32_t)std::min<size_t>(min_lanes, 0xFFFFFFFFu);
    for (uint64_t& v : scr.stats) v = 0;
    return MP_OK;
  }
  void sigma_screen_stats(uint64_t out[4]) const override {
    for (int i = 0; i < 4; ++i) out[i] = scr.stats[i];
  }
  // Lanes per group for a call of B lanes of `per` points; 0 = this call keeps the per-proof path.  An explicit size is taken as it is.
  // AUTO sizes by points like group_size (mp_set_group_verify, mp_set_bucket_bits / _split decide the kernel from there): a call with
  // enough points for the split pipeline (GROUP_WG_POINTS_MIN) takes equations of up to group_points_wg points, as few and as even as
  // B allows -- its units are a thirty-second of a window, one equation already spreads over the chip.  Below that the
  // one-wave-per-window kernel wants an (equation, window) item per persistent wave: 64 equations of 32 windows, up to group_points
  // points each; groups of fewer than 16 lanes pay a window's reduction (~40 additions) for ~80 points and stay on the Straus plans.
  uint32_t screen_group_lanes(uint32_t B, uint32_t per) const {
    if (scr.lanes != MP_SIGMA_SCREEN_AUTO) return std::min(scr.lanes, B);
    uint32_t want = 0;
    if (group_points_wg && (uint64_t)B * per >= GROUP_WG_POINTS_MIN) {
      want = std::min<uint32_t>((group_points_wg + per / 2) / per, B);
    } else if (group_points) {
      want = std::min<uint32_t>((group_points + per / 2) / per, B / 64u);
      if (want < 16) return 0;
    }
    if (want < 2) return 0;
    const uint32_t T = (B + want - 1) / want;
    return (B + T - 1) / T;
  }
  // The plan builder: the variable terms of a lane over SigmaLay -- (z, g_i) unless g_i is the table's G, (-c, a_i), (-1, A_i) with
  // the weight of check i -- in the order k_screen_tile lays the lane's points out; G's terms collapsed as build_equation_plan
  // collapses the fixed bases (runs of at most 64 lanes)
  void build_screen_plan(const SigmaLay& l, int gi, uint32_t g, uint32_t bits) {
    if (scr.nb == l.nb && scr.gi == gi && scr.g == g && scr.bits == bits) return;
    if (scr.g) rt::stream_sync(ctx->stream);      // (the plan being replaced may still be read)
    ChainPlan& p = scr.plan;
    p.ph = Phase();
    scr.terms.clear();
    uint32_t next_partial = 1;                    // J slot 0 = the equation's value
    PhaseBuilder pb(p.ph, next_partial, FCHUNK, VCHUNK, 1u, bk_windows(R::BITS, bits), 1u, bits);
    pb.begin(0);
    uint32_t per = 0;
    for (uint32_t i = 0; i < l.nb; ++i) {
      if ((int)i != gi) scr.pslot[per++] = l.g + i;
      scr.pslot[per++] = l.a + i;
      scr.pslot[per++] = l.A + i;
    }
    auto var = [&](uint32_t s, uint32_t pslot, uint32_t j, uint32_t i) {
      pb.var((uint32_t)scr.terms.size(), (uint32_t)scr.terms.size());      // (a term's point: its index in the group's contiguous run)
      scr.terms.push_back(ScreenTerm{s, pslot, j, 1u, i});
    };
    for (uint32_t j = 0; j < g; ++j)
      for (uint32_t i = 0; i < l.nb; ++i) {
        if ((int)i != gi) var(l.z, l.g + i, j, i);
        var(l.negc, l.a + i, j, i);
        var(l.minus_one, l.A + i, j, i);
      }
    p.K = (uint32_t)scr.terms.size();
    if (gi >= 0)
      for (uint32_t j0 = 0; j0 < g; j0 += 64u) {
        pb.fixed((uint32_t)scr.terms.size(), FixedBases{n}.G());
        scr.terms.push_back(ScreenTerm{l.z, NO_SLOT, j0, std::min(64u, g - j0), (uint32_t)gi});
      }
    p.nfix = (uint32_t)scr.terms.size() - p.K;
    pb.end();
    p.nJ = next_partial;
    p.dev.upload(p.ph, ctx->stream);
    scr.dterms.upload(scr.terms, ctx->stream);
    scr.nb = l.nb; scr.gi = gi; scr.g = g; scr.bits = bits; scr.per = per;
  }
  // what a verifier hands over in place of "run_phase(vdev); k_sigma_verdict": its lanes in w (statement, commitments, z, -c, -1 and the
  // transcript state in place, subgroup and encoding findings in w.status), gi = which base is the table's G (-1: none), its per-proof
  // phase and what that needs of a workspace.  true: w.status holds the final word of every lane; false: not screened, the caller goes on
  // as before.  Waits once for the 4-byte flag; a second time, for the groups' words, only if some group failed.
  struct ScreenCall {
    const SigmaLay& l;
    int gi;
    PhaseDev& vdev;
    uint32_t nP, nJ, nD, nT;
    int32_t fail_code;
  };
  bool screen_sigma(Workspace& w, uint32_t B, const ScreenCall& c) {
    if (!scr.lanes || !B || B < scr.min_lanes || B > 0x7FFFFFFFu || c.l.nb > 2) return false;
    // (a curve with a cofactor: without the per-point subgroup test a weighted sum and a per-proof check can disagree on points with a
    // low-order component -- the screen runs only while the test does)
    if (!Cofactor<C>::ONE && !subgroup_check) return false;
    const SigmaLay& l = c.l;
    const uint32_t per = 3 * l.nb - (c.gi >= 0 ? 1u : 0u);
    const uint32_t g = screen_group_lanes(B, per);
    if (!g) return false;
    const uint32_t K = g * per, bits = bucket_bits_of(K);
    // (one bucket job; the one-wave-per-window kernel sorts up to 65 535 points per window)
    if (K > BUCKET_TERMS_MAX || (bits < bucket_split_bits && K > 65535u)) return false;
    const uint32_t T = (B + g - 1) / g, Tpad = (T + 63u) & ~63u, L = g * l.nb, nblk = (L + CW_BLOCK - 1) / CW_BLOCK;
    if ((uint64_t)T * g >= ((uint64_t)1 << 31) || (uint64_t)T * K >= ((uint64_t)1 << 32)) return false;
    rt::Stream s = ctx->stream;
    build_screen_plan(l, c.gi, g, bits);
    ChainPlan& p = scr.plan;
    const uint32_t nterms = p.K + p.nfix;
    scr.w.fw = G_::FW;
    scr.w.ensure(T, 1, 1, std::max(p.nJ, 8u), 0, 0, nwin, 4, s, 0);
    scr.seeds.alloc((size_t)8 * L * T, s, false);
    scr.dig.alloc((size_t)nblk * 8 * Tpad, s, false);
    scr.cw.alloc((size_t)L * Tpad * 8, s, false);
    scr.cs.alloc((size_t)nterms * Tpad * 8, s);
    scr.d16.alloc((size_t)p.dev.b_dig_bytes * Tpad, s);
    scr.tile.alloc((size_t)T * K * G_::PW, s, false);
    scr.part.alloc(T, s, false);
    scr.gbad.alloc(T, s, false);
    if (!scr.flag.n) scr.flag.alloc(1, s);
    rt::dzero(scr.part.p, (size_t)T * 4, s);
    rt::dzero(scr.flag.p, 4, s);
    // weights
    ScreenDigestArgs da{w.seed.p, w.S.p, scr.seeds.p, w.Bpad, L * T, B, g, T, l.nb, l.z};
    MP_RUN(k_screen_digest, C, T * g, 1, da);
    ChainWeightsArgs wa{scr.seeds.p, scr.cw.p, scr.dig.p, L * T, Tpad, T, L};
    MP_RUN(k_chain_digest, C, T, nblk, wa);
    MP_RUN(k_chain_weights, C, T, nblk, wa);
    // one scalar per point / run of G, the points as one run per group, ONE bucket MSM + fixed-base part per group
    ScreenScalArgs sa{w.S.p, w.P.p, scr.cw.p, scr.cs.p, scr.dterms.p, w.Bpad, Tpad, B, g, l.nb};
    MP_RUN(k_screen_scalars, C, T, nterms, sa);
    ScreenTileArgs ta{w.P.p, scr.tile.p, {0, 0, 0, 0, 0, 0, 0, 0}, w.Bpad, B, g, per};
    for (uint32_t y = 0; y < per; ++y) ta.pslot[y] = scr.pslot[y];
    MP_RUN(k_screen_tile, C, T * g, per, ta);
    run_equation_msm(scr.w, p.dev, scr.cs.p, scr.d16.p, T, "sigma screening: too many groups for one launch", scr.tile.p, p.K);
    ScreenVerdictArgs va{scr.w.J.p, w.status.p, scr.part.p, scr.gbad.p, scr.flag.p, scr.w.Bpad, B, g};
    MP_RUN(k_screen_check, C, B, 1, va);
    MP_RUN(k_screen_verdict, C, T, 1, va);
    MP_RUN(k_screen_mark, C, B, 1, va);
    scr.stats[0] += B;
    scr.stats[1] += T;
    uint32_t flag = 0;
    rt::d2h(&flag, scr.flag.p, 4, s);
    rt::stream_sync(s);
    if (!flag) return true;
    // some group failed: ITS lanes, compacted, through the verifier's per-proof phase; everybody else's word stands
    std::vector<uint32_t> hbad(T), hidx;
    rt::d2h(hbad.data(), scr.gbad.p, (size_t)T * 4, s);
    rt::stream_sync(s);
    for (uint32_t t = 0; t < T; ++t)
      if (hbad[t]) {
        scr.stats[2] += 1;
        for (uint64_t b = (uint64_t)t * g; b < std::min<uint64_t>((uint64_t)(t + 1) * g, B); ++b) hidx.push_back((uint32_t)b);
      }
    const uint32_t nsub = (uint32_t)hidx.size();
    scr.stats[3] += nsub;
    Workspace& rw = scr.rw;
    rw.fw = G_::FW;
    rw.ensure(nsub, 6, c.nP, c.nJ, c.nD, c.nT, nwin, 4, s);
    scr.idx.alloc(nsub, s, false);
    rt::h2d(scr.idx.p, hidx.data(), (size_t)nsub * 4, s);
    ScreenGatherArgs ga{w.P.p, w.S.p, w.status.p, rw.P.p, rw.S.p, rw.status.p, scr.idx.p, w.Bpad, rw.Bpad, 3 * l.nb, 6};
    MP_RUN(k_screen_gather, C, nsub, 3 * l.nb + 6 + 1, ga);
    run_phase(c.vdev, rw, nsub);
    SigmaVerdictArgs sv{rw.J.p, rw.status.p, l, rw.Bpad, c.fail_code};
    MP_RUN(k_sigma_verdict, C, nsub, 1, sv);
    ScatterStatusArgs ss{rw.status.p, w.status.p, scr.idx.p};
    MP_RUN(k_scatter_status, C, nsub, 1, ss);
    rt::stream_sync(s);      // (idx[] was uploaded from pageable memory)
    return true;
  }

  // ---------------------------------------------------------------- sigma protocols
  void sigma_host(bool prove, size_t B_, uint32_t nb, const uint8_t* bases, const uint8_t* publics, const uint8_t* witness,
                  const uint8_t* fs_init, const uint8_t* seeds, uint8_t* proofs, int32_t* status) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)B_;
    const SigmaLay l = make_sigma_lay(nb);
    const size_t psz = (size_t)nb * G_::PB + 32;
    Adhoc ad;
    uint32_t next_partial = l.chk + nb;
    {
      PhaseBuilder pb(ad.ph, next_partial, FCHUNK, VCHUNK);
      if (prove) {
        for (uint32_t i = 0; i < nb; ++i) {
          pb.begin(l.A + i);
          pb.var(l.r, l.g + i);
          pb.end();
        }
        pb.normalize(l.A, nb);
      } else {
        for (uint32_t i = 0; i < nb; ++i) {
          pb.begin(l.chk + i);
          pb.var(l.z, l.g + i);
          pb.var(l.negc, l.a + i);
          pb.var(l.minus_one, l.A + i);
          pb.end();
        }
      }
    }
    ad.dev.upload(ad.ph, s);
    ad.w.fw = G_::FW;
    ad.w.ensure(B, 6, 3 * nb, next_partial, ad.ph.n_dslots, ad.ph.n_tslots, nwin, (3 * nb * (G_::PB + 1) + 32) / 4 + 4, s);
    Workspace& w = ad.w;
    DevBuf<uint8_t> dg, da, dx, dfs, dseed, dpf;
    DevBuf<int32_t> dst;
    dg.alloc((size_t)B * nb * G_::PB, s, false); da.alloc((size_t)B * nb * G_::PB, s, false); dfs.alloc((size_t)B * 32, s, false);
    dpf.alloc((size_t)B * psz, s, false);
    rt::h2d(dg.p, bases, (size_t)B * nb * G_::PB, s);
    rt::h2d(da.p, publics, (size_t)B * nb * G_::PB, s);
    rt::h2d(dfs.p, fs_init, (size_t)B * 32, s);
    rt::dzero(w.status.p, (size_t)w.Bpad * 4, s);
    LoadPointsArgs lg{dg.p, w.P.p, w.status.p, w.Bpad, nb, l.g};
    MP_RUN(k_load_points, C, B, nb, lg);
    LoadPointsArgs la{da.p, w.P.p, w.status.p, w.Bpad, nb, l.a};
    MP_RUN(k_load_points, C, B, nb, la);
    // wire points are validated like those of the shuffle calls (mp_set_subgroup_check): z g - c a - A = O also holds for a + L
    // whenever c L = O, so a key or a reveal token shifted by a low-order point would pass with probability 1 / ord(L)
    check_subgroup(w, B, l.g, 2 * nb);      // bases and publics are consecutive P slots
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    if (prove) {
      dx.alloc((size_t)B * 32, s, false); dseed.alloc((size_t)B * 32, s, false);
      rt::h2d(dx.p, witness, (size_t)B * 32, s);
      rt::h2d(dseed.p, seeds, (size_t)B * 32, s);
      LoadScalarsArgs lx{dx.p, w.S.p, w.status.p, w.Bpad, 1, l.x};
      MP_RUN(k_load_scalars, C, B, 1, lx);
      SigmaInitArgs ia{w.S.p, dseed.p, l, w.Bpad, f, w.P.p, dfs.p};
      MP_RUN(k_sigma_init, C, B, 1, ia);
      run_phase(ad.dev, w, B);
      SigmaFsArgs fa{f, w.S.p, w.P.p, dfs.p, l, 1};
      MP_RUN(k_sigma_fs, C, B, 1, fa);
      SigmaIoArgs io{dpf.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
      MP_RUN(k_sigma_store, C, B, nb + 1, io);
      rt::d2h(proofs, dpf.p, (size_t)B * psz, s);
    } else {
      rt::h2d(dpf.p, proofs, (size_t)B * psz, s);
      SigmaIoArgs io{dpf.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
      MP_RUN(k_sigma_load, C, B, nb + 1, io);
      check_subgroup(w, B, l.A, nb);
      SigmaFsArgs fa{f, w.S.p, w.P.p, dfs.p, l, 0};
      MP_RUN(k_sigma_fs, C, B, 1, fa);
      if (!screen_sigma(w, B, ScreenCall{l, -1, ad.dev, 3 * nb, next_partial, ad.ph.n_dslots, ad.ph.n_tslots, nb == 1 ? 5 : 6})) {
        run_phase(ad.dev, w, B);
        SigmaVerdictArgs va{w.J.p, w.status.p, l, w.Bpad, nb == 1 ? 5 : 6};
        MP_RUN(k_sigma_verdict, C, B, 1, va);
      }
    }
    rt::d2h(status, w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
  }

  // ---------------------------------------------------------------- opening cards (kernels_open.hpp)
  // Reveal tokens with their Chaum-Pedersen proofs, and their verification with the token sums and the card lookup, for the T tokens
  // of C cards at once: lane b = c * T + j (or, with an offsets array, the lanes first[c] .. first[c+1] - 1), the statement slots of kernels_sigma.hpp filled on the device (k_open_stmt).  Against
  // sigma_host, which knows nothing about its statements: G is the table's fixed base (window table in HBM, no doubling chain), the
  // commitments enter the checks as affine addends instead of terms with the scalar -1, and the prover builds the window table of c0
  // once for token and commitment.  The plans are static and the workspace stays with the table: a device-resident call allocates
  // nothing once it has seen its batch size.
  struct OpenState {
    bool ready = false;
    Phase vph, rph1, rph2;          // checks of the verifier | the token x c0 | the commitments r c0, r G
    PhaseDev vdev, rdev1, rdev2;
    uint32_t nJ = 0, nD = 0, nT = 0;
    uint32_t fs_seed[8];            // Blake2s("Reveal Proof")  [REF mod.rs:83]
    Workspace w;
    DevBuf<uint8_t> fs;             // [B][32]
    DevBuf<uint32_t> c1, sumJ, sumP, scratch;      // the C-lane section: second halves of the cards, plaintexts
    DevBuf<int32_t> cstat;
  } op;
  void open_prepare(uint32_t B) {
    rt::Stream s = ctx->stream;
    const SigmaLay l = make_sigma_lay(2);
    if (!op.ready) {
      FixedBases fb{n};
      uint32_t np = l.chk + 2;
      {
        PhaseBuilder pb(op.vph, np, FCHUNK, VCHUNK);      // z g_i - c a_i - A_i, i = 0, 1
        pb.begin(l.chk);
        pb.var(l.z, l.g);
        pb.var(l.negc, l.a);
        pb.addend(l.A, true);
        pb.end();
        pb.begin(l.chk + 1);
        pb.fixed(l.z, fb.G());
        pb.var(l.negc, l.a + 1);
        pb.addend(l.A + 1, true);
        pb.end();
      }
      {
        PhaseBuilder pb(op.rph1, np, FCHUNK, VCHUNK);
        pb.begin(l.a);
        pb.var(l.x, l.g);
        pb.end();
        pb.normalize(l.a, 1);
      }
      {
        PhaseBuilder pb(op.rph2, np, FCHUNK, VCHUNK);
        pb.begin(l.A);
        pb.var(l.r, l.g);
        pb.end();
        pb.begin(l.A + 1);
        pb.fixed(l.r, fb.G());
        pb.end();
        pb.normalize(l.A, 2);
      }
      // token and commitment share the base c0: both phases know its window table as table slot 0, and the first one builds it
      if (op.rph1.tables.size() != 1 || op.rph2.tables.size() != 1 || op.rph1.tables[0].s != l.g || op.rph2.tables[0].s != l.g ||
          op.rph1.tables[0].b != 0 || op.rph2.tables[0].b != 0)
        throw std::logic_error("reveal plan: the phases do not share the table of c0");
      op.rph2.tables.clear();
      op.nJ = np;
      for (const Phase* ph : {&op.vph, &op.rph1, &op.rph2}) {
        op.nD = std::max(op.nD, ph->n_dslots);
        op.nT = std::max(op.nT, ph->n_tslots);
      }
      op.vdev.upload(op.vph, s);
      op.rdev1.upload(op.rph1, s);
      op.rdev2.upload(op.rph2, s);
      Blake2sState st;
      blake2s_init(st);
      uint32_t mblk[16] = {0};
      memcpy(mblk, "Reveal Proof", 12);
      blake2s_compress(st, mblk, 12, true);
      memcpy(op.fs_seed, st.h, 32);
      op.ready = true;
    }
    op.w.fw = G_::FW;
    op.w.ensure(B, 6, 6, op.nJ, op.nD, op.nT, nwin, (6 * (G_::PB + 1) + 32) / 4 + 4, s);
    op.fs.alloc((size_t)op.w.cap * 32, s, false);
    rt::dzero(op.w.status.p, (size_t)op.w.Bpad * 4, s);
  }
  OpenStmtArgs open_stmt_args(size_t K, const uint8_t* keys, const uint8_t* cards, uint32_t T, const uint32_t* signer, const uint32_t* first,
                              size_t C_) {
    OpenStmtArgs a{};
    Workspace& w = op.w;
    a.P = w.P.p; a.S = w.S.p; a.status = w.status.p;
    a.keys = keys; a.cards = cards; a.signer = signer;
    a.fbpts = fbpts.p;
    a.fs_init = op.fs.p;
    memcpy(a.fs_seed, op.fs_seed, 32);
    a.l = make_sigma_lay(2);
    a.Bpad = w.Bpad; a.K = (uint32_t)K; a.T = T; a.g_base = FixedBases{n}.G();
    a.first = first; a.C = (uint32_t)C_;
    return a;
  }
  int check_card_list(size_t n_plain, const uint8_t* plain) {
    for (size_t i = 0; i < n_plain; ++i) {
      Aff<C> p;
      if (!wire_point_host(plain + i * G_::PB, p))
        return fail(MP_ERR_BAD_ENCODING, "card list: entry " + std::to_string(i) + " is not a canonical point of the curve");
    }
    return MP_OK;
  }
  // every pointer a device pointer; everything is enqueued on the context's stream.  (The card list is only ever compared with
  // canonical bytes: it is validated as an encoding -- on the host, one short copy back unless the caller has done it -- and not
  // tested for the subgroup.)
  int unmask_dev(size_t K, const uint8_t* keys, size_t C_, const uint8_t* cards, uint32_t T, const uint32_t* signer, const uint8_t* tokens,
                 const uint8_t* proofs, size_t n_plain, const uint8_t* plain, uint8_t* out_plain, uint32_t* out_index,
                 int32_t* token_status, int32_t* card_status, bool plain_validated, const uint32_t* first, size_t lanes) override {
    rt::Stream s = ctx->stream;
    const uint32_t Cn = (uint32_t)C_, B = first ? (uint32_t)lanes : Cn * T;
    if (n_plain && !plain_validated) {
      std::vector<uint8_t> hp(n_plain * G_::PB);
      rt::d2h(hp.data(), plain, hp.size(), s);
      rt::stream_sync(s);
      const int rc = check_card_list(n_plain, hp.data());
      if (rc != MP_OK) return rc;
    }
    open_prepare(B);
    Workspace& w = op.w;
    const SigmaLay l = make_sigma_lay(2);
    op.c1.alloc((size_t)Cn * G_::PW, s, false); op.sumJ.alloc((size_t)Cn * G_::JW, s, false); op.sumP.alloc((size_t)Cn * G_::PW, s, false);
    op.scratch.alloc((size_t)Cn * G_::FW, s, false); op.cstat.alloc(Cn, s, false);
    rt::dzero(op.cstat.p, (size_t)Cn * 4, s);
    OpenStmtArgs sa = open_stmt_args(K, keys, cards, T, signer, first, C_);
    sa.tokens = tokens; sa.c1 = op.c1.p; sa.cstat = op.cstat.p;
    MP_RUN(k_open_stmt, C, B, 4, sa);
    SigmaIoArgs io{const_cast<uint8_t*>(proofs), w.S.p, w.P.p, w.status.p, l, w.Bpad};
    MP_RUN(k_sigma_load, C, B, 3, io);
    if (subgroup_check) {      // c0 | token, key | commitments (G is the table's own); c1 through the C-lane section
      check_subgroup(w, B, l.g, 1);
      check_subgroup(w, B, l.a, 4);      // publics and commitments are consecutive P slots
      SubgroupArgs ca{op.c1.p, op.cstat.p, Cn, 0};
      MP_RUN(k_subgroup_check, C, Cn, 1, ca);
    }
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    SigmaFsArgs fa{f, w.S.p, w.P.p, op.fs.p, l, 0};
    MP_RUN(k_sigma_fs, C, B, 1, fa);
    if (!screen_sigma(w, B, ScreenCall{l, 1, op.vdev, 6, op.nJ, op.nD, op.nT, 6})) {
      run_phase(op.vdev, w, B);
      SigmaVerdictArgs va{w.J.p, w.status.p, l, w.Bpad, 6};
      MP_RUN(k_sigma_verdict, C, B, 1, va);
    }
    UnmaskSumArgs ua{w.P.p, w.status.p, signer, op.c1.p, op.cstat.p, op.sumJ.p, token_status, card_status, w.Bpad, (uint32_t)K, T, l.a, first};
    MP_RUN(k_unmask_sum, C, Cn, 1, ua);
    normalize_flat(op.sumJ.p, op.sumP.p, op.scratch.p, Cn);
    CardMatchArgs ma{op.sumP.p, card_status, plain, out_plain, out_index, (uint32_t)n_plain};
    MP_RUN(k_card_match, C, Cn, 1, ma);
    return MP_OK;
  }
  int unmask_host(size_t K, const uint8_t* keys, size_t C_, const uint8_t* cards, uint32_t T, const uint32_t* signer, const uint8_t* tokens,
                  const uint8_t* proofs, size_t n_plain, const uint8_t* plain, uint8_t* out_plain, uint32_t* out_index,
                  int32_t* token_status, int32_t* card_status, const uint32_t* first, size_t lanes) override {
    rt::Stream s = ctx->stream;
    const size_t B = first ? lanes : C_ * T, psz = 2 * (size_t)G_::PB + 32;
    const int rc = check_card_list(n_plain, plain);
    if (rc != MP_OK) return rc;
    DevBuf<uint8_t> dk, dc, dt, dp, dl, dout;
    DevBuf<uint32_t> dsg, didx;
    DevBuf<int32_t> dts, dcs;
    dk.alloc(K * G_::PB, s, false); dc.alloc(C_ * 2 * G_::PB, s, false); dt.alloc(B * G_::PB, s, false); dp.alloc(B * psz, s, false);
    dl.alloc(std::max<size_t>(n_plain * G_::PB, 4), s, false); dout.alloc(C_ * G_::PB, s, false);
    dsg.alloc(B, s, false); didx.alloc(C_, s, false); dts.alloc(B, s, false); dcs.alloc(C_, s, false);
    rt::h2d(dk.p, keys, K * G_::PB, s);
    rt::h2d(dc.p, cards, C_ * 2 * G_::PB, s);
    rt::h2d(dt.p, tokens, B * G_::PB, s);
    rt::h2d(dp.p, proofs, B * psz, s);
    rt::h2d(dsg.p, signer, B * 4, s);
    if (n_plain) rt::h2d(dl.p, plain, n_plain * G_::PB, s);
    unmask_dev(K, dk.p, C_, dc.p, T, dsg.p, dt.p, dp.p, n_plain, dl.p, dout.p, didx.p, dts.p, dcs.p, true, first, lanes);
    rt::d2h(out_plain, dout.p, C_ * G_::PB, s);
    rt::d2h(out_index, didx.p, C_ * 4, s);
    rt::d2h(token_status, dts.p, B * 4, s);
    rt::d2h(card_status, dcs.p, C_ * 4, s);
    rt::stream_sync(s);
    return MP_OK;
  }
  // token = sk[signer] c0 first: the hedged nonce hashes the whole statement, the token included (k_sigma_init)
  void reveal_host(size_t K, const uint8_t* keys, const uint8_t* sks, size_t C_, const uint8_t* cards, uint32_t T, const uint32_t* signer,
                   const uint8_t* seeds, uint8_t* out_tokens, uint8_t* out_proofs, int32_t* status, const uint32_t* first, size_t lanes) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)(first ? lanes : C_ * T);
    const size_t psz = 2 * (size_t)G_::PB + 32;
    open_prepare(B);
    Workspace& w = op.w;
    const SigmaLay l = make_sigma_lay(2);
    DevBuf<uint8_t> dk, dx, dc, dseed, dtok, dpf;
    DevBuf<uint32_t> dsg;
    dk.alloc(K * G_::PB, s, false); dx.alloc(K * 32, s, false); dc.alloc(C_ * 2 * G_::PB, s, false); dseed.alloc((size_t)B * 32, s, false);
    dtok.alloc((size_t)B * G_::PB, s, false); dpf.alloc((size_t)B * psz, s, false); dsg.alloc(B, s, false);
    rt::h2d(dk.p, keys, K * G_::PB, s);
    rt::h2d(dx.p, sks, K * 32, s);
    rt::h2d(dc.p, cards, C_ * 2 * G_::PB, s);
    rt::h2d(dseed.p, seeds, (size_t)B * 32, s);
    rt::h2d(dsg.p, signer, (size_t)B * 4, s);
    OpenStmtArgs sa = open_stmt_args(K, dk.p, dc.p, T, dsg.p, first, C_);
    sa.sks = dx.p;
    MP_RUN(k_open_stmt, C, B, 4, sa);
    check_subgroup(w, B, l.g, 1);          // c0 and the key, as the sigma calls test bases and publics (the token is computed here)
    check_subgroup(w, B, l.a + 1, 1);
    run_phase(op.rdev1, w, B);
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    SigmaInitArgs ia{w.S.p, dseed.p, l, w.Bpad, f, w.P.p, op.fs.p};
    MP_RUN(k_sigma_init, C, B, 1, ia);
    run_phase(op.rdev2, w, B);             // (its table list is empty: the table of c0 is the first phase's)
    SigmaFsArgs fa{f, w.S.p, w.P.p, op.fs.p, l, 1};
    MP_RUN(k_sigma_fs, C, B, 1, fa);
    SigmaIoArgs io{dpf.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
    MP_RUN(k_sigma_store, C, B, 3, io);
    StorePointsArgs so{dtok.p, w.P.p, w.Bpad, 1, l.a};
    MP_RUN(k_store_points, C, B, 1, so);
    rt::d2h(out_tokens, dtok.p, (size_t)B * G_::PB, s);
    rt::d2h(out_proofs, dpf.p, (size_t)B * psz, s);
    rt::d2h(status, w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
  }

  // ---------------------------------------------------------------- dealing and seating (kernels_deal.hpp)
  // Masking / remasking with their Chaum-Pedersen proofs, their verification, and the key-ownership proofs of the seated players with
  // the tables' aggregate keys: one lane per card, or per player.  As in the opening phase the statements are filled on the device
  // (k_deal_stmt, k_seat_stmt), G is the table's fixed base, the commitments enter the checks as affine addends, and the prover builds
  // the window table of pk once for x pk and r pk.  What differs: the verifier's publics masked - in are computed here, one complete
  // mixed addition each and one batched inversion for all of them.  Static plans; the workspace stays with the table.
  struct DealState {
    bool ready = false;
    Phase vph, pph1, pph2, sph;     // checks of the verifier | (x G, x pk) | the commitments (r G, r pk) | checks of the seating proofs
    PhaseDev vdev, pdev1, pdev2, sdev;
    Phase kph1, kph2;               // key generation: pk = sk G | the commitment r G
    PhaseDev kdev1, kdev2;
    Phase qph1, qph2;               // dealing by index: x G | r G alone, the products with pk come from the key set's tables
    PhaseDev qdev1, qdev2;
    uint32_t nJ = 0, nD = 0, nT = 0;
    uint32_t fs_seed[2][8];         // Blake2s("Masking Proof"), Blake2s("Remasking Proof")  [REF mod.rs:80-81]
    Workspace w;
    DevBuf<uint8_t> fs;             // [lanes][32]
    DevBuf<uint32_t> sumJ, sumP, scratch;      // seating: one entry per table
  } deal;
  static SigmaLay seat_lay() {      // one base; the check slot is the dealing lanes' first one
    SigmaLay l = make_sigma_lay(1);
    l.chk = make_deal_lay().s.chk;
    return l;
  }
  void deal_prepare(uint32_t B) {
    rt::Stream s = ctx->stream;
    const DealLay d = make_deal_lay();
    const SigmaLay& l = d.s;
    if (!deal.ready) {
      FixedBases fb{n};
      const SigmaLay sl = seat_lay();
      uint32_t np = l.chk + 2;
      {
        PhaseBuilder pb(deal.vph, np, FCHUNK, VCHUNK);      // z g_i - c a_i - A_i, i = 0, 1
        pb.begin(l.chk);
        pb.fixed(l.z, fb.G());
        pb.var(l.negc, l.a);
        pb.addend(l.A, true);
        pb.end();
        pb.begin(l.chk + 1);
        pb.var(l.z, l.g + 1);
        pb.var(l.negc, l.a + 1);
        pb.addend(l.A + 1, true);
        pb.end();
      }
      {
        PhaseBuilder pb(deal.pph1, np, FCHUNK, VCHUNK);
        pb.begin(l.a);
        pb.fixed(l.x, fb.G());
        pb.end();
        pb.begin(l.a + 1);
        pb.var(l.x, l.g + 1);
        pb.end();
        pb.normalize(l.a, 2);
      }
      {
        PhaseBuilder pb(deal.pph2, np, FCHUNK, VCHUNK);
        pb.begin(l.A);
        pb.fixed(l.r, fb.G());
        pb.end();
        pb.begin(l.A + 1);
        pb.var(l.r, l.g + 1);
        pb.end();
        pb.normalize(l.A, 2);
      }
      {
        PhaseBuilder pb(deal.qph1, np, FCHUNK, VCHUNK);
        pb.begin(l.a);
        pb.fixed(l.x, fb.G());
        pb.end();
        pb.normalize(l.a, 2);
      }
      {
        PhaseBuilder pb(deal.qph2, np, FCHUNK, VCHUNK);
        pb.begin(l.A);
        pb.fixed(l.r, fb.G());
        pb.end();
        pb.normalize(l.A, 2);
      }
      {
        PhaseBuilder pb(deal.sph, np, FCHUNK, VCHUNK);      // z G - c pk - A
        pb.begin(sl.chk);
        pb.fixed(sl.z, fb.G());
        pb.var(sl.negc, sl.a);
        pb.addend(sl.A, true);
        pb.end();
      }
      {
        PhaseBuilder pb(deal.kph1, np, FCHUNK, VCHUNK);
        pb.begin(sl.a);
        pb.fixed(sl.x, fb.G());
        pb.end();
        pb.normalize(sl.a, 1);
      }
      {
        PhaseBuilder pb(deal.kph2, np, FCHUNK, VCHUNK);
        pb.begin(sl.A);
        pb.fixed(sl.r, fb.G());
        pb.end();
        pb.normalize(sl.A, 1);
      }
      // x pk and r pk share the base: both phases know the window table of pk as table slot 0, and the first one builds it
      if (deal.pph1.tables.size() != 1 || deal.pph2.tables.size() != 1 || deal.pph1.tables[0].s != l.g + 1 || deal.pph2.tables[0].s != l.g + 1 ||
          deal.pph1.tables[0].b != 0 || deal.pph2.tables[0].b != 0)
        throw std::logic_error("deal plan: the phases do not share the table of pk");
      deal.pph2.tables.clear();
      deal.nJ = np;
      for (const Phase* ph : {&deal.vph, &deal.pph1, &deal.pph2, &deal.sph, &deal.kph1, &deal.kph2, &deal.qph1, &deal.qph2}) {
        deal.nD = std::max(deal.nD, ph->n_dslots);
        deal.nT = std::max(deal.nT, ph->n_tslots);
      }
      deal.vdev.upload(deal.vph, s);
      deal.pdev1.upload(deal.pph1, s);
      deal.pdev2.upload(deal.pph2, s);
      deal.sdev.upload(deal.sph, s);
      deal.kdev1.upload(deal.kph1, s);
      deal.kdev2.upload(deal.kph2, s);
      deal.qdev1.upload(deal.qph1, s);
      deal.qdev2.upload(deal.qph2, s);
      const char* names[2] = {"Masking Proof", "Remasking Proof"};
      for (int k = 0; k < 2; ++k) {
        Blake2sState st;
        blake2s_init(st);
        uint32_t mblk[16] = {0};
        memcpy(mblk, names[k], strlen(names[k]));
        blake2s_compress(st, mblk, (uint32_t)strlen(names[k]), true);
        memcpy(deal.fs_seed[k], st.h, 32);
      }
      deal.ready = true;
    }
    deal.w.fw = G_::FW;
    deal.w.ensure(B, 6, d.nP, deal.nJ, deal.nD, deal.nT, nwin, (6 * (G_::PB + 1) + 32) / 4 + 4, s);
    deal.fs.alloc((size_t)deal.w.cap * 32, s, false);
    rt::dzero(deal.w.status.p, (size_t)deal.w.Bpad * 4, s);
  }
  DealStmtArgs deal_stmt_args(int kind, size_t K, const uint8_t* keys, const uint32_t* key_index, const uint8_t* inputs,
                              const mp_keyset* ks = nullptr) {
    DealStmtArgs a{};
    if (ks) {      // dealing by index: the set's own copy of the wire keys, validated when they entered
      keys = reinterpret_cast<const uint8_t*>(ks->wire.p);
      K = ks->K;
      a.live = ks->live.p;
    }
    Workspace& w = deal.w;
    a.P = w.P.p; a.J = w.J.p; a.S = w.S.p; a.status = w.status.p;
    a.keys = keys; a.key_index = key_index; a.inputs = inputs;
    a.fbpts = fbpts.p;
    a.fs_init = deal.fs.p;
    memcpy(a.fs_seed, deal.fs_seed[kind == MP_DEAL_REMASK ? 1 : 0], 32);
    a.l = make_deal_lay();
    a.Bpad = w.Bpad; a.K = (uint32_t)K; a.g_base = FixedBases{n}.G(); a.remask = kind == MP_DEAL_REMASK ? 1u : 0u;
    return a;
  }
  // every pointer a device pointer; everything is enqueued on the context's stream
  void verify_mask_dev(int kind, size_t K, const uint8_t* keys, size_t C_, const uint32_t* key_index, const uint8_t* inputs,
                       const uint8_t* masked, const uint8_t* proofs, int32_t* status, const mp_keyset* ks) override {
    const uint32_t B = (uint32_t)C_;
    deal_prepare(B);
    Workspace& w = deal.w;
    const DealLay d = make_deal_lay();
    const SigmaLay& l = d.s;
    DealStmtArgs sa = deal_stmt_args(kind, K, keys, key_index, inputs, ks);
    sa.masked = masked;
    MP_RUN(k_deal_stmt, C, B, 4, sa);
    // the publics a_i = masked_i - in_i become affine before the transcript absorbs them: one batched inversion for both slots
    normalize_flat(w.J.p + j_off<C>(l.a, w.Bpad, 0), w.P.p + p_off<C>(l.a, w.Bpad, 0), w.NS.p, (size_t)2 * w.Bpad);
    SigmaIoArgs io{const_cast<uint8_t*>(proofs), w.S.p, w.P.p, w.status.p, l, w.Bpad};
    MP_RUN(k_sigma_load, C, B, 3, io);
    if (!ks) check_subgroup(w, B, l.g + 1, 1);      // the key (G is the table's own; the differences of subgroup points are subgroup points; a set's keys were tested when they entered)
    check_subgroup(w, B, l.A, 6);          // commitments, input card and masked card are consecutive P slots
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    SigmaFsArgs fa{f, w.S.p, w.P.p, deal.fs.p, l, 0};
    MP_RUN(k_sigma_fs, C, B, 1, fa);
    if (!screen_sigma(w, B, ScreenCall{l, 0, deal.vdev, d.nP, deal.nJ, deal.nD, deal.nT, 6})) {
      run_phase(deal.vdev, w, B);
      SigmaVerdictArgs va{w.J.p, w.status.p, l, w.Bpad, 6};
      MP_RUN(k_sigma_verdict, C, B, 1, va);
    }
    DealFinishArgs fin{w.status.p, key_index, status, nullptr, nullptr, sa.K, sa.live};
    MP_RUN(k_deal_finish, C, B, 1, fin);
  }
  static size_t deal_input_bytes(int kind) { return (kind == MP_DEAL_REMASK ? 2 : 1) * (size_t)G_::PB; }
  void verify_mask_host(int kind, size_t K, const uint8_t* keys, size_t C_, const uint32_t* key_index, const uint8_t* inputs,
                        const uint8_t* masked, const uint8_t* proofs, int32_t* status, const mp_keyset* ks) override {
    rt::Stream s = ctx->stream;
    const size_t psz = 2 * (size_t)G_::PB + 32, isz = deal_input_bytes(kind);
    DevBuf<uint8_t> dk, din, dm, dp;
    DevBuf<uint32_t> dki;
    DevBuf<int32_t> dst;
    if (ks) K = 0;
    dk.alloc(K * G_::PB, s, false); din.alloc(C_ * isz, s, false); dm.alloc(C_ * 2 * G_::PB, s, false); dp.alloc(C_ * psz, s, false);
    dki.alloc(C_, s, false); dst.alloc(C_, s, false);
    if (K) rt::h2d(dk.p, keys, K * G_::PB, s);
    rt::h2d(din.p, inputs, C_ * isz, s);
    rt::h2d(dm.p, masked, C_ * 2 * G_::PB, s);
    rt::h2d(dp.p, proofs, C_ * psz, s);
    rt::h2d(dki.p, key_index, C_ * 4, s);
    verify_mask_dev(kind, K, dk.p, C_, dki.p, din.p, dm.p, dp.p, dst.p, ks);
    rt::d2h(status, dst.p, C_ * 4, s);
    rt::stream_sync(s);
  }
  // (x G, x pk) first: the hedged nonce hashes the whole statement, the publics included (k_sigma_init)
  void mask_host(int kind, size_t K, const uint8_t* keys, size_t C_, const uint32_t* key_index, const uint8_t* inputs, const uint8_t* factors,
                 const uint8_t* seeds, uint8_t* out_masked, uint8_t* out_proofs, int32_t* status, const mp_keyset* ks) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)C_;
    if (ks) K = 0;
    const size_t psz = 2 * (size_t)G_::PB + 32, isz = deal_input_bytes(kind);
    deal_prepare(B);
    Workspace& w = deal.w;
    const DealLay d = make_deal_lay();
    const SigmaLay& l = d.s;
    DevBuf<uint8_t> dk, din, dx, dseed, dm, dpf;
    DevBuf<uint32_t> dki;
    DevBuf<int32_t> dst;
    dk.alloc(K * G_::PB, s, false); din.alloc(C_ * isz, s, false); dx.alloc(C_ * 32, s, false); dseed.alloc(C_ * 32, s, false);
    dm.alloc(C_ * 2 * G_::PB, s, false); dpf.alloc(C_ * psz, s, false); dki.alloc(C_, s, false); dst.alloc(C_, s, false);
    if (K) rt::h2d(dk.p, keys, K * G_::PB, s);
    rt::h2d(din.p, inputs, C_ * isz, s);
    rt::h2d(dx.p, factors, C_ * 32, s);
    rt::h2d(dseed.p, seeds, C_ * 32, s);
    rt::h2d(dki.p, key_index, C_ * 4, s);
    DealStmtArgs sa = deal_stmt_args(kind, K, dk.p, dki.p, din.p, ks);
    sa.factors = dx.p;
    MP_RUN(k_deal_stmt, C, B, 4, sa);
    if (!ks) check_subgroup(w, B, l.g + 1, 1);      // the key and the input card, as the sigma calls test bases and publics
    check_subgroup(w, B, d.in, 2);
    // by index: x pk and r pk are sums of entries of the set's tables (k_deal_key_term) beside x G and r G from the table's own; the
    // phase's normalisation takes both slots
    auto key_term = [&](uint32_t s_slot, uint32_t j_slot) {
      DealKeyTermArgs ka{w.S.p, w.J.p, w.Bpad, s_slot, j_slot, ks->FB.p, dki.p, ks->live.p, FbGeom{ks->bits, ks->windows, ks->entries}, (uint32_t)ks->K};
      MP_RUN(k_deal_key_term, C, B, 1, ka);
    };
    if (ks) {
      run_phase(deal.qdev1, w, B, PH_ALL & ~PH_NORM);
      key_term(l.x, l.a + 1);
      run_phase(deal.qdev1, w, B, PH_NORM);
    } else {
      run_phase(deal.pdev1, w, B);
    }
    DealAddArgs aa{w.P.p, w.J.p, d, w.Bpad};
    MP_RUN(k_deal_add, C, B, 2, aa);
    normalize_flat(w.J.p + j_off<C>(d.out, w.Bpad, 0), w.P.p + p_off<C>(d.out, w.Bpad, 0), w.NS.p, (size_t)2 * w.Bpad);
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    SigmaInitArgs ia{w.S.p, dseed.p, l, w.Bpad, f, w.P.p, deal.fs.p};
    MP_RUN(k_sigma_init, C, B, 1, ia);
    if (ks) {
      run_phase(deal.qdev2, w, B, PH_ALL & ~PH_NORM);
      key_term(l.r, l.A + 1);
      run_phase(deal.qdev2, w, B, PH_NORM);
    } else {
      run_phase(deal.pdev2, w, B);             // (its table list is empty: the table of pk is the first phase's)
    }
    SigmaFsArgs fa{f, w.S.p, w.P.p, deal.fs.p, l, 1};
    MP_RUN(k_sigma_fs, C, B, 1, fa);
    SigmaIoArgs io{dpf.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
    MP_RUN(k_sigma_store, C, B, 3, io);
    StorePointsArgs so{dm.p, w.P.p, w.Bpad, 2, d.out};
    MP_RUN(k_store_points, C, B, 2, so);
    DealFinishArgs fin{w.status.p, dki.p, dst.p, dm.p, dpf.p, sa.K, sa.live};
    MP_RUN(k_deal_finish, C, B, 1, fin);
    rt::d2h(out_masked, dm.p, C_ * 2 * G_::PB, s);
    rt::d2h(out_proofs, dpf.p, C_ * psz, s);
    rt::d2h(status, dst.p, C_ * 4, s);
    rt::stream_sync(s);
  }
  // seating: lane = table * seats + seat, or with an offsets array the lanes first[table] .. first[table + 1] - 1
  void aggregate_keys_host(size_t tables, uint32_t seats, const uint8_t* keys, const uint8_t* proofs, const uint8_t* fs_init, uint8_t* out_keys,
                           int32_t* player_status, int32_t* table_status, const uint32_t* first, size_t lanes, mp_keyset* seat_ks,
                           const uint32_t* d_slots, int32_t* slot_status) override {
    rt::Stream s = ctx->stream;
    const uint32_t Tn = (uint32_t)tables, B = first ? (uint32_t)lanes : Tn * seats;
    const size_t psz = (size_t)G_::PB + 32;
    deal_prepare(B);
    Workspace& w = deal.w;
    const SigmaLay l = seat_lay();
    DevBuf<uint8_t> dk, dp, dout;
    DevBuf<int32_t> dps, dts;
    dk.alloc((size_t)B * G_::PB, s, false); dp.alloc((size_t)B * psz, s, false); dout.alloc((size_t)Tn * G_::PB, s, false);
    dps.alloc(B, s, false); dts.alloc(Tn, s, false);
    deal.sumJ.alloc((size_t)Tn * G_::JW, s, false); deal.sumP.alloc((size_t)Tn * G_::PW, s, false); deal.scratch.alloc((size_t)Tn * G_::FW, s, false);
    rt::h2d(dk.p, keys, (size_t)B * G_::PB, s);
    rt::h2d(dp.p, proofs, (size_t)B * psz, s);
    rt::h2d(deal.fs.p, fs_init, (size_t)B * 32, s);
    SeatStmtArgs sa{w.P.p, w.status.p, dk.p, fbpts.p, l, w.Bpad, FixedBases{n}.G()};
    MP_RUN(k_seat_stmt, C, B, 2, sa);
    SigmaIoArgs io{dp.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
    MP_RUN(k_sigma_load, C, B, 2, io);
    check_subgroup(w, B, l.a, 2);          // key and commitment are consecutive P slots
    const FsDev f{w.stage.p, w.seed.p, w.Bpad};
    SigmaFsArgs fa{f, w.S.p, w.P.p, deal.fs.p, l, 0};
    MP_RUN(k_sigma_fs, C, B, 1, fa);
    if (!screen_sigma(w, B, ScreenCall{l, 0, deal.sdev, make_deal_lay().nP, deal.nJ, deal.nD, deal.nT, 5})) {
      run_phase(deal.sdev, w, B);
      SigmaVerdictArgs va{w.J.p, w.status.p, l, w.Bpad, 5};
      MP_RUN(k_sigma_verdict, C, B, 1, va);
    }
    KeySumArgs ka{w.P.p, w.status.p, deal.sumJ.p, dps.p, dts.p, w.Bpad, seats, l.a, first};
    MP_RUN(k_key_sum, C, Tn, 1, ka);
    normalize_flat(deal.sumJ.p, deal.sumP.p, deal.scratch.p, Tn);
    StorePointsArgs so{dout.p, deal.sumP.p, Tn, 1, 0};      // (the identity is zero bytes on the wire: a refused table's key)
    MP_RUN(k_store_points, C, Tn, 1, so);
    DevBuf<int32_t> dss;
    if (seat_ks) {
      // the sums never leave HBM: they enter the set through the validation and the table build of an update.  A refused table's sum
      // is the identity, which the validation refuses: its slot is emptied, as for keys that cancel
      dss.alloc(Tn, s, false);
      keyset_update(*seat_ks, Tn, d_slots, dout.p, dss.p);
      KeysetSeatStatusArgs ss{dts.p, dss.p};
      MP_RUN(k_keyset_seat_status, C, Tn, 1, ss);
      rt::d2h(slot_status, dss.p, (size_t)Tn * 4, s);
    }
    if (out_keys) rt::d2h(out_keys, dout.p, (size_t)Tn * G_::PB, s);
    rt::d2h(player_status, dps.p, (size_t)B * 4, s);
    rt::d2h(table_status, dts.p, (size_t)Tn * 4, s);
    rt::stream_sync(s);
  }

  // ---------------------------------------------------------------- secrets from seeds (kernels_sample.hpp)
  // One lane per seed; nothing is allocated and nothing waits: a seeded prove call is this launch in front of prove_dev.
  void sample_dev(size_t L, const uint8_t* seeds, uint32_t S, uint32_t P, uint8_t* out_scalars, uint32_t* out_perms) override {
    SampleArgs a{seeds, out_scalars, out_perms, S, P};
    MP_RUN(k_sample_secrets, C, (uint32_t)L, 1, a);
  }
  void sample_host(size_t L, const uint8_t* seeds, uint32_t S, uint32_t P, uint8_t* out_scalars, uint32_t* out_perms) override {
    rt::Stream s = ctx->stream;
    DevBuf<uint8_t> dseed, dsc;
    DevBuf<uint32_t> dpm;
    dseed.alloc(L * 32, s, false);
    if (S) dsc.alloc(L * S * 32, s, false);
    if (P) dpm.alloc(L * P, s, false);
    rt::h2d(dseed.p, seeds, L * 32, s);
    sample_dev(L, dseed.p, S, P, dsc.p, dpm.p);
    if (S) rt::d2h(out_scalars, dsc.p, L * S * 32, s);
    if (P) rt::d2h(out_perms, dpm.p, L * P * 4, s);
    rt::stream_sync(s);
  }
  // Key generation [REF mod.rs:123-149]: the secret key goes from the sampler's output into the statement on the device; pk = sk G
  // and the commitment r G come from the table's fixed-base table, the transcript is that of the seating lanes (one base).
  void keygen_host(size_t K_, const uint8_t* seeds, const uint8_t* fs_init, uint8_t* out_keys, uint8_t* out_secret_keys, uint8_t* out_proofs,
                   int32_t* status) override {
    rt::Stream s = ctx->stream;
    const uint32_t B = (uint32_t)K_;
    const size_t psz = (size_t)G_::PB + 32;
    deal_prepare(B);
    Workspace& w = deal.w;
    const SigmaLay l = seat_lay();
    DevBuf<uint8_t> dseed, dsk, dpk, dpf;
    dseed.alloc((size_t)B * 32, s, false); dsk.alloc((size_t)B * 32, s, false); dpk.alloc((size_t)B * G_::PB, s, false);
    rt::h2d(dseed.p, seeds, (size_t)B * 32, s);
    sample_dev(B, dseed.p, 1, 0, dsk.p, nullptr);
    KeygenStmtArgs ka{w.P.p, fbpts.p, l.g, w.Bpad, FixedBases{n}.G()};
    MP_RUN(k_keygen_stmt, C, B, 1, ka);
    LoadScalarsArgs lx{dsk.p, w.S.p, w.status.p, w.Bpad, 1, l.x};
    MP_RUN(k_load_scalars, C, B, 1, lx);
    run_phase(deal.kdev1, w, B);
    StorePointsArgs so{dpk.p, w.P.p, w.Bpad, 1, l.a};
    MP_RUN(k_store_points, C, B, 1, so);
    if (fs_init) {
      dpf.alloc((size_t)B * psz, s, false);
      rt::h2d(deal.fs.p, fs_init, (size_t)B * 32, s);
      const FsDev f{w.stage.p, w.seed.p, w.Bpad};
      SigmaInitArgs ia{w.S.p, dseed.p, l, w.Bpad, f, w.P.p, deal.fs.p};
      MP_RUN(k_sigma_init, C, B, 1, ia);
      run_phase(deal.kdev2, w, B);
      SigmaFsArgs fa{f, w.S.p, w.P.p, deal.fs.p, l, 1};
      MP_RUN(k_sigma_fs, C, B, 1, fa);
      SigmaIoArgs io{dpf.p, w.S.p, w.P.p, w.status.p, l, w.Bpad};
      MP_RUN(k_sigma_store, C, B, 2, io);
      rt::d2h(out_proofs, dpf.p, (size_t)B * psz, s);
    }
    rt::d2h(out_keys, dpk.p, (size_t)B * G_::PB, s);
    rt::d2h(out_secret_keys, dsk.p, (size_t)B * 32, s);
    rt::d2h(status, w.status.p, (size_t)B * 4, s);
    rt::stream_sync(s);
  }

  void census(uint64_t* pt, uint64_t* vt, uint64_t* po, uint64_t* vo) override {
    auto count = [&](const Phase& ph, uint64_t& terms, uint64_t& ops) {
      terms += ph.fterms.size() + ph.vterms.size();
      ops += (uint64_t)ph.fterms.size() * fbg.windows;                      // mixed additions
      ops += (uint64_t)ph.vterms.size() * nwin;                             // mixed additions
      ops += (uint64_t)ph.vjobs.size() * (nwin - 1) * VB_WINDOW_BITS;       // doublings
      ops += (uint64_t)ph.tables.size() * (VB_ENTRIES - 1);                 // table construction (affine additions)
      ops += ph.cterms.size() + ph.cterms2.size() + ph.cterms0.size();      // combines
      terms += ph.bterms.size();
      const uint32_t bwin = bk_windows(R::BITS, ph.b_bits), bnb = bk_buckets(ph.b_bits) / 64;
      ops += (uint64_t)ph.bterms.size() * bwin;                             // bucket method: one mixed addition per term and window
      ops += (uint64_t)ph.bjobs.size() * bwin * (13 + 2 * bnb - 3 + ph.b_bits + 1);   // wave-wide reduction + fold
    };
    uint64_t t = 0, o = 0;
    for (int i = 0; i < 6; ++i) count(ps[0].pplan.ph[i], t, o);
    t += 2 * N;
    o += (uint64_t)2 * N * (fbg.windows + 1);  // remask
    *pt = t; *po = o;
    t = 0; o = 0;
    count(merged_verify ? ps[0].vplan.mph : ps[0].vplan.ph, t, o);
    *vt = t; *vo = o;
  }
};

// DLCards::setup [REF mod.rs:105-121]: n + 3 independent `C::rand` points (setup_host.hpp) -- host work, once per table
template <class C>
static void aff_to_wire_host(const Aff<C>& a, uint8_t* out) {
  alignas(8) uint8_t tmp[Geo<C>::PB];
  aff_to_wire<C>(a, tmp);
  memcpy(out, tmp, Geo<C>::PB);
}
template <class C>
static int setup_device(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t seed[32], uint8_t* out) {
  (void)ctx;
  (void)m;
  setup_points_host<C>(n, seed, out, &aff_to_wire_host<C>, Geo<C>::PB);
  return MP_OK;
}

// ---- on-device point decompression (kernels_decompress.hpp): square-root tables of the base field, once per context (host work with
// the kernels' own field code), then one lane per point
template <class C>
static void build_sqrt_tables(mp_ctx* ctx) {
  typedef typename C::FqP F;
  constexpr int W = F::NW;
  uint32_t q[W], half[W], e[W];
  for (int i = 0; i < W; ++i) q[i] = F::MOD[i];
  q[0] -= 1u;                                                // p - 1
  auto shr1 = [](uint32_t* r, const uint32_t* x) {
    for (int i = 0; i < W; ++i) r[i] = (x[i] >> 1) | (i + 1 < W ? x[i + 1] << 31 : 0u);
  };
  shr1(half, q);                                             // (p - 1) / 2
  uint32_t S = 0;
  while (!(q[0] & 1u)) {
    shr1(q, q);
    ++S;
  }
  for (int i = 0; i < W; ++i) e[i] = q[i];
  e[0] -= 1u;                                                // q odd
  shr1(e, e);                                                // (q - 1) / 2
  const uint32_t w = S % 4 == 0 ? 4u : (S % 2 == 0 ? 2u : 1u), k = S / w, nd = 1u << w;
  const Fe<F> one = fe_one<F>(), minus_one = fe_neg<F>(one);
  Fe<F> z = fe_from_u32<F>(2);
  for (uint32_t c = 2; !fe_eq<F>(fe_pow_host<F>(z, half, W), minus_one); ++c) z = fe_from_u32<F>(c + 1);      // smallest non-residue
  const Fe<F> g = fe_pow_host<F>(z, q, W), ginv = fe_inv<F>(g);
  std::vector<uint32_t> t_ghalf((size_t)k * nd * W, 0u), t_hh((size_t)nd * W);
  Fe<F> gi = ginv, gh = ginv;                                // gi = ginv^(2^(w i)); gh = ginv^(2^(w i - 1)) for i >= 1
  for (uint32_t i = 0; i < k; ++i) {
    if (i) {
      gh = gi;                                               // still ginv^(2^(w (i-1)))
      for (uint32_t j = 0; j + 1 < w; ++j) gh = fe_sqr<F>(gh);
      gi = fe_sqr<F>(gh);
    }
    Fe<F> ph = one;
    for (uint32_t d = 0; d < nd; ++d) {
      if (i) {
        fe_pack<F>(ph, &t_ghalf[((size_t)i * nd + d) * W]);
        ph = fe_mul<F>(ph, gh);
      } else if (!(d & 1u)) {
        fe_pack<F>(ph, &t_ghalf[(size_t)d * W]);             // ginv^(d / 2)
        ph = fe_mul<F>(ph, ginv);
      }
    }
  }
  // R[c][d] = ginv^(d 2^(S - w c)), c = 1 .. k (c = k: ginv itself; row 1 is h^-d, unused; row 0 empty)
  std::vector<uint32_t> t_rr((size_t)(k + 1) * nd * W, 0u);
  {
    Fe<F> base = ginv;                                       // ginv^(2^(S - w c)) for c = k, k-1, ..
    for (uint32_t c = k; c >= 1; --c) {
      Fe<F> pr = one;
      for (uint32_t d = 0; d < nd; ++d) {
        fe_pack<F>(pr, &t_rr[((size_t)c * nd + d) * W]);
        pr = fe_mul<F>(pr, base);
      }
      for (uint32_t j = 0; j < w; ++j) base = fe_sqr<F>(base);
    }
  }
  ctx->sq_rr.upload(t_rr, ctx->stream);
  Fe<F> h = g;
  for (uint32_t j = 0; j < S - w; ++j) h = fe_sqr<F>(h);      // order 2^w
  Fe<F> hp = one;
  for (uint32_t d = 0; d < nd; ++d) {
    fe_pack<F>(hp, &t_hh[(size_t)d * W]);
    hp = fe_mul<F>(hp, h);
  }
  ctx->sq_ghalf.upload(t_ghalf, ctx->stream);
  ctx->sq_hh.upload(t_hh, ctx->stream);
  uint32_t ebits = 32 * W;
  while (ebits && !((e[(ebits - 1) >> 5] >> ((ebits - 1) & 31)) & 1u)) --ebits;
  ctx->sq_geom[0] = S; ctx->sq_geom[1] = w; ctx->sq_geom[2] = k; ctx->sq_geom[3] = ebits;
  for (int i = 0; i < 12; ++i) ctx->sq_exp[i] = i < W ? e[i] : 0u;
  rt::stream_sync(ctx->stream);
}
template <class C>
static int decompress_device(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const uint8_t* d_in, uint8_t* d_out,
                             int32_t* d_status) {
  if (!ctx->sq_geom[0]) build_sqrt_tables<C>(ctx);
  if ((uint64_t)groups * per_group >= ((uint64_t)1 << 32)) return fail(MP_ERR_BAD_ARGUMENT, "point decompression: too many points for one call");
  rt::dzero(d_status, groups * sizeof(int32_t), ctx->stream);
  DecompressArgs a{};
  a.in = d_in; a.out = d_out; a.status = d_status;
  a.ghalf = ctx->sq_ghalf.p; a.hh = ctx->sq_hh.p; a.rr = ctx->sq_rr.p;
  a.per_group = per_group; a.prefix = prefix;
  a.g = SqrtGeom{ctx->sq_geom[0], ctx->sq_geom[1], ctx->sq_geom[2], ctx->sq_geom[3]};
  for (int i = 0; i < 12; ++i) a.e[i] = ctx->sq_exp[i];
  // launches of up to 2^20 points: the scratch column of a point (its chain of k - 1 powers) is 1.5 KB on the STARK prime
  const size_t total = groups * per_group, chunk = std::min<size_t>(total, (size_t)1 << 20);
  if (a.g.k > 1) ctx->sq_chain.alloc((size_t)(a.g.k - 1) * chunk * C::FqP::NW, ctx->stream, false);
  a.chain = ctx->sq_chain.p;
  for (size_t off = 0; off < total; off += chunk) {
    a.first = (uint32_t)off;
    a.lanes = (uint32_t)std::min(chunk, total - off);
    MP_RUN(k_decompress, C, a.lanes, 1, a);
  }
  return MP_OK;
}

// ---- the other canonical conversions on the device (kernels_canonical.hpp).  Launches of up to 2^22 elements: nothing here has a scratch
// column, the cut only keeps the grid of a launch small
static const size_t CANON_LAUNCH = (size_t)1 << 22;
// wire -> canonical: `groups` x `per_group` points; tab = null: uniform groups behind `prefix` bytes (points: 1, 0; decks: 2 cards, 8),
// else the proof's element table
template <class C>
static int compress_device(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const uint32_t* tab, uint32_t wire_stride,
                           uint32_t canon_stride, const uint8_t* d_in, uint8_t* d_out, int32_t* d_status, bool zero_status) {
  if ((uint64_t)groups * per_group >= ((uint64_t)1 << 32)) return fail(MP_ERR_BAD_ARGUMENT, "point compression: too many points for one call");
  if (zero_status) rt::dzero(d_status, groups * sizeof(int32_t), ctx->stream);
  CompressArgs a{};
  a.in = d_in; a.out = d_out; a.status = d_status; a.tab = tab;
  a.per_group = per_group; a.prefix = prefix;
  a.wire_stride = wire_stride; a.canon_stride = canon_stride;
  const size_t total = groups * per_group;
  for (size_t off = 0; off < total; off += CANON_LAUNCH) {
    a.first = (uint32_t)off;
    MP_RUN(k_compress, C, (uint32_t)std::min(CANON_LAUNCH, total - off), 1, a);
  }
  return MP_OK;
}
// B proofs, either direction, through the context's element table (capi.hip: canon_table; np point and ns scalar entries)
template <class C>
static int proof_convert_device(mp_ctx* ctx, bool de, uint32_t np, uint32_t ns, uint32_t canon_stride, uint32_t wire_stride, size_t B,
                                const uint8_t* d_in, uint8_t* d_out, int32_t* d_status) {
  if ((uint64_t)B * np >= ((uint64_t)1 << 32) || (uint64_t)B * ns >= ((uint64_t)1 << 32))
    return fail(MP_ERR_BAD_ARGUMENT, "proof conversion: too many proofs for one call");
  if (de && !ctx->sq_geom[0]) build_sqrt_tables<C>(ctx);
  rt::dzero(d_status, B * sizeof(int32_t), ctx->stream);
  const uint32_t* tab = ctx->cn_tab.p;
  if (!de) {
    const int rc = compress_device<C>(ctx, B, np, 0, tab, wire_stride, canon_stride, d_in, d_out, d_status, false);
    if (rc) return rc;
  } else {
    DecompressMapArgs a{};
    a.d.in = d_in; a.d.out = d_out; a.d.status = d_status;
    a.d.ghalf = ctx->sq_ghalf.p; a.d.hh = ctx->sq_hh.p; a.d.rr = ctx->sq_rr.p;
    a.d.per_group = np; a.d.prefix = 0;
    a.d.g = SqrtGeom{ctx->sq_geom[0], ctx->sq_geom[1], ctx->sq_geom[2], ctx->sq_geom[3]};
    for (int i = 0; i < 12; ++i) a.d.e[i] = ctx->sq_exp[i];
    a.tab = tab; a.canon_stride = canon_stride; a.wire_stride = wire_stride;
    // the launches of decompress_device: 2^20 points each, one scratch column per lane of a launch
    const size_t total = B * np, chunk = std::min<size_t>(total, (size_t)1 << 20);
    if (a.d.g.k > 1) ctx->sq_chain.alloc((size_t)(a.d.g.k - 1) * chunk * C::FqP::NW, ctx->stream, false);
    a.d.chain = ctx->sq_chain.p;
    for (size_t off = 0; off < total; off += chunk) {
      a.d.first = (uint32_t)off;
      a.d.lanes = (uint32_t)std::min(chunk, total - off);
      MP_RUN(k_decompress_map, C, a.d.lanes, 1, a);
    }
  }
  ScalarMapArgs s{};
  s.in = d_in; s.out = d_out; s.status = d_status; s.tab = tab + 3 * (size_t)np;
  s.per_group = ns; s.canon_stride = canon_stride; s.wire_stride = wire_stride; s.de = de ? 1u : 0u;
  const size_t total = B * ns;
  for (size_t off = 0; off < total; off += CANON_LAUNCH) {
    s.first = (uint32_t)off;
    MP_RUN(k_scalar_map, C, (uint32_t)std::min(CANON_LAUNCH, total - off), 1, s);
  }
  return MP_OK;
}

}  // namespace mp

#define MP_DEFINE_CURVE(NAME)                                                                                  \
  namespace mp {                                                                                               \
  mp_table* make_table_##NAME(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* pk,  \
                              uint32_t fb_bits, int* rc, const mp_table* fb_from) {                            \
    std::unique_ptr<Table<NAME>> p(new Table<NAME>());      /* (an init that throws -- out of memory -- gives everything back) */ \
    *rc = p->init(ctx, m, n, params, pk, fb_bits, fb_from);                                                    \
    return p.release();                                                                                        \
  }                                                                                                            \
  int setup_##NAME(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t seed[32], uint8_t* out) {                \
    return setup_device<NAME>(ctx, m, n, seed, out);                                                           \
  }                                                                                                            \
  long ser_points_##NAME(bool de, size_t count, const uint8_t* in, uint8_t* out) {                             \
    return Ser<NAME>::points(de, count, in, out);                                                              \
  }                                                                                                            \
  bool ser_scalars_ok_##NAME(size_t count, const uint8_t* in) { return Ser<NAME>::scalars_ok(count, in); }     \
  int decompress_dev_##NAME(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const uint8_t* d_in,  \
                            uint8_t* d_out, int32_t* d_status) {                                               \
    return decompress_device<NAME>(ctx, groups, per_group, prefix, d_in, d_out, d_status);                     \
  }                                                                                                            \
  int compress_dev_##NAME(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const uint8_t* d_in,    \
                          uint8_t* d_out, int32_t* d_status) {                                                 \
    return compress_device<NAME>(ctx, groups, per_group, prefix, nullptr, per_group * Geo<NAME>::PB,           \
                                 prefix + per_group * Ser<NAME>::CB, d_in, d_out, d_status, true);             \
  }                                                                                                            \
  int proof_convert_dev_##NAME(mp_ctx* ctx, bool de, uint32_t np, uint32_t ns, uint32_t canon_stride,          \
                               uint32_t wire_stride, size_t B, const uint8_t* d_in, uint8_t* d_out,            \
                               int32_t* d_status) {                                                            \
    return proof_convert_device<NAME>(ctx, de, np, ns, canon_stride, wire_stride, B, d_in, d_out, d_status);   \
  }                                                                                                            \
  }
