// capi.hip -- the C ABI of libmpshuffle.so (include/mpshuffle.h): argument checking, error mapping and
// dispatch to the per-curve engines (curve_*.hip).  Mirrors DLCards::{setup, shuffle_and_remask, verify_shuffle}
// [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:105-121, 380-418, 420-443].
#include <algorithm>
#include <cstring>
#include <functional>

#include "engine_base.hpp"
#include "coalesce.hpp"
#include "pool.hpp"

namespace mp {
std::string& last_error() {
  static thread_local std::string e;
  return e;
}
static inline size_t proof_size_bytes_(uint32_t m, uint32_t n) { return proof_size_bytes(m, n); }
}  // namespace mp

using namespace mp;

// the context's lock for the length of the call + its device for this host thread (engine_base.hpp mp_ctx::mu)
#define MP_ENTER(CTX)                                          \
  std::lock_guard<std::recursive_mutex> mp_lock_((CTX)->mu);   \
  rt::set_device((CTX)->device)
#define MP_TRY try {
#define MP_CATCH                                                                     \
  }                                                                                  \
  catch (const std::invalid_argument& e) { return fail(MP_ERR_BAD_ENCODING, e.what()); } \
  catch (const std::exception& e) { return fail(MP_ERR_INTERNAL, e.what()); }

// ---- canonical (arkworks-0.3 compressed) serialisation of the trait's associated types: host work, no context ---------------
namespace {
long ser_points(int curve, bool de, size_t count, const uint8_t* in, uint8_t* out) {
  switch (curve) {
    case 0: return ser_points_Stark(de, count, in, out);
    case 1: return ser_points_Bn254(de, count, in, out);
    case 3: return ser_points_Bls12_377(de, count, in, out);
    default: return ser_points_Secp256k1(de, count, in, out);
  }
}
bool ser_scalars_ok(int curve, size_t count, const uint8_t* in) {
  switch (curve) {
    case 0: return ser_scalars_ok_Stark(count, in);
    case 1: return ser_scalars_ok_Bn254(count, in);
    case 3: return ser_scalars_ok_Bls12_377(count, in);
    default: return ser_scalars_ok_Secp256k1(count, in);
  }
}
const int kCurveBits[4] = {252, 254, 256, 377};
// element groups of the shuffle proof in wire order: {points?, count, is_vec, vec_len}
struct Group {
  bool point;
  uint32_t count;
  bool vec;
  uint32_t vec_len;
};
std::vector<Group> proof_schema(uint32_t m, uint32_t n) {
  return {
      {true, m, true, m}, {true, m, true, m}, {true, 1, false, 0}, {true, m, true, m},
      {true, 1, false, 0}, {true, 1, false, 0}, {true, 2 * m + 1, true, 2 * m + 1},
      {false, n, true, n}, {false, n, true, n}, {false, 1, false, 0}, {false, 1, false, 0}, {false, 1, false, 0},
      {true, 1, false, 0}, {true, 1, false, 0}, {true, 1, false, 0},
      {false, n, true, n}, {false, n, true, n}, {false, 1, false, 0}, {false, 1, false, 0},
      {true, 1, false, 0}, {true, 2 * m, true, 2 * m}, {true, 4 * m, true, 2 * m},      // E: 2m ciphertexts = 4m points
      {false, n, true, n}, {false, 1, false, 0}, {false, 1, false, 0}, {false, 1, false, 0}, {false, 1, false, 0}};
}
void put_u64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }
uint64_t get_u64(const uint8_t* p) {
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
}
bool curve_ok(int c) { return c >= 0 && c <= 3; }
// the host-buffer entry points and chain verification order their own transfers around verify_dev: not pipelined
struct NoPipeline {
  mp_table* t;
  int keep;
  explicit NoPipeline(mp_table* tt) : t(tt), keep(tt->pipeline) {
    if (keep) t->flush();
    t->pipeline = 0;
  }
  ~NoPipeline() { t->pipeline = keep; }
};
}  // namespace

extern "C" {

const char* mp_last_error(void) { return mp::last_error().c_str(); }
const char* mp_check_name(int code) {
  switch (code) {
    case 0: return "Ok";
    case 1: return "Hadamard Product (5.1)";
    case 2: return "Zero Argument (5.2)";
    case 3: return "Single Value Product (5.3)";
    case 4: return "Multi-Exponentiation Argument (4)";
    case 5: return "Schnorr Identification";
    case 6: return "Chaum-Pedersen";
    case MP_ERR_BAD_ENCODING: return "IoError: bad encoding";
    case MP_ERR_BAD_PERMUTATION: return "IoError: not a permutation";
    case MP_ERR_BAD_ARGUMENT: return "IoError: bad argument";
    case MP_ERR_NO_DEVICE: return "IoError: no MI355X device";
    default: return "IoError: internal";
  }
}
size_t mp_proof_size(uint32_t m, uint32_t n) { return proof_size_bytes(m, n); }
size_t mp_params_size(uint32_t n) { return (size_t)(n + 3) * 64; }
size_t mp_point_size(int curve_id) { return curve_id == MP_CURVE_BLS12_377 ? 96 : 64; }
size_t mp_proof_size_curve(int curve_id, uint32_t m, uint32_t n) { return proof_size_bytes(m, n, (uint32_t)mp_point_size(curve_id)); }
size_t mp_params_size_curve(int curve_id, uint32_t n) { return (size_t)(n + 3) * mp_point_size(curve_id); }

int mp_ctx_create(int curve_id, int device, mp_ctx** out) {
  if (!out) return fail(MP_ERR_BAD_ARGUMENT, "null out pointer");
  if (curve_id < 0 || curve_id > 3) return fail(MP_ERR_BAD_ARGUMENT, "unknown curve id");
  MP_TRY
  int ndev = rt::device_count();
  if (ndev <= 0 || device < 0 || device >= ndev)
    return fail(MP_ERR_NO_DEVICE, "no HIP device: libmpshuffle has no CPU path (runtime " MP_RT_NAME ")");
  rt::set_device(device);
  mp_ctx* c = new mp_ctx();
  c->curve = curve_id;
  c->device = device;
  // HIP streams become hardware queues in the order they are created, the queues sit on the compute pipes round robin (four of them), and
  // two streams overlap fully only on different pipes -- measured, not documented: with the verify lane's streams created fifth and sixth
  // (GPU_MAX_HW_QUEUES=8) or on first use, a pipelined 1 024-proof step ran at 172-176 k proofs/s; created second and fourth, at 198-202 k
  // with 4 or 8 queues.  So a context has exactly four streams, the two lanes interleaved; the host-buffer entry points -- which do not
  // pipeline their verify calls -- run their uploads and downloads on the verify lane's two streams (with copy streams of their own,
  // fifth and sixth, they lost 2-9 %).
  c->stream = rt::stream_create();
  c->vstream = rt::stream_create();
  c->side = rt::stream_create();
  c->vside = rt::stream_create();
  c->h2d = c->vstream;
  c->d2h = c->vside;
  c->ev_fork = rt::event_create();
  c->ev_shuf = rt::event_create();
  c->ev_tab = rt::event_create();
  c->ev_vfork = rt::event_create();
  c->ev_vshuf = rt::event_create();
  c->ev_vtab = rt::event_create();
  c->ev_vin = rt::event_create();
  *out = c;
  return MP_OK;
  MP_CATCH
}
static void ctx_release(mp_ctx* ctx) {
  for (rt::Stream st : {ctx->stream, ctx->side, ctx->vstream, ctx->vside})      // (h2d / d2h are the verify lane's)
    if (st) rt::stream_destroy(st);
  for (rt::Event e : {ctx->ev_fork, ctx->ev_shuf, ctx->ev_tab, ctx->ev_vfork, ctx->ev_vshuf, ctx->ev_vtab, ctx->ev_vin})
    if (e) rt::event_destroy(e);
  delete ctx;
}
void mp_ctx_destroy(mp_ctx* ctx) {
  if (!ctx) return;
  // tables hold a pointer to their context (streams, events, the registry mp_sync walks): a context that still has tables is only
  // marked and goes with the last of them (mp_table_destroy), so the two destroy calls may come in either order
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    if (!ctx->tables.empty()) {
      ctx->dying = true;
      return;
    }
  }
  ctx_release(ctx);
}
int mp_setup(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t seed[32], uint8_t* out_params) {
  if (!ctx || !seed || !out_params || m < 2 || n < 2) return fail(MP_ERR_BAD_ARGUMENT, "mp_setup: bad argument");
  MP_TRY
  MP_ENTER(ctx);
  switch (ctx->curve) {
    case 0: return setup_Stark(ctx, m, n, seed, out_params);
    case 1: return setup_Bn254(ctx, m, n, seed, out_params);
    case 3: return setup_Bls12_377(ctx, m, n, seed, out_params);
    default: return setup_Secp256k1(ctx, m, n, seed, out_params);
  }
  MP_CATCH
}

// mp_table_create: the widest fixed-base windows whose tables fit the HBM that is free right now.  A table of b-bit windows holds
// (n + 5) bases x ceil(scalar bits / b) windows x (2^b - 1) affine points; building it needs ~3.3x that for a moment (Jacobian
// entries and inversion scratch before the normalisation).  Rule: table <= 30 % of the free memory and the build <= 85 % of it.
static uint32_t auto_window_bits(int curve, uint32_t n) {
  size_t free_b = 0, total_b = 0;
  rt::mem_info(&free_b, &total_b);
  const uint32_t sbits[4] = {252, 254, 256, 253};
  const size_t pbytes = curve == MP_CURVE_BLS12_377 ? 96 : 64;
  for (uint32_t bits : {21u, 20u, 16u}) {
    if (bits == 21 && sbits[curve] > 252) continue;      // 21 bits only save a window on the 252-bit STARK scalars
    const double tbl = (double)(n + 5) * ((sbits[curve] + bits - 1) / bits) * (double)((1u << bits) - 1u) * (double)pbytes;
    if (tbl <= 0.30 * (double)free_b && 3.3 * tbl <= 0.85 * (double)free_b) return bits;
  }
  return 8;
}
int mp_table_create(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key, mp_table** out) {
  return mp_table_create_ex(ctx, m, n, params, shared_key, 0, out);
}
// fb_from: a table of the same parameters and key on the same device whose fixed-base tables the new one reads instead of building its
// own (the lanes of a pool, pool.hpp); it takes that table's window width
static int table_create(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key, uint32_t fb_window_bits,
                        const mp_table* fb_from, mp_table** out) {
  if (!ctx || !params || !shared_key || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_table_create: null pointer");
  if (m < 2 || n < 2 || (uint64_t)m * n > 4096) return fail(MP_ERR_BAD_ARGUMENT, "mp_table_create: need m >= 2, n >= 2, m*n <= 4096");
  MP_TRY
  MP_ENTER(ctx);
  if (fb_from) fb_window_bits = fb_from->fb_bits;
  const bool auto_bits = fb_window_bits == 0;
  if (auto_bits) fb_window_bits = auto_window_bits(ctx->curve, n);
  int rc = MP_OK;
  mp_table* t = nullptr;
  auto make = [&](uint32_t bits) {
    switch (ctx->curve) {
      case 0: return make_table_Stark(ctx, m, n, params, shared_key, bits, &rc, fb_from);
      case 1: return make_table_Bn254(ctx, m, n, params, shared_key, bits, &rc, fb_from);
      case 3: return make_table_Bls12_377(ctx, m, n, params, shared_key, bits, &rc, fb_from);
      default: return make_table_Secp256k1(ctx, m, n, params, shared_key, bits, &rc, fb_from);
    }
  };
  if (!auto_bits) {
    t = make(fb_window_bits);
  } else {
    // the width was chosen from ONE snapshot of the free memory: other ranks / contexts on this GPU may have taken it since (the
    // build needs ~3.3x the table for a moment).  A build that runs out of memory is retried with the next narrower windows
    for (;;) {
      try {
        t = make(fb_window_bits);
        break;
      } catch (const std::exception& e) {
        rt::clear_error();
        // (only a failed allocation is worth narrower windows: anything else would fail again)
        if (fb_window_bits <= 8 || (!strstr(e.what(), "hipMalloc") && !strstr(e.what(), "memory"))) throw;
        fb_window_bits = fb_window_bits > 20 ? 20 : (fb_window_bits > 16 ? 16 : 8);
      }
    }
  }
  if (rc != MP_OK) {
    delete t;
    return rc;
  }
  t->co = new mp_coalescer();
  ctx->tables.push_back(t);
  *out = t;
  return MP_OK;
  MP_CATCH
}
int mp_table_create_ex(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key,
                       uint32_t fb_window_bits, mp_table** out) {
  return table_create(ctx, m, n, params, shared_key, fb_window_bits, nullptr, out);
}
int mp_table_create_params(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, uint32_t fb_window_bits, mp_table** out) {
  // a table of the shared parameters only, for keyed batches: the enc generator G stands in for the (unused) fixed key
  int rc = mp_table_create_ex(ctx, m, n, params, params, fb_window_bits, out);
  if (rc == MP_OK) (*out)->keyless = true;
  return rc;
}
void mp_table_destroy(mp_table* t) {
  if (!t) return;
  try {
    MP_ENTER(t->ctx);
    t->flush();
  } catch (...) {
  }
  mp_ctx* ctx = t->ctx;
  bool last = false;
  {
    std::lock_guard<std::recursive_mutex> lock(ctx->mu);
    auto& reg = ctx->tables;
    reg.erase(std::remove(reg.begin(), reg.end(), t), reg.end());
    if (t->ragged_first_up) {
      try {
        rt::event_sync(t->ragged_first_up);
      } catch (...) {
      }
      rt::event_destroy(t->ragged_first_up);
    }
    if (t->ck_off_up) {
      try {
        rt::event_sync(t->ck_off_up);
      } catch (...) {
      }
      rt::event_destroy(t->ck_off_up);
    }
    if (t->cp_plan_up) {
      try {
        rt::event_sync(t->cp_plan_up);
      } catch (...) {
      }
      rt::event_destroy(t->cp_plan_up);
    }
    for (auto& st : t->io) {
      if (st.up) rt::event_destroy(st.up);
      if (st.done) rt::event_destroy(st.done);
      if (st.down) rt::event_destroy(st.down);
    }
    delete t->co;
    delete t;
    last = ctx->dying && reg.empty();
  }
  if (last) ctx_release(ctx);      // mp_ctx_destroy came first (the lock is not held: it goes with the context)
}
void* mp_host_alloc(size_t bytes) {
  try {
    return rt::host_alloc(bytes);
  } catch (const std::exception& e) {
    fail(MP_ERR_INTERNAL, e.what());
    return nullptr;
  }
}
void mp_host_free(void* p) { rt::host_free(p); }

uint32_t mp_table_window_bits(const mp_table* t) {
  if (!t) return 0;
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  return t->fb_bits;
}
int mp_set_latency_batch(mp_table* t, size_t B) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_latency_batch: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_latency_batch(B);
  return MP_OK;
}
int mp_set_io_chunk(mp_table* t, size_t proofs) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_io_chunk: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->io_chunk = proofs;
  return MP_OK;
}
int mp_set_merged_verify(mp_table* t, int on) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_merged_verify: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_merged_verify(on != 0);
  return MP_OK;
}
int mp_set_group_refine(mp_table* t, uint32_t points_per_subgroup, uint32_t min_subgroups) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_refine: null table");
  if (points_per_subgroup > BUCKET_TERMS_MAX - 4096) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_refine: at most 585 728 points per equation");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_group_refine(points_per_subgroup, min_subgroups);
  return MP_OK;
}
uint64_t mp_reverified_count(const mp_table* t) {
  if (!t) return 0;
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);      // (a verify call on another thread writes it)
  return t->reverified();
}
int mp_set_group_adapt(mp_table* t, int on) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_adapt: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_group_adapt(on != 0);
  return MP_OK;
}
int mp_set_bucket_min(mp_table* t, size_t terms) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_bucket_min: null table");
  MP_TRY
  MP_ENTER(t->ctx);
  t->set_bucket_min((uint32_t)std::min<size_t>(terms, 0x7FFFFFFFu));
  return MP_OK;
  MP_CATCH
}
int mp_set_bucket_bits(mp_table* t, uint32_t bits) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_bucket_bits: null table");
  if (bits != 0 && (bits < 8 || bits > 14)) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_bucket_bits: 0 (by size) or 8 .. 14");
  MP_TRY
  MP_ENTER(t->ctx);
  t->set_bucket_bits(bits);
  return MP_OK;
  MP_CATCH
}
int mp_set_bucket_split(mp_table* t, uint32_t min_bits) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_bucket_split: null table");
  if (min_bits < 10 || min_bits > 15) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_bucket_split: 10 .. 15 (none)");
  MP_TRY
  MP_ENTER(t->ctx);
  t->flush();
  t->bucket_split_bits = min_bits;
  return MP_OK;
  MP_CATCH
}
int mp_set_validated(mp_table* t, uint32_t what) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_validated: null table");
  if (what & ~(MP_VALIDATED_DECKS | MP_VALIDATED_SHUFFLED | MP_VALIDATED_PROOFS)) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_validated: unknown flag");
  MP_TRY
  MP_ENTER(t->ctx);
  t->flush();
  t->validated = what;
  return MP_OK;
  MP_CATCH
}
int mp_deck_validate_dev(mp_table* t, size_t decks, const void* d_wire_decks, void* d_status) {
  if (!t || !decks || !d_wire_decks || !d_status || decks >= ((size_t)1 << 31)) return fail(MP_ERR_BAD_ARGUMENT, "mp_deck_validate_dev: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->validate_decks_dev(decks, (const uint8_t*)d_wire_decks, (int32_t*)d_status);
  return MP_OK;
  MP_CATCH
}
int mp_set_chain_max_links(mp_table* t, uint32_t links) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_max_links: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->chain_max_links = links;
  return MP_OK;
}
int mp_set_chain_slice(mp_table* t, size_t tables_per_pass) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_slice: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->chain_slice = tables_per_pass;
  return MP_OK;
}
int mp_set_chain_group(mp_table* t, uint32_t tables_per_equation) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_group: null table");
  if (tables_per_equation > 4094) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_group: at most 4 094 tables per equation");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->chain_group = tables_per_equation;
  return MP_OK;
}
int mp_set_transcript_lanes(mp_table* t, uint32_t lanes) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_transcript_lanes: null table");
  if (lanes != 0 && lanes != 1 && lanes != 4) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_transcript_lanes: 0 (by batch size), 1 or 4");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->fs_lanes = lanes;
  return MP_OK;
}
int mp_set_group_lanes(mp_table* t, uint32_t lanes) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_lanes: null table");
  if (lanes != 0 && lanes != 1 && lanes != 4) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_lanes: 0 (by batch size), 1 or 4");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->group_lanes = lanes;
  return MP_OK;
}
int mp_set_work_split(mp_table* t, int split) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_work_split: null table");
  if (split < -1 || split > 5) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_work_split: -1 (by batch size) or 0 .. 5");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->forced_split = split;
  return MP_OK;
}
int mp_set_group_verify(mp_table* t, uint32_t points_per_group, size_t min_batch) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_verify: null table");
  if (points_per_group > BUCKET_TERMS_MAX - 4096) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_group_verify: 0 (off) or up to 585 728 points per group equation");
  MP_TRY
  MP_ENTER(t->ctx);
  t->flush();
  t->set_group_verify(points_per_group, min_batch);
  return MP_OK;
  MP_CATCH
}
uint32_t mp_group_size(const mp_table* t, size_t B) {
  if (!t) return 0;
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);      // (the group adaptation of a verify call on another thread writes it)
  return t->group_size_of(B);
}
// How a chain is cut: the links one chain equation takes at the most (0 = not even one: deck too large).  An equation holds at most
// 32 767 distinct points ((L + 1) 2N decks + L (11m + 8) proof elements + key): longer chains are verified as consecutive sub-chains,
// equations of their own.  One link does not always fit 32 767 points -- m = 2048, n = 2: 4N + 11m + 9 = 38 921 -- but it fits one
// bucket job: the kernel sorts up to BUCKET_TERMS_MAX = 65 535 points per window, and 4N + 11m + 9 <= 38 921 for every table
// mp_table_create accepts, m n <= 4096
static uint32_t chain_links_max(const mp_table* t) {
  const size_t per_link = (size_t)2 * t->N + 11 * t->m + 8, fixed_part = (size_t)2 * t->N + 1;
  const size_t eq_cap = fixed_part + per_link > 32767 ? (size_t)65535 : 32767;
  if (fixed_part + per_link > eq_cap) return 0;
  uint32_t lmax = std::min<uint32_t>((uint32_t)((eq_cap - fixed_part) / per_link), 1022u);      // (links 0 .. L in 10 bits of a sorted entry: kernels_bucket.hpp)
  if (t->chain_max_links) lmax = std::max(1u, std::min(lmax, t->chain_max_links));
  return lmax;
}
uint32_t mp_chain_group_size(const mp_table* t, size_t tables, uint32_t links, int keyed) {
  if (!t || !tables || !links) return 0;
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  const uint32_t lmax = chain_links_max(t);      // (as mp_verify_shuffle_chain_dev cuts the chain)
  return lmax ? t->chain_group_size(tables, std::min(lmax, links), keyed != 0) : 0;
}
size_t mp_chain_last_slice(const mp_table* t) {
  if (!t) return 0;
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  return t->chain_last_slice;
}
int mp_set_pipeline(mp_table* t, int depth) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_pipeline: null table");
  MP_TRY
  MP_ENTER(t->ctx);
  if (depth < 0 || depth > 8) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_pipeline: depth 0 (off) .. 8");
  t->flush();
  t->pipeline = depth;
  return MP_OK;
  MP_CATCH
}
int mp_set_plan_params(mp_table* t, int split, uint32_t fixed_terms, uint32_t var_terms, uint32_t table_group, uint32_t norm_chunk,
                       uint32_t window_lanes) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_plan_params: null table");
  MP_TRY
  MP_ENTER(t->ctx);
  if (t->set_plan_params(split, fixed_terms, var_terms, table_group, norm_chunk, window_lanes) != MP_OK)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_set_plan_params: split 0 .. 5, sizes >= 1, table_group <= 64, window_lanes <= 16");
  return MP_OK;
  MP_CATCH
}
int mp_set_plan_thresholds(mp_table* t, size_t finest, size_t small, size_t latency, size_t medium, size_t wide) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_plan_thresholds: null table");
  if (finest > small || small > latency || latency > medium || medium > wide)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_set_plan_thresholds: finest <= small <= latency <= medium <= wide");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_plan_thresholds(finest, small, latency, medium, wide);
  return MP_OK;
}
int mp_set_toom_cook(mp_table* t, int on) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_toom_cook: null table");
  MP_TRY
  MP_ENTER(t->ctx);
  t->set_toom_cook(on != 0);
  return MP_OK;
  MP_CATCH
}
int mp_set_sigma_screen(mp_table* t, uint32_t lanes_per_group, size_t min_lanes) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_sigma_screen: null table");
  MP_TRY
  MP_ENTER(t->ctx);
  if (t->set_sigma_screen(lanes_per_group, min_lanes) != MP_OK)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_set_sigma_screen: 0 (off), MP_SIGMA_SCREEN_AUTO or up to 98 304 lanes per group (one bucket job)");
  return MP_OK;
  MP_CATCH
}
int mp_sigma_screen_stats(const mp_table* t, uint64_t out[4]) {
  if (!t || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_sigma_screen_stats: null argument");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);      // (a verify call on another thread writes the counters)
  t->sigma_screen_stats(out);
  return MP_OK;
}
int mp_set_subgroup_check(mp_table* t, int on) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_subgroup_check: null table");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->set_subgroup_check(on != 0);
  return MP_OK;
}
int mp_reserve(mp_table* t, size_t B) {
  if (!t || !B) return fail(MP_ERR_BAD_ARGUMENT, "mp_reserve: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->reserve(B);
  rt::stream_sync(t->ctx->stream);
  return MP_OK;
  MP_CATCH
}

int mp_shuffle_and_remask_batch_dev(mp_table* t, size_t B, const void* d_decks, const void* d_masking_factors,
                                    const void* d_permutations, const void* d_prover_seeds, void* d_out_decks,
                                    void* d_out_proofs, void* d_status) {
  if (!t || !B || !d_decks || !d_masking_factors || !d_permutations || !d_prover_seeds || !d_out_decks || !d_out_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_dev: bad argument");
  if (t->keyless) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: use the _keys entry points");
  MP_TRY
  MP_ENTER(t->ctx);
  t->prove_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_masking_factors, (const uint32_t*)d_permutations,
               (const uint8_t*)d_prover_seeds, (uint8_t*)d_out_decks, (uint8_t*)d_out_proofs, (int32_t*)d_status);
  return MP_OK;
  MP_CATCH
}
int mp_verify_shuffle_batch_dev(mp_table* t, size_t B, const void* d_decks, const void* d_shuffled_decks,
                                const void* d_proofs, void* d_status) {
  if (!t || !B || !d_decks || !d_shuffled_decks || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_batch_dev: bad argument");
  if (t->keyless) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: use the _keys entry points");
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_shuffled_decks, (const uint8_t*)d_proofs, (int32_t*)d_status);
  return MP_OK;
  MP_CATCH
}
int mp_shuffle_and_remask_batch_keys_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks, const void* d_masking_factors,
                                         const void* d_permutations, const void* d_prover_seeds, void* d_out_decks,
                                         void* d_out_proofs, void* d_status) {
  if (!t || !B || !d_keys || !d_decks || !d_masking_factors || !d_permutations || !d_prover_seeds || !d_out_decks || !d_out_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_keys_dev: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->prove_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_masking_factors, (const uint32_t*)d_permutations,
               (const uint8_t*)d_prover_seeds, (uint8_t*)d_out_decks, (uint8_t*)d_out_proofs, (int32_t*)d_status, (const uint8_t*)d_keys);
  return MP_OK;
  MP_CATCH
}
int mp_verify_shuffle_batch_keys_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks, const void* d_shuffled_decks,
                                     const void* d_proofs, void* d_status) {
  if (!t || !B || !d_keys || !d_decks || !d_shuffled_decks || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_batch_keys_dev: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_shuffled_decks, (const uint8_t*)d_proofs, (int32_t*)d_status,
                (const uint8_t*)d_keys);
  return MP_OK;
  MP_CATCH
}
int mp_keyset_create(mp_table* t, size_t n_keys, const uint8_t* keys, mp_keyset** out) {
  if (!t || !n_keys || !keys || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_create: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  std::unique_ptr<mp_keyset> ks(new mp_keyset());
  ks->owner = t;
  const int rc = t->keyset_build(*ks, n_keys, keys);
  if (rc != MP_OK) return rc;
  *out = ks.release();
  return MP_OK;
  MP_CATCH
}
void mp_keyset_destroy(mp_keyset* ks) {
  if (!ks) return;
  try {
    MP_ENTER(ks->owner->ctx);
    if (ks->up_slots_up) {
      try {
        rt::event_sync(ks->up_slots_up);
      } catch (...) {
      }
      rt::event_destroy(ks->up_slots_up);
    }
    delete ks;
  } catch (...) {
  }
}
size_t mp_keyset_size(const mp_keyset* ks) { return ks ? ks->K : 0; }
int mp_keyset_create_empty(mp_table* t, size_t capacity, mp_keyset** out) {
  if (!t || !capacity || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_create_empty: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  std::unique_ptr<mp_keyset> ks(new mp_keyset());
  ks->owner = t;
  const int rc = t->keyset_build_empty(*ks, capacity);
  if (rc != MP_OK) return rc;
  *out = ks.release();
  return MP_OK;
  MP_CATCH
}
size_t mp_keyset_live(const mp_keyset* ks) {
  if (!ks) return 0;
  try {
    MP_ENTER(ks->owner->ctx);
    std::vector<uint32_t> live(ks->K);
    rt::Stream s = ks->owner->ctx->stream;
    rt::d2h(live.data(), ks->live.p, ks->K * 4, s);      // behind every update the stream holds
    rt::stream_sync(s);
    size_t n = 0;
    for (uint32_t v : live) n += v != 0u;
    return n;
  } catch (...) {
    return 0;
  }
}
// The slots array of an update (the rule of `first` in the ragged calls, ragged_take below): copied into the set's own vector, checked
// THERE -- count >= 1, every slot below the capacity, no slot twice -- and uploaded from there.  Nothing has been enqueued and the set
// is as it was when this fails.  Holds the context's lock.  -> the device array, or nullptr for a malformed one
static const uint32_t* keyset_take(mp_keyset* ks, size_t count, const uint32_t* slots) {
  if (count < 1 || count > ks->K) return nullptr;
  rt::Stream s = ks->owner->ctx->stream;
  if (ks->up_slots_up)
    rt::event_sync(ks->up_slots_up);
  else
    ks->up_slots_up = rt::event_create();
  std::vector<uint32_t>& h = ks->up_slots_host;
  h.assign(slots, slots + count);
  std::vector<uint32_t> sorted(h);
  std::sort(sorted.begin(), sorted.end());
  if (sorted.back() >= ks->K) return nullptr;
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return nullptr;
  ks->up_slots.alloc(count, s, false);
  rt::h2d(ks->up_slots.p, h.data(), count * 4, s);
  rt::event_record(ks->up_slots_up, s);
  return ks->up_slots.p;
}
static const char* const KEYSET_SLOTS = "1 <= count, every slot below the capacity of the set, no slot twice";
int mp_keyset_update_dev(mp_keyset* ks, size_t count, const uint32_t* slots, const void* d_keys, void* d_status) {
  if (!ks || !slots || !d_keys || !d_status) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_update_dev: null argument");
  MP_TRY
  mp_table* t = ks->owner;
  MP_ENTER(t->ctx);
  const uint32_t* d_slots = keyset_take(ks, count, slots);
  if (!d_slots) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_keyset_update_dev: ") + KEYSET_SLOTS);
  t->keyset_update(*ks, count, d_slots, (const uint8_t*)d_keys, (int32_t*)d_status);
  return MP_OK;
  MP_CATCH
}
int mp_keyset_update(mp_keyset* ks, size_t count, const uint32_t* slots, const uint8_t* keys, int32_t* status) {
  if (!ks || !slots || !keys || !status) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_update: null argument");
  MP_TRY
  mp_table* t = ks->owner;
  MP_ENTER(t->ctx);
  const uint32_t* d_slots = keyset_take(ks, count, slots);
  if (!d_slots) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_keyset_update: ") + KEYSET_SLOTS);
  rt::Stream s = t->ctx->stream;
  ks->up_keys.alloc(count * t->point_bytes, s, false);
  ks->up_status.alloc(count, s, false);
  rt::h2d(ks->up_keys.p, keys, count * t->point_bytes, s);
  t->keyset_update(*ks, count, d_slots, ks->up_keys.p, ks->up_status.p);
  rt::d2h(status, ks->up_status.p, count * 4, s);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}
int mp_keyset_clear(mp_keyset* ks, size_t count, const uint32_t* slots) {
  if (!ks || !slots) return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_clear: null argument");
  MP_TRY
  mp_table* t = ks->owner;
  MP_ENTER(t->ctx);
  const uint32_t* d_slots = keyset_take(ks, count, slots);
  if (!d_slots) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_keyset_clear: ") + KEYSET_SLOTS);
  t->keyset_update(*ks, count, d_slots, nullptr, nullptr);
  rt::stream_sync(t->ctx->stream);
  return MP_OK;
  MP_CATCH
}
int mp_shuffle_and_remask_batch_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                           const void* d_masking_factors, const void* d_permutations, const void* d_prover_seeds,
                                           void* d_out_decks, void* d_out_proofs, void* d_status) {
  if (!t || !ks || ks->owner != t || !B || !d_key_index || !d_decks || !d_masking_factors || !d_permutations || !d_prover_seeds || !d_out_decks ||
      !d_out_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_keyset_dev: bad argument (the key set must belong to this table)");
  MP_TRY
  MP_ENTER(t->ctx);
  t->prove_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_masking_factors, (const uint32_t*)d_permutations,
               (const uint8_t*)d_prover_seeds, (uint8_t*)d_out_decks, (uint8_t*)d_out_proofs, (int32_t*)d_status, nullptr, ks,
               (const uint32_t*)d_key_index);
  return MP_OK;
  MP_CATCH
}
int mp_verify_shuffle_batch_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                       const void* d_shuffled_decks, const void* d_proofs, void* d_status) {
  if (!t || !ks || ks->owner != t || !B || !d_key_index || !d_decks || !d_shuffled_decks || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_batch_keyset_dev: bad argument (the key set must belong to this table)");
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_dev(B, (const uint8_t*)d_decks, (const uint8_t*)d_shuffled_decks, (const uint8_t*)d_proofs, (int32_t*)d_status, nullptr, ks,
                (const uint32_t*)d_key_index);
  return MP_OK;
  MP_CATCH
}
int mp_verify_shuffle_chain_dev(mp_table* t, size_t tables, uint32_t links, const void* d_keys, const void* d_decks, const void* d_proofs,
                                void* d_status) {
  if (!t || !tables || !links || !d_decks || !d_proofs || !d_status || links > 4095)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_dev: bad argument");
  if (t->keyless && !d_keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: pass one key per link");
  if ((uint64_t)tables * links >= ((uint64_t)1 << 31)) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_dev: too many proofs for one call");
  MP_TRY
  MP_ENTER(t->ctx);
  NoPipeline nopipe(t);
  // chains longer than one equation takes: consecutive sub-chains (the decks array is link-major, so a sub-chain is a contiguous slice)
  const uint32_t lmax = chain_links_max(t);
  if (!lmax) return fail(MP_ERR_INTERNAL, "mp_verify_shuffle_chain_dev: deck too large for one chain equation");
  const size_t pb = t->point_bytes, deck_bytes = (size_t)2 * t->N * pb, psz = proof_size_bytes(t->m, t->n, (uint32_t)pb);
  auto sub_chains = [&](size_t T, const uint8_t* decks, const uint8_t* proofs, int32_t* status, const uint8_t* keys) {
    for (uint32_t j0 = 0; j0 < links; j0 += lmax) {
      const uint32_t lc = std::min(lmax, links - j0);
      t->verify_chain_dev(T, lc, decks + (size_t)j0 * T * deck_bytes, proofs + (size_t)j0 * T * psz, status + (size_t)j0 * T, keys ? keys + (size_t)j0 * T * pb : nullptr);
    }
  };
  // Tables per pass (round 5).  The chain workspace is ~68 KB per link in flight (52 cards): 49 152 tables x 32 links are 107 GB, and the
  // tables a caller holds are bounded by that long before its decks and proofs fill the HBM -- while the PROVER wants many tables per
  // launch (a link of every table is one batch).  So a call whose links do not fit the memory that is free (or the workspace that is
  // there already) is verified in passes of `slice` tables: their rows of the link-major arrays are gathered into the staging buffers
  // of the host-buffer calls (one copy per link and array: 13 KB per proof, ~10 ns at HBM rates), verified as a call of `slice` tables,
  // and their status words scattered back.  mp_set_chain_slice pins the number; verdicts do not depend on it.
  size_t slice = tables;
  const uint32_t lcmax = std::min(lmax, links);
  if (t->chain_slice) {
    slice = std::min(tables, t->chain_slice);
  } else if ((size_t)tables * lcmax > t->chain_lanes_held()) {
    size_t free_b = 0, total_b = 0;
    rt::mem_info(&free_b, &total_b);
    const size_t lane = t->chain_lane_bytes(lcmax, d_keys != nullptr);
    // (what is free now plus what the workspace gives back when it is re-allocated; 40 % of it: the bucket kernel's rows, the equation's
    // scalars and digits, the staging buffers below and the per-link fallback of a failing equation come on top, and smaller passes
    // cost nothing -- 65 536 tables in passes of 16 384 or 32 768: 677 k proofs/s either way, 195 GB against 241 GB in use)
    const size_t room = (size_t)(0.4 * (double)(free_b + t->chain_lanes_held() * lane));
    if (total_b && (size_t)tables * lcmax * lane > room) {
      slice = std::max<size_t>(1024, room / ((size_t)lcmax * lane) / 1024 * 1024);
      // (no sliver at the end: equal passes, whole multiples of 1 024 tables where that is possible)
      const size_t passes = (tables + slice - 1) / slice;
      slice = std::min(tables, ((tables + passes - 1) / passes + 1023) / 1024 * 1024);
    }
  }
  t->chain_last_slice = std::min(slice, tables);
  if (slice >= tables) {
    sub_chains(tables, (const uint8_t*)d_decks, (const uint8_t*)d_proofs, (int32_t*)d_status, (const uint8_t*)d_keys);
    return MP_OK;
  }
  rt::Stream s = t->ctx->stream;
  mp_io_stage& st = t->io[0];
  st.in0.alloc((size_t)(links + 1) * slice * deck_bytes, s, false);
  st.out1.alloc((size_t)links * slice * psz, s, false);
  st.status.alloc((size_t)links * slice, s, false);
  if (d_keys) st.keys.alloc((size_t)links * slice * pb, s, false);
  for (size_t t0 = 0; t0 < tables; t0 += slice) {
    const size_t ts = std::min(slice, tables - t0);
    for (uint32_t j = 0; j <= links; ++j)
      rt::d2d(st.in0.p + (size_t)j * ts * deck_bytes, (const uint8_t*)d_decks + ((size_t)j * tables + t0) * deck_bytes, ts * deck_bytes, s);
    for (uint32_t j = 0; j < links; ++j) {
      rt::d2d(st.out1.p + (size_t)j * ts * psz, (const uint8_t*)d_proofs + ((size_t)j * tables + t0) * psz, ts * psz, s);
      if (d_keys) rt::d2d(st.keys.p + (size_t)j * ts * pb, (const uint8_t*)d_keys + ((size_t)j * tables + t0) * pb, ts * pb, s);
    }
    sub_chains(ts, st.in0.p, st.out1.p, st.status.p, d_keys ? st.keys.p : nullptr);
    for (uint32_t j = 0; j < links; ++j) rt::d2d((int32_t*)d_status + (size_t)j * tables + t0, st.status.p + (size_t)j * ts, ts * 4, s);
  }
  return MP_OK;
  MP_CATCH
}
int mp_verify_shuffle_chain(mp_table* t, size_t tables, uint32_t links, const uint8_t* shared_keys, const uint8_t* decks, const uint8_t* proofs,
                            int32_t* status) {
  if (!t || !tables || !links || !decks || !proofs || !status) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  rt::Stream s = t->ctx->stream;
  const size_t B = tables * links, pb = t->point_bytes, deck_bytes = (size_t)2 * t->N * pb, psz = proof_size_bytes(t->m, t->n, (uint32_t)pb);
  DevBuf<uint8_t> dd, dp, dk;
  DevBuf<int32_t> ds;
  dd.alloc((B + tables) * deck_bytes, s, false);
  dp.alloc(B * psz, s, false);
  ds.alloc(B, s, false);
  rt::h2d(dd.p, decks, (B + tables) * deck_bytes, s);
  rt::h2d(dp.p, proofs, B * psz, s);
  if (shared_keys) {
    dk.alloc(B * pb, s, false);
    rt::h2d(dk.p, shared_keys, B * pb, s);
  }
  const int rc = mp_verify_shuffle_chain_dev(t, tables, links, shared_keys ? dk.p : nullptr, dd.p, dp.p, ds.p);
  if (rc != MP_OK) return rc;
  rt::d2h(status, ds.p, B * 4, s);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}
// ---- chains of different lengths: pieces and passes (include/mpshuffle.h; engine_base.hpp "Chains of different lengths")
// The plan of one call.  The caller's links are copied into cp_links and checked THERE, before anything is enqueued; everything below is
// derived from the copy.  Pieces: table by table, front to back -- one of links[t] links (WHOLE), or one per set bit of links[t] from the
// highest down (BINARY, where that gives fewer passes).  Passes: the distinct piece lengths, ascending; walking the tables in order leaves the pieces of a pass in
// (t, a) order.  cp_plan_host: [pieces][2] = deck row off(t) + t + a and proof row off(t) + a, the passes back to back; then
// [passes][3] = first word, first piece, pieces.  Holds the context's lock.  -> MP_OK, or MP_ERR_BAD_ARGUMENT with nothing touched
namespace {
struct ChainPass {
  uint32_t l;               // links of every piece of the pass
  size_t G, piece, word;    // its pieces; its first piece and first status word among those of the call
};
}  // namespace
static int chain_ragged_take(mp_table* t, size_t tables, const uint32_t* links, std::vector<ChainPass>& passes) {
  static const char* const SHAPE = "mp_verify_shuffle_chain_ragged: 1 <= links[t] <= 4 095 for every table, less than 2^31 links in all";
  if (tables >= ((size_t)1 << 31)) return fail(MP_ERR_BAD_ARGUMENT, SHAPE);
  std::vector<uint32_t>& lk = t->cp_links;
  lk.assign(links, links + tables);
  uint64_t total = 0;
  for (size_t k = 0; k < tables; ++k) {
    if (lk[k] < 1 || lk[k] > 4095) return fail(MP_ERR_BAD_ARGUMENT, SHAPE);
    total += lk[k];
  }
  if (total >= ((uint64_t)1 << 31)) return fail(MP_ERR_BAD_ARGUMENT, SHAPE);
  // BINARY is there for fewer passes -- one per bit set in some links[t] against one per distinct length --, and a pass costs milliseconds
  // whatever it holds (DESIGN.md "Ragged calls"): where whole chains need no more passes, as in every call whose chains have one length,
  // they stay whole and no boundary deck is verified twice.  mp_chain_ragged_stats reports the cut that was made
  std::vector<size_t> next(4096, 0);      // pieces of length l; then the slot of the next piece of that length
  uint32_t bits_set = 0, lengths = 0;
  for (size_t k = 0; k < tables; ++k) {
    bits_set |= lk[k];
    if (!next[lk[k]]) next[lk[k]] = ++lengths;
  }
  std::fill(next.begin(), next.end(), 0);
  const bool binary = t->chain_pieces == MP_CHAIN_PIECES_BINARY && (uint32_t)__builtin_popcount(bits_set) < lengths;
  for (size_t k = 0; k < tables; ++k) {
    if (!binary) ++next[lk[k]];
    for (uint32_t b = 2048; binary && b; b >>= 1)
      if (lk[k] & b) ++next[b];
  }
  passes.clear();
  size_t pieces = 0, words = 0, widest = 0;
  for (uint32_t l = 1; l < 4096; ++l)
    if (next[l]) {
      const size_t G = next[l];
      passes.push_back(ChainPass{l, G, pieces, words});
      next[l] = pieces;
      pieces += G;
      words += (size_t)l * G;
      widest = std::max(widest, G);
    }
  if (t->cp_plan_up)
    rt::event_sync(t->cp_plan_up);      // (the upload of the previous call's descriptors has read the vector)
  else
    t->cp_plan_up = rt::event_create();
  std::vector<uint64_t>& h = t->cp_plan_host;
  h.assign(2 * pieces + 3 * passes.size(), 0);
  uint64_t off = 0;
  auto put = [&](size_t k, uint32_t a, uint32_t l) {
    const size_t i = next[l]++;
    h[2 * i] = off + k + a;
    h[2 * i + 1] = off + a;
  };
  for (size_t k = 0; k < tables; ++k) {
    if (!binary) put(k, 0, lk[k]);
    uint32_t a = 0;
    for (uint32_t b = 2048; binary && b; b >>= 1)
      if (lk[k] & b) {
        put(k, a, b);
        a += b;
      }
    off += lk[k];
  }
  for (size_t p = 0; p < passes.size(); ++p) {
    h[2 * pieces + 3 * p] = passes[p].word;
    h[2 * pieces + 3 * p + 1] = passes[p].piece;
    h[2 * pieces + 3 * p + 2] = passes[p].G;
  }
  const uint64_t st[8] = {passes.size(), pieces, tables, total, 0, 0, widest, (uint64_t)(binary ? MP_CHAIN_PIECES_BINARY : MP_CHAIN_PIECES_WHOLE)};
  memcpy(t->cp_stats, st, sizeof st);
  return MP_OK;
}
// the passes of a planned call over device arrays: one gather launch and one mp_verify_shuffle_chain_dev per pass on the context's
// stream, the words of every pass kept in cp_words, and ONE scatter launch behind the last pass
static int chain_ragged_passes(mp_table* t, const std::vector<ChainPass>& passes, const uint8_t* d_keys, const uint8_t* d_decks,
                               const uint8_t* d_proofs, int32_t* d_status) {
  rt::Stream s = t->ctx->stream;
  const size_t pb = t->point_bytes, deck_bytes = (size_t)2 * t->N * pb, psz = proof_size_bytes(t->m, t->n, (uint32_t)pb);
  const size_t pieces = (size_t)t->cp_stats[1], total = (size_t)t->cp_stats[3];
  t->cp_plan.upload(t->cp_plan_host, s);
  rt::event_record(t->cp_plan_up, s);
  size_t max_d = 0, max_p = 0;
  for (const ChainPass& p : passes) {
    max_d = std::max(max_d, (size_t)(p.l + 1) * p.G);
    max_p = std::max(max_p, (size_t)p.l * p.G);
  }
  t->cp_decks.alloc(max_d * deck_bytes, s, false);
  t->cp_proofs.alloc(max_p * psz, s, false);
  if (d_keys) t->cp_keys.alloc(max_p * pb, s, false);
  t->cp_words.alloc(total, s, false);
  for (const ChainPass& p : passes) {
    t->cp_stats[4] += t->chain_piece_gather(t->cp_plan.p + 2 * p.piece, p.G, p.l, d_decks, d_proofs, d_keys, t->cp_decks.p, t->cp_proofs.p,
                                            d_keys ? t->cp_keys.p : nullptr);
    const int rc = mp_verify_shuffle_chain_dev(t, p.G, p.l, d_keys ? t->cp_keys.p : nullptr, t->cp_decks.p, t->cp_proofs.p, t->cp_words.p + p.word);
    if (rc != MP_OK) return rc;
  }
  t->chain_piece_scatter(t->cp_plan.p, t->cp_plan.p + 2 * pieces, (uint32_t)passes.size(), t->cp_words.p, total, d_status);
  return MP_OK;
}
int mp_verify_shuffle_chain_ragged_dev(mp_table* t, size_t tables, const uint32_t* links, const void* d_keys, const void* d_decks,
                                       const void* d_proofs, void* d_status) {
  if (!t || !tables || !links || !d_decks || !d_proofs || !d_status) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged_dev: bad argument");
  if (((uintptr_t)d_keys | (uintptr_t)d_decks | (uintptr_t)d_proofs) & 15u)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged_dev: the device arrays must be 16-byte aligned");
  if (t->keyless && !d_keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: pass one key per link");
  MP_TRY
  MP_ENTER(t->ctx);
  std::vector<ChainPass> passes;
  if (int bad = chain_ragged_take(t, tables, links, passes)) return bad;
  NoPipeline nopipe(t);
  return chain_ragged_passes(t, passes, (const uint8_t*)d_keys, (const uint8_t*)d_decks, (const uint8_t*)d_proofs, (int32_t*)d_status);
  MP_CATCH
}
// host buffers: the caller's arrays go up as they are, the passes run as above, the words come down
int mp_verify_shuffle_chain_ragged(mp_table* t, size_t tables, const uint32_t* links, const uint8_t* shared_keys, const uint8_t* decks,
                                   const uint8_t* proofs, int32_t* status) {
  if (!t || !tables || !links || !decks || !proofs || !status) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged: bad argument");
  if (t->keyless && !shared_keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: pass one key per link");
  MP_TRY
  MP_ENTER(t->ctx);
  std::vector<ChainPass> passes;
  if (int bad = chain_ragged_take(t, tables, links, passes)) return bad;
  NoPipeline nopipe(t);
  rt::Stream s = t->ctx->stream;
  const size_t pb = t->point_bytes, deck_bytes = (size_t)2 * t->N * pb, psz = proof_size_bytes(t->m, t->n, (uint32_t)pb);
  const size_t total = (size_t)t->cp_stats[3];
  t->cp_in_decks.alloc((total + tables) * deck_bytes, s, false);
  t->cp_in_proofs.alloc(total * psz, s, false);
  t->cp_in_status.alloc(total, s, false);
  rt::h2d(t->cp_in_decks.p, decks, (total + tables) * deck_bytes, s);
  rt::h2d(t->cp_in_proofs.p, proofs, total * psz, s);
  if (shared_keys) {
    t->cp_in_keys.alloc(total * pb, s, false);
    rt::h2d(t->cp_in_keys.p, shared_keys, total * pb, s);
  }
  const int rc = chain_ragged_passes(t, passes, shared_keys ? t->cp_in_keys.p : nullptr, t->cp_in_decks.p, t->cp_in_proofs.p, t->cp_in_status.p);
  if (rc != MP_OK) return rc;
  rt::d2h(status, t->cp_in_status.p, total * 4, s);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}
// ---- chains by index: one slot of a key set per TABLE; the per-link keys the passes want are written on the device
// the link offsets of the tables, from the validated copy of the links (chain_ragged_take) -> the device array [tables + 1]
static const uint32_t* chain_keyset_offsets(mp_table* t, size_t tables) {
  rt::Stream s = t->ctx->stream;
  if (t->ck_off_up)
    rt::event_sync(t->ck_off_up);
  else
    t->ck_off_up = rt::event_create();
  std::vector<uint32_t>& h = t->ck_off_host;
  h.assign(tables + 1, 0);
  for (size_t k = 0; k < tables; ++k) h[k + 1] = h[k] + t->cp_links[k];      // (less than 2^31 in all)
  t->ck_off.alloc(tables + 1, s, false);
  rt::h2d(t->ck_off.p, h.data(), (tables + 1) * 4, s);
  rt::event_record(t->ck_off_up, s);
  return t->ck_off.p;
}
static int chain_keyset_passes(mp_table* t, const mp_keyset* ks, size_t tables, const std::vector<ChainPass>& passes, const uint32_t* d_kidx,
                               const uint8_t* d_decks, const uint8_t* d_proofs, int32_t* d_status) {
  const size_t total = (size_t)t->cp_stats[3];
  const uint32_t* d_off = chain_keyset_offsets(t, tables);
  t->ck_keys.alloc(total * t->point_bytes, t->ctx->stream, false);
  t->keyset_chain_keys(*ks, tables, d_kidx, d_off, t->ck_keys.p);
  const int rc = chain_ragged_passes(t, passes, t->ck_keys.p, d_decks, d_proofs, d_status);
  if (rc != MP_OK) return rc;
  t->keyset_chain_status(*ks, tables, d_kidx, d_off, d_status);
  return MP_OK;
}
int mp_verify_shuffle_chain_ragged_keyset_dev(mp_table* t, const mp_keyset* ks, size_t tables, const uint32_t* links, const void* d_key_index,
                                              const void* d_decks, const void* d_proofs, void* d_status) {
  if (!t || !ks || ks->owner != t || !tables || !links || !d_key_index || !d_decks || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged_keyset_dev: bad argument (the key set must belong to this table)");
  if (((uintptr_t)d_decks | (uintptr_t)d_proofs) & 15u)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged_keyset_dev: the device arrays must be 16-byte aligned");
  MP_TRY
  MP_ENTER(t->ctx);
  std::vector<ChainPass> passes;
  if (int bad = chain_ragged_take(t, tables, links, passes)) return bad;
  NoPipeline nopipe(t);
  return chain_keyset_passes(t, ks, tables, passes, (const uint32_t*)d_key_index, (const uint8_t*)d_decks, (const uint8_t*)d_proofs,
                             (int32_t*)d_status);
  MP_CATCH
}
int mp_verify_shuffle_chain_ragged_keyset(mp_table* t, const mp_keyset* ks, size_t tables, const uint32_t* links, const uint32_t* key_index,
                                          const uint8_t* decks, const uint8_t* proofs, int32_t* status) {
  if (!t || !ks || ks->owner != t || !tables || !links || !key_index || !decks || !proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_chain_ragged_keyset: bad argument (the key set must belong to this table)");
  MP_TRY
  MP_ENTER(t->ctx);
  std::vector<ChainPass> passes;
  if (int bad = chain_ragged_take(t, tables, links, passes)) return bad;
  NoPipeline nopipe(t);
  rt::Stream s = t->ctx->stream;
  const size_t pb = t->point_bytes, deck_bytes = (size_t)2 * t->N * pb, psz = proof_size_bytes(t->m, t->n, (uint32_t)pb);
  const size_t total = (size_t)t->cp_stats[3];
  t->cp_in_decks.alloc((total + tables) * deck_bytes, s, false);
  t->cp_in_proofs.alloc(total * psz, s, false);
  t->cp_in_status.alloc(total, s, false);
  t->ck_idx.alloc(tables, s, false);
  rt::h2d(t->cp_in_decks.p, decks, (total + tables) * deck_bytes, s);
  rt::h2d(t->cp_in_proofs.p, proofs, total * psz, s);
  rt::h2d(t->ck_idx.p, key_index, tables * 4, s);
  const int rc = chain_keyset_passes(t, ks, tables, passes, t->ck_idx.p, t->cp_in_decks.p, t->cp_in_proofs.p, t->cp_in_status.p);
  if (rc != MP_OK) return rc;
  rt::d2h(status, t->cp_in_status.p, total * 4, s);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}
int mp_set_chain_pieces(mp_table* t, int mode) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_pieces: null table");
  if (mode != MP_CHAIN_PIECES_WHOLE && mode != MP_CHAIN_PIECES_BINARY)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_set_chain_pieces: MP_CHAIN_PIECES_WHOLE or MP_CHAIN_PIECES_BINARY");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->chain_pieces = mode;
  return MP_OK;
}
int mp_chain_ragged_stats(const mp_table* t, uint64_t out[8]) {
  if (!t || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_chain_ragged_stats: null argument");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  memcpy(out, t->cp_stats, sizeof t->cp_stats);
  return MP_OK;
}
int mp_sync(mp_ctx* ctx) {
  if (!ctx) return fail(MP_ERR_BAD_ARGUMENT, "mp_sync: null");
  MP_TRY
  MP_ENTER(ctx);
  rt::stream_sync(ctx->stream);
  for (mp_table* t : ctx->tables) t->flush();      // pipelined verify calls: deferred per-equation passes, then the verify lane
  return MP_OK;
  MP_CATCH
}

// ---- host-buffer entry points: the batch is cut into chunks and pipelined -- while the kernels of chunk k run on the
// context's stream, chunk k+1 is uploaded on a second stream and the results of chunk k-1 are downloaded on a third
// (PCIe is full duplex).  Staging buffers are persistent (two chunks in flight).  With page-locked caller buffers
// (mp_host_alloc) every copy is an asynchronous DMA; with pageable buffers the runtime stages them and the overlap is partial.
static const size_t IO_CHUNK = 65536;   // default proofs per chunk: the kernels need ~64 k lanes to run at full rate ...
static const size_t IO_CHUNK_LARGE = 131072;   // ... and calls of 262 144 proofs or more take chunks of twice that (round 5: the copies are
// hidden either way; what the chunked call loses against one batch is kernel efficiency -- 474 ms of kernels against 385 with 65 536-proof
// chunks, profiles/r04_pcie_inclusive.txt -- the screen of a 131 072-proof chunk runs on groups of 128 proofs, that of 65 536 on groups of 64)
static size_t io_chunk_of(const mp_table* t, size_t B) { return std::min(B, t->io_chunk ? t->io_chunk : (B >= 2 * IO_CHUNK_LARGE ? IO_CHUNK_LARGE : IO_CHUNK)); }
// The chunks of one call: full chunks in the middle, a ramp of C/8 and 3C/8 at either end -- the first upload and the last download
// are the only transfers nothing overlaps, so the first and the last chunk are small (262 144 proofs: 22 + 34 ms of exposed copies per
// prove call with four equal chunks, 3 + 4 ms with the ramp, for ~15 ms of less efficient small-batch kernels).  Calls of less
// than three chunks are cut evenly as before.  tail_ramp = false (verification: all that comes back is a status word per proof): see below
static std::vector<size_t> io_schedule(size_t B, size_t C, bool tail_ramp = true) {
  std::vector<size_t> v;
  if (B < 2 * C || C < 8) {
    for (size_t o = 0; o < B; o += C) v.push_back(std::min(C, B - o));
    return v;
  }
#ifndef MP_EXP_IO_RAMP      // (A/B hook of round 5, compile-time: profiles/r05g_ab_verify_upload_ramp.txt; no environment variable steers the library)
#define MP_EXP_IO_RAMP 1
#endif
  constexpr bool slow_ramp = MP_EXP_IO_RAMP != 0;
  if (!tail_ramp && !slow_ramp) {      // round 4's schedule without its tail: C/8, 3C/8, then full chunks
    v.push_back(C / 8);
    v.push_back(3 * C / 8);
    for (size_t left = B - C / 2; left;) {
      const size_t c = std::min(C, left);
      v.push_back(c);
      left -= c;
    }
    return v;
  }
  if (!tail_ramp) {
    // Verification uploads 19.7 KB per proof (both decks and the proof) for ~0.5 us of kernels: at PCIe rates the copy of chunk k + 1
    // takes about as long as the kernels of chunk k, so the chunks can only grow slowly -- by half from one to the next, starting at C / 8;
    // whatever is left when the next step would overshoot is the last chunk (nothing of a verify call is exposed at its end)
    size_t left = B;
    for (size_t c = C / 8; left; c = std::min(C, (c + c / 2 + 1023) / 1024 * 1024)) {
      // (no sliver at the end: what is left below 1.5 c goes as one chunk, or as two halves if that would exceed C)
      const size_t take = left >= c + c / 2 ? c : (left <= C ? left : (left + 1) / 2);
      v.push_back(take);
      left -= take;
    }
    return v;
  }
  const size_t r0 = C / 8, r1 = 3 * C / 8;
  v.push_back(r0);
  v.push_back(r1);
  for (size_t left = B - 2 * (r0 + r1); left;) {
    const size_t c = std::min(C, left);
    v.push_back(c);
    left -= c;
  }
  v.push_back(r1);
  v.push_back(r0);
  return v;
}
// the chunk size and the chunks of one host-buffer call: what prove_batch_host / verify_batch_host cut their batch with and what
// mp_io_schedule reports
static std::vector<size_t> io_chunks(const mp_table* t, size_t B, bool verify, size_t* chunk = nullptr) {
  const size_t C = io_chunk_of(t, B);
  if (chunk) *chunk = C;
  return io_schedule(B, C, !verify);
}
static void io_events(mp_io_stage& st) {
  if (!st.up) {
    st.up = rt::event_create();
    st.done = rt::event_create();
    st.down = rt::event_create();
  }
}

// the call-level argument checks of the host-buffer batch calls: 0, or the code the call returns (the pool's calls decide by the same
// checks before anything is dispatched)
static int prove_batch_args(const mp_table* t, size_t B, const uint8_t* keys, const uint8_t* decks, const uint8_t* masking_factors,
                            const uint32_t* permutations, const uint8_t* prover_seeds, const uint8_t* out_decks, const uint8_t* out_proofs,
                            const int32_t* status, bool seeded = false) {
  if (!t || !B || !decks || (!seeded && (!masking_factors || !permutations)) || !prover_seeds || !out_decks || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch: bad argument");
  if (t->keyless && !keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: use the _keys entry points");
  return 0;
}
static int verify_batch_args(const mp_table* t, size_t B, const uint8_t* keys, const uint8_t* decks, const uint8_t* shuffled_decks,
                             const uint8_t* proofs, const int32_t* status) {
  if (!t || !B || !decks || !shuffled_decks || !proofs || !status) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_batch: bad argument");
  if (t->keyless && !keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: use the _keys entry points");
  return 0;
}
// seeded (mp_shuffle_and_remask_batch_seeded): no witness comes from the host -- every chunk's masking factors and permutations are sampled
// from its prover seeds into the staging buffers the unseeded call uploads them to, and go back to the host only if asked for
static int prove_batch_host(mp_table* t, size_t B, const uint8_t* keys, const uint8_t* decks, const uint8_t* masking_factors,
                            const uint32_t* permutations, const uint8_t* prover_seeds, uint8_t* out_decks,
                            uint8_t* out_proofs, int32_t* status, bool seeded = false, uint32_t* out_perms = nullptr,
                            uint8_t* out_factors = nullptr) {
  if (int bad = prove_batch_args(t, B, keys, decks, masking_factors, permutations, prover_seeds, out_decks, out_proofs, status, seeded)) return bad;
  MP_TRY
  MP_ENTER(t->ctx);
  rt::Stream s = t->ctx->stream, up = t->ctx->h2d, down = t->ctx->d2h;
  const size_t N = t->N, psz = proof_size_bytes(t->m, t->n, t->point_bytes), dsz = N * 2 * t->point_bytes;
  size_t chunk = 0;
  const std::vector<size_t> sched = io_chunks(t, B, false, &chunk);
  std::vector<size_t> first(sched.size() + 1, 0);
  for (size_t k = 0; k < sched.size(); ++k) first[k + 1] = first[k] + sched[k];
  const size_t nchunks = sched.size();
  for (auto& st : t->io) {
    io_events(st);
    st.used = false;
    st.in0.alloc(chunk * dsz, s, false); st.in1.alloc(chunk * N * 32, s, false); st.perm.alloc(chunk * N, s, false);
    st.in2.alloc(chunk * 32, s, false); st.out0.alloc(chunk * dsz, s, false); st.out1.alloc(chunk * psz, s, false);
    st.status.alloc(chunk, s, false);
    if (keys) st.keys.alloc(chunk * t->point_bytes, s, false);
  }
  auto upload = [&](size_t k) {
    mp_io_stage& st = t->io[k & 1];
    const size_t o = first[k], c = sched[k];
    if (st.used) rt::stream_wait(up, st.done);          // the kernels of chunk k-2 have consumed these buffers
    rt::h2d(st.in0.p, decks + o * dsz, c * dsz, up);
    if (!seeded) {
      rt::h2d(st.in1.p, masking_factors + o * N * 32, c * N * 32, up);
      rt::h2d(st.perm.p, permutations + o * N, c * N * 4, up);
    }
    rt::h2d(st.in2.p, prover_seeds + o * 32, c * 32, up);
    if (keys) rt::h2d(st.keys.p, keys + o * t->point_bytes, c * t->point_bytes, up);
    rt::event_record(st.up, up);
  };
  upload(0);
  for (size_t k = 0; k < nchunks; ++k) {
    mp_io_stage& st = t->io[k & 1];
    const size_t o = first[k], c = sched[k];
    rt::stream_wait(s, st.up);
    if (st.used) rt::stream_wait(s, st.down);            // results of chunk k-2 have left the output buffers
    if (seeded) t->sample_dev(c, st.in2.p, (uint32_t)N, (uint32_t)N, st.in1.p, st.perm.p);
    t->prove_dev(c, st.in0.p, st.in1.p, st.perm.p, st.in2.p, st.out0.p, st.out1.p, st.status.p, keys ? st.keys.p : nullptr);
    rt::event_record(st.done, s);
    if (k + 1 < nchunks) upload(k + 1);
    rt::stream_wait(down, st.done);
    rt::d2h(out_decks + o * dsz, st.out0.p, c * dsz, down);
    rt::d2h(out_proofs + o * psz, st.out1.p, c * psz, down);
    rt::d2h(status + o, st.status.p, c * 4, down);
    if (out_perms) rt::d2h(out_perms + o * N, st.perm.p, c * N * 4, down);
    if (out_factors) rt::d2h(out_factors + o * N * 32, st.in1.p, c * N * 32, down);
    rt::event_record(st.down, down);
    st.used = true;
  }
  rt::stream_sync(down);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}
static int verify_batch_host(mp_table* t, size_t B, const uint8_t* keys, const uint8_t* decks, const uint8_t* shuffled_decks,
                             const uint8_t* proofs, int32_t* status) {
  if (int bad = verify_batch_args(t, B, keys, decks, shuffled_decks, proofs, status)) return bad;
  MP_TRY
  MP_ENTER(t->ctx);
  NoPipeline nopipe(t);
  rt::Stream s = t->ctx->stream, up = t->ctx->h2d, down = t->ctx->d2h;
  const size_t N = t->N, psz = proof_size_bytes(t->m, t->n, t->point_bytes), dsz = N * 2 * t->point_bytes;
  size_t chunk = 0;
  const std::vector<size_t> sched = io_chunks(t, B, true, &chunk);
  std::vector<size_t> first(sched.size() + 1, 0);
  for (size_t k = 0; k < sched.size(); ++k) first[k + 1] = first[k] + sched[k];
  const size_t nchunks = sched.size();
  for (auto& st : t->io) {
    io_events(st);
    st.used = false;
    st.in0.alloc(chunk * dsz, s, false); st.in3.alloc(chunk * dsz, s, false); st.out1.alloc(chunk * psz, s, false);
    st.status.alloc(chunk, s, false);
    if (keys) st.keys.alloc(chunk * t->point_bytes, s, false);
  }
  auto upload = [&](size_t k) {
    mp_io_stage& st = t->io[k & 1];
    const size_t o = first[k], c = sched[k];
    if (st.used) rt::stream_wait(up, st.done);
    rt::h2d(st.in0.p, decks + o * dsz, c * dsz, up);
    rt::h2d(st.in3.p, shuffled_decks + o * dsz, c * dsz, up);
    rt::h2d(st.out1.p, proofs + o * psz, c * psz, up);
    if (keys) rt::h2d(st.keys.p, keys + o * t->point_bytes, c * t->point_bytes, up);
    rt::event_record(st.up, up);
  };
  upload(0);
  for (size_t k = 0; k < nchunks; ++k) {
    mp_io_stage& st = t->io[k & 1];
    const size_t o = first[k], c = sched[k];
    if (k + 1 < nchunks) upload(k + 1);                  // before verify_dev: it ends with a read-back of the screening flag
    rt::stream_wait(s, st.up);
    if (st.used) rt::stream_wait(s, st.down);
    t->verify_dev(c, st.in0.p, st.in3.p, st.out1.p, st.status.p, keys ? st.keys.p : nullptr);
    rt::event_record(st.done, s);
    rt::stream_wait(down, st.done);
    rt::d2h(status + o, st.status.p, c * 4, down);
    rt::event_record(st.down, down);
    st.used = true;
  }
  rt::stream_sync(down);
  rt::stream_sync(s);
  return MP_OK;
  MP_CATCH
}

size_t mp_io_schedule(const mp_table* t, size_t B, int verify, size_t* out_chunks, size_t cap) {
  if (!t || !B) return 0;
  try {
    std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);      // (mp_set_io_chunk on another thread writes io_chunk)
    const std::vector<size_t> sched = io_chunks(t, B, verify != 0);
    for (size_t k = 0; k < sched.size() && k < cap && out_chunks; ++k) out_chunks[k] = sched[k];
    return sched.size();
  } catch (const std::exception& e) {
    fail(MP_ERR_INTERNAL, e.what());
    return 0;
  }
}
int mp_shuffle_and_remask_batch(mp_table* t, size_t B, const uint8_t* decks, const uint8_t* masking_factors,
                                const uint32_t* permutations, const uint8_t* prover_seeds, uint8_t* out_decks,
                                uint8_t* out_proofs, int32_t* status) {
  return prove_batch_host(t, B, nullptr, decks, masking_factors, permutations, prover_seeds, out_decks, out_proofs, status);
}
int mp_verify_shuffle_batch(mp_table* t, size_t B, const uint8_t* decks, const uint8_t* shuffled_decks,
                            const uint8_t* proofs, int32_t* status) {
  return verify_batch_host(t, B, nullptr, decks, shuffled_decks, proofs, status);
}
int mp_shuffle_and_remask_batch_keys(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                     const uint8_t* masking_factors, const uint32_t* permutations, const uint8_t* prover_seeds,
                                     uint8_t* out_decks, uint8_t* out_proofs, int32_t* status) {
  if (!shared_keys) return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_keys: null keys");
  return prove_batch_host(t, B, shared_keys, decks, masking_factors, permutations, prover_seeds, out_decks, out_proofs, status);
}
int mp_verify_shuffle_batch_keys(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                 const uint8_t* shuffled_decks, const uint8_t* proofs, int32_t* status) {
  if (!shared_keys) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_batch_keys: null keys");
  return verify_batch_host(t, B, shared_keys, decks, shuffled_decks, proofs, status);
}
// ---- single-proof entry points: one proof per call, as the reference's trait [REF src/lib.rs:181-197].  With coalescing on
// (mp_set_coalesce) the concurrent calls of a table are gathered into batched calls (coalesce.hpp); off, a call is a batch of one.
static int single_prove(mp_table* t, const uint8_t* key, const uint8_t* deck, const uint8_t* masking_factors, const uint32_t* permutation,
                        const uint8_t* prover_seed, uint8_t* out_deck, uint8_t* out_proof) {
  int32_t st = 0;
  int rc = 1;
  // (arguments that fail the batched call's checks go the uncoalesced way: same checks, same codes)
  if (t && co_on(t) && deck && masking_factors && permutation && prover_seed && out_deck && out_proof && (key || !t->keyless)) {
    MP_TRY
    CoRequest r;
    r.key = key;
    r.deck = deck;
    r.rho = masking_factors;
    r.perm = permutation;
    r.seed = prover_seed;
    r.out_deck = out_deck;
    r.out_proof = out_proof;
    const CoGeom g = co_geom(t, key ? CO_PROVE_KEYED : CO_PROVE);
    rc = co_submit(t, key ? CO_PROVE_KEYED : CO_PROVE, r, [&](CoSet& s, size_t f, size_t c) {
      return prove_batch_host(t, c, key ? s.keys + f * g.pb : nullptr, s.decks + f * g.dsz, s.rho + f * g.N * 32, s.perm + f * g.N,
                              s.seeds + f * 32, s.out_decks + f * g.dsz, s.out_proofs + f * g.psz, s.status + f);
    }, &st);
    MP_CATCH
  }
  if (rc == 1) rc = prove_batch_host(t, 1, key, deck, masking_factors, permutation, prover_seed, out_deck, out_proof, &st);
  if (rc != MP_OK) return rc;
  if (st < 0) return fail(st, mp_check_name(st));
  return st;
}
static int single_verify(mp_table* t, const uint8_t* key, const uint8_t* deck, const uint8_t* shuffled_deck, const uint8_t* proof,
                         size_t proof_len) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle: null table");
  if (proof_len != proof_size_bytes(t->m, t->n, t->point_bytes)) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle: wrong proof length");
  int32_t st = 0;
  int rc = 1;
  if (co_on(t) && deck && shuffled_deck && proof && (key || !t->keyless)) {
    MP_TRY
    CoRequest r;
    r.key = key;
    r.deck = deck;
    r.shuf = shuffled_deck;
    r.proof = proof;
    const CoGeom g = co_geom(t, key ? CO_VERIFY_KEYED : CO_VERIFY);
    rc = co_submit(t, key ? CO_VERIFY_KEYED : CO_VERIFY, r, [&](CoSet& s, size_t f, size_t c) {
      return verify_batch_host(t, c, key ? s.keys + f * g.pb : nullptr, s.decks + f * g.dsz, s.shuf + f * g.dsz, s.proofs + f * g.psz,
                               s.status + f);
    }, &st);
    MP_CATCH
  }
  if (rc == 1) rc = verify_batch_host(t, 1, key, deck, shuffled_deck, proof, &st);
  if (rc != MP_OK) return rc;
  if (st < 0) return fail(st, mp_check_name(st));
  return st;
}
int mp_shuffle_and_remask(mp_table* t, const uint8_t* deck, const uint8_t* masking_factors, const uint32_t* permutation,
                          const uint8_t prover_seed[32], uint8_t* out_deck, uint8_t* out_proof) {
  return single_prove(t, nullptr, deck, masking_factors, permutation, prover_seed, out_deck, out_proof);
}
int mp_verify_shuffle(mp_table* t, const uint8_t* deck, const uint8_t* shuffled_deck, const uint8_t* proof, size_t proof_len) {
  return single_verify(t, nullptr, deck, shuffled_deck, proof, proof_len);
}
int mp_shuffle_and_remask_keyed(mp_table* t, const uint8_t* shared_key, const uint8_t* deck, const uint8_t* masking_factors,
                                const uint32_t* permutation, const uint8_t prover_seed[32], uint8_t* out_deck, uint8_t* out_proof) {
  if (!shared_key) return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_keyed: null key");
  return single_prove(t, shared_key, deck, masking_factors, permutation, prover_seed, out_deck, out_proof);
}
int mp_verify_shuffle_keyed(mp_table* t, const uint8_t* shared_key, const uint8_t* deck, const uint8_t* shuffled_deck, const uint8_t* proof,
                            size_t proof_len) {
  if (!shared_key) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_shuffle_keyed: null key");
  return single_verify(t, shared_key, deck, shuffled_deck, proof, proof_len);
}
int mp_set_coalesce(mp_table* t, size_t max_batch, uint32_t max_wait_us) {
  if (!t) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_coalesce: null table");
  if (max_batch > 65536) return fail(MP_ERR_BAD_ARGUMENT, "mp_set_coalesce: max_batch 0 (off) .. 65 536");
  // (the queues' own mutexes only: the setting applies to the batches opened after this call, a batch in flight completes as it is)
  t->co->max_wait_us.store(max_wait_us);
  t->co->max_batch.store(max_batch);
  for (CoQueue& q : t->co->q) {
    std::lock_guard<std::mutex> lk(q.mu);
    q.reset();
  }
  return MP_OK;
}
int mp_coalesce_stats(const mp_table* t, uint64_t out[8]) {
  if (!t || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_coalesce_stats: bad argument");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);      // (context, then queue: the order of coalesce.hpp)
  uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (CoQueue& q : t->co->q) {
    std::lock_guard<std::mutex> lk(q.mu);
    v[0] += q.served;
    v[1] += q.calls;
    v[2] = std::max(v[2], q.largest);
    v[3] += q.closed_full;
    v[4] += q.closed_time;
    v[5] += q.rerun;
    v[6] += q.wait_us;
  }
  memcpy(out, v, sizeof(v));
  return MP_OK;
}

// ---- the device pool (pool.hpp): contexts on one or several devices behind one handle; batches are cut into contiguous blocks
int mp_pool_create(int curve_id, size_t n_members, const int* devices, mp_pool** out) {
  if (!out) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_create: null out pointer");
  if (curve_id < 0 || curve_id > 3) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_create: unknown curve id");
  if (n_members == 0 || n_members > 64) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_create: 1 .. 64 members");
  MP_TRY
  std::unique_ptr<mp_pool> p(new mp_pool());      // (its destructor gives back whatever was created when a later member fails)
  p->curve = curve_id;
  p->members.resize(n_members);
  for (size_t i = 0; i < n_members; ++i) {
    mp_pool::Member& mb = p->members[i];
    mb.device = devices ? devices[i] : (int)i;
    const int rc = mp_ctx_create(curve_id, mb.device, &mb.ctx);
    if (rc != MP_OK) return fail(rc, "mp_pool_create: " + pool_member_text(p.get(), i, last_error()));
    mb.worker.reset(new PoolWorker());
  }
  *out = p.release();
  return MP_OK;
  MP_CATCH
}
void mp_pool_destroy(mp_pool* p) { delete p; }
size_t mp_pool_size(const mp_pool* p) { return p ? p->members.size() : 0; }
mp_ctx* mp_pool_member_ctx(mp_pool* p, size_t i) { return p && i < p->members.size() ? p->members[i].ctx : nullptr; }

static void pool_table_release(mp_pool_table* pt) {
  // the members that borrow fixed-base tables first, their owners last
  for (size_t i = 0; i < pt->tables.size(); ++i)
    if (pt->owner[i] != (int)i) mp_table_destroy(pt->tables[i]);
  for (size_t i = 0; i < pt->tables.size(); ++i)
    if (pt->owner[i] == (int)i) mp_table_destroy(pt->tables[i]);
  delete pt;
}
int mp_pool_table_create(mp_pool* p, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key, uint32_t fb_window_bits,
                         mp_pool_table** out) {
  if (!p || !params || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_table_create: null pointer");
  MP_TRY
  std::lock_guard<std::mutex> lk(p->mu);
  const size_t M = p->members.size();
  mp_pool_table* pt = new mp_pool_table();
  pt->pool = p;
  pt->tables.assign(M, nullptr);
  pt->owner.assign(M, 0);
  pt->stats.resize(M);
  for (size_t i = 0; i < M; ++i) {
    size_t o = 0;
    while (p->members[o].device != p->members[i].device) ++o;      // (the first member of that device: o <= i)
    pt->owner[i] = (int)o;
    if (o == i) pt->builds++;
  }
  const uint8_t* key = shared_key ? shared_key : params;      // keyless, as mp_table_create_params: G stands in for the unused key
  std::vector<PoolResult> res;
  int rc = MP_OK;
  size_t bad = 0;
  // the owners build, one per device and all at once; then -- every build has been synchronised by its own call -- the borrowers
  for (int phase = 0; phase < 2 && rc == MP_OK; ++phase) {
    p->run(M, [&](size_t i) {
      const bool owns = pt->owner[i] == (int)i;
      if (owns != (phase == 0)) return (int)MP_OK;
      const int r = table_create(p->members[i].ctx, m, n, params, key, fb_window_bits, owns ? nullptr : pt->tables[pt->owner[i]], &pt->tables[i]);
      if (r == MP_OK && !shared_key) pt->tables[i]->keyless = true;
      return r;
    }, res);
    for (size_t i = M; i-- > 0;)
      if (res[i].rc != MP_OK) rc = res[i].rc, bad = i;
  }
  if (rc != MP_OK) {
    const std::string text = "mp_pool_table_create: " + pool_member_text(p, bad, res[bad].err);
    pool_table_release(pt);      // (mp_table_destroy of a null table is a no-op)
    return fail(rc, text);
  }
  *out = pt;
  return MP_OK;
  MP_CATCH
}
void mp_pool_table_destroy(mp_pool_table* pt) {
  if (!pt) return;
  std::lock_guard<std::mutex> lk(pt->pool->mu);
  pool_table_release(pt);
}
mp_table* mp_pool_table_member(mp_pool_table* pt, size_t i) { return pt && i < pt->tables.size() ? pt->tables[i] : nullptr; }
int mp_pool_set_min_shard(mp_pool_table* pt, size_t proofs) {
  if (!pt || !proofs) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_set_min_shard: a pool table and at least 1 proof per shard");
  std::lock_guard<std::mutex> lk(pt->pool->mu);
  pt->min_shard = proofs;
  return MP_OK;
}
int mp_pool_shuffle_and_remask_batch(mp_pool_table* pt, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                     const uint8_t* masking_factors, const uint32_t* permutations, const uint8_t* prover_seeds,
                                     uint8_t* out_decks, uint8_t* out_proofs, int32_t* status) {
  if (!pt) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_shuffle_and_remask_batch: null pool table");
  const mp_table* t0 = pt->tables[0];
  if (int bad = prove_batch_args(t0, B, shared_keys, decks, masking_factors, permutations, prover_seeds, out_decks, out_proofs, status)) return bad;
  MP_TRY
  const size_t N = t0->N, pb = t0->point_bytes, dsz = 2 * N * pb, psz = proof_size_bytes(t0->m, t0->n, t0->point_bytes);
  return pool_dispatch(pt, B, [&](size_t i, size_t f, size_t c) {
    mp_table* t = pt->tables[i];
    if (shared_keys)
      return mp_shuffle_and_remask_batch_keys(t, c, shared_keys + f * pb, decks + f * dsz, masking_factors + f * N * 32, permutations + f * N,
                                              prover_seeds + f * 32, out_decks + f * dsz, out_proofs + f * psz, status + f);
    return mp_shuffle_and_remask_batch(t, c, decks + f * dsz, masking_factors + f * N * 32, permutations + f * N, prover_seeds + f * 32,
                                       out_decks + f * dsz, out_proofs + f * psz, status + f);
  });
  MP_CATCH
}
int mp_pool_verify_shuffle_batch(mp_pool_table* pt, size_t B, const uint8_t* shared_keys, const uint8_t* decks, const uint8_t* shuffled_decks,
                                 const uint8_t* proofs, int32_t* status) {
  if (!pt) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_verify_shuffle_batch: null pool table");
  const mp_table* t0 = pt->tables[0];
  if (int bad = verify_batch_args(t0, B, shared_keys, decks, shuffled_decks, proofs, status)) return bad;
  MP_TRY
  const size_t N = t0->N, pb = t0->point_bytes, dsz = 2 * N * pb, psz = proof_size_bytes(t0->m, t0->n, t0->point_bytes);
  return pool_dispatch(pt, B, [&](size_t i, size_t f, size_t c) {
    mp_table* t = pt->tables[i];
    if (shared_keys)
      return mp_verify_shuffle_batch_keys(t, c, shared_keys + f * pb, decks + f * dsz, shuffled_decks + f * dsz, proofs + f * psz, status + f);
    return mp_verify_shuffle_batch(t, c, decks + f * dsz, shuffled_decks + f * dsz, proofs + f * psz, status + f);
  });
  MP_CATCH
}
int mp_pool_stats(const mp_pool_table* pt, uint64_t out[8]) {
  if (!pt || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_stats: bad argument");
  std::lock_guard<std::mutex> lk(pt->pool->mu);
  const uint64_t v[8] = {pt->calls, pt->proofs, pt->last_members, pt->builds, (uint64_t)pt->tables.size(), 0, 0, 0};
  memcpy(out, v, sizeof(v));
  return MP_OK;
}
int mp_pool_member_stats(const mp_pool_table* pt, size_t i, uint64_t out[4]) {
  if (!pt || !out || i >= pt->tables.size()) return fail(MP_ERR_BAD_ARGUMENT, "mp_pool_member_stats: bad argument");
  std::lock_guard<std::mutex> lk(pt->pool->mu);
  const uint64_t v[4] = {(uint64_t)pt->pool->members[i].device, pt->stats[i].calls, pt->stats[i].proofs, pt->stats[i].busy_us};
  memcpy(out, v, sizeof(v));
  return MP_OK;
}

int mp_remask_batch(mp_table* t, size_t count, const uint8_t* cards, const uint8_t* masking_factors, uint8_t* out) {
  if (!t || !count || !cards || !masking_factors || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_remask_batch: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->remask_host(count, cards, masking_factors, out);
  return MP_OK;
  MP_CATCH
}
int mp_msm(mp_table* t, size_t n_msm, size_t k, const uint8_t* scalars, const uint8_t* points, uint8_t* out) {
  if (!t || !n_msm || !k || !scalars || !points || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_msm: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->msm_host(n_msm, k, scalars, points, out);
  return MP_OK;
  MP_CATCH
}
int mp_commit_batch(mp_table* t, size_t count, size_t len, const uint8_t* values, const uint8_t* r, uint8_t* out) {
  if (!t || !count || !r || !out || (len && !values) || len > t->n) return fail(MP_ERR_BAD_ARGUMENT, "mp_commit_batch: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->commit_host(count, len, values, r, out);
  return MP_OK;
  MP_CATCH
}

int mp_profile_enable(mp_ctx* ctx, int on) {
  if (!ctx) return fail(MP_ERR_BAD_ARGUMENT, "null ctx");
  MP_TRY
  std::lock_guard<std::recursive_mutex> mp_lock_(ctx->mu);
  rt::stream_sync(ctx->stream);
  ctx->prof.report();
  ctx->prof.on = on != 0;
  return MP_OK;
  MP_CATCH
}
int mp_profile_report(mp_ctx* ctx, char* buf, size_t buf_len) {
  if (!ctx || !buf || !buf_len) return fail(MP_ERR_BAD_ARGUMENT, "mp_profile_report: bad argument");
  MP_TRY
  std::lock_guard<std::recursive_mutex> mp_lock_(ctx->mu);
  rt::stream_sync(ctx->stream);
  std::string r = ctx->prof.report();
  if (r.size() + 1 > buf_len) r.resize(buf_len - 1);
  memcpy(buf, r.c_str(), r.size() + 1);
  return MP_OK;
  MP_CATCH
}
int mp_work_census(mp_table* t, uint64_t* prove_terms, uint64_t* verify_terms, uint64_t* prove_point_ops, uint64_t* verify_point_ops) {
  if (!t || !prove_terms || !verify_terms || !prove_point_ops || !verify_point_ops) return fail(MP_ERR_BAD_ARGUMENT, "mp_work_census: bad argument");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->census(prove_terms, verify_terms, prove_point_ops, verify_point_ops);
  return MP_OK;
}

int mp_blake2s(const uint8_t* in, size_t len, uint8_t out[32]) {
  if ((!in && len) || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_blake2s: bad argument");
  Blake2sState st;
  blake2s_init(st);
  size_t off = 0;
  uint32_t m[16];
  while (len - off > 64) {
    memcpy(m, in + off, 64);
    off += 64;
    blake2s_compress(st, m, off, false);
  }
  memset(m, 0, 64);
  if (len - off) memcpy(m, in + off, len - off);
  blake2s_compress(st, m, len, true);
  memcpy(out, st.h, 32);
  return MP_OK;
}
int mp_sigma_prove_batch(mp_table* t, size_t B, uint32_t nbases, const uint8_t* bases, const uint8_t* publics,
                         const uint8_t* witness, const uint8_t* fs_init, const uint8_t* prover_seeds, uint8_t* out_proofs,
                         int32_t* status) {
  if (!t || !B || (nbases != 1 && nbases != 2) || !bases || !publics || !witness || !fs_init || !prover_seeds || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_sigma_prove_batch: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->sigma_host(true, B, nbases, bases, publics, witness, fs_init, prover_seeds, out_proofs, status);
  return MP_OK;
  MP_CATCH
}
int mp_sigma_verify_batch(mp_table* t, size_t B, uint32_t nbases, const uint8_t* bases, const uint8_t* publics,
                          const uint8_t* proofs, const uint8_t* fs_init, int32_t* status) {
  if (!t || !B || (nbases != 1 && nbases != 2) || !bases || !publics || !proofs || !fs_init || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_sigma_verify_batch: bad argument");
  MP_TRY
  MP_ENTER(t->ctx);
  t->sigma_host(false, B, nbases, bases, publics, nullptr, fs_init, nullptr, const_cast<uint8_t*>(proofs), status);
  return MP_OK;
  MP_CATCH
}

// ---- opening cards: reveal tokens with their proofs, and unmasking (engine_core.hpp "opening cards")
static const size_t OPEN_MAX_LANES = 1048576, OPEN_MAX_KEYS = 1048576, OPEN_MAX_CARD_LIST = 4096;
static bool open_shape_ok(size_t K, size_t C, uint32_t T) {
  return K >= 1 && K <= OPEN_MAX_KEYS && C >= 1 && C <= OPEN_MAX_LANES && T >= 1 && T <= OPEN_MAX_LANES && C * (size_t)T <= OPEN_MAX_LANES;
}
// The offsets array of the ragged calls, a host array: C + 1 entries, first[0] = 0, strictly increasing, first[C] <= max_lanes.  The
// caller's array is copied into a vector the table keeps and checked THERE, before anything is enqueued, and the device copy is made from
// that vector: no kernel ever sees an offset that was not validated, the caller may do what it likes with its array once the call has
// returned, and it does not matter whether the array is pageable or page-locked (a copy from page-locked memory is only queued when
// hipMemcpyAsync returns).  The vector is not touched again before the event behind its upload has passed.  Holds the context's lock.
// -> the device array, or nullptr for a malformed one
static const uint32_t* ragged_take(mp_table* t, size_t count, const uint32_t* first, size_t max_lanes) {
  if (count < 1 || count > max_lanes) return nullptr;
  rt::Stream s = t->ctx->stream;
  if (t->ragged_first_up)
    rt::event_sync(t->ragged_first_up);
  else
    t->ragged_first_up = rt::event_create();
  std::vector<uint32_t>& h = t->ragged_first_host;
  h.assign(first, first + count + 1);
  if (h[0] != 0 || h[count] > max_lanes) return nullptr;
  for (size_t c = 0; c < count; ++c)
    if (h[c + 1] <= h[c]) return nullptr;
  t->ragged_first.alloc(count + 1, s, false);
  rt::h2d(t->ragged_first.p, h.data(), (count + 1) * 4, s);
  rt::event_record(t->ragged_first_up, s);
  return t->ragged_first.p;
}
static const char* const RAGGED_SHAPE =
    "first[0] == 0, first strictly increasing, first[C] <= 1 048 576, 1 <= K <= 1 048 576, n_plain <= 4 096";
int mp_reveal_batch(mp_table* t, size_t K, const uint8_t* keys, const uint8_t* secret_keys, size_t C, const uint8_t* cards, uint32_t T,
                    const uint32_t* signer, const uint8_t* prover_seeds, uint8_t* out_tokens, uint8_t* out_proofs, int32_t* status) {
  if (!t || !keys || !secret_keys || !cards || !signer || !prover_seeds || !out_tokens || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_reveal_batch: null argument");
  if (!open_shape_ok(K, C, T)) return fail(MP_ERR_BAD_ARGUMENT, "mp_reveal_batch: 1 <= T, C * T <= 1 048 576, 1 <= K <= 1 048 576");
  MP_TRY
  MP_ENTER(t->ctx);
  t->reveal_host(K, keys, secret_keys, C, cards, T, signer, prover_seeds, out_tokens, out_proofs, status);
  return MP_OK;
  MP_CATCH
}
int mp_unmask_batch(mp_table* t, size_t K, const uint8_t* keys, size_t C, const uint8_t* cards, uint32_t T, const uint32_t* signer,
                    const uint8_t* tokens, const uint8_t* proofs, size_t n_plain, const uint8_t* plain_cards, uint8_t* out_plain,
                    uint32_t* out_index, int32_t* token_status, int32_t* card_status) {
  if (!t || !keys || !cards || !signer || !tokens || !proofs || (n_plain && !plain_cards) || !out_plain || !out_index || !token_status || !card_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_batch: null argument");
  if (!open_shape_ok(K, C, T) || n_plain > OPEN_MAX_CARD_LIST)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_batch: 1 <= T, C * T <= 1 048 576, 1 <= K <= 1 048 576, n_plain <= 4 096");
  MP_TRY
  MP_ENTER(t->ctx);
  return t->unmask_host(K, keys, C, cards, T, signer, tokens, proofs, n_plain, plain_cards, out_plain, out_index, token_status, card_status);
  MP_CATCH
}
int mp_unmask_batch_dev(mp_table* t, size_t K, const void* d_keys, size_t C, const void* d_cards, uint32_t T, const void* d_signer,
                        const void* d_tokens, const void* d_proofs, size_t n_plain, const void* d_plain_cards, void* d_out_plain,
                        void* d_out_index, void* d_token_status, void* d_card_status) {
  if (!t || !d_keys || !d_cards || !d_signer || !d_tokens || !d_proofs || (n_plain && !d_plain_cards) || !d_out_plain || !d_out_index ||
      !d_token_status || !d_card_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_batch_dev: null argument");
  if (!open_shape_ok(K, C, T) || n_plain > OPEN_MAX_CARD_LIST)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_batch_dev: 1 <= T, C * T <= 1 048 576, 1 <= K <= 1 048 576, n_plain <= 4 096");
  MP_TRY
  MP_ENTER(t->ctx);
  return t->unmask_dev(K, (const uint8_t*)d_keys, C, (const uint8_t*)d_cards, T, (const uint32_t*)d_signer, (const uint8_t*)d_tokens,
                       (const uint8_t*)d_proofs, n_plain, (const uint8_t*)d_plain_cards, (uint8_t*)d_out_plain, (uint32_t*)d_out_index,
                       (int32_t*)d_token_status, (int32_t*)d_card_status);
  MP_CATCH
}
int mp_reveal_ragged_batch(mp_table* t, size_t K, const uint8_t* keys, const uint8_t* secret_keys, size_t C, const uint8_t* cards,
                           const uint32_t* first, const uint32_t* signer, const uint8_t* prover_seeds, uint8_t* out_tokens,
                           uint8_t* out_proofs, int32_t* status) {
  if (!t || !keys || !secret_keys || !cards || !first || !signer || !prover_seeds || !out_tokens || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_reveal_ragged_batch: null argument");
  MP_TRY
  MP_ENTER(t->ctx);
  const uint32_t* d_first = K >= 1 && K <= OPEN_MAX_KEYS ? ragged_take(t, C, first, OPEN_MAX_LANES) : nullptr;
  if (!d_first) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_reveal_ragged_batch: ") + RAGGED_SHAPE);
  t->reveal_host(K, keys, secret_keys, C, cards, 0, signer, prover_seeds, out_tokens, out_proofs, status, d_first, t->ragged_first_host[C]);
  return MP_OK;
  MP_CATCH
}
int mp_unmask_ragged_batch(mp_table* t, size_t K, const uint8_t* keys, size_t C, const uint8_t* cards, const uint32_t* first,
                           const uint32_t* signer, const uint8_t* tokens, const uint8_t* proofs, size_t n_plain, const uint8_t* plain_cards,
                           uint8_t* out_plain, uint32_t* out_index, int32_t* token_status, int32_t* card_status) {
  if (!t || !keys || !cards || !first || !signer || !tokens || !proofs || (n_plain && !plain_cards) || !out_plain || !out_index || !token_status ||
      !card_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_ragged_batch: null argument");
  MP_TRY
  MP_ENTER(t->ctx);
  const uint32_t* d_first = K >= 1 && K <= OPEN_MAX_KEYS && n_plain <= OPEN_MAX_CARD_LIST ? ragged_take(t, C, first, OPEN_MAX_LANES) : nullptr;
  if (!d_first) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_unmask_ragged_batch: ") + RAGGED_SHAPE);
  return t->unmask_host(K, keys, C, cards, 0, signer, tokens, proofs, n_plain, plain_cards, out_plain, out_index, token_status, card_status,
                        d_first, t->ragged_first_host[C]);
  MP_CATCH
}
int mp_unmask_ragged_batch_dev(mp_table* t, size_t K, const void* d_keys, size_t C, const void* d_cards, const uint32_t* first,
                               const void* d_signer, const void* d_tokens, const void* d_proofs, size_t n_plain, const void* d_plain_cards,
                               void* d_out_plain, void* d_out_index, void* d_token_status, void* d_card_status) {
  if (!t || !d_keys || !d_cards || !first || !d_signer || !d_tokens || !d_proofs || (n_plain && !d_plain_cards) || !d_out_plain || !d_out_index ||
      !d_token_status || !d_card_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_unmask_ragged_batch_dev: null argument");
  MP_TRY
  MP_ENTER(t->ctx);
  const uint32_t* d_first = K >= 1 && K <= OPEN_MAX_KEYS && n_plain <= OPEN_MAX_CARD_LIST ? ragged_take(t, C, first, OPEN_MAX_LANES) : nullptr;
  if (!d_first) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_unmask_ragged_batch_dev: ") + RAGGED_SHAPE);
  return t->unmask_dev(K, (const uint8_t*)d_keys, C, (const uint8_t*)d_cards, 0, (const uint32_t*)d_signer, (const uint8_t*)d_tokens,
                       (const uint8_t*)d_proofs, n_plain, (const uint8_t*)d_plain_cards, (uint8_t*)d_out_plain, (uint32_t*)d_out_index,
                       (int32_t*)d_token_status, (int32_t*)d_card_status, false, d_first, t->ragged_first_host[C]);
  MP_CATCH
}

// ---- dealing and seating: masking / remasking with their proofs, and the tables' aggregate keys (engine_core.hpp "dealing and seating")
static const size_t DEAL_MAX_LANES = 1048576, DEAL_MAX_KEYS = 1048576;
static bool deal_shape_ok(int kind, size_t K, size_t C) {
  return (kind == MP_DEAL_MASK || kind == MP_DEAL_REMASK) && K >= 1 && K <= DEAL_MAX_KEYS && C >= 1 && C <= DEAL_MAX_LANES;
}
static const char* const DEAL_SHAPE = "kind is MP_DEAL_MASK or MP_DEAL_REMASK, 1 <= C <= 1 048 576, 1 <= K <= 1 048 576";
int mp_mask_batch(mp_table* t, int kind, size_t K, const uint8_t* keys, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                  const uint8_t* factors, const uint8_t* prover_seeds, uint8_t* out_masked, uint8_t* out_proofs, int32_t* status) {
  if (!t || !keys || !key_index || !inputs || !factors || !prover_seeds || !out_masked || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_mask_batch: null argument");
  if (!deal_shape_ok(kind, K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_mask_batch: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->mask_host(kind, K, keys, C, key_index, inputs, factors, prover_seeds, out_masked, out_proofs, status);
  return MP_OK;
  MP_CATCH
}
int mp_verify_mask_batch(mp_table* t, int kind, size_t K, const uint8_t* keys, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                         const uint8_t* masked, const uint8_t* proofs, int32_t* status) {
  if (!t || !keys || !key_index || !inputs || !masked || !proofs || !status) return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_mask_batch: null argument");
  if (!deal_shape_ok(kind, K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_verify_mask_batch: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_mask_host(kind, K, keys, C, key_index, inputs, masked, proofs, status);
  return MP_OK;
  MP_CATCH
}
int mp_verify_mask_batch_dev(mp_table* t, int kind, size_t K, const void* d_keys, size_t C, const void* d_key_index, const void* d_inputs,
                             const void* d_masked, const void* d_proofs, void* d_status) {
  if (!t || !d_keys || !d_key_index || !d_inputs || !d_masked || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_mask_batch_dev: null argument");
  if (!deal_shape_ok(kind, K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_verify_mask_batch_dev: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_mask_dev(kind, K, (const uint8_t*)d_keys, C, (const uint32_t*)d_key_index, (const uint8_t*)d_inputs, (const uint8_t*)d_masked,
                     (const uint8_t*)d_proofs, (int32_t*)d_status);
  return MP_OK;
  MP_CATCH
}
// dealing by index: the keys are those of a key set, key_index names slots
int mp_mask_batch_keyset(mp_table* t, const mp_keyset* ks, int kind, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                         const uint8_t* factors, const uint8_t* prover_seeds, uint8_t* out_masked, uint8_t* out_proofs, int32_t* status) {
  if (!t || !ks || ks->owner != t || !key_index || !inputs || !factors || !prover_seeds || !out_masked || !out_proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_mask_batch_keyset: bad argument (the key set must belong to this table)");
  if (!deal_shape_ok(kind, ks->K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_mask_batch_keyset: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->mask_host(kind, ks->K, nullptr, C, key_index, inputs, factors, prover_seeds, out_masked, out_proofs, status, ks);
  return MP_OK;
  MP_CATCH
}
int mp_verify_mask_batch_keyset(mp_table* t, const mp_keyset* ks, int kind, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                                const uint8_t* masked, const uint8_t* proofs, int32_t* status) {
  if (!t || !ks || ks->owner != t || !key_index || !inputs || !masked || !proofs || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_mask_batch_keyset: bad argument (the key set must belong to this table)");
  if (!deal_shape_ok(kind, ks->K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_verify_mask_batch_keyset: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_mask_host(kind, ks->K, nullptr, C, key_index, inputs, masked, proofs, status, ks);
  return MP_OK;
  MP_CATCH
}
int mp_verify_mask_batch_keyset_dev(mp_table* t, const mp_keyset* ks, int kind, size_t C, const void* d_key_index, const void* d_inputs,
                                    const void* d_masked, const void* d_proofs, void* d_status) {
  if (!t || !ks || ks->owner != t || !d_key_index || !d_inputs || !d_masked || !d_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_verify_mask_batch_keyset_dev: bad argument (the key set must belong to this table)");
  if (!deal_shape_ok(kind, ks->K, C)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_verify_mask_batch_keyset_dev: ") + DEAL_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->verify_mask_dev(kind, ks->K, nullptr, C, (const uint32_t*)d_key_index, (const uint8_t*)d_inputs, (const uint8_t*)d_masked,
                     (const uint8_t*)d_proofs, (int32_t*)d_status, ks);
  return MP_OK;
  MP_CATCH
}
int mp_aggregate_keys_batch(mp_table* t, size_t tables, uint32_t P, const uint8_t* keys, const uint8_t* proofs, const uint8_t* fs_init,
                            uint8_t* out_keys, int32_t* player_status, int32_t* table_status) {
  if (!t || !keys || !proofs || !fs_init || !out_keys || !player_status || !table_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_aggregate_keys_batch: null argument");
  if (P < 1 || tables < 1 || tables > DEAL_MAX_LANES || tables * (size_t)P > DEAL_MAX_LANES)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_aggregate_keys_batch: 1 <= P, 1 <= tables, tables * P <= 1 048 576");
  MP_TRY
  MP_ENTER(t->ctx);
  t->aggregate_keys_host(tables, P, keys, proofs, fs_init, out_keys, player_status, table_status);
  return MP_OK;
  MP_CATCH
}
int mp_aggregate_keys_ragged_batch(mp_table* t, size_t tables, const uint32_t* first, const uint8_t* keys, const uint8_t* proofs,
                                   const uint8_t* fs_init, uint8_t* out_keys, int32_t* player_status, int32_t* table_status) {
  if (!t || !first || !keys || !proofs || !fs_init || !out_keys || !player_status || !table_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_aggregate_keys_ragged_batch: null argument");
  MP_TRY
  MP_ENTER(t->ctx);
  const uint32_t* d_first = ragged_take(t, tables, first, DEAL_MAX_LANES);
  if (!d_first)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_aggregate_keys_ragged_batch: first[0] == 0, first strictly increasing, first[tables] <= 1 048 576");
  t->aggregate_keys_host(tables, 0, keys, proofs, fs_init, out_keys, player_status, table_status, d_first, t->ragged_first_host[tables]);
  return MP_OK;
  MP_CATCH
}
// seating straight into a key set: the sums of mp_aggregate_keys_ragged_batch go into the slots `slots` without leaving the device
int mp_keyset_seat_ragged_batch(mp_keyset* ks, size_t tables, const uint32_t* first, const uint32_t* slots, const uint8_t* keys,
                                const uint8_t* proofs, const uint8_t* fs_init, uint8_t* out_keys, int32_t* player_status, int32_t* table_status,
                                int32_t* slot_status) {
  if (!ks || !first || !slots || !keys || !proofs || !fs_init || !player_status || !table_status || !slot_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_seat_ragged_batch: null argument");
  MP_TRY
  mp_table* t = ks->owner;
  MP_ENTER(t->ctx);
  const uint32_t* d_slots = keyset_take(ks, tables, slots);
  if (!d_slots) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_keyset_seat_ragged_batch: ") + KEYSET_SLOTS);
  const uint32_t* d_first = ragged_take(t, tables, first, DEAL_MAX_LANES);
  if (!d_first)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_keyset_seat_ragged_batch: first[0] == 0, first strictly increasing, first[tables] <= 1 048 576");
  t->aggregate_keys_host(tables, 0, keys, proofs, fs_init, out_keys, player_status, table_status, d_first, t->ragged_first_host[tables], ks, d_slots,
                         slot_status);
  return MP_OK;
  MP_CATCH
}

// ---- secrets from seeds: "mpshuffle secret stream v1" (kernels_sample.hpp; engine_core.hpp "secrets from seeds")
static const size_t SAMPLE_MAX_LANES = 1048576;
static const uint32_t SAMPLE_MAX_COUNT = 4096;
static bool sample_shape_ok(size_t L, uint32_t S, uint32_t P) {
  return L >= 1 && L <= SAMPLE_MAX_LANES && S <= SAMPLE_MAX_COUNT && P <= SAMPLE_MAX_COUNT && (S || P);
}
static const char* const SAMPLE_SHAPE = "1 <= L <= 1 048 576, S <= 4 096, P <= 4 096, not both 0";
int mp_sample_secrets_batch(mp_table* t, size_t L, const uint8_t* seeds, uint32_t S, uint32_t P, uint8_t* out_scalars, uint32_t* out_perms) {
  if (!t || !seeds || (S && !out_scalars) || (P && !out_perms)) return fail(MP_ERR_BAD_ARGUMENT, "mp_sample_secrets_batch: null argument");
  if (!sample_shape_ok(L, S, P)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_sample_secrets_batch: ") + SAMPLE_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->sample_host(L, seeds, S, P, out_scalars, out_perms);
  return MP_OK;
  MP_CATCH
}
int mp_sample_secrets_batch_dev(mp_table* t, size_t L, const void* d_seeds, uint32_t S, uint32_t P, void* d_out_scalars, void* d_out_perms) {
  if (!t || !d_seeds || (S && !d_out_scalars) || (P && !d_out_perms)) return fail(MP_ERR_BAD_ARGUMENT, "mp_sample_secrets_batch_dev: null argument");
  if (!sample_shape_ok(L, S, P)) return fail(MP_ERR_BAD_ARGUMENT, std::string("mp_sample_secrets_batch_dev: ") + SAMPLE_SHAPE);
  MP_TRY
  MP_ENTER(t->ctx);
  t->sample_dev(L, (const uint8_t*)d_seeds, S, P, (uint8_t*)d_out_scalars, (uint32_t*)d_out_perms);
  return MP_OK;
  MP_CATCH
}
int mp_shuffle_and_remask_batch_seeded(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks, const uint8_t* seeds,
                                       uint8_t* out_decks, uint8_t* out_proofs, int32_t* status, uint32_t* out_perms, uint8_t* out_factors) {
  return prove_batch_host(t, B, shared_keys, decks, nullptr, nullptr, seeds, out_decks, out_proofs, status, true, out_perms, out_factors);
}
int mp_shuffle_and_remask_batch_seeded_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks, const void* d_seeds,
                                           void* d_out_decks, void* d_out_proofs, void* d_status, void* d_out_perms, void* d_out_factors) {
  if (!t || !B || !d_decks || !d_seeds || !d_out_decks || !d_out_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_seeded_dev: bad argument");
  if (t->keyless && !d_keys) return fail(MP_ERR_BAD_ARGUMENT, "this table has no aggregate key: pass one key per proof");
  if (B > SAMPLE_MAX_LANES) return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_seeded_dev: at most 1 048 576 proofs per call");
  MP_TRY
  MP_ENTER(t->ctx);
  rt::Stream s = t->ctx->stream;
  const size_t N = t->N;
  // the witness stays in the table's workspace unless the caller wants it
  if (!d_out_factors) t->seeded_rho.alloc(B * N * 32, s, false);
  if (!d_out_perms) t->seeded_perm.alloc(B * N, s, false);
  uint8_t* rho = d_out_factors ? (uint8_t*)d_out_factors : t->seeded_rho.p;
  uint32_t* perm = d_out_perms ? (uint32_t*)d_out_perms : t->seeded_perm.p;
  t->sample_dev(B, (const uint8_t*)d_seeds, (uint32_t)N, (uint32_t)N, rho, perm);
  t->prove_dev(B, (const uint8_t*)d_decks, rho, perm, (const uint8_t*)d_seeds, (uint8_t*)d_out_decks, (uint8_t*)d_out_proofs,
               (int32_t*)d_status, (const uint8_t*)d_keys);
  return MP_OK;
  MP_CATCH
}
int mp_shuffle_and_remask_batch_seeded_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                                  const void* d_seeds, void* d_out_decks, void* d_out_proofs, void* d_status, void* d_out_perms,
                                                  void* d_out_factors) {
  if (!t || !ks || ks->owner != t || !B || !d_key_index || !d_decks || !d_seeds || !d_out_decks || !d_out_proofs || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_seeded_keyset_dev: bad argument (the key set must belong to this table)");
  if (B > SAMPLE_MAX_LANES) return fail(MP_ERR_BAD_ARGUMENT, "mp_shuffle_and_remask_batch_seeded_keyset_dev: at most 1 048 576 proofs per call");
  MP_TRY
  MP_ENTER(t->ctx);
  rt::Stream s = t->ctx->stream;
  const size_t N = t->N;
  if (!d_out_factors) t->seeded_rho.alloc(B * N * 32, s, false);
  if (!d_out_perms) t->seeded_perm.alloc(B * N, s, false);
  uint8_t* rho = d_out_factors ? (uint8_t*)d_out_factors : t->seeded_rho.p;
  uint32_t* perm = d_out_perms ? (uint32_t*)d_out_perms : t->seeded_perm.p;
  t->sample_dev(B, (const uint8_t*)d_seeds, (uint32_t)N, (uint32_t)N, rho, perm);
  t->prove_dev(B, (const uint8_t*)d_decks, rho, perm, (const uint8_t*)d_seeds, (uint8_t*)d_out_decks, (uint8_t*)d_out_proofs,
               (int32_t*)d_status, nullptr, ks, (const uint32_t*)d_key_index);
  return MP_OK;
  MP_CATCH
}
int mp_keygen_batch(mp_table* t, size_t K, const uint8_t* seeds, const uint8_t* fs_init, uint8_t* out_keys, uint8_t* out_secret_keys,
                    uint8_t* out_proofs, int32_t* status) {
  if (!t || !seeds || !out_keys || !out_secret_keys || !status || (fs_init && !out_proofs))
    return fail(MP_ERR_BAD_ARGUMENT, "mp_keygen_batch: null argument");
  if (K < 1 || K > SAMPLE_MAX_LANES) return fail(MP_ERR_BAD_ARGUMENT, "mp_keygen_batch: 1 <= K <= 1 048 576");
  MP_TRY
  MP_ENTER(t->ctx);
  t->keygen_host(K, seeds, fs_init, out_keys, out_secret_keys, out_proofs, status);
  return MP_OK;
  MP_CATCH
}

int mp_plan_stats(mp_table* t, uint64_t out[16]) {
  if (!t || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_plan_stats: bad argument");
  std::lock_guard<std::recursive_mutex> mp_lock_(t->ctx->mu);
  t->plan_stats(out);
  return MP_OK;
}


// ---- canonical serialisation entry points (helpers: above the extern "C" block)

size_t mp_serialized_point_size(int curve_id) { return curve_ok(curve_id) ? (size_t)(kCurveBits[curve_id] + 2 + 7) / 8 : 0; }
size_t mp_serialized_deck_size(int curve_id, size_t cards) { return 8 + 2 * cards * mp_serialized_point_size(curve_id); }
size_t mp_serialized_params_size(int curve_id, uint32_t n) { return 24 + (size_t)(n + 3) * mp_serialized_point_size(curve_id); }
size_t mp_serialized_proof_size(int curve_id, uint32_t m, uint32_t n) {
  size_t sz = 0;
  for (const Group& g : proof_schema(m, n)) sz += (g.vec ? 8 : 0) + (size_t)g.count * (g.point ? mp_serialized_point_size(curve_id) : 32);
  return sz;
}
int mp_points_serialize(int curve_id, size_t count, const uint8_t* wire_points, uint8_t* out) {
  if (!curve_ok(curve_id) || (count && (!wire_points || !out))) return fail(MP_ERR_BAD_ARGUMENT, "mp_points_serialize: bad argument");
  MP_TRY
  if (ser_points(curve_id, false, count, wire_points, out) >= 0) return fail(MP_ERR_BAD_ENCODING, "point: coordinate out of range");
  return MP_OK;
  MP_CATCH
}
int mp_points_deserialize(int curve_id, size_t count, const uint8_t* data, uint8_t* out_wire_points) {
  if (!curve_ok(curve_id) || (count && (!data || !out_wire_points))) return fail(MP_ERR_BAD_ARGUMENT, "mp_points_deserialize: bad argument");
  MP_TRY
  if (ser_points(curve_id, true, count, data, out_wire_points) >= 0)
    return fail(MP_ERR_BAD_ENCODING, "point: non-canonical encoding, x not on the curve, or not in the prime-order subgroup");
  return MP_OK;
  MP_CATCH
}
int mp_deck_serialize(int curve_id, size_t cards, const uint8_t* wire_deck, uint8_t* out) {
  if (!curve_ok(curve_id) || !out || (cards && !wire_deck)) return fail(MP_ERR_BAD_ARGUMENT, "mp_deck_serialize: bad argument");
  put_u64(out, cards);
  return mp_points_serialize(curve_id, 2 * cards, wire_deck, out + 8);
}
int mp_deck_deserialize(int curve_id, const uint8_t* data, size_t len, size_t max_cards, uint8_t* out_wire_deck, size_t* out_cards) {
  if (!curve_ok(curve_id) || !data || !out_cards) return fail(MP_ERR_BAD_ARGUMENT, "mp_deck_deserialize: bad argument");
  if (len < 8) return fail(MP_ERR_BAD_ENCODING, "deck: not enough data");
  const uint64_t k = get_u64(data);
  if (k > max_cards || k > ((uint64_t)1 << 40)) return fail(MP_ERR_BAD_ARGUMENT, "deck: more cards than the output buffer holds");
  if (len != mp_serialized_deck_size(curve_id, (size_t)k)) return fail(MP_ERR_BAD_ENCODING, "deck: length does not match the card count");
  *out_cards = (size_t)k;
  return mp_points_deserialize(curve_id, 2 * (size_t)k, data + 8, out_wire_deck);
}
// Parameters { m, n, enc_parameters { generator }, commit_parameters { g: Vec, h }, generator } [REF mod.rs:37-43]; raw = G | ck | H | gen
int mp_params_serialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* raw_params, uint8_t* out) {
  if (!curve_ok(curve_id) || !raw_params || !out) return fail(MP_ERR_BAD_ARGUMENT, "mp_params_serialize: bad argument");
  const size_t pb = mp_point_size(curve_id), cb = mp_serialized_point_size(curve_id);
  put_u64(out, m);
  put_u64(out + 8, n);
  int rc = mp_points_serialize(curve_id, 1, raw_params, out + 16);
  if (rc) return rc;
  put_u64(out + 16 + cb, n);
  rc = mp_points_serialize(curve_id, n, raw_params + pb, out + 24 + cb);
  if (rc) return rc;
  return mp_points_serialize(curve_id, 2, raw_params + pb * (n + 1), out + 24 + cb * (n + 1));
}
int mp_params_deserialize(int curve_id, const uint8_t* data, size_t len, size_t max_n, uint32_t* m, uint32_t* n, uint8_t* out_raw_params) {
  if (!curve_ok(curve_id) || !data || !m || !n || !out_raw_params) return fail(MP_ERR_BAD_ARGUMENT, "mp_params_deserialize: bad argument");
  if (len < 16) return fail(MP_ERR_BAD_ENCODING, "parameters: not enough data");
  const uint64_t mm = get_u64(data), nn = get_u64(data + 8);
  if (nn > max_n || nn > 0x00FFFFFFull || mm > 0xFFFFFFFFull) return fail(MP_ERR_BAD_ARGUMENT, "parameters: n exceeds the output buffer");
  if (len != mp_serialized_params_size(curve_id, (uint32_t)nn)) return fail(MP_ERR_BAD_ENCODING, "parameters: length does not match n");
  const size_t pb = mp_point_size(curve_id), cb = mp_serialized_point_size(curve_id);
  if (get_u64(data + 16 + cb) != nn) return fail(MP_ERR_BAD_ENCODING, "parameters: commit key length != n");
  int rc = mp_points_deserialize(curve_id, 1, data + 16, out_raw_params);
  if (rc) return rc;
  rc = mp_points_deserialize(curve_id, (size_t)nn, data + 24 + cb, out_raw_params + pb);
  if (rc) return rc;
  rc = mp_points_deserialize(curve_id, 2, data + 24 + cb * (nn + 1), out_raw_params + pb * (nn + 1));
  if (rc) return rc;
  *m = (uint32_t)mm;
  *n = (uint32_t)nn;
  return MP_OK;
}
// ---- on-device decompression: compressed arkworks points in HBM -> wire v1 in HBM (kernels_decompress.hpp)
static int decompress_dev(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const void* d_in, void* d_out, void* d_status) {
  MP_TRY
  MP_ENTER(ctx);
  switch (ctx->curve) {
    case 0: return decompress_dev_Stark(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 1: return decompress_dev_Bn254(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 3: return decompress_dev_Bls12_377(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    default: return decompress_dev_Secp256k1(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
  }
  MP_CATCH
}
int mp_points_deserialize_dev(mp_ctx* ctx, size_t count, const void* d_data, void* d_out_wire_points, void* d_status) {
  if (!ctx || !count || !d_data || !d_out_wire_points || !d_status) return fail(MP_ERR_BAD_ARGUMENT, "mp_points_deserialize_dev: bad argument");
  return decompress_dev(ctx, count, 1, 0, d_data, d_out_wire_points, d_status);
}
int mp_deck_deserialize_dev(mp_ctx* ctx, size_t decks, size_t cards, const void* d_data, void* d_out_wire_decks, void* d_status) {
  if (!ctx || !decks || !cards || cards > 4096 || !d_data || !d_out_wire_decks || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_deck_deserialize_dev: bad argument");
  return decompress_dev(ctx, decks, (uint32_t)(2 * cards), 8, d_data, d_out_wire_decks, d_status);
}
int mp_proof_serialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* proof_wire, uint8_t* out) {
  if (!curve_ok(curve_id) || !proof_wire || !out || m < 2 || n < 2) return fail(MP_ERR_BAD_ARGUMENT, "mp_proof_serialize: bad argument");
  const size_t pb = mp_point_size(curve_id), cb = mp_serialized_point_size(curve_id);
  for (const Group& g : proof_schema(m, n)) {
    if (g.vec) {
      put_u64(out, g.vec_len);
      out += 8;
    }
    if (g.point) {
      const int rc = mp_points_serialize(curve_id, g.count, proof_wire, out);
      if (rc) return rc;
      proof_wire += pb * g.count;
      out += cb * g.count;
    } else {
      memcpy(out, proof_wire, 32 * (size_t)g.count);
      proof_wire += 32 * (size_t)g.count;
      out += 32 * (size_t)g.count;
    }
  }
  return MP_OK;
}
int mp_proof_deserialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* data, size_t len, uint8_t* out_proof_wire) {
  if (!curve_ok(curve_id) || !data || !out_proof_wire || m < 2 || n < 2) return fail(MP_ERR_BAD_ARGUMENT, "mp_proof_deserialize: bad argument");
  if (len != mp_serialized_proof_size(curve_id, m, n)) return fail(MP_ERR_BAD_ENCODING, "shuffle proof: wrong length");
  const size_t pb = mp_point_size(curve_id), cb = mp_serialized_point_size(curve_id);
  for (const Group& g : proof_schema(m, n)) {
    if (g.vec) {
      if (get_u64(data) != g.vec_len) return fail(MP_ERR_BAD_ENCODING, "shuffle proof: a vector has the wrong length");
      data += 8;
    }
    if (g.point) {
      const int rc = mp_points_deserialize(curve_id, g.count, data, out_proof_wire);
      if (rc) return rc;
      data += cb * g.count;
      out_proof_wire += pb * g.count;
    } else {
      if (!ser_scalars_ok(curve_id, g.count, data)) return fail(MP_ERR_BAD_ENCODING, "shuffle proof: scalar out of range");
      memcpy(out_proof_wire, data, 32 * (size_t)g.count);
      data += 32 * (size_t)g.count;
      out_proof_wire += 32 * (size_t)g.count;
    }
  }
  return MP_OK;
}

// ---- the remaining conversions on the device (kernels_canonical.hpp): wire -> canonical for points, decks and proofs, canonical ->
// wire for proofs; then the two host-buffer forms that upload, convert and download
static int compress_dev(mp_ctx* ctx, size_t groups, uint32_t per_group, uint32_t prefix, const void* d_in, void* d_out, void* d_status) {
  MP_TRY
  MP_ENTER(ctx);
  switch (ctx->curve) {
    case 0: return compress_dev_Stark(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 1: return compress_dev_Bn254(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 3: return compress_dev_Bls12_377(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    default: return compress_dev_Secp256k1(ctx, groups, per_group, prefix, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
  }
  MP_CATCH
}
// the element table of proof_schema(m, n) on the context (kernels_canonical.hpp: {canonical offset, wire offset, Vec length or 0}
// per element, points first): rebuilt when the shape changes, uploaded on the context's stream behind the kernels that read the old one
static void canon_table(mp_ctx* ctx, uint32_t m, uint32_t n, uint32_t* np, uint32_t* ns) {
  *np = 11 * m + 8;
  *ns = 5 * n + 9;
  if (ctx->cn_m == m && ctx->cn_n == n) return;
  const uint32_t pb = (uint32_t)mp_point_size(ctx->curve), cb = (uint32_t)mp_serialized_point_size(ctx->curve);
  std::vector<uint32_t> pts, scs;
  uint32_t co = 0, wo = 0;
  for (const Group& g : proof_schema(m, n)) {
    if (g.vec) co += 8;
    std::vector<uint32_t>& t = g.point ? pts : scs;
    const uint32_t cs = g.point ? cb : 32u, ws = g.point ? pb : 32u;
    for (uint32_t i = 0; i < g.count; ++i) {
      t.push_back(co);
      t.push_back(wo);
      t.push_back(g.vec && i == 0 ? g.vec_len : 0u);
      co += cs;
      wo += ws;
    }
  }
  if (pts.size() != 3 * (size_t)*np || scs.size() != 3 * (size_t)*ns) throw std::logic_error("proof schema: element count");
  ctx->cn_m = ctx->cn_n = 0;
  ctx->cn_tab_host = pts;
  ctx->cn_tab_host.insert(ctx->cn_tab_host.end(), scs.begin(), scs.end());
  ctx->cn_tab.upload(ctx->cn_tab_host, ctx->stream);
  rt::stream_sync(ctx->stream);      // (the host copy may be replaced by the next shape)
  ctx->cn_m = m;
  ctx->cn_n = n;
}
static int proof_convert_dev(mp_ctx* ctx, bool de, uint32_t m, uint32_t n, size_t B, const void* d_in, void* d_out, void* d_status) {
  MP_TRY
  MP_ENTER(ctx);
  uint32_t np, ns;
  canon_table(ctx, m, n, &np, &ns);
  const uint32_t cs = (uint32_t)mp_serialized_proof_size(ctx->curve, m, n), ws = (uint32_t)mp_proof_size_curve(ctx->curve, m, n);
  switch (ctx->curve) {
    case 0: return proof_convert_dev_Stark(ctx, de, np, ns, cs, ws, B, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 1: return proof_convert_dev_Bn254(ctx, de, np, ns, cs, ws, B, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    case 3: return proof_convert_dev_Bls12_377(ctx, de, np, ns, cs, ws, B, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
    default: return proof_convert_dev_Secp256k1(ctx, de, np, ns, cs, ws, B, (const uint8_t*)d_in, (uint8_t*)d_out, (int32_t*)d_status);
  }
  MP_CATCH
}
// shapes whose proofs the 32-bit offsets of the element table address
static bool proof_shape_ok(uint32_t m, uint32_t n) { return m >= 2 && n >= 2 && m <= (1u << 20) && n <= (1u << 20); }

int mp_points_serialize_dev(mp_ctx* ctx, size_t count, const void* d_wire_points, void* d_out, void* d_status) {
  if (!ctx || !count || !d_wire_points || !d_out || !d_status) return fail(MP_ERR_BAD_ARGUMENT, "mp_points_serialize_dev: bad argument");
  return compress_dev(ctx, count, 1, 0, d_wire_points, d_out, d_status);
}
int mp_deck_serialize_dev(mp_ctx* ctx, size_t decks, size_t cards, const void* d_wire_decks, void* d_out, void* d_status) {
  if (!ctx || !decks || !cards || cards > 4096 || !d_wire_decks || !d_out || !d_status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_deck_serialize_dev: bad argument");
  return compress_dev(ctx, decks, (uint32_t)(2 * cards), 8, d_wire_decks, d_out, d_status);
}
int mp_proof_serialize_dev(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const void* d_proofs_wire, void* d_out, void* d_status) {
  if (!ctx || !B || !d_proofs_wire || !d_out || !d_status || !proof_shape_ok(m, n))
    return fail(MP_ERR_BAD_ARGUMENT, "mp_proof_serialize_dev: bad argument");
  return proof_convert_dev(ctx, false, m, n, B, d_proofs_wire, d_out, d_status);
}
int mp_proof_deserialize_dev(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const void* d_data, void* d_out_proofs_wire, void* d_status) {
  if (!ctx || !B || !d_data || !d_out_proofs_wire || !d_status || !proof_shape_ok(m, n))
    return fail(MP_ERR_BAD_ARGUMENT, "mp_proof_deserialize_dev: bad argument");
  return proof_convert_dev(ctx, true, m, n, B, d_data, d_out_proofs_wire, d_status);
}
// host buffers: one upload, the _dev conversion, one download -- all on the context's stream, finished when the call returns.  The
// staging buffers stay with the context and grow to the largest call
static int deserialize_batch(mp_ctx* ctx, size_t units, size_t in_bytes, size_t out_bytes, const uint8_t* data, uint8_t* out, int32_t* status,
                             const std::function<int(void*, void*, void*)>& convert) {
  MP_TRY
  MP_ENTER(ctx);
  ctx->cn_in.alloc(in_bytes, ctx->stream, false);
  ctx->cn_out.alloc(out_bytes, ctx->stream, false);
  ctx->cn_status.alloc(units, ctx->stream, false);
  rt::h2d(ctx->cn_in.p, data, in_bytes, ctx->stream);
  const int rc = convert(ctx->cn_in.p, ctx->cn_out.p, ctx->cn_status.p);
  if (rc == MP_OK) {
    rt::d2h(out, ctx->cn_out.p, out_bytes, ctx->stream);
    rt::d2h(status, ctx->cn_status.p, units * sizeof(int32_t), ctx->stream);
  }
  rt::stream_sync(ctx->stream);
  return rc;
  MP_CATCH
}
int mp_decks_deserialize_batch(mp_ctx* ctx, size_t decks, size_t cards, const uint8_t* data, uint8_t* out_wire_decks, int32_t* status) {
  if (!ctx || !decks || !cards || cards > 4096 || !data || !out_wire_decks || !status)
    return fail(MP_ERR_BAD_ARGUMENT, "mp_decks_deserialize_batch: bad argument");
  return deserialize_batch(ctx, decks, decks * mp_serialized_deck_size(ctx->curve, cards), decks * 2 * cards * mp_point_size(ctx->curve), data,
                           out_wire_decks, status,
                           [&](void* d_in, void* d_out, void* d_st) { return mp_deck_deserialize_dev(ctx, decks, cards, d_in, d_out, d_st); });
}
int mp_proofs_deserialize_batch(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const uint8_t* data, uint8_t* out_proofs_wire, int32_t* status) {
  if (!ctx || !B || !data || !out_proofs_wire || !status || !proof_shape_ok(m, n))
    return fail(MP_ERR_BAD_ARGUMENT, "mp_proofs_deserialize_batch: bad argument");
  return deserialize_batch(ctx, B, B * mp_serialized_proof_size(ctx->curve, m, n), B * mp_proof_size_curve(ctx->curve, m, n), data,
                           out_proofs_wire, status,
                           [&](void* d_in, void* d_out, void* d_st) { return mp_proof_deserialize_dev(ctx, m, n, B, d_in, d_out, d_st); });
}

}
