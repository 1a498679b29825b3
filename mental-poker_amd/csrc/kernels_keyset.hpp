// kernels_keyset.hpp -- key sets whose slots change (mp_keyset_update[_dev], mp_keyset_clear; engine_core.hpp keyset_update) and the calls
// that name a key by its slot (dealing, seating and chains by index, further down): the
// validation of the keys that enter a set, and the way of their window tables from the staging of a build slice into the set.
//
// A set is `capacity` slots, each live or empty (mp_keyset::live, one word per slot).  An update names `count` distinct slots (a host
// array that capi.hip keyset_take has copied, checked and uploaded) and brings one wire key for each.  k_keyset_slots decides, one lane
// per key, whether the key may enter -- canonical, on the curve, not the identity, in the prime-order subgroup whatever
// mp_set_subgroup_check says: this IS the validation, as mp_keyset_create's host loop is -- and leaves the slot live with the key's
// wire words, or EMPTY with zero words whatever it held before.  The tables of the accepted keys are built by the passes of the table
// context's own fixed-base tables (k_fb_windows, k_fb_fill, k_normalize) into a staging of one slice and moved into their slots by
// k_keyset_scatter.  No LDS, no atomics: the slots of a call are distinct, so no two lanes write one word.
#pragma once
#include "kernels_msm.hpp"
#include "kernels_proto.hpp"

namespace mp {

struct KeysetSlotsArgs {
  const uint8_t* keys;      // [count] wire points, or null: the slots are emptied (mp_keyset_clear)
  const uint32_t* slots;    // [count]: distinct, below the set's capacity
  uint32_t* wire;           // the set's wire keys, [capacity][PB / 4]
  uint32_t* live;           // [capacity]
  uint32_t* pts;            // [count] affine: what the table build starts from (the identity for a refused key)
  int32_t* status;          // [count]: 0, or MP_ERR_BAD_ENCODING; null with keys == null
};
// x = key of the call
template <class C>
MP_HD void body_keyset_slots(const KeysetSlotsArgs& a, uint32_t i, uint32_t) {
  constexpr uint32_t W = Geo<C>::PB / 4;
  const uint32_t slot = a.slots[i];
  uint32_t k[W];
#pragma unroll
  for (uint32_t j = 0; j < W; ++j) k[j] = 0u;
  bool ok = false;
  if (a.keys) {
    const uint8_t* src = a.keys + (size_t)i * Geo<C>::PB;
    Aff<C> p;
    ok = wire_to_aff<C>(src, p) && !aff_is_inf<C>(p);
    if (!Cofactor<C>::ONE) ok = ok && aff_in_subgroup_dev<C>(p);
    if (ok) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(src);      // wire buffers are 4-byte aligned (API contract)
#pragma unroll
      for (uint32_t j = 0; j < W; ++j) k[j] = q[j];
    } else {
      p = aff_inf<C>();
    }
    st_aff<C>(a.pts + (size_t)i * Geo<C>::PW, p);
    a.status[i] = ok ? 0 : -1;      // MP_ERR_BAD_ENCODING
  }
  st_words<W>(a.wire + (size_t)slot * W, k);
  a.live[slot] = ok ? 1u : 0u;
}
MP_KERNEL_OCC(k_keyset_slots, KeysetSlotsArgs, body_keyset_slots, 2)

// x = 16-byte word of a key's tables, y = key of the slice; the tables of a refused key stay where they are
struct KeysetScatterArgs {
  const uint4* tab;         // [keys of the slice][words]: the staging
  uint4* FB;                // the set's tables, [capacity][words]
  const uint32_t* slots;
  const uint32_t* live;
  uint32_t words;           // 16-byte words of one key's tables
};
template <class C>
MP_HD void body_keyset_scatter(const KeysetScatterArgs& a, uint32_t x, uint32_t y) {
  const uint32_t slot = a.slots[y];
  if (a.live[slot]) a.FB[(size_t)slot * a.words + x] = a.tab[(size_t)y * a.words + x];
}
MP_KERNEL(k_keyset_scatter, KeysetScatterArgs, body_keyset_scatter)

// ---- dealing by index (mp_mask_batch_keyset): the prover's two products with the key, x pk for the masked card and r pk for the
// commitment, are sums of entries of the set's 8-bit tables -- one table addition per non-zero byte of the scalar, 32 at the most, and
// no window table of pk per card (the shape of body_key_terms with keyed == 2).  x = card; the sum goes, Jacobian, to J slot j_slot,
// which the phase's normalisation makes affine with its neighbour from the fixed-base table of G.  A card that names no key gets the
// identity (its word is MP_ERR_BAD_ARGUMENT and its output zero bytes: k_deal_stmt, k_deal_finish).
struct DealKeyTermArgs {
  const uint32_t* S;
  uint32_t* J;
  uint32_t Bpad, s_slot, j_slot;
  const uint32_t* KFB;      // the set's tables, [slot][window][entry] affine
  const uint32_t* kidx;     // [C]
  const uint32_t* live;
  FbGeom kg;
  uint32_t nkeys;
};
template <class C>
MP_HD void body_deal_key_term(const DealKeyTermArgs& a, uint32_t b, uint32_t) {
  typedef typename C::FrP R;
  bool named;
  const uint32_t key = keyset_slot(a.kidx, b, a.nkeys, a.live, named);
  Xyzz<C> acc = xyzz_inf<C>();
  if (named) {
    uint32_t k[8];
    fe_to_canonical<R>(ld_fe<R>(a.S + s_off(a.s_slot, a.Bpad, b)), k);
#pragma unroll 1
    for (uint32_t w = 0; w < a.kg.windows; ++w) {
      const uint32_t d = fb_digit(k, a.kg, w);
      if (d) xyzz_madd_ip<C>(acc, ld_aff<C>(fb_entry<C>(a.KFB, a.kg, key, w, d)));
    }
  }
  st_jac<C>(a.J + j_off<C>(a.j_slot, a.Bpad, b), xyzz_to_jac<C>(acc));
}
MP_KERNEL_OCC(k_deal_key_term, DealKeyTermArgs, body_deal_key_term, Geo<C>::OCC4)

// ---- seating into a set (mp_keyset_seat_ragged_batch): the word of slot k is the table's word where that is not 0, else the word of the
// update (MP_ERR_BAD_ENCODING for a sum that is the identity); x = table
struct KeysetSeatStatusArgs {
  const int32_t* table_status;
  int32_t* slot_status;     // in: the update's words
};
template <class C>
MP_HD void body_keyset_seat_status(const KeysetSeatStatusArgs& a, uint32_t k, uint32_t) {
  if (a.table_status[k] != 0) a.slot_status[k] = a.table_status[k];
}
MP_KERNEL(k_keyset_seat_status, KeysetSeatStatusArgs, body_keyset_seat_status)

// ---- chains by index (mp_verify_shuffle_chain_ragged_keyset[_dev]): table t names ONE slot, the chain verifier wants a key per link.
// The links of table t are the rows off[t] .. off[t + 1] - 1 of the table-major arrays.  x = table, y = 32-bit word of the point.
struct KeysetChainKeysArgs {
  const uint32_t* wire;     // the set's wire keys
  const uint32_t* live;
  const uint32_t* kidx;     // [tables]
  const uint32_t* off;      // [tables + 1]: validated by the host with the links
  uint32_t* out;            // [links in all][PB / 4]
  uint32_t nkeys;
};
template <class C>
MP_HD void body_keyset_chain_keys(const KeysetChainKeysArgs& a, uint32_t t, uint32_t y) {
  constexpr uint32_t W = Geo<C>::PB / 4;
  bool named;
  const uint32_t v = a.wire[(size_t)keyset_slot(a.kidx, t, a.nkeys, a.live, named) * W + y];
  for (uint32_t r = a.off[t]; r < a.off[t + 1]; ++r) a.out[(size_t)r * W + y] = v;
}
MP_KERNEL(k_keyset_chain_keys, KeysetChainKeysArgs, body_keyset_chain_keys)
// behind the chain verifier: every link of a table that named no key reads MP_ERR_BAD_ARGUMENT (x = table)
struct KeysetChainStatusArgs {
  const uint32_t* live;
  const uint32_t* kidx;
  const uint32_t* off;
  int32_t* status;          // [links in all]
  uint32_t nkeys;
};
template <class C>
MP_HD void body_keyset_chain_status(const KeysetChainStatusArgs& a, uint32_t t, uint32_t) {
  bool named;
  keyset_slot(a.kidx, t, a.nkeys, a.live, named);
  if (named) return;
  for (uint32_t r = a.off[t]; r < a.off[t + 1]; ++r) a.status[r] = -3;
}
MP_KERNEL(k_keyset_chain_status, KeysetChainStatusArgs, body_keyset_chain_status)

}  // namespace mp
