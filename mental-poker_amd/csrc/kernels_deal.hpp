// Dealing and seating in batches: the two phases of a round that come before the shuffle
// [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:151-298, examples/round.rs:228-262].
// Dealing: every card of the initial deck is masked (or a masked card remasked) with a Chaum-Pedersen proof, and every player verifies
// all of them.  mask is remask of (O, card) [REF remasking.rs:10-22], so one statement covers both:
//   bases (G, pk), publics (r G, r pk) = masked - in, fs_init = Blake2s("Masking Proof") | Blake2s("Remasking Proof").
// The statements of C cards are assembled on the device from the compact inputs (keys, key indices, cards), one lane per card; the
// verifier's two differences are one complete mixed addition each, made affine by the batched inversion before the transcript absorbs
// them.  Transcript, check MSMs and verdict are those of kernels_sigma.hpp.
// Seating: one Schnorr proof per player on (G, pk), lane = table * P + seat; the sum of a table's keys has one lane per table.
#pragma once
#include "kernels_open.hpp"

namespace mp {

// P slots of a dealing lane: the statement of kernels_sigma.hpp (g_0 = G, g_1 = pk, a_0, a_1, A_0, A_1), then the input card and the
// masked card (two points each; the J arena mirrors them).  The check slots follow.
struct DealLay {
  SigmaLay s;
  uint32_t in, out, nP;
};
MP_HD DealLay make_deal_lay() {
  DealLay l;
  l.s = make_sigma_lay(2);
  l.in = 3 * l.s.nb;
  l.out = l.in + 2;
  l.nP = l.out + 2;
  l.s.chk = l.nP;
  return l;
}

struct DealStmtArgs {
  uint32_t* P;
  uint32_t* J;
  uint32_t* S;
  int32_t* status;            // [Bpad], zeroed before
  const uint8_t* keys;        // [K] wire points
  const uint32_t* key_index;  // [C]
  const uint8_t* inputs;      // [C] one wire point (masking: the plaintext card) or c0 || c1 (remasking)
  const uint8_t* masked;      // [C] c0 || c1 (verifying) or nullptr (proving: the masked card is computed)
  const uint8_t* factors;     // [C][32] (proving) or nullptr
  const uint32_t* fbpts;      // the table's fixed bases, affine
  uint8_t* fs_init;           // [C][32]: every lane gets the one digest
  uint32_t fs_seed[8];
  DealLay l;
  uint32_t Bpad, K, g_base, remask;
  const uint32_t* live = nullptr;   // dealing by index (mp_mask_batch_keyset): keys are a key set's wire keys, [K] words, 1 = the slot holds a key
};
// x = card, y = 0: g_0 = G, the digest and (proving) the factor as the witness; 1: g_1 = keys[key_index]; 2, 3: component y - 2 of the
// input card and (verifying) of the masked card with their difference, Jacobian, in the J slot of a_{y-2}.  A lane whose key index is
// past the key list gets MP_ERR_BAD_ARGUMENT from every y and the identity in every slot; k_deal_finish writes the word once more
// after every other test (the rule of body_open_stmt).
template <class C>
MP_HD void body_deal_stmt(const DealStmtArgs& a, uint32_t b, uint32_t y) {
  typedef typename C::FrP R;
  constexpr uint32_t PB = Geo<C>::PB;
  const SigmaLay& l = a.l.s;
  const uint32_t ki = a.key_index[b];
  const bool known = ki < a.K && (!a.live || a.live[ki] != 0u);
  if (!known) status_fail(a.status, b, ST_BAD_ARGUMENT);
  bool ok = true;
  if (y == 0) {
    Aff<C> g = ld_aff<C>(a.fbpts + (size_t)a.g_base * Geo<C>::PW);
    if (!known) g = aff_inf<C>();
    st_aff<C>(a.P + p_off<C>(l.g, a.Bpad, b), g);
    uint32_t* fw = reinterpret_cast<uint32_t*>(a.fs_init + (size_t)b * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) fw[i] = a.fs_seed[i];
    if (a.factors) {
      Fe<R> x;
      if (!wire_to_fe<R>(a.factors + (size_t)b * 32, x)) {
        ok = false;
        x = fe_zero<R>();
      }
      st_fe<R>(a.S + s_off(l.x, a.Bpad, b), x);
    }
  } else if (y == 1) {
    Aff<C> pk = aff_inf<C>();
    if (known) ok = wire_to_aff<C>(a.keys + (size_t)ki * PB, pk);
    if (!ok) pk = aff_inf<C>();
    st_aff<C>(a.P + p_off<C>(l.g + 1, a.Bpad, b), pk);
  } else {
    const uint32_t i = y - 2;
    Aff<C> in = aff_inf<C>(), out = aff_inf<C>();
    if (a.remask)
      ok = wire_to_aff<C>(a.inputs + ((size_t)b * 2 + i) * PB, in);
    else if (i == 1)
      ok = wire_to_aff<C>(a.inputs + (size_t)b * PB, in);      // mask = remask of (O, card)
    if (a.masked) ok &= wire_to_aff<C>(a.masked + ((size_t)b * 2 + i) * PB, out);
    if (!ok || !known) in = out = aff_inf<C>();
    st_aff<C>(a.P + p_off<C>(a.l.in + i, a.Bpad, b), in);
    if (a.masked) {
      st_aff<C>(a.P + p_off<C>(a.l.out + i, a.Bpad, b), out);
      Jac<C> d = jac_from_aff<C>(out);
      jac_madd_ip<C>(d, aff_neg<C>(in));      // complete: in = O, out = O, out = in (d = O) and out = -in (a doubling) take its rare branches
      st_jac<C>(a.J + j_off<C>(l.a + i, a.Bpad, b), d);
    }
  }
  if (!ok && known) status_fail(a.status, b, ST_BAD_ENCODING);
}
MP_KERNEL_OCC(k_deal_stmt, DealStmtArgs, body_deal_stmt, 2)

struct DealAddArgs {
  const uint32_t* P;
  uint32_t* J;
  DealLay l;
  uint32_t Bpad;
};
// the prover's masked card: out_y = in_y + a_y, y = 0, 1 (a = (x G, x pk), affine by now), Jacobian in the J slot of out_y
template <class C>
MP_HD void body_deal_add(const DealAddArgs& a, uint32_t b, uint32_t y) {
  Jac<C> s = jac_from_aff<C>(ld_aff<C>(a.P + p_off<C>(a.l.in + y, a.Bpad, b)));
  jac_madd_ip<C>(s, ld_aff<C>(a.P + p_off<C>(a.l.s.a + y, a.Bpad, b)));
  st_jac<C>(a.J + j_off<C>(a.l.out + y, a.Bpad, b), s);
}
MP_KERNEL_OCC(k_deal_add, DealAddArgs, body_deal_add, 2)

struct DealFinishArgs {
  const int32_t* wstatus;     // [Bpad]: the lanes' words in the workspace
  const uint32_t* key_index;  // [C]
  int32_t* status;            // [C] out
  uint8_t* out_masked;        // [C] c0 || c1 (proving) or nullptr
  uint8_t* out_proofs;        // [C] proofs (proving) or nullptr
  uint32_t K;
  const uint32_t* live = nullptr;   // as DealStmtArgs::live
};
// the status word of a card, MP_ERR_BAD_ARGUMENT for a key index past the list whatever the later tests wrote; a prover lane with a
// word that is not 0 gives zero bytes
template <class C>
MP_HD void body_deal_finish(const DealFinishArgs& a, uint32_t b, uint32_t y) {
  constexpr uint32_t CW = 2 * Geo<C>::PB / 4, QW = (2 * Geo<C>::PB + 32) / 4;
  const uint32_t ki = a.key_index[b];
  const int32_t st = ki < a.K && (!a.live || a.live[ki] != 0u) ? a.wstatus[b] : ST_BAD_ARGUMENT;
  a.status[b] = st;
  if (st != 0 && a.out_masked) {
    uint32_t* m = reinterpret_cast<uint32_t*>(a.out_masked) + (size_t)b * CW;
    uint32_t* p = reinterpret_cast<uint32_t*>(a.out_proofs) + (size_t)b * QW;
    for (uint32_t i = 0; i < CW; ++i) m[i] = 0;
    for (uint32_t i = 0; i < QW; ++i) p[i] = 0;
  }
}
MP_KERNEL(k_deal_finish, DealFinishArgs, body_deal_finish)

// ---- seating
struct SeatStmtArgs {
  uint32_t* P;
  int32_t* status;          // [Bpad], zeroed before
  const uint8_t* keys;      // [lanes] wire points
  const uint32_t* fbpts;
  SigmaLay l;               // one base
  uint32_t Bpad, g_base;
};
// x = lane (table * P + seat), y = 0: g = G, 1: a = the player's key
template <class C>
MP_HD void body_seat_stmt(const SeatStmtArgs& a, uint32_t b, uint32_t y) {
  Aff<C> pt;
  if (y == 0) {
    pt = ld_aff<C>(a.fbpts + (size_t)a.g_base * Geo<C>::PW);
  } else if (!wire_to_aff<C>(a.keys + (size_t)b * Geo<C>::PB, pt)) {
    status_fail(a.status, b, ST_BAD_ENCODING);
    pt = aff_inf<C>();
  }
  st_aff<C>(a.P + p_off<C>(y == 0 ? a.l.g : a.l.a, a.Bpad, b), pt);
}
MP_KERNEL(k_seat_stmt, SeatStmtArgs, body_seat_stmt)

struct KeySumArgs {
  const uint32_t* P;        // keys: slot a of the lanes
  const int32_t* status;    // [Bpad]: the lanes' verdicts
  uint32_t* sumJ;           // [tables] Jacobian: the sum of the table's keys, the identity for a table with a bad seat
  int32_t* player_status;   // [lanes] out
  int32_t* table_status;    // [tables] out
  uint32_t Bpad, seats, a_slot;
  const uint32_t* first;    // [tables + 1] offsets (then seats is not read), or nullptr: the table's lanes are k * seats .. k * seats + seats - 1
};
// One lane per table (the shape of k_unmask_sum).  The table's word is the first of its seats' that is not 0, in seat order: the
// reference stops at the first bad proof.  A table whose proofs all verified gets the sum of its keys as they are given; every
// addition is the complete mixed addition of curve.hpp: a key at infinity, one key twice (a doubling) and keys that cancel take its
// rare branches.
template <class C>
MP_HD void body_key_sum(const KeySumArgs& a, uint32_t k, uint32_t y) {
  const uint32_t b0 = a.first ? a.first[k] : k * a.seats, b1 = a.first ? a.first[k + 1] : b0 + a.seats;
  int32_t first = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    const int32_t st = a.status[b];
    a.player_status[b] = st;
    if (first == 0) first = st;
  }
  Jac<C> acc = jac_inf<C>();
  if (first == 0) {
#pragma unroll 1
    for (uint32_t b = b0; b < b1; ++b) jac_madd_ip<C>(acc, ld_aff<C>(a.P + p_off<C>(a.a_slot, a.Bpad, b)));
  }
  st_jac<C>(a.sumJ + (size_t)k * Geo<C>::JW, acc);
  a.table_status[k] = first;
}
MP_KERNEL_OCC(k_key_sum, KeySumArgs, body_key_sum, 2)

}  // namespace mp
