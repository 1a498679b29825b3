// Opening cards in batches: every card that is looked at or shown takes one reveal token with a Chaum-Pedersen proof from each
// player, and whoever opens it verifies the proofs and computes c1 - sum of the tokens
// [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:300-378, examples/round.rs:159-206, 352-430].
// The statements of the T tokens of C cards are assembled on the device from the compact inputs (keys, cards, signer indices,
// tokens), lane b = c * T + j -- or, with an offsets array `first` ([C + 1], device memory), the lanes first[c] .. first[c+1] - 1 for
// card c, so that the cards of one call may carry different numbers of tokens; transcript, check MSMs and verdict are those of kernels_sigma.hpp with
//   bases (c0, G), publics (token, pk[signer]), fs_init = Blake2s("Reveal Proof").
// The token sums and the card lookup have one lane per card.
#pragma once
#include "kernels_sigma.hpp"

namespace mp {

static const int32_t ST_BAD_ARGUMENT = -3;          // MP_ERR_BAD_ARGUMENT: a signer index past the key list
static const uint32_t OPEN_NO_INDEX = 0xFFFFFFFFu;  // out_index of a card that is not in the list (or was not opened)

struct OpenStmtArgs {
  uint32_t* P;
  uint32_t* S;
  int32_t* status;          // [Bpad], zeroed before
  const uint8_t* keys;      // [K] wire points
  const uint8_t* cards;     // [C] c0 || c1
  const uint32_t* signer;   // [B]
  const uint8_t* tokens;    // [B] wire points (opening) or nullptr (revealing: the token is computed)
  const uint8_t* sks;       // [K][32] secret keys (revealing) or nullptr
  const uint32_t* fbpts;    // the table's fixed bases, affine
  uint8_t* fs_init;         // [B][32]: every lane gets the one digest
  uint32_t* c1;             // [C] affine: the cards' second halves (opening) or nullptr
  int32_t* cstat;           // [C], zeroed before: MP_ERR_BAD_ENCODING where c1 is no valid point
  uint32_t fs_seed[8];
  SigmaLay l;
  uint32_t Bpad, K, T, g_base;
  const uint32_t* first;    // [C + 1] offsets (then T is not read), or nullptr: lane b = c * T + j
  uint32_t C;               // the number of cards, read with `first` only
};
// The card of lane b under an offsets array: the last c with first[c] <= b.  A binary search, at most 21 probes (C <= 2^20) of an
// array that every lane of the launch reads and that stays in cache.  The host has checked first[0] = 0 < first[1] < ... < first[C]
// = the number of lanes, so the answer is below C for every lane of the launch.
MP_HD uint32_t card_of_lane(const uint32_t* first, uint32_t C, uint32_t b) {
  uint32_t lo = 0, hi = C;          // first[lo] <= b < first[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}
// x = lane, y = statement slot: 0 g_0 = c0 of the card, 1 g_1 = G, 2 a_0 = the token (revealing: the witness sk[signer] instead),
// 3 a_1 = keys[signer].  A lane whose signer is past the key list gets MP_ERR_BAD_ARGUMENT from every y and the identity in every
// slot, so that no later test can put another code in its place.
template <class C>
MP_HD void body_open_stmt(const OpenStmtArgs& a, uint32_t b, uint32_t y) {
  typedef typename C::FrP R;
  const uint32_t c = a.first ? card_of_lane(a.first, a.C, b) : b / a.T, sg = a.signer[b];
  const bool known = sg < a.K;
  if (!known) status_fail(a.status, b, ST_BAD_ARGUMENT);
  Aff<C> pt = aff_inf<C>();
  bool ok = true;
  if (y == 0) {
    const uint8_t* card = a.cards + (size_t)c * 2 * Geo<C>::PB;
    ok = wire_to_aff<C>(card, pt);
    if (a.c1 && b == (a.first ? a.first[c] : c * a.T)) {      // the card's first lane brings c1 along
      Aff<C> q;
      if (!wire_to_aff<C>(card + Geo<C>::PB, q)) {
        a.cstat[c] = ST_BAD_ENCODING;
        q = aff_inf<C>();
      }
      st_aff<C>(a.c1 + (size_t)c * Geo<C>::PW, q);
    }
  } else if (y == 1) {
    pt = ld_aff<C>(a.fbpts + (size_t)a.g_base * Geo<C>::PW);
    uint32_t* fw = reinterpret_cast<uint32_t*>(a.fs_init + (size_t)b * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) fw[i] = a.fs_seed[i];
  } else if (y == 2) {
    if (a.tokens) {
      ok = wire_to_aff<C>(a.tokens + (size_t)b * Geo<C>::PB, pt);
    } else {
      Fe<R> x = fe_zero<R>();
      if (known && !wire_to_fe<R>(a.sks + (size_t)sg * 32, x)) {
        ok = false;
        x = fe_zero<R>();
      }
      st_fe<R>(a.S + s_off(a.l.x, a.Bpad, b), x);
    }
  } else if (known) {
    ok = wire_to_aff<C>(a.keys + (size_t)sg * Geo<C>::PB, pt);
  }
  if (!ok && known) status_fail(a.status, b, ST_BAD_ENCODING);
  if (!ok || !known) pt = aff_inf<C>();
  const uint32_t slot = y < 2 ? a.l.g + y : a.l.a + (y - 2);
  st_aff<C>(a.P + p_off<C>(slot, a.Bpad, b), pt);
}
MP_KERNEL(k_open_stmt, OpenStmtArgs, body_open_stmt)

struct UnmaskSumArgs {
  const uint32_t* P;        // tokens: slot a_0 of the lanes
  const int32_t* status;    // [Bpad]: the lanes' verdicts
  const uint32_t* signer;   // [B]
  const uint32_t* c1;       // [C] affine
  const int32_t* cstat;     // [C]
  uint32_t* sumJ;           // [C] Jacobian: c1 - sum of the card's tokens, the identity for a card that is not opened
  int32_t* token_status;    // [B] out
  int32_t* card_status;     // [C] out
  uint32_t Bpad, K, T, a_slot;
  const uint32_t* first;    // [C + 1] offsets (then T is not read), or nullptr: the card's lanes are c * T .. c * T + T - 1
};
// One lane per card.  Folds the lanes' status words into the card's (the first that is not 0, in lane order: the reference stops at the
// first bad token) and, for a card whose tokens all verified, subtracts them from c1.  Every addition is the complete mixed addition
// of curve.hpp: tokens at infinity, two equal tokens (a doubling), tokens that cancel, c1 = O and a sum that is c1 all take its
// rare branches.
template <class C>
MP_HD void body_unmask_sum(const UnmaskSumArgs& a, uint32_t c, uint32_t y) {
  const int32_t cs = a.cstat[c];
  const uint32_t b0 = a.first ? a.first[c] : c * a.T, b1 = a.first ? a.first[c + 1] : b0 + a.T;
  int32_t first = 0;
  for (uint32_t b = b0; b < b1; ++b) {
    int32_t st = a.status[b];
    if (a.signer[b] >= a.K)
      st = ST_BAD_ARGUMENT;
    else if (cs < 0 && st >= 0)
      st = cs;                      // a bad c1 spoils every token of its card, as a bad c0 does
    a.token_status[b] = st;
    if (first == 0) first = st;
  }
  Jac<C> acc = jac_inf<C>();
  if (first == 0) {
    acc = jac_from_aff<C>(ld_aff<C>(a.c1 + (size_t)c * Geo<C>::PW));
#pragma unroll 1
    for (uint32_t b = b0; b < b1; ++b) jac_madd_ip<C>(acc, aff_neg<C>(ld_aff<C>(a.P + p_off<C>(a.a_slot, a.Bpad, b))));
  }
  st_jac<C>(a.sumJ + (size_t)c * Geo<C>::JW, acc);
  a.card_status[c] = first;
}
MP_KERNEL_OCC(k_unmask_sum, UnmaskSumArgs, body_unmask_sum, 2)

struct CardMatchArgs {
  const uint32_t* sumP;       // [C] affine plaintexts
  const int32_t* card_status; // [C]
  const uint8_t* plain;       // [n_plain] wire points, validated by the host
  uint8_t* out_plain;         // [C] wire points
  uint32_t* out_index;        // [C]
  uint32_t n_plain;
};
// One lane per card: the plaintext as a canonical wire point and the smallest index at which the list holds the same bytes.  A
// linear scan: the list is the 52 cards of a deck (4 096 at the most), every lane reads the same entry at the same time, and an
// entry is given up at its first differing word.
template <class C>
MP_HD void body_card_match(const CardMatchArgs& a, uint32_t c, uint32_t y) {
  typedef typename C::FqP F;
  constexpr uint32_t FW = Geo<C>::FW, WW = 2 * FW;
  const Aff<C> p = ld_aff<C>(a.sumP + (size_t)c * Geo<C>::PW);
  uint32_t w[WW];
  fe_to_canonical<F>(p.x, w);      // (0, 0) = the infinity encoding
  fe_to_canonical<F>(p.y, w + FW);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.out_plain + (size_t)c * Geo<C>::PB);
#pragma unroll
  for (uint32_t i = 0; i < WW; ++i) dst[i] = w[i];
  uint32_t idx = OPEN_NO_INDEX;
  if (a.card_status[c] == 0) {
    for (uint32_t i = 0; i < a.n_plain; ++i) {
      const uint32_t* e = reinterpret_cast<const uint32_t*>(a.plain + (size_t)i * Geo<C>::PB);
      if (e[0] != w[0]) continue;
      uint32_t diff = 0;
#pragma unroll
      for (uint32_t k = 1; k < WW; ++k) diff |= e[k] ^ w[k];
      if (diff == 0) {
        idx = i;
        break;
      }
    }
  }
  a.out_index[c] = idx;
}
MP_KERNEL(k_card_match, CardMatchArgs, body_card_match)

}  // namespace mp
