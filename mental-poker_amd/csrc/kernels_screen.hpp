// Screening of sigma-proof batches (engine_core.hpp screen_sigma): the checks z g_i - c a_i - A_i = O of the lanes of a GROUP -- g
// consecutive lanes, the last group of a call may be short -- added up with one weight per check into ONE equation on the bucket
// pipeline; only the lanes of a group whose equation fails go through the per-proof phase (k_sigma_verdict).  The third client of the
// equation machinery of kernels_proto.hpp after chains and groups of shuffle proofs.  What differs from those: a group's lanes are
// CONSECUTIVE (lane t g + j: sigma batches have arbitrary, also prime, sizes -- no divisor of B to pick), the weights come in `nw` per
// lane (one per check), and the transcript of a sigma proof does not absorb the response, so the lane digest below does.
// Short, memory-shaped kernels: one lane per item, nothing held across a loop iteration but an accumulator.
#pragma once
#include "kernels_sigma.hpp"

namespace mp {

// (1) lane digest = Blake2s(Fiat-Shamir state after k_sigma_fs || canonical z): the state covers bases, publics and commitments, the
//     response is hashed in here -- a weight is then a function of every byte of every proof of its group.  Written where
//     k_chain_digest / k_chain_weights look for the seed of "link" j nw + i of "table" t (the same digest for the nw checks of a lane:
//     the stream position tells the weights apart); the lanes past the end of the call (short last group) hash as zeros.
struct ScreenDigestArgs {
  const uint32_t* seed;    // [8][Bpad]
  const uint32_t* S;
  uint32_t* out;           // [8][SB], SB >= g nw T
  uint32_t Bpad, SB, B, g, T, nw, s_z;
};
// x = t g + j
template <class C>
MP_HD void body_screen_digest(const ScreenDigestArgs& a, uint32_t x, uint32_t) {
  typedef typename C::FrP R;
  const uint32_t t = x / a.g, j = x % a.g;
  uint32_t h[8];
  if (x < a.B) {
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 8; ++w) m[w] = a.seed[(size_t)w * a.Bpad + x];
    fe_to_canonical<R>(ld_fe<R>(a.S + s_off(a.s_z, a.Bpad, x)), m + 8);
    Blake2sState st;
    blake2s_init(st);
    blake2s_compress(st, m, 64ull, true);
#pragma unroll
    for (int w = 0; w < 8; ++w) h[w] = st.h[w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; ++w) h[w] = 0u;
  }
  for (uint32_t i = 0; i < a.nw; ++i)
#pragma unroll
    for (int w = 0; w < 8; ++w) a.out[(size_t)w * a.SB + (size_t)(j * a.nw + i) * a.T + t] = h[w];
}
MP_KERNEL(k_screen_digest, ScreenDigestArgs, body_screen_digest)

// (2) scalars of the group equation: CS[y][t] = sum_k rho_{(j0 + k) nw + i} S[s][lane t g + j0 + k].  A variable term is one point of
//     one lane (cnt = 1); the table's G collects the responses of up to 64 lanes (p = NO_SLOT).  A lane past the end of the call adds
//     nothing, and a term whose point is the identity gets the scalar 0: every digit zero, the bucket kernels never touch the point.
struct ScreenTerm {
  uint32_t s, p, j0, cnt, i;
};
struct ScreenScalArgs {
  const uint32_t* S;
  const uint32_t* P;
  const uint32_t* CW;      // [g nw][Tpad] Fr
  uint32_t* CS;            // [terms][Tpad] Fr
  const ScreenTerm* terms;
  uint32_t Bpad, Tpad, B, g, nw;
};
template <class C>
MP_HD bool screen_point_is_identity(const uint32_t* p) {
  uint32_t w[Geo<C>::PW];
  ld_words<Geo<C>::PW>(p, w);
  uint32_t d = 0;
#pragma unroll
  for (uint32_t i = 0; i < Geo<C>::PW; ++i) d |= w[i];
  return d == 0;
}
// x = group, y = term
template <class C>
MP_HD void body_screen_scalars(const ScreenScalArgs& a, uint32_t t, uint32_t y) {
  typedef typename C::FrP R;
  const ScreenTerm ct = a.terms[y];
  Fe<R> acc = fe_zero<R>();
  for (uint32_t k = 0; k < ct.cnt; ++k) {
    const uint32_t j = ct.j0 + k;
    const uint64_t b = (uint64_t)t * a.g + j;
    if (b >= a.B) break;
    if (ct.p != NO_SLOT && screen_point_is_identity<C>(a.P + p_off<C>(ct.p, a.Bpad, (uint32_t)b))) continue;
    acc = fe_add<R>(acc, fe_mul<R>(ld_fe<R>(a.CW + ((size_t)(j * a.nw + ct.i) * a.Tpad + t) * 8), ld_fe<R>(a.S + s_off(ct.s, a.Bpad, (uint32_t)b))));
  }
  st_fe<R>(a.CS + ((size_t)y * a.Tpad + t) * 8, acc);
}
MP_KERNEL(k_screen_scalars, ScreenScalArgs, body_screen_scalars)

// (3) the points of a group as one contiguous run (the role of k_group_tile): entry j per + y of run t = P slot pslot[y] of lane
//     t g + j; the identity for the lanes past the end of the call.  x = t g + j, y = point of the lane
struct ScreenTileArgs {
  const uint32_t* P;
  uint32_t* tile;          // [T][K][PW], K = g per
  uint32_t pslot[8];
  uint32_t Bpad, B, g, per;
};
template <class C>
MP_HD void body_screen_tile(const ScreenTileArgs& a, uint32_t x, uint32_t y) {
  uint32_t w[Geo<C>::PW];
  if (x < a.B) {
    ld_words<Geo<C>::PW>(a.P + p_off<C>(a.pslot[y], a.Bpad, x), w);
  } else {
#pragma unroll
    for (uint32_t i = 0; i < Geo<C>::PW; ++i) w[i] = 0u;
  }
  st_words<Geo<C>::PW>(a.tile + ((size_t)x * a.per + y) * Geo<C>::PW, w);
}
MP_KERNEL(k_screen_tile, ScreenTileArgs, body_screen_tile)

// (4) verdicts: k_screen_check -- x = lane: a lane whose status word is set already sends its group to the per-proof phase;
//     k_screen_verdict -- x = group: its equation's value and part[t] give gbad[t] and the flag; k_screen_mark -- x = lane: the lanes of
//     a failing group read MP_ERR_INTERNAL until the per-proof phase has given each its own word, never "accepted".
struct ScreenVerdictArgs {
  const uint32_t* J;       // the equations' arena: J slot 0 of lane t = value of equation t
  int32_t* status;         // [B] the lanes' status words
  uint32_t* part;          // [T] zero at launch
  uint32_t* gbad;          // [T]
  uint32_t* flag;
  uint32_t JBpad, B, g;
};
template <class C>
MP_HD void body_screen_check(const ScreenVerdictArgs& a, uint32_t b, uint32_t) {
  if (a.status[b] != 0) a.part[b / a.g] = 1u;      // (the same value from every lane that writes: no atomic needed)
}
MP_KERNEL(k_screen_check, ScreenVerdictArgs, body_screen_check)
template <class C>
MP_HD void body_screen_verdict(const ScreenVerdictArgs& a, uint32_t t, uint32_t) {
  const bool bad = a.part[t] != 0 || !fe_is_zero(ld_fe<typename C::FqP>(a.J + j_off<C>(0, a.JBpad, t) + 2 * Geo<C>::FW));
  a.gbad[t] = bad ? 1u : 0u;
  if (bad) a.flag[0] = 1u;
}
MP_KERNEL(k_screen_verdict, ScreenVerdictArgs, body_screen_verdict)
template <class C>
MP_HD void body_screen_mark(const ScreenVerdictArgs& a, uint32_t b, uint32_t) {
  if (a.gbad[b / a.g] && a.status[b] == 0) a.status[b] = -5;
}
MP_KERNEL(k_screen_mark, ScreenVerdictArgs, body_screen_mark)

// (5) compaction: the lanes of the failing groups, idx[i] in call order, copied into lanes 0 .. n - 1 of a workspace of their own -- what
//     the verifier's phase reads: P slots [0, nP), S slots [0, nS), the status word (a mark of k_screen_mark is taken off again) -- so
//     that the per-proof phase runs over n lanes instead of B; k_scatter_status brings the words back.  x = i, y = slot
struct ScreenGatherArgs {
  const uint32_t *P, *S;
  const int32_t* status;
  uint32_t *dP, *dS;
  int32_t* dstatus;
  const uint32_t* idx;
  uint32_t Bpad, dBpad, nP, nS;
};
template <class C>
MP_HD void body_screen_gather(const ScreenGatherArgs& a, uint32_t i, uint32_t y) {
  const uint32_t b = a.idx[i];
  if (y < a.nP) {
    uint32_t w[Geo<C>::PW];
    ld_words<Geo<C>::PW>(a.P + p_off<C>(y, a.Bpad, b), w);
    st_words<Geo<C>::PW>(a.dP + p_off<C>(y, a.dBpad, i), w);
  } else if (y < a.nP + a.nS) {
    uint32_t w[8];
    ld_words<8>(a.S + s_off(y - a.nP, a.Bpad, b), w);
    st_words<8>(a.dS + s_off(y - a.nP, a.dBpad, i), w);
  } else {
    const int32_t st = a.status[b];
    a.dstatus[i] = st == -5 ? 0 : st;
  }
}
MP_KERNEL(k_screen_gather, ScreenGatherArgs, body_screen_gather)

}  // namespace mp
