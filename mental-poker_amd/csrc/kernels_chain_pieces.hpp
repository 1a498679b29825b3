// kernels_chain_pieces.hpp -- chains of different lengths (mp_verify_shuffle_chain_ragged[_dev], capi.hip): the regrouping of the caller's
// table-major arrays into the link-major staging of one PASS, and the way back of the status words.
//
// A piece is (table t, first link a, length l): the l + 1 decks of links a .. a + l - 1 of table t are ONE contiguous run of the caller's
// decks array, from deck row off(t) + t + a on, and its l proofs and keys one contiguous run from row off(t) + a on (off(t) = the links of
// the tables in front of t).  A pass holds the G pieces of one length l in (t, a) order and is verified as a uniform call of G tables x
// l links (mp_verify_shuffle_chain_dev), whose arrays are link-major: row j of piece g lies at row j * G + g of the staging.
//
// All a kernel is told about a piece are its two source rows (64-bit: a call may hold 2^31 - 1 links, and a deck row of 52 cards is
// 6 656 bytes); every other row follows from them by arithmetic -- no index word per row, as for the other ragged calls (DESIGN.md
// "Ragged calls").  No LDS, no atomics; every lane moves one 16-byte word or one status word.
#pragma once
#include "rt.hpp"

namespace mp {

// 16-byte words a gather launch covers along x; the rest of a large pass goes along y (x + y * CP_X_SPAN)
static const uint32_t CP_X_SPAN = 1u << 30;

// One pass: decks, proofs and, if present, keys in one launch.  The 16-byte words of the staging are numbered section by section -- the
// (l + 1) G deck rows of dw words each, then the l G proof rows of pw words, then the l G key rows of kw words -- so consecutive lanes
// take consecutive words of one row, in the source as in the staging.  Word X of a section: staging row r = X / width = j * G + g,
// source row = the piece's first row + j.
struct ChainPieceGatherArgs {
  const uint64_t* desc;      // [G][2]: first deck row, first proof row of piece g in the caller's arrays
  const uint4* decks;        // the caller's arrays, table-major
  const uint4* proofs;
  const uint4* keys;         // nullptr: no keys (kw is 0 then)
  uint4* sdecks;             // the staging of the pass, link-major
  uint4* sproofs;
  uint4* skeys;
  uint64_t wd, wp, wk;       // 16-byte words of the three sections: (l + 1) G dw, l G pw, l G kw
  uint32_t G, dw, pw, kw;    // pieces of the pass; 16-byte words of a deck, a proof and a key row
};
// X / w and X % w for a word number below 2^46 and a row width below 2^32: in 32 bits whenever X fits them (every pass of less than 64 GB)
MP_HD void cp_divmod(uint64_t X, uint32_t w, uint64_t& q, uint32_t& r) {
  if ((X >> 32) == 0) {
    const uint32_t x = (uint32_t)X;
    q = x / w;
    r = x % w;
  } else {
    q = X / w;
    r = (uint32_t)(X % w);
  }
}
MP_HD void cp_move(const uint64_t* desc, uint32_t which, const uint4* src, uint4* dst, uint64_t X, uint32_t w, uint32_t G) {
  uint64_t row;
  uint32_t c, g;
  cp_divmod(X, w, row, c);
  uint64_t j;
  cp_divmod(row, G, j, g);
  dst[row * w + c] = src[(desc[2 * (size_t)g + which] + j) * w + c];
}
template <class C>
MP_HD void body_chain_piece_gather(const ChainPieceGatherArgs& a, uint32_t x, uint32_t y) {
  uint64_t X = (uint64_t)y * CP_X_SPAN + x;
  if (X < a.wd) {
    cp_move(a.desc, 0, a.decks, a.sdecks, X, a.dw, a.G);
    return;
  }
  X -= a.wd;
  if (X < a.wp) {
    cp_move(a.desc, 1, a.proofs, a.sproofs, X, a.pw, a.G);
    return;
  }
  X -= a.wp;
  if (X < a.wk) cp_move(a.desc, 1, a.keys, a.skeys, X, a.kw, a.G);
}
MP_KERNEL(k_chain_piece_gather, ChainPieceGatherArgs, body_chain_piece_gather)

// The way back, ONCE per call, after every pass has been enqueued: the words of all passes lie back to back in `words`, pass p from word
// pass[3 p] on as [l][G]; lane x takes word x, finds its pass (the first words are increasing: at most 12 steps for 4 095 passes), its
// link j and piece g there, and writes status[first proof row of the piece + j].
struct ChainPieceScatterArgs {
  const uint64_t* desc;      // [pieces][2], the passes back to back
  const uint64_t* pass;      // [passes][3]: first word, first piece, pieces of pass p
  const int32_t* words;
  int32_t* status;           // the caller's words, table-major
  uint32_t passes;
};
template <class C>
MP_HD void body_chain_piece_scatter(const ChainPieceScatterArgs& a, uint32_t x, uint32_t y) {
  uint32_t lo = 0, hi = a.passes;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.pass[3 * (size_t)mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t* p = a.pass + 3 * (size_t)lo;
  const uint32_t r = x - (uint32_t)p[0], G = (uint32_t)p[2];
  const uint32_t j = r / G, g = r % G;
  a.status[a.desc[2 * ((size_t)p[1] + g) + 1] + j] = a.words[x];
}
MP_KERNEL(k_chain_piece_scatter, ChainPieceScatterArgs, body_chain_piece_scatter)

}  // namespace mp
