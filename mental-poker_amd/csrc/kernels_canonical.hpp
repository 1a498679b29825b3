// kernels_canonical.hpp -- the conversions between wire v1 and arkworks-canonical bytes that kernels_decompress.hpp leaves to the host,
// ON THE DEVICE: wire -> canonical for points, decks and shuffle proofs (compression), canonical -> wire for shuffle proofs.
//
// A caller of the trait holds decks, shuffled decks and proofs as canonical bytes [REF barnett-smart-card-protocol/src/lib.rs:45-71].
// k_decompress covers uniform runs of points (single points, decks); a proof is 27 groups of points and scalars, 11 of them a Vec with
// its u64 length in front, so its elements are found through a small table per (m, n) (capi.hip: proof_schema):
//   tab[3 e + 0]  byte offset of element e in the canonical proof
//   tab[3 e + 1]  byte offset of element e in the wire proof
//   tab[3 e + 2]  the Vec length that stands in the 8 bytes in front of the element's canonical bytes, 0 if none does
// `np` point entries first, then `ns` scalar entries.  Points and scalars run as launches of their own: the point lanes of a wave all
// walk the square root (fe_sqrt_windowed, with the context's tables and scratch chain), the scalar lanes only compare and copy.
//
// Compression (k_compress) is one lane per point with no field multiplication: range check, p - y by limb subtraction, compare --
// Ser<C>::compress_one on the device -- and CB bytes out; decks and proofs are framed by addressing, and the lane of a group's first
// element writes the length.  Without a table the kernel addresses uniform groups the way k_decompress does (per_group, prefix).
// Verdicts are those of the host functions (serialize_host.hpp); unlike them every element is converted on its own, a refused one
// leaves zero bytes, and the unit it belongs to (point, deck, proof) reads -1.  Several lanes may write that same -1.
#pragma once
#include "kernels_decompress.hpp"

namespace mp {

// `n` bytes at any address <-> little-endian words (whole words where the address allows it: the 33-byte records of secp256k1 and
// whatever follows them in a proof are not aligned)
MP_HD void cn_load(const uint8_t* p, uint32_t* w, uint32_t n) {
  if (((size_t)p & 3u) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    for (uint32_t i = 0; i < (n >> 2); ++i) w[i] = q[i];
    for (uint32_t b = n & ~3u; b < n; ++b) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
  } else {
    for (uint32_t b = 0; b < n; ++b) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
  }
}
MP_HD void cn_store(uint8_t* p, const uint32_t* w, uint32_t n) {
  if (((size_t)p & 3u) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    for (uint32_t i = 0; i < (n >> 2); ++i) q[i] = w[i];
    for (uint32_t b = n & ~3u; b < n; ++b) p[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  } else {
    for (uint32_t b = 0; b < n; ++b) p[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  }
}
MP_HD uint64_t cn_load_u64(const uint8_t* p) {
  uint32_t w[2] = {0, 0};
  cn_load(p, w, 8);
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}
MP_HD void cn_store_u64(uint8_t* p, uint64_t v) {
  const uint32_t w[2] = {(uint32_t)v, (uint32_t)(v >> 32)};
  cn_store(p, w, 8);
}

struct CompressArgs {
  const uint8_t* in;         // wire: groups of `wire_stride` bytes
  uint8_t* out;              // canonical: groups of `canon_stride` bytes
  int32_t* status;           // one word per group: written only on failure (caller zeroes)
  const uint32_t* tab;       // element table of a group (above), or null: `per_group` points back to back behind `prefix` bytes
  uint32_t first;            // index of the launch's first element
  uint32_t per_group, prefix;
  uint32_t wire_stride, canon_stride;
};

// thread x = point index over all groups
template <class C>
MP_HD void body_compress(const CompressArgs& a, uint32_t lane, uint32_t) {
  typedef typename C::FqP F;
  constexpr uint32_t CB = (F::BITS + 2 + 7) / 8, PB = 8 * F::NW;
  const uint32_t idx = a.first + lane;
  const uint32_t grp = idx / a.per_group, j = idx - grp * a.per_group;
  uint32_t co = a.prefix + j * CB, wo = j * PB, vec = (a.prefix == 8 && j == 0) ? a.per_group / 2 : 0u;      // (a deck: 2 points per card)
  if (a.tab) {
    co = a.tab[3 * j];
    wo = a.tab[3 * j + 1];
    vec = a.tab[3 * j + 2];
  }
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.in + (size_t)grp * a.wire_stride + wo);
  uint8_t* dst = a.out + (size_t)grp * a.canon_stride + co;
  uint32_t xw[F::NW + 1], yw[F::NW];
  bool zero = true;
  for (uint32_t i = 0; i < F::NW; ++i) {
    xw[i] = src[i];
    yw[i] = src[F::NW + i];
    zero = zero && xw[i] == 0 && yw[i] == 0;
  }
  xw[F::NW] = 0;
  uint32_t flags = 0x40u;                                    // all-zero wire bytes: the point at infinity
  if (!zero) {
    if (fe_canonical_in_range<F>(xw) && fe_canonical_in_range<F>(yw)) {
      // y > p - y  <=>  2 y > p  (y < p), on canonical integers
      uint32_t ny[F::NW];
      uint64_t br = 0;
      for (uint32_t i = 0; i < F::NW; ++i) {
        const uint64_t t = (uint64_t)F::MOD[i] - yw[i] - br;
        ny[i] = (uint32_t)t;
        br = (t >> 32) & 1;
      }
      bool greater = false, differ = false;
      for (int i = F::NW - 1; i >= 0; --i)
        if (!differ && yw[i] != ny[i]) {
          differ = true;
          greater = yw[i] > ny[i];
        }
      flags = greater ? 0x80u : 0u;
    } else {
      a.status[grp] = -1;                                    // MP_ERR_BAD_ENCODING: a coordinate >= p leaves an all-zero slot
      flags = 0;
      for (uint32_t i = 0; i < F::NW; ++i) xw[i] = 0;
    }
  }
  xw[(CB - 1) >> 2] |= flags << (8 * ((CB - 1) & 3));
  cn_store(dst, xw, CB);
  if (vec) cn_store_u64(dst - 8, vec);
}
MP_KERNEL(k_compress, CompressArgs, body_compress)

// canonical -> wire for the points of proofs.  d: k_decompress's arguments (tables, scratch chain, launch window; in / out / status per
// proof, per_group = points of a proof); the element table replaces its per_group / prefix addressing
struct DecompressMapArgs {
  DecompressArgs d;
  const uint32_t* tab;
  uint32_t canon_stride, wire_stride;
};

// one compressed point at `src` -> canonical words of x and y; false (and nothing to rely on in xw / yw) if it is refused.  The
// decoding and validation of body_decompress, for a point at an arbitrary address
template <class C>
MP_HD bool decompress_point(const DecompressArgs& a, const uint8_t* src, uint32_t lane, uint32_t* xw, uint32_t* yw) {
  typedef typename C::FqP F;
  constexpr uint32_t CB = (F::BITS + 2 + 7) / 8;
  for (uint32_t i = 0; i <= F::NW; ++i) xw[i] = 0;
  for (uint32_t i = 0; i < F::NW; ++i) yw[i] = 0;
  cn_load(src, xw, CB);
  const uint32_t fl_word = (CB - 1) >> 2, fl_shift = 8 * ((CB - 1) & 3);
  const uint32_t flags = (xw[fl_word] >> fl_shift) & 0xC0u;
  xw[fl_word] &= ~(0xC0u << fl_shift);
  if (xw[F::NW] != 0) return false;                          // (33-byte secp256k1 encoding: the spare byte carries only flags)
  if (flags & 0x40u) {                                       // infinity: x = 0, sign flag clear -> all-zero wire point
    bool zero = (flags & 0x80u) == 0;
    for (uint32_t i = 0; i < F::NW; ++i) zero = zero && xw[i] == 0;
    return zero;
  }
  if (!fe_canonical_in_range<F>(xw)) return false;
  const Fe<F> x = fe_from_canonical<F>(xw);
  Fe<F> rhs = fe_add<F>(fe_mul<F>(fe_sqr<F>(x), x), fe_unpack<F>(C::B_MONT));
  if (C::A == 1) rhs = fe_add<F>(rhs, x);
  Fe<F> y = fe_zero<F>();
  bool ok = true;
  if (!fe_is_zero(rhs) && !fe_sqrt_windowed<F>(a, rhs, y, lane)) ok = false;
  uint32_t nyw[F::NW];
  fe_to_canonical<F>(y, yw);
  fe_to_canonical<F>(fe_neg<F>(y), nyw);
  bool greater = false, differ = false;
  for (int i = F::NW - 1; i >= 0; --i)
    if (!differ && yw[i] != nyw[i]) {
      differ = true;
      greater = yw[i] > nyw[i];
    }
  if (greater != ((flags & 0x80u) != 0))
    for (uint32_t i = 0; i < F::NW; ++i) yw[i] = nyw[i];
  if (ok && !Cofactor<C>::ONE) {
    Aff<C> p;
    p.x = x;
    p.y = fe_from_canonical<F>(yw);
    if (!aff_is_inf<C>(p) && !aff_in_subgroup_dev<C>(p)) ok = false;
  }
  return ok;
}

// thread x = point index over all proofs
template <class C>
MP_HD void body_decompress_map(const DecompressMapArgs& a, uint32_t lane, uint32_t) {
  typedef typename C::FqP F;
  const uint32_t idx = a.d.first + lane;
  const uint32_t grp = idx / a.d.per_group, j = idx - grp * a.d.per_group;
  const uint8_t* src = a.d.in + (size_t)grp * a.canon_stride + a.tab[3 * j];
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.d.out + (size_t)grp * a.wire_stride + a.tab[3 * j + 1]);
  const uint32_t vec = a.tab[3 * j + 2];
  if (vec && cn_load_u64(src - 8) != (uint64_t)vec) a.d.status[grp] = -1;      // a wrong length fails the proof; the element is still converted
  uint32_t xw[F::NW + 1], yw[F::NW];
  if (!decompress_point<C>(a.d, src, lane, xw, yw)) {
    a.d.status[grp] = -1;                                    // MP_ERR_BAD_ENCODING (same value from every failing lane)
    for (uint32_t i = 0; i < F::NW; ++i) xw[i] = yw[i] = 0;
  }
  for (uint32_t i = 0; i < F::NW; ++i) {
    dst[i] = xw[i];
    dst[F::NW + i] = yw[i];
  }
}
MP_KERNEL_OCC(k_decompress_map, DecompressMapArgs, body_decompress_map, Geo<C>::OCC3)

// the scalars of proofs, both directions: 32 bytes each, copied; canonical -> wire (de) refuses a scalar >= q and a wrong Vec length
struct ScalarMapArgs {
  const uint8_t* in;
  uint8_t* out;
  int32_t* status;           // one word per proof: written only on failure (caller zeroes)
  const uint32_t* tab;       // the scalar entries of the element table
  uint32_t first, per_group;
  uint32_t canon_stride, wire_stride;
  uint32_t de;
};
// thread x = scalar index over all proofs
template <class C>
MP_HD void body_scalar_map(const ScalarMapArgs& a, uint32_t lane, uint32_t) {
  const uint32_t idx = a.first + lane;
  const uint32_t grp = idx / a.per_group, j = idx - grp * a.per_group;
  const uint32_t co = a.tab[3 * j], wo = a.tab[3 * j + 1], vec = a.tab[3 * j + 2];
  const uint8_t* src = a.in + (size_t)grp * (a.de ? a.canon_stride : a.wire_stride) + (a.de ? co : wo);
  uint8_t* dst = a.out + (size_t)grp * (a.de ? a.wire_stride : a.canon_stride) + (a.de ? wo : co);
  uint32_t w[8];
  for (uint32_t i = 0; i < 8; ++i) w[i] = 0;
  cn_load(src, w, 32);
  if (a.de) {
    if (vec && cn_load_u64(src - 8) != (uint64_t)vec) a.status[grp] = -1;
    if (!fe_canonical_in_range<typename C::FrP>(w)) {
      a.status[grp] = -1;
      for (uint32_t i = 0; i < 8; ++i) w[i] = 0;
    }
  } else if (vec) {
    cn_store_u64(dst - 8, vec);
  }
  cn_store(dst, w, 32);
}
MP_KERNEL(k_scalar_map, ScalarMapArgs, body_scalar_map)

#define MP_CANONICAL_KERNELS(X, C)                      \
  MP_KERNEL_INST(X, k_compress, CompressArgs, C)        \
  MP_KERNEL_INST(X, k_decompress_map, DecompressMapArgs, C) \
  MP_KERNEL_INST(X, k_scalar_map, ScalarMapArgs, C)

}  // namespace mp
