// Probe library: runs ONE field operation or ONE group operation of the engine's headers per lane and hands the results back as
// canonical integers, so that tests/test_gpu_primitives.py (gfx950) and tests/test_primitives_emu.py (development emulator) can compare
// every primitive with Python integers (tests/prim_cases.py).  A separate shared object: nothing here is linked into libmpshuffle.so.
//
//   gfx950:    hipcc <the library's flags> [-DPRIM_CURVE=k] -I mental-poker_amd/csrc -c tools/primcheck/prim_check.hip   (_native.build():
//              one object per curve, linked into tools/primcheck/libprimcheck.so)
//   emulator:  g++ -O2 -std=c++17 -fPIC -fopenmp -shared -x c++ -include tools/hostemu/rt.hpp -Itools/hostemu -Imental-poker_amd/csrc
//              tools/primcheck/prim_check.hip -o tools/primcheck/libprimcheck_emu.so
//
// Data format: a field element is NW little-endian 32-bit words holding the canonical integer (NOT Montgomery), NW = 8 (12: BLS12-377 Fq).
// Every lane handles one case, every kernel checks its index against the case count, no loop length comes from an input.
#include <cstdint>
#include <exception>
#include <string>

#include "curve.hpp"
#include "kernels_quad.hpp"
#include "rt.hpp"

using namespace mp;

namespace {

// ---- a value pushed away from its canonical representative: the same residue, anywhere in [0, 4p) / [0, 2p) ---------------------------
template <class F>
MP_HD Fe<F> lazy_rep(const Fe<F>& x, const Fe<F>& t, uint32_t mode) {
  switch (mode & 7u) {
    case 1: return fe_add<F>(x, fe_sub<F>(t, t));
    case 2: return fe_sub<F>(fe_add<F>(x, t), t);
    case 3: return fe_add<F>(fe_sub<F>(x, t), t);
    case 4: return fe_neg<F>(fe_neg<F>(x));
    case 5: return fe_sub<F>(fe_add<F>(fe_add<F>(x, t), t), fe_dbl<F>(t));
    case 6: return fe_add<F>(x, fe_add<F>(fe_sub<F>(t, t), fe_sub<F>(x, x)));
    case 7: return fe_sub<F>(fe_sub<F>(x, t), fe_neg<F>(t));
    default: return x;
  }
}
template <class F>
MP_HD void st_flags(uint32_t* o, uint32_t flags) {
#pragma unroll
  for (int i = 0; i < F::NW; ++i) o[i] = 0;
  o[0] = flags;
}

// ---- field operations ----------------------------------------------------------------------------------------------------------------
// in: 4 operands a, b, c, d per case; aux: four 3-bit lazy_rep modes; out: field_nout(family) elements per case
enum { FAM_MUL = 0, FAM_LIN = 1, FAM_COMB = 2, FAM_ZERO = 3, FAM_MISC = 4, FAM_INV = 5, FAM_COUNT = 6 };
constexpr uint32_t field_nout(int fam) { return fam == FAM_MUL ? 6u : fam == FAM_LIN ? 8u : fam == FAM_COMB ? 9u : fam == FAM_ZERO ? 1u : fam == FAM_MISC ? 5u : 4u; }

struct FieldArgs {
  const uint32_t* in;
  const uint32_t* aux;
  uint32_t* out;
  uint32_t n;
};
template <class F, int FAM>
struct FieldOp {
  typedef F Field;
  static constexpr int fam = FAM;
};
template <class T>
MP_HD void body_field(const FieldArgs& a, uint32_t x, uint32_t) {
  typedef typename T::Field F;
  constexpr int NW = F::NW, FAM = T::fam;
  constexpr uint32_t NOUT = field_nout(FAM);
  if (x >= a.n) return;
  const uint32_t* in = a.in + (size_t)x * 4 * NW;
  uint32_t* out = a.out + (size_t)x * NOUT * NW;
  const uint32_t mode = a.aux[x];
  const Fe<F> A = fe_from_canonical<F>(in), B = fe_from_canonical<F>(in + NW), C = fe_from_canonical<F>(in + 2 * NW),
              D = fe_from_canonical<F>(in + 3 * NW);
  const Fe<F> Al = lazy_rep<F>(A, D, mode), Bl = lazy_rep<F>(B, C, mode >> 3), Cl = lazy_rep<F>(C, A, mode >> 6),
              Dl = lazy_rep<F>(D, B, mode >> 9);
  auto st = [&](uint32_t k, const Fe<F>& v) { fe_to_canonical<F>(v, out + k * NW); };
  if constexpr (FAM == FAM_MUL) {
    st(0, fe_mul<F>(A, B));
    st(1, fe_sqr<F>(A));
    st(2, fe_mulsub<F>(A, B, C, D));
    st(3, fe_mul<F>(Al, Bl));
    st(4, fe_sqr<F>(Al));
    st(5, fe_mulsub<F>(Al, Bl, Cl, Dl));
  } else if constexpr (FAM == FAM_LIN) {
    st(0, fe_add<F>(A, B));
    st(1, fe_sub<F>(A, B));
    st(2, fe_neg<F>(A));
    st(3, fe_dbl<F>(A));
    st(4, fe_add<F>(Al, Bl));
    st(5, fe_sub<F>(Al, Bl));
    st(6, fe_neg<F>(Al));
    st(7, fe_dbl<F>(Al));
  } else if constexpr (FAM == FAM_COMB) {
    // the one-pass combinations take direct products, as curve.hpp uses them
    const Fe<F> P1 = fe_mul<F>(Al, Bl), P2 = fe_sqr<F>(Cl), P3 = fe_mulsub<F>(Al, Bl, Cl, Dl);
    const Fe<F> X3 = fe_sub_sub_dbl<F>(P2, P1, P3);
    st(0, X3);                                                        // p2 - p1 - 2 p3
    st(1, fe_sub_dbl<F>(P2, P1));                                     // p2 - 2 p1
    st(2, fe_triple_add<F>(P2, P3));                                  // 3 p2 + p3
    st(3, fe_mulsub<F>(Al, fe_sub_lazy<F>(Bl, Cl), Dl, P1));          // a (b - c) - d p1
    st(4, fe_mul<F>(fe_neg_lazy<F>(Bl), Al));                         // -a b
    const Fe<F> Wd = fe_sub_wide<F>(P1, Dl);                          // p1 - d, no weak reduction
    st(5, fe_mul<F>(Wd, Bl));
    st(6, fe_sqr<F>(Wd));
    uint32_t fl = 0;
    fl |= fe_is_zero(Wd) ? 1u : 0u;                                                                 // <=> p1 = d
    fl |= fe_is_zero(fe_sub_wide<F>(P1, fe_add<F>(P1, fe_sub<F>(Dl, Dl)))) ? 2u : 0u;                // always
    fl |= fe_is_zero(fe_sub_wide<F>(P2, fe_sqr<F>(fe_neg<F>(Cl)))) ? 4u : 0u;                        // always
    st_flags<F>(out + 7 * NW, fl);
    st(8, fe_mulsub<F>(Wd, fe_sub_lazy<F>(P2, X3), Dl, P1));          // (p1 - d)(p2 - x3) - d p1: the y coordinate of a mixed addition
  } else if constexpr (FAM == FAM_ZERO) {
    const Fe<F> Z1 = fe_sub<F>(Al, Al), Z2 = fe_add<F>(Al, fe_neg<F>(Al)), Z3 = fe_sub<F>(fe_add<F>(A, B), fe_add<F>(B, A));
    const Fe<F> Z4 = fe_add<F>(fe_add<F>(Z1, Z2), fe_add<F>(Z3, Z2));
    uint32_t fl = 0;
    fl |= fe_is_zero(A) ? 1u << 0 : 0u;                               // a = 0
    fl |= fe_is_zero(Al) ? 1u << 1 : 0u;                              // a = 0
    fl |= fe_eq<F>(A, B) ? 1u << 2 : 0u;                              // a = b
    fl |= fe_eq<F>(Al, Bl) ? 1u << 3 : 0u;                            // a = b
    fl |= fe_is_zero(Z1) ? 1u << 4 : 0u;                              // always (bits 4 .. 8, 11, 13, 14)
    fl |= fe_is_zero(Z2) ? 1u << 5 : 0u;
    fl |= fe_is_zero(Z3) ? 1u << 6 : 0u;
    fl |= fe_is_zero(Z4) ? 1u << 7 : 0u;
    fl |= fe_eq<F>(fe_add<F>(Al, Z4), Al) ? 1u << 8 : 0u;
    fl |= fe_is_zero(fe_sub<F>(Al, Bl)) ? 1u << 9 : 0u;               // a = b
    fl |= fe_is_zero(fe_add<F>(Al, Cl)) ? 1u << 10 : 0u;              // a + c = 0
    fl |= fe_is_zero(fe_dbl<F>(fe_dbl<F>(Z1))) ? 1u << 11 : 0u;
    fl |= fe_is_zero(fe_mul<F>(Al, Bl)) ? 1u << 12 : 0u;              // a b = 0
    fl |= fe_is_zero(fe_zero<F>()) ? 1u << 13 : 0u;
    fl |= fe_is_zero(fe_neg<F>(fe_zero<F>())) ? 1u << 14 : 0u;
    fl |= fe_eq<F>(fe_neg<F>(Al), Cl) ? 1u << 15 : 0u;                // a + c = 0
    st_flags<F>(out, fl);
  } else if constexpr (FAM == FAM_MISC) {
    uint32_t pk[NW], back[NW];
    fe_pack<F>(Al, pk);                                               // the memory format: canonical Montgomery residue a R mod p
#pragma unroll
    for (int i = 0; i < NW; ++i) out[i] = pk[i];
    st(1, fe_unpack<F>(pk));
    st(2, fe_from_u32<F>(in[0]));
    if constexpr (!F::L29) {
      st(3, fe_half<F>(A));
    } else {
      st_flags<F>(out + 3 * NW, 0);
    }
    fe_to_canonical<F>(A, back);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) diff |= back[i] ^ in[i];
    st_flags<F>(out + 4 * NW, (fe_canonical_in_range<F>(pk) ? 1u : 0u) | (diff == 0 ? 2u : 0u));
  } else {
    st(0, fe_inv<F>(A));
    st(1, fe_inv_divsteps<F>(Al));
    st(2, fe_inv_fermat<F>(A));
    st(3, fe_inv_fermat<F>(Al));
  }
}
MP_KERNEL(k_field, FieldArgs, body_field)

// ---- group law, one lane per case ---------------------------------------------------------------------------------------------------
// p, q: 4 elements per case -- (X, Y, ZZ, ZZZ), (X, Y, Z, -) or (x, y, -, -) as the operation reads them; aux: bit 0 = subtract (mixed
// addition), bits 4 .. 6 = lazy_rep mode of every coordinate; out: 4 elements per case
enum { OP_XYZZ_DBL = 0, OP_XYZZ_MADD = 1, OP_XYZZ_ADD = 2, OP_JAC_DBL = 3, OP_JAC_MADD = 4, OP_JAC_ADD = 5, OP_XYZZ_TO_JAC = 6,
       OP_AFF_ON_CURVE = 7, OP_DBL_CHAIN = 8, OP_MADD_RUN = 9, OP_COUNT = 10 };
constexpr int DBL_CHAIN_LEN = 250;      // the window fold of the bucket method (k_bucket_fold_q) doubles this often in a row
constexpr int MADD_RUN_LEN = 300;

struct GroupArgs {
  const uint32_t* p;
  const uint32_t* q;
  const uint32_t* aux;
  uint32_t* out;
  uint32_t n;
};
template <class C, int OP>
struct GroupOp {
  typedef C Curve;
  static constexpr int op = OP;
};
template <class C>
MP_HD void ld4(const uint32_t* w, uint32_t mode, Fe<typename C::FqP>* v) {
  typedef typename C::FqP F;
  Fe<F> c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = fe_from_canonical<F>(w + i * F::NW);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = lazy_rep<F>(c[i], c[(i + 1) & 3], mode);
}
template <class C>
MP_HD void st_xyzz(uint32_t* o, const Xyzz<C>& p) {
  typedef typename C::FqP F;
  fe_to_canonical<F>(p.X, o);
  fe_to_canonical<F>(p.Y, o + F::NW);
  fe_to_canonical<F>(p.ZZ, o + 2 * F::NW);
  fe_to_canonical<F>(p.ZZZ, o + 3 * F::NW);
}
template <class C>
MP_HD void st_jac3(uint32_t* o, const Jac<C>& p) {
  typedef typename C::FqP F;
  fe_to_canonical<F>(p.X, o);
  fe_to_canonical<F>(p.Y, o + F::NW);
  fe_to_canonical<F>(p.Z, o + 2 * F::NW);
  st_flags<F>(o + 3 * F::NW, 0);
}
template <class T>
MP_HD void body_group(const GroupArgs& a, uint32_t x, uint32_t) {
  typedef typename T::Curve C;
  typedef typename C::FqP F;
  constexpr int NW = F::NW, OP = T::op;
  if (x >= a.n) return;
  const uint32_t aux = a.aux[x], mode = (aux >> 4) & 7u;
  const bool neg = (aux & 1u) != 0;
  uint32_t* out = a.out + (size_t)x * 4 * NW;
  Fe<F> pv[4], qv[4];
  ld4<C>(a.p + (size_t)x * 4 * NW, mode, pv);
  ld4<C>(a.q + (size_t)x * 4 * NW, mode, qv);
  Xyzz<C> P, Q;
  P.X = pv[0]; P.Y = pv[1]; P.ZZ = pv[2]; P.ZZZ = pv[3];
  Q.X = qv[0]; Q.Y = qv[1]; Q.ZZ = qv[2]; Q.ZZZ = qv[3];
  Jac<C> PJ, QJ;
  PJ.X = pv[0]; PJ.Y = pv[1]; PJ.Z = pv[2];
  QJ.X = qv[0]; QJ.Y = qv[1]; QJ.Z = qv[2];
  Aff<C> qa;
  qa.x = qv[0]; qa.y = qv[1];
  if constexpr (OP == OP_XYZZ_DBL) {
    xyzz_dbl_ip<C>(P);
    st_xyzz<C>(out, P);
  } else if constexpr (OP == OP_XYZZ_MADD) {
    xyzz_madd_signed_ip<C>(P, qa, neg);
    st_xyzz<C>(out, P);
  } else if constexpr (OP == OP_XYZZ_ADD) {
    xyzz_add_ip<C>(P, Q);
    st_xyzz<C>(out, P);
  } else if constexpr (OP == OP_JAC_DBL) {
    jac_dbl_ip<C>(PJ);
    st_jac3<C>(out, PJ);
  } else if constexpr (OP == OP_JAC_MADD) {
    jac_madd_ip<C>(PJ, qa);
    st_jac3<C>(out, PJ);
  } else if constexpr (OP == OP_JAC_ADD) {
    jac_add_ip<C>(PJ, QJ);
    st_jac3<C>(out, PJ);
  } else if constexpr (OP == OP_XYZZ_TO_JAC) {
    st_jac3<C>(out, xyzz_to_jac<C>(P));
  } else if constexpr (OP == OP_AFF_ON_CURVE) {
    Aff<C> pa;
    pa.x = pv[0]; pa.y = pv[1];
    const uint32_t on = aff_on_curve<C>(pa) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) st_flags<F>(out + i * NW, i == 0 ? on : 0u);
  } else if constexpr (OP == OP_DBL_CHAIN) {
#pragma unroll 1
    for (int i = 0; i < DBL_CHAIN_LEN; ++i) xyzz_dbl_ip<C>(P);
    st_xyzz<C>(out, P);
  } else {
#pragma unroll 1
    for (int i = 0; i < MADD_RUN_LEN; ++i) xyzz_madd_signed_ip<C>(P, qa, neg);
    st_xyzz<C>(out, P);
  }
}
MP_KERNEL(k_group, GroupArgs, body_group)

// ---- group law on four lanes: quad k of wave w holds case 16 w + k; aux: bits 0 .. 1 = the quad's `on`, bits 4 .. 6 = lazy_rep mode;
// out: 4 elements per LANE (all four lanes of a quad must end with the same accumulator)
enum { QOP_DBL = 0, QOP_MADD = 1, QOP_ADD = 2, QOP_COUNT = 3 };
template <class T, class W>
MP_HD void body_quad(const GroupArgs& a, uint32_t wid, W& wv) {
  typedef typename T::Curve C;
  typedef typename C::FqP F;
  constexpr int NW = F::NW, OP = T::op;
  PerLane<Xyzz<C>> p, q;
  PerLane<Aff<C>> qa;
  PerLane<uint32_t> on;
  wv.lanes([&](uint32_t l) {
    const uint32_t item = wid * 16u + (l >> 2);
    on[l] = 0;
    p[l] = xyzz_inf<C>();
    q[l] = xyzz_inf<C>();
    qa[l] = aff_inf<C>();
    if (item >= a.n) return;
    const uint32_t aux = a.aux[item], mode = (aux >> 4) & 7u;
    Fe<F> pv[4], qv[4];
    ld4<C>(a.p + (size_t)item * 4 * NW, mode, pv);
    ld4<C>(a.q + (size_t)item * 4 * NW, mode, qv);
    p[l].X = pv[0]; p[l].Y = pv[1]; p[l].ZZ = pv[2]; p[l].ZZZ = pv[3];
    q[l].X = qv[0]; q[l].Y = qv[1]; q[l].ZZ = qv[2]; q[l].ZZZ = qv[3];
    qa[l].x = qv[0]; qa[l].y = qv[1];
    on[l] = aux & 3u;
  });
  if constexpr (OP == QOP_DBL) {
    xyzz_dbl_quad<C>(wv, p, on);
  } else if constexpr (OP == QOP_MADD) {
    xyzz_madd_quad<C>(wv, p, qa, on);
  } else {
    xyzz_add_quad<C>(wv, p, q, on);
  }
  wv.lanes([&](uint32_t l) {
    const uint32_t item = wid * 16u + (l >> 2);
    if (item >= a.n) return;
    st_xyzz<C>(a.out + ((size_t)item * 4 + (l & 3u)) * 4 * NW, p[l]);
  });
}
MP_WAVE_KERNEL(k_quad, GroupArgs, body_quad)

// ---- the wave helpers of rt.hpp (the emulator replaces them wholesale) -----------------------------------------------------------------
// wave: 64 words in, WAVE_NOUT words per lane out; block: 256 words in, BLOCK_NOUT words per lane out
constexpr uint32_t WAVE_NOUT = 18, BLOCK_NOUT = 2;
struct HelperArgs {
  const uint32_t* in;
  uint32_t* out;
  uint32_t n;      // waves / blocks
};
struct Pair {
  uint32_t a, b;
};
template <class C, class W>
MP_HD void body_wave_helpers(const HelperArgs& a, uint32_t wid, W& wv) {
  if (wid >= a.n) return;
  PerLane<uint32_t> x, scan, r1, r2, r3, b0, b1, b2, b3;
  PerLane<Pair> pr, q0, q1, q2, q3;
  wv.lanes([&](uint32_t l) {
    x[l] = a.in[(size_t)wid * 64 + l];
    scan[l] = x[l];
    r1[l] = x[l]; r2[l] = x[l]; r3[l] = x[l];
    pr[l].a = x[l];
    pr[l].b = ~x[l] + l;
  });
  wv.excl_scan(scan);
  const uint32_t mx = wv.max(x);
  const uint32_t any = wv.any(x) ? 1u : 0u;
  wv.template quad_rot<1>(r1);
  wv.template quad_rot<2>(r2);
  wv.template quad_rot<3>(r3);
  wv.template quad_bcast<0>(x, b0);
  wv.template quad_bcast<1>(x, b1);
  wv.template quad_bcast<2>(x, b2);
  wv.template quad_bcast<3>(x, b3);
  wv.lanes([&](uint32_t l) {
    q0[l] = wv.template quad_read<0>(pr, l);
    q1[l] = wv.template quad_read<1>(pr, l);
    q2[l] = wv.template quad_read<2>(pr, l);
    q3[l] = wv.template quad_read<3>(pr, l);
  });
  wv.lanes([&](uint32_t l) {
    uint32_t* o = a.out + ((size_t)wid * 64 + l) * WAVE_NOUT;
    o[0] = scan[l]; o[1] = mx; o[2] = any;
    o[3] = r1[l]; o[4] = r2[l]; o[5] = r3[l];
    o[6] = b0[l]; o[7] = b1[l]; o[8] = b2[l]; o[9] = b3[l];
    o[10] = q0[l].a; o[11] = q0[l].b; o[12] = q1[l].a; o[13] = q1[l].b;
    o[14] = q2[l].a; o[15] = q2[l].b; o[16] = q3[l].a; o[17] = q3[l].b;
  });
}
MP_WAVE_KERNEL(k_wave_helpers, HelperArgs, body_wave_helpers)

template <class C, class W>
MP_HD void body_block_helpers(const HelperArgs& a, uint32_t bid, W& wv) {
  typename W::template PL<uint32_t> x, scan;
  const bool live = bid < a.n;      // (every lane of the workgroup reaches the scans: no early return)
  wv.lanes([&](uint32_t l) {
    x[l] = live ? a.in[(size_t)bid * 256 + l] : 0u;
    scan[l] = x[l];
  });
  wv.excl_scan(scan);
  const uint32_t mx = wv.max(x);
  wv.lanes([&](uint32_t l) {
    if (!live) return;
    uint32_t* o = a.out + ((size_t)bid * 256 + l) * BLOCK_NOUT;
    o[0] = scan[l];
    o[1] = mx;
  });
}
MP_BLOCK_KERNEL_OCC(k_block_helpers, HelperArgs, body_block_helpers, 1)

// ---- host side ------------------------------------------------------------------------------------------------------------------------
std::string g_error;

struct DevBuf {
  void* p;
  explicit DevBuf(size_t bytes) : p(rt::dmalloc(bytes)) {}
  ~DevBuf() { rt::dfree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};
template <class Fn>
int guarded(Fn f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_error = e.what();
    return -1;
  }
}
const rt::Stream STREAM = rt::Stream();      // the default stream

template <class F, int FAM>
void run_field(uint32_t n, const uint32_t* in, const uint32_t* aux, uint32_t* out) {
  typedef FieldOp<F, FAM> T;
  const size_t in_b = (size_t)n * 4 * F::NW * 4, aux_b = (size_t)n * 4, out_b = (size_t)n * field_nout(FAM) * F::NW * 4;
  DevBuf d_in(in_b), d_aux(aux_b), d_out(out_b);
  rt::h2d(d_in.p, in, in_b, STREAM);
  rt::h2d(d_aux.p, aux, aux_b, STREAM);
  rt::dzero(d_out.p, out_b, STREAM);
  const FieldArgs a{(const uint32_t*)d_in.p, (const uint32_t*)d_aux.p, (uint32_t*)d_out.p, n};
  MP_LAUNCH(k_field, T, STREAM, n, 1, a);
  rt::d2h(out, d_out.p, out_b, STREAM);
  rt::stream_sync(STREAM);
}
template <class F>
int field_entry(int family, uint32_t n, const uint32_t* in, const uint32_t* aux, uint32_t* out) {
  return guarded([&] {
    switch (family) {
      case FAM_MUL: run_field<F, FAM_MUL>(n, in, aux, out); break;
      case FAM_LIN: run_field<F, FAM_LIN>(n, in, aux, out); break;
      case FAM_COMB: run_field<F, FAM_COMB>(n, in, aux, out); break;
      case FAM_ZERO: run_field<F, FAM_ZERO>(n, in, aux, out); break;
      case FAM_MISC: run_field<F, FAM_MISC>(n, in, aux, out); break;
      case FAM_INV: run_field<F, FAM_INV>(n, in, aux, out); break;
      default: throw std::runtime_error("prim_check: unknown field family");
    }
  });
}

template <class C, int OP, bool QUAD>
void run_group(uint32_t n, const uint32_t* p, const uint32_t* q, const uint32_t* aux, uint32_t* out) {
  typedef GroupOp<C, OP> T;
  constexpr int NW = C::FqP::NW;
  const size_t pt_b = (size_t)n * 4 * NW * 4, aux_b = (size_t)n * 4, out_b = pt_b * (QUAD ? 4 : 1);
  DevBuf d_p(pt_b), d_q(pt_b), d_aux(aux_b), d_out(out_b);
  rt::h2d(d_p.p, p, pt_b, STREAM);
  rt::h2d(d_q.p, q, pt_b, STREAM);
  rt::h2d(d_aux.p, aux, aux_b, STREAM);
  rt::dzero(d_out.p, out_b, STREAM);
  const GroupArgs a{(const uint32_t*)d_p.p, (const uint32_t*)d_q.p, (const uint32_t*)d_aux.p, (uint32_t*)d_out.p, n};
  if constexpr (QUAD) {
    const uint32_t nwaves = (n + 15u) / 16u;
    MP_WAVE_LAUNCH(k_quad, T, STREAM, nwaves, 0, a);
  } else {
    MP_LAUNCH(k_group, T, STREAM, n, 1, a);
  }
  rt::d2h(out, d_out.p, out_b, STREAM);
  rt::stream_sync(STREAM);
}
template <class C>
int group_entry(int op, uint32_t n, const uint32_t* p, const uint32_t* q, const uint32_t* aux, uint32_t* out) {
  return guarded([&] {
    switch (op) {
      case OP_XYZZ_DBL: run_group<C, OP_XYZZ_DBL, false>(n, p, q, aux, out); break;
      case OP_XYZZ_MADD: run_group<C, OP_XYZZ_MADD, false>(n, p, q, aux, out); break;
      case OP_XYZZ_ADD: run_group<C, OP_XYZZ_ADD, false>(n, p, q, aux, out); break;
      case OP_JAC_DBL: run_group<C, OP_JAC_DBL, false>(n, p, q, aux, out); break;
      case OP_JAC_MADD: run_group<C, OP_JAC_MADD, false>(n, p, q, aux, out); break;
      case OP_JAC_ADD: run_group<C, OP_JAC_ADD, false>(n, p, q, aux, out); break;
      case OP_XYZZ_TO_JAC: run_group<C, OP_XYZZ_TO_JAC, false>(n, p, q, aux, out); break;
      case OP_AFF_ON_CURVE: run_group<C, OP_AFF_ON_CURVE, false>(n, p, q, aux, out); break;
      case OP_DBL_CHAIN: run_group<C, OP_DBL_CHAIN, false>(n, p, q, aux, out); break;
      case OP_MADD_RUN: run_group<C, OP_MADD_RUN, false>(n, p, q, aux, out); break;
      default: throw std::runtime_error("prim_check: unknown group operation");
    }
  });
}
template <class C>
int quad_entry(int op, uint32_t n, const uint32_t* p, const uint32_t* q, const uint32_t* aux, uint32_t* out) {
  return guarded([&] {
    switch (op) {
      case QOP_DBL: run_group<C, QOP_DBL, true>(n, p, q, aux, out); break;
      case QOP_MADD: run_group<C, QOP_MADD, true>(n, p, q, aux, out); break;
      case QOP_ADD: run_group<C, QOP_ADD, true>(n, p, q, aux, out); break;
      default: throw std::runtime_error("prim_check: unknown four-lane operation");
    }
  });
}

}  // namespace

// one set of entry points per curve: pc_field_<curve>(fr, family, ...), pc_group_<curve>(op, ...), pc_quad_<curve>(op, ...),
// pc_error_<curve>(); 0 = done, -1 = see the error text.  PRIM_CURVE = k compiles curve k only (one object per curve).
#define PC_ENTRIES(NAME, CURVE)                                                                                                   \
  extern "C" int pc_field_##NAME(int fr, int family, uint32_t n, const uint32_t* in, const uint32_t* aux, uint32_t* out) {        \
    return fr ? field_entry<CURVE::FrP>(family, n, in, aux, out) : field_entry<CURVE::FqP>(family, n, in, aux, out);              \
  }                                                                                                                               \
  extern "C" int pc_group_##NAME(int op, uint32_t n, const uint32_t* p, const uint32_t* q, const uint32_t* aux, uint32_t* out) {  \
    return group_entry<CURVE>(op, n, p, q, aux, out);                                                                             \
  }                                                                                                                               \
  extern "C" int pc_quad_##NAME(int op, uint32_t n, const uint32_t* p, const uint32_t* q, const uint32_t* aux, uint32_t* out) {   \
    return quad_entry<CURVE>(op, n, p, q, aux, out);                                                                              \
  }                                                                                                                               \
  extern "C" const char* pc_error_##NAME() { return g_error.c_str(); }

#if !defined(PRIM_CURVE) || PRIM_CURVE == 0
PC_ENTRIES(stark, Stark)
extern "C" const char* pc_rt_name() { return MP_RT_NAME; }
extern "C" int pc_wave_helpers(uint32_t nwaves, const uint32_t* in, uint32_t* out) {
  return guarded([&] {
    const size_t in_b = (size_t)nwaves * 64 * 4, out_b = in_b * WAVE_NOUT;
    DevBuf d_in(in_b), d_out(out_b);
    rt::h2d(d_in.p, in, in_b, STREAM);
    rt::dzero(d_out.p, out_b, STREAM);
    const HelperArgs a{(const uint32_t*)d_in.p, (uint32_t*)d_out.p, nwaves};
    MP_WAVE_LAUNCH(k_wave_helpers, Stark, STREAM, nwaves, 0, a);
    rt::d2h(out, d_out.p, out_b, STREAM);
    rt::stream_sync(STREAM);
  });
}
extern "C" int pc_block_helpers(uint32_t nblocks, const uint32_t* in, uint32_t* out) {
  return guarded([&] {
    const size_t in_b = (size_t)nblocks * 256 * 4, out_b = in_b * BLOCK_NOUT;
    DevBuf d_in(in_b), d_out(out_b);
    rt::h2d(d_in.p, in, in_b, STREAM);
    rt::dzero(d_out.p, out_b, STREAM);
    const HelperArgs a{(const uint32_t*)d_in.p, (uint32_t*)d_out.p, nblocks};
    MP_BLOCK_LAUNCH(k_block_helpers, Stark, STREAM, nblocks, 0, a);
    rt::d2h(out, d_out.p, out_b, STREAM);
    rt::stream_sync(STREAM);
  });
}
#endif
#if !defined(PRIM_CURVE) || PRIM_CURVE == 1
PC_ENTRIES(bn254, Bn254)
#endif
#if !defined(PRIM_CURVE) || PRIM_CURVE == 2
PC_ENTRIES(secp256k1, Secp256k1)
#endif
#if !defined(PRIM_CURVE) || PRIM_CURVE == 3
PC_ENTRIES(bls12_377, Bls12_377)
#endif
