// Probe library of the scalar recodings: cuts ONE scalar per lane into the digits the group kernels index their tables and buckets with
// and hands the digits back as plain integers, so that tests/test_gpu_digit.py (gfx950) and tests/test_digit_emu.py (development
// emulator) can compare them, digit for digit, with a Python-integer statement of each recoding (tests/digit_cases.py).  A separate
// shared object: nothing here is linked into libmpshuffle.so.
//
//   gfx950:    hipcc <the library's flags> -DDIGIT_CURVE=k -I mental-poker_amd/csrc -c tools/digitcheck/digit_check.hip   (_native.build():
//              one object per curve, linked into tools/digitcheck/libdigitcheck.so)
//   emulator:  g++ -O2 -std=c++17 -fPIC -fopenmp -shared -x c++ -include tools/hostemu/rt.hpp -Itools/hostemu -Imental-poker_amd/csrc
//              tools/digitcheck/digit_check.hip -o tools/digitcheck/libdigitcheck_emu.so
//
// The scalars arrive as wire bytes (32 little-endian bytes each) and go through the engine's own k_load_scalars (wire_to_fe + st_fe) into
// a one-slot S arena, so that every recoder reads them as the engine's do: ld_fe + fe_to_canonical.  Then
//   kind 0  fb_digit for the FbGeom of `width` (8, 16, 20, 21) bits, windows = ceil(R::BITS / width) as mp_table::init makes it;
//   kind 1  the engine's k_recode (body_recode): signed 5-bit Straus digits, nwin = vb_windows(R::BITS);
//   kind 2  the engine's k_bucket_recode (body_bucket_recode): signed `width`-bit digits of min(k, q - k), nwin = bk_windows(R::BITS, width).
// out: [n][stride] int32, digit w of scalar b at out[b * stride + w]; status: [n], what k_load_scalars reported; *nwin: the window count.
// Every kernel checks its index against the case count; every buffer size is derived on the host from the numbers the kernels index with.
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels_bucket.hpp"
#include "kernels_proto.hpp"
#include "layout.hpp"
#include "rt.hpp"

using namespace mp;

namespace {

std::string g_error;

struct DevBuf {
  void* p;
  size_t bytes;
  explicit DevBuf(size_t b) : p(rt::dmalloc(b)), bytes(b) {}
  ~DevBuf() { rt::dfree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  uint32_t* w() const { return (uint32_t*)p; }
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
void need(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(std::string("digit_check: ") + what);
}
const rt::Stream STREAM = rt::Stream();      // the default stream

enum { KIND_FIXED = 0, KIND_STRAUS = 1, KIND_BUCKET = 2 };

// ---- fixed-base digits: the scalar as k_fixed_msm / k_remask read it, every window through fb_digit ------------------------------------
struct FbDigArgs {
  const uint32_t* S;
  int32_t* out;      // [n][stride]
  uint32_t Bpad, n, stride;
  FbGeom g;
};
template <class C>
MP_HD void body_fb_digits(const FbDigArgs& a, uint32_t b, uint32_t) {
  typedef typename C::FrP R;
  if (b >= a.n) return;
  uint32_t k[8];
  fe_to_canonical<R>(ld_fe<R>(a.S + s_off(0, a.Bpad, b)), k);
  for (uint32_t w = 0; w < a.g.windows; ++w) a.out[(size_t)b * a.stride + w] = (int32_t)fb_digit(k, a.g, w);
}
MP_KERNEL(k_fb_digits, FbDigArgs, body_fb_digits)

template <class C>
void run_digits(int kind, uint32_t width, uint32_t n, const uint8_t* wire, uint32_t stride, int32_t* out, int32_t* status, uint32_t* nwin_out) {
  typedef typename C::FrP R;
  need(n > 0 && n < (1u << 24), "digits: 1 .. 2^24 - 1 scalars");
  uint32_t nwin = 0;
  if (kind == KIND_FIXED) {
    need(width == 8 || width == 16 || width == 20 || width == 21, "fixed-base windows are 8, 16, 20 or 21 bits wide");
    nwin = ((uint32_t)R::BITS + width - 1u) / width;
  } else if (kind == KIND_STRAUS) {
    need(width == (uint32_t)VB_WINDOW_BITS, "Straus windows are VB_WINDOW_BITS wide");
    nwin = (uint32_t)vb_windows(R::BITS);
  } else if (kind == KIND_BUCKET) {
    need(width >= BK_BITS_MIN && width <= BK_BITS_MAX, "bucket windows are BK_BITS_MIN .. BK_BITS_MAX bits wide");
    nwin = bk_windows(R::BITS, width);
  } else {
    need(false, "unknown kind");
  }
  need(nwin > 0 && nwin <= stride && stride <= 256, "digits: stride");
  *nwin_out = nwin;
  const uint32_t Bpad = (n + 63u) & ~63u;
  const size_t wire_b = (size_t)n * 32, S_b = (size_t)Bpad * 32, st_b = (size_t)n * 4, out_b = (size_t)n * stride * 4;
  DevBuf d_wire(wire_b), d_S(S_b), d_status(st_b);
  rt::h2d(d_wire.p, wire, wire_b, STREAM);
  rt::dzero(d_S.p, S_b, STREAM);
  rt::dzero(d_status.p, st_b, STREAM);
  const LoadScalarsArgs la{(const uint8_t*)d_wire.p, d_S.w(), (int32_t*)d_status.p, Bpad, 1u, 0u};
  MP_LAUNCH(k_load_scalars, C, STREAM, n, 1, la);
  rt::d2h(status, d_status.p, st_b, STREAM);
  for (size_t i = 0; i < (size_t)n * stride; ++i) out[i] = 0;
  if (kind == KIND_FIXED) {
    DevBuf d_out(out_b);
    rt::dzero(d_out.p, out_b, STREAM);
    const FbDigArgs a{d_S.w(), (int32_t*)d_out.p, Bpad, n, stride, FbGeom{width, nwin, (1u << width) - 1u}};
    MP_LAUNCH(k_fb_digits, C, STREAM, n, 1, a);
    rt::d2h(out, d_out.p, out_b, STREAM);
    rt::stream_sync(STREAM);
  } else if (kind == KIND_STRAUS) {
    const size_t D_b = (size_t)nwin * Bpad;                   // D[dslot 0][window][Bpad]
    DevBuf d_D(D_b), d_list(sizeof(Term));
    const Term one{0u, 0u};                                   // {S slot, digit slot}
    rt::h2d(d_list.p, &one, sizeof(Term), STREAM);
    rt::dzero(d_D.p, D_b, STREAM);
    const RecodeArgs a{d_S.w(), (int8_t*)d_D.p, (const Term*)d_list.p, Bpad, nwin};
    MP_LAUNCH(k_recode, C, STREAM, n, 1, a);
    std::vector<int8_t> h(D_b);
    rt::d2h(h.data(), d_D.p, D_b, STREAM);
    rt::stream_sync(STREAM);
    for (uint32_t b = 0; b < n; ++b)
      for (uint32_t w = 0; w < nwin; ++w) out[(size_t)b * stride + w] = h[(size_t)w * Bpad + b];
  } else {
    const size_t D_n = (size_t)n * nwin, D_b = D_n * 2;       // D16[b * dstride + pos + w * kpad] with dstride = nwin, pos = 0, kpad = 1
    DevBuf d_D(D_b), d_terms(sizeof(Term)), d_pos(sizeof(BTermPos));
    const Term one{0u, 0u};                                   // {S slot, P slot}
    const BTermPos pos{0u, 1u};
    rt::h2d(d_terms.p, &one, sizeof(Term), STREAM);
    rt::h2d(d_pos.p, &pos, sizeof(BTermPos), STREAM);
    rt::dzero(d_D.p, D_b, STREAM);
    const BRecodeArgs a{d_S.w(), (int16_t*)d_D.p, (const Term*)d_terms.p, (const BTermPos*)d_pos.p, Bpad, nwin, 1u, (size_t)nwin, width};
    MP_LAUNCH(k_bucket_recode, C, STREAM, n, 1, a);
    std::vector<int16_t> h(D_n);
    rt::d2h(h.data(), d_D.p, D_b, STREAM);
    rt::stream_sync(STREAM);
    for (uint32_t b = 0; b < n; ++b)
      for (uint32_t w = 0; w < nwin; ++w) out[(size_t)b * stride + w] = h[(size_t)b * nwin + w];
  }
}

}  // namespace

// one set of entry points per curve; 0 = done, -1 = see dc_error_<curve>().  DIGIT_CURVE = k compiles curve k only (one object per curve).
#define DC_ENTRIES(NAME, CURVE)                                                                                                       \
  extern "C" int dc_digits_##NAME(int kind, uint32_t width, uint32_t n, const uint8_t* wire, uint32_t stride, int32_t* out,           \
                                  int32_t* status, uint32_t* nwin) {                                                                  \
    return guarded([&] { run_digits<CURVE>(kind, width, n, wire, stride, out, status, nwin); });                                      \
  }                                                                                                                                   \
  extern "C" uint32_t dc_scalar_bits_##NAME() { return (uint32_t)CURVE::FrP::BITS; }                                                  \
  extern "C" const char* dc_error_##NAME() { return g_error.c_str(); }

#if !defined(DIGIT_CURVE) || DIGIT_CURVE == 0
DC_ENTRIES(stark, Stark)
extern "C" const char* dc_rt_name() { return MP_RT_NAME; }
#endif
#if !defined(DIGIT_CURVE) || DIGIT_CURVE == 1
DC_ENTRIES(bn254, Bn254)
#endif
#if !defined(DIGIT_CURVE) || DIGIT_CURVE == 2
DC_ENTRIES(secp256k1, Secp256k1)
#endif
#if !defined(DIGIT_CURVE) || DIGIT_CURVE == 3
DC_ENTRIES(bls12_377, Bls12_377)
#endif
