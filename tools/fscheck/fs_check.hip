// Probe library of the device Fiat-Shamir layer: BLAKE2s over the staging buffer on one lane and on four, the four-lane absorb, the
// ChaCha20 block, `Fr::rand`, the two-level chain / group weights, the lane digests of the sigma screen and the weights of the merged
// equation -- each as ONE launch with one case per lane (per quad / proof for the wave kernels), results handed back as plain
// little-endian words, so that tests/test_gpu_fs.py (gfx950) and tests/test_fs_emu.py (development emulator) can compare them with
// hashlib and the Python oracle (tests/fs_cases.py).  A separate shared object: nothing here is linked into libmpshuffle.so.
//
//   gfx950:    hipcc <the library's flags> -DFS_CURVE=k -I mental-poker_amd/csrc -c tools/fscheck/fs_check.hip   (_native.build(): one object
//              per curve, linked into tools/fscheck/libfscheck.so)
//   emulator:  g++ -O2 -std=c++17 -fPIC -fopenmp -shared -x c++ -include tools/hostemu/rt.hpp -Itools/hostemu -Imental-poker_amd/csrc
//              tools/fscheck/fs_check.hip -o tools/fscheck/libfscheck_emu.so
//
// Scalars of the S arena come and go in the memory format (8 words, canonical Montgomery residue), seeds and digests as 8 words.
// Every kernel checks its index against the case count; every buffer size is derived on the host from the same numbers the kernels
// index with, and the entry points refuse shapes that would not fit.
#include <cstdint>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "hash.hpp"
#include "kernels_proto.hpp"
#include "kernels_screen.hpp"
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
  if (!ok) throw std::runtime_error(std::string("fs_check: ") + what);
}
const rt::Stream STREAM = rt::Stream();      // the default stream

// a device buffer filled with one word (the staging buffers start as 0xFFFFFFFF: the hashers' zero padding is under test)
void fill_words(DevBuf& d, uint32_t word) {
  std::vector<uint32_t> h(d.bytes / 4, word);
  rt::h2d(d.p, h.data(), d.bytes, STREAM);
  rt::stream_sync(STREAM);
}

#if !defined(FS_CURVE) || FS_CURVE == 0
// ---- BLAKE2s over the staging buffer ---------------------------------------------------------------------------------------------------
// case x: two messages, A then B, staged into the SAME buffer one after the other (B after A without clearing) and hashed.
// data: [n][2][maxlen] bytes; lens: [n][2]; pats: [n]; out: mode 0 [n][2][8], mode 1 [n][2][4][8] (every lane of the quad)
enum { PAT_BYTES = 0, PAT_POINT65 = 1, PAT_POINT97 = 2, PAT_WORDS_AFTER_BYTES = 3, PAT_PIECES = 4 };
constexpr uint32_t PIECE_WORDS = 9;      // word-aligned pieces of 36 bytes
struct B2Args {
  const uint8_t* data;
  const uint32_t* lens;
  const uint32_t* pats;
  uint32_t* stage;      // [maxwords][stride]
  uint32_t* out;
  uint32_t n, stride, maxlen;
};
MP_HD uint32_t ld_le32(const uint8_t* d) { return (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24); }
// bytes [from, to) of d through the writer's two entry points, mixed as the pattern says
MP_HD void put_range(StageWriter& w, const uint8_t* d, uint32_t from, uint32_t to, uint32_t pat) {
  uint32_t i = from;
  if (pat == PAT_POINT65 || pat == PAT_POINT97) {      // 2 NW words, then the flag byte: nb cycles through 1, 2, 3
    const uint32_t nwords = pat == PAT_POINT65 ? 16u : 24u;
    while (i < to) {
      uint32_t k = 0;
      for (; k < nwords && to - i >= 4; ++k, i += 4) stage_word(w, ld_le32(d + i));
      if (k < nwords) break;
      if (i < to) stage_byte(w, d[i++]);
    }
  } else if (pat == PAT_WORDS_AFTER_BYTES || pat == PAT_PIECES) {      // 1, 2 or 3 bytes, then words
    const uint32_t lead = 1 + (to - from) % 3;
    for (uint32_t k = 0; k < lead && i < to; ++k) stage_byte(w, d[i++]);
    for (; to - i >= 4; i += 4) stage_word(w, ld_le32(d + i));
  }
  while (i < to) stage_byte(w, d[i++]);
}
struct B2One {};
template <class T>
MP_HD void body_b2s(const B2Args& a, uint32_t x, uint32_t) {
  if (x >= a.n) return;
  for (uint32_t s = 0; s < 2; ++s) {
    const uint8_t* d = a.data + ((size_t)x * 2 + s) * a.maxlen;
    const uint32_t len = a.lens[2 * x + s], pat = a.pats[x];
    StageWriter w = stage_begin(a.stage, a.stride, x);
    if (pat == PAT_PIECES) {      // every piece through a writer of its own; the last one (possibly empty) goes to the hasher
      const uint32_t full = len / (4 * PIECE_WORDS);
      for (uint32_t k = 0; k < full; ++k) {
        StageWriter p = stage_begin_at(a.stage, a.stride, x, k * PIECE_WORDS);
        put_range(p, d, k * 4 * PIECE_WORDS, (k + 1) * 4 * PIECE_WORDS, pat);
        stage_flush(p);
      }
      w = stage_begin_at(a.stage, a.stride, x, full * PIECE_WORDS);
      put_range(w, d, full * 4 * PIECE_WORDS, len, pat);
    } else {
      put_range(w, d, 0, len, pat);
    }
    uint32_t h[8];
    blake2s_staged(w, h);
#pragma unroll
    for (int i = 0; i < 8; ++i) a.out[((size_t)x * 2 + s) * 8 + i] = h[i];
  }
}
MP_KERNEL(k_b2s, B2Args, body_b2s)
// four lanes: quad k of wave w holds case 16 w + k; the length is the wave's (blake2s_staged_quad: the same for every lane)
template <class T, class W>
MP_HD void body_b2s_quad(const B2Args& a, uint32_t wid, W& wv) {
  for (uint32_t s = 0; s < 2; ++s) {
    const uint32_t len = a.lens[2 * (wid * 16u) + s];
    PerLane<const uint32_t*> base;
    PerLane<B2sSeed> out;
    wv.lanes([&](uint32_t l) {
      const uint32_t x = wid * 16u + (l >> 2), j = l & 3u;
      base[l] = a.stage + x;
      const uint8_t* d = a.data + ((size_t)x * 2 + s) * a.maxlen;
      const uint32_t pat = a.pats[x];
      if (pat == PAT_PIECES) {      // the pieces go round the lanes of the quad, as fsq_absorb deals the groups of four points
        const uint32_t np = len / (4 * PIECE_WORDS) + 1;
        for (uint32_t k = j; k < np; k += 4) {
          StageWriter p = stage_begin_at(a.stage, a.stride, x, k * PIECE_WORDS);
          const uint32_t to = (k + 1) * 4 * PIECE_WORDS < len ? (k + 1) * 4 * PIECE_WORDS : len;
          put_range(p, d, k * 4 * PIECE_WORDS, to, pat);
          stage_flush(p);
        }
      } else if (j == 0) {
        StageWriter w = stage_begin(a.stage, a.stride, x);
        put_range(w, d, 0, len, pat);
        stage_flush(w);
      }
    });
    wv.sync_global();
    blake2s_staged_quad(wv, base, a.stride, len, out);
    wv.sync_global();
    wv.lanes([&](uint32_t l) {
      const uint32_t x = wid * 16u + (l >> 2), j = l & 3u;
#pragma unroll
      for (int i = 0; i < 8; ++i) a.out[(((size_t)x * 2 + s) * 4 + j) * 8 + i] = out[l].s[i];
    });
  }
}
MP_WAVE_KERNEL(k_b2s_quad, B2Args, body_b2s_quad)

// ---- ChaCha20 block: one (key, counter) per lane ---------------------------------------------------------------------------------------
struct ChaArgs {
  const uint32_t* keys;      // [n][8]
  const uint32_t* ctr;       // [n][2]: low, high
  uint32_t* out;             // [n][16]
  uint32_t n;
};
template <class T>
MP_HD void body_chacha(const ChaArgs& a, uint32_t x, uint32_t) {
  if (x >= a.n) return;
  uint32_t key[8], blk[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = a.keys[(size_t)x * 8 + i];
  chacha20_block(key, (uint64_t)a.ctr[2 * x] | ((uint64_t)a.ctr[2 * x + 1] << 32), blk);
#pragma unroll
  for (int i = 0; i < 16; ++i) a.out[(size_t)x * 16 + i] = blk[i];
}
MP_KERNEL(k_chacha, ChaArgs, body_chacha)
#endif

// ---- Fr::rand: per key, NEXT_N values of frstream_next, then (a fresh stream) TRY_N steps of frstream_try -----------------------------------
constexpr uint32_t NEXT_N = 48, TRY_N = 96;
struct FrsArgs {
  const uint32_t* keys;      // [n][8]
  uint32_t* next;            // [n][NEXT_N][8]
  uint32_t* flag;            // [n][TRY_N]
  uint32_t* val;             // [n][TRY_N][8]
  uint32_t n;
};
template <class C>
MP_HD void body_frstream(const FrsArgs& a, uint32_t x, uint32_t) {
  typedef typename C::FrP R;
  if (x >= a.n) return;
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = a.keys[(size_t)x * 8 + i];
  FrStream s;
  frstream_init(s, key);
  for (uint32_t k = 0; k < NEXT_N; ++k) st_fe<R>(a.next + ((size_t)x * NEXT_N + k) * 8, frstream_next<R>(s));
  frstream_init(s, key);
  for (uint32_t k = 0; k < TRY_N; ++k) {
    Fe<R> f;
    const bool ok = frstream_try<R>(s, f);
    a.flag[(size_t)x * TRY_N + k] = ok ? 1u : 0u;
    // (a rejected candidate is no field element: its raw words go out as they are)
#pragma unroll
    for (int i = 0; i < 8; ++i) a.val[((size_t)x * TRY_N + k) * 8 + i] = f.v[i];
  }
}
MP_KERNEL(k_frstream, FrsArgs, body_frstream)

// ---- fsq_absorb with synthetic points: a point is 2 NW words and a flag byte from the input array ---------------------------------------
struct AbsArgs {
  FsDev f;
  FsqGeom g;
  const uint32_t* pts;       // [B][npts][2 NW + 1]
  const uint32_t* tail;      // [B][tail_words]
  const uint32_t* seed_in;   // [B][8]
  uint32_t* seed_out;        // [B][2][8]: after one absorb, after a second absorb of the same message
  uint32_t npts, tail_words;
};
template <class C, class W>
MP_HD void body_absorb(const AbsArgs& a, uint32_t wid, W& wv) {
  constexpr uint32_t PTW = 2 * C::FqP::NW + 1;
  PerLane<B2sSeed> seed;
  wv.lanes([&](uint32_t l) {
    const FsqLane q = fsq_lane(a.g, wid, l);
#pragma unroll
    for (int i = 0; i < 8; ++i) seed[l].s[i] = a.seed_in[(size_t)q.b * 8 + i];
  });
  for (uint32_t round = 0; round < 2; ++round) {
    fsq_absorb<C>(wv, a.f, a.g, wid, a.npts,
                  [&](StageWriter& w, uint32_t b, uint32_t i) {
                    const uint32_t* p = a.pts + ((size_t)b * a.npts + i) * PTW;
                    for (uint32_t k = 0; k + 1 < PTW; ++k) stage_word(w, p[k]);
                    stage_byte(w, p[PTW - 1]);
                  },
                  a.tail_words,
                  [&](StageWriter& w, uint32_t b) {
                    for (uint32_t k = 0; k < a.tail_words; ++k) stage_word(w, a.tail[(size_t)b * a.tail_words + k]);
                  },
                  seed);
    wv.lanes([&](uint32_t l) {
      const FsqLane q = fsq_lane(a.g, wid, l);
      if (!q.live || q.sub != 0) return;
#pragma unroll
      for (int i = 0; i < 8; ++i) a.seed_out[((size_t)q.b * 2 + round) * 8 + i] = seed[l].s[i];
    });
  }
}
MP_WAVE_KERNEL(k_absorb, AbsArgs, body_absorb)

// ---- weights of the merged equation: the engine's two functions on a synthetic S arena ---------------------------------------------------
struct MwArgs {
  FsDev f;
  FsqGeom g;
  uint32_t* S;
  const uint32_t* seed_in;   // [B][8]
  VerifyLay l;
};
template <class C>
MP_HD void body_mw_one(const MwArgs& a, uint32_t b, uint32_t) {
  if (b >= a.g.B) return;
  uint32_t seed[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) seed[i] = a.seed_in[(size_t)b * 8 + i];
  fs_merge_weights<C>(a.f, a.S, a.l, b, seed);
}
MP_KERNEL(k_mw_one, MwArgs, body_mw_one)
template <class C, class W>
MP_HD void body_mw_quad(const MwArgs& a, uint32_t wid, W& wv) {
  PerLane<B2sSeed> seed;
  wv.lanes([&](uint32_t l) {
    const FsqLane q = fsq_lane(a.g, wid, l);
#pragma unroll
    for (int i = 0; i < 8; ++i) seed[l].s[i] = a.seed_in[(size_t)q.b * 8 + i];
  });
  fsq_merge_weights<C>(wv, a.f, a.g, wid, a.S, a.l, seed);
}
MP_WAVE_KERNEL(k_mw_quad, MwArgs, body_mw_quad)

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool lpp_ok(uint32_t lpp) { return lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32 || lpp == 64; }

template <class C>
void run_frstream(uint32_t n, const uint32_t* keys, uint32_t* next, uint32_t* flag, uint32_t* val) {
  const size_t key_b = (size_t)n * 32, next_b = (size_t)n * NEXT_N * 32, flag_b = (size_t)n * TRY_N * 4, val_b = (size_t)n * TRY_N * 32;
  DevBuf d_keys(key_b), d_next(next_b), d_flag(flag_b), d_val(val_b);
  rt::h2d(d_keys.p, keys, key_b, STREAM);
  rt::dzero(d_next.p, next_b, STREAM);
  rt::dzero(d_flag.p, flag_b, STREAM);
  rt::dzero(d_val.p, val_b, STREAM);
  const FrsArgs a{d_keys.w(), d_next.w(), d_flag.w(), d_val.w(), n};
  MP_LAUNCH(k_frstream, C, STREAM, n, 1, a);
  rt::d2h(next, d_next.p, next_b, STREAM);
  rt::d2h(flag, d_flag.p, flag_b, STREAM);
  rt::d2h(val, d_val.p, val_b, STREAM);
  rt::stream_sync(STREAM);
}

template <class C>
void run_absorb(uint32_t B, uint32_t lpp, uint32_t npts, uint32_t tail_words, uint32_t Bpad, const uint32_t* pts, const uint32_t* tail,
                const uint32_t* seed_in, uint32_t* seed_out) {
  constexpr uint32_t NW = C::FqP::NW, PTW = 2 * NW + 1;
  need(B > 0 && Bpad >= B && lpp_ok(lpp) && npts <= 4096 && tail_words <= 64, "absorb: shape");
  const uint32_t len = npts * (8 * NW + 1) + 4 * tail_words + 32, words = (len + 3) / 4 + 1;
  const size_t pts_b = (size_t)B * npts * PTW * 4, tail_b = (size_t)B * tail_words * 4, seed_b = (size_t)B * 32;
  DevBuf d_stage((size_t)words * Bpad * 4), d_pts(pts_b), d_tail(tail_b), d_in(seed_b), d_out(2 * seed_b);
  fill_words(d_stage, 0xFFFFFFFFu);
  if (pts_b) rt::h2d(d_pts.p, pts, pts_b, STREAM);
  if (tail_b) rt::h2d(d_tail.p, tail, tail_b, STREAM);
  rt::h2d(d_in.p, seed_in, seed_b, STREAM);
  rt::dzero(d_out.p, 2 * seed_b, STREAM);
  const AbsArgs a{FsDev{d_stage.w(), nullptr, Bpad}, FsqGeom{lpp, B}, d_pts.w(), d_tail.w(), d_in.w(), d_out.w(), npts, tail_words};
  const uint32_t per = 64u / lpp, nwaves = (B + per - 1) / per;
  MP_WAVE_LAUNCH(k_absorb, C, STREAM, nwaves, 0, a);
  rt::d2h(seed_out, d_out.p, 2 * seed_b, STREAM);
  rt::stream_sync(STREAM);
}

// CW comes in pre-filled (an unwritten weight shows) and goes back; dig goes back
template <class C>
void launch_chain_weights(const uint32_t* d_seed, uint32_t* d_cw, uint32_t* d_dig, uint32_t Bpad, uint32_t Tpad, uint32_t T, uint32_t L) {
  const uint32_t nb = (L + CW_BLOCK - 1) / CW_BLOCK;
  const ChainWeightsArgs wa{d_seed, d_cw, d_dig, Bpad, Tpad, T, L};
  MP_LAUNCH(k_chain_digest, C, STREAM, T, nb, wa);
  MP_LAUNCH(k_chain_weights, C, STREAM, T, nb, wa);
}
template <class C>
void run_chain_weights(uint32_t T, uint32_t L, uint32_t Tpad, uint32_t Bpad, const uint32_t* seed, uint32_t* CW, uint32_t* dig) {
  need(T > 0 && L > 0 && Tpad >= T && (uint64_t)Bpad >= (uint64_t)L * T && (uint64_t)L * Tpad < (1u << 24), "chain weights: shape");
  const uint32_t nb = (L + CW_BLOCK - 1) / CW_BLOCK;
  const size_t seed_b = (size_t)8 * Bpad * 4, cw_b = (size_t)L * Tpad * 32, dig_b = (size_t)nb * 8 * Tpad * 4;
  DevBuf d_seed(seed_b), d_cw(cw_b), d_dig(dig_b);
  rt::h2d(d_seed.p, seed, seed_b, STREAM);
  rt::h2d(d_cw.p, CW, cw_b, STREAM);
  rt::dzero(d_dig.p, dig_b, STREAM);
  launch_chain_weights<C>(d_seed.w(), d_cw.w(), d_dig.w(), Bpad, Tpad, T, L);
  rt::d2h(CW, d_cw.p, cw_b, STREAM);
  rt::d2h(dig, d_dig.p, dig_b, STREAM);
  rt::stream_sync(STREAM);
}

// S: [3][Bpad][8], the response z in slot 2; out: [8][g nw T] pre-filled by the caller; then the chain-weight kernels on it, as screen_sigma
template <class C>
void run_screen_digest(uint32_t B, uint32_t g, uint32_t nw, uint32_t Bpad, uint32_t Tpad, const uint32_t* seed, const uint32_t* S,
                       uint32_t* out, uint32_t* CW, uint32_t* dig) {
  need(B > 0 && g > 0 && nw > 0 && nw <= 8 && Bpad >= B && g <= 4096, "screen digest: shape");
  const uint32_t T = (B + g - 1) / g, L = g * nw, SB = L * T, nb = (L + CW_BLOCK - 1) / CW_BLOCK, s_z = 2;
  need(Tpad >= T && (uint64_t)L * Tpad < (1u << 24), "screen digest: Tpad");
  const size_t seed_b = (size_t)8 * Bpad * 4, s_b = (size_t)3 * Bpad * 32, out_b = (size_t)8 * SB * 4, cw_b = (size_t)L * Tpad * 32,
               dig_b = (size_t)nb * 8 * Tpad * 4;
  DevBuf d_seed(seed_b), d_S(s_b), d_out(out_b), d_cw(cw_b), d_dig(dig_b);
  rt::h2d(d_seed.p, seed, seed_b, STREAM);
  rt::h2d(d_S.p, S, s_b, STREAM);
  rt::h2d(d_out.p, out, out_b, STREAM);
  rt::h2d(d_cw.p, CW, cw_b, STREAM);
  rt::dzero(d_dig.p, dig_b, STREAM);
  const ScreenDigestArgs da{d_seed.w(), d_S.w(), d_out.w(), Bpad, SB, B, g, T, nw, s_z};
  MP_LAUNCH(k_screen_digest, C, STREAM, T * g, 1, da);
  launch_chain_weights<C>(d_out.w(), d_cw.w(), d_dig.w(), SB, Tpad, T, L);
  rt::d2h(out, d_out.p, out_b, STREAM);
  rt::d2h(CW, d_cw.p, cw_b, STREAM);
  rt::d2h(dig, d_dig.p, dig_b, STREAM);
  rt::stream_sync(STREAM);
}

// scal: [5n + 9][B][8] (memory format); mr: [B][VC_COUNT][8]; seed_out: [B][8]
template <class C>
void run_merge_weights(int mode, uint32_t B, uint32_t m, uint32_t n, uint32_t lpp, uint32_t Bpad, const uint32_t* scal, const uint32_t* seed_in,
                       uint32_t* mr, uint32_t* seed_out) {
  need(B > 0 && Bpad >= B && m >= 2 && n >= 2 && m <= 64 && n <= 1024 && (mode == 0 || (mode == 1 && lpp_ok(lpp))), "merge weights: shape");
  const VerifyLay l = make_verify_lay(m, n);
  const uint32_t nsc = 5 * n + 9, words = 8 * nsc + 8 + 1;
  need(l.zabar == 0 && l.mr + VC_COUNT <= l.nS, "merge weights: layout");
  const size_t S_b = (size_t)l.nS * Bpad * 32, seed_b = (size_t)8 * Bpad * 4, in_b = (size_t)B * 32;
  DevBuf d_S(S_b), d_stage((size_t)words * Bpad * 4), d_seed(seed_b), d_in(in_b);
  fill_words(d_stage, 0xFFFFFFFFu);
  rt::dzero(d_S.p, S_b, STREAM);
  rt::dzero(d_seed.p, seed_b, STREAM);
  rt::h2d(d_in.p, seed_in, in_b, STREAM);
  std::vector<uint32_t> h((size_t)nsc * Bpad * 8, 0u);
  for (uint32_t i = 0; i < nsc; ++i)
    for (uint32_t b = 0; b < B; ++b)
      for (int t = 0; t < 8; ++t) h[s_off(l.zabar + i, Bpad, b) + t] = scal[((size_t)i * B + b) * 8 + t];
  rt::h2d(d_S.p, h.data(), h.size() * 4, STREAM);
  const MwArgs a{FsDev{d_stage.w(), d_seed.w(), Bpad}, FsqGeom{mode ? lpp : 1u, B}, d_S.w(), d_in.w(), l};
  if (mode == 0) {
    MP_LAUNCH(k_mw_one, C, STREAM, B, 1, a);
  } else {
    const uint32_t per = 64u / lpp, nwaves = (B + per - 1) / per;
    MP_WAVE_LAUNCH(k_mw_quad, C, STREAM, nwaves, 0, a);
  }
  std::vector<uint32_t> hs((size_t)8 * Bpad), hm((size_t)VC_COUNT * Bpad * 8);
  rt::d2h(hs.data(), d_seed.p, seed_b, STREAM);
  rt::d2h(hm.data(), d_S.w() + s_off(l.mr, Bpad, 0), hm.size() * 4, STREAM);
  rt::stream_sync(STREAM);
  for (uint32_t b = 0; b < B; ++b) {
    for (int t = 0; t < 8; ++t) seed_out[(size_t)b * 8 + t] = hs[(size_t)t * Bpad + b];
    for (uint32_t k = 0; k < (uint32_t)VC_COUNT; ++k)
      for (int t = 0; t < 8; ++t) mr[((size_t)b * VC_COUNT + k) * 8 + t] = hm[((size_t)k * Bpad + b) * 8 + t];
  }
}

}  // namespace

// one set of entry points per curve; 0 = done, -1 = see fc_error_<curve>().  FS_CURVE = k compiles curve k only (one object per curve).
#define FC_ENTRIES(NAME, CURVE)                                                                                                        \
  extern "C" int fc_frstream_##NAME(uint32_t n, const uint32_t* keys, uint32_t* next, uint32_t* flag, uint32_t* val) {                 \
    return guarded([&] { run_frstream<CURVE>(n, keys, next, flag, val); });                                                            \
  }                                                                                                                                    \
  extern "C" int fc_fsq_absorb_##NAME(uint32_t B, uint32_t lpp, uint32_t npts, uint32_t tail_words, uint32_t Bpad, const uint32_t* pts, \
                                      const uint32_t* tail, const uint32_t* seed_in, uint32_t* seed_out) {                             \
    return guarded([&] { run_absorb<CURVE>(B, lpp, npts, tail_words, Bpad, pts, tail, seed_in, seed_out); });                          \
  }                                                                                                                                    \
  extern "C" int fc_chain_weights_##NAME(uint32_t T, uint32_t L, uint32_t Tpad, uint32_t Bpad, const uint32_t* seed, uint32_t* CW,     \
                                         uint32_t* dig) {                                                                              \
    return guarded([&] { run_chain_weights<CURVE>(T, L, Tpad, Bpad, seed, CW, dig); });                                                \
  }                                                                                                                                    \
  extern "C" int fc_screen_digest_##NAME(uint32_t B, uint32_t g, uint32_t nw, uint32_t Bpad, uint32_t Tpad, const uint32_t* seed,      \
                                         const uint32_t* S, uint32_t* out, uint32_t* CW, uint32_t* dig) {                              \
    return guarded([&] { run_screen_digest<CURVE>(B, g, nw, Bpad, Tpad, seed, S, out, CW, dig); });                                    \
  }                                                                                                                                    \
  extern "C" int fc_merge_weights_##NAME(int mode, uint32_t B, uint32_t m, uint32_t n, uint32_t lpp, uint32_t Bpad, const uint32_t* scal, \
                                         const uint32_t* seed_in, uint32_t* mr, uint32_t* seed_out) {                                  \
    return guarded([&] { run_merge_weights<CURVE>(mode, B, m, n, lpp, Bpad, scal, seed_in, mr, seed_out); });                          \
  }                                                                                                                                    \
  extern "C" const char* fc_error_##NAME() { return g_error.c_str(); }

#if !defined(FS_CURVE) || FS_CURVE == 0
FC_ENTRIES(stark, Stark)
extern "C" const char* fc_rt_name() { return MP_RT_NAME; }
extern "C" uint32_t fc_vc_count() { return (uint32_t)VC_COUNT; }
extern "C" uint32_t fc_verify_lay_mr(uint32_t m, uint32_t n) { return make_verify_lay(m, n).mr; }
extern "C" int fc_blake2s(int mode, uint32_t n, uint32_t stride, uint32_t maxlen, const uint8_t* data, const uint32_t* lens,
                          const uint32_t* pats, uint32_t* out) {
  return guarded([&] {
    need(n > 0 && stride >= n && maxlen > 0 && maxlen < (1u << 20) && (mode == 0 || (mode == 1 && n % 16 == 0)), "blake2s: shape");
    for (uint32_t x = 0; x < n; ++x) {
      need(lens[2 * x] <= maxlen && lens[2 * x + 1] <= maxlen && pats[x] <= PAT_PIECES, "blake2s: case");
      if (mode == 1) need(lens[2 * x] == lens[2 * (x & ~15u)] && lens[2 * x + 1] == lens[2 * (x & ~15u) + 1], "blake2s: one length per wave");
    }
    const uint32_t maxwords = maxlen / 4 + 2;
    const size_t data_b = (size_t)n * 2 * maxlen, len_b = (size_t)n * 8, pat_b = (size_t)n * 4, out_b = (size_t)n * 2 * 32 * (mode ? 4 : 1);
    need((uint64_t)maxwords * stride * 4 < (1ull << 31), "blake2s: staging buffer");
    DevBuf d_data(data_b), d_lens(len_b), d_pats(pat_b), d_stage((size_t)maxwords * stride * 4), d_out(out_b);
    fill_words(d_stage, 0xFFFFFFFFu);
    rt::h2d(d_data.p, data, data_b, STREAM);
    rt::h2d(d_lens.p, lens, len_b, STREAM);
    rt::h2d(d_pats.p, pats, pat_b, STREAM);
    rt::dzero(d_out.p, out_b, STREAM);
    const B2Args a{(const uint8_t*)d_data.p, d_lens.w(), d_pats.w(), d_stage.w(), d_out.w(), n, stride, maxlen};
    if (mode == 0) {
      MP_LAUNCH(k_b2s, B2One, STREAM, n, 1, a);
    } else {
      MP_WAVE_LAUNCH(k_b2s_quad, B2One, STREAM, n / 16, 0, a);
    }
    rt::d2h(out, d_out.p, out_b, STREAM);
    rt::stream_sync(STREAM);
  });
}
extern "C" int fc_chacha(uint32_t n, const uint32_t* keys, const uint32_t* ctr, uint32_t* out) {
  return guarded([&] {
    need(n > 0, "chacha: shape");
    const size_t key_b = (size_t)n * 32, ctr_b = (size_t)n * 8, out_b = (size_t)n * 64;
    DevBuf d_keys(key_b), d_ctr(ctr_b), d_out(out_b);
    rt::h2d(d_keys.p, keys, key_b, STREAM);
    rt::h2d(d_ctr.p, ctr, ctr_b, STREAM);
    rt::dzero(d_out.p, out_b, STREAM);
    const ChaArgs a{d_keys.w(), d_ctr.w(), d_out.w(), n};
    MP_LAUNCH(k_chacha, B2One, STREAM, n, 1, a);
    rt::d2h(out, d_out.p, out_b, STREAM);
    rt::stream_sync(STREAM);
  });
}
#endif
#if !defined(FS_CURVE) || FS_CURVE == 1
FC_ENTRIES(bn254, Bn254)
#endif
#if !defined(FS_CURVE) || FS_CURVE == 2
FC_ENTRIES(secp256k1, Secp256k1)
#endif
#if !defined(FS_CURVE) || FS_CURVE == 3
FC_ENTRIES(bls12_377, Bls12_377)
#endif
