// What the exact-f32 inference kernels need on top of bf16_ref.h: plain C++, no HIP.
// `conv_check f32 <group>` (conv_check.cpp) and f32_ref_selftest.cpp include it.
//
// The f32 kernels multiply f32 operands and accumulate in f32, and store the f32 sum unconverted.
// On integer operands whose sum of |terms| stays below 2^24 every product and every partial sum is
// an integer that f32 holds exactly, in whatever order a kernel or the MFMA adds them, so every
// output must equal bfr::run_stage<long long>(stage, kNone, /*round_out=*/false, &cond) bit for
// bit (-0 folded into +0).  The reference, the data and the conditions (bfr::Cond) are bf16_ref.h's;
// nothing of them is repeated here.
//
// Data modes (bfr::conv_ranges):
//   int     x in {-2..2} ({-1..1} at K > 1536), w in {-1, 0, 1}: every dropped or misplaced nonzero
//           product changes an output
//   round   x in {-15..15}, w in {-3..3}: larger sums, products that are not +-x
//   widex   |x| <= 2047, |res| <= 2047, |bias| <= 2047, w in {-1, 0, 1}
//   widew   |w| <= 2047, |res| <= 2047, |bias| <= 2047, x in {-1, 0, 1}
// int and round operands have at most 4 significant bits: an operand path that lost precision (a
// bf16 operand keeps 8 bits, slip (g); a 10-bit mantissa, slip (h)) leaves them as they are.  A
// wide operand needs up to 11 significant bits, so either slip changes it.  Headroom: the largest
// K the f32 kernels take is 4608 + 256, and 2047 (4864 + 2) = 9 960 702 < 2^24 = 16 777 216.
// What no mode sees: an operand cut to 11 significant bits (10 stored mantissa bits, tf32; slip
// (i)) holds every |v| <= 2047 exactly.  Seeing it needs |v| >= 2049, and 4095 . 4864 >= 2^24.
#pragma once

#include "bf16_ref.h"

namespace f32r {

using bfr::u16;

// [Cout][K] as the device reads it: the first K1 columns tap-major (kh, kw, cin) when chunk == 0,
// else chunk-major (cin / chunk, kh, kw, cin % chunk) (ConvArgs::kcm = chunk); the downsample's
// columns [K1, K) in place
inline std::vector<float> device_weights(const std::vector<int>& w, int Cout, int K, int K1, int taps, int C, int chunk) {
  std::vector<float> d((size_t)Cout * K);
  for (int o = 0; o < Cout; ++o) {
    for (int t = 0; t < taps; ++t)
      for (int c = 0; c < C; ++c)
        d[(size_t)o * K + (chunk ? ((size_t)(c / chunk) * taps + t) * chunk + c % chunk : (size_t)t * C + c)] =
            (float)w[(size_t)o * K + (size_t)t * C + c];
    for (int kk = K1; kk < K; ++kk) d[(size_t)o * K + kk] = (float)w[(size_t)o * K + kk];
  }
  return d;
}

// the stem's device weights: [64][176], per kh 24 columns (kw * 3 + c, 21 used), 8 zero columns
inline std::vector<float> stem_device_weights(const bfr::StemCase& c) {
  std::vector<float> d(64 * 176, 0.f);
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int i = 0; i < 21; ++i) d[o * 176 + kh * 24 + i] = (float)c.w[o * 147 + kh * 21 + i];
  return d;
}
// the zero-bordered RGB rows the stem kernels read ([N][H + 6][Wp][3], Wp pixels per row; `elems`
// floats in all) and the f32 NCHW frames of the direct kernels
inline std::vector<float> stem_pack(const bfr::StemCase& c, int Wp, size_t elems) {
  std::vector<float> x(elems, 0.f);
  for (int n = 0; n < c.N; ++n)
    for (int i = 0; i < c.H; ++i)
      for (int j = 0; j < c.W; ++j)
        for (int ch = 0; ch < 3; ++ch)
          x[(((size_t)n * (c.H + 6) + i + 3) * Wp + j + 3) * 3 + ch] = (float)c.frames[(((size_t)n * c.H + i) * c.W + j) * 3 + ch];
  return x;
}
inline std::vector<float> stem_frames(const bfr::StemCase& c) {
  std::vector<float> fr((size_t)c.N * 3 * c.H * c.W);
  for (int n = 0; n < c.N; ++n)
    for (int i = 0; i < c.H; ++i)
      for (int j = 0; j < c.W; ++j)
        for (int ch = 0; ch < 3; ++ch)
          fr[(((size_t)n * 3 + ch) * c.H + i) * c.W + j] = (float)c.frames[(((size_t)n * c.H + i) * c.W + j) * 3 + ch];
  return fr;
}

// 7x7/2 pad 3 conv 3 -> 64 + shift + ReLU, then maxpool 3x3/2 pad 1; nothing is rounded in between
template <class Acc>
bfr::ChainOut run_stem(const bfr::StemCase& c, bfr::Slip slip = bfr::kNone) {
  bfr::ChainOut o;
  const std::vector<int> st = bfr::run_stage<Acc>(bfr::stem_stage(c), slip, false, &o.cond);
  o.y.resize((size_t)c.N * c.Hq * c.Wq * 64);
  for (int n = 0; n < c.N; ++n)
    for (int py = 0; py < c.Hq; ++py)
      for (int px = 0; px < c.Wq; ++px)
        for (int ch = 0; ch < 64; ++ch) {
          int m = 0;  // the stem output is a ReLU output, every window holds one
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int sy = 2 * py + dy, sx = 2 * px + dx;
              if (sy >= 0 && sy < c.Hs && sx >= 0 && sx < c.Ws) m = std::max(m, st[(((size_t)n * c.Hs + sy) * c.Ws + sx) * 64 + ch]);
            }
          o.y[(((size_t)n * c.Hq + py) * c.Wq + px) * 64 + ch] = m;
        }
  return o;
}

inline unsigned f32_bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u == 0x80000000u ? 0u : u;  // -0 and +0 compare equal
}

struct Diff {
  long long count = 0;
  long long first = -1;  // flat index of the first differing element
  long long want = 0;
  double got = 0;
};
// every element bitwise: the f32 the kernel stored against (float)ref (|ref| < 2^24: exact)
inline Diff compare(const std::vector<int>& ref, const float* got) {
  Diff d;
  for (size_t i = 0; i < ref.size(); ++i) {
    if (f32_bits((float)ref[i]) == f32_bits(got[i])) continue;
    if (!d.count++) d.first = (long long)i, d.want = ref[i], d.got = got[i];
  }
  return d;
}

// The split stem output: per pooled pixel 64 hi then 64 lo bf16 values, hi = bf16(v) and
// lo = bf16(v - hi), both rounded to nearest even (v - hi is exact in f32).  Compared bitwise
// against that split of the reference integer.  `inexact` counts the outputs whose hi + lo does not
// give v back: none while |v| < 2^16 (8 + 8 significant bits and the sign of lo), so none in int
// mode; in widex v has up to 19 bits and most outputs lose their low bits to the format -- the
// kernel is then still held to the one correct (hi, lo) pair, but the pair no longer shows v whole.
inline Diff compare_split(const std::vector<int>& ref, const u16* got, long long* inexact) {
  Diff d;
  *inexact = 0;
  const size_t pixels = ref.size() / 64;
  for (size_t p = 0; p < pixels; ++p)
    for (int ch = 0; ch < 64; ++ch) {
      const float v = (float)ref[p * 64 + ch];
      const u16 hi = bfr::bf16_rne(v);
      const float r = v - bfr::bf2f(hi);
      const u16 lo = bfr::bf16_rne(r);
      *inexact += bfr::bf2f(hi) + bfr::bf2f(lo) != v;
      const u16 ghi = got[p * 128 + ch], glo = got[p * 128 + 64 + ch];
      if (bfr::fold_zero(hi) == bfr::fold_zero(ghi) && bfr::fold_zero(lo) == bfr::fold_zero(glo)) continue;
      if (!d.count++) d.first = (long long)(p * 64 + ch), d.want = ref[p * 64 + ch], d.got = (double)bfr::bf2f(ghi) + bfr::bf2f(glo);
    }
  return d;
}

}  // namespace f32r
