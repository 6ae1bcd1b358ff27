// Integer data, an int64 reference and a host emulator for the bf16 inference kernels: plain C++,
// no HIP.  `conv_check bf16 <group>` (conv_check.cpp) and bf16_ref_selftest.cpp include it.
//
// The bf16 kernels multiply bf16 operands and accumulate in f32.  On integer operands whose
// sum of |terms| stays below 2^24 every product and every partial sum is an integer that f32
// holds exactly, in whatever order a kernel or the MFMA adds them.  The one rounding left is the
// f32 -> bf16 conversion of an output (round to nearest even), so a kernel can be held to bitwise
// equality with the reference at every output of every image.
//
// Maps and weights are kept as int vectors (NHWC; weights [Cout][K], K tap-major (kh, kw, cin),
// then the folded downsample's columns [K1, K)).  A stage's output holds the *values* of the
// bf16 numbers the kernel stores: integers again, so the fused chains feed them to the next stage.
//
//   int mode    x in {-2..2} ({-1..1} at K > 1536), w in {-1, 0, 1}: almost every output is an
//               integer of magnitude <= 256 that bf16 holds, nothing rounds, and every dropped or
//               misplaced nonzero product changes an output
//   round mode  x in {-15..15}, w in {-3..3}: most outputs need 9 to 12 significant bits, so the
//               conversion rounds, and every odd value in (256, 512) is an exact tie
// The fused chains use narrower ranges and sparse weights (Ranges below) so that the condition
// sum of |terms| < 2^24 holds at every stage.  The reference checks it at every output through an
// upper bound that costs one pass per pixel, max |w| . sum |x read by the pixel's taps| + |bias| +
// |res| (Cond::max_sabs), and counts the outputs that break it (Cond::violations): a case with
// violations has failed.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace bfr {

typedef unsigned short u16;

inline u16 bf16_rne(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
inline u16 bf16_trunc(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return (u16)(u >> 16);
}
inline float bf2f(u16 v) {
  unsigned u = (unsigned)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline u16 fold_zero(u16 v) { return v == 0x8000 ? (u16)0 : v; }  // -0 and +0 compare equal
// the integer an integer v (|v| < 2^24) becomes when stored as bf16
inline int round_int(long long v, bool trunc) {
  const float f = (float)v;
  return (int)bf2f(trunc ? bf16_trunc(f) : bf16_rne(f));
}
// a map as the device holds it (every value already bf16-representable)
inline std::vector<u16> to_bf16(const std::vector<int>& v) {
  std::vector<u16> o(v.size());
  for (size_t i = 0; i < v.size(); ++i) o[i] = bf16_rne((float)v[i]);
  return o;
}
inline std::vector<float> to_f32(const std::vector<int>& v) { return std::vector<float>(v.begin(), v.end()); }

struct Rng {
  unsigned s;
  unsigned next() {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
  }
  int sym(int m) { return (int)(next() % (unsigned)(2 * m + 1)) - m; }  // uniform in {-m..m}
  int sparse(int m, int den) {  // ... kept with probability 1 / den
    const int v = sym(m);
    return den > 1 && next() % (unsigned)den ? 0 : v;
  }
};
inline void fill(std::vector<int>& v, Rng& r, int m, int den = 1) {
  for (auto& e : v) e = r.sparse(m, den);
}

// kWideX / kWideW: the f32 kernels' wide modes (f32_ref.h), one operand of 11 significant bits
enum Mode { kInt = 0, kRound = 1, kWideX = 2, kWideW = 3 };
inline const char* mode_name(int m) {
  static const char* n[] = {"int", "round", "widex", "widew"};
  return n[m];
}

// The slips the host emulator can make (bf16_ref_selftest.cpp shows that the data reject them)
enum Slip {
  kNone = 0,
  kDropStep,       // (a) one 32-channel k-step of the centre tap dropped for pixels [0, 64) x couts [0, 64)
  kPadNeighbour,   // (b) a padding tap reads the neighbouring row or column instead of zero
  kTrunc,          // (c) the output conversion truncates instead of rounding to nearest even
  kResAfterRelu,   // (d) the residual is added after the ReLU
  kNoMidRound,     // (e) in a fused chain the intermediate maps are not rounded to bf16
  kDsNoStride,     // (f) the fused downsample reads x2 at (oh, ow) instead of (s2 oh, s2 ow)
  kOpBf16,         // (g) both operands truncated to bf16 (8 significant bits) before the product
  kOpMant10,       // (h) both operands truncated to a 10-bit mantissa (10 significant bits)
  kOpTf32          // (i) both operands truncated to 10 stored mantissa bits (11 significant bits, tf32)
};
inline const char* slip_name(int s) {
  static const char* n[] = {"none", "a_drop_kstep", "b_pad_neighbour", "c_truncate", "d_res_after_relu", "e_no_mid_round",
                            "f_ds_no_stride", "g_operands_bf16", "h_operands_mant10", "i_operands_tf32"};
  return n[s];
}

// what the reference saw of the data conditions: over256 counts the values handed to the
// conversion (after the ReLU) outside +-256
struct Cond {
  long long outputs = 0, over256 = 0, violations = 0, max_sabs = 0;
  void merge(const Cond& o) {
    outputs += o.outputs, over256 += o.over256, violations += o.violations;
    max_sabs = std::max(max_sabs, o.max_sabs);
  }
};

// One conv: y = cvt(relu(bias + sum taps x w + sum x2 w[K1..] + res))
struct Stage {
  int N = 1, H = 1, W = 1, C = 0, Cout = 0, k = 1, stride = 1, pad = 0;
  const int* x = nullptr;
  const int* w = nullptr;
  int K = 0;  // weight row length
  const int* bias = nullptr;
  const int* res = nullptr;
  bool relu = true;
  const int* x2 = nullptr;  // [N][H2][W2][C2] read at (oh s2, ow s2) against columns [K1, K1 + C2)
  int C2 = 0, s2 = 1, H2 = 0, W2 = 0, K1 = 0;
  int Ho() const { return (H + 2 * pad - k) / stride + 1; }
  int Wo() const { return (W + 2 * pad - k) / stride + 1; }
  long long M() const { return (long long)N * Ho() * Wo(); }
};

// reference dot products of one input run against four consecutive weight rows (stride K): int32
// partial sums (the caller has checked that they cannot overflow), widened to int64
#define BFR_DOT4_BODY                                          \
  const int *w1 = w0 + K, *w2 = w1 + K, *w3 = w2 + K;          \
  int a0 = 0, a1 = 0, a2 = 0, a3 = 0;                          \
  for (int i = 0; i < n; ++i) {                                \
    const int xi = x[i];                                       \
    a0 += xi * w0[i], a1 += xi * w1[i], a2 += xi * w2[i], a3 += xi * w3[i]; \
  }                                                            \
  acc[0] += a0, acc[1] += a1, acc[2] += a2, acc[3] += a3;
inline void dot4_plain(const int* x, const int* w0, int K, int n, long long* acc) { BFR_DOT4_BODY }
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2"))) inline void dot4_avx2(const int* x, const int* w0, int K, int n, long long* acc) { BFR_DOT4_BODY }
inline bool have_avx2() {
  static const bool v = __builtin_cpu_supports("avx2");
  return v;
}
#else
inline void dot4_avx2(const int* x, const int* w0, int K, int n, long long* acc) { dot4_plain(x, w0, K, n, acc); }
inline bool have_avx2() { return false; }
#endif
inline void dot4(const int* x, const int* w0, int K, int n, long long* acc) {
  if (have_avx2()) dot4_avx2(x, w0, K, n, acc);
  else dot4_plain(x, w0, K, n, acc);
}
inline void dot(const int* x, const int* w, int n, long long& acc) {
  int a = 0;
  for (int i = 0; i < n; ++i) a += x[i] * w[i];
  acc += a;
}
inline long long l1(const int* x, int n) {
  long long s = 0;
  for (int i = 0; i < n; ++i) s += x[i] < 0 ? -x[i] : x[i];
  return s;
}
// the emulator's: f32 products accumulated one by one in K order, as a scalar kernel would
inline void dot(const int* x, const int* w, int n, float& acc) {
  for (int i = 0; i < n; ++i) acc += (float)x[i] * (float)w[i];
}

// slips (g), (h), (i): an integer operand cut to `bits` significant bits (toward zero)
inline float keep_bits(int v, int bits) {
  float f = (float)v;  // |v| < 2^24: exact
  unsigned u;
  memcpy(&u, &f, 4);
  u &= ~((1u << (24 - bits)) - 1u);
  memcpy(&f, &u, 4);
  return f;
}
inline int slip_bits(Slip s) { return s == kOpBf16 ? 8 : s == kOpMant10 ? 10 : s == kOpTf32 ? 11 : 24; }
inline void dot_cut(const int* x, const int* w, int n, float& acc, int bits) {
  for (int i = 0; i < n; ++i) acc += keep_bits(x[i], bits) * keep_bits(w[i], bits);
}
inline void dot_cut(const int* x, const int* w, int n, long long& acc, int) { dot(x, w, n, acc); }  // (the reference takes no slip)

inline int host_threads() {
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::min(16u, std::max(1u, hw));
}

inline long long max_abs(const int* p, size_t n) {
  long long m = 0;
  for (size_t i = 0; i < n; ++i) m = std::max(m, (long long)std::abs(p[i]));
  return m;
}

// Acc = long long: the reference (int64, slip kNone, fills cond).  Acc = float: the emulator of the
// kernels' arithmetic, with the slip asked for.  round_out false: the values before the conversion
// (slip (e) on an intermediate map).
template <class Acc>
std::vector<int> run_stage(const Stage& s, Slip slip = kNone, bool round_out = true, Cond* cond = nullptr) {
  const int Ho = s.Ho(), Wo = s.Wo(), taps = s.k * s.k;
  const long long M = s.M();
  std::vector<int> out((size_t)M * s.Cout);
  const bool ref = sizeof(Acc) == 8;
  const bool ref4 = ref && slip == kNone && s.Cout % 4 == 0;
  const long long mw = max_abs(s.w, (size_t)s.Cout * s.K);
  const int cut = slip_bits(slip);
  if (ref) {  // the int32 partial sums of dot()
    const long long mx = std::max(max_abs(s.x, (size_t)s.N * s.H * s.W * s.C),
                                  s.x2 ? max_abs(s.x2, (size_t)s.N * s.H2 * s.W2 * s.C2) : 0LL);
    if (mx * mw * std::max(s.C, s.C2) >= (1LL << 31)) {
      printf("FAIL bf16_ref: operands too large for the reference's int32 partial sums\n");
      exit(2);
    }
  }
  const int nt = (int)std::min<long long>(host_threads(), std::max<long long>(1, M / 16));
  std::vector<Cond> conds(nt);
  auto work = [&](int ti) {
    Cond& lc = conds[ti];
    const long long m0 = M * ti / nt, m1 = M * (ti + 1) / nt;
    for (long long m = m0; m < m1; ++m) {
      const int n = (int)(m / ((long long)Ho * Wo)), rem = (int)(m % ((long long)Ho * Wo)), oh = rem / Wo, ow = rem % Wo;
      // the pixel's taps (null: a padding tap), and max |w| times the L1 norm of what they read: an
      // upper bound of the sum of |products| of every cout of this pixel, computed once per pixel
      const int* tap[49];
      long long norm = 0;
      for (int t = 0; t < taps; ++t) {
        int ih = oh * s.stride - s.pad + t / s.k, iw = ow * s.stride - s.pad + t % s.k;
        tap[t] = nullptr;
        if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W) {
          if (slip != kPadNeighbour) continue;
          ih = std::min(std::max(ih, 0), s.H - 1);
          iw = std::min(std::max(iw, 0), s.W - 1);
        }
        tap[t] = s.x + (((size_t)n * s.H + ih) * s.W + iw) * s.C;
        if (ref) norm += l1(tap[t], s.C);
      }
      const int f = slip == kDsNoStride ? 1 : s.s2;
      const int* xds = s.x2 ? s.x2 + (((size_t)n * s.H2 + oh * f) * s.W2 + ow * f) * s.C2 : nullptr;
      if (ref && xds) norm += l1(xds, s.C2);
      norm *= mw;
      Acc acc4[4] = {0, 0, 0, 0};
      for (int o = 0; o < s.Cout; ++o) {
        Acc acc = 0;
        const int* wrow = s.w + (size_t)o * s.K;
        if (ref4) {  // the reference: four couts per pass, runs of adjacent taps as one dot product
          if (o % 4 == 0) {
            long long a4[4] = {0, 0, 0, 0};
            for (int t = 0; t < taps;) {
              if (!tap[t]) { ++t; continue; }
              int r = 1;
              while (t + r < taps && tap[t + r] == tap[t] + (size_t)r * s.C) ++r;
              dot4(tap[t], wrow + (size_t)t * s.C, s.K, r * s.C, a4);
              t += r;
            }
            if (xds) dot4(xds, wrow + s.K1, s.K, s.C2, a4);
            for (int j = 0; j < 4; ++j) acc4[j] = (Acc)a4[j];
          }
          acc = acc4[o % 4];
        } else {
          for (int t = 0; t < taps; ++t) {
            if (!tap[t]) continue;
            const int c0 = slip == kDropStep && t == taps / 2 && m < 64 && o < 64 ? std::min(32, s.C) : 0;
            if (cut < 24) dot_cut(tap[t] + c0, wrow + (size_t)t * s.C + c0, s.C - c0, acc, cut);
            else dot(tap[t] + c0, wrow + (size_t)t * s.C + c0, s.C - c0, acc);
          }
          if (xds && cut < 24) dot_cut(xds, wrow + s.K1, s.C2, acc, cut);
          else if (xds) dot(xds, wrow + s.K1, s.C2, acc);
        }
        // epilogue as the kernels order it: shift, residual, ReLU, convert
        const int r = s.res ? s.res[(size_t)m * s.Cout + o] : 0;
        acc += (Acc)s.bias[o];
        Acc v = acc;
        if (slip == kResAfterRelu && s.relu) {
          v = (v > 0 ? v : (Acc)0) + (Acc)r;
        } else {
          v += (Acc)r;
          if (s.relu && v < 0) v = 0;
        }
        const long long sabs = norm + std::abs(s.bias[o]) + std::abs(r);
        ++lc.outputs;
        lc.over256 += v > 256 || v < -256;
        lc.violations += sabs >= (1LL << 24);
        lc.max_sabs = std::max(lc.max_sabs, sabs);
        out[(size_t)m * s.Cout + o] = round_out ? round_int((long long)v, slip == kTrunc) : (int)v;
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& t : th) t.join();
  if (cond)
    for (const Cond& c : conds) cond->merge(c);
  return out;
}

// ---------------------------------------------------------------- single convs (+ folded downsample)
struct Ranges {
  int x, w, wden, res, bias;
};
inline Ranges conv_ranges(int mode, int K) {
  if (mode == kRound) return {15, 3, 1, 63, 31};
  // f32 only (f32_ref.h): max |w| . K max |x| + |bias| + |res| <= 2047 (4864 + 2) < 2^24 at the largest K
  if (mode == kWideX) return {2047, 1, 1, 2047, 2047};
  if (mode == kWideW) return {1, 2047, 1, 2047, 2047};
  return {K > 1536 ? 1 : 2, 1, 1, 3, 4};
}

struct ConvCase {
  int N, H, W, C, Cout, k, stride, pad, Cds, s2, mode;
  int Ho, Wo, H2, W2, K1, K;
  std::vector<int> x, x2, w, bias, res;
  long long M() const { return (long long)N * Ho * Wo; }
  Stage stage(bool with_res, bool relu) const {
    Stage s;
    s.N = N, s.H = H, s.W = W, s.C = C, s.Cout = Cout, s.k = k, s.stride = stride, s.pad = pad;
    s.x = x.data(), s.w = w.data(), s.K = K, s.bias = bias.data(), s.res = with_res ? res.data() : nullptr, s.relu = relu;
    if (Cds) s.x2 = x2.data(), s.C2 = Cds, s.s2 = s2, s.H2 = H2, s.W2 = W2, s.K1 = K1;
    return s;
  }
  bool same_shape(const ConvCase& o) const {
    return N == o.N && H == o.H && W == o.W && C == o.C && Cout == o.Cout && k == o.k && stride == o.stride && pad == o.pad &&
           Cds == o.Cds && s2 == o.s2 && mode == o.mode;
  }
};
inline ConvCase make_conv(int N, int H, int W, int C, int Cout, int k, int stride, int pad, int Cds, int s2, int mode,
                          unsigned seed = 20240229u) {
  ConvCase c;
  c.N = N, c.H = H, c.W = W, c.C = C, c.Cout = Cout, c.k = k, c.stride = stride, c.pad = pad, c.Cds = Cds, c.s2 = s2,
  c.mode = mode;
  c.Ho = (H + 2 * pad - k) / stride + 1, c.Wo = (W + 2 * pad - k) / stride + 1;
  c.H2 = Cds ? c.Ho * s2 : 0, c.W2 = Cds ? c.Wo * s2 : 0;
  c.K1 = k * k * C, c.K = c.K1 + Cds;
  const Ranges r = conv_ranges(mode, c.K);
  Rng g{seed + 7u * (unsigned)mode};
  c.x.resize((size_t)N * H * W * C), c.x2.resize((size_t)N * c.H2 * c.W2 * Cds), c.w.resize((size_t)Cout * c.K);
  c.bias.resize(Cout), c.res.resize((size_t)c.M() * Cout);
  fill(c.x, g, r.x), fill(c.x2, g, r.x), fill(c.w, g, r.w, r.wden), fill(c.bias, g, r.bias), fill(c.res, g, r.res);
  return c;
}

// [Cout][K] in the order the device reads it: the first K1 columns chunk-major
// (cin / 64, kh, kw, cin % 64) when kcm, the downsample columns in place
inline std::vector<u16> device_weights(const std::vector<int>& w, int Cout, int K, int K1, int taps, int C, bool kcm) {
  std::vector<u16> d((size_t)Cout * K);
  for (int o = 0; o < Cout; ++o) {
    for (int t = 0; t < taps; ++t)
      for (int c = 0; c < C; ++c)
        d[(size_t)o * K + (kcm ? ((size_t)(c / 64) * taps + t) * 64 + c % 64 : (size_t)t * C + c)] =
            bf16_rne((float)w[(size_t)o * K + (size_t)t * C + c]);
    for (int kk = K1; kk < K; ++kk) d[(size_t)o * K + kk] = bf16_rne((float)w[(size_t)o * K + kk]);
  }
  return d;
}

// ---------------------------------------------------------------- fused chains
// A stage-1 bottleneck block as bneck_bf16 / bneck_tail_bf16 run it:
//   T1 = cvt(relu(conv1x1(x, w1) + b1))                  (tail: x is T1 already)
//   T2 = cvt(relu(conv3x3(T1, w2) + b2))
//   Y  = cvt(relu(conv1x1(T2, w3[:, :64]) + b3 + R))     R = x (cin 256), res (tail), or the folded
//                                                        stride-1 downsample x . w3[:, 64:128] (cin 64)
//   Z  = cvt(relu(conv1x1(Y, wn) + bn))                  (next / tail; cn = 64 / 128)
// The weights are sparse so that each stage's sum stays small (header comment).
struct BneckCase {
  int N, H, W, cin, cn, K3, mode;
  bool next, tail;
  std::vector<int> x, res, w1, b1, w2, b2, w3, b3, wn, bn;
  long long M() const { return (long long)N * H * W; }
};
inline BneckCase make_bneck(int N, int H, int W, int cin, bool next, bool tail, int mode, unsigned seed = 4242u) {
  BneckCase c;
  c.N = N, c.H = H, c.W = W, c.cin = tail ? 64 : cin, c.next = next || tail, c.tail = tail, c.mode = mode;
  c.cn = tail ? 128 : 64;
  c.K3 = !tail && cin == 64 ? 128 : 64;
  Rng g{seed + 13u * (unsigned)mode + (unsigned)cin + (tail ? 5u : 0u)};
  const size_t M = (size_t)c.M();
  c.x.resize(M * c.cin), c.res.resize(tail ? M * 256 : 0);
  c.w1.resize((size_t)64 * c.cin), c.w2.resize((size_t)64 * 576), c.w3.resize((size_t)256 * c.K3), c.wn.resize((size_t)c.cn * 256);
  c.b1.resize(64), c.b2.resize(64), c.b3.resize(256), c.bn.resize(c.cn);
  const bool rd = mode == kRound;
  if (tail) {  // T1 is a ReLU output: non-negative
    for (auto& e : c.x) e = std::abs(g.sym(rd ? 15 : 4));
  } else {
    fill(c.x, g, rd ? 7 : 1);
  }
  fill(c.res, g, rd ? 63 : 2);
  fill(c.w1, g, rd ? 2 : 1, c.cin == 256 ? (rd ? 2 : 8) : (rd ? 1 : 2));
  fill(c.w2, g, rd ? 2 : 1, rd ? 2 : 8);
  fill(c.w3, g, rd ? 2 : 1, rd ? 2 : 16);
  fill(c.wn, g, 1, rd ? 4 : 32);
  fill(c.b1, g, rd ? 15 : 2), fill(c.b2, g, rd ? 15 : 2), fill(c.b3, g, rd ? 31 : 2), fill(c.bn, g, rd ? 31 : 2);
  return c;
}
struct ChainOut {
  std::vector<int> y, z;
  Cond cond;
};
template <class Acc>
ChainOut run_bneck(const BneckCase& c, Slip slip = kNone) {
  ChainOut o;
  const bool mid = slip != kNoMidRound;
  Stage s;
  s.N = c.N, s.H = c.H, s.W = c.W;
  std::vector<int> t1;
  if (c.tail) {
    t1 = c.x;
  } else {
    s.C = c.cin, s.Cout = 64, s.x = c.x.data(), s.w = c.w1.data(), s.K = c.cin, s.bias = c.b1.data();
    t1 = run_stage<Acc>(s, slip, mid, &o.cond);
  }
  Stage s2 = s;
  s2.C = 64, s2.Cout = 64, s2.k = 3, s2.pad = 1, s2.x = t1.data(), s2.w = c.w2.data(), s2.K = 576, s2.bias = c.b2.data();
  const std::vector<int> t2 = run_stage<Acc>(s2, slip, mid, &o.cond);
  Stage s3 = s;
  s3.C = 64, s3.Cout = 256, s3.x = t2.data(), s3.w = c.w3.data(), s3.K = c.K3, s3.bias = c.b3.data();
  if (c.tail) s3.res = c.res.data();
  else if (c.cin == 256) s3.res = c.x.data();
  else s3.x2 = c.x.data(), s3.C2 = 64, s3.s2 = 1, s3.H2 = c.H, s3.W2 = c.W, s3.K1 = 64;
  o.y = run_stage<Acc>(s3, slip, true, &o.cond);
  if (c.next) {
    Stage sn = s;
    sn.C = 256, sn.Cout = c.cn, sn.x = o.y.data(), sn.w = c.wn.data(), sn.K = 256, sn.bias = c.bn.data();
    o.z = run_stage<Acc>(sn, slip, true, &o.cond);
  }
  return o;
}

// An R18 stage-1 basic block as bblock_bf16 runs it: T = cvt(relu(conv3x3(x, w1) + b1)),
// Y = cvt(relu(conv3x3(T, w2) + b2 + x))
struct BblockCase {
  int N, H, W, mode;
  std::vector<int> x, w1, b1, w2, b2;
};
inline BblockCase make_bblock(int N, int H, int W, int mode, unsigned seed = 99u) {
  BblockCase c;
  c.N = N, c.H = H, c.W = W, c.mode = mode;
  Rng g{seed + 13u * (unsigned)mode};
  c.x.resize((size_t)N * H * W * 64), c.w1.resize(64 * 576), c.w2.resize(64 * 576), c.b1.resize(64), c.b2.resize(64);
  const bool rd = mode == kRound;
  fill(c.x, g, rd ? 15 : 1);
  fill(c.w1, g, rd ? 2 : 1, rd ? 1 : 4);
  fill(c.w2, g, rd ? 2 : 1, rd ? 2 : 16);
  fill(c.b1, g, rd ? 15 : 2), fill(c.b2, g, rd ? 15 : 2);
  return c;
}
template <class Acc>
ChainOut run_bblock(const BblockCase& c, Slip slip = kNone) {
  ChainOut o;
  Stage s;
  s.N = c.N, s.H = c.H, s.W = c.W, s.C = 64, s.Cout = 64, s.k = 3, s.pad = 1, s.K = 576;
  s.x = c.x.data(), s.w = c.w1.data(), s.bias = c.b1.data();
  const std::vector<int> t = run_stage<Acc>(s, slip, slip != kNoMidRound, &o.cond);
  s.x = t.data(), s.w = c.w2.data(), s.bias = c.b2.data(), s.res = c.x.data();
  o.y = run_stage<Acc>(s, slip, true, &o.cond);
  return o;
}

// A bottleneck 1x1 pair as pair1x1(r)_bf16 / pairw_bf16 run it:
//   Y = cvt(relu(x . w3[:, :cmid] + b3 + R)),  R = res, or the folded downsample x2 . w3[:, cmid:]
//       (x2 [N][s2 H][s2 W][cds] read at (s2 oh, s2 ow); s2 = 1 in stage 1, 2 in pairw)
//   Z = cvt(relu(Y . w1 + b1))
struct PairCase {
  int N, H, W, cmid, cexp, c1, cds, s2, mode;
  std::vector<int> x, x2, res, w3, b3, w1, b1;
  long long M() const { return (long long)N * H * W; }
};
inline PairCase make_pair_case(int N, int H, int W, int cmid, int cexp, int c1, int cds, int s2, int mode, unsigned seed = 31337u) {
  PairCase c;
  c.N = N, c.H = H, c.W = W, c.cmid = cmid, c.cexp = cexp, c.c1 = c1, c.cds = cds, c.s2 = s2, c.mode = mode;
  Rng g{seed + 13u * (unsigned)mode + (unsigned)(cmid + c1 + cds)};
  const size_t M = (size_t)c.M();
  c.x.resize(M * cmid), c.x2.resize(cds ? (size_t)N * s2 * H * s2 * W * cds : 0), c.res.resize(cds ? 0 : M * cexp);
  c.w3.resize((size_t)cexp * (cmid + cds)), c.w1.resize((size_t)c1 * cexp), c.b3.resize(cexp), c.b1.resize(c1);
  const bool rd = mode == kRound;
  // x is a ReLU output in the network; signed here, so that the sum keeps cancelling
  fill(c.x, g, rd ? 15 : 2), fill(c.x2, g, rd ? 15 : 2), fill(c.res, g, rd ? 63 : 3);
  fill(c.w3, g, rd ? 3 : 1, rd ? 1 : (cmid + cds) / 32);  // int: ~32 nonzero terms per output
  fill(c.w1, g, rd ? 2 : 1, rd ? 2 : cexp / 16);
  fill(c.b3, g, rd ? 31 : 4), fill(c.b1, g, rd ? 31 : 4);
  return c;
}
template <class Acc>
ChainOut run_pair(const PairCase& c, Slip slip = kNone) {
  ChainOut o;
  Stage s;
  s.N = c.N, s.H = c.H, s.W = c.W, s.C = c.cmid, s.Cout = c.cexp, s.x = c.x.data(), s.w = c.w3.data(), s.K = c.cmid + c.cds;
  s.bias = c.b3.data();
  if (c.cds) s.x2 = c.x2.data(), s.C2 = c.cds, s.s2 = c.s2, s.H2 = c.s2 * c.H, s.W2 = c.s2 * c.W, s.K1 = c.cmid;
  else s.res = c.res.data();
  o.y = run_stage<Acc>(s, slip, true, &o.cond);
  Stage z;
  z.N = c.N, z.H = c.H, z.W = c.W, z.C = c.cexp, z.Cout = c.c1, z.x = o.y.data(), z.w = c.w1.data(), z.K = c.cexp;
  z.bias = c.b1.data();
  o.z = run_stage<Acc>(z, slip, true, &o.cond);
  return o;
}

// ---------------------------------------------------------------- fused stem + pool
// 7x7/2 pad 3 conv 3 -> 64 + shift + ReLU, rounded to bf16, then maxpool 3x3/2 pad 1
struct StemCase {
  int N, H, W, mode, Hs, Ws, Hq, Wq;
  std::vector<int> frames;  // [N][H][W][3]
  std::vector<int> w;       // [64][147] tap-major
  std::vector<int> bias;
};
inline StemCase make_stem(int N, int H, int W, int mode, unsigned seed = 555u) {
  StemCase c;
  c.N = N, c.H = H, c.W = W, c.mode = mode;
  c.Hs = (H - 1) / 2 + 1, c.Ws = (W - 1) / 2 + 1, c.Hq = (c.Hs - 1) / 2 + 1, c.Wq = (c.Ws - 1) / 2 + 1;
  Rng g{seed + 13u * (unsigned)mode};
  const Ranges r = conv_ranges(mode, 147);
  c.frames.resize((size_t)N * H * W * 3), c.w.resize(64 * 147), c.bias.resize(64);
  fill(c.frames, g, r.x), fill(c.w, g, r.w), fill(c.bias, g, r.bias);
  return c;
}
inline Stage stem_stage(const StemCase& c) {  // the conv alone (the unfused stem)
  Stage s;
  s.N = c.N, s.H = c.H, s.W = c.W, s.C = 3, s.Cout = 64, s.k = 7, s.stride = 2, s.pad = 3;
  s.x = c.frames.data(), s.w = c.w.data(), s.K = 147, s.bias = c.bias.data();
  return s;
}
template <class Acc>
ChainOut run_stem(const StemCase& c, Slip slip = kNone) {
  ChainOut o;
  const std::vector<int> st = run_stage<Acc>(stem_stage(c), slip, slip != kNoMidRound, &o.cond);
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
          o.y[(((size_t)n * c.Hq + py) * c.Wq + px) * 64 + ch] = slip == kNoMidRound ? round_int(m, false) : m;
        }
  return o;
}
// the stem's device weights: [64][192], per kh 24 columns (kw * 3 + c, 21 used)
inline std::vector<u16> stem_device_weights(const StemCase& c) {
  std::vector<u16> d(64 * 192, 0);
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int i = 0; i < 21; ++i) d[o * 192 + kh * 24 + i] = bf16_rne((float)c.w[o * 147 + kh * 21 + i]);
  return d;
}

// ---------------------------------------------------------------- comparison
struct Diff {
  long long count = 0;
  long long first = -1;  // flat index of the first differing element
  int want = 0;
  float got = 0;
};
// every element, bitwise after folding -0 into +0
inline Diff compare(const std::vector<int>& ref, const u16* got) {
  Diff d;
  for (size_t i = 0; i < ref.size(); ++i) {
    if (fold_zero(bf16_rne((float)ref[i])) == fold_zero(got[i])) continue;
    if (!d.count++) d.first = (long long)i, d.want = ref[i], d.got = bf2f(got[i]);
  }
  return d;
}
inline long long differing(const std::vector<int>& a, const std::vector<int>& b) {
  long long n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += a[i] != b[i];
  return n;
}

}  // namespace bfr
