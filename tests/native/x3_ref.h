// Reference, bounds and a host emulator for the f32x3 (split-bf16) convs: plain C++, no HIP.
//
// Layouts, as the library defines them (common.h ConvArgs::split, split_chan; fold_conv in
// eosv_api.hip):
//   activations  [N][H][W][2C] bf16, per pixel the hi block then the lo block
//   weights      [Cout][K], K = KH KW 3C (+ 3 Cds): per tap the virtual channel blocks
//                (w0, w1, w2) = (w_hi, w_hi, w_lo), read against (x_hi, x_lo, x_hi).  K order
//                tap-major (kh, kw, 3C) or, kcm, (c / 64, kh, kw, c % 64) over c < 3C
//   downsample   K columns [K1, K) over x2 [N][H2][W2][2 Cds], Cin2 = 3 Cds, read at
//                (oh s2, ow s2); always in block order (d0, d1, d2), never chunk-major
//   output       [M][2 Cout]: hi = bf16(v), lo = bf16(v - hi)
//
// The kernels are bilinear in what is stored: they sum x_hi w0 + x_lo w1 + x_hi w2 and know
// nothing about lo << hi.  In *probe* data the hi and lo blocks hold independent O(1) values, so
// each of the three products carries full weight and a dropped or mis-paired k-step is an O(0.1)
// error against a bound near 1e-4; *real* data splits f32 values as the library does, where the
// same slip is a 2^-9 effect.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace x3 {

typedef unsigned short u16;

inline float frand(unsigned& s) {
  s = s * 1664525u + 1013904223u;
  return ((s >> 8) & 0xffff) / 32768.f - 1.f;
}
inline u16 f2bf(float f) {  // RNE
  unsigned u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
inline float bf2f(u16 v) {
  unsigned u = (unsigned)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct Shape {
  int N, H, W, C, Cout, k, stride, pad;
  int Cds, s2;  // fused 1x1 downsample over x2 (Cds logical channels, stride s2); 0 = none
  bool real;    // data mode
  bool operator==(const Shape& o) const {
    return N == o.N && H == o.H && W == o.W && C == o.C && Cout == o.Cout && k == o.k && stride == o.stride &&
           pad == o.pad && Cds == o.Cds && s2 == o.s2 && real == o.real;
  }
};

// One conv's operands.  The residual is always generated; a run chooses whether to use it.
struct Case {
  Shape s;
  int Ho, Wo, H2, W2, K1, K;
  std::vector<u16> x, x2, res;  // stored split maps
  std::vector<u16> w;           // [Cout][K], tap-major (the logical order; device_weights reorders)
  std::vector<float> bias;
  std::vector<float> xf, x2f, resf, wf;  // real mode: the f32 values before the split; wf [Cout][taps C + Cds]
  std::vector<int> images;               // the images a check covers: 0, 1, N - 2, N - 1
  long long M() const { return (long long)s.N * Ho * Wo; }
};

inline void split_store(float v, u16* hi, u16* lo) {
  *hi = f2bf(v);
  *lo = f2bf(v - bf2f(*hi));
}

inline Case make_case(const Shape& s, unsigned seed = 777) {
  Case c;
  c.s = s;
  c.Ho = (s.H + 2 * s.pad - s.k) / s.stride + 1;
  c.Wo = (s.W + 2 * s.pad - s.k) / s.stride + 1;
  c.H2 = s.Cds ? c.Ho * s.s2 : 0;
  c.W2 = s.Cds ? c.Wo * s.s2 : 0;
  const int taps = s.k * s.k, C = s.C, D = s.Cds;
  c.K1 = taps * 3 * C;
  c.K = c.K1 + 3 * D;
  unsigned r = seed;
  const size_t npx = (size_t)s.N * s.H * s.W, npx2 = (size_t)s.N * c.H2 * c.W2, nout = (size_t)c.M();
  c.x.resize(npx * 2 * C);
  c.x2.resize(npx2 * 2 * D);
  c.res.resize(nout * 2 * s.Cout);
  c.w.assign((size_t)s.Cout * c.K, 0);
  c.bias.resize(s.Cout);
  auto fill_map = [&](std::vector<u16>& m, std::vector<float>& f, size_t pixels, int ch) {
    if (s.real) {
      f.resize(pixels * ch);
      for (size_t p = 0; p < pixels; ++p)
        for (int i = 0; i < ch; ++i) {
          const float v = frand(r);
          f[p * ch + i] = v;
          split_store(v, &m[p * 2 * ch + i], &m[p * 2 * ch + ch + i]);
        }
    } else {
      for (auto& v : m) v = f2bf(frand(r));  // hi and lo independent
    }
  };
  fill_map(c.x, c.xf, npx, C);
  fill_map(c.x2, c.x2f, npx2, D);
  fill_map(c.res, c.resf, nout, s.Cout);
  if (s.real) c.wf.resize((size_t)s.Cout * (taps * C + D));
  for (int o = 0; o < s.Cout; ++o) {
    u16* row = c.w.data() + (size_t)o * c.K;
    for (int g = 0; g <= taps; ++g) {  // the taps, then the downsample columns
      const int ch = g < taps ? C : D;
      u16* blk = g < taps ? row + (size_t)g * 3 * C : row + c.K1;
      for (int i = 0; i < ch; ++i) {
        if (s.real) {
          const float v = 0.1f * frand(r);
          c.wf[(size_t)o * (taps * C + D) + (size_t)g * C + i] = v;
          split_store(v, &blk[i], &blk[2 * ch + i]);
        } else {
          blk[i] = f2bf(0.1f * frand(r));
          blk[2 * ch + i] = f2bf(0.1f * frand(r));  // w_lo independent of w_hi
        }
        blk[ch + i] = blk[i];  // block 1 = block 0: the loader's contract (conv_rows_x3 reads only 0 and 2)
      }
    }
  }
  for (auto& v : c.bias) v = frand(r);
  const int cand[4] = {0, s.N > 1 ? 1 : 0, s.N > 2 ? s.N - 2 : 0, s.N - 1};
  for (int n : cand) {
    bool seen = false;
    for (int m : c.images) seen |= m == n;
    if (!seen) c.images.push_back(n);
  }
  return c;
}

// the weights in the order the device reads them: the first K1 columns chunk-major when kcm
inline std::vector<u16> device_weights(const Case& c, bool kcm) {
  if (!kcm) return c.w;
  std::vector<u16> d(c.w.size());
  const int taps = c.s.k * c.s.k, VC = 3 * c.s.C;
  for (int o = 0; o < c.s.Cout; ++o) {
    const u16* src = c.w.data() + (size_t)o * c.K;
    u16* dst = d.data() + (size_t)o * c.K;
    for (int t = 0; t < taps; ++t)
      for (int v = 0; v < VC; ++v) dst[((size_t)(v / 64) * taps + t) * 64 + v % 64] = src[(size_t)t * VC + v];
    for (int k = c.K1; k < c.K; ++k) dst[k] = src[k];
  }
  return d;
}

// Reference of the conv part in double, on the checked images: acc = bias + sum of the terms,
// sabs = |bias| + sum of |terms|.  probe: the terms are the three stored products per channel;
// real: the one product of the original f32 values.
struct Ref {
  std::vector<double> acc, sabs;  // [images][Ho][Wo][Cout]
};

inline Ref reference(const Case& c) {
  const Shape& s = c.s;
  const int C = s.C, D = s.Cds, taps = s.k * s.k;
  Ref r;
  const size_t per = (size_t)c.Ho * c.Wo * s.Cout;
  r.acc.resize(c.images.size() * per);
  r.sabs.resize(c.images.size() * per);
  // operands as float (exact), weights per cout contiguous
  std::vector<float> xv(c.x.size()), x2v(c.x2.size()), wv(c.w.size());
  for (size_t i = 0; i < xv.size(); ++i) xv[i] = bf2f(c.x[i]);
  for (size_t i = 0; i < x2v.size(); ++i) x2v[i] = bf2f(c.x2[i]);
  for (size_t i = 0; i < wv.size(); ++i) wv[i] = bf2f(c.w[i]);
  for (size_t ii = 0; ii < c.images.size(); ++ii) {
    const int n = c.images[ii];
    for (int oh = 0; oh < c.Ho; ++oh)
      for (int ow = 0; ow < c.Wo; ++ow)
        for (int o = 0; o < s.Cout; ++o) {
          double acc = c.bias[o], sabs = fabs(c.bias[o]);
          for (int t = 0; t <= taps; ++t) {
            size_t px;
            int ch;
            if (t < taps) {
              const int ih = oh * s.stride - s.pad + t / s.k, iw = ow * s.stride - s.pad + t % s.k;
              if (ih < 0 || ih >= s.H || iw < 0 || iw >= s.W) continue;
              px = ((size_t)n * s.H + ih) * s.W + iw;
              ch = C;
            } else {
              if (!D) continue;
              px = ((size_t)n * c.H2 + oh * s.s2) * c.W2 + ow * s.s2;
              ch = D;
            }
            if (s.real) {
              const float* xp = (t < taps ? c.xf.data() : c.x2f.data()) + px * ch;
              const float* wp = c.wf.data() + (size_t)o * (taps * C + D) + (size_t)t * C;
              for (int i = 0; i < ch; ++i) {
                const double p = (double)xp[i] * wp[i];
                acc += p;
                sabs += fabs(p);
              }
            } else {
              const float* xp = (t < taps ? xv.data() : x2v.data()) + px * 2 * ch;
              const float* wp = wv.data() + (size_t)o * c.K + (t < taps ? (size_t)t * 3 * C : (size_t)c.K1);
              for (int i = 0; i < ch; ++i) {
                const double p0 = (double)xp[i] * wp[i], p1 = (double)xp[ch + i] * wp[ch + i],
                             p2 = (double)xp[i] * wp[2 * ch + i];
                acc += p0 + p1 + p2;
                sabs += fabs(p0) + fabs(p1) + fabs(p2);
              }
            }
          }
          const size_t oi = ii * per + ((size_t)oh * c.Wo + ow) * s.Cout + o;
          r.acc[oi] = acc;
          r.sabs[oi] = sabs;
        }
  }
  return r;
}

// Per-element bound on |y_hi + y_lo - ref|:
//   probe  coef (1 + sabs) + 2^-17 |ref|
//   real   (coef + 3 2^-18) (1 + sabs) + 2^-17 |ref|
// coef = 2e-6: f32 MFMA accumulation, the coefficient conv_check uses for the exact-f32 convs at
// K up to 4864.  2^-17 |ref|: the output's hi + lo form (lo is within 2^-9 of a residual that is
// within 2^-9 of v; one bit of slack).  The three 2^-18 of real data: the hi + lo form of x, that
// of w, and the dropped lo.lo product.  And |y_lo| <= |y_hi| / 256: lo is the rounding residual
// of hi.
constexpr double kCoef = 2e-6;
struct Stats {
  double max_ratio = 0;  // max err / bound
  long bad = 0, bad_dup = 0;
  bool ok() const { return !bad && !bad_dup; }
};

// y: the whole output map [M][2 Cout]; res / relu as the run used them
inline Stats verify(const Case& c, const Ref& r, const u16* y, bool res, bool relu, double coef = kCoef,
                    bool print = true) {
  const Shape& s = c.s;
  const size_t per = (size_t)c.Ho * c.Wo * s.Cout;
  Stats st;
  for (size_t ii = 0; ii < c.images.size(); ++ii) {
    const int n = c.images[ii];
    for (size_t e = 0; e < per; ++e) {
      const size_t pix = (size_t)n * c.Ho * c.Wo + e / s.Cout;
      const int o = (int)(e % s.Cout);
      double ref = r.acc[ii * per + e], sabs = r.sabs[ii * per + e];
      if (res) {
        if (s.real) {
          const double v = c.resf[pix * s.Cout + o];
          ref += v, sabs += fabs(v);
        } else {
          const double h = bf2f(c.res[pix * 2 * s.Cout + o]), l = bf2f(c.res[pix * 2 * s.Cout + s.Cout + o]);
          ref += h + l, sabs += fabs(h) + fabs(l);
        }
      }
      if (relu && ref < 0) ref = 0;
      const double hi = bf2f(y[pix * 2 * s.Cout + o]), lo = bf2f(y[pix * 2 * s.Cout + s.Cout + o]);
      const double err = fabs(hi + lo - ref);
      const double bound = (coef + (s.real ? 3.0 / 262144 : 0.0)) * (1 + sabs) + fabs(ref) / 131072;
      const bool dup = fabs(lo) <= fabs(hi) / 256;
      const bool in = err <= bound;  // false for NaN
      if (!in || !dup) {
        if (print && st.bad + st.bad_dup < 5) {
          const int rem = (int)(e / s.Cout);
          printf("  bad n%d oh%d ow%d o%d ref %.9g got %.9g + %.9g err %.3e bound %.3e dup %d\n", n, rem / c.Wo,
                 rem % c.Wo, o, ref, hi, lo, err, bound, (int)dup);
        }
        st.bad += !in;
        st.bad_dup += in && !dup;
      }
      const double ratio = in || err == err ? err / bound : INFINITY;
      if (!(ratio <= st.max_ratio)) st.max_ratio = ratio;
    }
  }
  return st;
}

// Host emulator of the kernels' arithmetic: the bf16 products of the three virtual channel blocks
// accumulated in f32 in K order (tap-major, then the downsample columns), then the split epilogue
// v = acc + bias (+ res_hi + res_lo), ReLU, hi = bf16(v), lo = bf16(v - hi).  The mutations are
// the slips the GPU cases have to catch.
enum Mutation {
  kNone = 0,
  kDropLoStep,   // (a) x_lo w1 dropped for one 32-channel k-step of one tap
  kBlock2Lo,     // (b) virtual block 2 reads the lo block (split_chan off by one block)
  kNoResLo,      // (c) the residual's lo block ignored
  kZeroLo,       // (d) y_lo stored as 0
  kPadNeighbour  // (e) a padding tap reads the neighbouring row instead of zero
};

inline std::vector<u16> emulate(const Case& c, bool res, bool relu, Mutation mut = kNone) {
  const Shape& s = c.s;
  const int C = s.C, D = s.Cds, taps = s.k * s.k;
  std::vector<u16> y((size_t)c.M() * 2 * s.Cout);
  std::vector<float> xv(c.x.size()), x2v(c.x2.size()), wv(c.w.size());
  for (size_t i = 0; i < xv.size(); ++i) xv[i] = bf2f(c.x[i]);
  for (size_t i = 0; i < x2v.size(); ++i) x2v[i] = bf2f(c.x2[i]);
  for (size_t i = 0; i < wv.size(); ++i) wv[i] = bf2f(c.w[i]);
  const int drop_tap = taps / 2;
  for (int n = 0; n < s.N; ++n)
    for (int oh = 0; oh < c.Ho; ++oh)
      for (int ow = 0; ow < c.Wo; ++ow) {
        const size_t pix = ((size_t)n * c.Ho + oh) * c.Wo + ow;
        for (int o = 0; o < s.Cout; ++o) {
          float acc = 0.f;
          for (int t = 0; t <= taps; ++t) {
            const float* xp;
            int ch;
            if (t < taps) {
              int ih = oh * s.stride - s.pad + t / s.k;
              const int iw = ow * s.stride - s.pad + t % s.k;
              if (iw < 0 || iw >= s.W) continue;
              if (ih < 0 || ih >= s.H) {
                if (mut != kPadNeighbour) continue;
                ih = ih < 0 ? 0 : s.H - 1;
              }
              xp = xv.data() + (((size_t)n * s.H + ih) * s.W + iw) * 2 * C;
              ch = C;
            } else {
              if (!D) continue;
              xp = x2v.data() + (((size_t)n * c.H2 + oh * s.s2) * c.W2 + ow * s.s2) * 2 * D;
              ch = D;
            }
            const float* wp = wv.data() + (size_t)o * c.K + (t < taps ? (size_t)t * 3 * C : (size_t)c.K1);
            for (int v = 0; v < 3 * ch; ++v) {  // virtual channel v: block v / ch
              int phys = v >= 2 * ch ? v - 2 * ch : v;  // split_chan
              if (mut == kBlock2Lo && v >= 2 * ch) phys = v - ch;
              if (mut == kDropLoStep && t == drop_tap && v >= ch && v < ch + 32) continue;
              acc += xp[phys] * wp[v];  // a product of two bf16 is exact in f32
            }
          }
          float v = acc + c.bias[o];
          if (res) {
            const float h = bf2f(c.res[pix * 2 * s.Cout + o]), l = bf2f(c.res[pix * 2 * s.Cout + s.Cout + o]);
            v += mut == kNoResLo ? h : h + l;
          }
          if (relu) v = fmaxf(v, 0.f);
          const u16 hb = f2bf(v);
          y[pix * 2 * s.Cout + o] = hb;
          y[pix * 2 * s.Cout + s.Cout + o] = mut == kZeroLo ? (u16)0 : f2bf(v - bf2f(hb));
        }
      }
  return y;
}

}  // namespace x3
