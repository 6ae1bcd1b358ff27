// Layer-level check of the implicit-GEMM conv against a naive CPU conv (double accum).
// Build: hipcc --offload-arch=gfx950 -O2 -I include -I <pkg>/csrc conv_check.cpp -L<pkg> -leosv
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <unistd.h>
#include "common.h"
#include "x3_ref.h"
#include "bf16_ref.h"
#include "f32_ref.h"

using namespace eosv;

static float frand(unsigned& s) { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.f - 1.f; }

// ds_cin > 0: a fused 1x1 stride-2 downsample (ConvArgs::x2) reads x2 [N][2H][2W][ds_cin] into K
// columns [K1, K1 + ds_cin).  tol: bound on |err| / (1 + sum of |terms|) -- f32 rounding of a
// K-term dot product grows with the magnitudes summed, not with the (cancelling) result.
// kcm: device weights in the chunk-major K order (cin / 32, kh, kw, cin % 32) (ConvArgs::kcm, f32)
static int check(int N, int H, int W, int Cin, int Cout, int K, int stride, int pad, bool stem, bool res, bool relu,
                 int ds_cin = 0, double tol = 1e-5, bool kcm = false) {
  // stem: dense padded RGB input [N][H+2p][Wp][3] (zero borders), K = [kh][24] padded to 16
  const int KWp = stem ? 8 : K, Cinp = Cin;
  const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
  const int K1 = stem ? (K * 24 + 15) / 16 * 16 : K * KWp * Cinp;
  const int Kd = K1 + ds_cin;
  const int H2 = 2 * Ho, W2 = 2 * Wo;
  const int Hx = stem ? H + 2 * pad : H, Wx = stem ? stem_row_pixels(W, pad) : W, off = stem ? pad : 0;
  unsigned s = 12345;
  std::vector<float> x(stem ? stem_input_elems(N, H, W, pad) : (size_t)N * H * W * Cinp, 0.f),
      w((size_t)Cout * Kd, 0.f), b(Cout), r((size_t)N * Ho * Wo * Cout);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int c = 0; c < Cin; ++c) x[(((size_t)n * Hx + i + off) * Wx + j + off) * Cinp + c] = frand(s);
  for (int o = 0; o < Cout; ++o)
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw)
        for (int c = 0; c < Cin; ++c) w[(size_t)o * Kd + (kh * KWp + kw) * Cinp + c] = frand(s);
  for (auto& v : b) v = frand(s);
  for (auto& v : r) v = frand(s);
  std::vector<float> x2((size_t)N * H2 * W2 * ds_cin);
  for (auto& v : x2) v = frand(s);
  for (int o = 0; o < Cout; ++o)
    for (int c = 0; c < ds_cin; ++c) w[(size_t)o * Kd + K1 + c] = frand(s);
  float* dx2 = nullptr;
  if (ds_cin) {
    hipMalloc(&dx2, x2.size() * 4);
    hipMemcpy(dx2, x2.data(), x2.size() * 4, hipMemcpyHostToDevice);
  }
  float *dx, *dw, *db, *dr, *dy;
  hipMalloc(&dx, x.size() * 4); hipMalloc(&dw, w.size() * 4); hipMalloc(&db, b.size() * 4);
  hipMalloc(&dr, r.size() * 4); hipMalloc(&dy, r.size() * 4);
  hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice);
  std::vector<float> wd = w;
  if (kcm)
    for (int o = 0; o < Cout; ++o)
      for (int t = 0; t < K * K; ++t)
        for (int c = 0; c < Cin; ++c)
          wd[(size_t)o * Kd + ((c / 32) * K * K + t) * 32 + c % 32] = w[(size_t)o * Kd + t * Cinp + c];
  hipMemcpy(dw, wd.data(), wd.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(db, b.data(), b.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dr, r.data(), r.size() * 4, hipMemcpyHostToDevice);
  ConvArgs a{};
  a.kcm = kcm ? 32 : 0;
  a.x = dx; a.w = dw; a.bias = db; a.res = res ? dr : nullptr; a.y = dy;
  a.N = N; a.H = H; a.W = W; a.Cin = Cinp; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
  a.KH = K; a.KW = K; a.KWp = KWp; a.stride = stride; a.pad = pad; a.K = Kd; a.relu = relu;
  void* dz; hipMalloc(&dz, 256); hipMemset(dz, 0, 256); a.zero = dz;
  if (ds_cin) {
    a.x2 = dx2; a.H2 = H2; a.W2 = W2; a.Cin2 = ds_cin; a.stride2 = 2; a.K1 = K1;
  }
  int rc = launch_conv_f32(a, 0);
  hipDeviceSynchronize();
  std::vector<float> y(r.size());
  hipMemcpy(y.data(), dy, y.size() * 4, hipMemcpyDeviceToHost);
  double maxerr = 0, maxref = 0; long bad = 0;
  for (int n = 0; n < N; ++n)
    for (int oh = 0; oh < Ho; ++oh)
      for (int ow = 0; ow < Wo; ++ow)
        for (int o = 0; o < Cout; ++o) {
          double acc = b[o], sabs = fabs(b[o]);
          for (int kh = 0; kh < K; ++kh)
            for (int kw = 0; kw < K; ++kw) {
              int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
              if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
              for (int c = 0; c < Cin; ++c) {
                const double t = (double)x[(((size_t)n * Hx + ih + off) * Wx + iw + off) * Cinp + c] *
                                 w[(size_t)o * Kd + (kh * KWp + kw) * Cinp + c];
                acc += t;
                sabs += fabs(t);
              }
            }
          for (int c = 0; c < ds_cin; ++c) {
            const double t = (double)x2[(((size_t)n * H2 + 2 * oh) * W2 + 2 * ow) * ds_cin + c] * w[(size_t)o * Kd + K1 + c];
            acc += t;
            sabs += fabs(t);
          }
          size_t oi = (((size_t)n * Ho + oh) * Wo + ow) * Cout + o;
          if (res) acc += r[oi], sabs += fabs(r[oi]);
          if (relu && acc < 0) acc = 0;
          double e = fabs(acc - y[oi]);
          if (!(e <= tol * (1 + sabs))) { if (bad < 5) printf("  bad n%d oh%d ow%d o%d ref %f got %f\n", n, oh, ow, o, acc, y[oi]); ++bad; }
          maxerr = fmax(maxerr, e); maxref = fmax(maxref, fabs(acc));
        }
  printf("%s f32 N%d H%d W%d Cin%d Cout%d K%d s%d p%d res%d relu%d ds%d kcm%d rc=%d maxerr %.3e (maxref %.3e) bad %ld\n",
         bad || rc ? "FAIL" : "ok  ", N, H, W, Cin, Cout, K, stride, pad, res, relu, ds_cin, kcm, rc, maxerr, maxref, bad);
  hipFree(dx); hipFree(dw); hipFree(db); hipFree(dr); hipFree(dy);
  if (dx2) hipFree(dx2);
  hipFree(dz);
  return bad || rc ? 1 : 0;
}

static unsigned short f2bf(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
static float bf2f(unsigned short v) {
  unsigned u = (unsigned)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// bf16 conv through launch_conv_bf16 (stage-1 3x3 shapes take the row-strip kernel, Cout >= 128
// the phased 8-wave kernel); reference in double on the bf16-rounded operands, checked on images
// `checked` only
// the launcher check_bf16 goes through: launch_conv_bf16 (its default dispatch), or one kernel directly
static int (*g_bf16_launch)(const ConvArgs&, hipStream_t) = launch_conv_bf16;
static int check_bf16(int N, int H, int W, int Cin, int Cout, int k, int stride, int pad, bool res, bool relu,
                      bool kcm = false) {
  const int K = k * k * Cin;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  unsigned s = 777;
  std::vector<unsigned short> x((size_t)N * H * W * Cin), w((size_t)Cout * K), r((size_t)N * Ho * Wo * Cout);
  std::vector<float> b(Cout);
  for (auto& v : x) v = f2bf(frand(s));
  for (auto& v : w) v = f2bf(frand(s) * 0.1f);
  for (auto& v : r) v = f2bf(frand(s));
  for (auto& v : b) v = frand(s);
  unsigned short *dx, *dw, *dr, *dy;
  float* db;
  void* dz;
  hipMalloc(&dx, x.size() * 2); hipMalloc(&dw, w.size() * 2); hipMalloc(&dr, r.size() * 2);
  hipMalloc(&dy, r.size() * 2); hipMalloc(&db, Cout * 4); hipMalloc(&dz, 256); hipMemset(dz, 0, 256);
  hipMemcpy(dx, x.data(), x.size() * 2, hipMemcpyHostToDevice);
  {
    // kcm: device weights in K order (cin / 64, kh, kw, cin % 64) (ConvArgs::kcm)
    std::vector<unsigned short> wd(w.size());
    for (int o = 0; o < Cout; ++o)
      for (int t = 0; t < k * k; ++t)
        for (int c = 0; c < Cin; ++c)
          wd[(size_t)o * K + (kcm ? ((c / 64) * k * k + t) * 64 + c % 64 : t * Cin + c)] = w[(size_t)o * K + t * Cin + c];
    hipMemcpy(dw, wd.data(), wd.size() * 2, hipMemcpyHostToDevice);
  }
  hipMemcpy(dr, r.data(), r.size() * 2, hipMemcpyHostToDevice);
  hipMemcpy(db, b.data(), Cout * 4, hipMemcpyHostToDevice);
  hipMemset(dy, 0xff, r.size() * 2);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.res = res ? dr : nullptr; a.y = dy;
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
  a.KH = k; a.KW = k; a.KWp = k; a.stride = stride; a.pad = pad; a.K = K; a.relu = relu; a.zero = dz;
  a.xcd = 1;
  a.kcm = kcm;
  a.xs = Cin;  // dense pixels (launch_conv_bf16 sets it itself)
  const int rc = g_bf16_launch(a, 0);
  hipDeviceSynchronize();
  std::vector<unsigned short> y(r.size());
  hipMemcpy(y.data(), dy, y.size() * 2, hipMemcpyDeviceToHost);
  const int checked[4] = {0, N > 1 ? 1 : 0, N > 2 ? N - 2 : 0, N - 1};
  double maxerr = 0;
  long bad = 0;
  for (int ci = 0; ci < 4; ++ci) {
    const int n = checked[ci];
    if (ci > 0 && n == checked[ci - 1]) continue;
    for (int oh = 0; oh < Ho; ++oh)
      for (int ow = 0; ow < Wo; ++ow)
        for (int o = 0; o < Cout; ++o) {
          double acc = b[o];
          for (int kh = 0; kh < k; ++kh)
            for (int kw = 0; kw < k; ++kw) {
              const int ih = oh * stride - pad + kh, iw = ow * stride - pad + kw;
              if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
              for (int c = 0; c < Cin; ++c)
                acc += (double)bf2f(x[(((size_t)n * H + ih) * W + iw) * Cin + c]) *
                       bf2f(w[(size_t)o * K + (kh * k + kw) * Cin + c]);
            }
          const size_t oi = (((size_t)n * Ho + oh) * Wo + ow) * Cout + o;
          if (res) acc += bf2f(r[oi]);
          if (relu && acc < 0) acc = 0;
          const double e = fabs(acc - bf2f(y[oi]));
          if (!(e <= 1e-2 * (1 + fabs(acc)))) {
            if (bad < 5) printf("  bad n%d oh%d ow%d o%d ref %f got %f\n", n, oh, ow, o, acc, bf2f(y[oi]));
            ++bad;
          }
          maxerr = fmax(maxerr, e);
        }
  }
  printf("%s bf16 N%d H%d W%d Cin%d Cout%d k%d s%d p%d res%d relu%d kcm%d rc=%d maxerr %.3e bad %ld\n",
         bad ? "FAIL" : "ok  ", N, H, W, Cin, Cout, k, stride, pad, res, relu, kcm, rc, maxerr, bad);
  hipFree(dx); hipFree(dw); hipFree(dr); hipFree(dy); hipFree(db); hipFree(dz);
  return bad || rc ? 1 : 0;
}

// fused bf16 stem (7x7/2 p3, 3 -> 64) + bias + ReLU + maxpool 3x3/2 p1 vs a double reference
// on the same bf16 operands (bf16 rounding of the stem output before the pool, as the kernel)
static int check_stem_pool(int N, int H, int W, bool direct = false) {
  const int pad = 3, Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  const int Hs = (H + 6 - 7) / 2 + 1, Ws = (W + 6 - 7) / 2 + 1;
  const int Hq = (Hs - 1) / 2 + 1, Wq = (Ws - 1) / 2 + 1;
  unsigned s = 4242;
  std::vector<unsigned short> x(stem_input_elems(N, H, W, pad) + 256, 0), w(64 * 192, 0);
  std::vector<float> b(64);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int c = 0; c < 3; ++c) x[128 / 2 + (((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c] = f2bf(frand(s));
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int kw = 0; kw < 7; ++kw)
        for (int c = 0; c < 3; ++c) w[o * 192 + kh * 24 + kw * 3 + c] = f2bf(frand(s) * 0.2f);
  for (auto& v : b) v = frand(s) * 0.5f;
  unsigned short *dx, *dw, *dy;
  float* db;
  const size_t ny = (size_t)N * Hq * Wq * 64;
  hipMalloc(&dx, x.size() * 2); hipMalloc(&dw, w.size() * 2); hipMalloc(&dy, ny * 2); hipMalloc(&db, 64 * 4);
  hipMemcpy(dx, x.data(), x.size() * 2, hipMemcpyHostToDevice);
  hipMemcpy(dw, w.data(), w.size() * 2, hipMemcpyHostToDevice);
  hipMemcpy(db, b.data(), 64 * 4, hipMemcpyHostToDevice);
  hipMemset(dy, 0xff, ny * 2);
  // direct: the kernel reads f32 NCHW frames (the same values, exactly representable in bf16)
  std::vector<float> fr((size_t)N * 3 * H * W);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int c = 0; c < 3; ++c)
          fr[(((size_t)n * 3 + c) * H + i) * W + j] = bf2f(x[128 / 2 + (((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c]);
  float* dfr;
  hipMalloc(&dfr, fr.size() * 4);
  hipMemcpy(dfr, fr.data(), fr.size() * 4, hipMemcpyHostToDevice);
  const int rc = direct ? launch_stem_pool_bf16(nullptr, N, H, W, dw, db, dy, 0, dfr)
                        : launch_stem_pool_bf16(dx + 64, N, H, W, dw, db, dy, 0);  // 128 B front slack
  hipDeviceSynchronize();
  std::vector<unsigned short> y(ny);
  hipMemcpy(y.data(), dy, ny * 2, hipMemcpyDeviceToHost);
  std::vector<float> st((size_t)Hs * Ws * 64);
  long bad = 0;
  double maxerr = 0;
  for (int n = 0; n < N; ++n) {
    for (int sy = 0; sy < Hs; ++sy)
      for (int sx = 0; sx < Ws; ++sx)
        for (int o = 0; o < 64; ++o) {
          double acc = b[o];
          for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 7; ++kw)
              for (int c = 0; c < 3; ++c)
                acc += (double)bf2f(x[64 + (((size_t)n * Hp + 2 * sy + kh) * Wp + 2 * sx + kw) * 3 + c]) *
                       bf2f(w[o * 192 + kh * 24 + kw * 3 + c]);
          st[((size_t)sy * Ws + sx) * 64 + o] = bf2f(f2bf((float)(acc > 0 ? acc : 0)));
        }
    for (int py = 0; py < Hq; ++py)
      for (int px = 0; px < Wq; ++px)
        for (int o = 0; o < 64; ++o) {
          float m = -INFINITY;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int sy = 2 * py + dy, sx = 2 * px + dx;
              if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) m = fmaxf(m, st[((size_t)sy * Ws + sx) * 64 + o]);
            }
          const float got = bf2f(y[(((size_t)n * Hq + py) * Wq + px) * 64 + o]);
          const double e = fabs(got - m);
          if (e > 1e-2 * (1 + fabs(m))) {
            if (bad < 5) printf("  bad n%d py%d px%d o%d ref %f got %f\n", n, py, px, o, m, got);
            ++bad;
          }
          maxerr = fmax(maxerr, e);
        }
  }
  printf("%s stem_pool bf16%s N%d H%d W%d rc=%d maxerr %.3e bad %ld\n", bad ? "FAIL" : "ok  ", direct ? " direct" : "",
         N, H, W, rc, maxerr, bad);
  hipFree(dx); hipFree(dw); hipFree(dy); hipFree(db); hipFree(dfr);
  return bad || rc ? 1 : 0;
}


// EOSV_F32X3 split-bf16 fused stem vs a double reference on the f32 operands: the kernel splits
// frames and weights into bf16 hi + lo and drops lo.lo, so hi + lo of its output must be within
// ~1e-4 relative of the exact value (the north star's f32 bound)
static int check_stem_pool_x3(int N, int H, int W) {
  const int Hs = (H + 6 - 7) / 2 + 1, Ws = (W + 6 - 7) / 2 + 1;
  const int Hq = (Hs - 1) / 2 + 1, Wq = (Ws - 1) / 2 + 1;
  unsigned s = 777;
  std::vector<float> fr((size_t)N * 3 * H * W), wf(64 * 192, 0.f), b(64);
  for (auto& v : fr) v = frand(s) * 2.f;
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int kw = 0; kw < 7; ++kw)
        for (int c = 0; c < 3; ++c) wf[o * 192 + kh * 24 + kw * 3 + c] = frand(s) * 0.2f;
  for (auto& v : b) v = frand(s) * 0.5f;
  std::vector<unsigned short> w2(2 * 64 * 192);
  for (int i = 0; i < 64 * 192; ++i) {
    w2[i] = f2bf(wf[i]);
    w2[64 * 192 + i] = f2bf(wf[i] - bf2f(w2[i]));
  }
  float *dfr, *db;
  unsigned short *dw, *dy;
  const size_t ny = (size_t)N * Hq * Wq * 128;  // split layout: (hi 64 | lo 64) per pixel
  hipMalloc(&dfr, fr.size() * 4); hipMalloc(&dw, w2.size() * 2); hipMalloc(&dy, ny * 2); hipMalloc(&db, 64 * 4);
  hipMemcpy(dfr, fr.data(), fr.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dw, w2.data(), w2.size() * 2, hipMemcpyHostToDevice);
  hipMemcpy(db, b.data(), 64 * 4, hipMemcpyHostToDevice);
  hipMemset(dy, 0xff, ny * 2);
  const int rc = launch_stem_pool_x3(dfr, N, H, W, dw, db, dy, 0);
  hipDeviceSynchronize();
  std::vector<unsigned short> y(ny);
  hipMemcpy(y.data(), dy, ny * 2, hipMemcpyDeviceToHost);
  std::vector<double> st((size_t)Hs * Ws * 64);
  long bad = 0;
  double maxerr = 0, maxref = 0;
  for (int n = 0; n < N; ++n) {
    for (int sy = 0; sy < Hs; ++sy)
      for (int sx = 0; sx < Ws; ++sx)
        for (int o = 0; o < 64; ++o) {
          double acc = b[o];
          for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 7; ++kw) {
              const int iy = 2 * sy + kh - 3, ix = 2 * sx + kw - 3;
              if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
              for (int c = 0; c < 3; ++c)
                acc += (double)fr[(((size_t)n * 3 + c) * H + iy) * W + ix] * wf[o * 192 + kh * 24 + kw * 3 + c];
            }
          st[((size_t)sy * Ws + sx) * 64 + o] = acc > 0 ? acc : 0;
        }
    for (int py = 0; py < Hq; ++py)
      for (int px = 0; px < Wq; ++px)
        for (int o = 0; o < 64; ++o) {
          double m = -INFINITY;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int sy = 2 * py + dy, sx = 2 * px + dx;
              if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) m = fmax(m, st[((size_t)sy * Ws + sx) * 64 + o]);
            }
          const size_t base = (((size_t)n * Hq + py) * Wq + px) * 128 + o;
          const double got = (double)bf2f(y[base]) + bf2f(y[base + 64]);
          // lo is the rounding residual of hi: at most half an ulp of hi (2^-9 relative)
          const bool dup = fabs(bf2f(y[base + 64])) <= fabs(bf2f(y[base])) * (1.0 / 256);
          const double e = fabs(got - m);
          maxref = fmax(maxref, fabs(m));
          if (e > 1e-4 * (1 + fabs(m)) || !dup) {
            if (bad < 5) printf("  bad n%d py%d px%d o%d ref %f got %f dup %d\n", n, py, px, o, m, got, (int)dup);
            ++bad;
          }
          maxerr = fmax(maxerr, e);
        }
  }
  printf("%s stem_pool x3 N%d H%d W%d rc=%d maxerr %.3e (maxref %.3e) bad %ld\n", bad ? "FAIL" : "ok  ", N, H, W, rc,
         maxerr, maxref, bad);
  hipFree(dfr); hipFree(dw); hipFree(dy); hipFree(db);
  return bad || rc ? 1 : 0;
}

// fused f32 stem + shift + ReLU + maxpool vs a double reference on the same f32 operands
// (weights in the uploaded [64][176] = [kh 7][24] + 8 layout)
static int check_stem_pool_f32(int N, int H, int W, int every = 1) {
  const int pad = 3, Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  const int Hs = (H + 6 - 7) / 2 + 1, Ws = (W + 6 - 7) / 2 + 1;
  const int Hq = (Hs - 1) / 2 + 1, Wq = (Ws - 1) / 2 + 1;
  unsigned s = 5151;
  std::vector<float> x(stem_input_elems(N, H, W, pad) + 64, 0.f), w(64 * 176, 0.f), b(64);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int c = 0; c < 3; ++c) x[(((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c] = frand(s);
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int kw = 0; kw < 7; ++kw)
        for (int c = 0; c < 3; ++c) w[o * 176 + kh * 24 + kw * 3 + c] = frand(s) * 0.2f;
  for (auto& v : b) v = frand(s) * 0.5f;
  float *dx, *dw, *dy, *db;
  const size_t ny = (size_t)N * Hq * Wq * 64;
  hipMalloc(&dx, x.size() * 4); hipMalloc(&dw, w.size() * 4); hipMalloc(&dy, ny * 4); hipMalloc(&db, 64 * 4);
  hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(db, b.data(), 64 * 4, hipMemcpyHostToDevice);
  hipMemset(dy, 0xff, ny * 4);
  const int rc = launch_stem_pool_f32(dx, N, H, W, dw, db, dy, 0);
  hipDeviceSynchronize();
  std::vector<float> y(ny);
  hipMemcpy(y.data(), dy, ny * 4, hipMemcpyDeviceToHost);
  std::vector<double> st((size_t)Hs * Ws * 64);
  long bad = 0;
  double maxerr = 0;
  for (int n = 0; n < N; ++n) {
    if (n % every && n != N - 1) continue;  // large N: a sample of the images (every band count)
    for (int sy = 0; sy < Hs; ++sy)
      for (int sx = 0; sx < Ws; ++sx)
        for (int o = 0; o < 64; ++o) {
          double acc = b[o];
          for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 7; ++kw)
              for (int c = 0; c < 3; ++c)
                acc += (double)x[(((size_t)n * Hp + 2 * sy + kh) * Wp + 2 * sx + kw) * 3 + c] * w[o * 176 + kh * 24 + kw * 3 + c];
          st[((size_t)sy * Ws + sx) * 64 + o] = acc > 0 ? acc : 0;
        }
    for (int py = 0; py < Hq; ++py)
      for (int px = 0; px < Wq; ++px)
        for (int o = 0; o < 64; ++o) {
          double m = -INFINITY;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int sy = 2 * py + dy, sx = 2 * px + dx;
              if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) m = fmax(m, st[((size_t)sy * Ws + sx) * 64 + o]);
            }
          const float got = y[(((size_t)n * Hq + py) * Wq + px) * 64 + o];
          const double e = fabs(got - m);
          if (!(e <= 1e-5 * (1 + fabs(m)))) {
            if (bad < 5) printf("  bad n%d py%d px%d o%d ref %f got %f\n", n, py, px, o, m, got);
            ++bad;
          }
          maxerr = fmax(maxerr, e);
        }
  }
  // DIRECT (the f32 NCHW frames, no pack): the same values, so bit-identical to the pack run
  long dbad = 0;
  int rc2 = 0;
  const bool direct = stem_pool_f32_direct_ok(H, W);
  if (direct) {
    std::vector<float> fr((size_t)N * 3 * H * W);
    for (int n = 0; n < N; ++n)
      for (int c = 0; c < 3; ++c)
        for (int i = 0; i < H; ++i)
          for (int j = 0; j < W; ++j)
            fr[(((size_t)n * 3 + c) * H + i) * W + j] = x[(((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c];
    float *dfr, *dy2;
    hipMalloc(&dfr, fr.size() * 4); hipMalloc(&dy2, ny * 4);
    hipMemcpy(dfr, fr.data(), fr.size() * 4, hipMemcpyHostToDevice);
    hipMemset(dy2, 0xff, ny * 4);
    rc2 = launch_stem_pool_f32(nullptr, N, H, W, dw, db, dy2, 0, false, nullptr, dfr);
    hipDeviceSynchronize();
    std::vector<float> y2(ny);
    hipMemcpy(y2.data(), dy2, ny * 4, hipMemcpyDeviceToHost);
    for (size_t i = 0; i < ny; ++i) dbad += memcmp(&y[i], &y2[i], 4) != 0;
    hipFree(dfr); hipFree(dy2);
  }
  printf("%s stem_pool f32 N%d H%d W%d rc=%d maxerr %.3e bad %ld%s\n", bad || dbad || rc2 ? "FAIL" : "ok  ", N, H, W,
         rc, maxerr, bad, direct ? (dbad || rc2 ? " direct differs" : " direct identical") : "");
  hipFree(dx); hipFree(dw); hipFree(dy); hipFree(db);
  return bad || rc || dbad || rc2 ? 1 : 0;
}

// bottleneck 1x1 pair (pair1x1_bf16.hip) vs the unfused pair through launch_conv_bf16: conv3
// (1x1 64 -> 256, + residual or + a folded stride-1 downsample) then the next block's conv1
// (1x1 256 -> c1), both with folded-BN shifts and ReLU.  Same K order, same epilogue order:
// both maps must be bit-identical.
static int check_pair(int N, int H, int W, int c1, bool ds) {
  const long long M = (long long)N * H * W;
  const int K3 = ds ? 128 : 64;
  unsigned s = 777;
  auto fill = [&](std::vector<unsigned short>& v, float scale) {
    for (auto& e : v) e = f2bf(frand(s) * scale);
  };
  std::vector<unsigned short> x(M * 64), x2(ds ? M * 64 : 1), res(M * 256), w3(256 * K3), w1((size_t)c1 * 256);
  fill(x, 1.f); fill(x2, 1.f); fill(res, 1.f); fill(w3, 0.125f); fill(w1, 0.0625f);
  std::vector<float> b3(256), b1(c1);
  for (auto& v : b3) v = frand(s) * 0.5f;
  for (auto& v : b1) v = frand(s) * 0.5f;
  auto up = [](const void* p, size_t n) { void* d; hipMalloc(&d, n); hipMemcpy(d, p, n, hipMemcpyHostToDevice); return d; };
  void *dx = up(x.data(), x.size() * 2), *dx2 = up(x2.data(), x2.size() * 2), *dr = up(res.data(), res.size() * 2);
  void *dw3 = up(w3.data(), w3.size() * 2), *dw1 = up(w1.data(), w1.size() * 2);
  float *db3 = (float*)up(b3.data(), b3.size() * 4), *db1 = (float*)up(b1.data(), b1.size() * 4);
  void *y0, *z0, *y1, *z1, *dz;
  hipMalloc(&y0, M * 512); hipMalloc(&y1, M * 512); hipMalloc(&z0, M * c1 * 2); hipMalloc(&z1, M * c1 * 2);
  hipMalloc(&dz, 256); hipMemset(dz, 0, 256);
  // unfused: conv3 (+ residual | + downsample K columns), then conv1
  ConvArgs a{};
  a.x = dx; a.w = dw3; a.bias = db3; a.res = ds ? nullptr : dr; a.y = y0;
  a.N = N; a.H = H; a.W = W; a.Cin = 64; a.Ho = H; a.Wo = W; a.Cout = 256;
  a.KH = a.KW = a.KWp = 1; a.stride = 1; a.pad = 0; a.K = K3; a.relu = 1; a.zero = dz; a.xcd = 1;
  if (ds) { a.x2 = dx2; a.H2 = H; a.W2 = W; a.Cin2 = 64; a.stride2 = 1; a.K1 = 64; }
  int rc = launch_conv_bf16(a, 0);
  ConvArgs b{};
  b.x = y0; b.w = dw1; b.bias = db1; b.res = nullptr; b.y = z0;
  b.N = N; b.H = H; b.W = W; b.Cin = 256; b.Ho = H; b.Wo = W; b.Cout = c1;
  b.KH = b.KW = b.KWp = 1; b.stride = 1; b.pad = 0; b.K = 256; b.relu = 1; b.zero = dz; b.xcd = 1;
  rc |= launch_conv_bf16(b, 0);
  Pair1x1Args p{};
  p.x = dx; p.x2 = ds ? dx2 : nullptr; p.res = ds ? nullptr : dr; p.w3 = dw3; p.b3 = db3; p.w1 = dw1; p.b1 = db1;
  p.y = y1; p.z = z1; p.M = M; p.c1 = c1; p.cds = ds ? 64 : 0;
  rc |= launch_pair1x1_bf16(p, 0);
  hipDeviceSynchronize();
  std::vector<unsigned short> hy0(M * 256), hy1(M * 256), hz0(M * c1), hz1(M * c1);
  hipMemcpy(hy0.data(), y0, M * 512, hipMemcpyDeviceToHost); hipMemcpy(hy1.data(), y1, M * 512, hipMemcpyDeviceToHost);
  hipMemcpy(hz0.data(), z0, M * c1 * 2, hipMemcpyDeviceToHost); hipMemcpy(hz1.data(), z1, M * c1 * 2, hipMemcpyDeviceToHost);
  long bady = 0, badz = 0;
  double maxd = 0;
  for (size_t i = 0; i < hy0.size(); ++i)
    if (hy0[i] != hy1[i]) ++bady, maxd = std::max(maxd, (double)fabs(bf2f(hy0[i]) - bf2f(hy1[i])));
  for (size_t i = 0; i < hz0.size(); ++i)
    if (hz0[i] != hz1[i]) ++badz, maxd = std::max(maxd, (double)fabs(bf2f(hz0[i]) - bf2f(hz1[i])));
  // the unfused maps themselves against double on the bf16 operands (a few pixels)
  double maxerr = 0;
  for (long long m = 0; m < M; m += M / 7 + 1)
    for (int o = 0; o < 256; o += 5) {
      double acc = b3[o];
      for (int k = 0; k < 64; ++k) acc += (double)bf2f(x[m * 64 + k]) * bf2f(w3[o * K3 + k]);
      if (ds) for (int k = 0; k < 64; ++k) acc += (double)bf2f(x2[m * 64 + k]) * bf2f(w3[o * K3 + 64 + k]);
      else acc += bf2f(res[m * 256 + o]);
      acc = std::max(acc, 0.0);
      maxerr = std::max(maxerr, fabs(acc - bf2f(hy0[m * 256 + o])) / (1.0 + fabs(acc)));
    }
  const bool fail = rc || bady || badz || maxerr > 1e-2;
  printf("%s pair1x1 bf16 N%d H%d W%d c1 %d ds%d rc=%d differing y %ld z %ld (max %.3e) unfused maxerr %.3e\n",
         fail ? "FAIL" : "ok  ", N, H, W, c1, ds ? 1 : 0, rc, bady, badz, maxd, maxerr);
  for (void* q : {dx, dx2, dr, dw3, dw1, (void*)db3, (void*)db1, y0, y1, z0, z1, dz}) hipFree(q);
  return fail ? 1 : 0;
}

// wide bottleneck pair (pairw_bf16.hip, stages 2-3) vs the unfused conv3 (1x1 cmid -> cexp +
// residual) -> conv1 (1x1 cexp -> c1) through launch_conv_bf16: both maps bit-identical.  M
// need not be a multiple of the 128-pixel round: the tail round runs on the buffers' padding
// (filled with NaN here: no valid output may depend on it), and it is repeated REPS times (its
// results changed from run to run while it masked the padding with out-of-range buffer ops).
// every CU's LDS filled with 0xff (NaN in bf16): a kernel reading LDS words it did not write
__global__ __launch_bounds__(256) void lds_poison_k() {
  __shared__ unsigned lds[160 * 1024 / 4];
  volatile unsigned* q = lds;
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) q[i] = 0xffffffffu;
}

// inplace: y = res (as the engine runs the pair: Y lands in the residual's buffer); stress: before
// every repetition 1 GiB is written (cold caches) and the LDS poisoned
static int check_pairw(int N, int H, int W, int cmid, int cexp, int c1, int cds = 0, bool inplace = false,
                       bool stress = false, int reps = 0) {
  // cds > 0: block 0 of a stage, conv3 + the folded stride-2 downsample reading x2 [N][2H][2W][cds]
  // (ragged: 2H - 1 when odd sizes are asked for through H2/W2 below), no residual
  const long long M = (long long)N * H * W;
  const int H2 = 2 * H, W2 = 2 * W;
  const int K3 = cmid + cds;
  unsigned s = 4242 + cmid + c1;
  auto fill = [&](std::vector<unsigned short>& v, float scale) {
    for (auto& e : v) e = f2bf(frand(s) * scale);
  };
  const long long tile = pairw_tile(cmid, c1, cds);  // 128 pixels per round
  const long long Mp = (M + tile - 1) / tile * tile;  // padded to whole rounds
  std::vector<unsigned short> x(Mp * cmid, 0x7fc0), res(Mp * cexp, 0x7fc0), w3((size_t)cexp * K3), w1((size_t)c1 * cexp);
  std::vector<unsigned short> x2(cds ? (size_t)N * H2 * W2 * cds : 1);
  {
    std::vector<unsigned short> xv(M * cmid), rv(M * cexp);
    fill(xv, 1.f); fill(rv, 1.f);
    std::copy(xv.begin(), xv.end(), x.begin());
    std::copy(rv.begin(), rv.end(), res.begin());
  }
  fill(w3, 0.125f); fill(w1, 0.0625f); fill(x2, 1.f);
  std::vector<float> b3(cexp), b1(c1);
  for (auto& v : b3) v = frand(s) * 0.5f;
  for (auto& v : b1) v = frand(s) * 0.5f;
  auto up = [](const void* p, size_t n) { void* d; hipMalloc(&d, n); hipMemcpy(d, p, n, hipMemcpyHostToDevice); return d; };
  void *dx = up(x.data(), x.size() * 2), *dr = up(res.data(), res.size() * 2), *dx2 = up(x2.data(), x2.size() * 2);
  void *dw3 = up(w3.data(), w3.size() * 2), *dw1 = up(w1.data(), w1.size() * 2);
  float *db3 = (float*)up(b3.data(), b3.size() * 4), *db1 = (float*)up(b1.data(), b1.size() * 4);
  void *y0, *z0, *y1, *z1, *dz;
  hipMalloc(&y0, M * cexp * 2); hipMalloc(&y1, Mp * cexp * 2); hipMalloc(&z0, M * c1 * 2); hipMalloc(&z1, Mp * c1 * 2);
  hipMalloc(&dz, 256); hipMemset(dz, 0, 256);
  ConvArgs a{};
  a.x = dx; a.w = dw3; a.bias = db3; a.res = cds ? nullptr : dr; a.y = y0;
  a.N = N; a.H = H; a.W = W; a.Cin = cmid; a.Ho = H; a.Wo = W; a.Cout = cexp;
  a.KH = a.KW = a.KWp = 1; a.stride = 1; a.pad = 0; a.K = K3; a.relu = 1; a.zero = dz; a.xcd = 1;
  if (cds) { a.x2 = dx2; a.H2 = H2; a.W2 = W2; a.Cin2 = cds; a.stride2 = 2; a.K1 = cmid; }
  int rc = launch_conv_bf16(a, 0);
  ConvArgs b{};
  b.x = y0; b.w = dw1; b.bias = db1; b.res = nullptr; b.y = z0;
  b.N = N; b.H = H; b.W = W; b.Cin = cexp; b.Ho = H; b.Wo = W; b.Cout = c1;
  b.KH = b.KW = b.KWp = 1; b.stride = 1; b.pad = 0; b.K = cexp; b.relu = 1; b.zero = dz; b.xcd = 1;
  rc |= launch_conv_bf16(b, 0);
  Pair1x1Args p{};
  p.x = dx; p.res = cds ? nullptr : dr; p.w3 = dw3; p.b3 = db3; p.w1 = dw1; p.b1 = db1;
  p.y = y1; p.z = z1; p.M = M; p.c1 = c1; p.cmid = cmid; p.cexp = cexp;
  if (cds) { p.x2 = dx2; p.cds = cds; p.Ho = H; p.Wo = W; p.H2 = H2; p.W2 = W2; }
  p.cap_elems = Mp * std::max(cmid, std::max(cexp, c1));
  std::vector<unsigned short> hy0(M * cexp), hy1(M * cexp), hz0(M * c1), hz1(M * c1);
  hipMemcpy(hy0.data(), y0, M * cexp * 2, hipMemcpyDeviceToHost);
  hipMemcpy(hz0.data(), z0, M * c1 * 2, hipMemcpyDeviceToHost);
  long bady = 0, badz = 0;
  double maxd = 0;
  int rcp = 0;
  const int REPS = reps ? reps : M % tile ? 8 : 1;
  void* flush = nullptr;
  if (stress) hipMalloc(&flush, 1LL << 30);
  if (inplace && !cds) p.res = y1;
  for (int rep = 0; rep < REPS; ++rep) {
    hipMemset(y1, 0xff, Mp * cexp * 2); hipMemset(z1, 0xff, Mp * c1 * 2);
    if (inplace && !cds) hipMemcpy(y1, dr, M * cexp * 2, hipMemcpyDeviceToDevice);
    if (stress) {
      hipMemset(flush, rep, 1LL << 30);
      hipLaunchKernelGGL(lds_poison_k, dim3(1024), dim3(256), 0, 0);
    }
    rcp |= launch_pairw_bf16(p, 0);
    hipDeviceSynchronize();
    hipMemcpy(hy1.data(), y1, M * cexp * 2, hipMemcpyDeviceToHost);
    hipMemcpy(hz1.data(), z1, M * c1 * 2, hipMemcpyDeviceToHost);
    for (size_t i = 0; i < hy0.size(); ++i)
      if (hy0[i] != hy1[i]) ++bady, maxd = std::max(maxd, (double)fabs(bf2f(hy0[i]) - bf2f(hy1[i])));
    for (size_t i = 0; i < hz0.size(); ++i)
      if (hz0[i] != hz1[i]) ++badz, maxd = std::max(maxd, (double)fabs(bf2f(hz0[i]) - bf2f(hz1[i])));
  }
  double maxerr = 0;  // the unfused conv3 itself against double on the bf16 operands (a few pixels)
  for (long long m = 0; m < M; m += M / 7 + 1)
    for (int o = 0; o < cexp; o += 7) {
      double acc = b3[o];
      for (int k = 0; k < cmid; ++k) acc += (double)bf2f(x[m * cmid + k]) * bf2f(w3[(size_t)o * K3 + k]);
      if (cds) {
        const long long n = m / (H * W), rem = m % (H * W), oh = rem / W, ow = rem % W;
        const size_t p2 = (size_t)((n * H2 + 2 * oh) * W2 + 2 * ow) * cds;
        for (int k = 0; k < cds; ++k) acc += (double)bf2f(x2[p2 + k]) * bf2f(w3[(size_t)o * K3 + cmid + k]);
      } else {
        acc += bf2f(res[m * cexp + o]);
      }
      acc = std::max(acc, 0.0);
      maxerr = std::max(maxerr, fabs(acc - bf2f(hy0[m * cexp + o])) / (1.0 + fabs(acc)));
    }
  const bool fail = rc || rcp || bady || badz || maxerr > 1e-2;
  printf("%s pairw bf16 N%d H%d W%d %d(+ds %d)->%d->%d M%lld rc=%d/%d differing y %ld z %ld (max %.3e) unfused maxerr %.3e\n",
         fail ? "FAIL" : "ok  ", N, H, W, cmid, cds, cexp, c1, M, rc, rcp, bady, badz, maxd, maxerr);
  for (void* q : {dx, dr, dx2, dw3, dw1, (void*)db3, (void*)db1, y0, y1, z0, z1, dz, flush}) hipFree(q);
  return fail ? 1 : 0;
}

// ------------------------------------------------------------------ f32x3: `conv_check x3 <group>`
// The split instantiations (ConvArgs::split = 1) kernel by kernel against x3_ref.h's double
// reference and derived bound; DESIGN.md section 3X maps every split dispatch branch to its case.

using x3::u16;

// a device buffer of n bytes with a 4-KiB guard behind it, all 0xff
struct Guarded {
  unsigned char* p = nullptr;
  size_t n = 0;
  explicit Guarded(size_t bytes) : n(bytes) {
    hipMalloc(&p, n + 4096);
    hipMemset(p, 0xff, n + 4096);
  }
  // the payload into `host`; false if a guard byte changed
  bool fetch(void* host) const {
    std::vector<unsigned char> g(4096);
    hipMemcpy(host, p, n, hipMemcpyDeviceToHost);
    hipMemcpy(g.data(), p + n, 4096, hipMemcpyDeviceToHost);
    for (unsigned char b : g)
      if (b != 0xff) return false;
    return true;
  }
  ~Guarded() { hipFree(p); }
};
template <class T>
static T* upload(const std::vector<T>& v) {
  T* d = nullptr;
  hipMalloc(&d, v.size() * sizeof(T) + 16);
  if (!v.empty()) hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return d;
}
// a device error ends the run: nothing more is launched after a fault
static void sync_or_die(const char* what) {
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("FAIL %s: %s\n1 failures (stopped)\n", what, hipGetErrorString(e));
    fflush(stdout);
    _exit(3);
  }
}

// One launch of launch_conv_bf16 with split = 1.  BM x BN: the tile the case is meant for (BM 0:
// the row-strip kernel, whose planned "blocks" are its strips); the planned grid must equal it, so
// that a dispatch change that moves the case to another kernel fails here.  Operands and the
// reference of the conv part are shared by consecutive calls on one shape (x3::Shape).
static int check_x3(const char* id, const x3::Shape& s, bool res, bool relu, bool kcm, int BM, int BN,
                    double coef = x3::kCoef) {
  static x3::Case c;
  static x3::Ref ref;
  static bool have = false;
  if (!have || !(c.s == s)) {
    c = x3::make_case(s);
    ref = x3::reference(c);
    have = true;
  }
  const long long M = c.M();
  u16 *dx = upload(c.x), *dw = upload(x3::device_weights(c, kcm)), *dr = upload(c.res),
      *dx2 = s.Cds ? upload(c.x2) : nullptr;
  float* db = upload(c.bias);
  void* dz;
  hipMalloc(&dz, 256);
  hipMemset(dz, 0, 256);
  Guarded out((size_t)M * 2 * s.Cout * 2);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.res = res ? dr : nullptr; a.y = out.p;
  a.N = s.N; a.H = s.H; a.W = s.W; a.Cin = 3 * s.C; a.Ho = c.Ho; a.Wo = c.Wo; a.Cout = s.Cout;
  a.KH = a.KW = a.KWp = s.k; a.stride = s.stride; a.pad = s.pad; a.K = c.K; a.relu = relu; a.zero = dz;
  a.xcd = 1; a.kcm = kcm; a.split = 1;  // xs / x2s stay 0: the library derives them
  if (s.Cds) { a.x2 = dx2; a.H2 = c.H2; a.W2 = c.W2; a.Cin2 = 3 * s.Cds; a.stride2 = s.s2; a.K1 = c.K1; }
  LaunchInfo li{-1, -1};
  ConvArgs p = a;
  p.plan = &li;
  const int prc = launch_conv_bf16(p, 0);
  const long long expect = BM ? (M + BM - 1) / BM * (s.Cout / BN) : (long long)s.N * (s.H / 2);
  const bool grid_ok = prc == 0 && li.blocks == expect;
  int rc = -1;
  bool guard_ok = true;
  x3::Stats st;
  st.bad = -1;
  if (grid_ok) {  // the wrong kernel is not run: the case has failed already
    rc = launch_conv_bf16(a, 0);
    sync_or_die(id);
    std::vector<u16> y((size_t)M * 2 * s.Cout);
    guard_ok = out.fetch(y.data());
    st = x3::verify(c, ref, y.data(), res, relu, coef);
  }
  const bool fail = !grid_ok || rc || !guard_ok || !st.ok();
  printf("%s x3 %s %s N%d %dx%d %d->%d k%d s%d res%d relu%d kcm%d ds%d/%d M%lld tile %dx%d grid %lld (expected %lld) "
         "rc=%d max err / bound %.3f bad %ld dup %ld guard %s\n",
         fail ? "FAIL" : "ok  ", id, s.real ? "real " : "probe", s.N, s.H, s.W, s.C, s.Cout, s.k, s.stride, res, relu, kcm,
         s.Cds, s.s2, M, BM, BN, li.blocks, expect, rc, st.max_ratio, st.bad, st.bad_dup, guard_ok ? "ok" : "OVERWRITTEN");
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)dr, (void*)dx2, (void*)db, dz}) hipFree(q);
  return fail;
}

// launch_stem_pool_f32(..., split = true): the exact-f32 stem storing (hi, lo), which f32x3 takes
// when stem_pool_x3_ok refuses the frame size.  Reference and data as check_stem_pool_f32; bound
// its 1e-5 (1 + |m|) plus 2^-17 |m| for the hi + lo form, and the dup condition.
static int check_stem_pool_f32_split(int N, int H, int W, bool direct) {
  const int pad = 3, Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  const int Hs = (H + 6 - 7) / 2 + 1, Ws = (W + 6 - 7) / 2 + 1;
  const int Hq = (Hs - 1) / 2 + 1, Wq = (Ws - 1) / 2 + 1;
  unsigned s = 5151;
  std::vector<float> x(stem_input_elems(N, H, W, pad) + 64, 0.f), w(64 * 176, 0.f), b(64);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int c = 0; c < 3; ++c) x[(((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c] = frand(s);
  for (int o = 0; o < 64; ++o)
    for (int kh = 0; kh < 7; ++kh)
      for (int kw = 0; kw < 7; ++kw)
        for (int c = 0; c < 3; ++c) w[o * 176 + kh * 24 + kw * 3 + c] = frand(s) * 0.2f;
  for (auto& v : b) v = frand(s) * 0.5f;
  std::vector<float> fr((size_t)N * 3 * H * W);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j)
          fr[(((size_t)n * 3 + c) * H + i) * W + j] = x[(((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + c];
  float *dx = upload(x), *dw = upload(w), *db = upload(b), *dfr = upload(fr);
  const size_t ny = (size_t)N * Hq * Wq * 128;  // (hi 64 | lo 64) per pooled pixel
  Guarded out(ny * 2);
  if (direct && !stem_pool_f32_direct_ok(H, W)) {
    printf("FAIL stem_pool f32 split direct N%d H%d W%d: the direct path does not take this size\n", N, H, W);
    return 1;
  }
  const int rc = direct ? launch_stem_pool_f32(nullptr, N, H, W, dw, db, out.p, 0, true, nullptr, dfr)
                        : launch_stem_pool_f32(dx, N, H, W, dw, db, out.p, 0, true);
  sync_or_die("stem_pool f32 split");
  std::vector<u16> y(ny);
  const bool guard_ok = out.fetch(y.data());
  std::vector<double> st((size_t)Hs * Ws * 64);
  long bad = 0, baddup = 0;
  double maxr = 0;
  for (int n = 0; n < N; ++n) {
    for (int sy = 0; sy < Hs; ++sy)
      for (int sx = 0; sx < Ws; ++sx)
        for (int o = 0; o < 64; ++o) {
          double acc = b[o];
          for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 7; ++kw)
              for (int c = 0; c < 3; ++c)
                acc += (double)x[(((size_t)n * Hp + 2 * sy + kh) * Wp + 2 * sx + kw) * 3 + c] * w[o * 176 + kh * 24 + kw * 3 + c];
          st[((size_t)sy * Ws + sx) * 64 + o] = acc > 0 ? acc : 0;
        }
    for (int py = 0; py < Hq; ++py)
      for (int px = 0; px < Wq; ++px)
        for (int o = 0; o < 64; ++o) {
          double m = -INFINITY;
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx_ = -1; dx_ <= 1; ++dx_) {
              const int sy = 2 * py + dy, sx = 2 * px + dx_;
              if (sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) m = fmax(m, st[((size_t)sy * Ws + sx) * 64 + o]);
            }
          const size_t base = (((size_t)n * Hq + py) * Wq + px) * 128 + o;
          const double hi = bf2f(y[base]), lo = bf2f(y[base + 64]);
          const double e = fabs(hi + lo - m), bound = 1e-5 * (1 + fabs(m)) + fabs(m) / 131072;
          const bool dup = fabs(lo) <= fabs(hi) / 256, in = e <= bound;
          if (!in || !dup) {
            if (bad + baddup < 5) printf("  bad n%d py%d px%d o%d ref %.9g got %.9g + %.9g dup %d\n", n, py, px, o, m, hi, lo, (int)dup);
            bad += !in;
            baddup += in && !dup;
          }
          const double ratio = e == e ? e / bound : INFINITY;
          if (!(ratio <= maxr)) maxr = ratio;
        }
  }
  const bool fail = rc || bad || baddup || !guard_ok;
  printf("%s x3 stem_pool f32 split %s N%d H%d W%d (stem %dx%d, pooled %dx%d) rc=%d max err / bound %.3f bad %ld dup %ld guard %s\n",
         fail ? "FAIL" : "ok  ", direct ? "direct" : "pack  ", N, H, W, Hs, Ws, Hq, Wq, rc, maxr, bad, baddup,
         guard_ok ? "ok" : "OVERWRITTEN");
  for (void* q : {(void*)dx, (void*)dw, (void*)db, (void*)dfr}) hipFree(q);
  return fail;
}

// csrc/layout.hip against the host, bit for bit
static int report_exact(const char* what, long diff, int rc, bool guard_ok) {
  const bool fail = diff || rc || !guard_ok;
  printf("%s x3 layout %s rc=%d differing %ld guard %s\n", fail ? "FAIL" : "ok  ", what, rc, diff,
         guard_ok ? "ok" : "OVERWRITTEN");
  return fail;
}
// mode 0 f32, 1 bf16, 2 split: the sequential f32 sum in pixel order (mode 2: hi + lo per pixel
// first), then / (float)HW -- the documented arithmetic
static int check_avgpool(int B, int HW, int C, int mode) {
  unsigned s = 99 + mode;
  const size_t n = (size_t)B * HW * C * (mode == 2 ? 2 : 1);
  std::vector<float> xf(mode ? 0 : n);
  std::vector<u16> xb(mode ? n : 0);
  for (auto& v : xf) v = frand(s);
  for (auto& v : xb) v = f2bf(frand(s));  // mode 2: lo as large as hi
  void* dx = mode ? (void*)upload(xb) : (void*)upload(xf);
  Guarded out((size_t)B * C * 4);
  const int rc = launch_avgpool(dx, B, HW, C, (float*)out.p, mode, 0);
  sync_or_die("avgpool");
  std::vector<float> y((size_t)B * C);
  const bool guard_ok = out.fetch(y.data());
  long diff = 0;
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c) {
      volatile float acc = 0.f;  // volatile: one rounding per add, in this order
      for (int p = 0; p < HW; ++p) {
        const size_t px = (size_t)b * HW + p;
        if (mode == 2) {
          volatile float t = bf2f(xb[px * 2 * C + c]) + bf2f(xb[px * 2 * C + C + c]);
          acc = acc + t;
        } else {
          acc = acc + (mode ? bf2f(xb[px * C + c]) : xf[px * C + c]);
        }
      }
      const float want = acc / (float)HW;
      diff += memcmp(&want, &y[(size_t)b * C + c], 4) != 0;
    }
  char what[96];
  snprintf(what, sizeof what, "avgpool mode %d B%d HW%d C%d", mode, B, HW, C);
  hipFree(dx);
  return report_exact(what, diff, rc, guard_ok);
}
static int check_act_to_f32(long long pixels, int C, int mode) {
  unsigned s = 31 + mode;
  const long long n = pixels * C;
  std::vector<float> xf(mode ? 0 : n);
  std::vector<u16> xb(mode ? n * (mode == 2 ? 2 : 1) : 0);
  for (auto& v : xf) v = frand(s);
  for (auto& v : xb) v = f2bf(frand(s));
  void* dx = mode ? (void*)upload(xb) : (void*)upload(xf);
  Guarded out((size_t)n * 4);
  const int rc = launch_act_to_f32(dx, n, C, mode, (float*)out.p, 0);
  sync_or_die("act_to_f32");
  std::vector<float> y(n);
  const bool guard_ok = out.fetch(y.data());
  long diff = 0;
  for (long long i = 0; i < n; ++i) {
    const long long p = i / C, c = i % C;
    volatile float want = mode == 2 ? bf2f(xb[p * 2 * C + c]) + bf2f(xb[p * 2 * C + C + c]) : mode ? bf2f(xb[i]) : xf[i];
    const float wv = want;
    diff += memcmp(&wv, &y[i], 4) != 0;
  }
  char what[96];
  snprintf(what, sizeof what, "act_to_f32 mode %d n%lld C%d", mode, n, C);
  hipFree(dx);
  return report_exact(what, diff, rc, guard_ok);
}
static int check_maxpool(int B, int H, int W, int C, bool bf16) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  unsigned s = 57 + C;
  const size_t n = (size_t)B * H * W * C, no = (size_t)B * Ho * Wo * C;
  std::vector<float> xf(n);  // bf16: the values are bf16-representable, so the max is too
  for (auto& v : xf) v = bf16 ? bf2f(f2bf(frand(s))) : frand(s);
  std::vector<u16> xb(bf16 ? n : 0);
  for (size_t i = 0; i < xb.size(); ++i) xb[i] = f2bf(xf[i]);
  void* dx = bf16 ? (void*)upload(xb) : (void*)upload(xf);
  Guarded out(no * (bf16 ? 2 : 4));
  const int rc = launch_maxpool3x3s2(dx, B, H, W, C, out.p, Ho, Wo, bf16, 0);
  sync_or_die("maxpool");
  std::vector<unsigned char> y(no * (bf16 ? 2 : 4));
  const bool guard_ok = out.fetch(y.data());
  long diff = 0;
  for (int b = 0; b < B; ++b)
    for (int oh = 0; oh < Ho; ++oh)
      for (int ow = 0; ow < Wo; ++ow)
        for (int c = 0; c < C; ++c) {
          float m = -INFINITY;
          for (int dh = -1; dh <= 1; ++dh)
            for (int dw = -1; dw <= 1; ++dw) {
              const int ih = 2 * oh + dh, iw = 2 * ow + dw;
              if (ih >= 0 && ih < H && iw >= 0 && iw < W) m = fmaxf(m, xf[(((size_t)b * H + ih) * W + iw) * C + c]);
            }
          const size_t oi = (((size_t)b * Ho + oh) * Wo + ow) * C + c;
          if (bf16) {
            const u16 want = f2bf(m);
            diff += memcmp(&want, &y[oi * 2], 2) != 0;
          } else {
            diff += memcmp(&m, &y[oi * 4], 4) != 0;
          }
        }
  char what[96];
  snprintf(what, sizeof what, "maxpool3x3s2 %s B%d %dx%d -> %dx%d C%d", bf16 ? "bf16" : "f32", B, H, W, Ho, Wo, C);
  hipFree(dx);
  return report_exact(what, diff, rc, guard_ok);
}
// interior exact (bf16: RNE of the input), borders untouched (a sentinel prefilled)
static int check_pack_rgb_pad(int B, int H, int W, int pad, bool bf16) {
  const int Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  unsigned s = 73;
  std::vector<float> fr((size_t)B * 3 * H * W);
  for (auto& v : fr) v = frand(s) * 3.f;
  float* dfr = upload(fr);
  const size_t esz = bf16 ? 2 : 4, n = (size_t)B * Hp * Wp * 3;
  Guarded out(n * esz);
  hipMemset(out.p, 0xa5, n * esz);  // the sentinel; the guard behind stays 0xff
  const int rc = launch_pack_rgb_pad(dfr, B, H, W, pad, out.p, bf16, 0);
  sync_or_die("pack_rgb_pad");
  std::vector<unsigned char> y(n * esz);
  const bool guard_ok = out.fetch(y.data());
  long diff = 0;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < Hp; ++i)
      for (int j = 0; j < Wp; ++j)
        for (int c = 0; c < 3; ++c) {
          const size_t oi = (((size_t)b * Hp + i) * Wp + j) * 3 + c;
          const int yy = i - pad, xx = j - pad;
          if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const float v = fr[(((size_t)b * 3 + c) * H + yy) * W + xx];
            const u16 vb = f2bf(v);
            diff += memcmp(bf16 ? (const void*)&vb : (const void*)&v, &y[oi * esz], esz) != 0;
          } else {
            for (size_t k = 0; k < esz; ++k) diff += y[oi * esz + k] != 0xa5;
          }
        }
  char what[96];
  snprintf(what, sizeof what, "pack_rgb_pad %s B%d %dx%d pad %d (rows of %d)", bf16 ? "bf16" : "f32", B, H, W, pad, Wp);
  hipFree(dfr);
  return report_exact(what, diff, rc, guard_ok);
}

// Shape{N, H, W, C, Cout, k, stride, pad, Cds, s2, real}
static int run_x3(const char* group) {
  int f = 0;
  bool known = false;
  auto is = [&](const char* g) {
    const bool m = !strcmp(group, g);
    known |= m;
    return m;
  };
  if (is("rows")) {  // conv_rows_x3 (W 56, H even, 64 -> 64 3x3): BM 0 = strips
    // 300 strips > device_cu_count(): some workgroups take a second strip and the double buffer
    // turns over; images N - 2, N - 1 hold those strips
    const x3::Shape big{50, 12, 56, 64, 64, 3, 1, 1, 0, 0, false};
    if (50 * 6 <= device_cu_count()) printf("FAIL x3 rows: %d CUs take 300 strips in one trip\n", device_cu_count()), ++f;
    for (int kcm = 0; kcm < 2; ++kcm)
      for (int res = 0; res < 2; ++res)
        for (int relu = 0; relu < 2; ++relu) f += check_x3("rows.trips", big, res, relu, kcm, 0, 64);
    f += check_x3("rows.one", {1, 2, 56, 64, 64, 3, 1, 1, 0, 0, false}, true, true, true, 0, 64);  // one strip, both borders
    f += check_x3("rows.real", {3, 56, 56, 64, 64, 3, 1, 1, 0, 0, true}, true, true, true, 0, 64);
  }
  if (is("ts")) {  // tap-shift tiles (conv_bf16_ts.hip)
    f += check_x3("ts64.tail", {3, 9, 11, 64, 64, 3, 1, 1, 0, 0, false}, false, false, false, 512, 64);  // M 297 < one tile
    f += check_x3("ts64.cross", {5, 28, 28, 64, 64, 3, 1, 1, 0, 0, false}, true, true, false, 512, 64);  // 7.66 tiles
    f += check_x3("ts128", {2, 28, 28, 128, 128, 3, 1, 1, 0, 0, false}, true, true, true, 512, 128);
    f += check_x3("ts128.tail", {2, 9, 11, 128, 128, 3, 1, 1, 0, 0, false}, true, false, true, 512, 128);
    f += check_x3("ts128.ds", {3, 14, 14, 128, 128, 3, 1, 1, 64, 2, false}, false, true, true, 512, 128);
    f += check_x3("ts128.real", {2, 28, 28, 128, 128, 3, 1, 1, 0, 0, true}, true, true, true, 512, 128);
  }
  if (is("g64")) {  // conv_bf16_kernel<256,64,4,1>: 1x1 with Cout 64
    for (int C : {64, 256}) {
      f += check_x3("g64.tail", {2, 9, 11, C, 64, 1, 1, 0, 0, 0, false}, false, true, false, 256, 64);  // M 198
      f += check_x3("g64", {3, 20, 20, C, 64, 1, 1, 0, 0, 0, false}, false, true, false, 256, 64);      // 4.7 tiles
    }
  }
  if (is("g128")) {  // conv_bf16_kernel<512,128,4,2>
    f += check_x3("g128.1x1", {3, 14, 14, 256, 128, 1, 1, 0, 0, 0, false}, false, true, false, 512, 128);
    f += check_x3("g128.1x1.tail", {2, 9, 11, 512, 128, 1, 1, 0, 0, 0, false}, false, true, false, 512, 128);
    f += check_x3("g128.s2.ragged", {3, 13, 11, 64, 128, 3, 2, 1, 0, 0, false}, false, true, false, 512, 128);
    f += check_x3("g128.s2", {2, 56, 56, 64, 128, 3, 2, 1, 0, 0, false}, false, true, false, 512, 128);
    f += check_x3("g128.s2.kcm", {2, 28, 28, 128, 128, 3, 2, 1, 0, 0, false}, false, true, true, 512, 128);
  }
  if (is("g256")) {  // conv_bf16_kernel<256,256,2,4>, one ring: 3x3 stride 1
    f += check_x3("g256.ring1", {2, 14, 14, 256, 256, 3, 1, 1, 0, 0, false}, true, true, true, 256, 256);
    f += check_x3("g256.ring1.c512", {3, 7, 7, 512, 512, 3, 1, 1, 0, 0, false}, false, true, true, 256, 256);  // M 147, two cout tiles
    f += check_x3("g256.ring1.real", {2, 14, 14, 256, 256, 3, 1, 1, 0, 0, true}, true, true, true, 256, 256);
    // ... split rings (NSA = 3): 1x1s, stride 2, the fused downsample (DS)
    f += check_x3("g256.nsa.1x1", {3, 20, 20, 64, 256, 1, 1, 0, 0, 0, false}, true, true, false, 256, 256);
    f += check_x3("g256.nsa.k1024", {2, 7, 7, 1024, 256, 1, 1, 0, 0, 0, false}, false, true, false, 256, 256);
    f += check_x3("g256.nsa.s2", {3, 13, 11, 128, 256, 3, 2, 1, 0, 0, false}, false, true, true, 256, 256);
    f += check_x3("g256.ds.s1", {2, 9, 11, 64, 256, 1, 1, 0, 64, 1, false}, false, true, false, 256, 256);   // R50 layer1.0
    f += check_x3("g256.ds.s2", {2, 7, 5, 128, 512, 1, 1, 0, 256, 2, false}, false, true, false, 256, 256);  // R50 layer2.0
    f += check_x3("g256.ds.3x3", {2, 7, 7, 256, 256, 3, 1, 1, 128, 2, false}, false, true, true, 256, 256);  // R18 layer3.0.conv2
  }
  if (is("stem")) {
    f += check_stem_pool_f32_split(3, 100, 86, false);  // W % 4 != 0: the pack path
    f += check_stem_pool_f32_split(2, 98, 96, true);    // direct, odd stem height (49)
    f += check_stem_pool_f32_split(2, 98, 96, false);
    f += check_stem_pool_f32_split(2, 40, 200, true);   // Ws 100: a partial last column tile
    f += check_stem_pool_f32_split(2, 40, 200, false);
  }
  if (is("layout")) {
    for (int mode = 0; mode < 3; ++mode) {
      f += check_avgpool(3, 49, 512, mode);
      f += check_avgpool(1, 1, 64, mode);
      f += check_avgpool(5, 12, 100, mode);  // 500 (frame, channel) pairs: a ragged last block
      f += check_act_to_f32(7 * 9, 100, mode);  // n 6300, not a multiple of 256
    }
    for (int bf16 = 0; bf16 < 2; ++bf16) {
      f += check_maxpool(2, 15, 13, 64, bf16);  // Ho 8, Wo 7: odd sizes, border windows
      f += check_maxpool(2, 15, 13, 8, bf16);
      f += check_pack_rgb_pad(2, 9, 7, 3, bf16);
    }
  }
  if (!known) printf("FAIL x3: unknown group %s\n", group), ++f;
  printf("%d failures\n", f);
  return f ? 1 : 0;
}

// ------------------------------------------------------------------ bf16: `conv_check bf16 <group>`
// The bf16 inference kernels one by one against bf16_ref.h's int64 reference on integer data:
// every output of every image bitwise (-0 folded into +0), outputs prefilled with 0xff between two
// 4-KiB guards, every launch done twice, the planned grid pinned to the kernel the case is meant
// for.  DESIGN.md section 3B maps every release dispatch branch and launcher to its case.

// n payload bytes between two 4-KiB guards, all 0xff
struct Fenced {
  unsigned char* base = nullptr;
  size_t n = 0;
  explicit Fenced(size_t bytes) : n(bytes) {
    hipMalloc(&base, n + 8192);
    poison();
  }
  unsigned char* p() const { return base + 4096; }
  void poison() const { hipMemset(base, 0xff, n + 8192); }
  void put(const void* host, size_t bytes) const { hipMemcpy(p(), host, bytes, hipMemcpyHostToDevice); }
  // the payload into `host`; false if a guard byte changed
  bool fetch(void* host) const {
    std::vector<unsigned char> all(n + 8192);
    hipMemcpy(all.data(), base, n + 8192, hipMemcpyDeviceToHost);
    memcpy(host, all.data() + 4096, n);
    for (size_t i = 0; i < 4096; ++i)
      if (all[i] != 0xff || all[4096 + n + i] != 0xff) return false;
    return true;
  }
  ~Fenced() { hipFree(base); }
  Fenced(const Fenced&) = delete;
};
struct OutBuf {
  const Fenced* f;
  std::vector<bfr::u16> first, second;
};
// poison the outputs, prep() (an in-place kernel's input goes back into its output), launch(),
// fetch -- twice; the guards of every output and the bitwise difference of the two runs
template <class Prep, class Launch>
static int launch_twice(const char* id, std::vector<OutBuf>& outs, Prep prep, Launch launch, bool& guards, long long& rerun) {
  int rc = 0;
  guards = true;
  rerun = 0;
  for (int rep = 0; rep < 2; ++rep) {
    for (auto& o : outs) o.f->poison();
    prep();
    rc |= launch();
    sync_or_die(id);
    for (auto& o : outs) {
      auto& v = rep ? o.second : o.first;
      v.resize((o.f->n + 1) / 2);
      guards &= o.f->fetch(v.data());
    }
  }
  for (auto& o : outs)
    for (size_t i = 0; i < o.first.size(); ++i) rerun += o.first[i] != o.second[i];
  return rc;
}
static void print_first(const char* what, const bfr::Diff& d, int HW, int W, int C) {
  if (!d.count) return;
  const long long p = d.first / C;
  printf("  first differing %s: image %lld row %lld col %lld ch %lld: want %d got %g\n", what, p / HW, p % HW / W, p % W,
         d.first % C, d.want, d.got);
}
static bool cond_ok(const bfr::Cond& c, long long extra = 0) { return !c.violations && c.max_sabs + extra < (1LL << 24); }

enum Route { kRows, kRowsr, kRowsrDispatch, kS2rows, kTs, kG512, kG256, kG64 };
static const char* route_name(Route r) {
  static const char* n[] = {"conv_rows", "conv_rowsr (direct)", "conv_rowsr", "conv_s2rows", "tap-shift 512x128", "ws 512x128",
                            "ws 256x256", "128x64"};
  return n[r];
}

// One conv through launch_conv_bf16 (kRowsr: launch_conv_rowsr_bf16 directly).  The reference of the
// conv part (before residual, ReLU and conversion) is shared by consecutive cases on one shape.
static int bf16_conv(const char* id, Route route, int mode, int N, int H, int W, int C, int Cout, int k, int stride, int pad,
                     int Cds, int s2, bool res, bool relu, bool kcm) {
  static bfr::ConvCase c;
  static std::vector<int> raw;
  static bfr::Cond cond;
  static bool have = false;
  {
    bfr::ConvCase q;
    q.N = N, q.H = H, q.W = W, q.C = C, q.Cout = Cout, q.k = k, q.stride = stride, q.pad = pad, q.Cds = Cds, q.s2 = s2, q.mode = mode;
    if (!have || !c.same_shape(q)) {
      c = bfr::make_conv(N, H, W, C, Cout, k, stride, pad, Cds, s2, mode);
      cond = bfr::Cond();
      raw = bfr::run_stage<long long>(c.stage(false, false), bfr::kNone, false, &cond);
      have = true;
    }
  }
  const long long M = c.M();
  std::vector<int> ref(raw.size());
  for (size_t i = 0; i < raw.size(); ++i) {
    long long v = raw[i] + (res ? c.res[i] : 0);
    if (relu && v < 0) v = 0;
    ref[i] = bfr::round_int(v, false);
  }
  bfr::u16 *dx = upload(bfr::to_bf16(c.x)), *dw = upload(bfr::device_weights(c.w, Cout, c.K, c.K1, k * k, C, kcm)),
           *dr = upload(bfr::to_bf16(c.res)), *dx2 = Cds ? upload(bfr::to_bf16(c.x2)) : nullptr;
  float* db = upload(bfr::to_f32(c.bias));
  void* dz;
  hipMalloc(&dz, 256);
  hipMemset(dz, 0, 256);
  Fenced out((size_t)M * Cout * 2);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.res = res ? dr : nullptr; a.y = out.p();
  a.N = N; a.H = H; a.W = W; a.Cin = C; a.Ho = c.Ho; a.Wo = c.Wo; a.Cout = Cout;
  a.KH = a.KW = a.KWp = k; a.stride = stride; a.pad = pad; a.K = c.K; a.relu = relu; a.zero = dz;
  a.xcd = 1; a.kcm = kcm; a.xs = C;
  if (Cds) { a.x2 = dx2; a.H2 = c.H2; a.W2 = c.W2; a.Cin2 = Cds; a.stride2 = s2; a.K1 = c.K1; a.x2s = Cds; }
  int (*launch)(const ConvArgs&, hipStream_t) = route == kRowsr ? launch_conv_rowsr_bf16 : launch_conv_bf16;
  // the dispatch of the release library, from the kernels' own predicates
  const int cu = device_cu_count();
  const bool rowsr_d = !a.x2 && conv_rowsr_bf16_ok(a) && C == 64 && W == 64;
  const bool strip = rowsr_d || (!a.x2 && conv_rows_bf16_ok(a));
  const bool gemm = !strip && !conv_s2rows_bf16_ok(a);
  const bool ts = gemm && conv_bf16_ts_ok(a) && Cout == 128;
  bool pred = false, persistent = false;
  long long expect = -1;
  switch (route) {
    case kRows: pred = strip && !rowsr_d, expect = (long long)N * (H / 4), persistent = true; break;
    case kRowsr: pred = conv_rowsr_bf16_ok(a), expect = (long long)N * (H / 4), persistent = true; break;
    case kRowsrDispatch: pred = rowsr_d, expect = (long long)N * (H / 4), persistent = true; break;
    case kS2rows: pred = !strip && conv_s2rows_bf16_ok(a), expect = (long long)N * 7, persistent = true; break;
    case kTs: pred = ts, expect = (M + 511) / 512; break;
    case kG512: pred = gemm && !ts && Cout == 128, expect = (M + 511) / 512; break;
    case kG256: pred = gemm && Cout >= 256, expect = (M + 255) / 256 * ((Cout + 255) / 256); break;
    case kG64: pred = gemm && Cout == 64, expect = (M + 127) / 128; break;
  }
  LaunchInfo li{-1, -1};
  ConvArgs p = a;
  p.plan = &li;
  const int prc = launch(p, 0);
  const bool grid_ok = prc == 0 && pred && li.blocks == expect && (!persistent || li.slots == cu);
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  bfr::Diff d;
  d.count = -1;
  if (grid_ok) {  // the wrong kernel is not run: the case has failed already
    std::vector<OutBuf> outs{{&out}};
    rc = launch_twice(id, outs, [] {}, [&] { return launch(a, 0); }, guards, rerun);
    d = bfr::compare(ref, outs[0].first.data());
  }
  const bool data_ok = cond_ok(cond, 64);
  const bool fail = !grid_ok || rc || !guards || rerun || d.count || !data_ok;
  printf("%s bf16 %s %s N%d %dx%d %d->%d k%d s%d res%d relu%d kcm%d ds%d/%d M%lld | %s grid %lld (expected %lld) slots %lld "
         "route %s | rc=%d differing %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s, %lld of %lld conv sums "
         "outside +-256\n",
         fail ? "FAIL" : "ok  ", id, bfr::mode_name(mode), N, H, W, C, Cout, k, stride, res, relu, kcm, Cds, s2, M,
         route_name(route), li.blocks, expect, li.slots, pred ? "ok" : "OTHER KERNEL", rc, d.count, ref.size(), rerun,
         guards ? "ok" : "OVERWRITTEN", cond.max_sabs + 64, data_ok ? "" : " (>= 2^24)", cond.over256, cond.outputs);
  print_first("y", d, c.Ho * c.Wo, c.Wo, Cout);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)dr, (void*)dx2, (void*)db, dz}) hipFree(q);
  return fail;
}

// pair1x1 (launch_pair1x1_bf16, M % 64 == 0), pair1x1r (launch_pair1x1r_bf16, any M) and pairw
// (launch_pairw_bf16: whole rounds, so x and res / y carry NaN padding to the padded pixel count;
// inplace: y = res, as the engine runs it).  Y and Z against the integer chain reference.
enum PairKind { kPair, kPairR, kPairW };
static int bf16_pair(const char* id, PairKind kind, int mode, int N, int H, int W, int cmid, int cexp, int c1, int cds,
                     bool inplace = false) {
  const int s2 = kind == kPairW && cds ? 2 : 1;
  const bfr::PairCase c = bfr::make_pair_case(N, H, W, cmid, cexp, c1, cds, s2, mode);
  const bfr::ChainOut ref = bfr::run_pair<long long>(c);
  const long long M = c.M();
  const long long tile = kind == kPairW ? pairw_tile(cmid, c1, cds) : (cds || c1 == 64 ? 256 : 128);
  const long long Mp = kind == kPairW ? (M + tile - 1) / tile * tile : M;
  auto padded = [&](const std::vector<int>& v, int ch) {  // NaN behind the M pixels
    std::vector<bfr::u16> o((size_t)Mp * ch, 0x7fc0);
    const std::vector<bfr::u16> b = bfr::to_bf16(v);
    std::copy(b.begin(), b.end(), o.begin());
    return o;
  };
  const std::vector<bfr::u16> hres = cds ? std::vector<bfr::u16>(1) : padded(c.res, cexp);
  bfr::u16 *dx = upload(padded(c.x, cmid)), *dr = upload(hres), *dx2 = upload(bfr::to_bf16(c.x2));
  bfr::u16 *dw3 = upload(bfr::to_bf16(c.w3)), *dw1 = upload(bfr::to_bf16(c.w1));
  float *db3 = upload(bfr::to_f32(c.b3)), *db1 = upload(bfr::to_f32(c.b1));
  Fenced y((size_t)Mp * cexp * 2), z((size_t)Mp * c1 * 2);
  inplace = inplace && !cds;
  Pair1x1Args a{};
  a.x = dx; a.x2 = cds ? dx2 : nullptr; a.res = cds ? nullptr : inplace ? (void*)y.p() : (void*)dr;
  a.w3 = dw3; a.b3 = db3; a.w1 = dw1; a.b1 = db1; a.y = y.p(); a.z = z.p(); a.M = M; a.c1 = c1; a.cds = cds;
  bool pred = true;
  if (kind == kPairW) {
    a.cmid = cmid; a.cexp = cexp; a.cap_elems = Mp * std::max(cmid, std::max(cexp, c1));
    if (cds) { a.Ho = H; a.Wo = W; a.H2 = 2 * H; a.W2 = 2 * W; }
    pred = pairw_bf16_ok(cmid, cexp, c1, cds, M, a.cap_elems);
  } else {
    pred = cmid == 64 && cexp == 256 && (kind == kPairR || pair1x1_bf16_ok(cmid, cexp, c1, cds, M));
  }
  int (*launch)(const Pair1x1Args&, hipStream_t) =
      kind == kPairW ? launch_pairw_bf16 : kind == kPairR ? launch_pair1x1r_bf16 : launch_pair1x1_bf16;
  LaunchInfo li{-1, -1};
  Pair1x1Args p = a;
  p.plan = &li;
  const int prc = pred ? launch(p, 0) : -1;
  const long long expect = (M + tile - 1) / tile;  // rounds of `tile` pixels
  const bool grid_ok = prc == 0 && li.blocks == expect;
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  bfr::Diff dy, dz;
  dy.count = dz.count = -1;
  if (grid_ok) {
    std::vector<OutBuf> outs{{&y}, {&z}};
    rc = launch_twice(id, outs, [&] { if (inplace) y.put(hres.data(), hres.size() * 2); }, [&] { return launch(a, 0); },
                      guards, rerun);
    // the padding pixels of a pairw round are the kernel's to scribble on; the M pixels are compared
    rerun = 0;
    for (size_t i = 0; i < ref.y.size(); ++i) rerun += outs[0].first[i] != outs[0].second[i];
    for (size_t i = 0; i < ref.z.size(); ++i) rerun += outs[1].first[i] != outs[1].second[i];
    dy = bfr::compare(ref.y, outs[0].first.data());
    dz = bfr::compare(ref.z, outs[1].first.data());
  }
  const bool data_ok = cond_ok(ref.cond);
  const bool fail = !grid_ok || rc || !guards || rerun || dy.count || dz.count || !data_ok;
  static const char* kn[] = {"pair1x1", "pair1x1r", "pairw"};
  printf("%s bf16 %s %s %s N%d %dx%d %d(+ds %d/%d)->%d->%d M%lld%s | rounds of %lld: grid %lld (expected %lld) slots %lld | "
         "rc=%d differing y %lld of %zu z %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s, %lld of %lld outside "
         "+-256\n",
         fail ? "FAIL" : "ok  ", id, kn[kind], bfr::mode_name(mode), N, H, W, cmid, cds, s2, cexp, c1, M,
         inplace ? " in place" : "", tile, li.blocks, expect, li.slots, rc, dy.count, ref.y.size(), dz.count, ref.z.size(), rerun,
         guards ? "ok" : "OVERWRITTEN", ref.cond.max_sabs, data_ok ? "" : " (>= 2^24)", ref.cond.over256, ref.cond.outputs);
  print_first("y", dy, H * W, W, cexp);
  print_first("z", dz, H * W, W, c1);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dr, (void*)dx2, (void*)dw3, (void*)dw1, (void*)db3, (void*)db1}) hipFree(q);
  return fail;
}

// the whole-block stage-1 kernels: bneck_bf16 (cin 64 with the folded downsample, cin 256, cin 256
// with the next block's conv1), bneck_tail_bf16, bblock_bf16 (in place: y = x)
enum BlockKind { kBneck, kTail, kBblock };
static int bf16_block(const char* id, BlockKind kind, int mode, int N, int H, int W, int cin, bool next, bool inplace = false) {
  const int cu = device_cu_count();
  const long long M = (long long)N * H * W;
  bfr::ChainOut ref;
  BneckArgs a{};
  a.N = N; a.H = H; a.W = W; a.cin = 64;
  std::vector<void*> held;
  auto keep = [&](auto* q) { held.push_back((void*)q); return q; };
  std::vector<bfr::u16> hx;
  int cy = 256, cz = 0;
  bool pred = false;
  if (kind == kBblock) {
    const bfr::BblockCase c = bfr::make_bblock(N, H, W, mode);
    ref = bfr::run_bblock<long long>(c);
    hx = bfr::to_bf16(c.x);
    a.w1 = keep(upload(bfr::to_bf16(c.w1))); a.b1 = keep(upload(bfr::to_f32(c.b1)));
    a.w2 = keep(upload(bfr::to_bf16(c.w2))); a.b2 = keep(upload(bfr::to_f32(c.b2)));
    cy = 64;
    pred = bblock_bf16_ok(W, H);
  } else {
    const bfr::BneckCase c = bfr::make_bneck(N, H, W, cin, next, kind == kTail, mode);
    ref = bfr::run_bneck<long long>(c);
    hx = bfr::to_bf16(c.x);
    a.cin = c.cin;
    a.w1 = keep(upload(bfr::to_bf16(c.w1))); a.b1 = keep(upload(bfr::to_f32(c.b1)));
    a.w2 = keep(upload(bfr::to_bf16(c.w2))); a.b2 = keep(upload(bfr::to_f32(c.b2)));
    a.w3 = keep(upload(bfr::to_bf16(c.w3))); a.b3 = keep(upload(bfr::to_f32(c.b3)));
    if (c.next) { a.wn = keep(upload(bfr::to_bf16(c.wn))); a.bn = keep(upload(bfr::to_f32(c.bn))); cz = c.cn; }
    if (c.tail) a.res = keep(upload(bfr::to_bf16(c.res)));
    pred = kind == kTail ? bneck_tail_bf16_ok(W, H) : bneck_bf16_ok(c.cin, W, H, c.next);
    inplace = false;
  }
  Fenced y(inplace ? 0 : (size_t)M * cy * 2), z((size_t)M * cz * 2), xin(inplace ? hx.size() * 2 : 0);
  bfr::u16* dx = inplace ? (bfr::u16*)xin.p() : keep(upload(hx));
  a.x = dx; a.y = inplace ? (void*)dx : (void*)y.p(); a.z = cz ? z.p() : nullptr;
  int (*launch)(const BneckArgs&, hipStream_t) =
      kind == kBblock ? launch_bblock_bf16 : kind == kTail ? launch_bneck_tail_bf16 : launch_bneck_bf16;
  LaunchInfo li{-1, -1};
  BneckArgs p = a;
  p.plan = &li;
  const int prc = pred ? launch(p, 0) : -1;
  const bool grid_ok = prc == 0 && li.blocks == N && li.slots == cu;  // persistent: images over one workgroup per CU
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  bfr::Diff dy, dz;
  dy.count = -1;
  if (grid_ok) {
    std::vector<OutBuf> outs{{inplace ? &xin : &y}};
    if (cz) outs.push_back({&z});
    rc = launch_twice(id, outs, [&] { if (inplace) xin.put(hx.data(), hx.size() * 2); }, [&] { return launch(a, 0); }, guards,
                      rerun);
    dy = bfr::compare(ref.y, outs[0].first.data());
    if (cz) dz = bfr::compare(ref.z, outs[1].first.data());
  }
  const bool data_ok = cond_ok(ref.cond);
  const bool fail = !grid_ok || rc || !guards || rerun || dy.count || dz.count || !data_ok;
  static const char* kn[] = {"bneck", "bneck_tail", "bblock"};
  printf("%s bf16 %s %s %s N%d %dx%d cin %d next %d%s | images %lld (expected %d) slots %lld (CUs %d) | rc=%d differing y %lld of "
         "%zu z %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s, %lld of %lld outside +-256\n",
         fail ? "FAIL" : "ok  ", id, kn[kind], bfr::mode_name(mode), N, H, W, a.cin, cz, inplace ? " in place" : "", li.blocks, N,
         li.slots, cu, rc, dy.count, ref.y.size(), dz.count, ref.z.size(), rerun, guards ? "ok" : "OVERWRITTEN",
         ref.cond.max_sabs, data_ok ? "" : " (>= 2^24)", ref.cond.over256, ref.cond.outputs);
  print_first("y", dy, H * W, W, cy);
  print_first("z", dz, H * W, W, cz ? cz : 1);
  fflush(stdout);
  for (void* q : held) hipFree(q);
  return fail;
}

// launch_stem_pool_bf16: packed (the padded bf16 rows), direct (the f32 NCHW frames; W % 4 != 0 or
// an odd stem height) and column-blocked (frames, W % 4 == 0, even stem height)
enum StemKind { kPacked, kDirect, kColBlock };
static int bf16_stem(const char* id, StemKind kind, int mode, int N, int H, int W) {
  const bfr::StemCase c = bfr::make_stem(N, H, W, mode);
  const bfr::ChainOut ref = bfr::run_stem<long long>(c);
  const int pad = 3, Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  std::vector<bfr::u16> x(stem_input_elems(N, H, W, pad) + 256, 0);
  std::vector<float> fr((size_t)N * 3 * H * W);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int ch = 0; ch < 3; ++ch) {
          const int v = c.frames[(((size_t)n * H + i) * W + j) * 3 + ch];
          x[64 + (((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + ch] = bfr::bf16_rne((float)v);
          fr[(((size_t)n * 3 + ch) * H + i) * W + j] = (float)v;
        }
  bfr::u16 *dx = upload(x), *dw = upload(bfr::stem_device_weights(c));
  float *dfr = upload(fr), *db = upload(bfr::to_f32(c.bias));
  Fenced out(ref.y.size() * 2);
  const bool frames = kind != kPacked;
  auto launch = [&](LaunchInfo* info) {
    return frames ? launch_stem_pool_bf16(nullptr, N, H, W, dw, db, out.p(), 0, dfr, info)
                  : launch_stem_pool_bf16(dx + 64, N, H, W, dw, db, out.p(), 0, nullptr, info);  // 128 B front slack
  };
  const int cu = device_cu_count(), ntiles = (c.Wq + 6) / 7, ncb = (ntiles + 3) / 4;
  const bool cb = frames && W % 4 == 0 && c.Hs % 2 == 0;  // the release library's choice
  const bool pred = stem_pool_bf16_ok(H, W, frames) && cb == (kind == kColBlock);
  const long long expect = kind == kColBlock ? (long long)N * ncb : N;
  LaunchInfo li{-1, -1};
  const int prc = pred ? launch(&li) : -1;
  const bool grid_ok = prc == 0 && li.blocks == expect && (kind == kColBlock || li.slots == cu);
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  bfr::Diff d;
  d.count = -1;
  if (grid_ok) {
    std::vector<OutBuf> outs{{&out}};
    rc = launch_twice(id, outs, [] {}, [&] { return launch(nullptr); }, guards, rerun);
    d = bfr::compare(ref.y, outs[0].first.data());
  }
  const bool data_ok = cond_ok(ref.cond);
  const bool fail = !grid_ok || rc || !guards || rerun || d.count || !data_ok;
  static const char* kn[] = {"packed", "direct", "column-blocked"};
  printf("%s bf16 %s stem_pool %s %s N%d %dx%d (stem %dx%d, pooled %dx%d, %d column tiles) | grid %lld (expected %lld) slots %lld "
         "| rc=%d differing %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s, %lld of %lld outside +-256\n",
         fail ? "FAIL" : "ok  ", id, kn[kind], bfr::mode_name(mode), N, H, W, c.Hs, c.Ws, c.Hq, c.Wq, ntiles, li.blocks, expect,
         li.slots, rc, d.count, ref.y.size(), rerun, guards ? "ok" : "OVERWRITTEN", ref.cond.max_sabs,
         data_ok ? "" : " (>= 2^24)", ref.cond.over256, ref.cond.outputs);
  print_first("y", d, c.Hq * c.Wq, c.Wq, 64);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)dfr, (void*)db}) hipFree(q);
  return fail;
}

// the unfused bf16 stem, where the fused kernel refuses the frame size: launch_conv_bf16 with Cin 3
// (conv_bf16_kernel<128, 64, 2, 2, STEM>) on the padded RGB rows, K = [kh][24] padded to 192
static int bf16_stem_conv(const char* id, int mode, int N, int H, int W) {
  const bfr::StemCase c = bfr::make_stem(N, H, W, mode);
  bfr::Cond cond;
  const std::vector<int> ref = bfr::run_stage<long long>(bfr::stem_stage(c), bfr::kNone, true, &cond);
  const int pad = 3, Wp = stem_row_pixels(W, pad), Hp = H + 2 * pad;
  std::vector<bfr::u16> x(stem_input_elems(N, H, W, pad), 0);
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j)
        for (int ch = 0; ch < 3; ++ch)
          x[(((size_t)n * Hp + i + pad) * Wp + j + pad) * 3 + ch] = bfr::bf16_rne((float)c.frames[(((size_t)n * H + i) * W + j) * 3 + ch]);
  bfr::u16 *dx = upload(x), *dw = upload(bfr::stem_device_weights(c));
  float* db = upload(bfr::to_f32(c.bias));
  void* dz;
  hipMalloc(&dz, 256);
  hipMemset(dz, 0, 256);
  const long long M = (long long)N * c.Hs * c.Ws;
  Fenced out((size_t)M * 64 * 2);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.y = out.p();
  a.N = N; a.H = H; a.W = W; a.Cin = 3; a.Ho = c.Hs; a.Wo = c.Ws; a.Cout = 64;
  a.KH = a.KW = 7; a.KWp = 8; a.stride = 2; a.pad = pad; a.K = 192; a.relu = 1; a.zero = dz; a.xcd = 1; a.xs = 3;
  LaunchInfo li{-1, -1};
  ConvArgs p = a;
  p.plan = &li;
  const int prc = launch_conv_bf16(p, 0);
  const long long expect = (M + 127) / 128;
  const bool grid_ok = prc == 0 && li.blocks == expect;
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  bfr::Diff d;
  d.count = -1;
  if (grid_ok) {
    std::vector<OutBuf> outs{{&out}};
    rc = launch_twice(id, outs, [] {}, [&] { return launch_conv_bf16(a, 0); }, guards, rerun);
    d = bfr::compare(ref, outs[0].first.data());
  }
  const bool data_ok = cond_ok(cond);
  const bool fail = !grid_ok || rc || !guards || rerun || d.count || !data_ok;
  printf("%s bf16 %s stem conv %s N%d %dx%d -> %dx%d M%lld | 128x64 (stem) grid %lld (expected %lld) slots %lld | rc=%d differing "
         "%lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s, %lld of %lld outside +-256\n",
         fail ? "FAIL" : "ok  ", id, bfr::mode_name(mode), N, H, W, c.Hs, c.Ws, M, li.blocks, expect, li.slots, rc, d.count,
         ref.size(), rerun, guards ? "ok" : "OVERWRITTEN", cond.max_sabs, data_ok ? "" : " (>= 2^24)", cond.over256, cond.outputs);
  print_first("y", d, c.Hs * c.Ws, c.Ws, 64);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)db, dz}) hipFree(q);
  return fail;
}

static int run_bf16(const char* group) {
  using namespace bfr;
  int f = 0;
  bool known = false;
  auto is = [&](const char* g) {
    const bool m = !strcmp(group, g);
    known |= m;
    return m;
  };
  const int cu = device_cu_count();
  // a persistent kernel's "trips" case: 2 cu + 3 work items, so every workgroup takes a second item,
  // some a third, and the last trip is ragged; many images of the smallest map
  const int trips = 2 * cu + 3;
  if (is("rows")) {
    // conv_rows_bf16 (W 56, H % 4 == 0, 64 -> 64) through launch_conv_bf16; strips of 4 rows
    for (int res = 0; res < 2; ++res)
      for (int relu = 0; relu < 2; ++relu) f += bf16_conv("rows.trips", kRows, kInt, trips, 4, 56, 64, 64, 3, 1, 1, 0, 0, res, relu, false);
    // ... the same shape, conv_rowsr_bf16 <64, 56> called directly
    f += bf16_conv("rowsr.64x56.trips", kRowsr, kInt, trips, 4, 56, 64, 64, 3, 1, 1, 0, 0, true, true, false);
    for (int mode = 0; mode < 2; ++mode) {
      f += bf16_conv("rows.one", kRows, mode, 1, 4, 56, 64, 64, 3, 1, 1, 0, 0, true, true, false);  // one strip, both borders
      for (int res = 0; res < 2; ++res)
        for (int relu = 0; relu < 2; ++relu) {
          f += bf16_conv("rows.mid", kRows, mode, 3, 12, 56, 64, 64, 3, 1, 1, 0, 0, res, relu, false);  // 9 strips, interior ones
          f += bf16_conv("rowsr.64x56", kRowsr, mode, 3, 12, 56, 64, 64, 3, 1, 1, 0, 0, res, relu, false);
        }
    }
    // conv_rowsr_bf16: every shape rowsr_shape accepts, C 128 in both K orders; <64, 64> is also what
    // launch_conv_bf16 picks for that shape
    f += bf16_conv("rowsr.64x64.trips", kRowsrDispatch, kInt, trips, 4, 64, 64, 64, 3, 1, 1, 0, 0, true, true, false);
    f += bf16_conv("rowsr.128x28.trips", kRowsr, kInt, trips, 4, 28, 128, 128, 3, 1, 1, 0, 0, true, true, true);
    f += bf16_conv("rowsr.128x32.trips", kRowsr, kInt, trips, 4, 32, 128, 128, 3, 1, 1, 0, 0, true, true, false);
    for (int mode = 0; mode < 2; ++mode)
      for (int res = 0; res < 2; ++res)
        for (int relu = 0; relu < 2; ++relu) {
          f += bf16_conv("rowsr.64x64", kRowsr, mode, 3, 8, 64, 64, 64, 3, 1, 1, 0, 0, res, relu, false);
          f += bf16_conv("rowsr.64x64.dispatch", kRowsrDispatch, mode, 3, 8, 64, 64, 64, 3, 1, 1, 0, 0, res, relu, false);
          for (int kcm = 0; kcm < 2; ++kcm) {
            f += bf16_conv("rowsr.128x28", kRowsr, mode, 3, 8, 28, 128, 128, 3, 1, 1, 0, 0, res, relu, kcm);
            f += bf16_conv("rowsr.128x32", kRowsr, mode, 3, 8, 32, 128, 128, 3, 1, 1, 0, 0, res, relu, kcm);
          }
        }
    f += bf16_conv("rowsr.one", kRowsr, kInt, 1, 4, 28, 128, 128, 3, 1, 1, 0, 0, true, true, true);
    // conv_s2rows_bf16: 3x3/2 64 -> 128 at 56x56 only, 7 strips per image; it refuses a residual
    // (gemm.g512.s2.res below is where that goes)
    f += bf16_conv("s2rows.trips", kS2rows, kInt, (trips + 6) / 7, 56, 56, 64, 128, 3, 2, 1, 0, 0, false, true, false);
    for (int mode = 0; mode < 2; ++mode)
      for (int relu = 0; relu < 2; ++relu) {
        f += bf16_conv("s2rows.one", kS2rows, mode, 1, 56, 56, 64, 128, 3, 2, 1, 0, 0, false, relu, false);
        f += bf16_conv("s2rows", kS2rows, mode, 3, 56, 56, 64, 128, 3, 2, 1, 0, 0, false, relu, false);
      }
  }
  if (is("gemm")) {
    // tap-shift kernel (conv_bf16_ts_ws_kernel<512, 128>): stride-1 3x3 with Cout 128
    for (int kcm = 0; kcm < 2; ++kcm) {
      f += bf16_conv("ts.below", kTs, kInt, 2, 9, 11, 128, 128, 3, 1, 1, 0, 0, true, false, kcm);  // M 198 < one tile, odd map
      f += bf16_conv("ts.past", kTs, kInt, 1, 19, 27, 128, 128, 3, 1, 1, 0, 0, true, true, kcm);   // M 513: one pixel past a tile
      f += bf16_conv("ts.past", kTs, kInt, 1, 19, 27, 128, 128, 3, 1, 1, 0, 0, false, true, kcm);
    }
    f += bf16_conv("ts.past", kTs, kRound, 1, 19, 27, 128, 128, 3, 1, 1, 0, 0, true, true, true);
    f += bf16_conv("ts.c64", kTs, kInt, 3, 14, 14, 64, 128, 3, 1, 1, 0, 0, false, true, false);    // M 588
    f += bf16_conv("ts.ds", kTs, kInt, 3, 14, 14, 128, 128, 3, 1, 1, 64, 2, false, true, true);    // R18 layer2.0.conv2
    f += bf16_conv("ts.ds", kTs, kRound, 3, 14, 14, 128, 128, 3, 1, 1, 64, 2, false, true, true);
    // 512x128 tile (conv_bf16_ws_kernel<512, 128, 4, 2, 4, 0>): 1x1s, stride-2 3x3s that s2rows
    // refuses, the folded downsample on a 1x1
    f += bf16_conv("g512.1x1", kG512, kInt, 3, 14, 14, 256, 128, 1, 1, 0, 0, 0, false, true, false);  // M 588
    f += bf16_conv("g512.1x1", kG512, kRound, 3, 14, 14, 256, 128, 1, 1, 0, 0, 0, true, true, false);
    f += bf16_conv("g512.1x1.below", kG512, kInt, 2, 9, 11, 512, 128, 1, 1, 0, 0, 0, true, false, false);
    f += bf16_conv("g512.1x1.past", kG512, kInt, 1, 19, 27, 64, 128, 1, 1, 0, 0, 0, false, true, false);  // M 513
    f += bf16_conv("g512.s2.ragged", kG512, kInt, 3, 13, 11, 64, 128, 3, 2, 1, 0, 0, false, true, false);  // 7x6 maps
    f += bf16_conv("g512.s2.ragged", kG512, kRound, 3, 13, 11, 64, 128, 3, 2, 1, 0, 0, false, true, false);
    f += bf16_conv("g512.s2.res", kG512, kInt, 1, 56, 56, 64, 128, 3, 2, 1, 0, 0, true, true, false);  // the s2rows shape + residual
    f += bf16_conv("g512.s2.kcm", kG512, kInt, 2, 28, 28, 128, 128, 3, 2, 1, 0, 0, false, true, true);
    f += bf16_conv("g512.1x1s2", kG512, kInt, 2, 13, 11, 64, 128, 1, 2, 0, 0, 0, false, false, false);
    f += bf16_conv("g512.ds", kG512, kInt, 2, 7, 5, 64, 128, 1, 1, 0, 64, 2, false, true, false);
    f += bf16_conv("g512.ds", kG512, kRound, 2, 7, 5, 64, 128, 1, 1, 0, 64, 2, false, true, false);
    // 256x256 tile (conv_bf16_ws_kernel<256, 256, 2, 4, 4, 3>): stride-1 3x3s in both K orders (kcm:
    // the library's weights at Cin >= 128), 1x1s, stride-2 3x3s, the folded downsample, two cout tiles
    for (int kcm = 0; kcm < 2; ++kcm) {
      f += bf16_conv("g256.3x3", kG256, kInt, 2, 14, 14, 256, 256, 3, 1, 1, 0, 0, true, true, kcm);  // M 392
      f += bf16_conv("g256.3x3.ragged", kG256, kInt, 3, 10, 12, 128, 256, 3, 1, 1, 0, 0, true, false, kcm);  // M 360
    }
    f += bf16_conv("g256.3x3", kG256, kRound, 2, 14, 14, 256, 256, 3, 1, 1, 0, 0, true, true, true);
    f += bf16_conv("g256.3x3.c512", kG256, kInt, 3, 7, 7, 512, 512, 3, 1, 1, 0, 0, false, true, true);  // M 147 < one tile, two cout tiles
    f += bf16_conv("g256.3x3.c512", kG256, kRound, 3, 7, 7, 512, 512, 3, 1, 1, 0, 0, true, true, true);
    f += bf16_conv("g256.1x1", kG256, kInt, 3, 20, 20, 64, 256, 1, 1, 0, 0, 0, true, true, false);  // M 1200
    f += bf16_conv("g256.1x1.past", kG256, kInt, 1, 1, 257, 64, 256, 1, 1, 0, 0, 0, true, true, false);  // M 257
    f += bf16_conv("g256.1x1.k1024", kG256, kInt, 2, 7, 7, 1024, 256, 1, 1, 0, 0, 0, false, true, false);
    f += bf16_conv("g256.1x1.k1024", kG256, kRound, 2, 7, 7, 1024, 256, 1, 1, 0, 0, 0, false, true, false);
    f += bf16_conv("g256.1x1.c1024", kG256, kInt, 2, 7, 7, 256, 1024, 1, 1, 0, 0, 0, true, true, false);  // four cout tiles
    f += bf16_conv("g256.s2", kG256, kInt, 3, 13, 11, 128, 256, 3, 2, 1, 0, 0, false, true, true);
    f += bf16_conv("g256.s2", kG256, kInt, 3, 13, 11, 128, 256, 3, 2, 1, 0, 0, false, true, false);
    f += bf16_conv("g256.ds.s1", kG256, kInt, 2, 9, 11, 64, 256, 1, 1, 0, 64, 1, false, true, false);   // R50 layer1.0
    f += bf16_conv("g256.ds.s2", kG256, kInt, 2, 7, 5, 128, 512, 1, 1, 0, 256, 2, false, true, false);  // R50 layer2.0
    f += bf16_conv("g256.ds.s2", kG256, kRound, 2, 7, 5, 128, 512, 1, 1, 0, 256, 2, false, true, false);
    f += bf16_conv("g256.ds.3x3", kG256, kInt, 2, 7, 7, 256, 256, 3, 1, 1, 128, 2, false, true, true);  // R18 layer3.0.conv2
    // 128x64 tile (conv_bf16_kernel<128, 64, 2, 2>): Cout 64 off the row-strip shapes
    f += bf16_conv("g64.1x1", kG64, kInt, 3, 20, 20, 256, 64, 1, 1, 0, 0, 0, false, true, false);  // M 1200
    f += bf16_conv("g64.1x1", kG64, kRound, 3, 20, 20, 256, 64, 1, 1, 0, 0, 0, true, true, false);
    f += bf16_conv("g64.3x3.ragged", kG64, kInt, 2, 9, 11, 64, 64, 3, 1, 1, 0, 0, true, true, false);  // M 198
    f += bf16_conv("g64.below", kG64, kInt, 1, 5, 7, 64, 64, 3, 1, 1, 0, 0, true, false, false);       // M 35
    f += bf16_conv("g64.past", kG64, kInt, 1, 3, 43, 64, 64, 1, 1, 0, 0, 0, false, true, false);       // M 129
    // ... and its STEM instantiation (Cin 3): odd sizes with an M tail, M one pixel past a tile
    for (int mode = 0; mode < 2; ++mode) f += bf16_stem_conv("g64.stem", mode, 3, 37, 33);  // 19x17 maps, M 969
    f += bf16_stem_conv("g64.stem.past", kInt, 1, 5, 85);                                    // 3x43, M 129
  }
  if (is("pair") || is("pairw2") || is("pairw3")) {
    const bool wide = strcmp(group, "pair") != 0, stage3 = !strcmp(group, "pairw3");
    // the trips case needs the slots of each instantiation: planned on one pixel first
    auto slots_of = [&](PairKind kind, int cmid, int cexp, int c1, int cds) {
      LaunchInfo li{-1, -1};
      Pair1x1Args p{};
      int dummy = 0;
      p.x = p.x2 = p.res = p.w3 = p.w1 = p.y = p.z = &dummy;
      p.b3 = p.b1 = (const float*)&dummy;
      if (cds) p.res = nullptr; else p.x2 = nullptr;
      p.M = 64; p.c1 = c1; p.cds = cds; p.cmid = cmid; p.cexp = cexp; p.plan = &li;
      p.cap_elems = 1LL << 40; p.Ho = p.Wo = 8; p.H2 = p.W2 = 16;
      const int rc = kind == kPairW ? launch_pairw_bf16(p, 0) : launch_pair1x1r_bf16(p, 0);
      return rc ? -1LL : li.slots;
    };
    if (!wide) {
      // every (c1, cds) the stage-1 pair takes (cmid 64, cexp 256): residual c1 64 / 128, downsample c1 64
      const int shapes[3][2] = {{64, 0}, {128, 0}, {64, 64}};
      for (const auto& s : shapes) {
        const int c1 = s[0], cds = s[1];
        for (int mode = 0; mode < 2; ++mode) {
          f += bf16_pair("pair.one", kPair, mode, 1, 8, 8, 64, 256, c1, cds);      // M 64: one partial round
          f += bf16_pair("pair.rounds", kPair, mode, 5, 8, 24, 64, 256, c1, cds);  // M 960: 3.75 / 7.5 rounds
          f += bf16_pair("pairr.ragged", kPairR, mode, 3, 9, 11, 64, 256, c1, cds);  // M 297, not a multiple of 16
        }
        f += bf16_pair("pairr.tiny", kPairR, kInt, 1, 7, 5, 64, 256, c1, cds);  // M 35
        // 2 slots + 3 rounds of 8x8 images, the last round 64 pixels short (pair1x1 takes M % 64 == 0;
        // pairr.ragged above has the tail that is no multiple of 16)
        const long long slots = slots_of(kPairR, 64, 256, c1, cds), tile = cds || c1 == 64 ? 256 : 128;
        if (slots <= 0) { printf("FAIL bf16 pair.trips: no plan\n"); ++f; continue; }
        const int n = (int)((2 * slots + 3) * tile / 64 - 1);  // the last round 64 pixels short
        f += bf16_pair("pair.trips", kPair, kInt, n, 8, 8, 64, 256, c1, cds);
      }
    } else {
      // every (cmid, cexp, c1, cds) pairw_bf16_ok accepts -- group pairw2 the stage-2 shapes (cmid
      // 128), pairw3 the stage-3 one (cmid 256); NaN padding always, in place where the engine runs
      // it so (residual pairs)
      const int shapes[4][4] = {{128, 512, 128, 0}, {128, 512, 256, 0}, {128, 512, 128, 256}, {256, 1024, 256, 0}};
      for (const auto& s : shapes) {
        const int cmid = s[0], cexp = s[1], c1 = s[2], cds = s[3];
        if ((cmid == 256) != stage3) continue;
        for (int mode = 0; mode < 2; ++mode) {
          f += bf16_pair("pairw.tiny", kPairW, mode, 1, 7, 5, cmid, cexp, c1, cds, mode == 1);  // M 35: one partial round
          f += bf16_pair("pairw.ragged", kPairW, mode, 3, 14, 14, cmid, cexp, c1, cds, mode == 0);  // M 588: 4.6 / 2.3 rounds
        }
        const long long slots = slots_of(kPairW, cmid, cexp, c1, cds), tile = pairw_tile(cmid, c1, cds);
        if (slots <= 0) { printf("FAIL bf16 pairw.trips: no plan\n"); ++f; continue; }
        // 7x5 images: (2 slots + 2) rounds and a ragged one
        const int n = (int)(((2 * slots + 2) * tile + 34) / 35 + 1);
        f += bf16_pair("pairw.trips", kPairW, kInt, n, 7, 5, cmid, cexp, c1, cds, true);
      }
    }
  }
  if (is("block")) {
    const int sizes[4][2] = {{2, 56}, {6, 56}, {2, 64}, {6, 64}};  // (H, W): the smallest legal map and three steps
    for (const auto& s : sizes) {
      const int H = s[0], W = s[1];
      for (int mode = 0; mode < 2; ++mode) {
        if (mode == kRound && H == 2) continue;  // round mode on the H 6 maps
        f += bf16_block("bneck.ds", kBneck, mode, 3, H, W, 64, false);
        f += bf16_block("bneck.256", kBneck, mode, 3, H, W, 256, false);
        f += bf16_block("bneck.next", kBneck, mode, 3, H, W, 256, true);
        f += bf16_block("tail", kTail, mode, 3, H, W, 64, false);
        f += bf16_block("bblock", kBblock, mode, 3, H, W, 64, false, false);
        f += bf16_block("bblock", kBblock, mode, 3, H, W, 64, false, true);
      }
    }
    f += bf16_block("bneck.one", kBneck, kInt, 1, 2, 56, 64, false);  // one image, one step
    // every workgroup walks 2-3 images: the stream crosses image borders, the last trip is ragged
    f += bf16_block("bneck.ds.trips", kBneck, kInt, trips, 2, 56, 64, false);
    f += bf16_block("bneck.256.trips", kBneck, kInt, trips, 2, 56, 256, false);
    f += bf16_block("bneck.next.trips", kBneck, kInt, trips, 2, 64, 256, true);
    f += bf16_block("tail.trips", kTail, kInt, trips, 2, 56, 64, false);
    f += bf16_block("bblock.trips", kBblock, kInt, trips, 2, 64, 64, false, true);
  }
  if (is("stem")) {
    for (int mode = 0; mode < 2; ++mode) {
      f += bf16_stem("stem.8x8", kPacked, mode, 3, 8, 8);       // the smallest legal size
      f += bf16_stem("stem.8x8", kColBlock, mode, 3, 8, 8);
      f += bf16_stem("stem.10x10", kDirect, mode, 3, 10, 10);   // the smallest direct size: odd stem height 5
      f += bf16_stem("stem.100x86", kPacked, mode, 3, 100, 86);  // partial last column tile (pooled 25 x 22)
      f += bf16_stem("stem.100x86", kDirect, mode, 3, 100, 86);
      f += bf16_stem("stem.38x30", kPacked, mode, 2, 38, 30);   // stem 19x15, pooled 10x8: odd stem sizes
      f += bf16_stem("stem.38x30", kDirect, mode, 2, 38, 30);
      f += bf16_stem("stem.100x88", kColBlock, mode, 3, 100, 88);  // W % 4 == 0, one partial column block
      f += bf16_stem("stem.60x36", kColBlock, mode, 2, 60, 36);
    }
    f += bf16_stem("stem.64x256", kColBlock, kInt, 2, 64, 256);  // 10 column tiles: 3 column blocks, the last partial
  }
  if (!known) printf("FAIL bf16: unknown group %s\n", group), ++f;
  printf("%d failures\n", f);
  return f ? 1 : 0;
}

// ------------------------------------------------------------------ f32: `conv_check f32 <group>`
// The exact-f32 inference kernels one by one against bf16_ref.h's int64 reference on integer data
// (f32_ref.h): the f32 output is not converted, so every output of every image is held bitwise (-0
// folded into +0).  Outputs prefilled with 0xff between two 4-KiB guards, every launch twice,
// ConvArgs::xcd = 1 as the engine sets it (ragged grids also with 0), the planned grid pinned to the
// kernel the case is meant for.  DESIGN.md section 3F maps every release dispatch branch to its case.

enum F32Route { kFRows, kFD256x64, kFD128x64, kFHead, kFW256, kFW128, kFK256, kFK128 };
static const char* f32_route_name(F32Route r) {
  static const char* n[] = {"conv_rows_f32", "dma 256x64", "dma 128x64", "dma 128x64 per-element", "ws 256x128", "ws 128x128",
                            "dma 256x128 (split-K)", "dma 128x128 (split-K)"};
  return n[r];
}
// what the release library's launch_conv_f32 does with a non-stem conv, from its predicates and
// device_cu_count(); *grid: that kernel's grid (the row kernel: its strips; split-K: one slice's).  With a
// split-K workspace (ConvArgs::kws, the training entry) the large tiles are launch_dma's.
static F32Route f32_dispatch(const ConvArgs& a, long long* grid) {
  const long long M = (long long)a.N * a.Ho * a.Wo, cu = device_cu_count();
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn); };
  if (!a.kcm && conv_rows_f32_ok(a)) return *grid = (long long)a.N * (a.H / 2), kFRows;
  if (a.Cout % 4) return *grid = blocks(128, 64), kFHead;
  if (a.Cout <= 64) return *grid = blocks(256, 64), kFD256x64;
  if (a.Cout <= 256 && blocks(256, 128) >= cu) return *grid = blocks(256, 128), a.kws ? kFK256 : kFW256;
  if (blocks(128, 128) >= cu) return *grid = blocks(128, 128), a.kws ? kFK128 : kFW128;
  return *grid = blocks(128, 64), kFD128x64;
}
static void print_first_f32(const char* what, const f32r::Diff& d, int HW, int W, int C) {
  if (d.count <= 0) return;
  const long long p = d.first / C;
  printf("  first differing %s: image %lld row %lld col %lld ch %lld: want %lld got %.9g\n", what, p / HW, p % HW / W, p % W,
         d.first % C, d.want, d.got);
}
static long long f32_failures = 0, f32_cases = 0;

// One conv through launch_conv_f32.  kcm: the chunk of the chunk-major K order (0: tap-major).  The
// reference of the conv part (before residual and ReLU) is shared by consecutive cases on one shape.
// slices > 0: with a split-K workspace of exactly the bytes that many slices need, fenced like the
// output; conv_f32_ksplit_slices must plan that many.
static int f32_conv(const char* id, F32Route route, int mode, int N, int H, int W, int C, int Cout, int k, int stride, int pad,
                    int Cds, int s2, bool res, bool relu, int kcm, int xcd = 1, int slices = 0) {
  static bfr::ConvCase c;
  static std::vector<int> raw;
  static bfr::Cond cond;
  static bool have = false;
  {
    bfr::ConvCase q;
    q.N = N, q.H = H, q.W = W, q.C = C, q.Cout = Cout, q.k = k, q.stride = stride, q.pad = pad, q.Cds = Cds, q.s2 = s2, q.mode = mode;
    if (!have || !c.same_shape(q)) {
      c = bfr::make_conv(N, H, W, C, Cout, k, stride, pad, Cds, s2, mode);
      cond = bfr::Cond();
      raw = bfr::run_stage<long long>(c.stage(false, false), bfr::kNone, false, &cond);
      have = true;
    }
  }
  const long long M = c.M();
  std::vector<int> ref(raw.size());
  for (size_t i = 0; i < raw.size(); ++i) {
    long long v = raw[i] + (res ? c.res[i] : 0);
    if (relu && v < 0) v = 0;
    ref[i] = (int)v;
  }
  float *dx = upload(bfr::to_f32(c.x)), *dw = upload(f32r::device_weights(c.w, Cout, c.K, c.K1, k * k, C, kcm)),
        *dr = upload(bfr::to_f32(c.res)), *dx2 = Cds ? upload(bfr::to_f32(c.x2)) : nullptr, *db = upload(bfr::to_f32(c.bias));
  void* dz;
  hipMalloc(&dz, 256);
  hipMemset(dz, 0, 256);
  Fenced out((size_t)M * Cout * 4);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.res = res ? dr : nullptr; a.y = out.p();
  a.N = N; a.H = H; a.W = W; a.Cin = C; a.Ho = c.Ho; a.Wo = c.Wo; a.Cout = Cout;
  a.KH = a.KW = a.KWp = k; a.stride = stride; a.pad = pad; a.K = c.K; a.relu = relu; a.zero = dz;
  a.xcd = xcd; a.kcm = kcm;
  if (Cds) { a.x2 = dx2; a.H2 = c.H2; a.W2 = c.W2; a.Cin2 = Cds; a.stride2 = s2; a.K1 = c.K1; }
  Fenced ws(slices ? (size_t)slices * M * Cout * 4 : 16);
  const int planned = conv_f32_ksplit_slices(a);
  if (slices) a.kws = (float*)ws.p(), a.kws_bytes = (long long)ws.n;
  long long expect = -1;
  const F32Route taken = f32_dispatch(a, &expect);
  LaunchInfo li{-1, -1};
  ConvArgs p = a;
  p.plan = &li;
  const int prc = launch_conv_f32(p, 0);
  const bool grid_ok = prc == 0 && taken == route && li.blocks == expect && (route != kFRows || li.slots == device_cu_count()) &&
                       (!slices || planned == slices);
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  f32r::Diff d;
  d.count = -1;
  if (grid_ok) {  // the wrong kernel is not run: the case has failed already
    std::vector<OutBuf> outs{{&out}, {&ws}};  // the slices' partial sums too: fenced, and equal in both runs
    rc = launch_twice(id, outs, [] {}, [&] { return launch_conv_f32(a, 0); }, guards, rerun);
    d = f32r::compare(ref, (const float*)outs[0].first.data());
  }
  const long long extra = res ? bfr::max_abs(c.res.data(), c.res.size()) : 0;
  const bool data_ok = cond_ok(cond, extra);
  const bool fail = !grid_ok || rc || !guards || rerun || d.count || !data_ok;
  printf("%s f32 %s %s N%d %dx%d %d->%d k%d s%d res%d relu%d kcm%d ds%d/%d xcd%d M%lld | %s grid %lld (expected %lld, %% 8 = %lld) "
         "slots %lld slices %d (expected %d) dispatch %s | rc=%d differing %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s\n",
         fail ? "FAIL" : "ok  ", id, bfr::mode_name(mode), N, H, W, C, Cout, k, stride, res, relu, kcm, Cds, s2, xcd, M,
         f32_route_name(route), li.blocks, expect, expect % 8, li.slots, slices ? planned : 1, slices ? slices : 1,
         taken == route ? "ok" : f32_route_name(taken), rc,
         d.count, ref.size(), rerun, guards ? "ok" : "OVERWRITTEN", cond.max_sabs + extra, data_ok ? "" : " (>= 2^24)");
  print_first_f32("y", d, c.Ho * c.Wo, c.Wo, Cout);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)dr, (void*)dx2, (void*)db, dz}) hipFree(q);
  ++f32_cases, f32_failures += fail;
  return fail;
}

// the band count launch_stem_pool_f32 plans: fewest (rounds of the grid over the slots) x (stem rows
// per band), at most 8 and at most the pooled height
static int f32_stem_bands(long long B, int Hq, long long slots) {
  int best = 1;
  long long best_cost = -1;
  for (int b = 1; b <= 8 && b <= Hq; ++b) {
    const int rpb = (Hq + b - 1) / b;
    const long long cost = ((B * b + slots - 1) / slots) * (2LL * rpb + (b > 1));
    if (best_cost < 0 || cost < best_cost) best = b, best_cost = cost;
  }
  return best;
}

// launch_stem_pool_f32 on one frame size: the packed rows, the f32 NCHW frames (direct) where
// stem_pool_f32_direct_ok, each with the f32 output and with the split (hi, lo) bf16 output; direct
// bitwise against pack.  multi: the planned grid must show more than one band per image.
static int f32_stem(const char* id, int mode, int N, int H, int W, bool multi = false) {
  const bfr::StemCase c = bfr::make_stem(N, H, W, mode);
  const bfr::ChainOut ref = f32r::run_stem<long long>(c);
  const int Wp = stem_row_pixels(W, 3), nt = (c.Ws + 15) / 16, cu = device_cu_count();
  float *dx = upload(f32r::stem_pack(c, Wp, stem_input_elems(N, H, W, 3) + 64)), *dw = upload(f32r::stem_device_weights(c)),
        *dfr = upload(f32r::stem_frames(c)), *db = upload(bfr::to_f32(c.bias));
  const bool data_ok = cond_ok(ref.cond);
  const bool can_direct = stem_pool_f32_direct_ok(H, W);
  int fails = 0;
  std::vector<bfr::u16> pack_bits[2];
  for (int split = 0; split < 2; ++split)
    for (int direct = 0; direct < 2; ++direct) {
      if (direct && !can_direct) continue;
      Fenced out(ref.y.size() * 4);  // f32: 64 floats per pooled pixel; split: 64 hi + 64 lo bf16
      auto launch = [&](LaunchInfo* info) {
        return direct ? launch_stem_pool_f32(nullptr, N, H, W, dw, db, out.p(), 0, split != 0, info, dfr)
                      : launch_stem_pool_f32(dx, N, H, W, dw, db, out.p(), 0, split != 0, info);
      };
      LaunchInfo li{-1, -1};
      const int prc = stem_pool_f32_ok(H, W) ? launch(&li) : -1;
      const bool slots_ok = prc == 0 && li.slots >= cu && li.slots % cu == 0;
      const int bands = slots_ok ? f32_stem_bands(N, c.Hq, li.slots) : -1;
      const bool grid_ok = slots_ok && li.blocks == (long long)N * bands && (!multi || bands > 1);
      int rc = -1;
      bool guards = true;
      long long rerun = -1, inexact = 0, vs_pack = 0;
      f32r::Diff d;
      d.count = -1;
      if (grid_ok) {
        std::vector<OutBuf> outs{{&out}};
        rc = launch_twice(id, outs, [] {}, [&] { return launch(nullptr); }, guards, rerun);
        d = split ? f32r::compare_split(ref.y, outs[0].first.data(), &inexact) : f32r::compare(ref.y, (const float*)outs[0].first.data());
        if (!direct) pack_bits[split] = outs[0].first;
        else if (pack_bits[split].size() != outs[0].first.size()) vs_pack = -1;  // the pack run failed: nothing to compare with
        else
          for (size_t i = 0; i < pack_bits[split].size(); ++i) vs_pack += pack_bits[split][i] != outs[0].first[i];
      }
      // int mode: every value fits hi + lo exactly, so the split output shows the f32 value whole
      const bool split_ok = !(split && mode == bfr::kInt && inexact);
      const bool fail = !grid_ok || rc || !guards || rerun || d.count || vs_pack || !data_ok || !split_ok;
      printf("%s f32 %s stem_pool NT %d %s %s %s N%d %dx%d (stem %dx%d, pooled %dx%d) | grid %lld (expected %d x %d bands) slots %lld "
             "| rc=%d differing %lld of %zu rerun %lld guards %s%s | data: sum|terms| <= %lld%s",
             fail ? "FAIL" : "ok  ", id, nt, direct ? "direct" : "pack  ", split ? "split" : "plain", bfr::mode_name(mode), N, H, W,
             c.Hs, c.Ws, c.Hq, c.Wq, li.blocks, N, bands, li.slots, rc, d.count, ref.y.size(), rerun, guards ? "ok" : "OVERWRITTEN",
             !direct ? "" : vs_pack ? " direct DIFFERS from pack" : " direct = pack", ref.cond.max_sabs, data_ok ? "" : " (>= 2^24)");
      if (split) printf(", hi + lo inexact at %lld outputs", inexact);
      printf("\n");
      print_first_f32("y", d, c.Hq * c.Wq, c.Wq, 64);
      fflush(stdout);
      ++f32_cases, f32_failures += fail, fails += fail;
    }
  for (void* q : {(void*)dx, (void*)dw, (void*)dfr, (void*)db}) hipFree(q);
  return fails;
}

// the unfused f32 stem: launch_conv_f32 with Cin 3 (conv_f32_dma_kernel<128, 64, 16, 2, 2, STEM>) on the
// padded RGB rows, K = [kh][24] padded to 176
static int f32_stem_conv(const char* id, int mode, int N, int H, int W, int xcd = 1) {
  const bfr::StemCase c = bfr::make_stem(N, H, W, mode);
  bfr::Cond cond;
  const std::vector<int> ref = bfr::run_stage<long long>(bfr::stem_stage(c), bfr::kNone, false, &cond);
  const int Wp = stem_row_pixels(W, 3);
  float *dx = upload(f32r::stem_pack(c, Wp, stem_input_elems(N, H, W, 3))), *dw = upload(f32r::stem_device_weights(c)),
        *db = upload(bfr::to_f32(c.bias));
  void* dz;
  hipMalloc(&dz, 256);
  hipMemset(dz, 0, 256);
  const long long M = (long long)N * c.Hs * c.Ws;
  Fenced out((size_t)M * 64 * 4);
  ConvArgs a{};
  a.x = dx; a.w = dw; a.bias = db; a.y = out.p();
  a.N = N; a.H = H; a.W = W; a.Cin = 3; a.Ho = c.Hs; a.Wo = c.Ws; a.Cout = 64;
  a.KH = a.KW = 7; a.KWp = 8; a.stride = 2; a.pad = 3; a.K = 176; a.relu = 1; a.zero = dz; a.xcd = xcd;
  LaunchInfo li{-1, -1};
  ConvArgs p = a;
  p.plan = &li;
  const int prc = launch_conv_f32(p, 0);
  const long long expect = (M + 127) / 128;
  const bool grid_ok = prc == 0 && li.blocks == expect;
  int rc = -1;
  bool guards = true;
  long long rerun = -1;
  f32r::Diff d;
  d.count = -1;
  if (grid_ok) {
    std::vector<OutBuf> outs{{&out}};
    rc = launch_twice(id, outs, [] {}, [&] { return launch_conv_f32(a, 0); }, guards, rerun);
    d = f32r::compare(ref, (const float*)outs[0].first.data());
  }
  const bool data_ok = cond_ok(cond);
  const bool fail = !grid_ok || rc || !guards || rerun || d.count || !data_ok;
  printf("%s f32 %s stem conv %s N%d %dx%d -> %dx%d xcd%d M%lld | dma 128x64 (stem) grid %lld (expected %lld, %% 8 = %lld) | rc=%d "
         "differing %lld of %zu rerun %lld guards %s | data: sum|terms| <= %lld%s\n",
         fail ? "FAIL" : "ok  ", id, bfr::mode_name(mode), N, H, W, c.Hs, c.Ws, xcd, M, li.blocks, expect, expect % 8, rc, d.count,
         ref.size(), rerun, guards ? "ok" : "OVERWRITTEN", cond.max_sabs, data_ok ? "" : " (>= 2^24)");
  print_first_f32("y", d, c.Hs * c.Ws, c.Ws, 64);
  fflush(stdout);
  for (void* q : {(void*)dx, (void*)dw, (void*)db, dz}) hipFree(q);
  ++f32_cases, f32_failures += fail;
  return fail;
}

// a call the launcher must refuse on the host: EOSV_ERR_UNSUPPORTED, and the poisoned output untouched
template <class Call>
static int f32_refuse(const char* id, const Fenced& out, Call call) {
  out.poison();
  const int rc = call();
  sync_or_die(id);
  std::vector<unsigned char> y(out.n);
  const bool guards = out.fetch(y.data());
  long long touched = 0;
  for (unsigned char b : y) touched += b != 0xff;
  const bool fail = rc != EOSV_ERR_UNSUPPORTED || touched || !guards;
  printf("%s f32 %s rc=%d (expected %d) output bytes touched %lld guards %s\n", fail ? "FAIL" : "ok  ", id, rc,
         (int)EOSV_ERR_UNSUPPORTED, touched, guards ? "ok" : "OVERWRITTEN");
  fflush(stdout);
  ++f32_cases, f32_failures += fail;
  return fail;
}

static int run_f32(const char* group) {
  using namespace bfr;
  bool known = false;
  auto is = [&](const char* g) {
    const bool m = !strcmp(group, g);
    known |= m;
    return m;
  };
  const int cu = device_cu_count();
  const int kMain[2] = {kInt, kWideX}, kSide[2] = {kRound, kWideW};  // every shape / one shape per group
  const int MAP = 27 * 29;  // the large-grid cases' map: 783 pixels, so that M has a tail at every tile
  auto images = [&](long long pixels) { return (int)((pixels + MAP - 1) / MAP); };  // of 27 x 29, to reach M >= pixels
  if (is("rows")) {
    // conv_rows_f32_kernel <RW, RES> (64 -> 64, 3x3, W 56 / 64, strips of 2 rows) through launch_conv_f32
    const int trips = 2 * cu + 3;  // strips: every workgroup takes a second, some a third; both buffers refilled
    for (int mode : kMain) {
      f32_conv("rows.56.one", kFRows, mode, 1, 2, 56, 64, 64, 3, 1, 1, 0, 0, true, true, 0);  // one strip, both borders
      for (int res = 0; res < 2; ++res)
        for (int relu = 0; relu < 2; ++relu)
          f32_conv("rows.56.mid", kFRows, mode, 3, 6, 56, 64, 64, 3, 1, 1, 0, 0, res, relu, 0);  // 9 strips, interior ones
      f32_conv("rows.56.trips", kFRows, mode, trips, 2, 56, 64, 64, 3, 1, 1, 0, 0, true, true, 0);
      f32_conv("rows.56.trips", kFRows, mode, trips, 2, 56, 64, 64, 3, 1, 1, 0, 0, false, true, 0);
      f32_conv("rows.64.one", kFRows, mode, 1, 2, 64, 64, 64, 3, 1, 1, 0, 0, false, true, 0);
      for (int relu = 0; relu < 2; ++relu) f32_conv("rows.64.mid", kFRows, mode, 2, 6, 64, 64, 64, 3, 1, 1, 0, 0, false, relu, 0);
      f32_conv("rows.64.trips", kFRows, mode, cu + 3, 2, 64, 64, 64, 3, 1, 1, 0, 0, false, true, 0);
      // W 64 with a residual exceeds the row kernel's LDS: the 256x64 tile (5 tiles, an M tail)
      for (int xcd = 0; xcd < 2; ++xcd)
        f32_conv("rows.64.res->dma", kFD256x64, mode, 3, 6, 64, 64, 64, 3, 1, 1, 0, 0, true, true, 0, xcd);
    }
    for (int mode : kSide) {
      f32_conv("rows.56.mid", kFRows, mode, 3, 6, 56, 64, 64, 3, 1, 1, 0, 0, true, true, 0);
      f32_conv("rows.64.mid", kFRows, mode, 2, 6, 64, 64, 64, 3, 1, 1, 0, 0, false, true, 0);
    }
  }
  if (is("c64")) {
    // launch_dma<256, 64, 16, 4, 1>: Cout <= 64
    for (int mode : kMain) {
      f32_conv("c64.1x1.below", kFD256x64, mode, 2, 9, 11, 64, 64, 1, 1, 0, 0, 0, false, false, 0);  // M 198: below one tile
      for (int xcd = 0; xcd < 2; ++xcd)
        f32_conv("c64.3x3.ragged", kFD256x64, mode, 3, 9, 11, 64, 64, 3, 1, 1, 0, 0, true, true, 0, xcd);  // M 297: 2 tiles
      f32_conv("c64.3x3.kcm32", kFD256x64, mode, 3, 9, 11, 64, 64, 3, 1, 1, 0, 0, true, false, 32);
      f32_conv("c64.3x3.kcm64", kFD256x64, mode, 3, 9, 11, 64, 64, 3, 1, 1, 0, 0, false, true, 64);
      f32_conv("c64.1x1.cout32", kFD256x64, mode, 5, 9, 11, 64, 32, 1, 1, 0, 0, 0, true, true, 0);  // half an n-tile
      f32_conv("c64.3x3.cin32.cout32", kFD256x64, mode, 3, 9, 11, 32, 32, 3, 1, 1, 0, 0, false, true, 0);
      f32_conv("c64.3x3.cin32.kcm32", kFD256x64, mode, 3, 9, 11, 32, 64, 3, 1, 1, 0, 0, true, true, 32);  // one chunk
      f32_conv("c64.3x3s2", kFD256x64, mode, 3, 13, 11, 32, 64, 3, 2, 1, 0, 0, false, true, 0);
      for (int xcd = 0; xcd < 2; ++xcd)
        f32_conv("c64.1x1.18tiles", kFD256x64, mode, 45, 9, 11, 64, 64, 1, 1, 0, 0, 0, true, true, 0, xcd);  // M 4455: 18 tiles
    }
    for (int mode : kSide) f32_conv("c64.3x3.ragged", kFD256x64, mode, 3, 9, 11, 64, 64, 3, 1, 1, 0, 0, true, true, 0);
  }
  if (is("t64")) {
    // launch_dma<128, 64, 16, 2, 2> (Cout >= 128, grids below the CU count), plain and DS
    for (int mode : kMain) {
      f32_conv("t64.3x3", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 0, 0, true, true, 0);
      f32_conv("t64.3x3.kcm32", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 0, 0, true, false, 32);
      for (int xcd = 0; xcd < 2; ++xcd) f32_conv("t64.3x3.kcm64", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 0, 0, false, true, 64, xcd);
      f32_conv("t64.3x3s2", kFD128x64, mode, 3, 13, 11, 64, 128, 3, 2, 1, 0, 0, false, true, 0);
      f32_conv("t64.3x3s2.kcm64", kFD128x64, mode, 3, 13, 11, 64, 128, 3, 2, 1, 0, 0, false, true, 64);
      f32_conv("t64.1x1s2.64->128", kFD128x64, mode, 3, 7, 5, 64, 128, 1, 2, 0, 0, 0, false, false, 0);
      f32_conv("t64.1x1s2.128->256", kFD128x64, mode, 3, 7, 5, 128, 256, 1, 2, 0, 0, 0, false, false, 64);
      for (int xcd = 0; xcd < 2; ++xcd) f32_conv("t64.cout96", kFD128x64, mode, 2, 9, 11, 32, 96, 3, 1, 1, 0, 0, true, true, 0, xcd);
      // fused downsample (DS = true) at the three forms the networks run, each with an M tail
      f32_conv("t64.ds.3x3+s2", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 64, 2, false, true, 0);
      f32_conv("t64.ds.3x3+s2.kcm64", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 64, 2, false, true, 64);
      f32_conv("t64.ds.1x1.64->256+s1", kFD128x64, mode, 3, 9, 11, 64, 256, 1, 1, 0, 64, 1, false, true, 0);
      f32_conv("t64.ds.1x1.128->512+s2", kFD128x64, mode, 3, 7, 5, 128, 512, 1, 1, 0, 256, 2, false, true, 64);
    }
    for (int mode : kSide) f32_conv("t64.ds.3x3+s2", kFD128x64, mode, 2, 9, 11, 128, 128, 3, 1, 1, 64, 2, false, true, 0);
  }
  // launch_ws<256, 128, 4, 2, 2>: Cout <= 256 and a 256x128 grid of at least the CU count
  const int n128 = images((cu - 1) * 256LL + 1), n256 = images((cu / 2 - 1) * 256LL + 1);
  if (is("ws256")) {
    for (int mode : kMain) {
      for (int xcd = 0; xcd < 2; ++xcd) f32_conv("ws256.3x3.cout128", kFW256, mode, n128, 27, 29, 32, 128, 3, 1, 1, 0, 0, true, true, 0, xcd);
      f32_conv("ws256.3x3.cout128.kcm32", kFW256, mode, n128, 27, 29, 32, 128, 3, 1, 1, 0, 0, false, false, 32);
      f32_conv("ws256.1x1.cout256", kFW256, mode, n256, 27, 29, 64, 256, 1, 1, 0, 0, 0, true, true, 0);
      f32_conv("ws256.ds.1x1.64->256+s1", kFW256, mode, n256, 27, 29, 64, 256, 1, 1, 0, 64, 1, false, true, 0);
      f32_conv("ws256.ds.1x1.64->128+s2", kFW256, mode, n128, 27, 29, 64, 128, 1, 1, 0, 32, 2, false, true, 0);
    }
    for (int mode : kSide) f32_conv("ws256.ds.1x1.64->256+s1", kFW256, mode, n256, 27, 29, 64, 256, 1, 1, 0, 64, 1, false, true, 0);
  }
  if (is("ws256k")) {
    // long K (72 k-steps: the A ring turns over 24 times), chunk-major, and a 3x3 with the fused downsample
    for (int mode : kMain) f32_conv("ws256k.3x3.cin128.kcm64", kFW256, mode, n128, 27, 29, 128, 128, 3, 1, 1, 0, 0, true, true, 64);
    f32_conv("ws256k.ds.3x3+s2", kFW256, kInt, n128, 27, 29, 32, 128, 3, 1, 1, 32, 2, false, true, 0);
    f32_conv("ws256k.ds.3x3+s2", kFW256, kWideX, n128, 27, 29, 32, 128, 3, 1, 1, 32, 2, false, true, 0);
    f32_conv("ws256k.ds.3x3+s2", kFW256, kWideW, n128, 27, 29, 32, 128, 3, 1, 1, 32, 2, false, true, 0);
    f32_conv("ws256k.ds.3x3+s2", kFW256, kRound, n128, 27, 29, 32, 128, 3, 1, 1, 32, 2, false, true, 0);
  }
  if (is("ws128")) {
    // launch_ws<128, 128, 2, 2, 2>: a 128x128 grid of at least the CU count where 256x128 is not taken
    const int n512 = images((cu / 4 - 1) * 128LL + 1), n2048 = images((cu / 16 - 1) * 128LL + 1);
    const int n256b = images((cu / 2 - 1) * 128LL + 1);  // Cout 256: 256x128 grid below the CU count, 128x128 grid not
    for (int mode : kMain) {
      for (int xcd = 0; xcd < 2; ++xcd) f32_conv("ws128.1x1.cout512", kFW128, mode, n512, 27, 29, 32, 512, 1, 1, 0, 0, 0, true, true, 0, xcd);
      f32_conv("ws128.1x1.cout2048", kFW128, mode, n2048, 27, 29, 64, 2048, 1, 1, 0, 0, 0, true, true, 0);
      f32_conv("ws128.1x1.cout256", kFW128, mode, n256b, 27, 29, 32, 256, 1, 1, 0, 0, 0, false, true, 0);
      f32_conv("ws128.3x3.cout512.kcm32", kFW128, mode, n512, 27, 29, 32, 512, 3, 1, 1, 0, 0, false, false, 32);
      f32_conv("ws128.ds.1x1.128->512+s2", kFW128, mode, n512, 27, 29, 128, 512, 1, 1, 0, 256, 2, false, true, 64);
      f32_conv("ws128.ds.3x3+s2", kFW128, mode, n512, 27, 29, 32, 512, 3, 1, 1, 32, 2, false, true, 0);
    }
    for (int mode : kSide) f32_conv("ws128.ds.1x1.128->512+s2", kFW128, mode, n512, 27, 29, 128, 512, 1, 1, 0, 256, 2, false, true, 64);
  }
  if (is("ksplit")) {
    // the training entry's split-K (ConvArgs::kws) on the two large launch_dma tiles, which
    // tests/test_gpu_train_convs.py reaches only unsplit (its split cases are M 35 on the 128x64 tile): K 1152
    // = 72 k-steps in 2 slices, the second starting mid-tap (tap-major: tap 4, channel 64) or mid-chunk
    const int n512 = images((cu / 4 - 1) * 128LL + 1);
    for (int mode : kMain) {
      f32_conv("ksplit.256x128", kFK256, mode, n128, 27, 29, 128, 128, 3, 1, 1, 0, 0, true, true, 0, 1, 2);
      f32_conv("ksplit.256x128.kcm64", kFK256, mode, n128, 27, 29, 128, 128, 3, 1, 1, 0, 0, false, false, 64, 1, 2);
      f32_conv("ksplit.128x128", kFK128, mode, n512, 27, 29, 128, 512, 3, 1, 1, 0, 0, true, true, 0, 1, 2);
      f32_conv("ksplit.128x128.kcm32", kFK128, mode, n512, 27, 29, 128, 512, 3, 1, 1, 0, 0, false, true, 32, 1, 2);
    }
    for (int mode : kSide) f32_conv("ksplit.128x128", kFK128, mode, n512, 27, 29, 128, 512, 3, 1, 1, 0, 0, true, true, 0, 1, 2);
  }
  if (is("head")) {
    // Cout % 4 != 0 (the fc head): launch_dma<128, 64, ..., EPI = false>, the per-element epilogue
    for (int mode : kMain)
      for (int cout : {5, 50, 101})
        for (int m : {1, 37}) {
          f32_conv("head.fc", kFHead, mode, m, 1, 1, 512, cout, 1, 1, 0, 0, 0, false, false, 0);
          f32_conv("head.fc", kFHead, mode, m, 1, 1, 512, cout, 1, 1, 0, 0, 0, true, true, 0, 0);
        }
    for (int mode : kSide) f32_conv("head.fc", kFHead, mode, 37, 1, 1, 512, 101, 1, 1, 0, 0, 0, true, true, 0);
    // the unfused stem on frames the fused kernel refuses (below 8 rows / columns, more than 128 stem
    // columns) and on an odd size
    for (int mode : kMain) {
      f32_stem_conv("head.stem.6x20", mode, 3, 6, 20);
      f32_stem_conv("head.stem.20x7", mode, 2, 20, 7);
      for (int xcd = 0; xcd < 2; ++xcd) f32_stem_conv("head.stem.10x260", mode, 2, 10, 260, xcd);  // M 1300: 11 tiles
      f32_stem_conv("head.stem.37x33", mode, 3, 37, 33);
    }
    for (int mode : kSide) f32_stem_conv("head.stem.37x33", mode, 3, 37, 33);
  }
  if (is("stem")) {
    // launch_stem_pool_f32, every NT 1..8 (stem widths 8, 24, 43, 44, 56, 72, 90, 100, 128) x pack /
    // direct x plain / split; odd H and W, pooled heights below 8
    // 4/3 of the slots the launcher counts for 24 x 16 frames (pooled 6 x 4): two rounds of whole images
    // cost 24 stem rows, three rounds of half images 21, so whatever the occupancy the plan has >= 2 bands
    LaunchInfo pi{-1, -1};
    launch_stem_pool_f32(nullptr, 1, 24, 16, nullptr, nullptr, nullptr, 0, false, &pi);  // records, launches nothing
    const int nbands = pi.slots >= cu ? (int)(pi.slots + pi.slots / 3) : 1;
    for (int mode : kMain) {
      f32_stem("stem.8x8", mode, 3, 8, 8);         // the smallest frame: stem 4x4, pooled 2x2
      f32_stem("stem.nt1", mode, 2, 22, 16);       // Ws 8
      f32_stem("stem.nt2", mode, 2, 18, 48);       // Ws 24, pooled height 5
      f32_stem("stem.nt3.odd", mode, 2, 37, 85);   // Ws 43: odd H and W, pack only
      f32_stem("stem.nt3", mode, 2, 26, 88);       // Ws 44
      f32_stem("stem.nt4", mode, 2, 30, 112);      // Ws 56
      f32_stem("stem.nt5", mode, 2, 20, 144);      // Ws 72
      f32_stem("stem.nt6", mode, 2, 17, 180);      // Ws 90, odd H
      f32_stem("stem.nt7", mode, 2, 36, 200);      // Ws 100: a partial last column tile
      f32_stem("stem.nt8", mode, 2, 24, 256);      // Ws 128
      f32_stem("stem.bands", mode, nbands, 24, 16, true);  // more images than slots
    }
    for (int mode : kSide) f32_stem("stem.nt3", mode, 2, 26, 88);
  }
  if (is("refuse")) {
    // every refusal of the three launchers: the status, and nothing written
    const ConvCase c = make_conv(2, 4, 4, 96, 64, 1, 1, 0, 0, 0, kInt);
    float *dx = upload(to_f32(c.x)), *dw = upload(to_f32(c.w)), *db = upload(to_f32(c.bias));
    void* dz;
    hipMalloc(&dz, 256);
    hipMemset(dz, 0, 256);
    Fenced out(2 * 16 * 128 * 4);
    ConvArgs a{};  // a 1x1 96 -> 64 on 2 x 4 x 4 that launch_conv_f32 accepts
    a.x = dx; a.w = dw; a.bias = db; a.y = out.p();
    a.N = 2; a.H = a.W = a.Ho = a.Wo = 4; a.Cin = 96; a.Cout = 64; a.KH = a.KW = a.KWp = 1; a.stride = 1; a.K = 96; a.zero = dz; a.xcd = 1;
    auto conv = [&](const char* id, ConvArgs b) { f32_refuse(id, out, [&] { return launch_conv_f32(b, 0); }); };
    ConvArgs b = a;
    b.zero = nullptr;
    conv("refuse.conv.no_zero", b);
    b = a, b.K = 80;
    conv("refuse.conv.K%32", b);
    b = a, b.Cin = 48, b.KW = b.KWp = 2, b.K = 96;
    conv("refuse.conv.Cin%32", b);
    b = a, b.kcm = 48;
    conv("refuse.conv.kcm.not_pow2", b);
    b = a, b.kcm = 16;
    conv("refuse.conv.kcm.below32", b);
    b = a, b.kcm = 64;
    conv("refuse.conv.kcm.not_dividing", b);
    b = a, b.Cin = 3, b.KH = b.KW = 7, b.KWp = 7, b.K = 176;
    conv("refuse.conv.stem_layout", b);
    // fused downsample: x2 = x read as 32 + 64 channels would be K1 32, Cin2 64
    b = a, b.x2 = dx, b.H2 = b.W2 = 4, b.stride2 = 1, b.Cin = 32, b.K1 = 32, b.Cin2 = 64, b.Cout = 6;
    conv("refuse.conv.x2.Cout%4", b);
    b.Cout = 64, b.K1 = 40, b.Cin2 = 56;
    conv("refuse.dma.x2.K1%16", b);
    b.K1 = 32, b.Cin2 = 56;
    conv("refuse.dma.x2.Cin2%16", b);
    b.Cout = 128, b.K1 = 40, b.Cin2 = 56;  // (the 128x64 tile; out holds 2 x 16 x 128 floats)
    conv("refuse.dma128.x2.K1%16", b);
    {  // the same refusal in launch_ws<256, 128>: a grid of the CU count, on buffers of the full size
      const long long M = (long long)n128 * MAP;
      float *bx = nullptr, *bw = nullptr;
      hipMalloc(&bx, M * 64 * 4), hipMalloc(&bw, 128 * 96 * 4);
      hipMemset(bx, 0, M * 64 * 4), hipMemset(bw, 0, 128 * 96 * 4);
      Fenced big((size_t)M * 128 * 4);
      b = a, b.x = bx, b.w = bw, b.bias = nullptr, b.y = big.p(), b.N = n128, b.H = b.Ho = 27, b.W = b.Wo = 29, b.Cin = 32, b.Cout = 128;
      b.x2 = bx, b.H2 = 27, b.W2 = 29, b.stride2 = 1, b.K1 = 40, b.Cin2 = 56;
      long long grid = 0;
      if (f32_dispatch(b, &grid) != kFW256) printf("FAIL f32 refuse.ws256.x2.K1%%16: the shape does not reach ws 256x128\n"), ++f32_failures;
      else f32_refuse("refuse.ws256.x2.K1%16", big, [&] { return launch_conv_f32(b, 0); });
      hipFree(bx), hipFree(bw);
    }
    b = a, b.Cin = b.Cout = 64, b.KH = b.KW = b.KWp = 3, b.pad = 1, b.K = 576, b.H = b.Ho = 2, b.W = b.Wo = 60;
    f32_refuse("refuse.rows.W60", out, [&] { return launch_conv_rows_f32(b, 0); });
    f32_refuse("refuse.stem.7x8", out, [&] { return launch_stem_pool_f32(dx, 1, 7, 8, dw, db, out.p(), 0); });
    f32_refuse("refuse.stem.8x7", out, [&] { return launch_stem_pool_f32(dx, 1, 8, 7, dw, db, out.p(), 0, true); });
    f32_refuse("refuse.stem.wide", out, [&] { return launch_stem_pool_f32(dx, 1, 8, 258, dw, db, out.p(), 0); });
    f32_refuse("refuse.stem.direct.W%4", out, [&] { return launch_stem_pool_f32(nullptr, 1, 10, 10, dw, db, out.p(), 0, false, nullptr, dx); });
    for (void* q : {(void*)dx, (void*)dw, (void*)db, dz}) hipFree(q);
  }
  if (!known) printf("FAIL f32: unknown group %s\n", group), ++f32_failures;
  printf("%lld cases\n%lld failures\n", f32_cases, f32_failures);
  return f32_failures ? 1 : 0;
}

int main(int argc, char** argv) {
  int fails = 0;
  if (argc > 2 && !strcmp(argv[1], "x3")) return run_x3(argv[2]);
  if (argc > 2 && !strcmp(argv[1], "f32")) return run_f32(argv[2]);
  if (argc > 2 && !strcmp(argv[1], "bf16")) return run_bf16(argv[2]);
  if (argc > 1 && !strcmp(argv[1], "pairw_stress")) {  // the engine's in-place pairs at C2/C3 chunk sizes
    for (int n : {64, 130, 43, 257})
      for (int c1 : {128, 256}) fails += check_pairw(n, 28, 28, 128, 512, c1, 0, true, true, 4);
    fails += check_pairw(64, 14, 14, 256, 1024, 256, 0, true, true, 4);
    fails += check_pairw(64, 28, 28, 128, 512, 128, 256, false, true, 4);
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
  }
  // R50 layer2 / layer3 wide pairs: within a stage (c1 = cmid) and into the next stage; many rounds
  // per workgroup (300 x 784 = 1838 rounds), ragged M (3 x 196 = 588: 4.6 rounds), tiny M
  fails += check_pairw(300, 28, 28, 128, 512, 128);
  fails += check_pairw(3, 28, 28, 128, 512, 256);
  fails += check_pairw(3, 14, 14, 256, 1024, 256);
  fails += check_pairw(200, 14, 14, 256, 1024, 256);
  fails += check_pairw(1, 7, 5, 128, 512, 128);
  // stage-2 block 0: conv3 + the folded stride-2 downsample (x2 = the 56x56x256 stage-1 output)
  fails += check_pairw(40, 28, 28, 128, 512, 128, 256);
  fails += check_pairw(3, 7, 5, 128, 512, 128, 256);
  // R50 layer1 pairs: block 1/2 (residual, c1 64), block 0 (downsample), layer1 -> layer2 (c1 128);
  // 700 images = 34300 tiles (~134 per workgroup), 64-wide maps (R101 @ 256)
  fails += check_pair(700, 56, 56, 64, false);
  fails += check_pair(9, 56, 56, 64, true);
  fails += check_pair(9, 56, 56, 128, false);
  fails += check_pair(5, 64, 64, 64, false);
  fails += check_pair(1, 8, 8, 64, true);  // one tile: the grid is smaller than the CU count
  fails += check_stem_pool(2, 224, 224);
  fails += check_stem_pool(3, 100, 86);  // ragged: partial last column tile, odd pooled sizes
  fails += check_stem_pool(2, 64, 48);
  fails += check_stem_pool(2, 224, 224, true);
  fails += check_stem_pool(3, 100, 86, true);
  fails += check_stem_pool(2, 64, 48, true);
  // column-blocked direct kernel (W % 4 == 0): ResNet-101's 256 x 256 (3 column blocks, the last
  // half idle), a ragged last block, a single partial block
  if (stem_pool_bf16_ok(256, 256, true)) fails += check_stem_pool(2, 256, 256, true);  // (EOSV_STEM_CB=0: unfused)
  fails += check_stem_pool(3, 100, 88, true);
  fails += check_stem_pool(2, 60, 36, true);
  fails += check_stem_pool_x3(2, 224, 224);
  fails += check_stem_pool_x3(2, 256, 256);
  fails += check_stem_pool_x3(3, 60, 36);
  fails += check_stem_pool_f32(2, 224, 224);
  fails += check_stem_pool_f32(3, 100, 86);
  fails += check_stem_pool_f32(2, 64, 48);
  fails += check_stem_pool_f32(2, 40, 200);  // Ws 100: a partial last column tile
  fails += check_stem_pool_f32(2, 256, 256);  // 8 column tiles
  // row bands (one workgroup per band of pooled rows): 8 bands at small N, 3 at 1000, 7-8 at 2400
  fails += check_stem_pool_f32(1000, 224, 224, 333);
  fails += check_stem_pool_f32(2400, 224, 224, 797);
  // stage-1 shape (row-strip kernel): 300 images = 4200 strips, several strips per workgroup
  fails += check_bf16(300, 56, 56, 64, 64, 3, 1, 1, true, true);
  fails += check_bf16(3, 56, 56, 64, 64, 3, 1, 1, false, true);
  // phased 8-wave kernel: 512x128 (Cout 128) and 256x256 tiles, strided entries, 1x1s, M tails
  fails += check_bf16(40, 28, 28, 128, 128, 3, 1, 1, true, true);
  fails += check_bf16(40, 28, 28, 128, 128, 3, 1, 1, true, true, true);
  fails += check_bf16(30, 14, 14, 256, 256, 3, 1, 1, true, true, true);
  fails += check_bf16(9, 28, 28, 128, 256, 3, 2, 1, false, true, true);
  fails += check_bf16(3, 7, 7, 512, 512, 3, 1, 1, false, true, true);
  fails += check_bf16(2, 9, 11, 128, 128, 3, 1, 1, true, false, true);
  fails += check_bf16(7, 56, 56, 64, 128, 3, 2, 1, false, true);
  // r05 register-weight row strips (conv_rowsr_bf16.hip) called directly: C 64 at 56x56, C 128 at 28x28
  g_bf16_launch = launch_conv_rowsr_bf16;
  fails += check_bf16(300, 56, 56, 64, 64, 3, 1, 1, true, true);
  fails += check_bf16(37, 56, 56, 64, 64, 3, 1, 1, false, true);
  fails += check_bf16(3, 56, 56, 64, 64, 3, 1, 1, true, false);
  fails += check_bf16(300, 28, 28, 128, 128, 3, 1, 1, true, true);
  fails += check_bf16(41, 28, 28, 128, 128, 3, 1, 1, false, true);
  fails += check_bf16(2, 28, 28, 128, 128, 3, 1, 1, true, false);
  fails += check_bf16(40, 28, 28, 128, 128, 3, 1, 1, true, true, true);   // chunk-major K weights
  fails += check_bf16(45, 64, 64, 64, 64, 3, 1, 1, true, true);
  fails += check_bf16(7, 64, 64, 64, 64, 3, 1, 1, false, true);
  fails += check_bf16(33, 32, 32, 128, 128, 3, 1, 1, true, true, true);
  fails += check_bf16(6, 32, 32, 128, 128, 3, 1, 1, false, true, true);
  g_bf16_launch = launch_conv_bf16;
  fails += check_bf16(300, 56, 56, 64, 128, 3, 2, 1, false, true);   // stride-2 entry row strips: several per workgroup
  fails += check_bf16(37, 56, 56, 64, 128, 3, 2, 1, false, false);   // ... without ReLU, ragged strip count
  fails += check_bf16(5, 56, 56, 128, 128, 3, 2, 1, false, true, true);  // R50 layer2.0.conv2 (kcm)
  fails += check_bf16(3, 13, 11, 64, 128, 3, 2, 1, false, true);         // ragged stride-2 entry, M tail
  fails += check_bf16(7, 56, 56, 64, 128, 1, 2, 0, false, false);
  fails += check_bf16(30, 14, 14, 256, 256, 3, 1, 1, true, true);
  fails += check_bf16(9, 28, 28, 128, 256, 3, 2, 1, false, true);
  fails += check_bf16(20, 7, 7, 512, 512, 3, 1, 1, true, true);
  fails += check_bf16(3, 7, 7, 512, 512, 3, 1, 1, false, true);  // M = 147 < one 256-row tile
  fails += check_bf16(5, 14, 14, 1024, 256, 1, 1, 0, false, true);
  fails += check_bf16(5, 14, 14, 256, 1024, 1, 1, 0, true, true);
  fails += check_bf16(2, 9, 11, 128, 128, 3, 1, 1, true, false);  // ragged map, M = 198
  // halo-staged stride-1 3x3s (conv_halo_bf16, kcm weights, Cout % 256 == 0): 16x16 / 8x8 maps
  // (256x256 input), a ragged map with an M tail, Cout 512 (two cout tiles)
  fails += check_bf16(7, 16, 16, 256, 256, 3, 1, 1, true, true, true);
  fails += check_bf16(5, 8, 8, 512, 512, 3, 1, 1, false, true, true);
  fails += check_bf16(3, 10, 12, 128, 256, 3, 1, 1, true, false, true);
  fails += check_bf16(11, 7, 7, 256, 512, 3, 1, 1, true, true, true);
  fails += check(1, 8, 8, 32, 64, 1, 1, 0, false, false, false);
  fails += check(2, 9, 7, 64, 64, 3, 1, 1, false, false, false);
  fails += check(2, 14, 14, 64, 128, 3, 2, 1, false, true, true);
  fails += check(3, 7, 7, 256, 512, 1, 2, 0, false, false, false);
  fails += check(1, 7, 7, 512, 512, 3, 1, 1, false, true, true);
  fails += check(2, 30, 30, 3, 64, 7, 2, 3, true, false, true);
  fails += check(3, 37, 33, 3, 64, 7, 2, 3, true, false, true);  // odd sizes: row-width rounding, M tail
  fails += check(5, 1, 1, 512, 64, 1, 1, 0, false, false, false);
  // f32 stride-1 3x3 convs at the stage shapes of R18/R50, the fused downsample (K columns
  // [K1, K) from x2), ragged maps and M tails; exact-f32 products, so a tight bound
  fails += check(12, 56, 56, 64, 64, 3, 1, 1, false, true, true, 0, 2e-6);
  // f32 stage-1 row-strip kernel (conv_rows_f32.hip): 560 strips (2-3 per workgroup), R50's
  // residual-free conv, 64-wide maps (256x256 input), no ReLU
  fails += check(20, 56, 56, 64, 64, 3, 1, 1, false, true, true, 0, 2e-6);
  fails += check(3, 56, 56, 64, 64, 3, 1, 1, false, false, true, 0, 2e-6);
  fails += check(4, 64, 64, 64, 64, 3, 1, 1, false, true, true, 0, 2e-6);
  fails += check(2, 64, 64, 64, 64, 3, 1, 1, false, false, false, 0, 2e-6);
  fails += check(5, 28, 28, 128, 128, 3, 1, 1, false, false, true, 64, 2e-6);
  fails += check(6, 14, 14, 256, 256, 3, 1, 1, false, true, true, 0, 2e-6);
  fails += check(4, 14, 14, 256, 256, 3, 1, 1, false, false, true, 128, 2e-6);
  fails += check(3, 7, 7, 512, 512, 3, 1, 1, false, false, true, 256, 2e-6);
  // chunk-major K order (r04, the library's f32 weights at Cin >= 128): the R18 / R50 stage-2..4
  // 3x3s at grids that take every tile (256x128, 128x128, 128x64), stride 2, the fused downsample
  fails += check(50, 28, 28, 128, 128, 3, 1, 1, false, true, true, 0, 2e-6, true);
  fails += check(40, 28, 28, 128, 128, 3, 1, 1, false, false, true, 64, 2e-6, true);
  fails += check(60, 14, 14, 256, 256, 3, 1, 1, false, true, true, 0, 2e-6, true);
  fails += check(30, 28, 28, 128, 256, 3, 2, 1, false, false, true, 0, 2e-6, true);
  fails += check(40, 7, 7, 512, 512, 3, 1, 1, false, true, true, 0, 2e-6, true);
  fails += check(4, 14, 14, 256, 256, 3, 1, 1, false, false, true, 128, 2e-6, true);
  fails += check(3, 9, 11, 160, 96, 3, 1, 1, false, true, false, 0, 2e-6, true);
  // grids at / above the CU count: the large 256x128 and 128x128 tiles (small N takes 128x64)
  fails += check(21, 56, 56, 32, 128, 3, 1, 1, false, true, true, 0, 2e-6);
  fails += check(11, 28, 28, 32, 512, 1, 1, 0, false, false, true, 0, 2e-6);
  fails += check(3, 9, 11, 32, 64, 3, 1, 1, false, true, false, 0, 2e-6);
  fails += check(2, 5, 3, 32, 128, 3, 1, 1, false, true, true, 32, 2e-6);
  printf("%d failures\n", fails);
  return fails;
}
