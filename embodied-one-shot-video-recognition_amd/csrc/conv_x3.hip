// f32x3 implicit GEMMs of the training step's KxK and strided convs (opt-in:
// NativeTrainer(f32x3_convs=...)): the arithmetic of gemm_x3.hip (f32 operands in memory, split into
// hi + lo bf16 on the way into LDS, lo*hi, hi*lo, hi*hi per 32-k step on bf16 MFMA, f32 accumulation,
// k strictly increasing within a slice, no atomics) with an operand gathered by filter tap instead
// of read as a matrix.  X is NHWC [N][H][W][Cin], W [Cout][KH][KW][Cin], Y / dY [P][Cout] with
// P = N Ho Wo (model(video) in train mode and loss.backward(), reference network_train.py:98-116):
//   * forward / stride-1 input gradient   Y[P][Cout] = col(X)[P][K] . W[Cout][K]^T + addend   (NT)
//   * weight gradient                     dW[Cout][K] = dY[P][Cout]^T . col(X)[P][K]           (TN, split over P)
// K = KH KW Cin in (kh, kw, c) order, as W lies in memory; col(X) is never stored.  Cin % 32 == 0, so
// a 32-k step lies in one tap: the NT kernel's A rows are pixels, decoded to (n, oh, ow) once per
// thread, and a step reads 32 channels of each row's tap pixel, or holds zeros (no load) where the
// tap falls outside the image.  The TN kernel's B columns are 4 consecutive (tap, c) of one tap per
// thread, decoded once; its reduction index is the pixel, walked as (n, oh, ow) without a division.
// Frames are kept apart by n: a pixel of frame n never reads frame n +- 1.
//
// Both kernels run X3Tile::k_loop (x3_tile.h) over two sets of the four LDS images and state only how a
// step's operands are fetched.
#include "x3_tile.h"

namespace eosv {

namespace {
struct ConvX3Args {
  const float* x;    // [N][H][W][Cin]
  const float* w;    // NT: [Cout][K]
  const float* dy;   // TN: [P][Cout]
  const float* add;  // NT: [P][Cout] addend or nullptr
  float* out;        // NT: Y; TN: dW, or the [slices][Cout][K] partials when partial
  long long P;       // output pixels
  int H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
  int K;    // KH KW Cin
  int nt;   // tiles along n
  // TN
  int kps;               // pixels per slice (a multiple of XB_K unless one slice)
  int partial;           // 1: raw partial sums to out[slice][Cout][K]
  int s_ow, s_oh, s_n;   // 32 pixels on, as (n, oh, ow) steps before the carries
  double* stats;         // NT, STATS: [row tiles][2][Cout] column sums and sums of squares of Y per row tile
};

// STATS (eosv_conv2d_x3_stats: no addend): the tile's BN batch statistics besides Y (x3_tile_stats)
template <int WM, int WN, bool STATS = false>
__global__ __launch_bounds__(XB_NT) void conv_x3_kernel(ConvX3Args g) {
  using Tile = X3Tile<WM, WN>;
  constexpr int NP = Tile::BM / 32;   // rows of A a thread stages
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * Tile::IMG];
  const Tile t;
  const int tid = t.tid;
  const int tn = blockIdx.x % g.nt, tm = blockIdx.x / g.nt;
  const long long m0 = (long long)tm * t.BM, n0 = (long long)tn * t.BN;

  Stage<Tile::BM, false> sa;
  Stage<Tile::BN, false> sb;

  // this thread's rows: the top-left input pixel of each and its frame's first pixel; a row past P
  // lies outside the image at every tap
  int ih0[NP], iw0[NP];
  long long frame[NP];
  const long long how = (long long)g.Ho * g.Wo;
#pragma unroll
  for (int s = 0; s < NP; ++s) {
    const long long p = m0 + ((tid + s * XB_NT) >> 3);
    ih0[s] = -0x40000000, iw0[s] = 0, frame[s] = 0;
    if (p < g.P) {
      const long long n = p / how;
      const int rem = (int)(p - n * how), oh = rem / g.Wo, ow = rem - oh * g.Wo;
      ih0[s] = oh * g.stride - g.pad;
      iw0[s] = ow * g.stride - g.pad;
      frame[s] = n * g.H * g.W;
    }
  }
  int kh = 0, kw = 0, c0 = 0;   // the step's tap and first channel: uniform
  auto gather = [&] {
#pragma unroll
    for (int s = 0; s < NP; ++s) {
      const int ih = ih0[s] + kh, iw = iw0[s] + kw;
      sa.v[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
        sa.v[s] = *(const f32x4*)(g.x + (frame[s] + (long long)ih * g.W + iw) * g.Cin + c0 + 4 * (tid & 7));
    }
  };

  typename Tile::Acc acc;
  t.zero(acc);
  const int steps = g.K / XB_K;
  // every entry that launches this kernel refuses Cin <= 0 (conv_x3_shape) and Cin % 32 != 0
  // (conv_x3_refusal) on the host: K >= 32, and the prologue needs no test
  __builtin_assume(steps > 0);
  t.k_loop(lds, steps, sa, sb, acc, [&](int step) {
    if (step) {   // one step on: the next 32 channels, or the next tap
      c0 += XB_K;
      if (c0 == g.Cin) {
        c0 = 0;
        if (++kw == g.KW) kw = 0, ++kh;
      }
    }
    gather();
    sb.load(g.w, g.K, n0, g.Cout, (long long)step * XB_K, g.K, tid);
  });

  t.each(acc, m0, g.P, n0, g.Cout, [&](long long m, long long n, f32x4 v) {
    if (g.add) v += *(const f32x4*)(g.add + m * g.Cout + n);
    *(f32x4*)(g.out + m * g.Cout + n) = v;
  });
  if constexpr (STATS) x3_tile_stats(t, acc, m0, g.P, n0, g.Cout, tm, lds, g.stats);
}

template <int WM, int WN>
__global__ __launch_bounds__(XB_NT) void conv_wgrad_x3_kernel(ConvX3Args g) {
  using Tile = X3Tile<WM, WN>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * Tile::IMG];
  const Tile t;
  const int tid = t.tid;
  const int tn = blockIdx.x % g.nt, tm = blockIdx.x / g.nt;
  const long long m0 = (long long)tm * t.BM, n0 = (long long)tn * t.BN;   // rows: Cout, columns: K
  const long long k0 = (long long)blockIdx.y * g.kps;
  const long long k1 = min(g.P, k0 + g.kps);
  const int steps = (int)((k1 - k0 + XB_K - 1) / XB_K);   // 0: a slice past P

  Stage<Tile::BM, true> sa;
  Stage<Tile::BN, true> sb;

  // a thread stages 4 pixels (k group kg) x 4 rows of dY and x 4 columns of col(X) (row group rg)
  const int kg = tid & 7, rg = tid >> 3;
  const bool a_on = rg < t.BM / 4 && m0 + 4 * rg < g.Cout;
  const long long col = n0 + 4 * rg;
  const bool b_on = rg < t.BN / 4 && col < g.K;
  // the 4 columns are 4 channels of one tap
  const int tap = (int)(col / g.Cin), ci = (int)(col - (long long)tap * g.Cin);
  const int dh = tap / g.KW - g.pad, dw = tap % g.KW - g.pad;
  // (n, oh, ow) of the first of the 4 pixels, 32 pixels on per step
  long long pix = k0 + 4 * kg;
  const long long how = (long long)g.Ho * g.Wo;
  long long n = pix / how;
  int oh = (int)(pix - n * how) / g.Wo, ow = (int)(pix - n * how) - oh * g.Wo;
  auto gather = [&] {
    long long nn = n;
    int h = oh, w = ow;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool live = pix + t < k1;
      const int ih = h * g.stride + dh, iw = w * g.stride + dw;
      sa.v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      sb.v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a_on && live) sa.v[t] = *(const f32x4*)(g.dy + (pix + t) * g.Cout + m0 + 4 * rg);
      if (b_on && live && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
        sb.v[t] = *(const f32x4*)(g.x + ((nn * g.H + ih) * g.W + iw) * g.Cin + ci);
      if (++w == g.Wo) {
        w = 0;
        if (++h == g.Ho) h = 0, ++nn;
      }
    }
  };
  auto advance = [&] {   // s_ow < Wo and s_oh < Ho: one carry each
    pix += XB_K;
    ow += g.s_ow;
    const int cw = ow >= g.Wo;
    ow -= cw ? g.Wo : 0;
    oh += g.s_oh + cw;
    const int ch = oh >= g.Ho;
    oh -= ch ? g.Ho : 0;
    n += g.s_n + ch;
  };

  typename Tile::Acc acc;
  t.zero(acc);
  t.k_loop(lds, steps, sa, sb, acc, [&](int step) {
    if (step) advance();
    gather();
  });

  float* out = g.partial ? g.out + (long long)blockIdx.y * g.Cout * g.K : g.out;
  t.each(acc, m0, g.Cout, n0, g.K, [&](long long m, long long nn, f32x4 v) { *(f32x4*)(out + m * g.K + nn) = v; });
}

// What the kernels do not take, naming the operand, then the first of `ops` that is off 16 bytes;
// empty: taken
std::string conv_x3_refusal(int H, int W, int Cin, int Cout, int pad, const ConvX3Shape& g, bool wgrad,
                            std::initializer_list<std::pair<const char*, const void*>> ops = {}) {
  if (Cin % 32) return "Cin = " + std::to_string(Cin) + " is not a multiple of 32";
  if (Cout % 64) return "Cout = " + std::to_string(Cout) + " is not a multiple of 64";
  const long long tiles = (((wgrad ? g.K : g.P) + 63) / 64) * (Cout / 64);
  if (g.K > 0x7fffffffLL || (long long)H + 2LL * pad > 0x3fffffffLL || (long long)W + 2LL * pad > 0x3fffffffLL ||
      (long long)g.Ho * g.Wo > 0x7fffffffLL || tiles > 0x7fffffffLL)
    return "a grid too large";
  if (const char* op = x3_misaligned(ops)) return std::string(op) + " is off 16 bytes";
  return "";
}

ConvX3Args conv_x3_args(const float* x, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                        const ConvX3Shape& sh, const X3Plan& p) {
  ConvX3Args g{};
  g.x = x, g.P = sh.P;
  g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.KH = KH, g.KW = KW, g.stride = stride, g.pad = pad;
  g.Ho = sh.Ho, g.Wo = sh.Wo, g.K = (int)sh.K, g.nt = p.nt;
  return g;
}

}  // namespace

}  // namespace eosv

using namespace eosv;

extern "C" {

int eosv_conv2d_x3(const float* d_x, int N, int H, int W, int Cin, const float* d_w, int Cout, int KH, int KW,
                   int stride, int pad, const float* d_add, float* d_y, eosv_stream_t stream) {
  ConvX3Shape sh{};
  if (!d_x || !d_w || !d_y || !conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh))
    return set_error("eosv_conv2d_x3: bad argument"), EOSV_ERR_ARG;
  if (N == 0) return EOSV_OK;
  const std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, false,
                                          {{"d_x", d_x}, {"d_w", d_w}, {"d_add", d_add}, {"d_y", d_y}});
  if (!why.empty()) return set_error("eosv_conv2d_x3: " + why), EOSV_ERR_UNSUPPORTED;
  const X3Plan p = x3_plan(sh.P, Cout, sh.K, false, 1);
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.w = d_w, g.add = d_add, g.out = d_y;
  const dim3 grid((unsigned)(p.mt * p.nt));
  x3_dispatch(p, [&](auto wm, auto wn) {
    hipLaunchKernelGGL((conv_x3_kernel<wm(), wn()>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g);
  });
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

int eosv_conv2d_x3_stats_chunks(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
  ConvX3Shape sh{};
  if (!conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh) || sh.P == 0 ||
      !conv_x3_refusal(H, W, Cin, Cout, pad, sh, false).empty())
    return 0;
  return x3_plan(sh.P, Cout, sh.K, false, 1).mt;
}

int eosv_conv2d_x3_stats(const float* d_x, int N, int H, int W, int Cin, const float* d_w, int Cout, int KH, int KW,
                         int stride, int pad, float* d_y, double* d_stats, int64_t stats_bytes,
                         eosv_stream_t stream) {
  ConvX3Shape sh{};
  if (!d_x || !d_w || !d_y || !d_stats || !conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh))
    return set_error("eosv_conv2d_x3_stats: bad argument"), EOSV_ERR_ARG;
  if (N == 0) return EOSV_OK;
  const X3Plan p = x3_plan(sh.P, Cout, sh.K, false, 1);
  if (stats_bytes < (int64_t)p.mt * 2 * Cout * (int64_t)sizeof(double))
    return set_error("eosv_conv2d_x3_stats: d_stats smaller than [row tiles][2][Cout] doubles"), EOSV_ERR_ARG;
  const std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, false,
                                          {{"d_x", d_x}, {"d_w", d_w}, {"d_y", d_y}, {"d_stats", d_stats}});
  if (!why.empty()) return set_error("eosv_conv2d_x3_stats: " + why), EOSV_ERR_UNSUPPORTED;
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.w = d_w, g.out = d_y, g.stats = d_stats;
  const dim3 grid((unsigned)(p.mt * p.nt));
  x3_dispatch(p, [&](auto wm, auto wn) {
    hipLaunchKernelGGL((conv_x3_kernel<wm(), wn(), true>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g);
  });
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

int64_t eosv_conv_wgrad_x3_workspace(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
  ConvX3Shape sh{};
  if (!conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh) || sh.P == 0 ||
      !conv_x3_refusal(H, W, Cin, Cout, pad, sh, true).empty())
    return 0;
  const X3Plan p = x3_plan(Cout, sh.K, sh.P, true, 1024);
  return p.cap > 1 ? (int64_t)p.cap * Cout * sh.K * (int64_t)sizeof(float) : 0;
}

int eosv_conv_wgrad_x3(const float* d_x, int N, int H, int W, int Cin, const float* d_dy, int Cout, int KH, int KW,
                       int stride, int pad, float* d_dw, float* d_work, int64_t work_bytes, eosv_stream_t stream) {
  ConvX3Shape sh{};
  if (!d_x || !d_dy || !d_dw || work_bytes < 0 || (!d_work && work_bytes > 0) ||
      !conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh))
    return set_error("eosv_conv_wgrad_x3: bad argument"), EOSV_ERR_ARG;
  if (N == 0) return EOSV_OK;
  const int room = x3_split_room(d_work, work_bytes, eosv_conv_wgrad_x3_workspace(N, H, W, Cin, Cout, KH, KW, stride, pad),
                                 (int64_t)Cout * sh.K * (int64_t)sizeof(float));
  if (!room) return set_error("eosv_conv_wgrad_x3: workspace smaller than one slice"), EOSV_ERR_ARG;
  const std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, true,
                                          {{"d_x", d_x}, {"d_dy", d_dy}, {"d_dw", d_dw}, {"d_work", d_work}});
  if (!why.empty()) return set_error("eosv_conv_wgrad_x3: " + why), EOSV_ERR_UNSUPPORTED;
  const X3Plan p = x3_plan(Cout, sh.K, sh.P, true, room);
  if (p.slices > 65535) return set_error("eosv_conv_wgrad_x3: a grid too large"), EOSV_ERR_UNSUPPORTED;
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.dy = d_dy, g.kps = p.kps, g.partial = p.slices > 1;
  g.out = g.partial ? d_work : d_dw;
  const int rows = XB_K / sh.Wo;
  g.s_ow = XB_K % sh.Wo, g.s_oh = rows % sh.Ho, g.s_n = rows / sh.Ho;
  const dim3 grid((unsigned)(p.mt * p.nt), (unsigned)p.slices);
  x3_dispatch(p, [&](auto wm, auto wn) {
    hipLaunchKernelGGL((conv_wgrad_x3_kernel<wm(), wn()>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g);
  });
  EOSV_LAUNCH_CHECK();
  if (g.partial) return launch_x3_slice_sum(d_work, p.slices, Cout, (int)sh.K, d_dw, sh.K, (hipStream_t)stream);
  return EOSV_OK;
}

}  // extern "C"
