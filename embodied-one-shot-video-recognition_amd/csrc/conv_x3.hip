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
// Both kernels keep two sets of the four LDS images: step s + 1 is loaded to registers before the
// MFMAs of step s and stored into the other set after them, one barrier per step.
#include "x3_tile.h"

#include <utility>

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
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int SUB = 4 / (WM * WN);   // waves per 64 x 64 part, as gemm_x3_kernel
  constexpr int MI = 4 / SUB;
  constexpr int IMG = 2 * (BM + BN) * XB_ROWB;   // one set of the four images
  constexpr int NP = BM / 32;                     // rows of A a thread stages
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * IMG];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = wave / SUB, sub = wave - SUB * part;
  const int wm = part / WN, wn = part - WN * wm;
  const int tn = blockIdx.x % g.nt, tm = blockIdx.x / g.nt;
  const long long m0 = (long long)tm * BM, n0 = (long long)tn * BN;
  const int steps = g.K / XB_K;

  Stage<BM, false> sa;
  Stage<BN, false> sb;

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

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int q = lane >> 4, c = lane & 15;
  gather();
  sb.load(g.w, g.K, n0, g.Cout, 0, g.K, tid);
  sa.store(lds, lds + BM * XB_ROWB, tid);
  sb.store(lds + 2 * BM * XB_ROWB, lds + (2 * BM + BN) * XB_ROWB, tid);
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    unsigned char* const cur = lds + (step & 1) * IMG;
    unsigned char* const nxt = lds + ((step + 1) & 1) * IMG;
    const bool more = step + 1 < steps;
    if (more) {
      c0 += XB_K;
      if (c0 == g.Cin) {
        c0 = 0;
        if (++kw == g.KW) kw = 0, ++kh;
      }
      gather();
      sb.load(g.w, g.K, n0, g.Cout, (long long)(step + 1) * XB_K, g.K, tid);
    }
    x3_mma_step<MI>(cur, cur + BM * XB_ROWB, cur + 2 * BM * XB_ROWB, cur + (2 * BM + BN) * XB_ROWB,
                    64 * wm + 16 * MI * sub, 64 * wn, c, q, acc);
    if (more) {
      sa.store(nxt, nxt + BM * XB_ROWB, tid);
      sb.store(nxt + 2 * BM * XB_ROWB, nxt + (2 * BM + BN) * XB_ROWB, tid);
    }
    __syncthreads();
  }

  // lane holds, of block (i, j), m = m0 + 64 wm + 16 (MI sub + i) + c and n = n0 + 64 wn + 16 j + 4 q + (0..3)
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const long long m = m0 + 64 * wm + 16 * (MI * sub + i) + c;
    if (m >= g.P) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long n = n0 + 64 * wn + 16 * j + 4 * q;
      if (n >= g.Cout) continue;
      f32x4 v = acc[i][j];
      if (g.add) v += *(const f32x4*)(g.add + m * g.Cout + n);
      *(f32x4*)(g.out + m * g.Cout + n) = v;
    }
  }
  if constexpr (STATS) x3_tile_stats<WM, WN, MI>(acc, m0, g.P, n0, g.Cout, tm, wm, sub, c, q, wave, tid, lds, g.stats);
}

template <int WM, int WN>
__global__ __launch_bounds__(XB_NT) void conv_wgrad_x3_kernel(ConvX3Args g) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int SUB = 4 / (WM * WN);
  constexpr int MI = 4 / SUB;
  constexpr int IMG = 2 * (BM + BN) * XB_ROWB;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * IMG];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = wave / SUB, sub = wave - SUB * part;
  const int wm = part / WN, wn = part - WN * wm;
  const int tn = blockIdx.x % g.nt, tm = blockIdx.x / g.nt;
  const long long m0 = (long long)tm * BM, n0 = (long long)tn * BN;   // rows: Cout, columns: K
  const long long k0 = (long long)blockIdx.y * g.kps;
  const long long k1 = min(g.P, k0 + g.kps);
  const int steps = (int)((k1 - k0 + XB_K - 1) / XB_K);

  Stage<BM, true> sa;
  Stage<BN, true> sb;

  // a thread stages 4 pixels (k group kg) x 4 rows of dY and x 4 columns of col(X) (row group rg)
  const int kg = tid & 7, rg = tid >> 3;
  const bool a_on = rg < BM / 4 && m0 + 4 * rg < g.Cout;
  const long long col = n0 + 4 * rg;
  const bool b_on = rg < BN / 4 && col < g.K;
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

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int q = lane >> 4, c = lane & 15;
  if (steps > 0) {
    gather();
    sa.store(lds, lds + BM * XB_ROWB, tid);
    sb.store(lds + 2 * BM * XB_ROWB, lds + (2 * BM + BN) * XB_ROWB, tid);
  }
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    unsigned char* const cur = lds + (step & 1) * IMG;
    unsigned char* const nxt = lds + ((step + 1) & 1) * IMG;
    const bool more = step + 1 < steps;
    if (more) {
      advance();
      gather();
    }
    x3_mma_step<MI>(cur, cur + BM * XB_ROWB, cur + 2 * BM * XB_ROWB, cur + (2 * BM + BN) * XB_ROWB,
                    64 * wm + 16 * MI * sub, 64 * wn, c, q, acc);
    if (more) {
      sa.store(nxt, nxt + BM * XB_ROWB, tid);
      sb.store(nxt + 2 * BM * XB_ROWB, nxt + (2 * BM + BN) * XB_ROWB, tid);
    }
    __syncthreads();
  }

  float* out = g.partial ? g.out + (long long)blockIdx.y * g.Cout * g.K : g.out;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const long long m = m0 + 64 * wm + 16 * (MI * sub + i) + c;
    if (m >= g.Cout) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long nn = n0 + 64 * wn + 16 * j + 4 * q;
      if (nn >= g.K) continue;
      *(f32x4*)(out + m * g.K + nn) = acc[i][j];
    }
  }
}

// the conv's output map and GEMM sizes
struct ConvX3Shape {
  long long P, K;
  int Ho, Wo;
};

// false: a non-positive size or an empty output map
bool conv_x3_shape(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, ConvX3Shape& o) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return false;
  const long long eh = (long long)H + 2LL * pad - KH, ew = (long long)W + 2LL * pad - KW;
  if (eh < 0 || ew < 0) return false;
  o.Ho = (int)(eh / stride + 1), o.Wo = (int)(ew / stride + 1);
  o.P = (long long)N * o.Ho * o.Wo;
  o.K = (long long)KH * KW * Cin;
  return true;
}

// what the kernels do not take, naming the operand (pointers apart: the entries check those); empty: taken
std::string conv_x3_refusal(int H, int W, int Cin, int Cout, int pad, const ConvX3Shape& g, bool wgrad) {
  if (Cin % 32) return "Cin = " + std::to_string(Cin) + " is not a multiple of 32";
  if (Cout % 64) return "Cout = " + std::to_string(Cout) + " is not a multiple of 64";
  const long long tiles = (((wgrad ? g.K : g.P) + 63) / 64) * (Cout / 64);
  if (g.K > 0x7fffffffLL || (long long)H + 2LL * pad > 0x3fffffffLL || (long long)W + 2LL * pad > 0x3fffffffLL ||
      (long long)g.Ho * g.Wo > 0x7fffffffLL || tiles > 0x7fffffffLL)
    return "a grid too large";
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

#define EOSV_CONV_X3_LAUNCH(KERNEL, P_, GRID, S, G)                                       \
  switch ((P_).wm * 2 + (P_).wn) {                                                         \
    case 3: hipLaunchKernelGGL((KERNEL<1, 1>), GRID, dim3(XB_NT), 0, S, G); break;         \
    case 4: hipLaunchKernelGGL((KERNEL<1, 2>), GRID, dim3(XB_NT), 0, S, G); break;         \
    case 5: hipLaunchKernelGGL((KERNEL<2, 1>), GRID, dim3(XB_NT), 0, S, G); break;         \
    default: hipLaunchKernelGGL((KERNEL<2, 2>), GRID, dim3(XB_NT), 0, S, G); break;        \
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
  std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, false);
  for (const auto& op : {std::make_pair("d_x", (const void*)d_x), std::make_pair("d_w", (const void*)d_w),
                         std::make_pair("d_add", (const void*)d_add), std::make_pair("d_y", (const void*)d_y)})
    if (why.empty() && !aligned16(op.second)) why = std::string(op.first) + " is off 16 bytes";
  if (!why.empty()) return set_error("eosv_conv2d_x3: " + why), EOSV_ERR_UNSUPPORTED;
  const X3Plan p = x3_plan(sh.P, Cout, sh.K, false, 1);
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.w = d_w, g.add = d_add, g.out = d_y;
  const dim3 grid((unsigned)(p.mt * p.nt));
  EOSV_CONV_X3_LAUNCH(conv_x3_kernel, p, grid, (hipStream_t)stream, g)
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
  std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, false);
  for (const auto& op : {std::make_pair("d_x", (const void*)d_x), std::make_pair("d_w", (const void*)d_w),
                         std::make_pair("d_y", (const void*)d_y), std::make_pair("d_stats", (const void*)d_stats)})
    if (why.empty() && !aligned16(op.second)) why = std::string(op.first) + " is off 16 bytes";
  if (!why.empty()) return set_error("eosv_conv2d_x3_stats: " + why), EOSV_ERR_UNSUPPORTED;
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.w = d_w, g.out = d_y, g.stats = d_stats;
  const dim3 grid((unsigned)(p.mt * p.nt));
  switch (p.wm * 2 + p.wn) {
    case 3: hipLaunchKernelGGL((conv_x3_kernel<1, 1, true>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g); break;
    case 4: hipLaunchKernelGGL((conv_x3_kernel<1, 2, true>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g); break;
    case 5: hipLaunchKernelGGL((conv_x3_kernel<2, 1, true>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g); break;
    default: hipLaunchKernelGGL((conv_x3_kernel<2, 2, true>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g); break;
  }
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
  const int64_t slice_bytes = (int64_t)Cout * sh.K * (int64_t)sizeof(float);
  // a workspace is given where the plan splits: it must hold one slice at least
  if (d_work && eosv_conv_wgrad_x3_workspace(N, H, W, Cin, Cout, KH, KW, stride, pad) > 0 && work_bytes < slice_bytes)
    return set_error("eosv_conv_wgrad_x3: workspace smaller than one slice"), EOSV_ERR_ARG;
  std::string why = conv_x3_refusal(H, W, Cin, Cout, pad, sh, true);
  for (const auto& op : {std::make_pair("d_x", (const void*)d_x), std::make_pair("d_dy", (const void*)d_dy),
                         std::make_pair("d_dw", (const void*)d_dw), std::make_pair("d_work", (const void*)d_work)})
    if (why.empty() && !aligned16(op.second)) why = std::string(op.first) + " is off 16 bytes";
  if (!why.empty()) return set_error("eosv_conv_wgrad_x3: " + why), EOSV_ERR_UNSUPPORTED;
  // no workspace: one slice straight into dW; a short one: as many slices as it holds
  const int room = d_work ? (int)std::min<int64_t>(work_bytes / slice_bytes, 1024) : 1;
  const X3Plan p = x3_plan(Cout, sh.K, sh.P, true, room);
  if (p.slices > 65535) return set_error("eosv_conv_wgrad_x3: a grid too large"), EOSV_ERR_UNSUPPORTED;
  ConvX3Args g = conv_x3_args(d_x, H, W, Cin, Cout, KH, KW, stride, pad, sh, p);
  g.dy = d_dy, g.kps = p.kps, g.partial = p.slices > 1;
  g.out = g.partial ? d_work : d_dw;
  const int rows = XB_K / sh.Wo;
  g.s_ow = XB_K % sh.Wo, g.s_oh = rows % sh.Ho, g.s_n = rows / sh.Ho;
  const dim3 grid((unsigned)(p.mt * p.nt), (unsigned)p.slices);
  EOSV_CONV_X3_LAUNCH(conv_wgrad_x3_kernel, p, grid, (hipStream_t)stream, g)
  EOSV_LAUNCH_CHECK();
  if (g.partial) return launch_x3_slice_sum(d_work, p.slices, Cout, (int)sh.K, d_dw, sh.K, (hipStream_t)stream);
  return EOSV_OK;
}

}  // extern "C"
