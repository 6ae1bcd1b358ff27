// f32x3 implicit GEMM of a strided conv's input gradient (opt-in: NativeTrainer(f32x3_dgrad=...)): the
// arithmetic of gemm_x3.hip and conv_x3.hip (f32 operands in memory, split into hi + lo bf16 on the way
// into LDS, lo*hi, hi*lo, hi*hi per 32-k step on bf16 MFMA, f32 accumulation, k strictly increasing, no
// atomics) for
//   dX[n, h, w, ci] = sum over (kh, kw, co) of dY[n, (h + p - kh) / s, (w + p - kw) / s, co] W[co, kh, kw, ci]
// over the taps whose two quotients are exact and inside the output map (loss.backward(), reference
// network_train.py:114).  No dcol[P][KH KW Cin] buffer, no col2im pass, and no zero-dilated dY either:
// the input pixels with ((h + p) mod s, (w + p) mod s) = (ph, pw) form one of s^2 parity classes, and only
// the taps kh = ph + s jh < KH, kw = pw + s jw < KW reach a class.  Within a class the gather is a stride-1
// correlation: with oh0 = (h + p - ph) / s, tap jh reads output row oh0 - jh where that lies in [0, Ho).
// Each class is one GEMM: rows its pixels (n, hc, wc), columns Cin, reduction k = (tap in increasing
// (kh, kw) order, co), so the MACs of all classes together are P K Cin, the explicit GEMM's.  Cout % 32
// == 0, so a 32-k step lies in one tap.  The weight operand is eosv_flip_weights' [Cin][KH][KW][Cout]
// tap-reversed copy: tap (kh, kw) starts at k offset ((KH - 1 - kh) KW + (KW - 1 - kw)) Cout.
//
// One launch covers the s^2 classes: the grid is the sum of the classes' row tiles x the column tiles, and
// a block finds its class from the prefix table in the arguments (uniform).  Every pixel of dX is written
// exactly once; a class without taps (a 1x1 stride-2 shortcut has three) and a pixel whose taps all fall
// outside the output map get 0 + addend from blocks that run no step.  The K loop is conv_x3_kernel's
// (X3Tile::k_loop): two sets of the four LDS images, one barrier per step.
#include "x3_tile.h"

namespace eosv {

namespace {
constexpr int XD_MAXS = 4;                  // strides 2 .. XD_MAXS: the class table holds XD_MAXS^2 entries
constexpr int XD_MAXC = XD_MAXS * XD_MAXS;

struct ConvDgradX3Args {
  const float* dy;    // [N][Ho][Wo][Cout]
  const float* wf;    // [Cin][KH][KW][Cout], taps reversed (eosv_flip_weights)
  const float* add;   // [N H W][Cin] addend or nullptr
  float* dx;          // [N][H][W][Cin]
  int N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
  int Kf;             // KH KW Cout: a row of wf
  int nt;             // tiles along Cin
  int first[XD_MAXC]; // class (ph, pw) = ph stride + pw: its first row tile; classes past stride^2: the tile count
};

// the pixels of one parity class along one axis: the first coordinate, how many there are, the output
// coordinate tap 0 reads at the first one, and the taps that reach the class
struct ClassAxis {
  int first, count, ob, taps;
};

__host__ __device__ __forceinline__ ClassAxis class_axis(int ph, int size, int k, int s, int pad) {
  ClassAxis a;
  a.first = ((ph - pad) % s + s) % s;
  a.count = a.first < size ? (size - a.first + s - 1) / s : 0;
  a.ob = (a.first + pad - ph) / s;
  a.taps = ph < k ? (k - ph + s - 1) / s : 0;
  return a;
}

template <int WM, int WN>
__global__ __launch_bounds__(XB_NT) void conv_dgrad_x3_kernel(ConvDgradX3Args g) {
  using Tile = X3Tile<WM, WN>;
  constexpr int NP = Tile::BM / 32;   // rows of A a thread stages
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * Tile::IMG];
  const Tile t;
  const int tid = t.tid;
  const int tn = blockIdx.x % g.nt, rt = blockIdx.x / g.nt;

  // the block's class: the last one whose first tile is not past rt (an empty class shares its first
  // tile with the next one, which wins); uniform
  int cls = 0, tm = rt;
#pragma unroll
  for (int i = 1; i < XD_MAXC; ++i)
    if (rt >= g.first[i]) cls = i, tm = rt - g.first[i];
  const int s = g.stride;
  const int ph = cls / s, pw = cls - ph * s;
  const ClassAxis ah = class_axis(ph, g.H, g.KH, s, g.pad), aw = class_axis(pw, g.W, g.KW, s, g.pad);
  const int hw = ah.count * aw.count;
  const long long Pc = (long long)g.N * hw;   // the class's rows
  const long long m0 = (long long)tm * t.BM, n0 = (long long)tn * t.BN;
  const int steps = ah.taps * aw.taps * (g.Cout / XB_K);   // 0: a class without taps

  Stage<Tile::BM, false> sa;
  Stage<Tile::BN, false> sb;

  // this thread's rows: the output pixel tap (0, 0) reads and its frame's first output pixel; a row past
  // Pc lies outside the map at every tap
  int oh0[NP], ow0[NP];
  long long frame[NP];
#pragma unroll
  for (int r = 0; r < NP; ++r) {
    const long long p = m0 + ((tid + r * XB_NT) >> 3);
    oh0[r] = -0x40000000, ow0[r] = 0, frame[r] = 0;
    if (p < Pc) {
      const long long n = p / hw;
      const int rem = (int)(p - n * hw), hc = rem / aw.count, wc = rem - hc * aw.count;
      oh0[r] = ah.ob + hc;
      ow0[r] = aw.ob + wc;
      frame[r] = n * g.Ho * g.Wo;
    }
  }
  int jh = 0, jw = 0, c0 = 0;   // the step's tap within the class and first channel: uniform
  auto gather = [&] {
#pragma unroll
    for (int r = 0; r < NP; ++r) {
      const int oh = oh0[r] - jh, ow = ow0[r] - jw;
      sa.v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((unsigned)oh < (unsigned)g.Ho && (unsigned)ow < (unsigned)g.Wo)
        sa.v[r] = *(const f32x4*)(g.dy + (frame[r] + (long long)oh * g.Wo + ow) * g.Cout + c0 + 4 * (tid & 7));
    }
  };
  // k offset of the step in a row of wf: tap (kh, kw) = (ph + s jh, pw + s jw) lies reversed
  auto koff = [&] {
    return (long long)((g.KH - 1 - (ph + s * jh)) * g.KW + (g.KW - 1 - (pw + s * jw))) * g.Cout + c0;
  };

  typename Tile::Acc acc;
  t.zero(acc);
  t.k_loop(lds, steps, sa, sb, acc, [&](int step) {
    if (step) {   // one step on: the next 32 channels, or the class's next tap
      c0 += XB_K;
      if (c0 == g.Cout) {
        c0 = 0;
        if (++jw == aw.taps) jw = 0, ++jh;
      }
    }
    gather();
    sb.load(g.wf, g.Kf, n0, g.Cin, koff(), g.Kf, tid);
  });

  // the tile's rows are the class's: row p is pixel m of dX.  The kernel is short of SGPRs: what the
  // stores need is captured by value, or it is read again from the arguments at every store
  t.each(
      acc, m0, Pc, n0, g.Cin,
      [add = g.add, dx = g.dx, Cin = g.Cin](long long m, long long ci, f32x4 v) {
        if (add) v += *(const f32x4*)(add + m * Cin + ci);
        *(f32x4*)(dx + m * Cin + ci) = v;
      },
      [&](long long p) {
        const long long n = p / hw;
        const int rem = (int)(p - n * hw), hc = rem / aw.count, wc = rem - hc * aw.count;
        return (n * g.H + ah.first + s * hc) * g.W + aw.first + s * wc;
      });
}

// What a call runs, decided on the host from the sizes alone: the status the entry returns before any launch
// (EOSV_OK: g holds everything but the four pointers), the tile and the grid (0 workgroups at N = 0).  `who` prefixes the message.
int conv_dgrad_x3_plan(const char* who, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                       ConvDgradX3Args& g, X3Plan& p, long long& blocks) {
  ConvX3Shape sh{};
  if (!conv_x3_shape(N, H, W, Cin, Cout, KH, KW, stride, pad, sh))
    return set_error(std::string(who) + ": bad argument"), EOSV_ERR_ARG;
  g = ConvDgradX3Args{};
  p = X3Plan{};
  p.wm = p.wn = 1, blocks = 0;
  if (N == 0) return EOSV_OK;   // nothing to do, whatever the other sizes
  const long long Kf = (long long)KH * KW * Cout;
  std::string why;
  if (Cout % 32) why = "Cout = " + std::to_string(Cout) + " is not a multiple of 32";
  else if (Cin % 64) why = "Cin = " + std::to_string(Cin) + " is not a multiple of 64";
  else if (stride == 1) why = "stride 1 is eosv_conv2d_x3's";
  else if (stride > XD_MAXS) why = "stride = " + std::to_string(stride) + " is past the class table (2 .. 4)";
  else if (Kf > 0x7fffffffLL || (long long)H + 2LL * pad > 0x3fffffffLL || (long long)W + 2LL * pad > 0x3fffffffLL ||
           (long long)H * W > 0x7fffffffLL || (long long)sh.Ho * sh.Wo > 0x7fffffffLL)
    why = "a grid too large";
  if (!why.empty()) return set_error(std::string(who) + ": " + why), EOSV_ERR_UNSUPPORTED;
  // one plan for the launch, from the largest class's rows: every class runs the same instantiation
  const int ncls = stride * stride;
  long long rows[XD_MAXC] = {}, most = 0;
  for (int cls = 0; cls < ncls; ++cls) {
    const ClassAxis ah = class_axis(cls / stride, H, KH, stride, pad), aw = class_axis(cls % stride, W, KW, stride, pad);
    rows[cls] = (long long)N * ah.count * aw.count;
    most = std::max(most, rows[cls]);
  }
  p = x3_plan(std::max(most, 1LL), Cin, Kf, false, 1);
  long long tiles = 0;
  for (int cls = 0; cls < XD_MAXC; ++cls) {
    g.first[cls] = (int)std::min(tiles, 0x7fffffffLL);
    if (cls < ncls) tiles += (rows[cls] + 64 * p.wm - 1) / (64 * p.wm);
  }
  blocks = tiles * p.nt;
  if (blocks > 0x7fffffffLL) return set_error(std::string(who) + ": a grid too large"), EOSV_ERR_UNSUPPORTED;
  g.N = N, g.H = H, g.W = W, g.Cin = Cin, g.Cout = Cout, g.KH = KH, g.KW = KW, g.stride = stride, g.pad = pad;
  g.Ho = sh.Ho, g.Wo = sh.Wo, g.Kf = (int)Kf, g.nt = p.nt;
  return EOSV_OK;
}
}  // namespace

}  // namespace eosv

using namespace eosv;

extern "C" {

int eosv_conv_dgrad_x3_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* tile_m,
                            int* tile_n, int64_t* grid) {
  if (!tile_m || !tile_n || !grid) return set_error("eosv_conv_dgrad_x3_plan: bad argument"), EOSV_ERR_ARG;
  ConvDgradX3Args g;
  X3Plan p{};
  long long blocks = 0;
  const int rc = conv_dgrad_x3_plan("eosv_conv_dgrad_x3_plan", N, H, W, Cin, Cout, KH, KW, stride, pad, g, p, blocks);
  if (rc != EOSV_OK) return rc;
  *tile_m = 64 * p.wm, *tile_n = 64 * p.wn, *grid = (int64_t)blocks;
  return EOSV_OK;
}

int eosv_conv_dgrad_x3(const float* d_dy, int N, int H, int W, int Cin, const float* d_wf, int Cout, int KH, int KW,
                       int stride, int pad, const float* d_add, float* d_dx, eosv_stream_t stream) {
  if (!d_dy || !d_wf || !d_dx) return set_error("eosv_conv_dgrad_x3: bad argument"), EOSV_ERR_ARG;
  ConvDgradX3Args g;
  X3Plan p{};
  long long blocks = 0;
  const int rc = conv_dgrad_x3_plan("eosv_conv_dgrad_x3", N, H, W, Cin, Cout, KH, KW, stride, pad, g, p, blocks);
  if (rc != EOSV_OK || N == 0) return rc;
  if (const char* op = x3_misaligned({{"d_dy", d_dy}, {"d_wf", d_wf}, {"d_add", d_add}, {"d_dx", d_dx}}))
    return set_error(std::string("eosv_conv_dgrad_x3: ") + op + " is off 16 bytes"), EOSV_ERR_UNSUPPORTED;
  g.dy = d_dy, g.wf = d_wf, g.add = d_add, g.dx = d_dx;
  const dim3 grid((unsigned)blocks);
  x3_dispatch(p, [&](auto wm, auto wn) {
    hipLaunchKernelGGL((conv_dgrad_x3_kernel<wm(), wn()>), grid, dim3(XB_NT), 0, (hipStream_t)stream, g);
  });
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

}  // extern "C"
