// What the f32x3 kernels share (gemm_x3.hip: the GEMMs of the stride-1 1x1 convs; conv_x3.hip: the
// implicit GEMMs of the KxK and strided convs; conv_dgrad_x3.hip: the strided convs' input gradient).
// Device side: the hi / lo split on the way into LDS, the LDS image layout, the staging of a 32-k
// operand tile (Stage), the fragment reads and MFMAs of a 32-k step, and X3Tile, the frame of a
// workgroup's tile: its constants, the thread's place in it, the double-buffered K loop of the three
// conv kernels, the epilogue walk and, for the STATS kernels, x3_tile_stats (gemm_x3_kernel takes the
// constants, the accumulators and the statistics and writes its indices, loop and epilogue out: the
// reason is at the kernel).  Host side: the plan, the
// tile dispatch, the checks the entries have in common and the slice sum of a split reduction
// (defined in gemm_x3.hip).  The arithmetic is stated in gemm_x3.hip's header comment.
#pragma once
#include "common.h"

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <utility>

namespace eosv {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int XB_K = 32;       // reduction rows per step (one 16x16x32 MFMA)
constexpr int XB_NT = 256;     // threads per workgroup
constexpr int XB_ROWB = 64;    // bytes of an LDS image row: 32 bf16
constexpr int X3_CUS = 256;    // the plan's CU count: fixed, so a plan does not depend on the device

// two f32 -> their bf16 (round to nearest even) as one word, element 0 in the low half
__device__ __forceinline__ unsigned pack_bf2(float e0, float e1) {
  const bf16x2v p = __builtin_convertvector((f32x2v){e0, e1}, bf16x2v);
  return __builtin_bit_cast(unsigned, p);
}

// 4 consecutive k of one row: hi and lo as 8 bytes each
__device__ __forceinline__ void split4(const f32x4 v, u32x2& hi, u32x2& lo) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const unsigned h = pack_bf2(v[2 * p], v[2 * p + 1]);
    const float r0 = v[2 * p] - __uint_as_float(h << 16);
    const float r1 = v[2 * p + 1] - __uint_as_float(h & 0xffff0000u);
    hi[p] = h;
    lo[p] = pack_bf2(r0, r1);
  }
}

// byte offset of 16-byte chunk `ch` (8 k) of row `row` in an image
__device__ __forceinline__ int img_off(int row, int ch) { return row * XB_ROWB + ((ch ^ ((row & 8) ? 3 : 0)) << 4); }

// An operand tile of R rows (m of A or n of B) x 32 k.  KSLOW: the operand is [k][row] in memory.
template <int R, bool KSLOW>
struct Stage {
  // k fast: float4 pieces of 4 k, 8 per row, R / 32 per thread.  k slow: 4 k x 4 row blocks, 8 k
  // groups (fastest over the threads: a wave's LDS writes then spread over the banks) x R / 4 row
  // groups; R = 64 has 128 blocks, for the first 128 threads.
  static constexpr int NP = KSLOW ? 1 : R / 32;
  static constexpr int NV = KSLOW ? 4 : NP;
  f32x4 v[NV];

  // rows [row0, row0 + R) of the operand, k in [kb, kb + 32); zeros for rows >= rows and k >= k1
  __device__ __forceinline__ void load(const float* __restrict__ p, long long ld, long long row0, long long rows,
                                       long long kb, long long k1, int tid) {
    if (KSLOW) {
      const int kg = tid & 7, rg = tid >> 3;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long k = kb + 4 * kg + t;
        v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rg < R / 4 && k < k1) v[t] = *(const f32x4*)(p + k * ld + row0 + 4 * rg);
      }
    } else {
#pragma unroll
      for (int s = 0; s < NP; ++s) {
        const int idx = tid + s * XB_NT, r = idx >> 3, c = idx & 7;
        v[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row0 + r < rows) v[s] = *(const f32x4*)(p + (row0 + r) * ld + kb + 4 * c);
      }
    }
  }

  __device__ __forceinline__ void store(unsigned char* hi_img, unsigned char* lo_img, int tid) const {
    if (KSLOW) {
      const int kg = tid & 7, rg = tid >> 3;
      if (rg < R / 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          u32x2 h, l;
          split4(f32x4{v[0][e], v[1][e], v[2][e], v[3][e]}, h, l);
          const int off = img_off(4 * rg + e, kg >> 1) + 8 * (kg & 1);
          *(u32x2*)(hi_img + off) = h;
          *(u32x2*)(lo_img + off) = l;
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < NP; ++s) {
        const int idx = tid + s * XB_NT, r = idx >> 3, c = idx & 7;
        u32x2 h, l;
        split4(v[s], h, l);
        const int off = img_off(r, c >> 1) + 8 * (c & 1);
        *(u32x2*)(hi_img + off) = h;
        *(u32x2*)(lo_img + off) = l;
      }
    }
  }
};

// One 32-k step of a wave: its 64 columns of B (image rows from `brow`) against MI 16-row blocks of
// A (image rows from `arow`), lane = 16 q + c.  D = (A B)^T: rows of D are n.  Per block the two
// cross terms, then hi * hi
template <int MI>
__device__ __forceinline__ void x3_mma_step(const unsigned char* a_hi, const unsigned char* a_lo,
                                            const unsigned char* b_hi, const unsigned char* b_lo, int arow, int brow,
                                            int c, int q, f32x4 (&acc)[MI][4]) {
  bf16x8 bh[4], bl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int off = img_off(brow + 16 * j + c, q);
    bh[j] = *(const bf16x8*)(b_hi + off);
    bl[j] = *(const bf16x8*)(b_lo + off);
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int off = img_off(arow + 16 * i + c, q);
    const bf16x8 ah = *(const bf16x8*)(a_hi + off);
    const bf16x8 al = *(const bf16x8*)(a_lo + off);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], ah, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], al, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], ah, acc[i][j], 0, 0, 0);
  }
}

// The frame of a workgroup's BM x BN tile: 2 x 2, 2 x 1, 1 x 2 or 1 x 1 parts of 64 x 64.  Always 4
// waves: a tile of fewer than four parts deals each part's four 16-row m-blocks over SUB waves.
template <int WM, int WN>
struct X3Tile {
  static constexpr int BM = 64 * WM, BN = 64 * WN;
  static constexpr int SUB = 4 / (WM * WN);             // waves per 64 x 64 part: 1, 2 or 4
  static constexpr int MI = 4 / SUB;                    // 16-row m-blocks per wave
  static constexpr int IMG = 2 * (BM + BN) * XB_ROWB;   // one set of the four images: A hi, A lo, B hi, B lo
  using Acc = f32x4[MI][4];

  const int tid = threadIdx.x, wave = tid >> 6;
  const int sub = wave % SUB;                           // the wave within its part
  const int wm = wave / SUB / WN, wn = wave / SUB % WN; // the part within the tile
  const int q = (tid & 63) >> 4, c = tid & 15;          // lane = 16 q + c

  // The lane's element of block (i, j) of the accumulators of the tile at (m0, n0): row(m0, i), and
  // the 4 columns from col(n0, j) (D = (A B)^T: x3_mma_step).  64-bit throughout: 16 i and 16 j then
  // fold into the address offsets of the epilogue's loads and stores
  __device__ __forceinline__ long long row(long long m0, int i) const { return m0 + 64 * wm + 16 * (MI * sub + i) + c; }
  __device__ __forceinline__ long long col(long long n0, int j) const { return n0 + 64 * wn + 16 * j + 4 * q; }

  __device__ __forceinline__ static void zero(Acc& acc) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // the staged step into the image set at img
  template <class SA, class SB>
  __device__ __forceinline__ void store(unsigned char* img, const SA& sa, const SB& sb) const {
    sa.store(img, img + BM * XB_ROWB, tid);
    sb.store(img + 2 * BM * XB_ROWB, img + (2 * BM + BN) * XB_ROWB, tid);
  }

  // the wave's MFMAs of the step in the image set at img
  __device__ __forceinline__ void mma(const unsigned char* img, Acc& acc) const {
    x3_mma_step<MI>(img, img + BM * XB_ROWB, img + 2 * BM * XB_ROWB, img + (2 * BM + BN) * XB_ROWB,
                    64 * wm + 16 * MI * sub, 64 * wn, c, q, acc);
  }

  // The K loop of the conv kernels over two image sets (lds: 2 IMG bytes): fetch(s) brings the
  // operands of step s into sa / sb (registers), called in step order, for s + 1 before the MFMAs of
  // step s; they are stored into the other set after them: one barrier per step.  No step: nothing is
  // fetched or stored.  The images are free once this returns.
  template <class SA, class SB, class Fetch>
  __device__ __forceinline__ void k_loop(unsigned char* lds, int steps, SA& sa, SB& sb, Acc& acc, Fetch fetch) const {
    if (steps > 0) {
      fetch(0);
      store(lds, sa, sb);
    }
    __syncthreads();
    for (int step = 0; step < steps; ++step) {
      const bool more = step + 1 < steps;
      if (more) fetch(step + 1);
      mma(lds + (step & 1) * IMG, acc);
      if (more) store(lds + ((step + 1) & 1) * IMG, sa, sb);
      __syncthreads();
    }
  }

  // The epilogue walk: f(r, n, acc[i][j]) for each block (i, j) of the lane with m = row(m0, i) < M
  // and n = col(n0, j) < N, where r = at(m), taken once per i (a kernel whose rows are not its
  // output's rows maps them there)
  template <class F, class At>
  __device__ __forceinline__ void each(const Acc& acc, long long m0, long long M, long long n0, long long N, F f,
                                       At at) const {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const long long m = row(m0, i);
      if (m >= M) continue;
      const long long r = at(m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long n = col(n0, j);
        if (n < N) f(r, n, acc[i][j]);
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void each(const Acc& acc, long long m0, long long M, long long n0, long long N, F f) const {
    each(acc, m0, M, n0, N, f, [](long long m) { return m; });
  }
};

// v of the lane `CTRL` names within its 16-lane DPP row (every lane of the wave active)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// the sum of v over the 16 lanes of a DPP row, in every lane of the row, in one fixed order: lane
// pairs (quad_perm [1 0 3 2]), quads ([2 3 0 1]), the two quads of a half row (row_half_mirror), the
// two half rows (row_mirror).  f64 addition commutes, so the 16 lanes hold the same bits.
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}

// The BN batch statistics of a forward tile (the STATS kernels): part[tm][0][n] = sum over the tile's
// rows m < M of v, part[tm][1][n] of v * v, in f64, v the f32 values as stored (acc: the epilogue of
// a STATS launch adds nothing to it).  Column by column of the lane's blocks (X3Tile::row, col; 8 f64
// live, not 32): the lane's rows in i order, the 16 lanes of its DPP row (row16_sum), then through
// LDS (red[wave][2][64], the images being free after the K loop's last barrier) the waves that hold
// the same columns in wave order.  One thread per column writes; columns n >= N are not written.  No
// atomics: a fixed order throughout.
template <int WM, int WN>
__device__ __forceinline__ void x3_tile_stats(const X3Tile<WM, WN>& t, const typename X3Tile<WM, WN>::Acc& acc,
                                              long long m0, long long M, long long n0, long long N, int tm,
                                              unsigned char* lds, double* __restrict__ part) {
  constexpr int SUB = X3Tile<WM, WN>::SUB, MI = X3Tile<WM, WN>::MI;
  const int c = t.c, q = t.q, wave = t.wave, tid = t.tid;
  double* const red = (double*)lds;
  bool live[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) live[i] = t.row(m0, i) < M;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const double d = live[i] ? (double)acc[i][j][e] : 0.0;
        s0 += d;
        s1 += d * d;  // exact in f64: fused or not, the same bits
      }
      s0 = row16_sum(s0);
      s1 = row16_sum(s1);
      if (c == 0) {
        red[(2 * wave) * 64 + 16 * j + 4 * q + e] = s0;
        red[(2 * wave + 1) * 64 + 16 * j + 4 * q + e] = s1;
      }
    }
  __syncthreads();
  const long long n = n0 + tid;
  if (tid < 64 * WN && n < N) {
    const int twn = tid >> 6, col = tid & 63;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int pm = 0; pm < WM; ++pm)
#pragma unroll
      for (int ps = 0; ps < SUB; ++ps) {
        const int w = (pm * WN + twn) * SUB + ps;
        s0 += red[(2 * w) * 64 + col];
        s1 += red[(2 * w + 1) * 64 + col];
      }
    part[((long long)tm * 2) * N + n] = s0;
    part[((long long)tm * 2 + 1) * N + n] = s1;
  }
}

struct X3Plan {
  int wm, wn, mt, nt;
  int slices;  // slices the grid runs
  int cap;     // the slice count the workspace is sized for (>= slices, monotone in k)
  int kps;
};

// tile: 128 x 128 (64 where a dimension is 64); unsplit, halved along m and then along n while the
// grid has fewer than two workgroups per CU; split (TN): slices so that tiles x slices is about
// three workgroups per CU, with at least 256 reduction rows per slice and at most 1024 slices
X3Plan x3_plan(long long m, long long n, long long k, bool split, int max_slices) {
  X3Plan p{};
  p.wm = m > 64 ? 2 : 1;
  p.wn = n > 64 ? 2 : 1;
  auto tiles = [&] {
    p.mt = (int)((m + 64 * p.wm - 1) / (64 * p.wm));
    p.nt = (int)((n + 64 * p.wn - 1) / (64 * p.wn));
    return (long long)p.mt * p.nt;
  };
  if (!split && tiles() < 2 * X3_CUS && p.wm == 2) p.wm = 1;
  if (!split && tiles() < 2 * X3_CUS && p.wn == 2) p.wn = 1;
  const long long t = tiles();
  long long s = 1;
  if (split) {
    s = std::max(1LL, std::min((3LL * X3_CUS + t - 1) / t, k / 256));
    s = std::min(s, 1024LL);
  }
  p.cap = (int)s;
  s = std::min<long long>(s, std::max(1, max_slices));
  long long kps = (k + s - 1) / s;
  if (s > 1) kps = (kps + XB_K - 1) / XB_K * XB_K;
  p.kps = (int)std::max(1LL, kps);
  p.slices = std::max(1, (int)((k + p.kps - 1) / p.kps));
  return p;
}
}  // namespace

// f(WM, WN) with the plan's tile as two std::integral_constant: the one place a plan picks among
// the four instantiations of a kernel
template <class F>
void x3_dispatch(const X3Plan& p, F f) {
  using one = std::integral_constant<int, 1>;
  using two = std::integral_constant<int, 2>;
  switch (p.wm * 2 + p.wn) {
    case 3: f(one{}, one{}); break;
    case 4: f(one{}, two{}); break;
    case 5: f(two{}, one{}); break;
    default: f(two{}, two{}); break;
  }
}

// the name of the first operand that is off 16 bytes, or nullptr (a null pointer is aligned)
inline const char* x3_misaligned(std::initializer_list<std::pair<const char*, const void*>> ops) {
  for (const auto& op : ops)
    if (((uintptr_t)op.second & 15) != 0) return op.first;
  return nullptr;
}

// The workspace rule of the split (TN) entries, `need` being what their _workspace function returns
// (0: the plan does not split).  0, the error and nothing else: a workspace is given where the plan
// splits and holds less than one slice.  Else the slices x3_plan may run, at least 1 (the clamp keeps
// a short workspace of a plan that does not split apart from the error): one, straight into the
// result, with no workspace, and as many as a short one holds.
inline int x3_split_room(const void* work, int64_t work_bytes, int64_t need, int64_t slice_bytes) {
  if (work && need > 0 && work_bytes < slice_bytes) return 0;
  return work ? (int)std::clamp<int64_t>(work_bytes / slice_bytes, 1, 1024) : 1;
}

// a conv's output map and GEMM sizes
struct ConvX3Shape {
  long long P, K;   // N Ho Wo, KH KW Cin
  int Ho, Wo;
};

// false: a non-positive size or an empty output map
inline bool conv_x3_shape(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, ConvX3Shape& o) {
  if (N < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return false;
  const long long eh = (long long)H + 2LL * pad - KH, ew = (long long)W + 2LL * pad - KW;
  if (eh < 0 || ew < 0) return false;
  o.Ho = (int)(eh / stride + 1), o.Wo = (int)(ew / stride + 1);
  o.P = (long long)N * o.Ho * o.Wo;
  o.K = (long long)KH * KW * Cin;
  return true;
}

// C[m][n] = sum over the slices, in slice order, of work[s][m][n] (n % 4 == 0): gemm_x3.hip
int launch_x3_slice_sum(const float* work, int slices, int m, int n, float* c, long long ldc, hipStream_t s);

}  // namespace eosv
