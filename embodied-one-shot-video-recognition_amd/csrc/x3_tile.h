// What the f32x3 kernels share (gemm_x3.hip: the GEMMs of the stride-1 1x1 convs; conv_x3.hip: the
// implicit GEMMs of the KxK and strided convs): the hi / lo split on the way into LDS, the LDS image
// layout, the staging of a 32-k operand tile, the fragment reads and MFMAs of a 32-k step, the plan
// and the slice sum of a split reduction.  The arithmetic is stated in gemm_x3.hip's header comment.
#pragma once
#include "common.h"

#include <algorithm>

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
// a STATS launch adds nothing to it).  A lane holds, of block (i, j), row m0 + 64 wm + 16 (MI sub + i)
// + c and columns 64 wn + 16 j + 4 q + (0..3).  Column by column (8 f64 live, not 32): the lane's rows
// in i order, the 16 lanes of its DPP row (row16_sum), then through LDS (red[wave][2][64], the images
// being free after the K loop's last barrier) the waves that hold the same columns in wave order.
// One thread per column writes; columns n >= N are not written.  No atomics: a fixed order throughout.
template <int WM, int WN, int MI>
__device__ __forceinline__ void x3_tile_stats(const f32x4 (&acc)[MI][4], long long m0, long long M, long long n0,
                                              long long N, int tm, int wm, int sub, int c, int q, int wave, int tid,
                                              unsigned char* lds, double* __restrict__ part) {
  constexpr int SUB = 4 / (WM * WN);
  double* const red = (double*)lds;
  bool live[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) live[i] = m0 + 64 * wm + 16 * (MI * sub + i) + c < M;
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

// C[m][n] = sum over slices (in slice order) of w[s][m][n]; one float4 per thread (n % 4 == 0), 8
// slices' loads in flight before their adds
__global__ __launch_bounds__(256) void gemm_x3_slice_sum_kernel(const float* __restrict__ w, int slices, int m, int n,
                                                                float* __restrict__ c, long long ldc) {
  const long long mn = (long long)m * n;
  const long long i = 4 * (blockIdx.x * (long long)blockDim.x + threadIdx.x);
  if (i >= mn) return;
  f32x4 s{0.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j + 8 <= slices; j += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(w + (j + u) * mn + i);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; j < slices; ++j) s += *(const f32x4*)(w + j * mn + i);
  const long long r = i / n, col = i - r * n;
  *(f32x4*)(c + r * ldc + col) = s;
}

int launch_x3_slice_sum(const float* work, int slices, int m, int n, float* c, long long ldc, hipStream_t s) {
  const long long mn = (long long)m * n;
  const dim3 sg((unsigned)((mn / 4 + 255) / 256));
  hipLaunchKernelGGL(gemm_x3_slice_sum_kernel, sg, dim3(256), 0, s, work, slices, m, n, c, ldc);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

}  // namespace eosv
