// f32x3 GEMMs of the training step's stride-1 1x1 convs (opt-in: NativeTrainer(f32x3=...)): f32
// operands and f32 result in memory, the products on bf16 MFMA.  The three GEMMs of such a conv
// (model(video) in train mode and loss.backward(), reference network_train.py:98-116):
//   * forward          Y[P][Cout]     = X[P][Cin] . W[Cout][Cin]^T           (NT)
//   * input gradient   dX[P][Cin]     = dY[P][Cout] . W[Cout][Cin] + addend  (NN)
//   * weight gradient  dW[Cout][Cin]  = dY[P][Cout]^T . X[P][Cin]            (TN, split over P)
//
//   C[m][n] = alpha * sum_k opA(m, k) opB(k, n) + beta * C[m][n] + add[m][n]    (row-major)
//
// Split.  On the way from global memory into LDS every operand element x becomes
//   hi = bf16_rne(x),  lo = bf16_rne(x - float(hi))      (the subtraction is exact in f32)
// so x = hi + lo + rho with |rho| <= 2^-16 |x|, and a product is a_hi b_hi + a_hi b_lo + a_lo b_hi
// on v_mfma_f32_16x16x32_bf16 with f32 accumulation; lo * lo (<= 2^-16 |a||b|) is dropped.  Per
// product the error is at most 3.02 * 2^-16 |a||b|.  A non-finite element, or one that rounds to a
// bf16 infinity, gives NaN or Inf in its row and column of C, as it would poison an f32 GEMM.
//
// One 256-thread workgroup computes a BM x BN tile (2 x 2, 2 x 1, 1 x 2 or 1 x 1 waves of 64 x 64)
// over one slice of the reduction in steps of 32 k.  A step's operands are loaded into registers
// one step ahead (the loads fly while the MFMAs of the current step run), split, and stored into
// four bf16 LDS images [row][32 k] (A hi, A lo, B hi, B lo; 64-byte rows, the four 16-byte chunks
// of a row XORed with 3 in rows 8..15 of every 16 so that each 16-lane group of the ds_read_b128
// fragment reads touches 16 different 16-byte slots).  An operand whose k is the slow index in
// memory (B of NN, both of TN) is transposed in registers on the way in: a thread loads a 4 k x 4
// column block as four float4 and writes four 8-byte runs of 4 k.  The MFMA takes the B fragment
// as its first operand, D = (A B)^T, so a lane holds 4 consecutive n of one m and the epilogue
// stores float4.  Every k is summed in increasing order within a slice; the slices of a split
// reduction write raw partial tiles to a workspace and are summed in slice order by a second
// kernel: no atomics, bitwise reproducible.
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

struct X3Args {
  const float* a;
  const float* b;
  const float* add;  // [m][ldc] addend of the epilogue or nullptr
  float* c;          // C, or the [slices][m][n] partials when partial
  long long lda, ldb, ldc;
  int m, n, k;
  int kps;  // reduction rows per slice (a multiple of XB_K unless one slice)
  int nt;   // tiles along n
  float alpha, beta;
  int partial;  // 1: raw partial sums to c[slice][m][n], no epilogue
};

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

template <int WM, int WN, bool TA, bool TB>
__global__ __launch_bounds__(XB_NT) void gemm_x3_kernel(X3Args g) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  // always 4 waves: a tile of fewer than four 64 x 64 parts deals each part's 4 m-blocks over
  // several waves
  constexpr int SUB = 4 / (WM * WN);   // waves per 64 x 64 part: 1, 2 or 4
  constexpr int MI = 4 / SUB;          // 16-row m-blocks per wave
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * (BM + BN) * XB_ROWB];
  unsigned char* const a_hi = lds;
  unsigned char* const a_lo = lds + BM * XB_ROWB;
  unsigned char* const b_hi = lds + 2 * BM * XB_ROWB;
  unsigned char* const b_lo = b_hi + BN * XB_ROWB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = wave / SUB, sub = wave - SUB * part;
  const int wm = part / WN, wn = part - WN * wm;
  const int tn = blockIdx.x % g.nt, tm = blockIdx.x / g.nt;
  const long long m0 = (long long)tm * BM, n0 = (long long)tn * BN;
  const long long k0 = (long long)blockIdx.y * g.kps;
  const long long k1 = min((long long)g.k, k0 + g.kps);
  const int steps = (int)((k1 - k0 + XB_K - 1) / XB_K);

  Stage<BM, TA> sa;
  Stage<BN, !TB> sb;

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int q = lane >> 4, c = lane & 15;
  if (steps > 0) {
    sa.load(g.a, g.lda, m0, g.m, k0, k1, tid);
    sb.load(g.b, g.ldb, n0, g.n, k0, k1, tid);
  }
  for (int step = 0; step < steps; ++step) {
    sa.store(a_hi, a_lo, tid);
    sb.store(b_hi, b_lo, tid);
    __syncthreads();
    if (step + 1 < steps) {
      const long long kb = k0 + (long long)(step + 1) * XB_K;
      sa.load(g.a, g.lda, m0, g.m, kb, k1, tid);
      sb.load(g.b, g.ldb, n0, g.n, kb, k1, tid);
    }
    bf16x8 bh[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = img_off(64 * wn + 16 * j + c, q);
      bh[j] = *(const bf16x8*)(b_hi + off);
      bl[j] = *(const bf16x8*)(b_lo + off);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int off = img_off(64 * wm + 16 * (MI * sub + i) + c, q);
      const bf16x8 ah = *(const bf16x8*)(a_hi + off);
      const bf16x8 al = *(const bf16x8*)(a_lo + off);
      // D = (A B)^T: rows of D are n.  The two cross terms, then hi * hi
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl[j], ah, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], al, acc[i][j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j], ah, acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // lane holds, of block (i, j), m = m0 + 64 wm + 16 (MI sub + i) + c and n = n0 + 64 wn + 16 j + 4 q + (0..3)
  float* out = g.partial ? g.c + (long long)blockIdx.y * g.m * g.n : g.c;
  const long long ldo = g.partial ? g.n : g.ldc;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const long long m = m0 + 64 * wm + 16 * (MI * sub + i) + c;
    if (m >= g.m) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long n = n0 + 64 * wn + 16 * j + 4 * q;
      f32x4 v = acc[i][j];
      if (!g.partial) {
        v *= g.alpha;
        if (g.beta != 0.f) v += g.beta * *(const f32x4*)(g.c + m * g.ldc + n);
        if (g.add) v += *(const f32x4*)(g.add + m * g.ldc + n);
      }
      *(f32x4*)(out + m * ldo + n) = v;
    }
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

struct X3Plan {
  int wm, wn, mt, nt;
  int slices;  // slices the grid runs
  int cap;     // the slice count the workspace is sized for (>= slices, monotone in k)
  int kps;
};

// the channel counts of ResNet-50's stride-1 1x1 convs
bool x3_channels(int c) { return c == 64 || c == 128 || c == 256 || c == 512 || c == 1024 || c == 2048; }

// tile: 128 x 128 (64 where a dimension is 64); unsplit, halved along m and then along n while the
// grid has fewer than two workgroups per CU; split (TN): slices so that tiles x slices is about
// three workgroups per CU, with at least 256 reduction rows per slice and at most 1024 slices
X3Plan x3_plan(int m, int n, int k, bool split, int max_slices) {
  X3Plan p{};
  p.wm = m > 64 ? 2 : 1;
  p.wn = n > 64 ? 2 : 1;
  auto tiles = [&] {
    p.mt = (m + 64 * p.wm - 1) / (64 * p.wm);
    p.nt = (n + 64 * p.wn - 1) / (64 * p.wn);
    return (long long)p.mt * p.nt;
  };
  if (!split && tiles() < 2 * X3_CUS && p.wm == 2) p.wm = 1;
  if (!split && tiles() < 2 * X3_CUS && p.wn == 2) p.wn = 1;
  const long long t = tiles();
  long long s = 1;
  if (split) {
    s = std::max(1LL, std::min((3LL * X3_CUS + t - 1) / t, (long long)k / 256));
    s = std::min(s, 1024LL);
  }
  p.cap = (int)s;
  s = std::min<long long>(s, std::max(1, max_slices));
  long long kps = (k + s - 1) / s;
  if (s > 1) kps = (kps + XB_K - 1) / XB_K * XB_K;
  p.kps = (int)std::max(1LL, kps);
  p.slices = std::max(1, (int)(((long long)k + p.kps - 1) / p.kps));
  return p;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what the kernels take, ARG checks done: NT / NN / TN over ResNet-50's channel counts (the two
// dimensions that are channels of the conv), 16-byte aligned operands, leading dimensions % 4
const char* x3_refusal(bool ta, bool tb, int m, int n, int k, const void* a, long long lda, const void* b,
                       long long ldb, const void* c, long long ldc, const void* add) {
  if (ta && tb) return "op(A) = A^T with op(B) = B^T is not a GEMM of a 1x1 conv";
  if (k < 1) return "empty reduction";
  if (!x3_channels(n) || !x3_channels(ta ? m : k)) return "a channel count outside {64, 128, 256, 512, 1024, 2048}";
  if (lda % 4 || ldb % 4 || ldc % 4) return "a leading dimension that is not a multiple of 4";
  if (!aligned16(a) || !aligned16(b) || !aligned16(c) || !aligned16(add)) return "an operand off 16 bytes";
  return nullptr;
}

int launch_x3(bool ta, bool tb, int m, int n, int k, float alpha, const float* a, long long lda, const float* b,
              long long ldb, float beta, float* c, long long ldc, const float* add, float* work, const X3Plan& p,
              hipStream_t s) {
  if ((long long)p.mt * p.nt > 0x7fffffffLL || p.slices > 65535)
    return set_error("eosv_sgemm_x3: grid too large"), EOSV_ERR_UNSUPPORTED;
  X3Args g{};
  g.a = a, g.b = b, g.add = add, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.m = m, g.n = n, g.k = k, g.kps = p.kps, g.nt = p.nt;
  g.alpha = alpha, g.beta = beta;
  g.partial = p.slices > 1;
  g.c = g.partial ? work : c;
  const dim3 grid((unsigned)(p.mt * p.nt), (unsigned)p.slices), blk(XB_NT);
  const int sel = (p.wm * 2 + p.wn) * 4 + (ta ? 2 : 0) + (tb ? 1 : 0);
#define EOSV_X3_CASE(WM, WN, TA, TB)                                                 \
  case ((WM * 2 + WN) * 4 + (TA ? 2 : 0) + (TB ? 1 : 0)):                            \
    hipLaunchKernelGGL((gemm_x3_kernel<WM, WN, TA, TB>), grid, blk, 0, s, g);        \
    break;
#define EOSV_X3_TILE(WM, WN) \
  EOSV_X3_CASE(WM, WN, false, false) EOSV_X3_CASE(WM, WN, false, true) EOSV_X3_CASE(WM, WN, true, false)
  switch (sel) {
    EOSV_X3_TILE(1, 1)
    EOSV_X3_TILE(1, 2)
    EOSV_X3_TILE(2, 1)
    EOSV_X3_TILE(2, 2)
    default: return set_error("eosv_sgemm_x3: no tile"), EOSV_ERR_UNSUPPORTED;
  }
#undef EOSV_X3_TILE
#undef EOSV_X3_CASE
  EOSV_LAUNCH_CHECK();
  if (g.partial) {
    const long long mn = (long long)m * n;
    const dim3 sg((unsigned)((mn / 4 + 255) / 256));
    hipLaunchKernelGGL(gemm_x3_slice_sum_kernel, sg, dim3(256), 0, s, work, p.slices, m, n, c, ldc);
    EOSV_LAUNCH_CHECK();
  }
  return EOSV_OK;
}
}  // namespace

}  // namespace eosv

using namespace eosv;

extern "C" {

int eosv_sgemm_x3(int trans_a, int trans_b, int m, int n, int k, float alpha, const float* d_a, int lda,
                  const float* d_b, int ldb, float beta, float* d_c, int ldc, const float* d_add,
                  eosv_stream_t stream) {
  if (m < 0 || n < 0 || k < 0 || !d_c || (k > 0 && (!d_a || !d_b)) || lda <= 0 || ldb <= 0 || ldc < n ||
      lda < (trans_a ? m : k) || ldb < (trans_b ? k : n))
    return set_error("eosv_sgemm_x3: bad argument"), EOSV_ERR_ARG;
  if (m == 0 || n == 0) return EOSV_OK;
  if (const char* why = x3_refusal(trans_a != 0, trans_b != 0, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, d_add))
    return set_error(std::string("eosv_sgemm_x3: ") + why), EOSV_ERR_UNSUPPORTED;
  const X3Plan p = x3_plan(m, n, k, false, 1);
  return launch_x3(trans_a != 0, trans_b != 0, m, n, k, alpha, d_a, lda, d_b, ldb, beta, d_c, ldc, d_add, nullptr, p,
                   (hipStream_t)stream);
}

int64_t eosv_sgemm_x3_tn_splitk_workspace(int m, int n, int k) {
  if (m <= 0 || n <= 0 || k <= 0) return 0;
  const X3Plan p = x3_plan(m, n, k, true, 1024);
  return p.cap > 1 ? (int64_t)p.cap * m * n * (int64_t)sizeof(float) : 0;
}

int eosv_sgemm_x3_tn_splitk(int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb, float* d_c,
                            int ldc, float* d_work, int64_t work_bytes, eosv_stream_t stream) {
  if (m <= 0 || n <= 0 || k <= 0 || !d_a || !d_b || !d_c || lda < m || ldb < n || ldc < n || work_bytes < 0 ||
      (!d_work && work_bytes > 0))
    return set_error("eosv_sgemm_x3_tn_splitk: bad argument"), EOSV_ERR_ARG;
  const int64_t slice_bytes = (int64_t)m * n * (int64_t)sizeof(float);
  // a workspace is given where the plan splits: it must hold one slice at least
  if (d_work && eosv_sgemm_x3_tn_splitk_workspace(m, n, k) > 0 && work_bytes < slice_bytes)
    return set_error("eosv_sgemm_x3_tn_splitk: workspace smaller than one slice"), EOSV_ERR_ARG;
  if (const char* why = x3_refusal(true, false, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, d_work))
    return set_error(std::string("eosv_sgemm_x3_tn_splitk: ") + why), EOSV_ERR_UNSUPPORTED;
  // no workspace: one slice straight into C; a short one: as many slices as it holds
  const int room = d_work ? (int)std::min<int64_t>(work_bytes / slice_bytes, 1024) : 1;
  const X3Plan p = x3_plan(m, n, k, true, room);
  return launch_x3(true, false, m, n, k, 1.f, d_a, lda, d_b, ldb, 0.f, d_c, ldc, nullptr, d_work, p,
                   (hipStream_t)stream);
}

}  // extern "C"
