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
// kernel: no atomics, bitwise reproducible.  The split, the images, the staging, the MFMA step, the
// tile frame of the conv kernels (X3Tile), the plan and the tile dispatch are in x3_tile.h, which
// conv_x3.hip (the KxK and strided convs) and conv_dgrad_x3.hip (the strided input gradient) share;
// their K loop (X3Tile::k_loop) keeps two sets of the images.  The slice sum is defined here, once.
#include "x3_tile.h"

namespace eosv {

namespace {
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
  double* stats;  // STATS: [row tiles][2][n] column sums and sums of squares of C per row tile
};

// STATS (the forward of eosv_sgemm_x3_stats: NT, alpha 1, beta 0, no addend, one slice): the tile's
// BN batch statistics besides C (x3_tile_stats)
template <int WM, int WN, bool TA, bool TB, bool STATS = false>
__global__ __launch_bounds__(XB_NT) void gemm_x3_kernel(X3Args g) {
  // The tile's constants, accumulators and statistics are X3Tile's; the thread's indices, the loop and the
  // epilogue are written out here: on the X3Tile object (its indices as members, store / mma / each) the
  // NT 64 x 64 instantiation took 84 VGPRs for 80 and paired its LDS writes differently, and the kernel alone
  // ran 1.2-1.4 % slower at m = 4704 (profiles/train_x3_refactor_ab.txt).  One set of the images, two barriers
  // per step: half the LDS of X3Tile::k_loop.
  using Tile = X3Tile<WM, WN>;
  constexpr int BM = Tile::BM, BN = Tile::BN, SUB = Tile::SUB, MI = Tile::MI;
  __shared__ __attribute__((aligned(16))) unsigned char lds[Tile::IMG];
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

  typename Tile::Acc acc;
  Tile::zero(acc);

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
    x3_mma_step<MI>(a_hi, a_lo, b_hi, b_lo, 64 * wm + 16 * MI * sub, 64 * wn, c, q, acc);
    __syncthreads();
  }

  float* out = g.partial ? g.c + (long long)blockIdx.y * g.m * g.n : g.c;
  const long long ldo = g.partial ? g.n : g.ldc;
  // X3Tile::each without the object (the lane's elements: X3Tile::row, col); n is a multiple of the tile's
  // width (x3_channels): no column test
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
  if constexpr (STATS) x3_tile_stats(Tile(), acc, m0, g.m, n0, g.n, tm, lds, g.stats);
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

// the channel counts of ResNet-50's stride-1 1x1 convs
bool x3_channels(int c) { return c == 64 || c == 128 || c == 256 || c == 512 || c == 1024 || c == 2048; }

// what the kernels take, ARG checks done: NT / NN / TN over ResNet-50's channel counts (the two
// dimensions that are channels of the conv), 16-byte aligned operands, leading dimensions % 4
const char* x3_refusal(bool ta, bool tb, int m, int n, int k, const void* a, long long lda, const void* b,
                       long long ldb, const void* c, long long ldc, const void* add) {
  if (ta && tb) return "op(A) = A^T with op(B) = B^T is not a GEMM of a 1x1 conv";
  if (k < 1) return "empty reduction";
  if (!x3_channels(n) || !x3_channels(ta ? m : k)) return "a channel count outside {64, 128, 256, 512, 1024, 2048}";
  if (lda % 4 || ldb % 4 || ldc % 4) return "a leading dimension that is not a multiple of 4";
  if (x3_misaligned({{"a", a}, {"b", b}, {"c", c}, {"add", add}})) return "an operand off 16 bytes";
  return nullptr;
}

int launch_x3(bool ta, bool tb, int m, int n, int k, float alpha, const float* a, long long lda, const float* b,
              long long ldb, float beta, float* c, long long ldc, const float* add, float* work, const X3Plan& p,
              hipStream_t s, double* stats = nullptr) {
  // no entry gets here with both (x3_refusal): the test keeps TA && TB out of the instantiations below
  if (ta && tb) return set_error("eosv_sgemm_x3: no tile"), EOSV_ERR_UNSUPPORTED;
  if ((long long)p.mt * p.nt > 0x7fffffffLL || p.slices > 65535)
    return set_error("eosv_sgemm_x3: grid too large"), EOSV_ERR_UNSUPPORTED;
  X3Args g{};
  g.a = a, g.b = b, g.add = add, g.lda = lda, g.ldb = ldb, g.ldc = ldc;
  g.m = m, g.n = n, g.k = k, g.kps = p.kps, g.nt = p.nt;
  g.alpha = alpha, g.beta = beta;
  g.partial = p.slices > 1;
  g.c = g.partial ? work : c;
  g.stats = stats;
  const dim3 grid((unsigned)(p.mt * p.nt), (unsigned)p.slices), blk(XB_NT);
  x3_dispatch(p, [&](auto wm, auto wn) {
    constexpr int WM = wm(), WN = wn();
    // stats: the NT forward, unsplit, with its epilogue's scale and addends off (the entry sees to it)
    if (stats) hipLaunchKernelGGL((gemm_x3_kernel<WM, WN, false, true, true>), grid, blk, 0, s, g);
    else if (ta) hipLaunchKernelGGL((gemm_x3_kernel<WM, WN, true, false>), grid, blk, 0, s, g);
    else if (tb) hipLaunchKernelGGL((gemm_x3_kernel<WM, WN, false, true>), grid, blk, 0, s, g);
    else hipLaunchKernelGGL((gemm_x3_kernel<WM, WN, false, false>), grid, blk, 0, s, g);
  });
  EOSV_LAUNCH_CHECK();
  if (g.partial) return launch_x3_slice_sum(work, p.slices, m, n, c, ldc, s);
  return EOSV_OK;
}
}  // namespace

int launch_x3_slice_sum(const float* work, int slices, int m, int n, float* c, long long ldc, hipStream_t s) {
  const long long mn = (long long)m * n;
  const dim3 sg((unsigned)((mn / 4 + 255) / 256));
  hipLaunchKernelGGL(gemm_x3_slice_sum_kernel, sg, dim3(256), 0, s, work, slices, m, n, c, ldc);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

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

int eosv_sgemm_x3_stats_chunks(int m, int n, int k) {
  if (m <= 0 || n <= 0 || k <= 0 || !x3_channels(n) || !x3_channels(k)) return 0;
  const X3Plan p = x3_plan(m, n, k, false, 1);
  return (long long)p.mt * p.nt > 0x7fffffffLL ? 0 : p.mt;
}

int eosv_sgemm_x3_stats(int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb, float* d_c, int ldc,
                        double* d_stats, int64_t stats_bytes, eosv_stream_t stream) {
  if (m < 0 || n < 0 || k < 0 || !d_c || !d_stats || (k > 0 && (!d_a || !d_b)) || lda < k || lda <= 0 || ldb < k ||
      ldb <= 0 || ldc < n)
    return set_error("eosv_sgemm_x3_stats: bad argument"), EOSV_ERR_ARG;
  if (m == 0 || n == 0) return EOSV_OK;
  const X3Plan p = x3_plan(m, n, std::max(k, 1), false, 1);
  if (stats_bytes < (int64_t)p.mt * 2 * n * (int64_t)sizeof(double))
    return set_error("eosv_sgemm_x3_stats: d_stats smaller than [row tiles][2][n] doubles"), EOSV_ERR_ARG;
  const char* why = x3_refusal(false, true, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, nullptr);
  if (!why && x3_misaligned({{"d_stats", d_stats}})) why = "d_stats off 16 bytes";
  if (why) return set_error(std::string("eosv_sgemm_x3_stats: ") + why), EOSV_ERR_UNSUPPORTED;
  return launch_x3(false, true, m, n, k, 1.f, d_a, lda, d_b, ldb, 0.f, d_c, ldc, nullptr, nullptr, p,
                   (hipStream_t)stream, d_stats);
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
  const int room = x3_split_room(d_work, work_bytes, eosv_sgemm_x3_tn_splitk_workspace(m, n, k),
                                 (int64_t)m * n * (int64_t)sizeof(float));
  if (!room) return set_error("eosv_sgemm_x3_tn_splitk: workspace smaller than one slice"), EOSV_ERR_ARG;
  if (const char* why = x3_refusal(true, false, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, d_work))
    return set_error(std::string("eosv_sgemm_x3_tn_splitk: ") + why), EOSV_ERR_UNSUPPORTED;
  const X3Plan p = x3_plan(m, n, k, true, room);
  return launch_x3(true, false, m, n, k, 1.f, d_a, lda, d_b, ldb, 0.f, d_c, ldc, nullptr, d_work, p,
                   (hipStream_t)stream);
}

}  // extern "C"
