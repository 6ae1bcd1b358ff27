// Weight gradient of the stride-1 pad-1 3x3 convs with Cin = Cout = C (C % 64 == 0) in the Winograd
// F(2x2, 3x3) domain, exact-f32 MFMA (training path: the conv part of loss.backward(), reference
// network_train.py:114; opt-in, NativeTrainer(winograd_wgrad=...)).  The transforms are those of
// conv_wino_f32.hip:
//
//   dU[pos][co][ci] = sum over tiles t of dM[pos][t][co] * V[pos][t][ci]    16 GEMMs C x C x tiles
//   V  = B^T d B      d: the 4 x 4 input patch of tile t (zero outside the image)
//   dM = A dY_t A^T   dY_t: the 2 x 2 output-gradient tile (zero outside the image and past the end)
//   dg[co][ci] = G^T dU[.][co][ci] G                                        4 x 4 -> 3 x 3
//
// 16 multiplies per tile and channel pair where the direct form (wgrad_f32.hip) uses 36.  Tiles are
// indexed flat over N x ceil(H/2) x ceil(W/2), as in the forward.
//
// conv_wgrad_wino_f32_kernel: a workgroup owns a 64 co x 64 ci block of all 16 positions over one
// slice of tiles; 8 waves, wave w owns positions 2w, 2w + 1 as 2 x 2 accumulators of
// v_mfma_f32_32x32x2_f32 (A = dM, B = V, the tile is the reduction index; 128 accumulator registers,
// 128 KB of LDS: one workgroup per CU).  The reduction runs in chunks of 8 tiles, one barrier per
// chunk, both images double-buffered:
//   V image [16][8 tiles][64 ci], dM image [16][8 tiles][64 co], 32 KB each.
// Wave w stages tile w of the chunk, lane l channel l of the block: the tile's decode, its taps'
// offsets and its in-image mask are wave-uniform (scalar), the 16 patch loads and 4 dY loads are
// 256 B runs across the lanes, and the 32 LDS writes are 64 consecutive words each.  The operand
// reads are 32 consecutive words per half-wave.  So neither side needs a row rotation: every LDS
// access covers 32 distinct banks with consecutive words.  Out-of-image taps and
// outputs load the block's first word instead and are dropped by a select: no branch per tap.
// The loads of chunk k + 2 are issued and chunk k + 1 is transformed between the MFMA groups of
// chunk k (two register sets, so a load has a whole chunk to land).
//
// Grid: (C / 64)^2 blocks x S slices, S chosen so that one round of workgroups fills the chip.
// Each slice applies G^T . G to its partial dU in the epilogue (f32, one fixed order) and writes
// 9 C^2 words in dW's layout to the workspace [S][C][3][3][C]; conv_wgrad_wino_sum_kernel sums the
// slices in a fixed order into dW.  (First form: raw dU partials, 16 C^2 words per slice, transformed
// by the second kernel; the workspace round trip, 67 MB each way at every stage of the training
// batch, was 40 of 140 us per call.)  No atomics: one fixed summation order per output for a given
// (N, H, W, C) and workspace size.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace eosv {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GB = 64;              // channels per block side
constexpr int GT = 8;               // tiles per chunk
constexpr int GIMG = 16 * GT * GB;  // floats of one V or dM image
constexpr int GMINCH = 4;           // chunks a slice holds at least (the 144 KB epilogue per workgroup)

struct WgradWinoArgs {
  const float* x;   // [N][H][W][C]
  const float* dy;  // [N][H][W][C]
  float* part;      // [slices][C][3][3][C]
  int N, H, W, C;
  unsigned T;                // tiles
  unsigned tiles_per_slice;  // % GT == 0
  unsigned xbytes;           // of x and of dy
};

__global__ __launch_bounds__(512) void conv_wgrad_wino_f32_kernel(WgradWinoArgs a) {
  // V0 | V1 | dM0 | dM1
  __shared__ __attribute__((aligned(16))) float smem[4 * GIMG];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, C = a.C;
  const unsigned TW = (unsigned)(W + 1) >> 1, THW = ((unsigned)(H + 1) >> 1) * TW;
  const int ncb = C / GB;
  // block -> (slice, co block, ci block): the blocks of a slice are neighbours, they read the
  // same tiles
  int b = blockIdx.x;
  const int cib = b % ncb;
  b /= ncb;
  const int cob = b % ncb;
  const unsigned slice = (unsigned)(b / ncb);
  const unsigned t0 = slice * a.tiles_per_slice;
  const unsigned t1 = min(a.T, t0 + a.tiles_per_slice);
  const int nk = (int)((t1 - t0 + GT - 1) / GT);

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)a.xbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yr =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, (short)0, (int)a.xbytes, 0x00020000);
  const int xvo = (cib * GB + lane) * 4, yvo = (cob * GB + lane) * 4;  // this lane's channel, bytes

  // d: raw patch (16) and dY tile (4) in flight, chunk j's in set j & 1; msk: bit 4p + q patch
  // pixel (p, q) is inside the image, bit 16 + 2a + b output (a, b) is (0 for a tile past the end)
  float d[2][20];
  unsigned msk[2];
  auto load_tile = [&](float* ds, unsigned& m, int kc) {
    const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)(t0 + (unsigned)kc * GT + (unsigned)wid));
    // all of this is wave-uniform (scalar) and free of branches; a tile past the end decodes as
    // the slice's first and gets an empty mask
    const unsigned tc = t < t1 ? t : t0;
    const unsigned n = tc / THW, rem = tc - n * THW;
    const unsigned th = rem / TW, tw = rem - th * TW;
    const int ih0 = 2 * (int)th - 1, iw0 = 2 * (int)tw - 1;
    const int pix0 = ((int)n * H + ih0) * W + iw0;  // may be negative; only in-image taps use it
    unsigned cols = 0, mm = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) cols |= (unsigned)((unsigned)(iw0 + q) < (unsigned)W) << q;
#pragma unroll
    for (int p = 0; p < 4; ++p) mm |= (0u - (unsigned)((unsigned)(ih0 + p) < (unsigned)H) & cols) << (4 * p);
    // output (a, b) is patch pixel (a + 1, b + 1)
    mm |= ((mm >> 5) & 3u) << 16 | ((mm >> 9) & 3u) << 18;
    mm = t < t1 ? mm : 0u;
    m = mm;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool in = (mm >> (4 * p + q)) & 1;
        const unsigned so = in ? (unsigned)(pix0 + p * W + q) * (unsigned)(C * 4) : 0u;
        ds[4 * p + q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, xvo, (int)so, 0));
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = (mm >> (16 + e)) & 1;
      const unsigned so = in ? (unsigned)(pix0 + ((e >> 1) + 1) * W + (e & 1) + 1) * (unsigned)(C * 4) : 0u;
      ds[16 + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yr, yvo, (int)so, 0));
    }
  };
  // V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: t = B^T d, then row p of t B
  float t[16];
  auto col_stage = [&](const float* ds, unsigned m) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float z[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) z[p] = (m >> (4 * p + q)) & 1 ? ds[4 * p + q] : 0.f;
      t[q] = z[0] - z[2];
      t[4 + q] = z[1] + z[2];
      t[8 + q] = z[2] - z[1];
      t[12 + q] = z[1] - z[3];
    }
  };
  const int lw = wid * GB + lane;  // this thread's word of an image row
  auto store_row = [&](float* Vs, int p) {
    float* dst = Vs + lw;
    dst[(4 * p + 0) * (GT * GB)] = t[4 * p] - t[4 * p + 2];
    dst[(4 * p + 1) * (GT * GB)] = t[4 * p + 1] + t[4 * p + 2];
    dst[(4 * p + 2) * (GT * GB)] = t[4 * p + 2] - t[4 * p + 1];
    dst[(4 * p + 3) * (GT * GB)] = t[4 * p + 1] - t[4 * p + 3];
  };
  // dM = A dY A^T, A = [1 0; 1 1; 1 -1; 0 -1]
  auto store_dm = [&](float* Ms, const float* ds, unsigned m) {
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (m >> (16 + e)) & 1 ? ds[16 + e] : 0.f;
    float s[4][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      s[0][c] = y[c];
      s[1][c] = y[c] + y[2 + c];
      s[2][c] = y[c] - y[2 + c];
      s[3][c] = -y[2 + c];
    }
    float* dst = Ms + lw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dst[(4 * i + 0) * (GT * GB)] = s[i][0];
      dst[(4 * i + 1) * (GT * GB)] = s[i][0] + s[i][1];
      dst[(4 * i + 2) * (GT * GB)] = s[i][0] - s[i][1];
      dst[(4 * i + 3) * (GT * GB)] = -s[i][1];
    }
  };
  using std::integral_constant;

  f32x16 acc[2][2][2];  // [position of the wave][co half][ci half]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[p][i][j][q] = 0.f;

  const int h = lane >> 5, r = lane & 31;
  // prologue: chunk 0 staged, chunk 1 in flight (past the slice's end a tile loads and counts nothing)
  load_tile(d[0], msk[0], 0);
  load_tile(d[1], msk[1], 1);
  col_stage(d[0], msk[0]);
#pragma unroll
  for (int p = 0; p < 4; ++p) store_row(smem, p);
  store_dm(smem + 2 * GIMG, d[0], msk[0]);
  __syncthreads();
  // One chunk = 8 groups of 4 MFMAs (position p of the wave, tile pair kp).  The staging of the next
  // chunks is dealt over the groups so that it issues under the MFMAs:
  //   group 0     loads of chunk kc + 2 into the set the previous chunk has transformed
  //   group 1     column stage of chunk kc + 1
  //   group 2..5  row stage and V stores of chunk kc + 1, four positions each
  //   group 6     dM of chunk kc + 1
  // and the operands of group g + 1 are read before the MFMAs of group g.  Unrolled by two so that
  // the register set of a chunk is a compile-time index.
  auto chunk = [&](int kc, auto par) {
    constexpr int slot = decltype(par)::value;
    float* dn = d[1 - slot];
    const float* Vs = smem + slot * GIMG + (2 * wid) * (GT * GB);
    const float* Ms = smem + (2 + slot) * GIMG + (2 * wid) * (GT * GB);
    float* Vn = smem + (1 - slot) * GIMG;
    float* Mn = smem + (3 - slot) * GIMG;
    float a0[2], a1[2], b0[2], b1[2];
    auto read_ops = [&](int g) {
      const int o = (g >> 2) * (GT * GB) + (2 * (g & 3) + h) * GB + r;
      a0[g & 1] = Ms[o];
      a1[g & 1] = Ms[o + 32];
      b0[g & 1] = Vs[o];
      b1[g & 1] = Vs[o + 32];
    };
    read_ops(0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g < 7) read_ops(g + 1);
      if (g == 0) load_tile(d[slot], msk[slot], kc + 2);
      if (g == 1) col_stage(dn, msk[1 - slot]);
      if (g >= 2 && g < 6) store_row(Vn, g - 2);
      if (g == 6) store_dm(Mn, dn, msk[1 - slot]);
      const int p = g >> 2, c = g & 1;
      acc[p][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c], b0[c], acc[p][0][0], 0, 0, 0);
      acc[p][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c], b1[c], acc[p][0][1], 0, 0, 0);
      acc[p][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c], b0[c], acc[p][1][0], 0, 0, 0);
      acc[p][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c], b1[c], acc[p][1][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the next images are written and every wave is done reading this slot before it is refilled
    __syncthreads();
  };
  for (int kc = 0; kc < nk; kc += 2) {
    chunk(kc, integral_constant<int, 0>{});
    if (kc + 1 < nk) chunk(kc + 1, integral_constant<int, 1>{});
  }

  // ---- epilogue: dg = G^T dU G of this slice's partial sums (the transform is linear, so it
  // commutes with the sum over slices; 9 words leave the CU per channel pair instead of 16).  The 16
  // positions of a channel pair live in 8 waves, so dU goes through LDS (the ring, free by now) in
  // two halves of 16 positions x 32 co x 64 ci = 128 KB.  Lane holds D[m = (q & 3) + 8 (q >> 2) +
  // 4 h][n = r] of accumulator (i, j): co = 32 i + m, ci = 32 j + n.  Thread (co row, 4 ci) then
  // reads 16 float4, applies G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1] by rows, then by
  // columns, and stores 9 float4 in dW's own layout [co][3][3][ci].
  const int trow = tid >> 4, c4 = tid & 15;
  float* __restrict__ o = a.part + ((size_t)slice * C + (size_t)cob * GB) * 9 * C + (size_t)cib * GB + c4 * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (i) __syncthreads();  // the first half has been read
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q)
          smem[(2 * wid + p) * (32 * GB) + ((q & 3) + 8 * (q >> 2) + 4 * h) * GB + j * 32 + r] = acc[p][i][j][q];
    __syncthreads();
    f32x4 rw[3][4];  // G^T dU: row kh, column q
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 u0 = *(const f32x4*)(smem + (q) * (32 * GB) + trow * GB + c4 * 4);
      const f32x4 u1 = *(const f32x4*)(smem + (4 + q) * (32 * GB) + trow * GB + c4 * 4);
      const f32x4 u2 = *(const f32x4*)(smem + (8 + q) * (32 * GB) + trow * GB + c4 * 4);
      const f32x4 u3 = *(const f32x4*)(smem + (12 + q) * (32 * GB) + trow * GB + c4 * 4);
      const f32x4 hs = 0.5f * (u1 + u2);
      rw[0][q] = u0 + hs;
      rw[1][q] = 0.5f * (u1 - u2);
      rw[2][q] = hs + u3;
    }
    float* orow = o + (size_t)(32 * i + trow) * 9 * C;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const f32x4 hs = 0.5f * (rw[kh][1] + rw[kh][2]);
      *(f32x4*)(orow + (size_t)(3 * kh + 0) * C) = rw[kh][0] + hs;
      *(f32x4*)(orow + (size_t)(3 * kh + 1) * C) = 0.5f * (rw[kh][1] - rw[kh][2]);
      *(f32x4*)(orow + (size_t)(3 * kh + 2) * C) = hs + rw[kh][3];
    }
  }
}

// dW[i] = sum over slices of part[slice][i], i over the n = 9 C^2 words of dW.  Workgroup = 64
// words x 4 quarters of the slices: each quarter sums its slices in slice order (256 B runs across a
// wave), the four sums are added in quarter order: one fixed order per output.
__global__ __launch_bounds__(256) void conv_wgrad_wino_sum_kernel(const float* __restrict__ part, int slices,
                                                                  long long n, float* __restrict__ dw) {
  __shared__ float ps[4][64];
  const int e = threadIdx.x & 63, qd = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * 64 + e;  // n % 64 == 0
  const int per = (slices + 3) / 4;
  const int j1 = min(slices, (qd + 1) * per);
  const float* src = part + i;
  float s = 0.f;
  int j = qd * per;
  for (; j + 8 <= j1; j += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = src[(size_t)(j + k) * n];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; j < j1; ++j) s += src[(size_t)j * n];
  ps[qd][e] = s;
  __syncthreads();
  if (qd == 0) dw[i] = ((ps[0][e] + ps[1][e]) + ps[2][e]) + ps[3][e];
}

struct WgradWinoPlan {
  long long T;         // tiles
  long long tps;       // tiles per slice, % GT == 0
  long long slices;
  long long slice_bytes;
};

// slices so that (C / 64)^2 x slices is one workgroup per CU, at least GMINCH chunks each
bool wgrad_wino_plan(int N, int H, int W, int C, WgradWinoPlan* pl) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % GB) return false;
  const long long T = (long long)N * ((H + 1) / 2) * ((W + 1) / 2);
  const long long nblk = (long long)(C / GB) * (C / GB);
  const long long chunks = (T + GT - 1) / GT;
  long long s = (device_cu_count() + nblk - 1) / nblk;
  s = std::max(1LL, std::min(s, chunks / GMINCH));
  long long tps = (T + s - 1) / s;
  tps = (tps + GT - 1) / GT * GT;
  pl->T = T;
  pl->tps = tps;
  pl->slices = (T + tps - 1) / tps;
  pl->slice_bytes = 9LL * C * C * (long long)sizeof(float);
  return true;
}
}  // namespace

}  // namespace eosv

using namespace eosv;

extern "C" {

int64_t eosv_conv_wgrad_wino_f32_workspace(int N, int H, int W, int C) {
  WgradWinoPlan pl;
  if (!wgrad_wino_plan(N, H, W, C, &pl)) return 0;
  // never below 16 C^2 floats, the documented lower bound of the interface
  return std::max(pl.slices * pl.slice_bytes, 16LL * C * C * (long long)sizeof(float));
}

int eosv_conv_wgrad_wino_f32(const float* d_x, const float* d_dy, int N, int H, int W, int C, float* d_dw,
                             float* d_work, int64_t work_bytes, eosv_stream_t stream) {
  WgradWinoPlan pl;
  if (!d_x || !d_dy || !d_dw || !d_work) return set_error("eosv_conv_wgrad_wino_f32: null pointer"), EOSV_ERR_ARG;
  if (!wgrad_wino_plan(N, H, W, C, &pl))
    return set_error("eosv_conv_wgrad_wino_f32: needs N, H, W > 0 and C % 64 == 0, C > 0"), EOSV_ERR_ARG;
  if (work_bytes < pl.slice_bytes)
    return set_error("eosv_conv_wgrad_wino_f32: workspace below one slice (9 C^2 floats)"), EOSV_ERR_ARG;
  // the kernel's 32-bit tile count and byte offsets into x and dy
  const long long xbytes = (long long)N * H * W * C * 4;
  if (xbytes > 0xffffffffLL || pl.T + pl.tps > 0x7fffffffLL)
    return set_error("eosv_conv_wgrad_wino_f32: x exceeds 32-bit byte offsets"), EOSV_ERR_UNSUPPORTED;
  if (work_bytes < pl.slices * pl.slice_bytes) {  // one slice: correct in any workspace that holds it
    pl.slices = 1;
    pl.tps = (pl.T + GT - 1) / GT * GT;
  }
  const long long blocks = pl.slices * (C / GB) * (C / GB);
  if (blocks > 0x7fffffffLL) return set_error("eosv_conv_wgrad_wino_f32: grid too large"), EOSV_ERR_UNSUPPORTED;
  WgradWinoArgs a{};
  a.x = d_x, a.dy = d_dy, a.part = d_work;
  a.N = N, a.H = H, a.W = W, a.C = C;
  a.T = (unsigned)pl.T, a.tiles_per_slice = (unsigned)pl.tps, a.xbytes = (unsigned)xbytes;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(conv_wgrad_wino_f32_kernel, dim3((unsigned)blocks), dim3(512), 0, s, a);
  EOSV_LAUNCH_CHECK();
  const long long n = 9LL * C * C;
  hipLaunchKernelGGL(conv_wgrad_wino_sum_kernel, dim3((unsigned)(n / 64)), dim3(256), 0, s, (const float*)d_work,
                     (int)pl.slices, n, d_dw);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

}  // extern "C"
