// Winograd F(2x2, 3x3) conv, exact-f32 MFMA, one launch per conv (stride 1, pad 1,
// Cin = Cout = C, C % 64 == 0): the plain 3x3 convs of an f32 inference handle, and (opt-in) the
// forward and the input gradient of those convs in the training step (eosv/train.py).
//
// Y = A^T [ sum_c (G g G^T) . (B^T d B) ] A per 2x2 output tile: 16 multiplies per channel pair
// where the direct form uses 36.  U = G g G^T comes from the host (eosv_wino_weights_f32, load
// time: inference) or from wino_weights_kernel below (eosv_wino_weights_f32_device, every step:
// training, also of the rotated and transposed weights of the input gradient); V = B^T d B and the
// output transform never leave the CU.
//
// Workgroup = 64 tiles x 64 output channels, 8 waves.  Tiles are indexed flat over
// N x ceil(H/2) x ceil(W/2), so a workgroup may straddle frames and the last one is ragged.  Wave w
// owns transform positions 2w, 2w + 1 for the whole 64 x 64 block: per position a 64 x 64 x C GEMM,
// M[pos][tile][cout] = sum_c V[pos][c][tile] U[pos][c][cout], as 2 x 2 accumulators of
// v_mfma_f32_32x32x2_f32 (128 accumulator registers per lane).
//
// K loop in chunks of 8 channels, one barrier per chunk, both images double-buffered:
//   U slab [16][8][64]  32 KB, contiguous in HBM (wino_u_index), by LDS-DMA (4 x 1 KiB per wave);
//   V image [16][8][64] 32 KB: thread (tile, channel) loads its 4 x 4 patch (out-of-image taps
//     and tiles past the end read nothing and count as zero), does B^T d B in registers (32 adds)
//     and writes 16 words.  Row (pos, c) is rotated by 4c tiles: the 32 lanes of a write group
//     (4 tiles x 8 channels) and of an operand read (32 tiles of one channel) each cover 32 banks.
//   The patch of chunk k + 3 is loaded and that of chunk k + 1 transformed between the MFMA groups
//   of chunk k (see the K loop): two register sets of patches, each load has two chunks to land.
// 256 MFMAs per chunk and CU = 4,096 cycles against 64 KB of fill.
//
// Output transform: the 16 positions of a tile live in 8 waves, so M goes through LDS (the ring,
// free by then) in two halves of 32 tiles x 64 channels x 16 positions = 128 KB; thread
// (tile, 4 channels) then reads 16 float4, applies A^T M A, bias, residual and ReLU in the order of
// the direct kernels ((acc + bias) + res, max 0) and stores float4 rows; outputs outside the image
// (odd H or W) and tiles past the end are not stored.
//
// Every output has one fixed summation order (channels ascending, no split-K, no atomics), the
// same wherever its tile sits in a workgroup: results do not depend on the batch or the grid.
#include <type_traits>

#include "common.h"

namespace eosv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {
constexpr int WT = 64;            // tiles per workgroup
constexpr int WC = 64;            // output channels per workgroup
constexpr int WK = 8;             // channels per K chunk
constexpr int IMG = 16 * WK * 64;  // floats of one V or U image
}  // namespace

__global__ __launch_bounds__(512) void conv_wino_f32_kernel(WinoArgs a) {
  // V0 | V1 | U0 | U1, then the output transform's M halves
  __shared__ __attribute__((aligned(16))) float smem[4 * IMG];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, C = a.C;
  const int TH = (H + 1) >> 1, TW = (W + 1) >> 1;
  const long long T = (long long)a.N * TH * TW;
  const int ncb = C / WC;
  const int nmt = (int)((T + WT - 1) / WT);
  const int bt = xcd_tile(blockIdx.x, gridDim.x, a.xcd);
  // C >= 512: channel-block major, so the workgroups resident together walk the same U slabs
  // (U of 512 channels is 16.8 MB, one channel block of it 2.1 MB against 4 MB of L2 per XCD)
  const int mt = a.cbmajor ? bt % nmt : bt / ncb;
  const int cb = a.cbmajor ? bt / nmt : bt % ncb;
  const float* __restrict__ x = a.x;

  // ---- input patch of this thread: tile lt of the group, channel lc of the chunk.  Addresses are
  // a wave-uniform buffer resource on x at the first frame of the workgroup's tile group, a scalar
  // offset kc * WK per chunk and a 32-bit byte offset per tap (buffer loads: no 64-bit address
  // arithmetic per lane): a group's 64 tiles span at most 65 frames, whose bytes the launcher
  // checks against 32 bits.
  const int lt = tid >> 3, lc = tid & 7;
  const int n0 = (int)(((long long)mt * WT) / (TH * TW));  // < N: the group's first tile exists
  const long long xrem = ((long long)a.N - n0) * H * W * C * 4;  // bytes of x from that frame on
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(x + (long long)n0 * H * W * C), (short)0, (int)(xrem > 0xffffffffLL ? 0xffffffffLL : xrem), 0x00020000);
  unsigned xoff = 0;
  unsigned mask = 0;  // bit 4a + b: patch pixel (a, b) is inside the image
  {
    const long long t = (long long)mt * WT + lt;
    if (t < T) {
      const int n = (int)(t / (TH * TW));
      const int rem = (int)(t - (long long)n * (TH * TW));
      const int th = rem / TW, tw = rem - th * TW;
      const int ih0 = 2 * th - 1, iw0 = 2 * tw - 1;
      // (wraps for ih0 or iw0 = -1; only in-image taps, whose sums do not, use it)
      xoff = (unsigned)(((((long long)(n - n0) * H + ih0) * W + iw0) * C + lc) * 4);
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((unsigned)(ih0 + p) < (unsigned)H && (unsigned)(iw0 + q) < (unsigned)W) mask |= 1u << (4 * p + q);
    }
  }
  const int vrot = (lt + 4 * lc) & 63;
  // d: the raw patches in flight, chunk j's in set j & 1 (chunk j + 2 is loaded into a set once the
  // row stage of chunk j has read it); t: the row stage of the next chunk
  float d[2][16], t[16];
  auto load_rows = [&](float* ds, int kc, int p0) {  // patch rows p0, p0 + 1 of chunk kc
#pragma unroll
    for (int p = p0; p < p0 + 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // an out-of-image tap loads the thread's channel of the group's first pixel instead (always
        // inside x); the row stage drops it: 16 unconditional loads, no branch per tap, no wait here
        const bool in = (mask >> (4 * p + q)) & 1;
        const unsigned o = in ? xoff + (unsigned)((p * W + q) * C * 4) : (unsigned)(lc * 4);
        ds[4 * p + q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)o, kc * (WK * 4), 0));
      }
  };
  // V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: t = B^T d, then row p of t B
  auto row_stage = [&](float* ds) {
    // pins the first use of the set here: without it hipcc selects a tap of the set a chunk early
    // (to reuse its register), behind a vmcnt(0) that waits for the loads just issued
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(ds[i]));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float z[4];  // column q of the patch, out-of-image taps as zero
#pragma unroll
      for (int p = 0; p < 4; ++p) z[p] = (mask >> (4 * p + q)) & 1 ? ds[4 * p + q] : 0.f;
      t[q] = z[0] - z[2];
      t[4 + q] = z[1] + z[2];
      t[8 + q] = z[2] - z[1];
      t[12 + q] = z[1] - z[3];
    }
  };
  auto store_row = [&](float* Vs, int p) {
    float* dst = Vs + lc * 64 + vrot;
    dst[(4 * p + 0) * (WK * 64)] = t[4 * p] - t[4 * p + 2];
    dst[(4 * p + 1) * (WK * 64)] = t[4 * p + 1] + t[4 * p + 2];
    dst[(4 * p + 2) * (WK * 64)] = t[4 * p + 2] - t[4 * p + 1];
    dst[(4 * p + 3) * (WK * 64)] = t[4 * p + 1] - t[4 * p + 3];
  };
  // U slab (cb, kc): IMG contiguous floats; wave w moves pieces 4w .. 4w + 3 of 1 KiB
  const float* __restrict__ uslab = a.u + (long long)cb * (C / WK) * IMG + (wid * 4) * 256 + lane * 4;
  auto dma_u = [&](int kc, float* Us) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(uslab + (long long)kc * IMG + j * 256),
                                       (__attribute__((address_space(3))) void*)(Us + (wid * 4 + j) * 256), 16, 0, 0);
  };
  // The wait covers the U DMA and every patch load issued before it; the `ahead` patch loads issued
  // after it (the DMA goes first in group 1) stay in flight across the barrier.  The builtin: hipcc
  // then knows which loads have retired (no wider wait of its own at the row stage).
  auto sync_ring = [&](auto ahead) {
    vm_wait<decltype(ahead)::value>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  using std::integral_constant;

  f32x16 acc[2][2][2];  // [position of the wave][tile half][channel half]
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[p][i][j][q] = 0.f;

  const int h = lane >> 5, r = lane & 31;
  const int nk = C / WK;
  // prologue: chunks 0 .. 2 (nk >= 8: C is a multiple of 64)
  load_rows(d[0], 0, 0);
  load_rows(d[0], 0, 2);
  dma_u(0, smem + 2 * IMG);
  row_stage(d[0]);
#pragma unroll
  for (int p = 0; p < 4; ++p) store_row(smem, p);
  load_rows(d[1], 1, 0);
  load_rows(d[1], 1, 2);
  __builtin_amdgcn_sched_barrier(0);  // issue order = the order the counted wait assumes
  load_rows(d[0], 2, 0);
  load_rows(d[0], 2, 2);
  sync_ring(integral_constant<int, 16>{});  // as in the loop: all but chunk 2's patch
  // One K chunk = 8 groups of 4 MFMAs (position p of the wave, channel pair kp).  The VALU and
  // memory work of the next chunks is dealt over the groups, so that it issues under the MFMAs
  // instead of in a phase of its own between the barrier and the first MFMA (both waves of a SIMD
  // are in the same phase, so nothing else would fill the matrix pipe meanwhile):
  //   group 0     row stage of chunk kc + 1 (its patch was loaded during chunk kc - 2)
  //   group 1, 2  U DMA of chunk kc + 1; patch loads of chunk kc + 3 into the set the row stage
  //               has just read, two rows each
  //   group 3..6  column stage and V stores of chunk kc + 1, four positions each
  // and the operands of group g + 1 are read before the MFMAs of group g.  The loop is unrolled by
  // two so that the patch set of a chunk is a compile-time index.  It has no tail guards: past the
  // last chunk the next-chunk work is repeated on chunk nk - 1 (loads inside x and U, V and U
  // images into the slot nobody reads any more), so that the body has no branches and every
  // chunk issues the same loads in the same order -- the counted wait below depends on that.
  auto chunk = [&](int kc, auto par) {
    constexpr int slot = decltype(par)::value;
    float* dn = d[1 - slot];  // the set of chunks kc + 1 and kc + 3
    const float* Vs = smem + slot * IMG + (2 * wid) * (WK * 64);
    const float* Us = smem + (2 + slot) * IMG + (2 * wid) * (WK * 64);
    float* Vn = smem + (1 - slot) * IMG;
    const int k1 = min(kc + 1, nk - 1), k3 = min(kc + 3, nk - 1);
    float a0[2], a1[2], b0[2], b1[2];
    auto read_ops = [&](int g) {
      const int k = 2 * (g & 3) + h;
      const float* vr = Vs + (g >> 2) * (WK * 64) + k * 64;
      const float* ur = Us + (g >> 2) * (WK * 64) + k * 64;
      a0[g & 1] = vr[(r + 4 * k) & 63];
      a1[g & 1] = vr[(r + 32 + 4 * k) & 63];
      b0[g & 1] = ur[r];
      b1[g & 1] = ur[32 + r];
    };
    read_ops(0);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g < 7) read_ops(g + 1);
      if (g == 0) row_stage(dn);
      if (g == 1) {
        dma_u(k1, smem + (3 - slot) * IMG);
        __builtin_amdgcn_sched_barrier(0);  // the DMA issues before the patch loads: vmcnt(16) covers it
      }
      if (g == 1 || g == 2) load_rows(dn, k3, 2 * (g - 1));
      if (g >= 3 && g < 7) store_row(Vn, g - 3);
      const int p = g >> 2, c = g & 1;
      acc[p][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c], b0[c], acc[p][0][0], 0, 0, 0);
      acc[p][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c], b1[c], acc[p][0][1], 0, 0, 0);
      acc[p][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c], b0[c], acc[p][1][0], 0, 0, 0);
      acc[p][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[c], b1[c], acc[p][1][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // all but the 16 newest loads have landed: the next U image (its DMA was issued before those
    // 16) and the patch of chunk kc + 2; the patch of chunk kc + 3 stays in flight.  And every wave
    // is done reading this slot before it is refilled.
    sync_ring(integral_constant<int, 16>{});
  };
  for (int kc = 0; kc < nk; kc += 2) {  // nk is a multiple of 8
    chunk(kc, integral_constant<int, 0>{});
    chunk(kc + 1, integral_constant<int, 1>{});
  }
  vm_wait<0>();  // the repeated loads of the last chunks, before their registers are reused

  // ---- output transform: Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1]
  float* __restrict__ y = a.y;
  const float* __restrict__ res = a.res;
  const int trow = tid >> 4, c4 = tid & 15;
  const int co = cb * WC + c4 * 4;
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bv = *(const f32x4*)(a.bias + co);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // this thread's tile of the half: its four output pixels, and their residual rows loaded now,
    // under the LDS round trip of M
    const long long t = (long long)mt * WT + i * 32 + trow;
    long long o[4];
    bool ok[4];
    f32x4 rv[4];
    {
      const long long tc = t < T ? t : 0;
      const int n = (int)(tc / (TH * TW));
      const int rem = (int)(tc - (long long)n * (TH * TW));
      const int th = rem / TW, tw = rem - th * TW;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int oh = 2 * th + (e >> 1), ow = 2 * tw + (e & 1);
        ok[e] = t < T && oh < H && ow < W;
        o[e] = (((long long)n * H + oh) * W + ow) * C + co;
        rv[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (res && ok[e]) rv[e] = *(const f32x4*)(res + o[e]);
      }
    }
    if (i) __syncthreads();  // the first half has been read
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q)
          smem[(2 * wid + p) * (32 * WC) + ((q & 3) + 8 * (q >> 2) + 4 * h) * WC + j * 32 + r] = acc[p][i][j][q];
    __syncthreads();
    f32x4 m[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) m[p] = *(const f32x4*)(smem + p * (32 * WC) + trow * WC + c4 * 4);
    f32x4 s[8];  // A^T M: rows 0, 1 x columns 0..3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s[q] = (m[q] + m[4 + q]) + m[8 + q];
      s[4 + q] = (m[4 + q] - m[8 + q]) - m[12 + q];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int dy = e >> 1;
      f32x4 v = (e & 1) ? (s[4 * dy + 1] - s[4 * dy + 2]) - s[4 * dy + 3] : (s[4 * dy] + s[4 * dy + 1]) + s[4 * dy + 2];
      v += bv;
      if (res) v += rv[e];
      if (a.relu) {
        v.x = fmaxf(v.x, 0.f);
        v.y = fmaxf(v.y, 0.f);
        v.z = fmaxf(v.z, 0.f);
        v.w = fmaxf(v.w, 0.f);
      }
      if (ok[e]) *(f32x4*)(y + o[e]) = v;
    }
  }
}

bool conv_wino_f32_ok(int C) { return C >= WC && C % WC == 0; }

int launch_conv_wino_f32(const WinoArgs& a0, hipStream_t s) {
  if (!conv_wino_f32_ok(a0.C) || a0.N <= 0 || a0.H <= 0 || a0.W <= 0)
    return set_error("conv_wino_f32: needs C % 64 == 0 and a non-empty input"), EOSV_ERR_UNSUPPORTED;
  const long long T = (long long)a0.N * ((a0.H + 1) / 2) * ((a0.W + 1) / 2);
  const long long nb = ((T + WT - 1) / WT) * (a0.C / WC);
  if (nb > 0x7fffffffLL) return set_error("conv_wino_f32: grid too large"), EOSV_ERR_UNSUPPORTED;
  // the kernel's 32-bit patch offsets: the (at most) 65 frames a workgroup's tiles span
  if (65LL * a0.H * a0.W * a0.C * 4 > 0xffffffffLL)
    return set_error("conv_wino_f32: 65 frames exceed 32-bit byte offsets"), EOSV_ERR_UNSUPPORTED;
  if (a0.plan) return record_launch(a0.plan, nb, 1);  // 128 KB of LDS: one workgroup per CU
  WinoArgs a = a0;
  a.cbmajor = a.C >= 512;
  hipLaunchKernelGGL(conv_wino_f32_kernel, dim3((unsigned)nb), dim3(512), 0, s, a);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

// U = G g G^T on the device, from the trainer's weights w [cout][3][3][cin] (they change every
// step).  One workgroup per U slab (64 output channels x 8 input channels x 16 positions, 32 KB
// contiguous: wino_u_index), thread (i = tid / 64, o = tid % 64) one 3x3 filter.
//   flip 0: U of the conv itself: output channel = cout index, input channel = cin index.
//   flip 1: U of the input-gradient conv w'[ci][kh][kw][co] = w[co][2 - kh][2 - kw][ci]: output
//           channel = cin index, input channel = cout index, tap 8 - t; no flipped copy of w exists.
// The slab's 9 x 8 x 64 weights go through LDS ([tap][i][o], rows padded to 65 words): the global
// reads walk w's innermost axis (flip 0: 8 lanes per 32-byte run of cin, a wave covers eight
// adjacent (cout, tap) rows; flip 1: a wave reads 64 consecutive cin = 256 B), the LDS reads and
// the 16 U stores of a wave walk the 64 output channels (256 B per store).
// Arithmetic: eosv_wino_weights_f32's, in its order (G g by rows, then (G g) G^T, in double, one
// rounding to f32).  G's entries are 0, 1 and +-1/2, every product is exact, so a contracted
// multiply-add rounds as the separate operations do: the result is bitwise the host's.
namespace {
constexpr int GROW = 65;         // LDS words per (tap, i) row of 64 output channels
constexpr int GTAP = 8 * GROW;   // words per tap (= 8 mod 32 banks)
}  // namespace

__global__ __launch_bounds__(512) void wino_weights_kernel(const float* __restrict__ w, int cin, int nchunk, int flip,
                                                           float* __restrict__ u) {
  __shared__ float gs[9 * GTAP];
  const int tid = threadIdx.x;
  const int ob = blockIdx.x / nchunk, kc = blockIdx.x - ob * nchunk;  // U's channel block and K chunk
  const int o0 = ob * 64, i0 = kc * 8;
  // flip 0: 64 x 9 (cout, tap) rows of 8 cin; flip 1: 8 x 9 (cout, tap) rows of 64 cin; the rows
  // are consecutive in w's [cout][tap] order: 4,608 words, 9 per thread
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int e = j * 512 + tid;
    if (flip) {
      const int o = e & 63, r = e >> 6;  // r = 9 i + tap
      const int i = r / 9, tap = r - 9 * i;
      gs[(8 - tap) * GTAP + i * GROW + o] = w[((size_t)i0 * 9 + r) * cin + o0 + o];
    } else {
      const int i = e & 7, r = e >> 3;  // r = 9 o + tap
      const int o = r / 9, tap = r - 9 * o;
      gs[tap * GTAP + i * GROW + o] = w[((size_t)o0 * 9 + r) * cin + i0 + i];
    }
  }
  __syncthreads();
  const int i = tid >> 6, o = tid & 63;
  double gf[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) gf[k] = (double)gs[k * GTAP + i * GROW + o];
  // G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
  constexpr double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  double Gg[4][3];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) Gg[p][c] = G[p][0] * gf[c] + G[p][1] * gf[3 + c] + G[p][2] * gf[6 + c];
  float* dst = u + (size_t)blockIdx.x * IMG + i * 64 + o;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      dst[(4 * p + q) * (WK * 64)] = (float)(Gg[p][0] * G[q][0] + Gg[p][1] * G[q][1] + Gg[p][2] * G[q][2]);
}

}  // namespace eosv

extern "C" int eosv_wino_weights_f32(const float* w_ocihw, const float* alpha_or_null, int cout, int cin,
                                     float* u_out) {
  using namespace eosv;
  if (!w_ocihw || !u_out || cout <= 0 || cin <= 0 || cout % 64 || cin % 8)
    return set_error("eosv_wino_weights_f32: needs cout % 64 == 0 and cin % 8 == 0"), EOSV_ERR_ARG;
  // G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  for (int o = 0; o < cout; ++o) {
    const float al = alpha_or_null ? alpha_or_null[o] : 1.f;
    for (int i = 0; i < cin; ++i) {
      const float* g = w_ocihw + ((size_t)o * cin + i) * 9;
      float gf[9];
      for (int k = 0; k < 9; ++k) gf[k] = alpha_or_null ? g[k] * al : g[k];  // the folded weight, as fold_conv's
      double Gg[4][3];
      for (int p = 0; p < 4; ++p)
        for (int c = 0; c < 3; ++c) Gg[p][c] = G[p][0] * gf[c] + G[p][1] * gf[3 + c] + G[p][2] * gf[6 + c];
      for (int p = 0; p < 4; ++p)
        for (int q = 0; q < 4; ++q)
          u_out[wino_u_index(o, i, 4 * p + q, cin)] =
              (float)(Gg[p][0] * G[q][0] + Gg[p][1] * G[q][1] + Gg[p][2] * G[q][2]);
    }
  }
  return EOSV_OK;
}

extern "C" int eosv_wino_weights_f32_device(const float* d_w_ohwi, int cout, int cin, int flip, float* d_u,
                                            eosv_stream_t stream) {
  using namespace eosv;
  if (!d_w_ohwi || !d_u) return set_error("eosv_wino_weights_f32_device: null pointer"), EOSV_ERR_ARG;
  if (flip != 0 && flip != 1) return set_error("eosv_wino_weights_f32_device: flip must be 0 or 1"), EOSV_ERR_ARG;
  // U's output channels (blocks of 64) and input channels (chunks of 8)
  const int oc = flip ? cin : cout, ic = flip ? cout : cin;
  if (cout <= 0 || cin <= 0 || oc % 64 || ic % 8)
    return set_error(flip ? "eosv_wino_weights_f32_device: flip = 1 needs cin % 64 == 0 and cout % 8 == 0"
                          : "eosv_wino_weights_f32_device: flip = 0 needs cout % 64 == 0 and cin % 8 == 0"),
           EOSV_ERR_ARG;
  const long long nb = (long long)(oc / 64) * (ic / 8);
  if (nb > 0x7fffffffLL) return set_error("eosv_wino_weights_f32_device: grid too large"), EOSV_ERR_ARG;
  hipLaunchKernelGGL(wino_weights_kernel, dim3((unsigned)nb), dim3(512), 0, (hipStream_t)stream, d_w_ohwi, cin,
                     ic / 8, flip, d_u);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

extern "C" int eosv_conv_wino_f32(const float* d_x, const float* d_u, const float* d_bias, const float* d_res,
                                  int relu, float* d_y, int N, int H, int W, int C, eosv_stream_t stream) {
  using namespace eosv;
  if (!d_x || !d_u || !d_y || N <= 0 || H <= 0 || W <= 0 || C <= 0)
    return set_error("eosv_conv_wino_f32: bad argument"), EOSV_ERR_ARG;
  WinoArgs a{};
  a.x = d_x;
  a.u = d_u;
  a.bias = d_bias;
  a.res = d_res;
  a.y = d_y;
  a.N = N;
  a.H = H;
  a.W = W;
  a.C = C;
  a.relu = relu;
  a.xcd = 1;
  return launch_conv_wino_f32(a, (hipStream_t)stream);
}
