// What the bf16 kernels share: the vector types, the bf16 <-> f32 conversions and the 16-B LDS-DMA
// piece that every bf16 file uses, and the LDS-staged epilogue of the implicit-GEMM convs
// (conv_bf16_kernel and the two kernels of conv_bf16_ts.hip).
#pragma once
#include <hip/hip_bf16.h>

#include "common.h"

namespace eosv {

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((unsigned)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __bfloat16_as_ushort(__float2bfloat16(f)); }
// one 16-B-per-lane LDS-DMA piece: the wave's 1 KiB lands linearly from lds_base
__device__ __forceinline__ void dma16(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)lds_base, 16, 0, 0);
}

// When a pass's residual chunks are loaded (each kernel keeps the schedule it was tuned with):
enum ResSched {
  // two register sets, pass i + 1 loaded ahead of pass i's first barrier (pass 0's right after the
  // K loop): the latency overlaps the LDS staging instead of stalling each store
  RES_AHEAD,
  // one set, pass i loaded after its first barrier, under its LDS write (conv_bf16_ts_ws_kernel:
  // two sets spilled at 168 VGPRs)
  RES_ONE_SET
};

// Epilogue of a BM x BN tile of 16x16x32-MFMA accumulators held by WM x WN waves (wave (wm, wn):
// rows wm * BM / WM .., columns wn * BN / WN ..; C/D map: row 4 (lane / 16) + e, column lane % 16):
// v = (acc + bias) + residual, max(v, relu ? 0 : -inf), RNE to bf16; SPLIT (the f32x3 layout:
// pixels stored as (hi, lo) blocks of Cout) adds hi + lo of the residual and stores lo = v - hi.
//
// Staged through LDS (`ep`: the kernel's ring, free by now; WM * 32 rows of BN + 4 f32): pass i
// moves the i-th 32-row M-subtile of every wave, so that the residual loads and output stores are
// 16 B (8 bf16) per lane, whole 128-B lines.  Output and residual go through buffer resources
// based at the tile's first row: rows past M lie beyond num_records and, with NTAIL (Cout no
// multiple of BN), columns past Cout get an out-of-range offset, so such loads return 0 and such
// stores are dropped, without a branch; with no residual its resource has num_records 0.
// Straight-line code lets hipcc count vmcnt exactly; the former per-chunk `if (m < M)` form made
// it wait vmcnt(0) -- for every earlier store -- before each residual use (r01g: the epilogue was
// 5-25 % of a layer).  The barriers are raw: only the LDS staging needs ordering, and a
// __syncthreads() fence would also wait for the residual prefetch and the stores.
// Only the tile's 64 * WM * WN accumulator-holding threads call this (tid below that), all of them.
// (conv_bf16_ws_kernel keeps this epilogue written out: the reason is at the kernel.)
template <int BM, int BN, int WM, int WN, bool SPLIT, bool NTAIL, ResSched RS>
__device__ __forceinline__ void bf16_epilogue(const f32x4 (&acc)[BM / WM / 16][BN / WN / 16], float* ep, u16* y,
                                              const u16* res, const float* bias, const u16* zero, int relu,
                                              int Cout, int M, int m0, int n0, int tid, int wm, int wn) {
  constexpr int NW = WM * WN, TN = BN / WN / 16;
  constexpr int EPR = WM * 32;  // rows per pass
  constexpr int EPS = BN + 4;   // f32 row stride
  constexpr int nthreads = 64 * NW;
  constexpr int NPASS = BM / WM / 32;
  constexpr int IPT = EPR * (BN / 8) / nthreads;  // 16-B output chunks per thread per pass
  static_assert(IPT * nthreads == EPR * (BN / 8), "epilogue work divides evenly");
  constexpr int NRB = RS == RES_ONE_SET ? 1 : 2;  // residual register sets
  const int r = tid & 15, q = (tid & 63) >> 4;
  float bcol[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n0 + wn * (BN / WN) + j * 16 + r;
    bcol[j] = (bias && (!NTAIL || n < Cout)) ? bias[n] : 0.f;
  }
  const long long ostr = SPLIT ? 2LL * Cout : Cout;  // output / residual pixel stride
  const long long tile_bytes = (long long)min(BM, M - m0) * ostr * 2;
  const int nrec = (int)min(tile_bytes, 0x7fffffffLL);
  const __amdgpu_buffer_rsrc_t yr =
      __builtin_amdgcn_make_buffer_rsrc((void*)(y + (long long)m0 * ostr), (short)0, nrec, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(res ? res + (long long)m0 * ostr : zero), (short)0, res ? nrec : 0, 0x00020000);
  v4u rv[NRB][IPT];
  v4u rl[NRB][SPLIT ? IPT : 1];  // SPLIT: the residual's lo block
  auto chunk = [&](int i, int t, int& lrow, int& c8, int& voff) {
    const int idx = tid + t * nthreads;
    lrow = idx / (BN / 8);
    c8 = idx - lrow * (BN / 8);
    const int ml = (lrow >> 5) * (BM / WM) + i * 32 + (lrow & 31);  // row within the tile
    const int n = n0 + c8 * 8;
    voff = (!NTAIL || n < Cout) ? (int)(((long long)ml * ostr + n) * 2) : (int)0x80000000;
  };
  auto load_res = [&](int i) {
#pragma unroll
    for (int t = 0; t < IPT; ++t) {
      int lrow, c8, voff;
      chunk(i, t, lrow, c8, voff);
      rv[i % NRB][t] = __builtin_amdgcn_raw_buffer_load_b128(rr, voff, 0, 0);
      if constexpr (SPLIT) rl[i % NRB][SPLIT ? t : 0] = __builtin_amdgcn_raw_buffer_load_b128(rr, voff + 2 * Cout, 0, 0);
    }
  };
  if constexpr (RS != RES_ONE_SET) load_res(0);
  const float rlow = relu ? 0.f : -INFINITY;  // ReLU as max(v, rlow)
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    if (RS == RES_AHEAD && i + 1 < NPASS) load_res(i + 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (RS == RES_ONE_SET) load_res(i);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int lrow = wm * 32 + t * 16 + 4 * q + e;
          ep[lrow * EPS + wn * (BN / WN) + j * 16 + r] = acc[i * 2 + t][j][e] + bcol[j];
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int t = 0; t < IPT; ++t) {
      int lrow, c8, voff;
      chunk(i, t, lrow, c8, voff);
      const float4 v0 = *(const float4*)(ep + lrow * EPS + c8 * 8);
      const float4 v1 = *(const float4*)(ep + lrow * EPS + c8 * 8 + 4);
      float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const v4u r4 = rv[i % NRB][t];
      const unsigned ru[4] = {r4.x, r4.y, r4.z, r4.w};
      if constexpr (SPLIT) {
        const v4u l4 = rl[i % NRB][SPLIT ? t : 0];
        const unsigned rlo[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // hi + lo is exact in f32
          v[2 * k] += bf2f((u16)(ru[k] & 0xffff)) + bf2f((u16)(rlo[k] & 0xffff));
          v[2 * k + 1] += bf2f((u16)(ru[k] >> 16)) + bf2f((u16)(rlo[k] >> 16));
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[2 * k] += bf2f((u16)(ru[k] & 0xffff));
          v[2 * k + 1] += bf2f((u16)(ru[k] >> 16));
        }
      }
      v4u pk, pl;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float lo = fmaxf(v[2 * k], rlow), hi = fmaxf(v[2 * k + 1], rlow);
        const u16 blo = f2bf(lo), bhi = f2bf(hi);
        pk[k] = (unsigned)blo | ((unsigned)bhi << 16);
        if constexpr (SPLIT)  // residual parts (exact differences)
          pl[k] = (unsigned)f2bf(lo - bf2f(blo)) | ((unsigned)f2bf(hi - bf2f(bhi)) << 16);
      }
      __builtin_amdgcn_raw_buffer_store_b128(pk, yr, voff, 0, 0);
      if constexpr (SPLIT) __builtin_amdgcn_raw_buffer_store_b128(pl, yr, voff + 2 * Cout, 0, 0);
    }
  }
}
}  // namespace

}  // namespace eosv
