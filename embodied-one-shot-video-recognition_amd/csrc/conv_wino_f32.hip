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
// Work item = 64 tiles x 64 output channels, on a workgroup of 8 waves.  Tiles are indexed flat
// over N x ceil(H/2) x ceil(W/2), so an item may straddle frames and the last one is ragged.  Wave w
// owns the position column q = w >> 1 (positions 4 p + q, p = 0 .. 3: the four that the column stage
// of the output transform combines) and the output-channel half j = w & 1, for all 64 tiles: per
// position a 64 x 32 x C GEMM, M[pos][tile][cout] = sum_c V[pos][c][tile] U[pos][c][cout], as two
// accumulators (tile halves) of v_mfma_f32_32x32x2_f32 (128 accumulator registers per lane).
//
// K loop in chunks of 8 channels, one barrier per chunk, both images double-buffered:
//   U slab [16][8][64]  32 KB, contiguous in HBM (wino_u_index), by LDS-DMA (4 x 1 KiB per wave,
//     buffer_load_dwordx4 ... lds through one resource on U: scalar slab offset, see dma_piece);
//   V image [16][2][64][4] 32 KB: thread (tile, channel) loads its 4 x 4 patch (out-of-image taps
//     and tiles past the end are buffer loads beyond the resource's range: they touch no memory
//     and return +0), does B^T d B in registers (32 adds) and writes 16 words.  Channel c = 2 kp + h
//     of the chunk is word kp of [pos][h][tile]: lane (h, r) of an MFMA reads the A operands of all
//     four k-pairs of a tile with one ds_read_b128 (8 A reads per chunk and lane, two addresses);
//     the B operands of a group (two k-pairs of one position) are one ds_read2st64_b32.
//     Plane h is rotated by 4h tiles: the 32 lanes of a write group (4 tiles x 8 channels) cover
//     32 banks, and the 16 lanes of a ds_read_b128 group (16 tiles, distinct mod 16) cover 64.
//   The patch of chunk k + 3 is loaded and that of chunk k + 1 transformed between the MFMAs
//   of chunk k (see the K loop): two register sets of patches, each load has two chunks to land.
//   The chunk's barrier stands ahead of its last MFMA group, and the first operands of chunk k + 1
//   are read behind it, under that group's MFMAs: no chunk starts with an LDS round trip.
// 256 MFMAs per chunk and CU = 4,096 cycles against 64 KB of fill.
//
// Output transform, Y = A^T M A.  The column stage S = A^T M runs on the wave's own accumulators
// (it owns the four positions of a column), so 8 values per (tile, channel) go through LDS and
// not 16: S [8][64 tiles][64 channels] = 128 KB in one pass into the ring, free by then, but
// for U0.  Thread (tile, 4 channels) then reads 8 float4 for each of its two tiles, applies the row
// stage, bias, residual and ReLU in the order of the direct kernels ((acc + bias) + res, max 0) and
// stores float4 rows; outputs outside the image (odd H or W) and tiles past the end are not stored
// (buffer stores beyond the range).  The residual rows of both tiles are loaded into the registers
// the column stage frees, ahead of the S pass and of every store of the item.  Three barriers per
// item outside the K loop: S written, S read, V0 written.
//
// Persistent: min(items, CUs) workgroups (160 KB of LDS: one per CU), workgroup b walks items
// b, b + G, ... in the XCD-aware order a grid of one workgroup per item would have.  The patch
// loads, the row stage and the U DMA run ahead of the MFMAs across item boundaries: the last three
// chunks of an item load the first three patches of the next, its last chunk row-stages the next
// chunk 0 and DMAs the next U slab 0 into U0, which S leaves alone (it takes V0, V1, U1 and a
// fifth image).  Between two K loops a workgroup therefore only runs the output transform, writes
// the V image of chunk 0 from registers and clears its accumulators (four zero-operand MFMAs: the
// matrix pipe is idle there, the vector issue is what the item's fixed part is made of); the next
// item's index arithmetic (multiply-shift divisions, wino_fdiv) runs under the S writes.
// The source waits for an item's output stores nowhere before the kernel's end, and in the built
// code (hipcc) no wait outside the K loop reaches them: the residual rows wait with
// vmcnt(7) and (6), ahead of and between the stores.  Inside the K loop the counted wait of the
// next item's first chunk covers them, a chunk after their issue.
//
// Every output has one fixed summation order (channels ascending, no split-K, no atomics), the
// same wherever its tile sits in a workgroup: results do not depend on the batch or the grid.
#include <type_traits>

#include "common.h"

namespace eosv {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int WT = 64;            // tiles per workgroup
constexpr int WC = 64;            // output channels per workgroup
constexpr int WK = 8;             // channels per K chunk
constexpr int IMG = 16 * WK * 64;  // floats of one V or U image
// a patch byte offset no tap has (65 frames are < 2^32 B and a multiple of 256 B: launcher), and the
// most bytes a patch resource spans: a buffer load at OOB is out of range and returns +0
constexpr unsigned OOB = 0xffffff00u;
}  // namespace

// a - b on two floats by one v_pk_add_f32 with the second operand negated (the same IEEE
// subtraction; hipcc has no packed form for a vector fsub and emits two v_sub_f32).  Outside the
// K loop only: beside the MFMAs a packed add costs more than the two it replaces.
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 r;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// fmaxf(v, 0) of a v that an add produced (so never a signalling NaN): the one v_max_f32 that
// fmaxf ends in.  Across the uniform branch on relu hipcc no longer sees the add and puts a
// canonicalising v_max_f32 v, v, v in front of every maximum.
__device__ __forceinline__ float relu_of_sum(float v) {
  float r;
  asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(v));
  return r;
}
template <typename V>
__device__ __forceinline__ f32x2 pair(const V& v, int e) {
  return f32x2{v[e], v[e + 1]};
}
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) {
  const f32x2 lo = pk_sub(pair(a, 0), pair(b, 0)), hi = pk_sub(pair(a, 2), pair(b, 2));
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}

// WIDE: some tile index needs more than 31 bits (no tensor that fits a device's memory does): the
// tile decode then divides on 64 bits, as the kernel did before it was persistent.
template <bool WIDE>
__global__ __launch_bounds__(512) void conv_wino_f32_kernel(WinoArgs a) {
  // V0 | V1 | U0 | U1 | a fifth image; the output transform's S rows take all but U0, where the
  // next item's first U slab waits meanwhile
  __shared__ __attribute__((aligned(16))) float smem[5 * IMG];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W, C = a.C;
  const int TH = (H + 1) >> 1, TW = (W + 1) >> 1, TT = TH * TW;
  const long long T = (long long)a.N * TT;
  const int ncb = C / WC;
  const int nmt = (int)((T + WT - 1) / WT);
  const int nb = nmt * ncb, G = gridDim.x;
  const float* __restrict__ x = a.x;
  using tidx = std::conditional_t<WIDE, long long, int>;  // a tile index

  // tile t -> frame and tile coordinates, one multiply per division (wino_fdiv)
  auto tile_of = [&](long long t, int& n, int& th, int& tw) {
    int rem;
    if (WIDE) {
      n = (int)(t / TT);
      rem = (int)(t - (long long)n * TT);
    } else {
      n = wino_fdiv((int)t, a.dtt);
      rem = (int)t - n * TT;
    }
    th = wino_fdiv(rem, a.dtw);
    tw = rem - th * TW;
  };

  // ---- a work item (tile group mt, channel block cb) as the K loop sees it.  The input patch of
  // this thread is tile lt of the group, channel lc of the chunk.  Addresses are a wave-uniform
  // buffer resource on x at the first frame of the tile group, a scalar offset kc * WK per chunk
  // and a 32-bit byte offset per tap (buffer loads: no 64-bit address arithmetic per lane): a
  // group's 64 tiles span at most 65 frames, whose bytes the launcher checks against 32 bits.
  const int lt = tid >> 3, lc = tid & 7;
  struct Item {
    __amdgpu_buffer_rsrc_t xr;
    unsigned xoff;
    unsigned mask;  // bit 4a + b: patch pixel (a, b) is inside the image
    int mt, cb;
  };
  auto decode = [&](int w, int tid) {  // tid: see the output transform
    const int lt = tid >> 3, lc = tid & 7;
    Item it;
    const int bt = xcd_tile(w, nb, a.xcd);
    // C >= 512: channel-block major, so the workgroups resident together walk the same U slabs
    // (U of 512 channels is 16.8 MB, one channel block of it 2.1 MB against 4 MB of L2 per XCD)
    if (a.cbmajor) {
      it.cb = wino_fdiv(bt, a.dnmt);
      it.mt = bt - it.cb * nmt;
    } else {
      it.mt = wino_fdiv(bt, a.dncb);
      it.cb = bt - it.mt * ncb;
    }
    const long long t0 = (long long)it.mt * WT;
    int n0, th, tw;
    tile_of(t0, n0, th, tw);  // n0 < N: the group's first tile exists
    const long long xrem = ((long long)a.N - n0) * H * W * C * 4;  // bytes of x from that frame on
    it.xr = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (long long)n0 * H * W * C), (short)0,
                                              (int)(xrem > OOB ? OOB : xrem), 0x00020000);
    it.xoff = 0;
    it.mask = 0;
    const tidx t = (tidx)t0 + lt;
    if (t < (tidx)T) {
      int n;
      tile_of(t, n, th, tw);
      const int ih0 = 2 * th - 1, iw0 = 2 * tw - 1;
      // (wraps for ih0 or iw0 = -1; only in-image taps, whose sums do not, use it)
      it.xoff = ((((unsigned)(n - n0) * H + ih0) * W + iw0) * C + lc) * 4;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((unsigned)(ih0 + p) < (unsigned)H && (unsigned)(iw0 + q) < (unsigned)W) it.mask |= 1u << (4 * p + q);
    }
    return it;
  };
  // this thread's word of a V row [2][64][4] (see store_row)
  const int vword = (lc & 1) * 256 + ((lt + 4 * (lc & 1)) & 63) * 4 + (lc >> 1);
  // d: the raw patches in flight, chunk j's in set j & 1 (chunk j + 2 is loaded into a set once the
  // row stage of chunk j has read it); t: the row stage of the next chunk
  float d[2][16], t[16];
  // The loads run three chunks ahead of the MFMAs and the row stage one, across item boundaries,
  // so the loads keep the item they are in: its resource and the 16 tap offsets, set per item
  // (set_taps) and not per chunk: the loop body then holds the loads alone, as it would for a
  // single item.  The row stage needs nothing of the item: an out-of-image tap, and every tap of
  // a tile past the end, has the offset OOB, beyond the resource's range (num_records is clamped
  // below it), so the buffer load returns +0 for it and touches no memory.
  __amdgpu_buffer_rsrc_t ld_xr;
  unsigned ld_off[16];
  auto set_taps = [&](const Item& it) {
    ld_xr = it.xr;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // 16 unconditional loads, no branch per tap, no wait here
        const bool in = (it.mask >> (4 * p + q)) & 1;
        ld_off[4 * p + q] = in ? it.xoff + (unsigned)((p * W + q) * C * 4) : OOB;
      }
  };
  auto load_row = [&](float* ds, int kc, int p) {  // patch row p of the load item's chunk kc
#pragma unroll
    for (int i = 4 * p; i < 4 * p + 4; ++i)
      ds[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ld_xr, (int)ld_off[i], kc * (WK * 4), 0));
  };
  // V = B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]: t = B^T d, then row p of t B
  auto row_stage = [&](float* ds) {
    // pins the first use of the set here: without it hipcc selects a tap of the set a chunk early
    // (to reuse its register), behind a vmcnt(0) that waits for the loads just issued
#pragma unroll
    for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(ds[i]));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* z = ds + q;  // column q of the patch (out-of-image taps were loaded as +0)
      t[q] = z[0] - z[8];
      t[4 + q] = z[4] + z[8];
      t[8 + q] = z[8] - z[4];
      t[12 + q] = z[4] - z[12];
    }
  };
  auto store_row = [&](float* Vs, int p) {
    float* dst = Vs + vword;
    dst[(4 * p + 0) * (WK * 64)] = t[4 * p] - t[4 * p + 2];
    dst[(4 * p + 1) * (WK * 64)] = t[4 * p + 1] + t[4 * p + 2];
    dst[(4 * p + 2) * (WK * 64)] = t[4 * p + 2] - t[4 * p + 1];
    dst[(4 * p + 3) * (WK * 64)] = t[4 * p + 1] - t[4 * p + 3];
  };
  // U slab (cb, kc): IMG contiguous floats; wave w moves pieces 4w .. 4w + 3 of 1 KiB.
  // U is one buffer of 16 C^2 floats (< 2^32 B: launcher) behind one wave-uniform resource: the
  // slab is a scalar byte offset, the lane's place in the wave's 4 KiB a constant vector offset and
  // the piece the instruction's immediate, so no address is built per chunk (the flat
  // global_load_lds form took five 64-bit vector adds per chunk beside the MFMAs).  The
  // immediate moves the source and the LDS destination alike: one LDS base per slab, not per piece.
  const unsigned ulane = ((wid * 4) * 256 + lane * 4) * 4;
  const __amdgpu_buffer_rsrc_t ur =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.u, (short)0, (int)(16u * C * C * 4u), 0x00020000);
  auto dma_piece = [&](int cb, int kc, float* Us, int j) {
    const unsigned slab = (unsigned)(cb * (C / WK) + kc) * (IMG * 4);  // scalar
    __attribute__((address_space(3))) void* dst = (__attribute__((address_space(3))) void*)(Us + wid * 4 * 256);
    // (the builtin takes a literal offset; j is one after unrolling, and the other cases fold away)
    if (j == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, dst, 16, (int)ulane, (int)slab, 0, 0);
    if (j == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, dst, 16, (int)ulane, (int)slab, 1024, 0);
    if (j == 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, dst, 16, (int)ulane, (int)slab, 2048, 0);
    if (j == 3) __builtin_amdgcn_raw_ptr_buffer_load_lds(ur, dst, 16, (int)ulane, (int)slab, 3072, 0);
  };
  auto dma_u = [&](int cb, int kc, float* Us) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dma_piece(cb, kc, Us, j);
  };
  auto load_patch = [&](float* ds, int kc) {
#pragma unroll
    for (int p = 0; p < 4; ++p) load_row(ds, kc, p);
  };
  // The wait covers the U DMA and every patch load issued before it; the `ahead` patch loads issued
  // after it (the DMA goes in groups 0 .. 3, the loads in 4 .. 7, the barrier ahead of group 7) stay
  // in flight across the barrier.  The builtin: hipcc then knows which loads have retired (no wider wait of its own at the row stage).
  auto sync_ring = [&](auto ahead) {
    vm_wait<decltype(ahead)::value>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  using std::integral_constant;

  f32x16 acc[4][2];  // [position 4 p + q of the wave's column][tile half], the wave's 32 channels

  const int h = lane >> 5, r = lane & 31;
  const int wq = wid >> 1, wj = wid & 1;  // the wave's position column and output-channel half
  // operand reads of a V row: the four k-pairs of tiles r and r + 32, one ds_read_b128 each
  const int va0 = h * 256 + (r + 4 * h) * 4, va1 = h * 256 + ((r + 32 + 4 * h) & 63) * 4;
  const int nk = C / WK;
  // The workgroup walks items w, w + G, ...  `cur` is the item whose K loop runs, `nxt` the one
  // after it (the workgroup's last item: itself, so that whatever is loaded ahead stays inside x
  // and U).  The patch loads and the row stage run three, two and one chunks ahead of the MFMAs
  // and do not stop at an item's end: the last three chunks of an item load chunks 0 .. 2 of the
  // next, and its last chunk row-stages the next chunk 0 and DMAs the next U slab 0 (into U0,
  // which the output transform leaves alone).
  int w = blockIdx.x;
  Item cur = decode(w, tid);
  Item nxt = decode(w + G < nb ? w + G : w, tid);
  // prologue of the first item only: chunks 0 .. 2 (nk >= 8: C is a multiple of 64)
  set_taps(cur);
  load_patch(d[0], 0);
  dma_u(cur.cb, 0, smem + 2 * IMG);
  row_stage(d[0]);
  load_patch(d[1], 1);
  load_patch(d[0], 2);
  // Everything lands here, chunk 2's patch too (once per workgroup).  Entering the item loop with
  // that patch pending, as the K loop's counted wait would allow, made hipcc wait vmcnt(0) in the
  // K loop's preheader of every item, the previous item's output stores included.
  vm_wait<0>();

  // One K chunk = 8 groups of 4 MFMAs: the wave's four positions one after another, two groups
  // each (k-pairs 0, 1 and 2, 3 for both tile halves).  The VALU and
  // memory work of the next chunks is dealt over the groups, so that it issues under the MFMAs
  // instead of in a phase of its own between the barrier and the first MFMA (both waves of a SIMD
  // are in the same phase, so nothing else would fill the matrix pipe meanwhile).  The two waves
  // of a SIMD share its vector issue and are in the same group at the same time, so the deal
  // spreads the memory instructions: no group holds more than one DMA piece or four loads, and
  // inside a group they stand behind its MFMAs, a quarter behind each (the A/B of the deals):
  //   group 0     row stage of chunk kc + 1 (its patch was loaded during chunk kc - 2)
  //   group 0..3  one piece of the U DMA of chunk kc + 1 each
  //   group 1..4  column stage and V stores of chunk kc + 1, four positions each
  //   group 4..7  patch loads of chunk kc + 3 into the set the row stage has read, one row each
  // All four DMA pieces precede the 16 loads, which the counted wait ahead of group 7 needs.
  // The B operands of group g + 1 are read before the MFMAs of group g, the A operands of a
  // position (two ds_read_b128) two groups ahead of its first MFMA: two positions' A operands are
  // live at a time, 16 registers.  The operands of the next chunk's group 0 are read behind this
  // chunk's barrier, under the MFMAs of group 7 (the item's top reads those of chunk 0; the last
  // chunk's read ahead lands nowhere: chunk 0 of the next item is read again).  The loop is unrolled by
  // two so that the patch set of a chunk is a compile-time index.  Chunks nk, nk + 1, nk + 2 are
  // chunks 0, 1, 2 of `nxt`: the chunk index and the U slab wrap by scalar selects, the loads
  // move on to nxt in chunk nk - 3 (odd: one uniform branch around register moves in the odd
  // chunk, none around a load).  So the body has no tail guards and every chunk issues the same
  // loads in the same order -- the counted wait depends on that.  The V image the last
  // chunk writes (the next item's chunk 0, into slot 0) is overwritten by the output transform
  // and written again after it; the U image it fills (U0) is not.
  // [p & 1]: tiles r and r + 32 of position 4 p + q, component kp = channels 2 kp + h
  f32x4 a0[2], a1[2];
  float bb[2][2];  // [g & 1]: the group's two k-pairs of the wave's channel half
  auto read_a0 = [&](const float* Vs, int p) {
    a0[p & 1] = *(const f32x4*)(Vs + 4 * p * (WK * 64) + va0);
    a1[p & 1] = *(const f32x4*)(Vs + 4 * p * (WK * 64) + va1);
  };
  auto read_b0 = [&](const float* Us, int g) {  // words 128 apart: one ds_read2st64_b32
    const float* ur = Us + 4 * (g >> 1) * (WK * 64) + 4 * (g & 1) * 64;
    bb[g & 1][0] = ur[0];
    bb[g & 1][1] = ur[128];
  };
  auto chunk = [&](int kc, auto par) {
    constexpr int slot = decltype(par)::value;
    float* dn = d[1 - slot];  // the set of chunks kc + 1 and kc + 3
    const bool s1 = kc + 1 >= nk, s3 = kc + 3 >= nk;
    const int k1 = s1 ? kc + 1 - nk : kc + 1, k3 = s3 ? kc + 3 - nk : kc + 3;
    const int cb1 = s1 ? nxt.cb : cur.cb;
    float* Un = smem + (3 - slot) * IMG;
    const float* Vs = smem + slot * IMG + wq * (WK * 64);
    const float* Us = smem + (2 + slot) * IMG + wq * (WK * 64) + h * 64 + wj * 32 + r;
    float* Vn = smem + (1 - slot) * IMG;
    auto read_a = [&](int p) { read_a0(Vs, p); };
    auto read_b = [&](int g) { read_b0(Us, g); };
    // (the operands of group 0 were read during the previous chunk's last group, or at the item's top)
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      if (g == 7) {
        // All but the 12 newest loads have landed: the next U image (its DMA was issued before
        // the patch loads of groups 4 .. 6) and the patch of chunk kc + 2; the patch of chunk
        // kc + 3 stays in flight (older output stores of the previous item count as landed loads
        // do: the wait only gets stricter).  The next V image was written in groups 1 .. 4.  And
        // every wave has read all it takes from this slot (the last A operands in group 4, the
        // last B operands ahead of group 6's MFMAs) before the next chunk refills it.  The barrier
        // stands ahead of the last group, not behind it, so that the next chunk's first operands
        // are read under this group's MFMAs and not in front of its own.
        sync_ring(integral_constant<int, 12>{});
        read_a0(smem + (1 - slot) * IMG + wq * (WK * 64), 0);
        read_b0(smem + (3 - slot) * IMG + wq * (WK * 64) + h * 64 + wj * 32 + r, 0);
        __builtin_amdgcn_sched_barrier(0);  // the three reads right behind the barrier: four MFMAs cover them
      }
      if (g == 0) row_stage(dn);
      if (g < 7) read_b(g + 1);
      if (g < 6 && !(g & 1)) read_a((g >> 1) + 1);  // the next position's, two groups ahead
      if (g >= 1 && g < 5) store_row(Vn, g - 1);
      if (g < 4) {
        dma_piece(cb1, k1, Un, g);  // all four ahead of the patch loads: the counted wait covers them
      } else {
        if (g == 4 && slot == 1 && kc + 3 == nk) set_taps(nxt);
        load_row(dn, k3, g - 4);
      }
      // the wave's four positions one after another, two groups each; the two MFMAs of an
      // accumulator stand two instructions apart
      const int p = g >> 1, kp = 2 * (g & 1), c = g & 1;
      acc[p][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[p & 1][kp], bb[c][0], acc[p][0], 0, 0, 0);
      acc[p][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[p & 1][kp], bb[c][0], acc[p][1], 0, 0, 0);
      acc[p][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[p & 1][kp + 1], bb[c][1], acc[p][0], 0, 0, 0);
      acc[p][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[p & 1][kp + 1], bb[c][1], acc[p][1], 0, 0, 0);
      // placed behind the group's MFMAs, a quarter behind each (0x008: an MFMA; 0x096: VALU, SALU,
      // vector memory or LDS), not all ahead of the first
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (g == 0) __builtin_amdgcn_sched_group_barrier(0x096, 12, 0);
        if (g >= 1 && g < 4) __builtin_amdgcn_sched_group_barrier(0x096, 3, 0);
        if (g == 4) __builtin_amdgcn_sched_group_barrier(0x096, 4, 0);  // row, four loads and two A reads
        if (g >= 5) __builtin_amdgcn_sched_group_barrier(0x096, 2, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  float* __restrict__ y = a.y;
  const float* __restrict__ res = a.res;
  for (;;) {
    // V image of chunk 0 from the row stage the previous item's last chunk (or the prologue) left
    // in t; its U image and the patch of chunk 1 landed before that chunk's barrier
#pragma unroll
    for (int p = 0; p < 4; ++p) store_row(smem, p);
    // (the loads' tap offsets are the ones the previous item's chunk nk - 3, or the prologue, set:
    // they stay in their 16 registers through the output transform, which has room for them since
    // it holds S rows and not M halves beside the accumulators)
    // (the accumulators are cleared while those stores drain and the other waves arrive)
    // by the matrix pipe, idle here: one two-block MFMA of zero operands writes the 32 registers
    // of a position (0 * 0 + 0), where 32 v_mov would stand in the vector issue both waves of a
    // SIMD share.  The operand is hidden from the compiler so that the four stay four.
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float z = 0.f;
      asm volatile("" : "+v"(z));
      const f32x32 c = __builtin_amdgcn_mfma_f32_32x32x1f32(z, z, f32x32(0.f), 0, 0, 0);
      acc[p][0] = __builtin_shufflevector(c, c, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
      acc[p][1] = __builtin_shufflevector(c, c, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // the first operands of chunk 0 (every later chunk's are read during the chunk before it)
    read_a0(smem + wq * (WK * 64), 0);
    read_b0(smem + 2 * IMG + wq * (WK * 64) + h * 64 + wj * 32 + r, 0);
    for (int kc = 0; kc < nk; kc += 2) {  // nk is a multiple of 8
      chunk(kc, integral_constant<int, 0>{});
      chunk(kc + 1, integral_constant<int, 1>{});
    }

    // ---- output transform: Y = A^T M A, A^T = [1 1 1 0; 0 1 -1 -1].  t, d[1] and d[0] hold the
    // next item's chunks 0 (row-staged), 1 and 2 (in flight) meanwhile.
    // Its lane constants are derived here, from a thread index rebuilt from the lane count and
    // hidden from the compiler: hoisted out of the item loop they, or tid itself, would stay live
    // across the K loop, which has no room (they were spilled).
    int te;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(te));
    te += wid * 64;
    const int trow = te >> 4, c4 = te & 15, he = (te >> 5) & 1, re = te & 31;
    const int we = __builtin_amdgcn_readfirstlane(te >> 6);
    const int qe = we >> 1, je = we & 1;
    const int mt = cur.mt;
    const int co = cur.cb * WC + c4 * 4;
    w += G;
    const bool more = w < nb;
    cur = nxt;
    // Column stage, S = A^T M, on the wave's own accumulators: it owns the four positions 4 p + q
    // that a column combines.  In place: row 0 of S takes the registers of position 0, row 1 those
    // of position 3; positions 1 and 2 are free from here on.
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      acc[0][i] = (acc[0][i] + acc[1][i]) + acc[2][i];
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const f32x2 d = pk_sub(pk_sub(pair(acc[1][i], e), pair(acc[2][i], e)), pair(acc[3][i], e));
        acc[3][i][e] = d.x;
        acc[3][i][e + 1] = d.y;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (a.bias) bv = *(const f32x4*)(a.bias + co);
    // y and the residual through buffer resources at the item's first frame, as x (32-bit byte
    // offsets over the item's frames); no residual: an empty resource, every load returns zeros
    int n0, th0, tw0;
    tile_of((long long)mt * WT, n0, th0, tw0);
    const long long fbytes = (long long)H * W * C * 4, yrem = ((long long)a.N - n0) * fbytes;
    const int yrec = (int)(yrem > OOB ? OOB : yrem);
    const __amdgpu_buffer_rsrc_t yr =
        __builtin_amdgcn_make_buffer_rsrc((void*)((char*)y + n0 * fbytes), (short)0, yrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(res ? (const char*)res + n0 * fbytes : (const char*)nullptr), (short)0, res ? yrec : 0, 0x00020000);
    // this thread's two tiles (trow and trow + 32 of the item): their four output pixels each, and
    // the residual rows of both, loaded into the registers the column stage freed: ahead of the
    // barrier, the reads of S and every store of the item, so no row waits behind a store.  Pixels
    // outside the image (odd H or W) and tiles past the end get the offset OOB: their residual
    // loads return zeros, their stores are dropped, and neither takes a branch.
    unsigned o[2][4];
    f32x4 rv[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const tidx tl = (tidx)mt * WT + k * 32 + trow;
      const bool tok = tl < (tidx)T;
      int n, th, tw;
      tile_of(tok ? tl : 0, n, th, tw);
      // the tile's first pixel; 32-bit arithmetic, as the patch offsets (launcher: 65 frames fit)
      const unsigned o0 = ((((unsigned)(n - n0) * H + 2 * th) * W + 2 * tw) * C + co) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = tok && 2 * th + (e >> 1) < H && 2 * tw + (e & 1) < W;
        o[k][e] = ok ? o0 + (unsigned)(((e >> 1) * W + (e & 1)) * C * 4) : OOB;
        rv[k][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)o[k][e], 0, 0));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // S [8][64 tiles][64 channels], 128 KB in one pass: rows 4 dy + q, row half dy = 0 in V0 | V1,
    // dy = 1 in U1 | the fifth image (U0 keeps the next item's slab)
    {
      float* s0 = smem + qe * (WT * WC) + (4 * he) * WC + je * 32 + re;
      float* s1 = s0 + IMG + 4 * (WT * WC);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = i * 32 + (e & 3) + 8 * (e >> 2);
          s0[row * WC] = acc[0][i][e];
          s1[row * WC] = acc[3][i][e];
        }
    }
    // the item after the next: its index arithmetic runs while the LDS writes drain
    nxt = decode(w + G < nb ? w + G : w < nb ? w : w - G, te);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // row stage, thread (tile, 4 channels): the 8 float4 of each of its two tiles
    f32x4 s[2][8];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        s[k][i] = *(const f32x4*)(smem + (i >= 4 ? IMG : 0) + i * (WT * WC) + (k * 32 + trow) * WC + c4 * 4);
    // S has been read: the next item's V image may be written
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int dy = e >> 1;
        const f32x4* sr = s[k] + 4 * dy;
        f32x4 v = (e & 1) ? sub4(sub4(sr[1], sr[2]), sr[3]) : (sr[0] + sr[1]) + sr[2];
        v += bv;
        // no residual: the rows are -0, and v + -0 is v bit for bit (a select on the row and not on
        // the sum: the sum stays the result of an add, which the maximum need not canonicalise)
        v += res ? rv[k][e] : f32x4(-0.f);
        if (a.relu) {
          v.x = relu_of_sum(v.x);
          v.y = relu_of_sum(v.y);
          v.z = relu_of_sum(v.z);
          v.w = relu_of_sum(v.w);
        }
        // not waited for: only the kernel's end is
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yr, (int)o[k][e], 0, 0);
      }
    if (!more) break;
  }
  vm_wait<0>();  // the loads and the U DMA issued past the last item: nothing may land after the end
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
  // the U DMA's buffer resource and scalar slab offsets: 16 C^2 floats within 32 bits of bytes
  if (16LL * a0.C * a0.C * 4 >= 0x100000000LL)
    return set_error("conv_wino_f32: U exceeds 32-bit byte offsets"), EOSV_ERR_UNSUPPORTED;
  if (a0.plan) return record_launch(a0.plan, nb, 1);  // nb items, one workgroup per CU at a time
  WinoArgs a = a0;
  a.cbmajor = a.C >= 512;
  const int TW = (a.W + 1) / 2, TT = ((a.H + 1) / 2) * TW;
  a.dtt = wino_div(TT);
  a.dtw = wino_div(TW);
  a.dncb = wino_div(a.C / WC);
  a.dnmt = wino_div((unsigned)((T + WT - 1) / WT));
  // a tile index (they run up to the end of the last group) needs more than 31 bits: 64-bit division
  const bool wide = T + 2 * WT > 0x7fffffffLL;
  // persistent: one workgroup per CU (160 KB of LDS) walks items b, b + G, ...
  const long long G = std::min<long long>(nb, a.max_wg > 0 ? a.max_wg : device_cu_count());
  if (wide)
    hipLaunchKernelGGL(conv_wino_f32_kernel<true>, dim3((unsigned)G), dim3(512), 0, s, a);
  else
    hipLaunchKernelGGL(conv_wino_f32_kernel<false>, dim3((unsigned)G), dim3(512), 0, s, a);
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

namespace eosv {
static int conv_wino_f32_entry(const float* d_x, const float* d_u, const float* d_bias, const float* d_res, int relu,
                               float* d_y, int N, int H, int W, int C, int max_wg, eosv_stream_t stream) {
  if (!d_x || !d_u || !d_y || N <= 0 || H <= 0 || W <= 0 || C <= 0)
    return set_error("eosv_conv_wino_f32: bad argument"), EOSV_ERR_ARG;
  WinoArgs a{};
  a.max_wg = max_wg;
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
}  // namespace eosv

extern "C" int eosv_conv_wino_f32(const float* d_x, const float* d_u, const float* d_bias, const float* d_res,
                                  int relu, float* d_y, int N, int H, int W, int C, eosv_stream_t stream) {
  return eosv::conv_wino_f32_entry(d_x, d_u, d_bias, d_res, relu, d_y, N, H, W, C, 0, stream);
}

extern "C" int eosv_conv_wino_f32_grid(const float* d_x, const float* d_u, const float* d_bias, const float* d_res,
                                       int relu, float* d_y, int N, int H, int W, int C, eosv_stream_t stream,
                                       int max_workgroups) {
  if (max_workgroups <= 0)
    return eosv::set_error("eosv_conv_wino_f32_grid: max_workgroups must be positive"), EOSV_ERR_ARG;
  return eosv::conv_wino_f32_entry(d_x, d_u, d_bias, d_res, relu, d_y, N, H, W, C, max_workgroups, stream);
}
