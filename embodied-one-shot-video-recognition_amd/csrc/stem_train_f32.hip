// The training step's stem, conv 7x7 / 2 pad 3 (3 -> 64), without the im2col buffer: the forward
// z = conv(frames, w) (models.py:19 in train mode, reference network_train.py:99) and the weight
// gradient dW = sum over pixels of dz . x (the stem's part of loss.backward(), network_train.py:114).
// Both read the caller's f32 NCHW frames [N][3][H][W] themselves (W % 4 == 0, W <= 256) and keep
// the input rows in LDS as interleaved RGB rows with real zero borders, the layout of
// stem_pool_f32.hip's DIRECT mode: padded column p = x + 3 at floats 3p .. 3p + 2, a row
// stt_row_floats(W) floats.  Weights are the trainer's [64][7][7][3] = [64][147] dense, read as
// they are (they change every step: no upload layout).  Exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
//
// Forward: one workgroup = one band of stem rows of one image, 4 waves, wave g = output channels
// 16g .. 16g + 15 of every stem column (NT tiles of 16 columns), D = W . X^T with dense
// K = [kh 7][21] + 1 zero = 37 k-steps, the weights in 37 VGPRs.  A step whose 4 k straddle two
// kernel rows selects the row base per lane (stem_pool_f32.hip).  One stem row per step: the two
// input rows the next step adds are loaded into registers before the step's MFMAs (16-byte loads
// of the plane rows) and interleaved into a 9-row ring after them; every stem row and column is
// stored raw, NHWC, 4 consecutive channels (16 B) per lane.
//
// Weight gradient: the pixel is the MFMA reduction index (wgrad_f32.hip): A = dz [pixel][co], one
// 16-byte load per lane straight from HBM (block i of the 4 co-blocks takes co = 4m + i), B = the
// staged input, X[pixel][k] = row 2 oh + kh, float 6 ow + (kw 3 + c), one ds_read_b32 per k-block
// of 16 (147 -> 10 blocks).  A work item is a band of 4 output rows of one image: its 13 input
// rows are staged once and reused by all 49 taps.  The 4 waves are 2 pixel groups (alternate
// quads) x 2 halves of the k-blocks, 64 x 80 accumulators (80 VGPRs) each, kept across all items of
// the workgroup (all 160 k-columns in one wave spilled); at the end pixel group 1 is added to
// group 0 through LDS and the workgroup writes ONE partial dW to the workspace.  At most
// STW_MAX_BLOCKS workgroups (3 per CU on 256 CUs) walk the items, the same number each where the
// items divide; a second kernel sums the partials in a fixed order.  No atomics: bitwise
// reproducible.
#include "common.h"

#include <algorithm>

namespace eosv {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int STT_MAX_W = 256;  // 8 tiles of 16 stem columns; 3 W / 4 <= 192 load units per row
constexpr int STT_K = 147;      // 7 kernel rows x 21 (kw*3 + c)
constexpr int STT_STEPS = 37;   // k-steps of 4 over dense K = 148
constexpr int STT_NT = 256;     // 4 waves
constexpr int STF_RING = 9;     // a step reads rows 2sy .. 2sy + 6 and writes 2sy + 7, 2sy + 8
constexpr int STF_SLACK = 128;  // floats past the ring: reads of columns past the map
constexpr int STW_R = 4;        // output rows per work item
constexpr int STW_ROWS = 2 * STW_R + 5;
constexpr int STW_NBW = 5;      // k-blocks of 16 per wave: 2 x 5 cover 147 -> 160
constexpr int STW_MAX_BLOCKS = 768;  // 3 workgroups per CU on 256 CUs
constexpr int STW_MN = 64 * STT_K;
constexpr int STW_ACC_FLOATS = 2 * 4 * STW_NBW * 4 * 64;  // the accumulators of one pixel group (2 waves)

__host__ __device__ constexpr int stt_row_floats(int W) { return (3 * (W + 6) + 3) & ~3; }

// The input rows are moved in units of 4 columns of one plane row: unit u of a run of rows starting
// at padded row pr0 is (row u / (3 W4), plane, column group); rows outside the image are zeros.
struct RowUnits {
  const float* ximg;
  int H, W, W4, upr;
  __device__ __forceinline__ f32x4 load(int pr0, int u) const {
    const int rr = u / upr, v = u - rr * upr, c = v / W4, j = v - c * W4;
    const int yy = pr0 + rr - 3;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)yy < (unsigned)H) r = *(const f32x4*)(ximg + ((long long)c * H + yy) * W + 4 * j);
    return r;
  }
  // d: the LDS row of unit u's input row
  __device__ __forceinline__ void write(float* d, int u, f32x4 v) const {
    const int w = u % upr, c = w / W4, j = w - c * W4;
    d += 3 * (4 * j + 3) + c;
    d[0] = v[0], d[3] = v[1], d[6] = v[2], d[9] = v[3];
  }
};

// zero the border floats of `rows` LDS rows: padded columns 0 .. 2 and W + 3 .. (the row's end);
// the row fills write the columns between only
__device__ __forceinline__ void zero_borders(float* rows_base, int rows, int RF, int W, int tid) {
  const int right = 3 * (W + 3), npad = 9 + RF - right;
  for (int t = tid; t < rows * npad; t += STT_NT) {
    const int r = t / npad, e = t - npad * r;
    rows_base[r * RF + (e < 9 ? e : right + e - 9)] = 0.f;
  }
}

template <int NT>
__global__ __launch_bounds__(STT_NT, 3) void stem_conv_f32_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ w, float* z, int H, int W,
                                                                 int Hs, int Ws, int bands) {
  extern __shared__ __attribute__((aligned(16))) float stt_smem[];
  float* ring = stt_smem;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6, r16 = lane & 15, q = lane >> 4;
  const int img = blockIdx.x / bands, band = blockIdx.x - bands * img;
  const int rpb = (Hs + bands - 1) / bands;
  const int sy0 = band * rpb, sy1 = min(Hs, sy0 + rpb);
  if (sy0 >= sy1) return;
  const int RF = stt_row_floats(W);
  const RowUnits ru{x + (long long)img * 3 * H * W, H, W, W >> 2, 3 * (W >> 2)};

  // A fragments: w[16g + r16][k = 4s + q], k = 147 is the zero column
  float wa[STT_STEPS];
#pragma unroll
  for (int s = 0; s < STT_STEPS; ++s) {
    const int k = 4 * s + q;
    wa[s] = k < STT_K ? w[(16 * g + r16) * STT_K + k] : 0.f;
  }

  zero_borders(ring, STF_RING, RF, W, tid);
  for (int u = tid; u < 7 * ru.upr; u += STT_NT)
    ru.write(ring + ((2 * sy0 + u / ru.upr) % STF_RING) * RF, u, ru.load(2 * sy0, u));
  __syncthreads();

  const int xoff = 6 * r16 + q;  // tile k, this lane: stem column 16k + r16, float 6 * column of a row
  bool colok[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) colok[k] = 16 * k + r16 < Ws;
  const __amdgpu_buffer_rsrc_t zr =
      __builtin_amdgcn_make_buffer_rsrc(z + (long long)img * Hs * Ws * 64, (short)0, Hs * Ws * 256, 0x00020000);
  const int zvo = r16 * 256 + 4 * (16 * g + 4 * q);  // lane part: its column in the tile, its 4 channels

  const int nu = 2 * ru.upr;  // <= 384: two units per thread at most
  for (int sy = sy0; sy < sy1; ++sy) {
    const bool more = sy + 1 < sy1;
    f32x4 p0 = {0.f, 0.f, 0.f, 0.f}, p1 = p0;
    if (more) {
      if (tid < nu) p0 = ru.load(2 * sy + 7, tid);
      if (tid + STT_NT < nu) p1 = ru.load(2 * sy + 7, tid + STT_NT);
    }
    f32x4 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    int rowb[7];  // ring offsets of input rows 2sy .. 2sy + 6 (wave-uniform)
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) rowb[kh] = ((2 * sy + kh) % STF_RING) * RF;
#pragma unroll
    for (int s = 0; s < STT_STEPS; ++s) {
      // k = 4s + q lies in kernel row kh0 for q < qs, else kh0 + 1; the zero-weight k = 147 stays in
      // row 6 and reads the real element of k = 146 (0 * finite)
      const int kh0 = (4 * s) / 21;
      const int qs = kh0 < 6 ? 21 * (kh0 + 1) - 4 * s : 4;
      const int b0 = rowb[kh0] + 4 * s - 21 * kh0;
      int off = b0;
      if (qs < 4) off = q < qs ? b0 : rowb[kh0 < 6 ? kh0 + 1 : 6] + 4 * s - 21 * (kh0 + 1);
      off += (s == STT_STEPS - 1 && q == 3) ? xoff - 1 : xoff;
#pragma unroll
      for (int k = 0; k < NT; ++k)
        acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], ring[off + 96 * k], acc[k], 0, 0, 0);
    }
    // lane: channels 16g + 4q .. + 3 of stem pixel (sy, 16k + r16)
#pragma unroll
    for (int k = 0; k < NT; ++k)
      if (colok[k]) store_b128_guarded(__builtin_bit_cast(u32x4, acc[k]), zr, zvo, (sy * Ws + 16 * k) * 256);
    if (more) {
      if (tid < nu) ru.write(ring + ((2 * sy + 7 + tid / ru.upr) % STF_RING) * RF, tid, p0);
      if (tid + STT_NT < nu) ru.write(ring + ((2 * sy + 7 + (tid + STT_NT) / ru.upr) % STF_RING) * RF, tid + STT_NT, p1);
    }
    // every wave has read this step's rows and written the next step's two (slots last read a step
    // ago); the stores stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

__global__ __launch_bounds__(STT_NT, 3) void stem_wgrad_f32_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ dz,
                                                                  float* __restrict__ part, int H, int W, int Ho,
                                                                  int Wo, int items, int bpi) {
  extern __shared__ __attribute__((aligned(16))) float stt_smem[];
  float* rows = stt_smem;
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int RF = stt_row_floats(W);
  const int QW = (Wo + 3) >> 2;  // pixel quads per output row

  // waves (pg, kb): pixel quads t = pg, pg + 2, ... and k-blocks 5 kb .. 5 kb + 4
  const int pg = wave >> 1, kb = wave & 1;
  // k-block j, this lane: k = 16 (5 kb + j) + r16 at row kh = k / 21, float k % 21; the 13 columns
  // past 146 read k = 146 (finite) and are not written
  int koff[STW_NBW];
#pragma unroll
  for (int j = 0; j < STW_NBW; ++j) {
    const int k = min(16 * (STW_NBW * kb + j) + r16, STT_K - 1);
    koff[j] = (k / 21) * RF + k % 21;
  }
  f32x4 acc[4][STW_NBW];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < STW_NBW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  zero_borders(rows, STW_ROWS, RF, W, tid);

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int img = item / bpi, oh0 = (item - bpi * img) * STW_R;
    const RowUnits ru{x + (long long)img * 3 * H * W, H, W, W >> 2, 3 * (W >> 2)};
    __syncthreads();  // the previous item's reads are done
    // input rows 2 oh0 - 3 .. + 12 = padded rows 2 oh0 .. 2 oh0 + 12
    for (int u = tid; u < STW_ROWS * ru.upr; u += STT_NT) ru.write(rows + (u / ru.upr) * RF, u, ru.load(2 * oh0, u));
    __syncthreads();
    const float* dzi = dz + ((long long)img * Ho + oh0) * Wo * 64 + 4 * r16;
    const int nrows = min(STW_R, Ho - oh0);
    // Quad (row ohl, columns 4 owq + q) walks the band two quads at a time; (ohl, owq) are
    // wave-uniform.  A of a quad: dz[its pixel][co = 4 r16 .. + 3], loaded two quads ahead and
    // masked (a column past the row: 0) only when used, so no wait follows the load.
    auto advance = [&](int& ohl, int& owq) {
      owq += 2;
      while (owq >= QW) owq -= QW, ++ohl;
    };
    auto load_a = [&](int ohl, int owq) {  // past the band: any valid address, never used
      return *(const f32x4*)(dzi + (min(ohl, nrows - 1) * Wo + min(4 * owq + q, Wo - 1)) * 64);
    };
    int ohl = 0, owq = pg;
    while (owq >= QW) owq -= QW, ++ohl;
    int lh = ohl, lq = owq;
    f32x4 r0 = load_a(lh, lq), r2;
    advance(lh, lq);
    f32x4 r1 = load_a(lh, lq);
    // one quad: refill `fill` for the quad after the next, 20 MFMAs on `use`; false after the last
    auto quad = [&](const f32x4& use, f32x4& fill) {
      advance(lh, lq);
      fill = load_a(lh, lq);
      const int ow = 4 * owq + q;
      const f32x4 a = ow < Wo ? use : f32x4{0.f, 0.f, 0.f, 0.f};
      const float* rb = rows + 2 * ohl * RF + 6 * min(ow, Wo - 1);
      float b[STW_NBW];
#pragma unroll
      for (int j = 0; j < STW_NBW; ++j) b[j] = rb[koff[j]];
#pragma unroll
      for (int j = 0; j < STW_NBW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      advance(ohl, owq);
      return ohl < nrows;
    };
    // the three registers rotate by name (a rotation by moves waits for the load just issued)
    if (ohl < nrows)
      while (quad(r0, r2) && quad(r1, r0) && quad(r2, r1)) {
      }
  }

  // pixel group 1 added to pixel group 0
  float* red = stt_smem + kb * (STW_ACC_FLOATS / 2);  // [i][j][e][lane]
  __syncthreads();
  if (pg == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < STW_NBW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[((i * STW_NBW + j) * 4 + e) * 64 + lane] = acc[i][j][e];
  }
  __syncthreads();
  // lane holds D[m = 4q + e][n = r16] of block (i, j): co = 4m + i, k = 16 (5 kb + j) + n
  if (pg == 0) {
    float* o = part + (long long)blockIdx.x * STW_MN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < STW_NBW; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int co = 4 * (4 * q + e) + i, k = 16 * (STW_NBW * kb + j) + r16;
          if (k < STT_K) o[co * STT_K + k] = acc[i][j][e] + red[((i * STW_NBW + j) * 4 + e) * 64 + lane];
        }
  }
}

// dw[o] = sum of the nb partials: 8 groups of consecutive partials per output summed in order, then
// the 8 group sums in order
__global__ __launch_bounds__(256) void stem_wgrad_sum_kernel(const float* __restrict__ part, int nb,
                                                            float* __restrict__ dw) {
  __shared__ float red[8][32];
  const int o = blockIdx.x * 32 + (threadIdx.x & 31), grp = threadIdx.x >> 5;
  const int chunk = (nb + 7) >> 3;
  const int s0 = grp * chunk, s1 = min(nb, s0 + chunk);
  float s = 0.f;
  for (int i = s0; i < s1; ++i) s += part[(long long)i * STW_MN + o];
  red[grp][threadIdx.x & 31] = s;
  __syncthreads();
  if (grp == 0) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += red[i][threadIdx.x];
    dw[o] = t;
  }
}
static_assert(STW_MN % 32 == 0, "the sum kernel's blocks of 32 outputs cover dW exactly");

template <int NT>
void launch_fwd_nt(const float* x, const float* w, float* z, int N, int H, int W, int Hs, int Ws, hipStream_t s) {
  const size_t lds = (size_t)(STF_RING * stt_row_floats(W) + STF_SLACK) * 4;
  // (the ring is at most 29 KB: registers, not LDS, bound the occupancy, so the first call's holds)
  static const int occ = kernel_occupancy((const void*)stem_conv_f32_kernel<NT>, STT_NT, lds);
  // bands of stem rows per image: the grid fills the chip's slots once, bands of 4 rows at least
  const long long slots = (long long)occ * device_cu_count();
  const int bands = (int)std::max(1LL, std::min<long long>((slots + N - 1) / N, (Hs + 3) / 4));
  hipLaunchKernelGGL((stem_conv_f32_kernel<NT>), dim3((unsigned)(N * bands)), dim3(STT_NT), lds, s, x, w, z, H, W, Hs,
                     Ws, bands);
}

// EOSV_OK, or the status both entries share for (pointers, N, H, W); z_bytes / frames bytes < 2^31
int stem_train_check(const char* fn, bool null_ptr, uintptr_t ptr_bits, int N, int H, int W) {
  if (null_ptr || N <= 0 || H <= 0 || W <= 0) return set_error(std::string(fn) + ": bad argument"), EOSV_ERR_ARG;
  const long long Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  if (W % 4 || W > STT_MAX_W || (ptr_bits & 15) || 12LL * N * H * W >= (1LL << 31) ||
      256LL * N * Ho * Wo >= (1LL << 31))
    return set_error(std::string(fn) + ": needs W % 4 == 0, W <= 256, 16-byte aligned pointers and frames and "
                                       "stem map below 2 GiB each"),
           EOSV_ERR_UNSUPPORTED;
  return EOSV_OK;
}

long long stem_wgrad_items(int N, int H) { return (long long)N * (((H - 1) / 2 + 1 + STW_R - 1) / STW_R); }
// workgroups (= partials): the fewest that walk the items in the same number of rounds as
// STW_MAX_BLOCKS would
int stem_wgrad_blocks(long long items) {
  const long long rounds = (items + STW_MAX_BLOCKS - 1) / STW_MAX_BLOCKS;
  return (int)((items + rounds - 1) / rounds);
}
}  // namespace

}  // namespace eosv

using namespace eosv;

extern "C" {

int eosv_stem_conv_f32(const float* d_frames, int N, int H, int W, const float* d_w, float* d_z,
                       eosv_stream_t stream) {
  const int rc = stem_train_check("eosv_stem_conv_f32", !d_frames || !d_w || !d_z,
                                  (uintptr_t)d_frames | (uintptr_t)d_w | (uintptr_t)d_z, N, H, W);
  if (rc != EOSV_OK) return rc;
  const int Hs = (H - 1) / 2 + 1, Ws = (W - 1) / 2 + 1;
  const hipStream_t s = (hipStream_t)stream;
  switch ((Ws + 15) / 16) {
#define EOSV_STT_NT(n) \
  case n:              \
    launch_fwd_nt<n>(d_frames, d_w, d_z, N, H, W, Hs, Ws, s); \
    break;
    EOSV_STT_NT(1) EOSV_STT_NT(2) EOSV_STT_NT(3) EOSV_STT_NT(4) EOSV_STT_NT(5) EOSV_STT_NT(6) EOSV_STT_NT(7)
    EOSV_STT_NT(8)
#undef EOSV_STT_NT
  }
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

int64_t eosv_stem_wgrad_f32_workspace(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return stem_wgrad_blocks(stem_wgrad_items(N, H)) * (int64_t)STW_MN * (int64_t)sizeof(float);
}

int eosv_stem_wgrad_f32(const float* d_frames, const float* d_dz, int N, int H, int W, float* d_dw, float* d_work,
                        int64_t work_bytes, eosv_stream_t stream) {
  int rc = stem_train_check("eosv_stem_wgrad_f32", !d_frames || !d_dz || !d_dw || !d_work,
                            (uintptr_t)d_frames | (uintptr_t)d_dz | (uintptr_t)d_dw | (uintptr_t)d_work, N, H, W);
  if (rc != EOSV_OK) return rc;
  if (work_bytes < eosv_stem_wgrad_f32_workspace(N, H, W))
    return set_error("eosv_stem_wgrad_f32: workspace too small"), EOSV_ERR_ARG;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long items = stem_wgrad_items(N, H);
  const int nb = stem_wgrad_blocks(items);
  const size_t lds = (size_t)std::max(STW_ROWS * stt_row_floats(W), STW_ACC_FLOATS) * 4;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(stem_wgrad_f32_kernel, dim3(nb), dim3(STT_NT), lds, s, d_frames, d_dz, d_work, H, W, Ho, Wo,
                     (int)items, (Ho + STW_R - 1) / STW_R);
  EOSV_LAUNCH_CHECK();
  hipLaunchKernelGGL(stem_wgrad_sum_kernel, dim3(STW_MN / 32), dim3(256), 0, s, d_work, nb, d_dw);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}

}  // extern "C"
