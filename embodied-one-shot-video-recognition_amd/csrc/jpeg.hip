// Baseline JPEG, GPU stage: the DCT coefficients the host stage wrote (jpeg_host.hip) -> the
// [F,3,crop,crop] f32 NCHW frames the backbone takes.  Replaces the pixel half of
// the decode behind Image.open(image_path) (utils.py:121) and the transform behind it (ingest.hip).
//
// Everything is libjpeg's integer arithmetic, so the pixels equal PIL's bit for bit:
//   jpeg_idct_kernel   dequantise, 13-bit slow-integer inverse DCT, +128, clamp -> uint8 component
//                      planes in the workspace; only the blocks the window (and, for 4:2:0, its
//                      one-sample chroma halo) touches.  Eight lanes per block: a column each in
//                      the first pass, a row each in the second, transposed through LDS.
//   jpeg_pixel_kernel  one thread per output pixel (consecutive lanes = consecutive x): triangle
//                      chroma upsampling, YCbCr -> RGB, crop, flip, then the /255, -mean, /std of
//                      ingest.hip in the same correctly rounded order.
#include "common.h"

#include <algorithm>
#include <vector>

namespace eosv {
namespace jpeg {

// what the kernels read per frame, built and checked on the host (eosv_jpeg_render)
struct FrameInfo {
  long long coef;      // first coefficient of the frame in d_coef
  long long plane;     // first byte of its planes in the workspace
  int W, H, sampling;  // EOSV_JPEG_*
  int top, left, flip;
  int bw[2], bh[2];    // blocks per row / rows of blocks: [0] Y, [1] each chroma plane
  int r0[2], c0[2];    // first block row / column computed
  int nr[2], nc[2];    // block rows / columns computed
};

// one line of the 8-point inverse DCT (jidctint.c, CONST_BITS 13), before the descale
__device__ __forceinline__ void idct8(const int i[8], int o[8]) {
  const int z = (i[2] + i[6]) * 4433;
  const int t2 = z - i[6] * 15137, t3 = z + i[2] * 6270;
  const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a = i[7], b = i[5], c = i[3], d = i[1];
  const int z5 = (a + c + b + d) * 9633;
  const int z1 = -(a + d) * 7373, z2 = -(b + c) * 20995;
  const int z3 = -(a + c) * 16069 + z5, z4 = -(b + d) * 3196 + z5;
  a = a * 2446 + z1 + z3;
  b = b * 16819 + z2 + z4;
  c = c * 25172 + z2 + z3;
  d = d * 12299 + z1 + z4;
  o[0] = t10 + d;
  o[7] = t10 - d;
  o[1] = t11 + c;
  o[6] = t11 - c;
  o[2] = t12 + b;
  o[5] = t12 - b;
  o[3] = t13 + a;
  o[4] = t13 - a;
}

constexpr int kBlocksPerWg = 32;  // 8 lanes each: 256 threads
constexpr size_t kSyncBytes = 256 << 10;  // descriptor tables above this are waited for (eosv_jpeg_render)

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* __restrict__ coef,
                                                        const unsigned short* __restrict__ quant,
                                                        const FrameInfo* __restrict__ info,
                                                        unsigned char* __restrict__ work) {
  __shared__ int ta[kBlocksPerWg][64];  // dequantised block, [row][column]
  __shared__ int tb[kBlocksPerWg][64];  // after the column pass
  const int f = blockIdx.y;
  const FrameInfo fi = info[f];
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  int b = blockIdx.x * kBlocksPerWg + g;  // index among the blocks this frame computes
  const int ny = fi.nr[0] * fi.nc[0], nch = fi.nr[1] * fi.nc[1];
  const int total = ny + (fi.sampling == EOSV_JPEG_GREY ? 0 : 2 * nch);
  const bool live = b < total;
  int comp = 0, k = 0;  // component, and 0 = Y geometry, 1 = chroma geometry
  if (live && b >= ny) {
    b -= ny;
    comp = 1 + (b >= nch);
    if (b >= nch) b -= nch;
    k = 1;
  }
  long long blk = 0, pbase = 0;
  int br = 0, bc = 0;
  if (live) {
    br = fi.r0[k] + b / fi.nc[k];
    bc = fi.c0[k] + b % fi.nc[k];
    const long long ysz = (long long)fi.bw[0] * fi.bh[0], csz = (long long)fi.bw[1] * fi.bh[1];
    const long long first = comp == 0 ? 0 : ysz + (comp - 1) * csz;  // blocks in front of this component
    blk = first + (long long)br * fi.bw[k] + bc;
    pbase = fi.plane + first * 64;
    // row l of the block: 8 coefficients and their 8 quantisers, 16 bytes each
    const uint4 cw = *reinterpret_cast<const uint4*>(coef + fi.coef + blk * 64 + l * 8);
    const uint4 qw = *reinterpret_cast<const uint4*>(quant + ((long long)f * 3 + comp) * 64 + l * 8);
    const unsigned cu[4] = {cw.x, cw.y, cw.z, cw.w}, qu[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ta[g][l * 8 + 2 * j] = (int)(short)(cu[j] & 0xffff) * (int)(qu[j] & 0xffff);
      ta[g][l * 8 + 2 * j + 1] = (int)(short)(cu[j] >> 16) * (int)(qu[j] >> 16);
    }
  }
  __syncthreads();
  if (live) {
    int i[8], o[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) i[u] = ta[g][u * 8 + l];  // column l
    idct8(i, o);
#pragma unroll
    for (int u = 0; u < 8; ++u) tb[g][u * 8 + l] = (o[u] + (1 << 10)) >> 11;
  }
  __syncthreads();
  if (live) {
    int i[8], o[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) i[u] = tb[g][l * 8 + u];  // row l
    idct8(i, o);
    unsigned w[2] = {0, 0};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int v = ((o[u] + (1 << 17)) >> 18) + 128;
      v = v < 0 ? 0 : v > 255 ? 255 : v;
      w[u >> 2] |= (unsigned)v << (8 * (u & 3));
    }
    // plane row stride bw * 8, plane bases multiples of 64: the 8 bytes are 8-byte aligned
    unsigned char* dst = work + pbase + ((long long)br * 8 + l) * (fi.bw[k] * 8) + bc * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  }
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// h2v2 "fancy" upsampling (jdsample.c): sample (sy, sx) of the full-size plane from the
// ceil(H/2) x ceil(W/2) plane p of row stride `stride`
__device__ __forceinline__ int chroma420(const unsigned char* __restrict__ p, int stride, int ch, int cw, int sy,
                                         int sx) {
  const int r = sy >> 1, x = sx >> 1;
  int r2 = (sy & 1) ? r + 1 : r - 1;
  r2 = r2 < 0 ? 0 : r2 > ch - 1 ? ch - 1 : r2;
  const unsigned char* a = p + (long long)r * stride;
  const unsigned char* b = p + (long long)r2 * stride;
  const int s = 3 * a[x] + b[x];
  if (sx & 1) {
    if (x == cw - 1) return (4 * s + 7) >> 4;
    return (3 * s + (3 * a[x + 1] + b[x + 1]) + 7) >> 4;
  }
  if (x == 0) return (4 * s + 8) >> 4;
  return (3 * s + (3 * a[x - 1] + b[x - 1]) + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_pixel_kernel(const FrameInfo* __restrict__ info,
                                                         const unsigned char* __restrict__ work, int crop, float m0,
                                                         float m1, float m2, float s0, float s1, float s2,
                                                         float* __restrict__ out) {
  const int f = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int cc = crop * crop;
  if (p >= cc) return;
  const FrameInfo fi = info[f];
  const int y = p / crop, x = p - y * crop;
  const int sy = fi.top + y, sx = fi.left + (fi.flip ? crop - 1 - x : x);
  const unsigned char* yp = work + fi.plane;
  const int ys = fi.bw[0] * 8;
  const int Y = yp[(long long)sy * ys + sx];
  int rgb[3] = {Y, Y, Y};
  if (fi.sampling != EOSV_JPEG_GREY) {
    const long long ysz = (long long)fi.bw[0] * fi.bh[0] * 64, csz = (long long)fi.bw[1] * fi.bh[1] * 64;
    const unsigned char* cbp = yp + ysz;
    const unsigned char* crp = cbp + csz;
    const int cs = fi.bw[1] * 8;
    int cb, cr;
    if (fi.sampling == EOSV_JPEG_420) {
      const int ch = (fi.H + 1) >> 1, cw = (fi.W + 1) >> 1;
      cb = chroma420(cbp, cs, ch, cw, sy, sx);
      cr = chroma420(crp, cs, ch, cw, sy, sx);
    } else {
      cb = cbp[(long long)sy * cs + sx];
      cr = crp[(long long)sy * cs + sx];
    }
    cb -= 128;
    cr -= 128;
    rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
  float* o = out + (long long)f * 3 * cc + p;
  const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = __fdiv_rn((float)rgb[c], 255.0f);
    o[(long long)c * cc] = __fdiv_rn(__fsub_rn(v, mean[c]), sd[c]);
  }
}

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

// geometry of one descriptor; false where it is not a frame the host stage can have produced
static bool frame_geometry(const eosv_jpeg_desc& d, FrameInfo& fi, long long& elems) {
  if (d.width < 1 || d.height < 1 || d.width > 4096 || d.height > 4096) return false;
  if (d.sampling != EOSV_JPEG_444 && d.sampling != EOSV_JPEG_420 && d.sampling != EOSV_JPEG_GREY) return false;
  const int s = d.sampling == EOSV_JPEG_420 ? 2 : 1;
  const int mx = (d.width + 8 * s - 1) / (8 * s), my = (d.height + 8 * s - 1) / (8 * s);
  fi.W = d.width;
  fi.H = d.height;
  fi.sampling = d.sampling;
  fi.bw[0] = mx * s;
  fi.bh[0] = my * s;
  fi.bw[1] = d.sampling == EOSV_JPEG_GREY ? 0 : mx;
  fi.bh[1] = d.sampling == EOSV_JPEG_GREY ? 0 : my;
  elems = ((long long)fi.bw[0] * fi.bh[0] + 2ll * fi.bw[1] * fi.bh[1]) * 64;
  return true;
}

// total workspace bytes; fills `table` (when given) with the frames' entries.  Negative on a bad
// descriptor.  crop < 0: geometry only (the workspace function).
static long long plan(const eosv_jpeg_desc* desc, int n, int crop, long long coef_elems, std::vector<FrameInfo>* table,
                      int* max_blocks) {
  long long bytes = align_up((long long)n * (long long)sizeof(FrameInfo), 256);
  int mb = 0;
  for (int f = 0; f < n; ++f) {
    FrameInfo fi = {};
    long long elems = 0;
    if (!frame_geometry(desc[f], fi, elems)) return -1;
    fi.plane = bytes;
    bytes += align_up(elems, 256);  // one byte per coefficient
    if (crop >= 0) {
      const eosv_jpeg_desc& d = desc[f];
      if (d.top < 0 || d.left < 0 || d.top > d.height - crop || d.left > d.width - crop) return -1;
      if (d.coef_offset < 0 || (d.coef_offset & 7) || d.coef_offset > coef_elems || elems > coef_elems - d.coef_offset)
        return -1;
      fi.coef = d.coef_offset;
      fi.top = d.top;
      fi.left = d.left;
      fi.flip = d.flip ? 1 : 0;
      // Y: the blocks under the window
      fi.r0[0] = d.top / 8;
      fi.c0[0] = d.left / 8;
      fi.nr[0] = (d.top + crop - 1) / 8 - fi.r0[0] + 1;
      fi.nc[0] = (d.left + crop - 1) / 8 - fi.c0[0] + 1;
      if (d.sampling == EOSV_JPEG_444) {
        fi.r0[1] = fi.r0[0];
        fi.c0[1] = fi.c0[0];
        fi.nr[1] = fi.nr[0];
        fi.nc[1] = fi.nc[0];
      } else if (d.sampling == EOSV_JPEG_420) {
        // chroma samples under the window and one around it, inside the ceil(H/2) x ceil(W/2) plane
        const int ch = (d.height + 1) / 2, cw = (d.width + 1) / 2;
        const int ra = std::max(0, d.top / 2 - 1), rb = std::min(ch - 1, (d.top + crop - 1) / 2 + 1);
        const int ca = std::max(0, d.left / 2 - 1), cb = std::min(cw - 1, (d.left + crop - 1) / 2 + 1);
        fi.r0[1] = ra / 8;
        fi.c0[1] = ca / 8;
        fi.nr[1] = rb / 8 - fi.r0[1] + 1;
        fi.nc[1] = cb / 8 - fi.c0[1] + 1;
      }
      const int blocks = fi.nr[0] * fi.nc[0] + 2 * fi.nr[1] * fi.nc[1];
      mb = std::max(mb, blocks);
      if (table) table->push_back(fi);
    }
  }
  if (max_blocks) *max_blocks = mb;
  return bytes;
}

}  // namespace jpeg
}  // namespace eosv

using namespace eosv;

extern "C" int64_t eosv_jpeg_render_workspace(const eosv_jpeg_desc* desc, int n_frames) {
  if (n_frames < 0 || n_frames > 65535 || (n_frames && !desc)) {
    set_error("eosv_jpeg_render_workspace: bad argument (null table; 0 <= n_frames <= 65535)");
    return EOSV_ERR_ARG;
  }
  const long long b = jpeg::plan(desc, n_frames, -1, 0, nullptr, nullptr);
  if (b < 0) {
    set_error("eosv_jpeg_render_workspace: bad descriptor (size 1..4096, sampling class)");
    return EOSV_ERR_ARG;
  }
  return b;
}

extern "C" int eosv_jpeg_render(const int16_t* d_coef, int64_t coef_elems, const uint16_t* d_quant,
                                const eosv_jpeg_desc* desc, int n_frames, int crop, const float* mean, const float* sd,
                                float* d_out, void* d_work, int64_t work_bytes, eosv_stream_t stream) {
  if (n_frames < 0 || n_frames > 65535 || crop <= 0 || crop > 4096 || !mean || !sd || coef_elems < 0 ||
      (n_frames && (!d_coef || !d_quant || !desc || !d_out || !d_work)) || ((uintptr_t)d_coef & 15) ||
      ((uintptr_t)d_quant & 15) || ((uintptr_t)d_work & 15)) {
    set_error("eosv_jpeg_render: bad argument (null or unaligned pointer; crop 1..4096; n_frames <= 65535)");
    return EOSV_ERR_ARG;
  }
  if (n_frames == 0) return EOSV_OK;
  std::vector<jpeg::FrameInfo> table;
  table.reserve(n_frames);
  int max_blocks = 0;
  const long long need = jpeg::plan(desc, n_frames, crop, coef_elems, &table, &max_blocks);
  if (need < 0) {
    set_error("eosv_jpeg_render: bad descriptor (window inside its frame; coefficient range inside d_coef)");
    return EOSV_ERR_ARG;
  }
  if (work_bytes < need) {
    set_error("eosv_jpeg_render: workspace below eosv_jpeg_render_workspace");
    return EOSV_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  // The table is pageable host memory that dies with this call.  The runtime copies a small pageable
  // source into its own staging memory before hipMemcpyAsync returns; a large one it may pin and read
  // later, so above kSyncBytes (about 2900 frames) the call waits for the copy.
  const size_t table_bytes = table.size() * sizeof(jpeg::FrameInfo);
  EOSV_HIP_CHECK(hipMemcpyAsync(d_work, table.data(), table_bytes, hipMemcpyHostToDevice, s));
  if (table_bytes > jpeg::kSyncBytes) EOSV_HIP_CHECK(hipStreamSynchronize(s));
  const jpeg::FrameInfo* d_info = (const jpeg::FrameInfo*)d_work;
  dim3 g1((max_blocks + jpeg::kBlocksPerWg - 1) / jpeg::kBlocksPerWg, n_frames);
  hipLaunchKernelGGL(jpeg::jpeg_idct_kernel, g1, dim3(256), 0, s, (const short*)d_coef, (const unsigned short*)d_quant,
                     d_info, (unsigned char*)d_work);
  EOSV_LAUNCH_CHECK();
  dim3 g2((crop * crop + 255) / 256, n_frames);
  hipLaunchKernelGGL(jpeg::jpeg_pixel_kernel, g2, dim3(256), 0, s, d_info, (const unsigned char*)d_work, crop, mean[0],
                     mean[1], mean[2], sd[0], sd[1], sd[2], d_out);
  EOSV_LAUNCH_CHECK();
  return EOSV_OK;
}
