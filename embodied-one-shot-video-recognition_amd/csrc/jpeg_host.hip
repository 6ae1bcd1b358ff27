// Baseline JPEG, host stage: header parse (eosv_jpeg_scan) and Huffman entropy decode on host
// threads (eosv_jpeg_entropy), which write the DCT coefficients the GPU stage (jpeg.hip) turns into
// pixels.  Replaces the serial half of the decode behind Image.open(image_path) (utils.py:121).
//
// Plain C++: no HIP header, no device call, so that tests/native/jpeg_host_check.cpp can run this
// file alone under the host sanitizers.  Every read of the file goes through a bounds-checked
// cursor, every coefficient write through an index proven below 64 inside the frame's own range.
#include "eosv.h"

#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace eosv {
void set_error(const std::string& msg);

namespace jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;  // lookahead bits: one table read decodes every code of <= 9 bits

struct Huff {
  bool present = false;
  uint8_t bits[17];
  uint8_t vals[256];
  int nvals = 0;
  // decode tables (build())
  uint16_t look[1 << kLook];  // (length << 8) | symbol, 0 = longer than kLook bits
  int32_t maxcode[18];        // largest code of each length, -1 = none; [17] ends every walk
  int32_t valoff[17];         // vals index of a length's first code minus that code
};

struct Comp {
  int id, h, v, tq, td, ta;
};

struct Header {
  int width = 0, height = 0, ncomp = 0;
  Comp comp[3];
  bool have_sof = false;
  uint16_t qt[4][64];  // natural order
  bool qt_present[4] = {false, false, false, false};
  Huff dc[4], ac[4];
  int restart = 0;
  int64_t scan_pos = 0;  // first byte of entropy-coded data
  int sampling = 0;
  int bw[3], bh[3];  // blocks per component, padded to whole MCUs
  int mcux = 0, mcuy = 0;
};

static bool build(Huff& t, bool is_dc) {
  int code = 0, k = 0;
  memset(t.look, 0, sizeof(t.look));
  for (int l = 1; l <= 16; ++l) {
    const int n = t.bits[l];
    if (n == 0) {
      t.maxcode[l] = -1;
      t.valoff[l] = 0;
    } else {
      if (code + n > (1 << l)) return false;  // more codes than the length holds
      t.valoff[l] = k - code;
      for (int i = 0; i < n; ++i, ++k, ++code) {
        if (is_dc && t.vals[k] > 15) return false;
        if (l <= kLook) {
          const int base = code << (kLook - l);
          for (int j = 0; j < (1 << (kLook - l)); ++j) t.look[base + j] = (uint16_t)((l << 8) | t.vals[k]);
        }
      }
      t.maxcode[l] = code - 1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return true;
}

// EOSV_OK, EOSV_ERR_ARG (not a JPEG / ends early / broken tables) or EOSV_ERR_UNSUPPORTED
static int parse(const uint8_t* d, int64_t n, Header& h) {
  if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return EOSV_ERR_ARG;
  int64_t p = 2;
  for (;;) {
    if (p >= n || d[p] != 0xFF) return EOSV_ERR_ARG;
    while (p < n && d[p] == 0xFF) ++p;  // fill bytes
    if (p >= n) return EOSV_ERR_ARG;
    const int m = d[p++];
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return EOSV_ERR_ARG;  // no segment may stand here
    if (p + 2 > n) return EOSV_ERR_ARG;
    const int len = (d[p] << 8) | d[p + 1];
    if (len < 2 || p + len > n) return EOSV_ERR_ARG;
    const uint8_t* s = d + p + 2;
    const int sl = len - 2;
    p += len;
    if (m == 0xC0) {
      if (h.have_sof) return EOSV_ERR_UNSUPPORTED;
      if (sl < 6) return EOSV_ERR_ARG;
      if (s[0] != 8) return EOSV_ERR_UNSUPPORTED;
      h.height = (s[1] << 8) | s[2];
      h.width = (s[3] << 8) | s[4];
      h.ncomp = s[5];
      if (sl < 6 + 3 * h.ncomp) return EOSV_ERR_ARG;
      if (h.width == 0 || h.height == 0 || h.ncomp == 0) return EOSV_ERR_ARG;
      if (h.ncomp != 1 && h.ncomp != 3) return EOSV_ERR_UNSUPPORTED;
      if (h.width > 4096 || h.height > 4096) return EOSV_ERR_UNSUPPORTED;
      for (int c = 0; c < h.ncomp; ++c) {
        Comp& k = h.comp[c];
        k.id = s[6 + 3 * c];
        k.h = s[7 + 3 * c] >> 4;
        k.v = s[7 + 3 * c] & 15;
        k.tq = s[8 + 3 * c];
        if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4 || k.tq > 3) return EOSV_ERR_ARG;
      }
      h.have_sof = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
      return EOSV_ERR_UNSUPPORTED;  // extended / progressive / lossless / arithmetic frames, DAC
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return EOSV_ERR_ARG;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return EOSV_ERR_ARG;
        Huff& t = tc ? h.ac[th] : h.dc[th];
        int cnt = 0;
        t.bits[0] = 0;
        for (int l = 1; l <= 16; ++l) cnt += (t.bits[l] = s[q + l]);
        if (cnt > 256 || q + 17 + cnt > sl) return EOSV_ERR_ARG;
        memcpy(t.vals, s + q + 17, cnt);
        t.nvals = cnt;
        if (!build(t, tc == 0)) return EOSV_ERR_ARG;
        t.present = true;
        q += 17 + cnt;
      }
    } else if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (tq > 3 || pq > 1) return EOSV_ERR_ARG;
        if (pq) return EOSV_ERR_UNSUPPORTED;  // 16-bit tables
        if (q + 65 > sl) return EOSV_ERR_ARG;
        for (int i = 0; i < 64; ++i) h.qt[tq][kZigzag[i]] = s[q + 1 + i];
        h.qt_present[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {
      if (sl < 2) return EOSV_ERR_ARG;
      h.restart = (s[0] << 8) | s[1];
    } else if (m == 0xEE) {
      if (sl >= 5 && memcmp(s, "Adobe", 5) == 0) return EOSV_ERR_UNSUPPORTED;  // colour transform flag
    } else if (m == 0xDA) {
      if (!h.have_sof) return EOSV_ERR_ARG;
      if (sl < 1) return EOSV_ERR_ARG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl < 1 + 2 * ns + 3) return EOSV_ERR_ARG;
      if (ns != h.ncomp) return EOSV_ERR_UNSUPPORTED;  // several scans
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != h.comp[c].id) return EOSV_ERR_UNSUPPORTED;
        h.comp[c].td = s[2 + 2 * c] >> 4;
        h.comp[c].ta = s[2 + 2 * c] & 15;
        if (h.comp[c].td > 3 || h.comp[c].ta > 3) return EOSV_ERR_ARG;
        if (!h.dc[h.comp[c].td].present || !h.ac[h.comp[c].ta].present || !h.qt_present[h.comp[c].tq])
          return EOSV_ERR_ARG;
      }
      h.scan_pos = p;
      break;
    }
    // APPn, COM and every other segment with a length: skipped
  }
  if (h.ncomp == 1) {
    h.sampling = EOSV_JPEG_GREY;  // a single component is never interleaved: its factors do not matter
    h.mcux = (h.width + 7) / 8;
    h.mcuy = (h.height + 7) / 8;
    h.bw[0] = h.mcux;
    h.bh[0] = h.mcuy;
  } else {
    const Comp* k = h.comp;
    if (k[0].id == 'R' && k[1].id == 'G' && k[2].id == 'B') return EOSV_ERR_UNSUPPORTED;
    if (k[1].h != 1 || k[1].v != 1 || k[2].h != 1 || k[2].v != 1) return EOSV_ERR_UNSUPPORTED;
    if (k[0].h == 1 && k[0].v == 1) h.sampling = EOSV_JPEG_444;
    else if (k[0].h == 2 && k[0].v == 2) h.sampling = EOSV_JPEG_420;
    else return EOSV_ERR_UNSUPPORTED;
    const int s = h.sampling == EOSV_JPEG_420 ? 2 : 1;
    h.mcux = (h.width + 8 * s - 1) / (8 * s);
    h.mcuy = (h.height + 8 * s - 1) / (8 * s);
    h.bw[0] = h.mcux * s;
    h.bh[0] = h.mcuy * s;
    h.bw[1] = h.bw[2] = h.mcux;
    h.bh[1] = h.bh[2] = h.mcuy;
  }
  return EOSV_OK;
}

static int64_t coef_count(const Header& h) {
  int64_t b = 0;
  for (int c = 0; c < h.ncomp; ++c) b += (int64_t)h.bw[c] * h.bh[c];
  return b * 64;
}

// Bit reader over the entropy-coded segment.  Bytes are shifted into the low end of a 64-bit
// window; FF 00 is the byte FF; at any other marker or the end of the file it stops taking bytes
// and shifts zeros in, counting them (`fake`), so that a decoder that went past the real data is
// caught by n < fake without a branch per bit.
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t acc = 0;
  int n = 0;     // bits in acc
  int fake = 0;  // how many of its lowest bits are padding that the file does not hold
  bool stop = false;

  inline void fill() {
    if (n >= 32) return;  // a symbol (<= 16 bits) and its value (<= 15) fit
    if (!stop && end - p >= 4) {  // four bytes at once where none of them is FF
      uint32_t w;
      memcpy(&w, p, 4);
      const uint32_t v = ~w;
      if (!((v - 0x01010101u) & ~v & 0x80808080u)) {
        acc = (acc << 32) | __builtin_bswap32(w);
        n += 32;
        p += 4;
        return;
      }
    }
    while (n <= 56) {
      unsigned b = 0;
      if (!stop) {
        if (p < end && *p != 0xFF) {
          b = *p++;
        } else if (p + 1 < end && p[1] == 0x00) {
          b = 0xFF;
          p += 2;
        } else {
          stop = true;
        }
      }
      if (stop) fake += 8;
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)((acc >> (n - k)) & ((1u << k) - 1)); }
  inline void skip(int k) { n -= k; }
  inline bool overrun() const { return n < fake; }
};

// one Huffman symbol, -1 for a code no length holds; needs >= 16 bits in the window
static inline int symbol(Bits& b, const Huff& t) {
  const unsigned e = t.look[b.peek(kLook)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  int l = kLook + 1;
  int code = (int)b.peek(l);
  while (code > t.maxcode[l]) {
    ++l;
    if (l > 16) return -1;
    code = (int)b.peek(l);
  }
  b.skip(l);
  const int idx = code + t.valoff[l];
  if (idx < 0 || idx >= t.nvals) return -1;
  return t.vals[idx];
}

static inline int extend(Bits& b, int s) {  // s in 1..15: the next s bits as a signed magnitude
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - ((1 << s) - 1) : v;
}

// one 8x8 block into out[64] (zeroed by the caller); false on a bad code or run
static inline bool block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* out) {
  b.fill();
  int s = symbol(b, dc);
  if (s < 0) return false;
  int diff = 0;
  if (s) diff = extend(b, s);  // s <= 15 (build())
  pred = (int16_t)(uint16_t)(pred + diff);
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    b.fill();
    const int rs = symbol(b, ac);
    if (rs < 0) return false;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;  // end of block
      k += 16;
      if (k > 64) return false;
      continue;
    }
    k += r;
    if (k > 63) return false;  // the run leaves the block
    out[kZigzag[k]] = (int16_t)extend(b, s);
    ++k;
  }
  return !b.overrun();
}

static int decode(const uint8_t* d, int64_t n, const Header& h, int16_t* coef) {
  Bits b;
  b.p = d + h.scan_pos;
  b.end = d + n;
  int pred[3] = {0, 0, 0};
  int16_t* base[3];
  base[0] = coef;
  for (int c = 1; c < h.ncomp; ++c) base[c] = base[c - 1] + (int64_t)h.bw[c - 1] * h.bh[c - 1] * 64;
  const int s = h.sampling == EOSV_JPEG_420 ? 2 : 1;
  int left = h.restart, rst = 0;
  for (int my = 0; my < h.mcuy; ++my) {
    for (int mx = 0; mx < h.mcux; ++mx) {
      if (h.restart && left == 0) {
        // the interval's bits end inside its last byte, and RSTn follows (after any fill bytes)
        b.fill();
        if (b.n - b.fake >= 8 || !b.stop) return EOSV_ERR_ARG;
        const uint8_t* q = b.p;
        while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
        if (q + 1 >= b.end || q[0] != 0xFF || q[1] != 0xD0 + rst) return EOSV_ERR_ARG;
        rst = (rst + 1) & 7;
        b.p = q + 2;
        b.acc = 0;
        b.n = b.fake = 0;
        b.stop = false;
        pred[0] = pred[1] = pred[2] = 0;
        left = h.restart;
      }
      for (int c = 0; c < h.ncomp; ++c) {
        const int cs = c == 0 ? s : 1;
        for (int v = 0; v < cs; ++v)
          for (int u = 0; u < cs; ++u) {
            const int64_t br = (int64_t)my * cs + v, bc = (int64_t)mx * cs + u;  // < bh[c], bw[c]
            if (!block(b, h.dc[h.comp[c].td], h.ac[h.comp[c].ta], pred[c], base[c] + (br * h.bw[c] + bc) * 64))
              return EOSV_ERR_ARG;
          }
      }
      if (h.restart) --left;
    }
  }
  return EOSV_OK;
}

}  // namespace jpeg
}  // namespace eosv

using namespace eosv;

extern "C" int eosv_jpeg_scan(const uint8_t* const* data, const int64_t* nbytes, int n, eosv_jpeg_frame* frames) {
  if (n < 0 || (n && (!data || !nbytes || !frames))) {
    set_error("eosv_jpeg_scan: bad argument (null pointer or n < 0)");
    return EOSV_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) {
    eosv_jpeg_frame& f = frames[i];
    f.width = f.height = f.sampling = 0;
    f.coef_elems = 0;
    jpeg::Header h;
    f.status = nbytes[i] < 0 ? (int)EOSV_ERR_ARG : jpeg::parse(data[i], nbytes[i], h);
    if (f.status != EOSV_OK) continue;
    f.width = h.width;
    f.height = h.height;
    f.sampling = h.sampling;
    f.coef_elems = jpeg::coef_count(h);
  }
  return EOSV_OK;
}

extern "C" int eosv_jpeg_entropy(const uint8_t* const* data, const int64_t* nbytes, int n, eosv_jpeg_frame* frames,
                                 int16_t* coef, int64_t coef_elems, uint16_t* quant, int n_threads) {
  if (n < 0 || coef_elems < 0 || (n && (!data || !nbytes || !frames || !coef || !quant))) {
    set_error("eosv_jpeg_entropy: bad argument (null pointer, n < 0 or coef_elems < 0)");
    return EOSV_ERR_ARG;
  }
  int T = n_threads < 1 ? 1 : n_threads > 16 ? 16 : n_threads;
  if (T > n) T = n < 1 ? 1 : n;
  auto work = [&](int t) {
    for (int i = t; i < n; i += T) {
      eosv_jpeg_frame& f = frames[i];
      if (f.status != EOSV_OK) continue;
      jpeg::Header h;  // parsed again: the scan keeps no state between the calls
      int rc = nbytes[i] < 0 ? (int)EOSV_ERR_ARG : jpeg::parse(data[i], nbytes[i], h);
      if (rc == EOSV_OK) {
        const int64_t cnt = jpeg::coef_count(h);
        if (cnt != f.coef_elems || f.coef_offset < 0 || f.coef_offset > coef_elems || cnt > coef_elems - f.coef_offset)
          rc = EOSV_ERR_ARG;
        else {
          int16_t* out = coef + f.coef_offset;
          memset(out, 0, (size_t)cnt * sizeof(int16_t));
          uint16_t* q = quant + (int64_t)i * 192;
          memset(q, 0, 192 * sizeof(uint16_t));
          for (int c = 0; c < h.ncomp; ++c) memcpy(q + 64 * c, h.qt[h.comp[c].tq], 64 * sizeof(uint16_t));
          rc = jpeg::decode(data[i], nbytes[i], h, out);
        }
      }
      f.status = rc;
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(T);
  for (int t = 1; t < T; ++t) {
    try {
      pool.emplace_back(work, t);
    } catch (...) {  // no thread to be had: its frames are decoded here
      work(t);
    }
  }
  work(0);
  for (auto& th : pool) th.join();
  return EOSV_OK;
}
