// Host stage of the JPEG decoder (csrc/jpeg_host.hip: eosv_jpeg_scan, eosv_jpeg_entropy) under the
// host sanitizers, on its own: `make -C csrc jpeg_check` compiles that file and this one with
// -fsanitize=address,undefined.  No device call is made and no HIP runtime is initialised.
//
//   jpeg_host_check FILE...
//
// For every file, at 1 and at 4 threads: the intact file (one line `OK name threads w h sampling
// checksum` per file and thread count, which tests/test_cpu_jpeg.py compares with the release
// library's), every prefix at a stride of 97 bytes, and 200 seeded single-byte corruptions.  Every variant is a heap block of its
// exact length, so a read past a truncated file is an ASan report; the coefficient buffer sits
// between sentinel regions.  Exit 0 and a last line `jpeg_host_check: ok` when every call returned
// EOSV_OK, every frame carries a status of the ABI and the sentinels are intact.
#include "eosv.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

namespace eosv {
void set_error(const std::string&) {}  // the library's error slot lives in eosv_api.hip, not linked here
}  // namespace eosv

namespace {

constexpr int64_t kGuard = 4096;        // int16 elements on either side
constexpr int16_t kSentinel = 0x5A5A;
constexpr int64_t kBatchElems = 32ll << 20;  // a corrupted header may announce up to 4096 x 4096

struct Blob {
  std::unique_ptr<uint8_t[]> p;  // exact length: no slack behind a truncated file
  int64_t n;
};

Blob blob(const uint8_t* d, int64_t n) {
  Blob b{std::unique_ptr<uint8_t[]>(new uint8_t[n > 0 ? n : 1]), n};
  if (n > 0) memcpy(b.p.get(), d, n);
  return b;
}

uint64_t checksum(const int16_t* c, int64_t n, const uint16_t* q) {
  uint64_t s = 0;
  for (int64_t i = 0; i < n; ++i) s += (uint64_t)(uint16_t)c[i] * (uint64_t)(i % 65521 + 1);
  for (int i = 0; i < 192; ++i) s += (uint64_t)q[i] * (uint64_t)(1000003 + i);
  return s;
}

int fail(const char* what) {
  printf("jpeg_host_check: FAILED: %s\n", what);
  return 1;
}

// scan + entropy over blobs[lo, hi); 0, or 1 after printing what went wrong
int run(const std::vector<Blob>& blobs, size_t lo, size_t hi, int threads, const char* name, bool print) {
  const int n = (int)(hi - lo);
  std::vector<const uint8_t*> data(n);
  std::vector<int64_t> nbytes(n);
  for (int i = 0; i < n; ++i) {
    data[i] = blobs[lo + i].p.get();
    nbytes[i] = blobs[lo + i].n;
  }
  std::vector<eosv_jpeg_frame> fr(n);
  if (eosv_jpeg_scan(data.data(), nbytes.data(), n, fr.data()) != EOSV_OK) return fail("eosv_jpeg_scan returned an error");
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    const int st = fr[i].status;
    if (st != EOSV_OK && st != EOSV_ERR_ARG && st != EOSV_ERR_UNSUPPORTED) return fail("scan status outside the ABI");
    fr[i].coef_offset = total;
    if (st == EOSV_OK) total += fr[i].coef_elems;
  }
  std::vector<int16_t> buf(total + 2 * kGuard, kSentinel);
  std::vector<uint16_t> quant((size_t)n * 192 + 1, 0);
  if (eosv_jpeg_entropy(data.data(), nbytes.data(), n, fr.data(), buf.data() + kGuard, total, quant.data(), threads) !=
      EOSV_OK)
    return fail("eosv_jpeg_entropy returned an error");
  for (int64_t i = 0; i < kGuard; ++i)
    if (buf[i] != kSentinel || buf[kGuard + total + i] != kSentinel) return fail("sentinel overwritten");
  for (int i = 0; i < n; ++i) {
    const int st = fr[i].status;
    if (st != EOSV_OK && st != EOSV_ERR_ARG && st != EOSV_ERR_UNSUPPORTED) return fail("entropy status outside the ABI");
    if (print) {
      if (st != EOSV_OK) return fail("an intact file was refused");
      printf("OK %s %d %d %d %d %llu\n", name, threads, fr[i].width, fr[i].height, fr[i].sampling,
             (unsigned long long)checksum(buf.data() + kGuard + fr[i].coef_offset, fr[i].coef_elems,
                                          quant.data() + (size_t)i * 192));
    }
  }
  return 0;
}

// the variants in batches whose announced coefficient counts stay below kBatchElems
int run_batched(const std::vector<Blob>& blobs, int threads) {
  std::vector<const uint8_t*> data(blobs.size());
  std::vector<int64_t> nbytes(blobs.size());
  for (size_t i = 0; i < blobs.size(); ++i) {
    data[i] = blobs[i].p.get();
    nbytes[i] = blobs[i].n;
  }
  std::vector<eosv_jpeg_frame> fr(blobs.size());
  if (eosv_jpeg_scan(data.data(), nbytes.data(), (int)blobs.size(), fr.data()) != EOSV_OK)
    return fail("eosv_jpeg_scan returned an error");
  size_t lo = 0;
  int64_t sum = 0;
  for (size_t i = 0; i <= blobs.size(); ++i) {
    const int64_t e = i < blobs.size() && fr[i].status == EOSV_OK ? fr[i].coef_elems : 0;
    if (i == blobs.size() || (i > lo && sum + e > kBatchElems)) {
      if (i > lo && run(blobs, lo, i, threads, "", false)) return 1;
      lo = i;
      sum = 0;
    }
    sum += e;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return fail("usage: jpeg_host_check FILE...");
  for (int a = 1; a < argc; ++a) {
    std::ifstream in(argv[a], std::ios::binary);
    std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (file.empty()) return fail("cannot read a file");
    const int64_t n = (int64_t)file.size();
    const char* base = strrchr(argv[a], '/');
    base = base ? base + 1 : argv[a];
    std::vector<Blob> intact, variants;
    intact.push_back(blob(file.data(), n));
    for (int64_t cut = 0; cut < n; cut += 97) variants.push_back(blob(file.data(), cut));
    uint64_t rng = 0x9E3779B97F4A7C15ull * (uint64_t)(a + 1);
    for (int i = 0; i < 200; ++i) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      // every other corruption falls into the first 640 bytes, where the headers and tables are
      const int64_t span = (i & 1) && n > 640 ? 640 : n;
      const int64_t pos = (int64_t)((rng >> 33) % (uint64_t)span);
      Blob b = blob(file.data(), n);
      b.p[pos] ^= (uint8_t)(1 + ((rng >> 20) % 255));
      variants.push_back(std::move(b));
    }
    for (int threads : {1, 4}) {
      if (run(intact, 0, 1, threads, base, true)) return 1;
      if (run_batched(variants, threads)) return 1;
    }
  }
  printf("jpeg_host_check: ok\n");
  return 0;
}
