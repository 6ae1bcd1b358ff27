// Host check of the Winograd kernel's multiply-shift division (csrc/common.h: wino_div, wino_fdiv)
// against `/`: for a divisor d >= 1 and every dividend 0 <= t < 2^31 the two must agree.  Dense
// over small divisors and dividends, around every multiple boundary near 2^31, around powers of
// two, and random pairs.  No device call.  Built and run by tests/test_cpu_wino_persist.py.
#include <cstdio>
#include <random>

#include "common.h"

int main() {
  using eosv::wino_div;
  using eosv::wino_fdiv;
  long long n = 0, bad = 0;
  auto chk = [&](unsigned d, long long t) {
    if (t < 0 || t > 0x7fffffffLL) return;
    ++n;
    if (wino_fdiv((int)t, wino_div(d)) != (int)((unsigned)t / d) && bad++ < 5)
      std::printf("FAIL d = %u t = %lld\n", d, t);
  };
  for (unsigned d = 1; d <= 2048; ++d) {
    for (long long t = 0; t < 20000; ++t) chk(d, t);
    for (long long k = 0; k < 64; ++k) {
      chk(d, 0x7fffffffLL - k);
      const long long m = (0x7fffffffLL / d - k) * d;  // a multiple of d near 2^31, and its neighbours
      chk(d, m - 1), chk(d, m), chk(d, m + 1);
    }
  }
  for (int l = 0; l < 31; ++l)
    for (int e = -2; e <= 2; ++e) {
      const long long d = (1LL << l) + e;
      if (d < 1) continue;
      for (long long k = 0; k < 4096; ++k) chk((unsigned)d, 0x7fffffffLL - k), chk((unsigned)d, d * k + d - 1), chk((unsigned)d, d * k);
    }
  std::mt19937_64 g(1);
  for (int i = 0; i < 4000000; ++i) {
    const unsigned d = (unsigned)(g() % 0x7fffffffu) + 1;
    chk(d, (long long)(g() & 0x7fffffff));
    const long long q = 0x7fffffffLL / d;
    if (q) {
      const long long m = (long long)(g() % q + 1) * d;
      chk(d, m - 1), chk(d, m);
    }
  }
  std::printf("%s: %lld pairs, %lld wrong\n", bad ? "FAIL" : "ok", n, bad);
  return bad != 0;
}
