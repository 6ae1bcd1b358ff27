// Self-test of tests/native/bf16_ref.h on the host.  Per (shape, data mode):
//   cond <shape> <mode> outputs <n> over256 <n> max_sabs <n> violations <n>
//       the data conditions as the int64 reference saw them: its upper bound of the sum of |terms|
//       (max_sabs: the largest over all outputs of all stages) below 2^24 at every output
//       (violations 0), and how many of the values handed to the conversion lie outside +-256
//   <shape> <mode> none EQUAL|MISMATCH differing <n> of <total>
//       the unmutated f32 emulator against the int64 reference, bitwise
//   <shape> <mode> <slip> DIFF|SAME differing <n> of <total>
//       the emulator with one slip against the unmutated emulator
// Build: hipcc -x hip --cuda-host-only -O2 bf16_ref_selftest.cpp (tests/test_cpu_bf16_ref.py).
#include "bf16_ref.h"

using namespace bfr;

static void report(const char* shape, int mode, const Cond& c) {
  printf("cond %s %s outputs %lld over256 %lld max_sabs %lld violations %lld\n", shape, mode_name(mode), c.outputs, c.over256,
         c.max_sabs, c.violations);
}
static long long diff2(const ChainOut& a, const ChainOut& b) { return differing(a.y, b.y) + differing(a.z, b.z); }

template <class Run>
static void sweep(const char* shape, int mode, Run run) {
  const ChainOut ref = run(true, kNone), base = run(false, kNone);
  report(shape, mode, ref.cond);
  const long long total = (long long)(ref.y.size() + ref.z.size());
  const long long d0 = diff2(ref, base);
  printf("%s %s none %s differing %lld of %lld\n", shape, mode_name(mode), d0 ? "MISMATCH" : "EQUAL", d0, total);
  for (int s = kDropStep; s <= kDsNoStride; ++s) {
    const long long d = diff2(base, run(false, (Slip)s));
    printf("%s %s %s %s differing %lld of %lld\n", shape, mode_name(mode), slip_name(s), d ? "DIFF" : "SAME", d, total);
  }
}

int main() {
  for (int mode = 0; mode < 2; ++mode) {
    {
      const ConvCase c = make_conv(1, 6, 56, 64, 64, 3, 1, 1, 0, 0, mode);
      sweep("3x3_64_64_6x56_res", mode, [&](bool ref, Slip s) {
        ChainOut o;
        o.y = ref ? run_stage<long long>(c.stage(true, true), kNone, true, &o.cond) : run_stage<float>(c.stage(true, true), s);
        return o;
      });
    }
    {
      const ConvCase c = make_conv(1, 5, 7, 128, 64, 1, 1, 0, 64, 2, mode);
      sweep("1x1_128_64_5x7_ds2_res", mode, [&](bool ref, Slip s) {
        ChainOut o;
        o.y = ref ? run_stage<long long>(c.stage(true, true), kNone, true, &o.cond) : run_stage<float>(c.stage(true, true), s);
        return o;
      });
    }
    {
      const ConvCase c = make_conv(1, 4, 4, 512, 512, 3, 1, 1, 0, 0, mode);
      sweep("3x3_512_512_4x4_res", mode, [&](bool ref, Slip s) {
        ChainOut o;
        o.y = ref ? run_stage<long long>(c.stage(true, true), kNone, true, &o.cond) : run_stage<float>(c.stage(true, true), s);
        return o;
      });
    }
    {
      const BneckCase c = make_bneck(1, 4, 56, 64, false, false, mode);
      sweep("bneck_64_ds_4x56", mode, [&](bool ref, Slip s) { return ref ? run_bneck<long long>(c) : run_bneck<float>(c, s); });
    }
    {
      const BneckCase c = make_bneck(1, 2, 56, 256, true, false, mode);
      sweep("bneck_256_next_2x56", mode, [&](bool ref, Slip s) { return ref ? run_bneck<long long>(c) : run_bneck<float>(c, s); });
    }
  }
  return 0;
}
