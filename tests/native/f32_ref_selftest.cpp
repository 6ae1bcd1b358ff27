// Self-test of tests/native/f32_ref.h (and of the wide data modes and operand slips it adds to
// bf16_ref.h) on the host.  Per (shape, data mode), in bf16_ref_selftest.cpp's format:
//   cond <shape> <mode> outputs <n> over256 <n> max_sabs <n> violations <n>
//   <shape> <mode> none EQUAL|MISMATCH differing <n> of <total>
//       the unmutated f32 emulator against the int64 reference, bitwise, nothing rounded
//   <shape> <mode> <slip> DIFF|SAME differing <n> of <total>
//       the emulator with one slip against the unmutated emulator
// Slips (c) and (e) concern the bf16 conversion and are not run: an f32 output is not converted.
// Build: hipcc -x hip --cuda-host-only -O2 f32_ref_selftest.cpp (tests/test_cpu_f32_ref.py).
#include "f32_ref.h"

using namespace bfr;

static const Slip kSlips[] = {kDropStep, kPadNeighbour, kResAfterRelu, kDsNoStride, kOpBf16, kOpMant10, kOpTf32};

template <class Run>
static void sweep(const char* shape, int mode, Run run) {
  const ChainOut ref = run(true, kNone), base = run(false, kNone);
  printf("cond %s %s outputs %lld over256 %lld max_sabs %lld violations %lld\n", shape, mode_name(mode), ref.cond.outputs,
         ref.cond.over256, ref.cond.max_sabs, ref.cond.violations);
  const long long total = (long long)ref.y.size();
  const long long d0 = differing(ref.y, base.y);
  printf("%s %s none %s differing %lld of %lld\n", shape, mode_name(mode), d0 ? "MISMATCH" : "EQUAL", d0, total);
  for (Slip s : kSlips) {
    const long long d = differing(base.y, run(false, s).y);
    printf("%s %s %s %s differing %lld of %lld\n", shape, mode_name(mode), slip_name(s), d ? "DIFF" : "SAME", d, total);
  }
}

static void conv(const char* shape, int mode, const ConvCase& c) {
  sweep(shape, mode, [&](bool ref, Slip s) {
    ChainOut o;
    o.y = ref ? run_stage<long long>(c.stage(true, true), kNone, false, &o.cond) : run_stage<float>(c.stage(true, true), s, false);
    return o;
  });
}

int main() {
  for (int mode = 0; mode < 4; ++mode) {
    conv("1x1_64_64_5x7_res", mode, make_conv(2, 5, 7, 64, 64, 1, 1, 0, 0, 0, mode));
    conv("3x3_64_96_6x10_res", mode, make_conv(1, 6, 10, 64, 96, 3, 1, 1, 0, 0, mode));
    conv("3x3s2_32_64_9x11_ds2_res", mode, make_conv(2, 9, 11, 32, 64, 3, 2, 1, 32, 2, mode));
    // the largest K the f32 kernels take: 3x3 at 512 channels plus a 256-channel shortcut
    conv("3x3_512_8_3x3_ds2_256_res", mode, make_conv(1, 3, 3, 512, 8, 3, 1, 1, 256, 2, mode));
    const StemCase st = make_stem(2, 20, 18, mode);
    sweep("stem_pool_20x18", mode, [&](bool ref, Slip s) { return ref ? f32r::run_stem<long long>(st) : f32r::run_stem<float>(st, s); });
  }
  return 0;
}
