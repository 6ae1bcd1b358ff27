// Self-test of tests/native/x3_ref.h on the host: the unmutated emulator of the f32x3 conv
// arithmetic must pass the per-element bound and the dup condition, and every mutation must be
// rejected by the bound with probe data.  One line per (shape, data mode, mutation):
//   <shape> <mode> <mutation> PASS|REJECT|SAME ratio <max err / bound> bad <n> dup <n>
// SAME: the mutated emulator's output is bit-identical to the unmutated one (the shape has
// nothing the mutation touches: a 1x1 without padding has no padding tap), so no check can see it.
// Build: hipcc -x hip --cuda-host-only -O2 x3_ref_selftest.cpp (tests/test_cpu_x3_ref.py).
#include "x3_ref.h"

int main() {
  struct Sh {
    const char* name;
    x3::Shape s;
    bool res;
  };
  const Sh shapes[] = {
      {"3x3_64_64_6x56_res", {1, 6, 56, 64, 64, 3, 1, 1, 0, 0, false}, true},
      {"1x1_256_64_5x7_res", {1, 5, 7, 256, 64, 1, 1, 0, 0, 0, false}, true},
      {"3x3_512_64_4x4_res", {1, 4, 4, 512, 64, 3, 1, 1, 0, 0, false}, true},  // large K: the real-data margins
  };
  const char* mnames[] = {"none", "a_drop_lo_step", "b_block2_reads_lo", "c_no_res_lo", "d_zero_y_lo", "e_pad_neighbour"};
  for (const Sh& sh : shapes)
    for (int real = 0; real < 2; ++real) {
      x3::Shape s = sh.s;
      s.real = real;
      const x3::Case c = x3::make_case(s);
      const x3::Ref r = x3::reference(c);
      const std::vector<x3::u16> base = x3::emulate(c, sh.res, true, x3::kNone);
      for (int m = 0; m <= x3::kPadNeighbour; ++m) {
        const std::vector<x3::u16> y = m ? x3::emulate(c, sh.res, true, (x3::Mutation)m) : base;
        const x3::Stats st = x3::verify(c, r, y.data(), sh.res, true, x3::kCoef, false);
        const char* verdict = m && y == base ? "SAME" : st.bad ? "REJECT" : st.bad_dup ? "REJECT_DUP" : "PASS";
        printf("%s %s %s %s ratio %.3e bad %ld dup %ld\n", sh.name, real ? "real" : "probe", mnames[m], verdict,
               st.max_ratio, st.bad, st.bad_dup);
      }
    }
  return 0;
}
