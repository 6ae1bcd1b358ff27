"""tests/native/f32_ref.h on the host: the integer data, the int64 reference and the emulator that
`conv_check f32` (tests/test_gpu_native.py) holds the exact-f32 inference kernels to, bit for bit.

tests/native/f32_ref_selftest.cpp (host pass only) runs, per shape and data mode (int, round, widex,
widew), bf16_ref.h's int64 reference with nothing rounded, the f32 emulator of the kernels'
arithmetic, and the emulator with seven slips:
  a  one 32-channel k-step of one tap dropped for one 64-pixel x 64-cout tile
  b  a padding tap reads the neighbouring row or column instead of zero
  d  the residual is added after the ReLU
  f  the fused downsample reads x2 at (oh, ow) instead of (s2 oh, s2 ow)
  g  both operands truncated to bf16 (8 significant bits) before the product
  h  both operands truncated to a 10-bit mantissa (10 significant bits)
  i  both operands truncated to 10 stored mantissa bits (11 significant bits, tf32)
The unmutated emulator must equal the reference bitwise in all four modes, and every slip must
change an output wherever it applies.  The pairs that cannot differ are asserted SAME, so that they
stay the only blind spots: (b) without padding, (d) without a residual, (f) without a strided
downsample; (g) and (h) in int and round mode, whose operands have at most 4 significant bits --
which is why the wide modes exist: there one operand has up to 11 bits and both slips show; and (i)
in every mode, because 11 significant bits hold every |v| <= 2047 and a wider operand would break
sum |terms| < 2^24 at the largest K."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("int", "round", "widex", "widew")
SLIPS = ("a_drop_kstep", "b_pad_neighbour", "d_res_after_relu", "f_ds_no_stride", "g_operands_bf16", "h_operands_mant10",
         "i_operands_tf32")
# shape -> what it has: padding taps, a residual, a strided downsample
SHAPES = {
    "1x1_64_64_5x7_res": dict(pad=False, res=True, ds2=False),
    "3x3_64_96_6x10_res": dict(pad=True, res=True, ds2=False),
    "3x3s2_32_64_9x11_ds2_res": dict(pad=True, res=True, ds2=True),
    "3x3_512_8_3x3_ds2_256_res": dict(pad=True, res=True, ds2=True),  # the largest K: 4608 + 256
    "stem_pool_20x18": dict(pad=True, res=False, ds2=False),
}


def applies(slip, shape, mode):
    has = SHAPES[shape]
    wide = mode in ("widex", "widew")
    return {"a": True, "b": has["pad"], "d": has["res"], "f": has["ds2"], "g": wide, "h": wide, "i": False}[slip[0]]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("f32_ref") / "f32_ref_selftest")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-w",
                    os.path.join(REPO, "tests", "native", "f32_ref_selftest.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    out, cond = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "cond":
            cond[(f[1], f[2])] = {f[i]: int(f[i + 1]) for i in range(3, len(f), 2)}
        else:
            out[(f[0], f[1], f[2])] = dict(verdict=f[3], differing=int(f[5]), total=int(f[7]))
    assert len(out) == len(SHAPES) * len(MODES) * (1 + len(SLIPS)) and len(cond) == len(SHAPES) * len(MODES), r.stdout
    return out, cond


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_data_conditions(selftest, shape, mode):
    """At every output the reference's upper bound of the sum of |terms| (bias and residual
    included) is below 2^24, so f32 accumulation is exact in any order -- also at the largest K the
    f32 kernels take, in the wide modes."""
    c = selftest[1][(shape, mode)]
    assert c["outputs"] > 0 and c["violations"] == 0 and c["max_sabs"] < 2 ** 24, c
    if mode in ("widex", "widew") and shape != "stem_pool_20x18":
        assert c["max_sabs"] > 2047, c  # the wide operand is there


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_emulator_equals_reference(selftest, shape, mode):
    r = selftest[0][(shape, mode, "none")]
    assert r["verdict"] == "EQUAL" and r["differing"] == 0 and r["total"] > 0, r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slip", SLIPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_slip_changes_an_output_where_it_applies(selftest, shape, slip, mode):
    r = selftest[0][(shape, mode, slip)]
    print(f"{shape} {mode} {slip}: {r['verdict']} {r['differing']} of {r['total']} outputs differ")
    if applies(slip, shape, mode):
        assert r["verdict"] == "DIFF" and r["differing"] > 0, r
    else:
        assert r["verdict"] == "SAME" and r["differing"] == 0, r
