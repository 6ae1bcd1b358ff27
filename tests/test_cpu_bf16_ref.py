"""tests/native/bf16_ref.h on the host: the integer data, the int64 reference and the emulator that
`conv_check bf16` (tests/test_gpu_native.py) holds the bf16 inference kernels to, bit for bit.

tests/native/bf16_ref_selftest.cpp (host pass only) runs, per shape and data mode, the int64
reference, the f32 emulator of the kernels' arithmetic, and the emulator with six slips:
  a  one 32-channel k-step of one tap dropped for one 64-pixel x 64-cout tile
  b  a padding tap reads the neighbouring row or column instead of zero
  c  the output conversion truncates instead of rounding to nearest even
  d  the residual is added after the ReLU
  e  in a fused chain the intermediate maps are not rounded to bf16
  f  the fused downsample reads x2 at (oh, ow) instead of (s2 oh, s2 ow)
The unmutated emulator must equal the reference bitwise, and every slip must change an output on
every shape that has what the slip touches; this shows without a GPU that a bitwise GPU comparison
on these data fails on these classes of bug.  The pairs that cannot differ are asserted SAME, so
that they stay the only blind spots: (c) and (e) in int mode (nothing rounds there, which is why
round mode exists), (b) without padding, (d) without a residual, (e) outside a chain, (f) without
a strided downsample."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("int", "round")
SLIPS = ("a_drop_kstep", "b_pad_neighbour", "c_truncate", "d_res_after_relu", "e_no_mid_round", "f_ds_no_stride")
# shape -> what it has: padding taps, a residual, a chain of convs, a strided downsample; and
# whether it is one conv (the 99 % condition of int mode is stated for those)
SHAPES = {
    "3x3_64_64_6x56_res": dict(pad=True, res=True, chain=False, ds2=False),
    "1x1_128_64_5x7_ds2_res": dict(pad=False, res=True, chain=False, ds2=True),
    "3x3_512_512_4x4_res": dict(pad=True, res=True, chain=False, ds2=False),
    "bneck_64_ds_4x56": dict(pad=True, res=False, chain=True, ds2=False),  # the downsample has stride 1
    "bneck_256_next_2x56": dict(pad=True, res=True, chain=True, ds2=False),
}


def applies(slip, shape, mode):
    has = SHAPES[shape]
    return {"a": True, "b": has["pad"], "c": mode == "round", "d": has["res"],
            "e": has["chain"] and mode == "round", "f": has["ds2"]}[slip[0]]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bf16_ref") / "bf16_ref_selftest")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-w",
                    os.path.join(REPO, "tests", "native", "bf16_ref_selftest.cpp"), "-o", exe], check=True, timeout=300)
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
    """At every output of every stage the int64 sum of |terms| (bias and residual included) is
    below 2^24, so f32 accumulation is exact in any order.  In int mode at least 99 % of the
    pre-rounding outputs are integers of magnitude <= 256, which bf16 holds exactly; in round
    mode at least 10 % lie outside, so the conversion has something to round."""
    c = selftest[1][(shape, mode)]
    assert c["violations"] == 0 and c["max_sabs"] < 2 ** 24, c
    if mode == "int":
        assert c["over256"] * 100 <= c["outputs"], c
    else:
        assert c["over256"] * 10 >= c["outputs"], c


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
