"""Layer-level native checks on the GPU: tests/native/conv_check (built by
__graft_entry__.build()) runs every bf16 / f32 conv kernel family of libeosv.so on
seeded random operands against a double-precision CPU conv, including the zero-padding
taps, M tails, stride-2 entries, 1x1 convs, both K orders, and the fused stem + pool.
`conv_check x3 <group>` holds the f32x3 instantiations to a derived bound on probe data, and
`conv_check bf16 <group>` the bf16 inference kernels to bitwise equality with an int64 reference on
integer data, and `conv_check f32 <group>` does the same for the exact-f32 inference kernels."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "conv_check")


def test_conv_check():
    if not os.path.exists(BIN):
        pytest.fail("tests/native/conv_check missing: run __graft_entry__.build()")
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "\n0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# group -> timeout (s): a group is a few launches plus its double-precision host convs, 1-2 s each
X3_GROUPS = {"rows": 60, "ts": 60, "g64": 30, "g128": 60, "g256": 90, "stem": 60, "layout": 30}


@pytest.mark.parametrize("group", list(X3_GROUPS))
def test_conv_check_x3(group):
    """`conv_check x3 <group>`: the f32x3 (ConvArgs::split) instantiations kernel by kernel --
    conv_rows_x3, the tap-shift 512x64 / 512x128 tiles, conv_bf16_kernel's 256x64, 512x128 and
    256x256 tiles (one ring, split rings, fused downsample), the split f32 stem -- and the layout
    kernels, against tests/native/x3_ref.h: a double reference on the stored values, probe data
    (independent O(1) hi and lo blocks, so a dropped or mis-paired k-step is an O(0.1) error), the
    derived bound 2e-6 (1 + sum |terms|) + 2^-17 |ref|, a guard behind every output, and the planned
    grid pinned to the tile each case is meant for."""
    if not os.path.exists(BIN):
        pytest.fail("tests/native/conv_check missing: run __graft_entry__.build()")
    r = subprocess.run([BIN, "x3", group], capture_output=True, text=True, timeout=X3_GROUPS[group])
    print(r.stdout)
    assert r.returncode == 0 and "\n0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# group -> timeout (s): about ten times the group's measured time on the MI355X, host reference
# included (rows 1.7 s, gemm 0.5, pair 2.0, pairw2 4.2, pairw3 2.1, block 1.9, stem 0.5; DESIGN.md
# section 3B), rounded up to a multiple of 30
BF16_GROUPS = {"rows": 30, "gemm": 30, "pair": 30, "pairw2": 60, "pairw3": 30, "block": 30, "stem": 30}


@pytest.mark.parametrize("group", list(BF16_GROUPS))
def test_conv_check_bf16(group):
    """`conv_check bf16 <group>`: the bf16 inference kernels one by one -- the row-strip kernels, the
    tap-shift kernel, the warp-specialised 512x128 and 256x256 tiles and the 128x64 tile, the fused
    1x1 pairs, the whole-block stage-1 kernels and the fused stem + pool -- bit for bit against
    tests/native/bf16_ref.h: an int64 reference on integer operands (every product and partial sum
    exact in f32, so the one rounding left is the RNE conversion of the output, which `round` mode
    exercises on exact ties), every output of every image, 0xff guards before and behind every
    output, every launch twice, and the planned grid pinned to the kernel each case is meant for
    (tests/test_cpu_bf16_ref.py shows what the data reject)."""
    if not os.path.exists(BIN):
        pytest.fail("tests/native/conv_check missing: run __graft_entry__.build()")
    r = subprocess.run([BIN, "bf16", group], capture_output=True, text=True, timeout=BF16_GROUPS[group])
    print(r.stdout)
    assert r.returncode == 0 and "\n0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# group -> timeout (s): about ten times the group's measured time on the MI355X, host reference
# included (rows 0.7 s, c64 0.5, t64 0.3, ws256 2.3, ws256k 1.7, ws128 1.2, ksplit 2.2, head 0.3, stem 0.3,
# refuse 0.2), rounded up to a multiple of 30
F32_GROUPS = {"rows": 30, "c64": 30, "t64": 30, "ws256": 30, "ws256k": 30, "ws128": 30, "ksplit": 30, "head": 30, "stem": 30,
              "refuse": 30}


@pytest.mark.parametrize("group", list(F32_GROUPS))
def test_conv_check_f32(group):
    """`conv_check f32 <group>`: the exact-f32 inference kernels one by one -- conv_rows_f32_kernel,
    conv_f32_dma_kernel's 256x64 and 128x64 tiles (plain, fused downsample, the stem form and the
    per-element epilogue of the fc head), conv_f32_ws_kernel's 256x128 and 128x128 tiles (plain and
    fused downsample), the training entry's split-K on the 256x128 and 128x128 DMA tiles,
    stem_pool_f32_kernel at every column-tile count 1..8 (pack, direct, split) and every refusal of
    the three launchers -- bit for bit against tests/native/f32_ref.h: bf16_ref.h's
    int64 reference on integer operands (every product and partial sum exact in f32 and the f32 output
    not converted, so there is no rounding at all), in the int and widex data modes (one shape per
    group also in round and widew), every output of every image, 0xff guards before and behind every
    output, every launch twice, ConvArgs::xcd = 1 as the engine sets it (ragged grids also with 0),
    and the planned grid pinned to the kernel each case is meant for (DESIGN.md section 3F;
    tests/test_cpu_f32_ref.py shows what the data reject)."""
    if not os.path.exists(BIN):
        pytest.fail("tests/native/conv_check missing: run __graft_entry__.build()")
    r = subprocess.run([BIN, "f32", group], capture_output=True, text=True, timeout=F32_GROUPS[group])
    print(r.stdout)
    assert r.returncode == 0 and "\n0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
