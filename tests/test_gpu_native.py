"""Layer-level native checks on the GPU: tests/native/conv_check (built by
__graft_entry__.build()) runs every bf16 / f32 conv kernel family of libeosv.so on
seeded random operands against a double-precision CPU conv, including the zero-padding
taps, M tails, stride-2 entries, 1x1 convs, both K orders, and the fused stem + pool."""
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
