"""eosv_conv_wino_f32_grid (the Winograd conv on a capped workgroup count, for tests of the
persistent tile loop): declared, exported, and its argument checks, which return before any device
call."""
import os

from eosv import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096  # never dereferenced: the launcher returns first
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def test_grid_entry_is_declared_and_exported():
    assert "eosv_conv_wino_f32_grid" in _lib.EXPORTS
    with open(os.path.join(REPO, "include", "eosv.h")) as fh:
        header = fh.read()
    assert "int eosv_conv_wino_f32_grid(" in header
    assert hasattr(_lib.lib(), "eosv_conv_wino_f32_grid")


def test_grid_entry_rejects_bad_arguments():
    L = _lib.lib()
    for cap in (0, -1):
        assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, P, 1, 8, 8, 64, None, cap) == ERR_ARG
        assert b"max_workgroups" in L.eosv_last_error()
    assert L.eosv_conv_wino_f32_grid(None, P, None, None, 0, P, 1, 8, 8, 64, None, 4) == ERR_ARG
    assert L.eosv_conv_wino_f32_grid(P, None, None, None, 0, P, 1, 8, 8, 64, None, 4) == ERR_ARG
    assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, None, 1, 8, 8, 64, None, 4) == ERR_ARG
    assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, P, 0, 8, 8, 64, None, 4) == ERR_ARG


def test_grid_entry_refuses_what_the_plain_entry_refuses():
    L = _lib.lib()
    assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, P, 1, 8, 8, 96, None, 4) == ERR_UNSUPPORTED  # C % 64
    # 65 * 512 * 512 * 64 * 4 B > 2^32: the kernel's 32-bit patch offsets
    assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, P, 1, 512, 512, 64, None, 4) == ERR_UNSUPPORTED
    assert b"32-bit" in L.eosv_last_error()


def test_multiply_shift_division_matches_integer_division(tmp_path):
    """wino_div / wino_fdiv (csrc/common.h), the kernel's tile decode, against `/` on the host:
    tests/native/wino_div_check.cpp, host pass only, 5.5e7 (divisor, dividend) pairs below 2^31."""
    import subprocess

    exe = str(tmp_path / "wino_div_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-w",
                    "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "embodied-one-shot-video-recognition_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "wino_div_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
