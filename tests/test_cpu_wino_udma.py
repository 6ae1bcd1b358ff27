"""conv_wino_f32_kernel's U DMA goes through one buffer resource on U with a 32-bit scalar slab
offset (csrc/conv_wino_f32.hip, dma_piece): the launcher refuses a U of 2^32 bytes or more before
any device call, and the kernel's assembly holds the buffer form of the LDS-DMA with no vmcnt(0)
in its K loop (hipcc's own waits)."""
import os
import re
import subprocess
import sys

from eosv import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "embodied-one-shot-video-recognition_amd", "csrc")
P = 4096  # never dereferenced: the launcher returns first
ERR_UNSUPPORTED = -4


def test_u_of_four_gib_is_refused_before_any_launch():
    L = _lib.lib()
    C = 8192  # 16 * C * C * 4 B = 2^32; 65 frames of 2 x 2 x C floats are 8.5 MB
    assert L.eosv_conv_wino_f32(P, P, None, None, 0, P, 1, 2, 2, C, None) == ERR_UNSUPPORTED
    assert b"U exceeds 32-bit" in L.eosv_last_error()
    assert L.eosv_conv_wino_f32_grid(P, P, None, None, 0, P, 1, 2, 2, C, None, 4) == ERR_UNSUPPORTED
    assert b"U exceeds 32-bit" in L.eosv_last_error()


def test_k_loop_dma_is_the_buffer_form_with_counted_waits(tmp_path):
    """Device-only assembly of the kernel, as the library builds it: the K loop (tools/kloop_census.py
    finds it) holds 8 LDS-DMA pieces per two chunks, all of them buffer loads, no flat
    global_load_lds, exactly two vmcnt waits, both counted (12), and no 64-bit vector address add."""
    asm = str(tmp_path / "wino.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
                    "-I", os.path.join(REPO, "include"), "--cuda-device-only", "-S",
                    os.path.join(CSRC, "conv_wino_f32.hip"), "-o", asm], check=True, timeout=600,
                   stderr=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import kloop_census
    finally:
        sys.path.pop(0)
    for kernel in ("_ZN4eosv20conv_wino_f32_kernelILb0EEEvNS_8WinoArgsE", "_ZN4eosv20conv_wino_f32_kernelILb1EEEvNS_8WinoArgsE"):
        body = kloop_census.loop_body(asm, kernel)
        dma = [(op, rest) for op, rest in body if kloop_census.classify(op, rest) == "LDS-DMA"]
        assert len(dma) == 8 and all(op == "buffer_load_dwordx4" for op, _ in dma), dma
        assert sorted(int(re.search(r"offset:(\d+)", rest).group(1)) if "offset:" in rest else 0 for _, rest in dma) == \
            [0, 0, 1024, 1024, 2048, 2048, 3072, 3072]
        waits = [rest for op, rest in body if op == "s_waitcnt" and "vmcnt" in rest]
        assert waits == ["vmcnt(12)", "vmcnt(12)"], waits
        assert not any(op == "v_lshl_add_u64" for op, _ in body)
