"""The V image of conv_wino_f32_kernel, [pos][h][tile][kp] with plane h rotated by four tiles
(csrc/conv_wino_f32.hip): tools/lds_sim.py's model of it must read conflict-free by ds_read_b128
(4 LDS cycles, one per lane group of 16) and store conflict-free by ds_write_b32 (one cycle per
group of 32 lanes), and the word every (tile, channel) is written to must be the word the MFMA
lane that consumes it reads."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim():
    spec = importlib.util.spec_from_file_location("lds_sim", os.path.join(REPO, "tools", "lds_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    return sim


def test_v_image_reads_and_writes_are_conflict_free():
    assert _sim().wino_v() == (4, 1)


def test_v_image_words_are_a_bijection_and_reads_meet_writes():
    # the kernel's expressions: writer (lt, lc), reader lane (h, r), tile half, component kp
    written = {}
    for lt in range(64):
        for lc in range(8):
            written[(lc & 1) * 256 + ((lt + 4 * (lc & 1)) & 63) * 4 + (lc >> 1)] = (lt, lc)
    assert sorted(written) == list(range(512))
    for h in range(2):
        for r in range(32):
            va = (h * 256 + (r + 4 * h) * 4, h * 256 + ((r + 32 + 4 * h) & 63) * 4)
            for half in range(2):
                assert va[half] % 4 == 0  # 16-byte aligned: one ds_read_b128
                for kp in range(4):
                    assert written[va[half] + kp] == (r + 32 * half, 2 * kp + h)
