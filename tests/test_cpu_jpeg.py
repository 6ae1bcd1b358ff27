"""CPU: host stage of the library's JPEG decoder (csrc/jpeg_host.hip: eosv_jpeg_scan,
eosv_jpeg_entropy; no device call) against PIL.

The files are written with PIL; the library's coefficients and quantisation tables go through the
numpy restatement of the GPU stage's pixel arithmetic (tests/_jpeg_np.py) and must equal
np.asarray(Image.open(f).convert('RGB')) in every byte: all of it is libjpeg's integer arithmetic,
so no tolerance exists.  Also: results independent of the thread count, refusals (progressive,
4:2:2, CMYK, no JPEG at all) that leave the other frames of the call alone, and the same two entry
points under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/native/jpeg_host_check.cpp) over intact, truncated and corrupted files."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import _jpeg_np
from eosv import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (9, 9), (16, 16), (17, 33), (33, 17), (70, 50), (320, 240)]  # w x h
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def content(kind, w, h, seed=0):
    rng = np.random.default_rng(seed + 1000 * w + h)
    if kind == "noise":  # uniform noise: every clamp of the IDCT and the colour conversion
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "smooth":  # 8x8 flat tiles: DC-only blocks
        t = rng.integers(0, 256, size=(-(-h // 8), -(-w // 8), 3), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:h, :w])
    if kind == "texture":  # a gradient with mild noise, like a camera frame
        g = np.linspace(0, 200, w)[None, :, None] + np.linspace(0, 40, h)[:, None, None]
        return np.clip(g + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return np.full((h, w, 3), {"black": 0, "white": 255}[kind], np.uint8)


def encode(a, mode="RGB", **kw):
    img = Image.fromarray(a[:, :, 0].copy()) if mode == "L" else Image.fromarray(a)
    if mode == "CMYK":
        img = img.convert("CMYK")
    b = io.BytesIO()
    img.save(b, "JPEG", **kw)
    return b.getvalue()


def pil_rgb(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def check_equal(blobs, threads=4):
    scan = _jpeg_np.Scan(blobs)
    assert scan.status() == [0] * len(blobs)
    coef, quant, offs = scan.entropy(threads, guard=256)
    assert scan.status() == [0] * len(blobs)
    for i, b in enumerate(blobs):
        ref = pil_rgb(b)
        f = scan.frames[i]
        assert (f.height, f.width) == ref.shape[:2]
        got = scan.image(i, coef, quant, offs)
        assert got.dtype == np.uint8 and np.array_equal(got, ref), f"frame {i}: {ref.shape}"


FORMATS = {"420": dict(subsampling=2), "444": dict(subsampling=0), "grey": dict()}


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("quality", [20, 75, 90, 100])
def test_every_size_equals_pil(fmt, quality):
    mode = "L" if fmt == "grey" else "RGB"
    check_equal([encode(content("noise", w, h, quality), mode, quality=quality, **FORMATS[fmt]) for w, h in SIZES])


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_encoder_options_equal_pil(fmt):
    """Optimised Huffman tables, restart intervals by MCU row and by block count, a COM segment."""
    mode = "L" if fmt == "grey" else "RGB"
    blobs = []
    for w, h in SIZES:
        # PIL's encoder cannot hold an optimised 4:4:4 file of 320x240 noise in its output buffer
        a = content("noise" if w < 320 else "texture", w, h, 7)
        for kw in (dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=3),
                   dict(comment=b"a comment segment"), dict(optimize=True, restart_marker_blocks=3, comment=b"xy")):
            blobs.append(encode(a, mode, quality=90, **kw, **FORMATS[fmt]))
    assert b"\xff\xdd" in blobs[1] and b"\xff\xfe" in blobs[3]  # DRI and COM are really there
    check_equal(blobs)


@pytest.mark.parametrize("kind", ["smooth", "texture", "black", "white"])
def test_content_kinds_equal_pil(kind):
    blobs = []
    for w, h in SIZES:
        for fmt, mode in (("420", "RGB"), ("444", "RGB"), ("grey", "L")):
            blobs.append(encode(content(kind, w, h), mode, quality=90, **FORMATS[fmt]))
    check_equal(blobs)


def mixed_batch():
    blobs = []
    for k, (w, h) in enumerate(SIZES * 3):
        fmt = list(FORMATS)[k % 3]
        kw = dict(restart_marker_blocks=5) if k % 4 == 1 else dict(optimize=bool(k % 2))
        blobs.append(encode(content("noise" if k % 2 else "texture", w, h, k), "L" if fmt == "grey" else "RGB",
                            quality=(20, 75, 90, 100)[k % 4], **kw, **FORMATS[fmt]))
    return blobs


def test_thread_count_does_not_change_the_result():
    blobs = mixed_batch()
    got = []
    for t in (1, 3, 16):
        scan = _jpeg_np.Scan(blobs)
        coef, quant, offs = scan.entropy(t, guard=64)
        assert scan.status() == [0] * len(blobs)
        got.append((coef.tobytes(), quant.tobytes(), offs))
    assert got[0] == got[1] == got[2]
    # out-of-range counts are clamped, not refused
    scan = _jpeg_np.Scan(blobs)
    assert scan.entropy(0)[0].tobytes() == got[0][0] and scan.entropy(1000)[0].tobytes() == got[0][0]


def test_refusals_leave_the_other_frames_alone():
    a = content("noise", 70, 50)
    good = encode(a, quality=90)
    rng = np.random.default_rng(5)
    blobs = [good,
             encode(a, quality=90, progressive=True),
             encode(a, quality=90, subsampling=1),  # 4:2:2
             encode(a, "CMYK", quality=90),
             rng.integers(0, 256, size=2000, dtype=np.uint8).tobytes(),
             b"",
             good[:len(good) // 2],  # header intact, stream cut
             good[:20],              # header cut
             encode(content("noise", 33, 17), quality=75, subsampling=0)]
    scan = _jpeg_np.Scan(blobs)
    assert scan.status() == [0, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_ARG, ERR_ARG, 0, ERR_ARG, 0]
    coef, quant, offs = scan.entropy(3, guard=64)
    assert scan.status() == [0, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_ARG, ERR_ARG, ERR_ARG, ERR_ARG, 0]
    for i in (0, 8):
        assert np.array_equal(scan.image(i, coef, quant, offs), pil_rgb(blobs[i]))


def test_broken_restart_marker_and_range_are_refused():
    good = encode(content("noise", 70, 50), quality=90, restart_marker_blocks=3)
    i = good.index(b"\xff\xd1")
    wrong = good[:i] + b"\xff\xd3" + good[i + 2:]  # RST3 where RST1 belongs
    gone = good[:i] + good[i + 2:]  # the marker dropped
    scan = _jpeg_np.Scan([good, wrong, gone])
    assert scan.status() == [0, 0, 0]
    scan.entropy(2, guard=64)
    assert scan.status() == [0, ERR_ARG, ERR_ARG]
    # a frame whose range does not fit the buffer is refused, and nothing is written for it
    scan = _jpeg_np.Scan([good])
    n = scan.frames[0].coef_elems
    scan.frames[0].coef_offset = 64
    coef = np.full(n + 64, 0x5A5A, np.int16)
    quant = np.zeros((1, 3, 64), np.uint16)
    assert _lib.lib().eosv_jpeg_entropy(scan.data, scan.nbytes, 1, scan.frames, coef.ctypes.data, n, quant.ctypes.data,
                                        1) == 0
    assert scan.frames[0].status == ERR_ARG and (coef == 0x5A5A).all()


def test_entry_points_reject_null_arguments():
    L = _lib.lib()
    assert L.eosv_jpeg_scan(None, None, 0, None) == 0
    assert L.eosv_jpeg_scan(None, None, 1, None) == ERR_ARG
    assert b"eosv_jpeg_scan" in L.eosv_last_error()
    assert L.eosv_jpeg_entropy(None, None, 1, None, None, 0, None, 1) == ERR_ARG
    assert L.eosv_jpeg_entropy(None, None, 0, None, None, 0, None, 1) == 0
    # the GPU stage checks its arguments before any device call: these run without a GPU
    m = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    d = (_lib.EosvJpegDesc * 1)()
    d[0].width, d[0].height, d[0].sampling = 70, 50, _lib.JPEG_420
    assert L.eosv_jpeg_render_workspace(d, 1) > 0
    assert L.eosv_jpeg_render(None, 0, None, None, 0, 32, m, m, None, None, 0, None) == 0  # empty
    assert L.eosv_jpeg_render(None, 0, None, d, 1, 32, m, m, None, None, 0, None) == ERR_ARG  # null pointers
    d[0].width = 5000
    assert L.eosv_jpeg_render_workspace(d, 1) == ERR_ARG
    assert L.eosv_jpeg_render_workspace(d, 70000) == ERR_ARG


def test_thread_default_ignores_the_core_count(monkeypatch):
    from eosv import engine

    monkeypatch.delenv("EOSV_JPEG_THREADS", raising=False)
    assert engine.jpeg_threads() == 8
    monkeypatch.setenv("EOSV_JPEG_THREADS", "3")
    assert engine.jpeg_threads() == 3
    monkeypatch.setenv("EOSV_JPEG_THREADS", "64")
    assert engine.jpeg_threads() == 16


# ----------------------------------------------------------------- host sanitizers, stand-alone
def checksum(coef, quant):
    n = coef.size
    s = (coef.view(np.uint16).astype(np.uint64) * (np.arange(n, dtype=np.uint64) % np.uint64(65521) + np.uint64(1))).sum(
        dtype=np.uint64)
    s += (quant.reshape(-1).astype(np.uint64) * (np.arange(192, dtype=np.uint64) + np.uint64(1000003))).sum(dtype=np.uint64)
    return int(s)


def test_host_stage_under_sanitizers(tmp_path):
    """tests/native/jpeg_host_check (address + undefined-behaviour sanitizers, its own main, the
    runtimes linked in): scan and entropy at 1 and 4 threads over the intact files, every prefix at a stride of
    97 bytes and 200 single-byte corruptions per file, the coefficient buffer between sentinels.  Every
    call returns a status, the sentinels hold, the sanitizers report nothing, and the checksums of the
    intact files equal the release library's."""
    src = os.path.join(REPO, "embodied-one-shot-video-recognition_amd", "csrc")
    subprocess.run(["make", "-s", "-C", src, "jpeg_check"], check=True, capture_output=True)
    files = {"a.jpg": encode(content("noise", 70, 50), quality=90, optimize=True),
             "b.jpg": encode(content("noise", 33, 17), quality=75, subsampling=0, restart_marker_blocks=3),
             "c.jpg": encode(content("texture", 50, 70), "L", quality=90, restart_marker_rows=1),
             "d.jpg": encode(content("texture", 320, 240), quality=90, comment=b"frame")}
    for name, b in files.items():
        (tmp_path / name).write_bytes(b)
    # the sanitizer runtimes are linked into the program: the environment is taken as it is
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(REPO, "tests", "native", "jpeg_host_check")] + [str(tmp_path / n) for n in files],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("jpeg_host_check: ok")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("OK ")]
    assert len(lines) == 2 * len(files)
    scan = _jpeg_np.Scan(list(files.values()))
    coef, quant, offs = scan.entropy(2)
    want = {}
    for i, name in enumerate(files):
        f = scan.frames[i]
        want[name] = [str(f.width), str(f.height), str(f.sampling),
                      str(checksum(coef[offs[i]:offs[i] + f.coef_elems], quant[i]))]
    for _, name, threads, *rest in lines:
        assert threads in ("1", "4") and rest == want[name], (name, threads)
