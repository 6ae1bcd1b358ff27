"""GPU: the library's JPEG decoder (host entropy decode, csrc/jpeg_host.hip; inverse DCT, chroma
upsampling, colour, crop, flip, normalise on the GPU, csrc/jpeg.hip) against the PIL path, bit for bit.

  * engine.jpeg_frames == engine.crop_normalize_frames on PIL's pixels of the same files (compared
    as uint32), at the smallest shapes that reach every rule of the pixel arithmetic;
  * JpegFrames(native) == JpegFrames(PIL) through utils.get_video_from_video_info_3 in test and train
    mode, RNG state included, for normal, narrow, crop-sized, short and partly progressive clips;
  * JpegFrames.clips_tensor: a batch of clips in one decode, fallbacks whole, == the driver's table;
  * TestNetwork.test_network_baseline over a JPEG tree with EOSV_JPEG_DECODE=native == without it.

All of it is integer arithmetic followed by the same three correctly rounded f32 operations, so
equality is the only tolerance."""
import io
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

FORMATS = {"420": ("RGB", dict(subsampling=2)), "444": ("RGB", dict(subsampling=0)), "grey": ("L", dict()),
           "420-rst": ("RGB", dict(subsampling=2, restart_marker_rows=1)),
           "444-rst": ("RGB", dict(subsampling=0, restart_marker_blocks=3))}

# (w, h, crop, [(top, left)]): crop = the image (all four edges, odd sizes, the last-column rule);
# both extreme offsets of a window as high / as wide as the image; odd and even offsets (both chroma
# phases, vertically and horizontally); the product shape centred and at its four corners
CASES = [(17, 17, 17, [(0, 0)]), (9, 9, 9, [(0, 0)]),
         (33, 17, 17, [(0, 0), (0, 16)]), (17, 33, 17, [(0, 0), (16, 0)]),
         (70, 50, 32, [(0, 0), (1, 1), (18, 38), (17, 37), (6, 11), (7, 10)]),
         (320, 240, 224, [(8, 48), (0, 0), (0, 96), (16, 0), (16, 96)])]


def noise(w, h, seed):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def encode(a, fmt, quality=90):
    mode, kw = FORMATS[fmt]
    img = Image.fromarray(a[:, :, 0].copy()) if mode == "L" else Image.fromarray(a)
    b = io.BytesIO()
    img.save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def pil_reference(blob, crop, top, left, flip):
    """[3,crop,crop] f32 (device): the PIL path on the same file."""
    from eosv import engine

    rgb = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
    return engine.crop_normalize_frames(torch.from_numpy(rgb[None].copy()).cuda(), crop, top, left, flip)[0]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("w,h,crop,windows", CASES)
def test_kernel_equals_pil_path(fmt, w, h, crop, windows):
    from eosv import engine

    blob = encode(noise(w, h, 1), fmt)
    blobs, wins, flips = [], [], []
    for win in windows:
        for flip in (False, True):
            blobs.append(blob)
            wins.append(win)
            flips.append(flip)
    got = engine.jpeg_frames(blobs, crop, wins, flips)
    assert got.is_cuda and tuple(got.shape) == (len(blobs), 3, crop, crop)
    for i, (win, flip) in enumerate(zip(wins, flips)):
        assert same_bits(got[i], pil_reference(blob, crop, win[0], win[1], flip)), (win, flip)
    if len(windows) > 1:  # the centre window is the default
        assert same_bits(engine.jpeg_frames([blob], crop)[0],
                         pil_reference(blob, crop, int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0)), False))


def test_one_call_mixes_sizes_formats_and_windows_between_sentinels():
    from eosv import engine

    crop = 9
    rng = np.random.default_rng(4)
    blobs, wins, flips = [], [], []
    for k, (w, h, _, _) in enumerate(CASES * 2):
        fmt = list(FORMATS)[k % len(FORMATS)]
        blobs.append(encode(noise(w, h, k), fmt, quality=(20, 75, 90, 100)[k % 4]))
        wins.append((int(rng.integers(0, h - crop + 1)), int(rng.integers(0, w - crop + 1))))
        flips.append(bool(k % 2))
    n, guard = len(blobs), 4096
    buf = torch.full((guard * 2 + n * 3 * crop * crop,), float("nan"), device="cuda")
    out = buf[guard:guard + n * 3 * crop * crop].view(n, 3, crop, crop)
    got = engine.jpeg_frames(blobs, crop, wins, flips, out=out, threads=3)
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n * 3 * crop * crop:]).all())
    for i in range(n):
        assert same_bits(got[i], pil_reference(blobs[i], crop, wins[i][0], wins[i][1], flips[i])), i


def test_empty_call_and_window_past_the_frame():
    from eosv import _lib, engine

    assert tuple(engine.jpeg_frames([], 32).shape) == (0, 3, 32, 32)
    blob = encode(noise(70, 50, 2), "420")
    out = torch.full((1, 3, 32, 32), float("nan"), device="cuda")
    for win in ((19, 0), (0, 39), (-1, 0)):
        with pytest.raises(_lib.EosvError, match="window"):
            engine.jpeg_frames([blob], 32, win, False, out=out)
    with pytest.raises(_lib.EosvError):  # a crop larger than the frame
        engine.jpeg_frames([blob], 64, out=torch.full((1, 3, 64, 64), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # refused before any launch: nothing written
    prog = io.BytesIO()
    Image.fromarray(noise(70, 50, 2)).save(prog, "JPEG", progressive=True)
    with pytest.raises(_lib.EosvError, match="refused"):
        engine.jpeg_frames([blob, prog.getvalue()], 32)


# ----------------------------------------------------------------- the loaders
# (video, width, height, frames on disk): normal, narrow (resized on the host: PIL path), exactly
# crop-sized (the train window draws nothing), short (zero padding), one progressive frame (PIL path)
VIDEOS = [("walk/v_a", 320, 240, 20), ("walk/v_narrow", 200, 150, 18), ("run/v_exact", 224, 224, 18),
          ("run/v_short", 300, 260, 9), ("run/v_prog", 320, 240, 18)]
NATIVE = {"walk/v_a": True, "walk/v_narrow": False, "run/v_exact": True, "run/v_short": True, "run/v_prog": False}


@pytest.fixture(scope="module")
def frame_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_frames")
    rng = np.random.default_rng(21)
    for vi, w, h, n in VIDEOS:
        d = root / vi
        d.mkdir(parents=True)
        base = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        for f in range(1, n + 1):
            a = np.clip(base.astype(np.int16) + rng.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(a).save(d / ("image_%05d.jpg" % f), quality=90,
                                    progressive=(vi == "run/v_prog" and f == 7))
        (d / "extra.txt").write_text("x")  # the reference counts listdir() - 1
    return str(root)


@pytest.mark.parametrize("mode", ["test", "train"])
@pytest.mark.parametrize("vi", [v[0] for v in VIDEOS])
def test_loader_native_equals_pil(frame_dir, vi, mode, monkeypatch):
    import utils
    from eosv import engine

    T = 16
    calls = []
    real = engine.jpeg_frames

    def spy(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)

    monkeypatch.setattr(engine, "jpeg_frames", spy)
    res = {}
    for native in (False, True):
        if native:
            monkeypatch.setenv("EOSV_JPEG_DECODE", "native")
        else:
            monkeypatch.delenv("EOSV_JPEG_DECODE", raising=False)
        random.seed(7)
        torch.manual_seed(7)
        v, n = utils.get_video_from_video_info_3(vi, mode, video_frames=T, frame_dir=frame_dir)
        res[native] = (v, int(n), random.getstate(), torch.get_rng_state())
        if not native:
            assert calls == []  # off by default
    a, b = res[False], res[True]
    assert b[0].is_cuda and tuple(b[0].shape) == (T, 3, 224, 224)
    assert same_bits(a[0], b[0]) and a[1] == b[1]
    assert a[2] == b[2] and torch.equal(a[3], b[3])  # the same draws from both RNGs
    assert calls == ([min(T, dict((v[0], v[3]) for v in VIDEOS)[vi])] if NATIVE[vi] else [])


def test_source_switch(frame_dir, monkeypatch):
    from eosv import frames as fr

    monkeypatch.delenv("EOSV_JPEG_DECODE", raising=False)
    assert not fr.JpegFrames(frame_dir).native and fr.JpegFrames(frame_dir, native=True).native
    monkeypatch.setenv("EOSV_JPEG_DECODE", "native")
    assert fr.JpegFrames(frame_dir).native
    src = fr.JpegFrames(frame_dir, native=True)
    ids = list(range(3, 12))
    a = src.frames_tensor("walk/v_a", ids, "test")
    b = fr.JpegFrames(frame_dir, native=False)
    monkeypatch.delenv("EOSV_JPEG_DECODE")
    assert same_bits(a, b.frames_tensor("walk/v_a", ids, "test"))


def test_clip_frames_with_the_switch_on(frame_dir, monkeypatch):
    """network_test._clip_frames (unchanged) with the switch on: every wide clip decodes natively,
    the narrow one through PIL, padded rows stay zero, and the frames are those of the PIL path."""
    import network_test
    import utils
    from eosv import engine

    monkeypatch.setattr(utils, "KINETICS_FRAME_DIR", frame_dir)
    dev = torch.device("cuda", torch.cuda.current_device())
    clips = [("walk/v_a", list(range(3, 19)), 16), ("run/v_short", list(range(1, 10)), 16), ("run/v_exact", [5, 6], 2),
             ("walk/v_narrow", list(range(2, 18)), 16)]
    monkeypatch.delenv("EOSV_JPEG_DECODE", raising=False)
    ref = network_test.TestNetwork._clip_frames(None, clips, 224, 224, dev)
    calls = []
    real = engine.jpeg_frames

    def spy(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)

    monkeypatch.setattr(engine, "jpeg_frames", spy)
    monkeypatch.setenv("EOSV_JPEG_DECODE", "native")
    got = network_test.TestNetwork._clip_frames(None, clips, 224, 224, dev)
    assert calls == [16, 9, 2] and tuple(got.shape) == (50, 3, 224, 224) and same_bits(got, ref)
    assert not bool(got[25:32].any())  # the short clip's padding


def test_clips_tensor_decodes_a_batch_in_one_call(frame_dir, monkeypatch):
    """JpegFrames.clips_tensor: every clip the native route can take goes through ONE jpeg_frames call
    into its rows, padding rows stay zero; the narrow and the partly progressive clip fall back whole
    to PIL; a stream that breaks in the entropy decode sends every clip to PIL; the table always
    equals the one the unchanged driver builds clip by clip without the switch."""
    import network_test
    import utils
    from eosv import engine, frames as fr

    monkeypatch.setattr(utils, "KINETICS_FRAME_DIR", frame_dir)
    dev = torch.device("cuda", torch.cuda.current_device())
    wide = [("walk/v_a", list(range(3, 19)), 16), ("run/v_short", list(range(1, 10)), 16), ("run/v_exact", [5, 6], 2)]
    mixed = wide[:2] + [("walk/v_narrow", list(range(2, 18)), 16), ("run/v_prog", list(range(2, 18)), 17), wide[2]]
    monkeypatch.delenv("EOSV_JPEG_DECODE", raising=False)
    ref_wide = network_test.TestNetwork._clip_frames(None, wide, 224, 224, dev)
    ref_mixed = network_test.TestNetwork._clip_frames(None, mixed, 224, 224, dev)
    calls = []
    real = engine.jpeg_frames

    def spy(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)

    monkeypatch.setattr(engine, "jpeg_frames", spy)
    assert same_bits(fr.JpegFrames(frame_dir).clips_tensor(wide, dev), ref_wide) and calls == []  # off by default
    src = fr.JpegFrames(frame_dir, native=True)
    got = src.clips_tensor(wide, dev)
    assert calls == [16 + 9 + 2] and tuple(got.shape) == (34, 3, 224, 224) and same_bits(got, ref_wide)
    assert not bool(got[25:32].any())  # the short clip's padding
    del calls[:]
    got = src.clips_tensor(mixed, dev)
    assert calls == [16 + 9 + 2] and same_bits(got, ref_mixed)  # one call for the three wide clips
    assert not bool(got[25:32].any()) and not bool(got[64].any())
    # a stream cut short passes the header scan and fails in the entropy decode: all clips through PIL,
    # which raises on that file as it does without the switch
    import shutil
    bad = os.path.join(frame_dir, "walk", "v_cut")
    shutil.copytree(os.path.join(frame_dir, "walk", "v_a"), bad)
    p = os.path.join(bad, "image_00004.jpg")
    blob = open(p, "rb").read()
    open(p, "wb").write(blob[:len(blob) // 2])
    del calls[:]
    with pytest.raises(OSError):
        src.clips_tensor(wide[1:] + [("walk/v_cut", [3, 4, 5], 3)], dev)
    assert calls == [9 + 2 + 3]
    shutil.rmtree(bad)


# ----------------------------------------------------------------- end to end
# every frame at least crop wide, two sizes: every clip of the batch decodes natively
E2E = [(f"c{c}/v{v}", 320 if (c + v) % 3 else 256, 240 if (c + v) % 3 else 230, 20 if v else 17)
       for c in range(6) for v in range(2)]
E2E[3] = ("c1/v1", 320, 240, 10)  # a short clip


@pytest.fixture(scope="module")
def e2e_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeg_e2e")
    rng = np.random.default_rng(22)
    for vi, w, h, n in E2E:
        d = root / vi
        d.mkdir(parents=True)
        cls = np.random.default_rng(int(vi[1])).integers(0, 256, size=(h, w, 3))
        for f in range(1, n + 1):
            a = np.clip(cls + rng.integers(-60, 61, size=(h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(a).save(d / ("image_%05d.jpg" % f), quality=90)
        (d / "extra.txt").write_text("x")
    (root / "test.list").write_text("".join(vi + "\n" for vi, *_ in E2E))
    return str(root)


def test_network_baseline_native_equals_pil(e2e_dir, tmp_path, monkeypatch):
    """TestNetwork.test_network_baseline (2 episodes, ResNet-18, one batch) over a JPEG tree with
    two frame sizes and a short clip: predictions and clip embeddings with EOSV_JPEG_DECODE=native are
    those of the run without it, bit for bit, and every clip of the batch decodes natively."""
    import network_test
    import utils
    from eosv import arch, engine, synth

    monkeypatch.setattr(utils, "TEST_LIST", os.path.join(e2e_dir, "test.list"))
    monkeypatch.setattr(utils, "KINETICS_FRAME_DIR", e2e_dir)
    monkeypatch.setitem(utils.EPISODE_NUMS, "test", 2)
    sd = synth.synth_state_dict(arch.SPECS["resnet18"], 64, 0)
    pkl = str(tmp_path / "model.pkl")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, pkl)
    calls = []
    real = engine.jpeg_frames

    def spy(*a, **k):
        calls.append(len(a[0]))
        return real(*a, **k)

    monkeypatch.setattr(engine, "jpeg_frames", spy)
    runs = {}
    for native in (False, True):
        if native:
            monkeypatch.setenv("EOSV_JPEG_DECODE", "native")
        else:
            monkeypatch.delenv("EOSV_JPEG_DECODE", raising=False)
        random.seed(5)
        tn = network_test.TestNetwork(str(tmp_path / f"acc{int(native)}.txt"), "resnet18", "protonet", True)
        tn.episodes_per_batch = 2
        tn.debug = {}
        tn.test_network_baseline(pre_model=pkl)
        tn.acc_file.close()
        runs[native] = ([int(p) for p in tn.last_preds], tn.debug["batches"])
        if not native:
            assert calls == []
    assert len(calls) == 12 and min(calls) >= 10, calls  # 2 episodes x (5 supports + 1 query), no fallback
    assert runs[True][0] == runs[False][0]
    assert len(runs[True][1]) == len(runs[False][1]) == 1
    for a, b in zip(runs[True][1], runs[False][1]):
        assert same_bits(a["sup"], b["sup"]) and same_bits(a["q"], b["q"]) and torch.equal(a["pred"], b["pred"])
