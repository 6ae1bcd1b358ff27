#!/usr/bin/env python
"""Frame ingest from JPEG files: today's PIL path against the library's decoder, in one run.

Writes 512 frames (320x240, quality 90, 4:2:0, seeded camera-like content) to a temporary directory
and reports, per frame and as frames/s:

  (a) the PIL path: Image.open(...).convert('RGB') of every frame in this process, one upload,
      eosv_crop_normalize_frames (what JpegFrames does without the switch);
  (b) the native path at 1, 4, 8 and 16 entropy threads, split into scan + entropy (host clock),
      the H2D copy of the coefficients and the two kernels of eosv_jpeg_render (HIP events), all 512
      frames in one call;
  (c) the native path called per clip of 16 frames, as the loaders do (wall clock);
  (d) JpegFrames.clips_tensor over the 32 clips at once, file reads included (wall clock).

Both conditions the route has to meet are measured against (a) in the same run:
  1. entropy decode per frame on ONE thread below PIL's whole decode per frame;
  2. kernel time per frame below the host stage's time per frame at 16 threads.

    python tools/bench_ingest.py [--out profiles/jpeg_ingest.txt] [--host-only]

--host-only measures the host columns alone (no device needed); the report says so.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "embodied-one-shot-video-recognition_amd"))

N, W, H, CROP, REPEATS = 512, 320, 240, 224, 5


def write_frames(root):
    from PIL import Image

    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:H, 0:W]
    paths = []
    for f in range(N):
        # moving soft shapes over a gradient plus sensor-like noise: neither flat nor white noise
        g = 90 + 60 * np.sin((xx + 3 * f) / 37.0)[..., None] + 50 * np.cos((yy - 2 * f) / 23.0)[..., None]
        g = g + np.array([20, 0, -20]) + rng.normal(0, 6, size=(H, W, 3))
        p = os.path.join(root, "image_%05d.jpg" % (f + 1))
        Image.fromarray(np.clip(g, 0, 255).astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    return paths


def best(fn):
    """min over REPEATS of fn() -> tuple of seconds (after one warm-up call)."""
    fn()
    runs = [fn() for _ in range(REPEATS)]
    return tuple(min(r[k] for r in runs) for k in range(len(runs[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_ingest.txt"))
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()

    from PIL import Image

    from eosv import _lib, engine

    gpu = not args.host_only
    if gpu:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("no HIP device: use --host-only for the host columns")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as root:
        paths = write_frames(root)
        blobs = [open(p, "rb").read() for p in paths]
        say(f"# JPEG ingest: {N} frames {W}x{H}, quality 90, 4:2:0, mean file {sum(map(len, blobs)) / N / 1024:.1f} KiB; "
            f"crop {CROP}; best of {REPEATS} after a warm-up")
        say(f"# library {_lib.library_kind()} {_lib.source_digest()}; "
            + ("host columns and device columns from one run on the GPU host" if gpu else
               "HOST COLUMNS ONLY, measured on a CPU-only machine: no device time in this file"))
        top, left = int(round((H - CROP) / 2.0)), int(round((W - CROP) / 2.0))

        # ---- (a) the PIL path
        def pil_run():
            t0 = time.perf_counter()
            raw = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
            t1 = time.perf_counter()
            if not gpu:
                return (t1 - t0, 0.0)
            rgb = torch.from_numpy(np.ascontiguousarray(np.stack(raw))).cuda()
            engine.crop_normalize_frames(rgb, CROP, top, left, False)
            torch.cuda.synchronize()
            return (t1 - t0, time.perf_counter() - t1)

        dec, rest = best(pil_run)
        say()
        say("(a) PIL path (one process, as JpegFrames.decode)")
        say(f"    decode {dec / N * 1e6:8.1f} us/frame   stack + upload + crop_normalize {rest / N * 1e6:8.1f} us/frame"
            f"   total {N / (dec + rest):9.0f} frames/s")
        pil_decode = dec / N

        # ---- (b) the native path
        scan = engine.JpegScan(blobs)
        assert scan.ok()
        total = int(scan.rec["coef_elems"].sum())
        nbytes = total * 2 + N * 192 * 2
        if gpu:
            pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            dbuf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            out = torch.empty(N, 3, CROP, CROP, device="cuda")
        else:
            host = np.empty(nbytes, np.uint8)
        coef, quant = host[:total * 2].view(np.int16), host[total * 2:].view(np.uint16)
        say()
        say("(b) native path (files already in memory, as in (a) the page cache)")
        say("    threads   scan+entropy us/frame   H2D us/frame   kernels us/frame   host frames/s   path frames/s")
        host16 = kern = None
        for threads in (1, 4, 8, 16):
            def native_run():
                t0 = time.perf_counter()
                sc = engine.JpegScan(blobs)
                engine.jpeg_coefficients(sc, coef, quant, threads)
                t1 = time.perf_counter()
                if not gpu:
                    return (t1 - t0, 0.0, 0.0, t1 - t0)
                import ctypes

                desc = (_lib.EosvJpegDesc * N)()
                for i in range(N):
                    d = desc[i]
                    d.coef_offset, d.width, d.height = int(sc.rec["coef_offset"][i]), W, H
                    d.sampling, d.top, d.left, d.flip = int(sc.rec["sampling"][i]), top, left, 0
                wb = int(_lib.lib().eosv_jpeg_render_workspace(desc, N))
                work = torch.empty(wb, dtype=torch.uint8, device="cuda")
                m = (ctypes.c_float * 3)(*engine.IMAGENET_MEAN)
                sd = (ctypes.c_float * 3)(*engine.IMAGENET_STD)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                s = torch.cuda.current_stream()
                e[0].record(s)
                dbuf.copy_(pinned, non_blocking=True)
                e[1].record(s)
                _lib.check(_lib.lib().eosv_jpeg_render(dbuf.data_ptr(), total, dbuf.data_ptr() + total * 2, desc, N, CROP,
                                                       m, sd, out.data_ptr(), work.data_ptr(), wb, s.cuda_stream),
                           "eosv_jpeg_render")
                e[2].record(s)
                torch.cuda.synchronize()
                return (t1 - t0, e[0].elapsed_time(e[1]) * 1e-3, e[1].elapsed_time(e[2]) * 1e-3, time.perf_counter() - t0)

            hs, h2d, kn, wall = best(native_run)
            say(f"    {threads:7d}   {hs / N * 1e6:21.1f}   {h2d / N * 1e6:12.1f}   {kn / N * 1e6:16.1f}   {N / hs:13.0f}   "
                f"{N / wall:13.0f}")
            if threads == 1:
                host1 = hs / N
            if threads == 16:
                host16, kern = hs / N, kn / N
        if gpu:
            # ---- (c) what the loaders do today: one engine.jpeg_frames call per clip of 16 frames
            def clip_run():
                t0 = time.perf_counter()
                for k in range(0, N, 16):
                    engine.jpeg_frames(blobs[k:k + 16], CROP, (top, left), False)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0,)

            say()
            say("(c) native path as the loaders call it: engine.jpeg_frames per clip of 16 frames, wall clock")
            for threads in (8, 16):
                os.environ["EOSV_JPEG_THREADS"] = str(threads)
                (wall,) = best(clip_run)
                say(f"    {threads:7d} threads   {wall / N * 1e6:8.1f} us/frame   {N / wall:9.0f} frames/s")
            del os.environ["EOSV_JPEG_THREADS"]

            # ---- (d) a test-mode batch through JpegFrames.clips_tensor: files read from disk, one decode
            from eosv import frames as fr

            src = fr.JpegFrames(os.path.dirname(root), crop=CROP, native=True)
            vi = os.path.basename(root)
            clips = [(vi, list(range(k + 1, k + 17)), 16) for k in range(0, N, 16)]

            def batch_run():
                t0 = time.perf_counter()
                src.clips_tensor(clips)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0,)

            say()
            say("(d) JpegFrames.clips_tensor over 32 clips of 16 frames (reads the files, one decode), wall clock")
            for threads in (8, 16):
                os.environ["EOSV_JPEG_THREADS"] = str(threads)
                (wall,) = best(batch_run)
                say(f"    {threads:7d} threads   {wall / N * 1e6:8.1f} us/frame   {N / wall:9.0f} frames/s")
            del os.environ["EOSV_JPEG_THREADS"]
        say()
        say(f"condition 1 (entropy on one thread below PIL's decode): {host1 * 1e6:.1f} us < {pil_decode * 1e6:.1f} us: "
            f"{'holds' if host1 < pil_decode else 'FAILS'} ({pil_decode / host1:.2f}x per core)")
        if gpu:
            say(f"condition 2 (kernels below the host stage at 16 threads): {kern * 1e6:.1f} us < {host16 * 1e6:.1f} us: "
                f"{'holds' if kern < host16 else 'FAILS'}")
        else:
            say("condition 2 (kernels below the host stage at 16 threads): not measured (no device in this run)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
