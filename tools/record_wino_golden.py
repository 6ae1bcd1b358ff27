#!/usr/bin/env python3
"""Records tests/golden/wino_otf_parent.npz: outputs of conv_wino_f32_kernel on non-integer data,
for tests/test_gpu_wino_otf.py to compare byte for byte.

Run once on an MI355X with EOSV_LIBRARY set to the library of the commit the kernel must agree
with (the parent of the change that moved the output transform's column stage into registers):

  EOSV_LIBRARY=/path/to/parent/libeosv.so python tools/record_wino_golden.py

Per case the file holds `y_<case>` (the output [N][H][W][C], launched uncapped) and `sum_<case>`
(SHA-256 of the seeded inputs x, w, bias, residual), so that the test can tell a changed generator
from a changed kernel.  The test imports the cases, the generator and the launchers from here.

Inputs: x, bias and the residual are standard normal, w is normal scaled by 1 / sqrt(9 C) (outputs of
order one), from numpy's frozen RandomState stream.  U = G g G^T is the host's (eosv_wino_weights_f32).
"""
import functools
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "embodied-one-shot-video-recognition_amd")
GOLDEN = os.path.join(REPO, "tests", "golden", "wino_otf_parent.npz")

SHAPES = [(9, 5, 5, 64), (11, 4, 6, 128), (2, 7, 7, 512)]  # (N, H, W, C): as tests/test_gpu_wino_exact.py
CASES = [(s, rr) for s in SHAPES for rr in (True, False)]   # rr: residual + ReLU, or neither

GUARD = 4096          # floats on each side of x and y
SENTINEL = -7.25


def case_name(shape, rr):
    return "x".join(map(str, shape)) + ("_res_relu" if rr else "_plain")


@functools.lru_cache(maxsize=None)
def problem(shape):
    """x [N][H][W][C], w [C][C][3][3], b [C], r [N][H][W][C]: f32, C-contiguous."""
    N, H, W, C = shape
    rs = np.random.RandomState(20261 + 1000 * C + 100 * N + 10 * H + W)
    x = rs.standard_normal((N, H, W, C)).astype(np.float32)
    w = (rs.standard_normal((C, C, 3, 3)) / np.sqrt(9.0 * C)).astype(np.float32)
    b = rs.standard_normal((C,)).astype(np.float32)
    r = rs.standard_normal((N, H, W, C)).astype(np.float32)
    return dict(x=x, w=w, b=b, r=r)


def checksum(p):
    h = hashlib.sha256()
    for k in ("x", "w", "b", "r"):
        h.update(np.ascontiguousarray(p[k]).tobytes())
    return h.hexdigest()


def guarded(x):
    """x (numpy, f32) on the device with GUARD floats of NaN on each side."""
    import torch

    buf = torch.full((x.size + 2 * GUARD,), float("nan"))
    buf[GUARD:GUARD + x.size] = torch.from_numpy(np.ascontiguousarray(x)).reshape(-1)
    return buf.cuda()


@functools.lru_cache(maxsize=None)
def _device(shape):
    import torch
    from eosv._lib import check, lib

    p = problem(shape)
    C = shape[3]
    u = np.empty(16 * C * C, np.float32)
    check(lib().eosv_wino_weights_f32(p["w"].ctypes.data, None, C, C, u.ctypes.data), "eosv_wino_weights_f32")
    return dict(x=guarded(p["x"]), u=torch.from_numpy(u).cuda(), b=torch.from_numpy(p["b"]).cuda(),
                r=torch.from_numpy(p["r"]).cuda())


def launch_arrays(shape, x, u, b, r, relu, cap=None):
    """One launch on device tensors (x with GUARD floats of NaN on each side; b, r may be None) ->
    y [N][H][W][C] as a numpy array.  y lies between two sentinel bands that must come back
    untouched.  cap: eosv_conv_wino_f32_grid's max_workgroups (None: eosv_conv_wino_f32)."""
    import torch
    from eosv._lib import check, lib, stream_ptr

    N, H, W, C = shape
    numel = N * H * W * C
    ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
    args = (x.data_ptr() + 4 * GUARD, u.data_ptr(), None if b is None else b.data_ptr(),
            None if r is None else r.data_ptr(), 1 if relu else 0, ybuf.data_ptr() + 4 * GUARD, N, H, W, C,
            stream_ptr())
    if cap is None:
        check(lib().eosv_conv_wino_f32(*args), "eosv_conv_wino_f32")
    else:
        check(lib().eosv_conv_wino_f32_grid(*args, cap), "eosv_conv_wino_f32_grid")
    torch.cuda.synchronize()
    ybuf = ybuf.cpu().numpy()
    assert (ybuf[:GUARD] == SENTINEL).all() and (ybuf[GUARD + numel:] == SENTINEL).all(), "store outside y"
    return ybuf[GUARD:GUARD + numel].reshape(N, H, W, C)


def launch(shape, rr, cap=None):
    """One launch of a golden case (rr: residual + ReLU, or neither; the bias is always given)."""
    d = _device(shape)
    return launch_arrays(shape, d["x"], d["u"], d["b"], d["r"] if rr else None, rr, cap)


def main():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from eosv import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    print(f"library: {_lib.LIB_PATH}")
    data = {}
    for shape, rr in CASES:
        name = case_name(shape, rr)
        y = launch(shape, rr)
        again = launch(shape, rr)
        assert y.tobytes() == again.tobytes(), f"{name}: two launches differ"
        # sanity against the f64 convolution, so that a broken library is not recorded as golden
        import torch
        p = problem(shape)
        ref = torch.nn.functional.conv2d(torch.from_numpy(p["x"]).double().permute(0, 3, 1, 2),
                                         torch.from_numpy(p["w"]).double(), torch.from_numpy(p["b"]).double(), padding=1)
        ref = ref.permute(0, 2, 3, 1)
        if rr:
            ref = torch.relu(ref + torch.from_numpy(p["r"]).double())
        err = float((torch.from_numpy(y).double() - ref).abs().max())
        assert err < 1e-4, f"{name}: {err} from the f64 convolution"
        data["y_" + name] = y
        data["sum_" + name] = np.array(checksum(p))
        print(f"{name}: {y.size} outputs, max |y - f64| {err:.2e}, inputs {checksum(p)[:16]}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
