"""The Winograd F(2x2, 3x3) f32 conv (csrc/conv_wino_f32.hip) through its stand-alone entry
eosv_conv_wino_f32, against torch.nn.functional.conv2d in float64 on the CPU.

Bound: conv_check's rule |err| <= 1e-5 (1 + sum |terms|), the sum from a conv of the absolute
values (a CPU emulation of the method stays below 2e-7 of it on these shapes).  x sits inside a
NaN-filled buffer and y inside a sentinel-filled one: a stray read makes the result non-finite, a
stray store changes the sentinel."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of x and y
SENTINEL = -7.25   # never a conv output of these inputs by chance, exact in f32

# (N, H, W, C): one partial workgroup; odd H and W (ragged tiles); 9 tiles per frame (a 64-tile
# group straddles frames, with a tail); several K chunks and two cout blocks; the long K walk
SHAPES = [(1, 8, 8, 64), (3, 7, 5, 64), (5, 6, 6, 64), (2, 14, 14, 128), (2, 7, 7, 512)]
# residual on / off x ReLU on / off, every combination on at least one shape
CASES = [(SHAPES[0], False, False), (SHAPES[1], True, True), (SHAPES[2], True, False),
         (SHAPES[3], False, True), (SHAPES[4], True, True)]


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """Inputs (f32, NCHW on the CPU), the device U buffer, and the f64 reference pieces."""
    from eosv._lib import check, lib

    N, H, W, C = shape
    g = torch.Generator().manual_seed(1000 * C + 10 * H + N)
    x = torch.relu(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g)
    r = torch.randn(N, C, H, W, generator=g)
    u = np.empty(16 * C * C, np.float32)
    wn = w.numpy()
    check(lib().eosv_wino_weights_f32(wn.ctypes.data, None, C, C, u.ctypes.data), "eosv_wino_weights_f32")
    conv = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    mag = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), padding=1)
    return dict(x=x, w=w, b=b, r=r, u=torch.from_numpy(u).cuda(), conv=conv, mag=mag)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _run(shape, res, relu, frames=None):
    """y (NHWC f32, on the CPU) of the kernel for frames `frames` (default all) of the problem."""
    from eosv._lib import check, lib, stream_ptr

    p = _problem(shape)
    _, H, W, C = shape
    sel = slice(None) if frames is None else frames
    x = _nhwc(p["x"][sel]).float()
    n = x.shape[0]
    numel = x.numel()
    xbuf = torch.full((numel + 2 * GUARD,), float("nan"))
    xbuf[GUARD:GUARD + numel] = x.reshape(-1)
    xbuf = xbuf.cuda()
    ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
    rd = _nhwc(p["r"][sel]).float().cuda() if res else None
    bd = p["b"].cuda()
    check(lib().eosv_conv_wino_f32(xbuf.data_ptr() + 4 * GUARD, p["u"].data_ptr(), bd.data_ptr(),
                                   rd.data_ptr() if res else None, 1 if relu else 0,
                                   ybuf.data_ptr() + 4 * GUARD, n, H, W, C, stream_ptr()), "eosv_conv_wino_f32")
    torch.cuda.synchronize()
    ybuf = ybuf.cpu()
    assert bool((ybuf[:GUARD] == SENTINEL).all()) and bool((ybuf[GUARD + numel:] == SENTINEL).all()), \
        "store outside y"
    return ybuf[GUARD:GUARD + numel].view(n, H, W, C)


@pytest.mark.parametrize("shape,res,relu", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(int(v)))
def test_wino_conv_vs_f64_conv2d(shape, res, relu):
    p = _problem(shape)
    y = _run(shape, res, relu)
    assert bool(torch.isfinite(y).all()), "non-finite output: a read outside x"
    ref = p["conv"] + p["b"].double()[None, :, None, None]
    if res:
        ref = ref + p["r"].double()
    if relu:
        ref = torch.relu(ref)
    err = (y.double() - _nhwc(ref)).abs()
    bound = 1e-5 * (1.0 + _nhwc(p["mag"]))
    worst = float((err / bound).max())
    print(f"wino {shape} res={res} relu={relu}: max err / bound = {worst:.3e}, max |err| = {float(err.max()):.3e}")
    assert worst <= 1.0


def test_wino_conv_batch_invariant_and_repeatable():
    shape = SHAPES[2]  # N = 5, 6 x 6: frame 3 starts mid-workgroup in the batch and at tile 0 alone
    y5 = _run(shape, True, True)
    again = _run(shape, True, True)
    assert y5.numpy().tobytes() == again.numpy().tobytes()
    y1 = _run(shape, True, True, frames=slice(3, 4))
    assert y1.numpy().tobytes() == y5[3:4].contiguous().numpy().tobytes()
