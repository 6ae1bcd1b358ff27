"""The persistent tile loop of conv_wino_f32_kernel (csrc/conv_wino_f32.hip): a workgroup walks
several (tile group, channel block) items, and the loads of an item's first chunks are issued
during the last chunks of the item before it.

eosv_conv_wino_f32_grid caps the workgroup count, so the walk is reached at tiny shapes: one
workgroup doing every item, items split unevenly, more workgroups than items.  Problems are built
as in tests/test_gpu_wino_ds.py: x inside NaN guard bands, y inside sentinel bands, f64 conv2d as
the reference with the bound 1e-5 (1 + conv(|x|, |w|)).  Every capped run must also be bitwise
the uncapped eosv_conv_wino_f32 of the same problem: one fixed summation order per output,
whatever the grid."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of x and y
SENTINEL = -7.25   # never a conv output of these inputs by chance, exact in f32

# (N, H, W, C), residual, ReLU, caps
CAPPED = [
    ((40, 6, 6, 64), True, True, (1, 2, 4, 7)),    # 6 items: a workgroup walks 6, 3 or 1-2; cap 7 leaves one idle
    ((9, 7, 7, 128), True, False, (1, 3, 4)),      # 3 tile groups x 2 channel blocks
    ((9, 7, 7, 128), False, True, (1, 3, 4)),
    ((2, 6, 6, 192), True, True, (1, 2)),          # one ragged tile group x 3 channel blocks, 24 chunks
    ((3, 4, 4, 512), True, True, (1, 3, 8)),       # channel-block-major order, 8 items, 64 chunks
    ((1, 3, 3, 64), True, True, (3,)),             # one ragged item, idle workgroups
    ((3, 5, 7, 64), False, False, (1,)),           # odd maps, fewer than 64 tiles
]
CASES = [(s, res, relu, cap) for s, res, relu, caps in CAPPED for cap in caps]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _inputs(N, H, W, C):
    """x, residual (NCHW) of N frames: frame n depends on (n, H, W, C) only, so a longer batch of
    the same map extends a shorter one."""
    xs, rs = [], []
    for n in range(N):
        g = torch.Generator().manual_seed(7919 * n + 1000 * C + 10 * H + W)
        xs.append(torch.relu(torch.randn(C, H, W, generator=g)))
        rs.append(torch.randn(C, H, W, generator=g))
    return torch.stack(xs), torch.stack(rs)


@functools.lru_cache(maxsize=None)
def _weights(C):
    from eosv._lib import check, lib

    g = torch.Generator().manual_seed(31 * C + 5)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = torch.randn(C, generator=g)
    u = np.empty(16 * C * C, np.float32)
    check(lib().eosv_wino_weights_f32(w.numpy().ctypes.data, None, C, C, u.ctypes.data), "eosv_wino_weights_f32")
    return w, b, torch.from_numpy(u).cuda()


@functools.lru_cache(maxsize=None)
def _problem(shape):
    N, H, W, C = shape
    x, r = _inputs(N, H, W, C)
    w, b, u = _weights(C)
    conv = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    mag = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), padding=1)
    return dict(x=x, r=r, b=b, u=u, conv=conv, mag=mag)


def _launch(shape, x_nchw, r_nchw, b, u, res, relu, cap):
    """One launch (cap None: eosv_conv_wino_f32) -> y [N][H][W][C] on the CPU, sentinels checked."""
    from eosv._lib import check, lib, stream_ptr

    N, H, W, C = shape
    x = _nhwc(x_nchw).float()
    numel = x.numel()
    xbuf = torch.full((numel + 2 * GUARD,), float("nan"))
    xbuf[GUARD:GUARD + numel] = x.reshape(-1)
    xbuf = xbuf.cuda()
    ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
    rd = _nhwc(r_nchw).float().cuda() if res else None
    bd = b.cuda()
    args = (xbuf.data_ptr() + 4 * GUARD, u.data_ptr(), bd.data_ptr(), rd.data_ptr() if res else None,
            1 if relu else 0, ybuf.data_ptr() + 4 * GUARD, N, H, W, C, stream_ptr())
    if cap is None:
        check(lib().eosv_conv_wino_f32(*args), "eosv_conv_wino_f32")
    else:
        check(lib().eosv_conv_wino_f32_grid(*args, cap), "eosv_conv_wino_f32_grid")
    torch.cuda.synchronize()
    ybuf = ybuf.cpu()
    assert bool((ybuf[:GUARD] == SENTINEL).all()) and bool((ybuf[GUARD + numel:] == SENTINEL).all()), \
        "store outside y"
    return ybuf[GUARD:GUARD + numel].view(N, H, W, C)


def _run(shape, res, relu, cap):
    p = _problem(shape)
    return _launch(shape, p["x"], p["r"], p["b"], p["u"], res, relu, cap)


@functools.lru_cache(maxsize=None)
def _uncapped(shape, res, relu):
    return _run(shape, res, relu, None)


@pytest.mark.parametrize("shape,res,relu,cap", CASES,
                         ids=["x".join(map(str, s)) + f"-res{int(a)}-relu{int(b)}-cap{c}" for s, a, b, c in CASES])
def test_capped_grid_matches_reference_and_uncapped_launch(shape, res, relu, cap):
    p = _problem(shape)
    y = _run(shape, res, relu, cap)
    assert bool(torch.isfinite(y).all()), "non-finite output: a read outside x"
    ref = p["conv"] + p["b"].double()[None, :, None, None]
    if res:
        ref = ref + p["r"].double()
    if relu:
        ref = torch.relu(ref)
    err = (y.double() - _nhwc(ref)).abs()
    bound = 1e-5 * (1.0 + _nhwc(p["mag"]))
    worst = float((err / bound).max())
    print(f"wino {shape} res={res} relu={relu} cap={cap}: max err / bound = {worst:.3e}, "
          f"max |err| = {float(err.max()):.3e}")
    assert worst <= 1.0
    assert torch.equal(y, _uncapped(shape, res, relu)), "capped and uncapped launches differ"


def test_default_grid_walks_several_items_per_workgroup():
    """3,700 frames of 6 x 6 x 64: 521 items on one workgroup per CU, so workgroups walk two or three
    items of their own accord.  The first 40 frames are those of the (40, 6, 6, 64) problem: bitwise
    equal outputs (independence of batch and grid)."""
    small, big = (40, 6, 6, 64), (3700, 6, 6, 64)
    p = _problem(small)
    x, r = _inputs(*big)
    assert torch.equal(x[:40], p["x"]) and torch.equal(r[:40], p["r"])
    y = _launch(big, x, r, p["b"], p["u"], True, True, None)
    assert bool(torch.isfinite(y).all()), "non-finite output: a read outside x"
    assert torch.equal(y[:40], _uncapped(small, True, True))


def test_capped_launch_repeats_bitwise():
    a = _run((9, 7, 7, 128), True, False, 3)
    b = _run((9, 7, 7, 128), True, False, 3)
    assert torch.equal(a, b)
