"""Exact tests of conv_wino_f32_kernel (csrc/conv_wino_f32.hip): outputs that must equal the f64
convolution bit for bit, whatever the order of summation, so that a tile, a channel or a k-pair
permuted inside the kernel's V image (LDS layout [pos][h][tile][kp], read by ds_read_b128) cannot
hide under the 1e-5 (1 + conv(|x|, |w|)) bound of the other Winograd tests.

Integer problems.  x holds integers in [-3, 3] (zeros among them), w holds 4 * integers in
[-2, 2], bias and residual hold small integers.  G's entries are 0, 1 and +-1/2, so U = G g G^T
is an integer with |U| <= 8 * 1.5 * 1.5 = 18; V = B^T d B adds four taps with signs, |V| <= 12;
M = sum_c V U has |M| <= C * 12 * 18 = 216 C <= 110,592 at C = 512, and every partial sum of it is
an integer no larger; the output transform adds nine M, then bias and residual: every intermediate
is an integer below 2^24, so every f32 operation is exact and the result is the f64 conv2d
(+ bias + residual, ReLU) exactly.  The test asserts those magnitudes on its inputs.

Identity weights.  w[o][i][1][1] = 4 delta(o, i): U is +-1 at the four middle positions and 0
elsewhere, y = 4 x (+ bias + residual).  x holds a distinct integer below 2^22 per (frame, pixel,
channel); V's entries add four of them (< 2^24), so the result is exact again, and a wrong output
names the (frame, pixel, channel) it was taken from.

Shapes: the smallest that reach each path (a full item followed by a ragged one, tile groups
straddling frames, two channel blocks, the channel-block-major order of C >= 512, a single tile),
each uncapped and through eosv_conv_wino_f32_grid with few workgroups, so that one workgroup walks
several items and the V image of an item's chunk 0 is written again after the output transform.
Buffers as in tests/test_gpu_wino_persist.py: NaN around x, a sentinel around y.  Every case is
launched twice and the two outputs must be equal: a U slab or a V image read before it was
complete gives a wrong number, not a fault."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of x and y
SENTINEL = -7.25   # not an integer: never an output of these problems

# (N, H, W, C), caps (None: eosv_conv_wino_f32)
SHAPES = [
    ((9, 5, 5, 64), (None, 1)),        # 81 tiles: a full item, then a ragged one of 17; odd map; nk = 8
    ((11, 4, 6, 128), (None, 1, 3)),   # tile groups straddle frames, two channel blocks, nk = 16
    ((2, 7, 7, 512), (None, 1, 2)),    # channel-block-major order, 64 chunks, out-of-image taps on every tile
    ((1, 2, 2, 64), (None,)),          # a single tile
]
CASES = [(s, res, relu, cap) for s, caps in SHAPES for cap in caps for res, relu in ((True, True), (False, False))]
IDS = ["x".join(map(str, s)) + f"-res{int(a)}-relu{int(b)}-cap{c}" for s, a, b, c in CASES]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _u_of(w):
    from eosv._lib import check, lib

    C = w.shape[0]
    u = np.empty(16 * C * C, np.float32)
    check(lib().eosv_wino_weights_f32(w.numpy().ctypes.data, None, C, C, u.ctypes.data), "eosv_wino_weights_f32")
    return u


@functools.lru_cache(maxsize=None)
def _integer_problem(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(104729 + 1000 * C + 100 * N + 10 * H + W)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
    w = 4.0 * torch.randint(-2, 3, (C, C, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (C,), generator=g).float()
    r = torch.randint(-9, 10, (N, C, H, W), generator=g).float()
    u = _u_of(w)
    # the analytic bound of the docstring, on the inputs as drawn
    assert bool((x == 0).any()) and float(x.abs().max()) == 3.0
    assert float(w.abs().max()) <= 8.0
    assert np.array_equal(u, np.rint(u)) and float(np.abs(u).max()) <= 18.0
    assert C * 12 * 18 * 9 + 5 + 9 < 2 ** 24
    conv = torch.nn.functional.conv2d(x.double(), w.double(), padding=1)
    assert float(conv.abs().max()) + 5 + 9 < 2 ** 24
    return dict(x=x, r=r, b=b, u=torch.from_numpy(u).cuda(), conv=conv)


@functools.lru_cache(maxsize=None)
def _identity_problem(shape):
    N, H, W, C = shape
    numel = N * C * H * W
    assert numel + 1 < 2 ** 22
    g = torch.Generator().manual_seed(7 + numel)
    # a distinct integer in [1, numel] per (frame, pixel, channel), in no simple order
    x = (torch.randperm(numel, generator=g) + 1).float().view(N, C, H, W)
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 4.0
    b = torch.randint(0, 4, (C,), generator=g).float()
    r = torch.randint(0, 6, (N, C, H, W), generator=g).float()
    u = _u_of(w)
    assert np.array_equal(u, np.rint(u)) and float(np.abs(u).max()) == 1.0
    return dict(x=x, r=r, b=b, u=torch.from_numpy(u).cuda(), conv=4.0 * x.double())


def _launch(shape, p, res, relu, cap):
    """One launch -> y [N][H][W][C] on the CPU; the sentinel bands around y are checked."""
    from eosv._lib import check, lib, stream_ptr

    N, H, W, C = shape
    x = _nhwc(p["x"])
    numel = x.numel()
    xbuf = torch.full((numel + 2 * GUARD,), float("nan"))
    xbuf[GUARD:GUARD + numel] = x.reshape(-1)
    xbuf = xbuf.cuda()
    ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
    rd = _nhwc(p["r"]).cuda() if res else None
    bd = p["b"].cuda()
    args = (xbuf.data_ptr() + 4 * GUARD, p["u"].data_ptr(), bd.data_ptr(), rd.data_ptr() if res else None,
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


def _expected(p, res, relu):
    ref = p["conv"] + p["b"].double()[None, :, None, None]
    if res:
        ref = ref + p["r"].double()
    if relu:
        ref = torch.relu(ref)
    ref = _nhwc(ref)
    assert torch.equal(ref.float().double(), ref), "the reference is not an f32 number"
    return ref.float()


def _twice(shape, p, res, relu, cap):
    y = _launch(shape, p, res, relu, cap)
    again = _launch(shape, p, res, relu, cap)
    assert bool((y != SENTINEL).all()), "an output was not written"
    assert torch.equal(y, again), "two launches of one problem differ"
    return y


@pytest.mark.parametrize("shape,res,relu,cap", CASES, ids=IDS)
def test_integer_problem_is_exact(shape, res, relu, cap):
    p = _integer_problem(shape)
    y = _twice(shape, p, res, relu, cap)
    ref = _expected(p, res, relu)
    bad = (y != ref).nonzero()
    n = len(bad)
    print(f"wino exact {shape} res={res} relu={relu} cap={cap}: {n} of {y.numel()} outputs differ")
    assert n == 0, f"first at (n, h, w, c) = {bad[0].tolist()}: {float(y[tuple(bad[0])])} != {float(ref[tuple(bad[0])])}"


@pytest.mark.parametrize("shape,res,relu,cap", CASES, ids=IDS)
def test_identity_weights_place_every_tile_and_channel(shape, res, relu, cap):
    N, H, W, C = shape
    p = _identity_problem(shape)
    y = _twice(shape, p, res, relu, cap)
    ref = _expected(p, res, relu)
    bad = (y != ref).nonzero()
    n = len(bad)
    print(f"wino identity {shape} res={res} relu={relu} cap={cap}: {n} of {y.numel()} outputs differ")
    if n:
        at = tuple(bad[0].tolist())
        # which x the wrong output is 4 times of (bias and residual taken off again)
        got = float(y[at]) - float(p["b"][at[3]]) - (float(_nhwc(p["r"])[at]) if res else 0.0)
        src = (_nhwc(p["x"]) == got / 4.0).nonzero()
        src = src[0].tolist() if len(src) else "no element of x"
        pytest.fail(f"{n} outputs differ; first at (n, h, w, c) = {list(at)}: {float(y[at])} != {float(ref[at])}, "
                    f"the value of x at {src}")
