"""The f32 basic blocks with a downsample on the Winograd kernel (EOSV_F32_WINO_DS, csrc/eosv_api.hip):
the 1x1 / 2 shortcut runs as a launch of its own and the block's conv2 takes its output as the
residual through conv_wino_f32_kernel.

Backbone parity uses the check and the bound of tests/test_gpu_parity.py::test_backbone_features_r18
(max |gpu - ref| < 1e-5 max |ref| against the f32 CPU oracle) at two small sizes: 112 x 112 with 3
frames (stage maps 14, 7 and 4: 147 tiles in stage 2, so tile groups straddle frames and the last
one is ragged; odd and even maps) and 64 x 64 with 5 frames (maps 8, 4 and 2).

The stand-alone kernel cases follow tests/test_gpu_wino.py (|err| <= 1e-5 (1 + sum |terms|) against
f64 conv2d, x inside NaN guard bands, y inside sentinel ones) at the shapes where a patch prefetch
that runs ahead of the K loop can go wrong: workgroups that start in a late frame and span many
frames, fewer tiles than a workgroup holds, and 8 / 24 K chunks (both parities of a loop unrolled
by two, with its prologue and tail)."""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, engine, synth
from oracle import resnet_ref

pytestmark = pytest.mark.gpu

SIZES = [(112, 3), (64, 5)]  # (H = W, frames)


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@functools.lru_cache(maxsize=None)
def _state_dict():
    return synth.synth_state_dict(arch.SPECS["resnet18"], 64, 0)


@functools.lru_cache(maxsize=None)
def _oracle():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    return resnet_ref.build_model("resnet18", _state_dict())


@functools.lru_cache(maxsize=None)
def _frames(res, B):
    return torch.randn(B, 3, res, res, generator=torch.Generator().manual_seed(100 * res + B))


def _backbone(res, max_frames):
    bb = engine.Backbone("resnet18", "f32", res, res, max_frames=max_frames)
    bb.load_state_dict(_state_dict())
    return bb


@pytest.mark.parametrize("res,B", SIZES)
def test_backbone_features_r18_small(res, B):
    x = _frames(res, B)
    with torch.no_grad():
        ref, ref_logits = _oracle()(x)
    bb = _backbone(res, B)
    try:
        out = bb.forward(x.cuda()).cpu()
        logits = bb.fc(out.cuda()).cpu()
    finally:
        bb.close()
    e_feat, e_logit = _rel_err(out.numpy(), ref.numpy()), _rel_err(logits.numpy(), ref_logits.numpy())
    print(f"r18 f32 {res}x{res} B={B}: feature rel err {e_feat:.3e}, logits rel err {e_logit:.3e}")
    assert e_feat < 1e-5
    assert e_logit < 1e-5


def test_downsample_blocks_take_the_unfused_winograd_route():
    """The profile shows the path: every downsample layer has launches of its own, and its block's
    conv2 has as many as a plain Winograd layer (the conv2 of the stage's second block)."""
    res, B = SIZES[0]
    bb = _backbone(res, B)
    try:
        x = _frames(res, B).cuda()
        bb.forward(x)
        bb.profile(True)
        bb.forward(x)
        _, fl, nl = bb.profile_read()
        bb.profile(False)
    finally:
        bb.close()
    blocks = arch.block_layer_ids(arch.SPECS["resnet18"])
    ds_blocks = [(i, b) for i, b in enumerate(blocks) if b[3] is not None]
    assert len(ds_blocks) == 3
    for i, (c1, c2, _, ds) in ds_blocks:
        plain = blocks[i + 1][1]
        assert nl[ds] > 0, f"downsample layer {ds} was not launched: {nl}"
        assert nl[c2] == nl[plain] == nl[ds], (c2, plain, ds, nl)
        # the downsample's FLOPs are its own, no longer part of conv2's: conv2 and the plain layer agree
        assert fl[c2] == fl[plain]


def test_backbone_batch_invariance_and_repeat_determinism():
    """One frame alone against the same frame inside a batch of 5, and the batch twice: bitwise."""
    res, B = SIZES[1]
    x = _frames(res, B).cuda()
    bb = _backbone(res, B)
    try:
        a = bb.forward(x)
        again = bb.forward(x)
        one = bb.forward(x[3:4].contiguous())
    finally:
        bb.close()
    assert torch.equal(a, again)
    assert torch.equal(a[3:4], one)
    chunked = _backbone(res, 2)  # 3 chunks, ragged tail
    try:
        b = chunked.forward(x)
    finally:
        chunked.close()
    assert torch.equal(a, b)


# ---- the Winograd kernel alone (eosv_conv_wino_f32)

GUARD = 4096       # floats on each side of x and y
SENTINEL = -7.25   # never a conv output of these inputs by chance, exact in f32

# (N, H, W, C), residual, ReLU
KERNEL_CASES = [
    ((40, 6, 6, 64), True, True),     # 9 tiles per frame: every workgroup but the first starts in a later frame, spans 7-8
    ((9, 7, 7, 128), False, True),    # 16 tiles per frame, two cout blocks
    ((9, 7, 7, 128), True, False),
    ((1, 3, 3, 64), True, True),      # 4 tiles: one ragged workgroup, most lanes past the end
    ((3, 5, 7, 64), False, False),    # 36 tiles < 64, odd maps
    ((2, 8, 8, 64), True, True),      # 8 K chunks
    ((2, 6, 6, 192), True, True),     # 24 K chunks, three cout blocks
]


@functools.lru_cache(maxsize=None)
def _problem(shape):
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
    return dict(x=x, b=b, r=r, u=torch.from_numpy(u).cuda(), conv=conv, mag=mag)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _run(shape, res, relu):
    from eosv._lib import check, lib, stream_ptr

    p = _problem(shape)
    N, H, W, C = shape
    x = _nhwc(p["x"]).float()
    numel = x.numel()
    xbuf = torch.full((numel + 2 * GUARD,), float("nan"))
    xbuf[GUARD:GUARD + numel] = x.reshape(-1)
    xbuf = xbuf.cuda()
    ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
    rd = _nhwc(p["r"]).float().cuda() if res else None
    bd = p["b"].cuda()
    check(lib().eosv_conv_wino_f32(xbuf.data_ptr() + 4 * GUARD, p["u"].data_ptr(), bd.data_ptr(),
                                   rd.data_ptr() if res else None, 1 if relu else 0,
                                   ybuf.data_ptr() + 4 * GUARD, N, H, W, C, stream_ptr()), "eosv_conv_wino_f32")
    torch.cuda.synchronize()
    ybuf = ybuf.cpu()
    assert bool((ybuf[:GUARD] == SENTINEL).all()) and bool((ybuf[GUARD + numel:] == SENTINEL).all()), \
        "store outside y"
    return ybuf[GUARD:GUARD + numel].view(N, H, W, C)


@pytest.mark.parametrize("shape,res,relu", KERNEL_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(int(v)))
def test_wino_kernel_prefetch_shapes(shape, res, relu):
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
