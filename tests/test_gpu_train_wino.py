"""GPU: the opt-in Winograd F(2x2, 3x3) path of the training step.

eosv_wino_weights_f32_device (csrc/conv_wino_f32.hip, wino_weights_kernel) transforms the trainer's
[cout][3][3][cin] weights on the device, of the conv itself (flip 0) and of its input-gradient conv
(flip 1); NativeTrainer(winograd=mask) then runs the forward and the input gradient of every
stride-1 3x3 conv with Cin = Cout on eosv_conv_wino_f32.

1. the device U is bitwise the host's (eosv_wino_weights_f32), inside guarded buffers;
2. forward and input gradient (+ fused accumulation) against f64 under the conv rule of
   test_gpu_wino.py, |err| <= 1e-5 (1 + sum |terms|), the sum over the conv's own terms;
3. two trainer steps with all four stages enabled against the f64 replay, with the bounds of
   tests/test_gpu_train.py (_oracle and _check_two_steps are restated here unchanged), and
   wino_launches equal to the count the architecture gives;
4. determinism; 5. the default path is untouched; 6. rejections.

The trainer tests pass winograd=15 rather than True: True resolves to TRAIN_WINO_DEFAULT, which holds
only the stages that won the A/B (today all four) and may lose bits later; the tests cover all four.
"""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _expected_wino_launches, _oracle, _same_bytes, _small_case

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of the guarded buffers
SENTINEL = -7.25   # exact in f32, never a transform or conv output of these inputs by chance

# (cout, cin, flip): the single-chunk edges, a cin (flip 1: cout) that is no multiple of 64 with two
# 64-blocks on the other axis, one square block, and several blocks on both axes
TRANSFORMS = [(64, 8, 0), (128, 72, 0), (64, 64, 0), (256, 256, 0),
              (8, 64, 1), (72, 128, 1), (64, 64, 1), (256, 256, 1)]


def _device_u(w_ohwi, cout, cin, flip):
    """U (on the CPU) of w_ohwi [cout][3][3][cin] (f32, CPU) from the device transform; w sits in a
    NaN-filled buffer and U in a sentinel-filled one, whose guards must come back untouched."""
    from eosv._lib import check, lib, stream_ptr

    n = 16 * cout * cin
    wbuf = torch.full((w_ohwi.numel() + 2 * GUARD,), float("nan"))
    wbuf[GUARD:GUARD + w_ohwi.numel()] = w_ohwi.reshape(-1)
    wbuf = wbuf.cuda()
    ubuf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    check(lib().eosv_wino_weights_f32_device(wbuf.data_ptr() + 4 * GUARD, cout, cin, flip,
                                             ubuf.data_ptr() + 4 * GUARD, stream_ptr()),
          "eosv_wino_weights_f32_device")
    torch.cuda.synchronize()
    ubuf = ubuf.cpu()
    assert bool((ubuf[:GUARD] == SENTINEL).all()) and bool((ubuf[GUARD + n:] == SENTINEL).all()), "store outside U"
    return ubuf[GUARD:GUARD + n]


def _host_u(w_oihw):
    from eosv._lib import check, lib

    co, ci = w_oihw.shape[:2]
    w = np.ascontiguousarray(w_oihw.numpy())
    u = np.empty(16 * co * ci, np.float32)
    check(lib().eosv_wino_weights_f32(w.ctypes.data, None, co, ci, u.ctypes.data), "eosv_wino_weights_f32")
    return torch.from_numpy(u)


@pytest.mark.parametrize("cout,cin,flip", TRANSFORMS)
def test_device_weight_transform_bitwise_equals_host(cout, cin, flip):
    g = torch.Generator().manual_seed(100 * cout + cin + flip)
    w_ohwi = torch.randn(cout, 3, 3, cin, generator=g)
    w_oihw = w_ohwi.permute(0, 3, 1, 2).contiguous()
    # flip 1: the input-gradient conv's weights, [cin][cout][3][3] rotated by 180 degrees
    host = _host_u(w_oihw.flip(2, 3).transpose(0, 1).contiguous() if flip else w_oihw)
    dev = _device_u(w_ohwi, cout, cin, flip)
    assert bool(torch.isfinite(dev).all()), "non-finite U: a read outside w"
    assert bool((dev != SENTINEL).all()), "a U slot was not written"
    assert dev.numpy().tobytes() == host.numpy().tobytes()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape", [(3, 7, 5, 64), (2, 14, 14, 128)], ids=lambda s: "x".join(map(str, s)))
def test_wino_forward_and_input_gradient_vs_f64(shape):
    """Ragged tiles and a workgroup straddling frames (7 x 5, 3 frames); two cout blocks (128).
    Weights in the trainer's layout, U from the device transform for both directions."""
    from eosv._lib import check, lib, stream_ptr

    N, H, W, C = shape
    g = torch.Generator().manual_seed(7 * C + H)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    dz = torch.randn(N, C, H, W, generator=g)
    acc = torch.randn(N, C, H, W, generator=g)
    xd = x.double().requires_grad_(True)
    ref_y = torch.nn.functional.conv2d(xd, w.double(), padding=1)
    ref_y.backward(dz.double())
    ref_dx = xd.grad + acc.double()
    mag_y = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), padding=1)
    mag_dx = torch.nn.functional.conv_transpose2d(dz.double().abs(), w.double().abs(), padding=1)

    L, s = lib(), stream_ptr()
    w_ohwi = w.permute(0, 2, 3, 1).contiguous().cuda()
    u = torch.empty(16 * C * C, device="cuda")

    def run(inp, flip, res):
        numel = inp.numel()
        ybuf = torch.full((numel + 2 * GUARD,), SENTINEL, device="cuda")
        ind = _nhwc(inp).cuda()
        rd = _nhwc(res).cuda() if res is not None else None
        check(L.eosv_wino_weights_f32_device(w_ohwi.data_ptr(), C, C, flip, u.data_ptr(), s),
              "eosv_wino_weights_f32_device")
        check(L.eosv_conv_wino_f32(ind.data_ptr(), u.data_ptr(), None, rd.data_ptr() if rd is not None else None, 0,
                                   ybuf.data_ptr() + 4 * GUARD, N, H, W, C, s), "eosv_conv_wino_f32")
        torch.cuda.synchronize()
        ybuf = ybuf.cpu()
        assert bool((ybuf[:GUARD] == SENTINEL).all()) and bool((ybuf[GUARD + numel:] == SENTINEL).all())
        return ybuf[GUARD:GUARD + numel].view(N, H, W, C)

    for what, got, ref, mag in (("forward", run(x, 0, None), ref_y.detach(), mag_y),
                                ("input gradient + acc", run(dz, 1, acc), ref_dx, mag_dx)):
        err = (got.double() - _nhwc(ref)).abs()
        bound = 1e-5 * (1.0 + _nhwc(mag))
        worst = float((err / bound).max())
        print(f"train wino {shape} {what}: max err / bound = {worst:.3e}, max |err| = {float(err.max()):.3e}")
        assert worst <= 1.0, what


# ---------------------------------------------------------------- the trainer
def _check_two_steps(name, frames, labels, T, H, winograd):
    lr1, lr2 = 1e-3, 1e-2  # 10x the reference's (network_train.py:140)
    sd = synth.synth_state_dict(arch.SPECS[name], 64, 0)
    ref_losses, ref_g, ref_sd = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float64)
    f32_losses, f32_g, f32_sd = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float32)

    tr = NativeTrainer(name, 64, device=0, winograd=winograd)
    tr.load_state_dict(sd)
    l0, logits = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.wino_launches == _expected_wino_launches(name, winograd) > 0
    g0 = tr.grads()
    l1, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.wino_launches == _expected_wino_launches(name, winograd)  # per step, not cumulative
    print(f"[{name} {tuple(frames.shape)} wino {winograd}] loss {l0:.6f} / {ref_losses[0]:.6f}, "
          f"{l1:.6f} / {ref_losses[1]:.6f}; {tr.wino_launches} Winograd launches per step")
    assert abs(l0 - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    # the second loss inherits the first step's gradient conditioning: same yardstick
    assert abs(l1 - ref_losses[1]) <= max(4 * abs(f32_losses[1] - ref_losses[1]), 1e-4 * abs(ref_losses[1]))
    worst = (0.0, None, 0.0)
    ratio = (0.0, None)
    for k, gr in ref_g.items():
        norm = max(float(gr.norm()), 1e-12)
        err = float((g0[k].double() - gr).norm()) / norm
        yard = float((f32_g[k] - gr).norm()) / norm
        if err > worst[0]:
            worst = (err, k, yard)
        if yard > 0 and err / yard > ratio[0]:
            ratio = (err / yard, k)
        assert err <= max(4 * yard, 2e-2), (k, err, yard)
    print(f"[{name} {tuple(frames.shape)} wino {winograd}] worst relative gradient error {worst[0]:.2e} at "
          f"{worst[1]} (torch-f32 yardstick there {worst[2]:.2e}); largest error / yardstick {ratio[0]:.2f} "
          f"at {ratio[1]}")
    got = tr.state_dict()
    for k, v in ref_sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v), k
            continue
        v = v.double()
        err = float((got[k].double() - v).norm())
        yard = float((f32_sd[k].double() - v).norm())
        assert err <= max(4 * yard, 1e-6 * v.numel() ** 0.5 + 1e-5 * float(v.norm())), (k, err, yard)


def test_expected_launch_counts():
    # R18: 4 + 3 + 3 + 3 eligible convs; R50: conv2 of 3 + 3 + 5 + 2 blocks; forward + input gradient
    assert _expected_wino_launches("resnet18") == 26 and _expected_wino_launches("resnet50") == 26
    assert _expected_wino_launches("resnet18", 1) == 8 and _expected_wino_launches("resnet50", 4) == 10


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_train_step_winograd_matches_torch_reference(name):
    frames, labels, T = _small_case()
    _check_two_steps(name, frames, labels, T, frames.shape[-1], 15)


@functools.lru_cache(maxsize=None)
def _r18_step(winograd):
    """(loss, grads, wino_launches) of one step of a fresh ResNet-18 trainer on the small case;
    winograd "default" builds the trainer without the keyword."""
    frames, labels, T = _small_case()
    kw = {} if winograd == "default" else {"winograd": winograd}
    tr = NativeTrainer("resnet18", 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS["resnet18"], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr.wino_launches


def test_winograd_step_is_deterministic():
    a = _r18_step(15)
    _r18_step.cache_clear()
    b = _r18_step(15)
    assert a[2] == b[2] == 26
    _same_bytes(a, b)


def test_default_step_untouched_by_the_keyword():
    a, b = _r18_step("default"), _r18_step(False)
    assert a[2] == 0 and b[2] == 0
    _same_bytes(a, b)
    # and the Winograd step really is another computation (it did not fall back to the direct kernels)
    c = _r18_step(15)
    assert any(c[1][k].numpy().tobytes() != a[1][k].numpy().tobytes() for k in a[1])


def test_device_weight_transform_rejects_bad_arguments():
    from eosv._lib import EosvError, check, lib, stream_ptr

    L = lib()
    w = torch.zeros(9 * 128 * 128, device="cuda")
    u = torch.full((16 * 128 * 128,), SENTINEL, device="cuda")
    bad = [(w.data_ptr(), 32, 64, 0, u.data_ptr()),    # cout = 32
           (w.data_ptr(), 64, 12, 0, u.data_ptr()),    # cin = 12
           (w.data_ptr(), 64, 72, 1, u.data_ptr()),    # flip: cin is U's 64-block axis
           (None, 64, 64, 0, u.data_ptr()),
           (w.data_ptr(), 64, 64, 0, None)]
    for args in bad:
        rc = L.eosv_wino_weights_f32_device(*args, stream_ptr())
        assert rc != 0, args
        with pytest.raises(EosvError, match="eosv_wino_weights_f32_device"):
            check(rc, "transform")
    torch.cuda.synchronize()
    assert bool((u == SENTINEL).all()), "a rejected call launched"
