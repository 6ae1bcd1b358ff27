"""GPU: the opt-in Winograd-domain weight gradient of the training step.

eosv_conv_wgrad_wino_f32 (csrc/conv_wgrad_wino_f32.hip) computes dW of a stride-1 pad-1 3x3 conv with
Cin = Cout = C as dU[pos] = sum over 2x2 tiles of (A dY A^T)[pos] (B^T d B)[pos]^T, sliced over the
tiles, each slice's G^T dU G written to a workspace and the slices summed in a fixed order;
NativeTrainer(winograd_wgrad=mask) runs the weight gradient of every eligible conv on it.

1. the kernel against f64 autograd under the conv rule of test_gpu_wino.py,
   |err| <= 1e-5 (1 + sum |terms|) per element, and the norm-relative bound 1e-5 that
   test_gpu_train.py puts on eosv_conv_wgrad_f32; guarded buffers;
2. determinism, also over a NaN-filled workspace;
3. two trainer steps against the f64 replay with the bounds of tests/test_gpu_train.py (_oracle and
   _check_two_steps of test_gpu_train_wino.py restated with their bounds unchanged), the launch counts
   from the architecture;
4. the default path is untouched; 5. step determinism.
"""
import functools

import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _expected_wino_launches, _oracle, _same_bytes, _small_case

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of the guarded buffers
SENTINEL = -7.25   # exact in f32, never a gradient of these inputs by chance

# (N, H, W, C, single_slice):
#   1x1x1: one tile, 12 of 16 patch taps and 3 of 4 outputs outside the image
#   3x7x5: odd H and W, a ragged chunk, a chunk straddling frames, 36 tiles
#   2x14x14x128: a 2 x 2 grid of channel blocks (x and dY independent: a co / ci swap fails)
#   5x28x28: 980 tiles, several slices with a ragged last one; again with one slice's workspace
#   2x4x4x256: 16 channel blocks over 8 tiles, a single partial chunk per block
CASES = [(1, 1, 1, 64, False), (3, 7, 5, 64, False), (2, 14, 14, 128, False), (5, 28, 28, 64, False),
         (5, 28, 28, 64, True), (2, 4, 4, 256, False)]


@functools.lru_cache(maxsize=None)
def _case(N, H, W, C):
    """x, dY (f32, NCHW, CPU), the f64 dW [co][3][3][ci] and the sum of |terms| per element."""
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
    x = torch.randn(N, C, H, W, generator=g)
    dy = torch.randn(N, C, H, W, generator=g)

    def dw(xv, dyv):
        w = torch.zeros(C, C, 3, 3, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xv.double(), w, padding=1).backward(dyv.double())
        return w.grad.permute(0, 2, 3, 1).contiguous()

    return x, dy, dw(x, dy), dw(x.abs(), dy.abs())


def _nan_guarded(t_nchw):
    """The NHWC values inside a NaN-filled device buffer; returns (buffer, pointer to the values)."""
    v = t_nchw.permute(0, 2, 3, 1).contiguous().reshape(-1)
    buf = torch.full((v.numel() + 2 * GUARD,), float("nan"))
    buf[GUARD:GUARD + v.numel()] = v
    buf = buf.cuda()
    return buf, buf.data_ptr() + 4 * GUARD


def _run(N, H, W, C, single_slice=False, work_fill=None):
    """dW [co][3][3][ci] (CPU, f32) of the case from the kernel, with every buffer guarded."""
    from eosv._lib import check, lib, stream_ptr

    L = lib()
    x, dy, _, _ = _case(N, H, W, C)
    xbuf, xp = _nan_guarded(x)
    ybuf, yp = _nan_guarded(dy)
    n = 9 * C * C
    out = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    wb = int(L.eosv_conv_wgrad_wino_f32_workspace(N, H, W, C))
    one = 16 * C * C * 4
    assert wb >= one
    if single_slice:
        assert wb > one, "the shape was meant to have several slices"
        wb = one
    ws = torch.empty(wb // 4, device="cuda")
    if work_fill is not None:
        ws.fill_(work_fill)
    check(L.eosv_conv_wgrad_wino_f32(xp, yp, N, H, W, C, out.data_ptr() + 4 * GUARD, ws.data_ptr(), wb, stream_ptr()),
          "eosv_conv_wgrad_wino_f32")
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + n:] == SENTINEL).all()), "store outside dW"
    got = out[GUARD:GUARD + n]
    assert bool((got != SENTINEL).all()), "a dW slot was not written"
    assert bool(torch.isfinite(got).all()), "non-finite dW: a read outside x or dY, or of an unwritten partial"
    return got.view(C, 3, 3, C)


@pytest.mark.parametrize("N,H,W,C,single", CASES,
                         ids=lambda v: str(int(v)) if not isinstance(v, bool) else ("one" if v else "full"))
def test_wino_wgrad_vs_f64(N, H, W, C, single):
    from eosv._lib import lib

    _, _, ref, mag = _case(N, H, W, C)
    if (N, H, W, C) == (5, 28, 28, 64):
        # really multi-slice, and 980 tiles over equal slices of whole chunks leave a ragged last one
        assert int(lib().eosv_conv_wgrad_wino_f32_workspace(N, H, W, C)) > 16 * C * C * 4
    got = _run(N, H, W, C, single)
    err = (got.double() - ref).abs()
    bound = 1e-5 * (1.0 + mag)
    worst = float((err / bound).max())
    rel = float((got.double() - ref).norm() / ref.norm())
    print(f"wino wgrad {(N, H, W, C)} single_slice={single}: max err / bound = {worst:.3e}, "
          f"norm-relative error = {rel:.3e}")
    assert worst <= 1.0
    assert rel < 1e-5


def test_wino_wgrad_is_deterministic():
    a = _run(5, 28, 28, 64)
    b = _run(5, 28, 28, 64)
    assert a.numpy().tobytes() == b.numpy().tobytes()
    c = _run(5, 28, 28, 64, work_fill=float("nan"))  # every partial that is read was written
    assert a.numpy().tobytes() == c.numpy().tobytes()


# ---------------------------------------------------------------- the trainer
def _expected_wgrad_launches(name, mask=15):
    """One weight gradient per eligible conv: half of forward + input gradient."""
    return _expected_wino_launches(name, mask) // 2


@functools.lru_cache(maxsize=None)
def _references(name):
    """The f64 and torch-f32 replays of two steps on the small case (shared by the two masks)."""
    frames, labels, T = _small_case()
    lr1, lr2 = 1e-3, 1e-2  # 10x the reference's (network_train.py:140)
    sd = synth.synth_state_dict(arch.SPECS[name], 64, 0)
    return (sd, _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float64),
            _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float32))


def _check_two_steps(name, frames, labels, T, H, winograd, winograd_wgrad):
    lr1, lr2 = 1e-3, 1e-2
    sd, (ref_losses, ref_g, ref_sd), (f32_losses, f32_g, f32_sd) = _references(name)

    tr = NativeTrainer(name, 64, device=0, winograd=winograd, winograd_wgrad=winograd_wgrad)
    tr.load_state_dict(sd)
    l0, logits = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.wino_launches == _expected_wino_launches(name, winograd)
    assert tr.wino_wgrad_launches == _expected_wgrad_launches(name, winograd_wgrad) > 0
    g0 = tr.grads()
    l1, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.wino_launches == _expected_wino_launches(name, winograd)  # per step, not cumulative
    assert tr.wino_wgrad_launches == _expected_wgrad_launches(name, winograd_wgrad)
    print(f"[{name} {tuple(frames.shape)} wino {winograd} wgrad {winograd_wgrad}] loss {l0:.6f} / {ref_losses[0]:.6f}, "
          f"{l1:.6f} / {ref_losses[1]:.6f}; {tr.wino_wgrad_launches} Winograd weight gradients per step")
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
    print(f"[{name} wino {winograd} wgrad {winograd_wgrad}] worst relative gradient error {worst[0]:.2e} at "
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


def test_expected_wgrad_launch_counts():
    assert _expected_wgrad_launches("resnet18") == 13 and _expected_wgrad_launches("resnet50") == 13


@pytest.mark.parametrize("winograd", [0, 15], ids=["alone", "with-winograd"])
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_train_step_winograd_wgrad_matches_torch_reference(name, winograd):
    frames, labels, T = _small_case()
    _check_two_steps(name, frames, labels, T, frames.shape[-1], winograd, 15)


@functools.lru_cache(maxsize=None)
def _r18_step(winograd, winograd_wgrad):
    """(loss, grads, wino_wgrad_launches) of one step of a fresh ResNet-18 trainer on the small case;
    winograd_wgrad "default" builds the trainer without the keyword."""
    frames, labels, T = _small_case()
    kw = {} if winograd_wgrad == "default" else {"winograd_wgrad": winograd_wgrad}
    tr = NativeTrainer("resnet18", 64, device=0, winograd=winograd, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS["resnet18"], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr.wino_wgrad_launches


def test_default_step_untouched_by_the_keyword():
    a, b, c = _r18_step(False, "default"), _r18_step(False, False), _r18_step(False, 0)
    assert a[2] == 0 and b[2] == 0 and c[2] == 0
    _same_bytes(a, b)
    _same_bytes(a, c)
    # and the Winograd weight gradient really is another computation (it did not fall back)
    d = _r18_step(False, 15)
    assert d[2] == _expected_wgrad_launches("resnet18")
    assert any(d[1][k].numpy().tobytes() != a[1][k].numpy().tobytes() for k in a[1] if "conv" in k)


def test_winograd_wgrad_step_is_deterministic():
    a = _r18_step(15, 15)
    _r18_step.cache_clear()
    b = _r18_step(15, 15)
    assert a[2] == b[2] == _expected_wgrad_launches("resnet18")
    _same_bytes(a, b)
