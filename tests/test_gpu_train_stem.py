"""GPU: the opt-in direct 7x7 stem kernels of the training step (csrc/stem_train_f32.hip).

eosv_stem_conv_f32 computes z = conv 7x7 / 2 pad 3 (3 -> 64) of the NCHW frames into NHWC,
eosv_stem_wgrad_f32 the weight gradient dW [64][7][7][3] from the same frames and NHWC dz;
NativeTrainer(stem_direct=True) runs the stem on them instead of NHWC copy + im2col + GEMMs.

References are plain torch on the CPU in f64 (conv2d, autograd for dW).  Per shape, forward and
gradient:
1. exact: small-integer inputs, every partial sum an integer below 2^24, so the result must equal
   the f64 reference bitwise whatever the summation order; output between sentinel guards and
   NaN-filled before the call, workspace NaN-filled;
2. rounding: N(0,1) inputs, |got - ref| <= gamma_n (|w| * |x|) per element with
   gamma_n = n u / (1 - n u), u = 2^-24, n = 148 (forward) or N Ho Wo (gradient) -- the bound of any
   summation order -- and by norm at most max(4 x torch-f32's own distance from f64, 1e-6);
3. two calls are bitwise equal.
Then two trainer steps against the f64 replay with the bounds of _check_two_steps
(test_gpu_wino_wgrad.py, restated unchanged), the launch counter, the untouched default, determinism
and the fall-back at a width the kernels do not take.
"""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _expected_wino_launches, _oracle, _same_bytes, _small_case
from test_gpu_wino_wgrad import _expected_wgrad_launches, _references

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of the guarded buffers
SENTINEL = -7.25   # exact in f32
U = 2.0 ** -24

# (N, H, W): every output at a border; less than one 16-column tile and odd N; plain; odd H and a
# ragged second tile; the forward's ring wraps over 7 tiles; the width cap (eosv.h: W <= 256)
SHAPES = [(1, 8, 8), (5, 16, 12), (2, 32, 32), (3, 37, 40), (1, 224, 224), (2, 64, 256)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _conv64(x, w_ohwi):
    """f64-or-f32 stem conv of NCHW x with trainer-layout weights, as NHWC."""
    y = torch.nn.functional.conv2d(x, w_ohwi.permute(0, 3, 1, 2), stride=2, padding=3)
    return y.permute(0, 2, 3, 1).contiguous()


def _dw(x, dz_nhwc):
    """dW [64][7][7][3] by autograd in the dtype of x."""
    w = torch.zeros(64, 3, 7, 7, dtype=x.dtype, requires_grad=True)
    torch.nn.functional.conv2d(x, w, stride=2, padding=3).backward(dz_nhwc.permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(N, H, W, exact):
    """Inputs (f32, CPU) and the f64 references of one shape, computed once:
    x, w, dz, z_ref, z_mag, z_f32, dw_ref, dw_mag, dw_f32 (mag: the same sums over absolute values)."""
    g = torch.Generator().manual_seed(7000 + 100 * H + W + (1 if exact else 0))
    Ho, Wo = _out_hw(H, W)
    if exact:
        x = torch.randint(-3, 4, (N, 3, H, W), generator=g).float()
        w = torch.randint(-2, 3, (64, 7, 7, 3), generator=g).float()
        dz = torch.randint(-2, 3, (N, Ho, Wo, 64), generator=g).float()
    else:
        x = torch.randn(N, 3, H, W, generator=g)
        w = torch.randn(64, 7, 7, 3, generator=g)
        dz = torch.randn(N, Ho, Wo, 64, generator=g)
    xd, wd, dzd = x.double(), w.double(), dz.double()
    return dict(x=x, w=w, dz=dz, z_ref=_conv64(xd, wd), z_mag=_conv64(xd.abs(), wd.abs()), z_f32=_conv64(x, w),
                dw_ref=_dw(xd, dzd), dw_mag=_dw(xd.abs(), dzd.abs()), dw_f32=_dw(x, dz))


def _nan_guarded(t):
    """t's values inside a NaN-filled device buffer: (buffer, pointer to the values)."""
    v = t.contiguous().reshape(-1)
    buf = torch.full((v.numel() + 2 * GUARD,), float("nan"))
    buf[GUARD:GUARD + v.numel()] = v
    buf = buf.cuda()
    return buf, buf.data_ptr() + 4 * GUARD


def _guarded_out(n):
    out = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    out[GUARD:GUARD + n] = float("nan")
    return out


def _take(out, n, what):
    out = out.cpu()
    assert bool((out[:GUARD] == SENTINEL).all()) and bool((out[GUARD + n:] == SENTINEL).all()), \
        f"store outside {what}"
    got = out[GUARD:GUARD + n]
    assert bool(torch.isfinite(got).all()), f"{what}: an unwritten element, or a read outside the inputs"
    return got


def _run_fwd(N, H, W, exact):
    from eosv._lib import check, lib, stream_ptr

    c = _case(N, H, W, exact)
    Ho, Wo = _out_hw(H, W)
    xbuf, xp = _nan_guarded(c["x"])
    wbuf, wp = _nan_guarded(c["w"])
    n = N * Ho * Wo * 64
    out = _guarded_out(n)
    check(lib().eosv_stem_conv_f32(xp, N, H, W, wp, out.data_ptr() + 4 * GUARD, stream_ptr()), "eosv_stem_conv_f32")
    torch.cuda.synchronize()
    return _take(out, n, "z").view(N, Ho, Wo, 64)


def _run_wgrad(N, H, W, exact):
    from eosv._lib import check, lib, stream_ptr

    L = lib()
    c = _case(N, H, W, exact)
    xbuf, xp = _nan_guarded(c["x"])
    zbuf, zp = _nan_guarded(c["dz"])
    n = 64 * 147
    out = _guarded_out(n)
    wb = int(L.eosv_stem_wgrad_f32_workspace(N, H, W))
    assert wb > 0
    ws = torch.full((wb // 4 + 2 * GUARD,), float("nan"), device="cuda")
    ws[:GUARD] = SENTINEL
    ws[GUARD + wb // 4:] = SENTINEL
    check(L.eosv_stem_wgrad_f32(xp, zp, N, H, W, out.data_ptr() + 4 * GUARD, ws.data_ptr() + 4 * GUARD, wb,
                                stream_ptr()), "eosv_stem_wgrad_f32")
    torch.cuda.synchronize()
    ws = ws.cpu()
    assert bool((ws[:GUARD] == SENTINEL).all()) and bool((ws[GUARD + wb // 4:] == SENTINEL).all()), \
        "store outside the workspace"
    return _take(out, n, "dW").view(64, 7, 7, 3)


def _same_values(got, ref64, what):
    diff = got.double() != ref64
    assert not bool(diff.any()), (what, int(diff.sum()), "elements differ; first at",
                                  tuple(int(i) for i in diff.nonzero()[0]),
                                  float(got[diff][0]), float(ref64[diff][0]))


@pytest.mark.parametrize("N,H,W", SHAPES, ids=IDS)
def test_stem_conv_exact_on_integers(N, H, W):
    c = _case(N, H, W, True)
    assert float(c["z_mag"].max()) < 2 ** 24
    _same_values(_run_fwd(N, H, W, True), c["z_ref"], "z")


@pytest.mark.parametrize("N,H,W", SHAPES, ids=IDS)
def test_stem_wgrad_exact_on_integers(N, H, W):
    c = _case(N, H, W, True)
    assert float(c["dw_mag"].max()) < 2 ** 24
    _same_values(_run_wgrad(N, H, W, True), c["dw_ref"], "dW")


def _check_rounding(got, ref, mag, f32, n, what, shape):
    gamma = n * U / (1 - n * U)
    bound = gamma * mag
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    rel = float((got.double() - ref).norm() / ref.norm())
    yard = float((f32.double() - ref).norm() / ref.norm())
    print(f"{what} {shape}: max err / (gamma_{n} sum|terms|) = {worst:.3e}; norm-relative error {rel:.3e}, "
          f"torch-f32 {yard:.3e}, measured / bound = {rel / max(4 * yard, 1e-6):.3f}")
    assert bool((err <= bound).all()), (what, shape, worst)
    assert rel <= max(4 * yard, 1e-6), (what, shape, rel, yard)


@pytest.mark.parametrize("N,H,W", SHAPES, ids=IDS)
def test_stem_conv_rounding_vs_f64(N, H, W):
    c = _case(N, H, W, False)
    a = _run_fwd(N, H, W, False)
    _check_rounding(a, c["z_ref"], c["z_mag"], c["z_f32"], 148, "stem conv", (N, H, W))
    b = _run_fwd(N, H, W, False)
    assert a.numpy().tobytes() == b.numpy().tobytes(), "two forward calls differ"


@pytest.mark.parametrize("N,H,W", SHAPES, ids=IDS)
def test_stem_wgrad_rounding_vs_f64(N, H, W):
    c = _case(N, H, W, False)
    Ho, Wo = _out_hw(H, W)
    a = _run_wgrad(N, H, W, False)
    _check_rounding(a, c["dw_ref"], c["dw_mag"], c["dw_f32"], N * Ho * Wo, "stem wgrad", (N, H, W))
    b = _run_wgrad(N, H, W, False)
    assert a.numpy().tobytes() == b.numpy().tobytes(), "two gradient calls differ"


# ---------------------------------------------------------------- the trainer
LR1, LR2 = 1e-3, 1e-2  # as _references


def _check_bounds(name, tr, l0, l1, g0, refs, tag):
    """The assertions of _check_two_steps (test_gpu_wino_wgrad.py), bounds unchanged."""
    (ref_losses, ref_g, ref_sd), (f32_losses, f32_g, f32_sd) = refs
    print(f"[{name} {tag}] loss {l0:.6f} / {ref_losses[0]:.6f}, {l1:.6f} / {ref_losses[1]:.6f}")
    assert abs(l0 - ref_losses[0]) <= 1e-4 * abs(ref_losses[0])
    assert abs(l1 - ref_losses[1]) <= max(4 * abs(f32_losses[1] - ref_losses[1]), 1e-4 * abs(ref_losses[1]))
    worst = (0.0, None, 0.0)
    for k, gr in ref_g.items():
        norm = max(float(gr.norm()), 1e-12)
        err = float((g0[k].double() - gr).norm()) / norm
        yard = float((f32_g[k] - gr).norm()) / norm
        if err > worst[0]:
            worst = (err, k, yard)
        assert err <= max(4 * yard, 2e-2), (k, err, yard)
    print(f"[{name} {tag}] worst relative gradient error {worst[0]:.2e} at {worst[1]} "
          f"(torch-f32 yardstick there {worst[2]:.2e})")
    got = tr.state_dict()
    for k, v in ref_sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v), k
            continue
        v = v.double()
        err = float((got[k].double() - v).norm())
        yard = float((f32_sd[k].double() - v).norm())
        assert err <= max(4 * yard, 1e-6 * v.numel() ** 0.5 + 1e-5 * float(v.norm())), (k, err, yard)


def _two_steps(name, sd, frames, labels, T, refs, mask, direct_launches):
    tr = NativeTrainer(name, 64, device=0, winograd=mask, winograd_wgrad=mask, stem_direct=True)
    tr.load_state_dict(sd)
    l0, _ = tr.step(frames.cuda(), labels, T, LR1, LR2)
    assert tr.stem_direct_launches == direct_launches
    assert tr.wino_launches == (_expected_wino_launches(name, mask) if mask else 0)
    assert tr.wino_wgrad_launches == (_expected_wgrad_launches(name, mask) if mask else 0)
    g0 = tr.grads()
    l1, _ = tr.step(frames.cuda(), labels, T, LR1, LR2)
    assert tr.stem_direct_launches == direct_launches  # per step, not cumulative
    _check_bounds(name, tr, l0, l1, g0, refs, f"{tuple(frames.shape)} stem_direct, winograd masks {mask}")


@pytest.mark.parametrize("mask", [0, 15], ids=["alone", "with-winograd"])
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_train_step_stem_direct_matches_torch_reference(name, mask):
    frames, labels, T = _small_case()
    sd, ref64, ref32 = _references(name)
    _two_steps(name, sd, frames, labels, T, (ref64, ref32), mask, 2)


def test_train_step_falls_back_at_an_unsupported_width():
    """Frames 96 x 90 (W % 4 != 0): both stem calls return EOSV_ERR_UNSUPPORTED and take the im2col
    path; the step passes the same bounds."""
    torch.manual_seed(1)
    T = 4
    frames, labels = torch.randn(2 * T, 3, 96, 90), [3, 17]
    name = "resnet18"
    sd = synth.synth_state_dict(arch.SPECS[name], 64, 0)
    refs = (_oracle(name, sd, frames, labels, T, LR1, LR2, 2, torch.float64),
            _oracle(name, sd, frames, labels, T, LR1, LR2, 2, torch.float32))
    _two_steps(name, sd, frames, labels, T, refs, 0, 0)


@functools.lru_cache(maxsize=None)
def _r18_step(stem_direct):
    """(loss, grads, stem_direct_launches) of one step of a fresh ResNet-18 trainer on the small case;
    "default" builds the trainer without the keyword."""
    frames, labels, T = _small_case()
    kw = {} if stem_direct == "default" else {"stem_direct": stem_direct}
    tr = NativeTrainer("resnet18", 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS["resnet18"], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, LR1, LR2)
    return loss, tr.grads(), tr.stem_direct_launches


def test_default_step_untouched_by_the_keyword():
    a, b = _r18_step("default"), _r18_step(False)
    assert a[2] == 0 and b[2] == 0
    _same_bytes(a, b)
    # and the direct stem really is another computation (it did not fall back)
    d = _r18_step(True)
    assert d[2] == 2
    k = "convnet.0.weight"
    assert d[1][k].numpy().tobytes() != a[1][k].numpy().tobytes()


def test_stem_direct_step_is_deterministic():
    a = _r18_step(True)
    _r18_step.cache_clear()
    b = _r18_step(True)
    assert a[2] == b[2] == 2
    _same_bytes(a, b)
