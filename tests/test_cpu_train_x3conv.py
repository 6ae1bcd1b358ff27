"""The opt-in f32x3 implicit GEMMs of the training step's 3x3 and strided convs (csrc/conv_x3.hip),
the parts that need no device: the numpy model of the gathered operand (im2col + x3_terms, which
tests/test_gpu_train_x3conv.py imports), the entry points' argument checks (every status below is
returned before any device call), the workspace function, NativeTrainer(f32x3_convs=...) and its
plans, the dispatcher over an `x3c` route, and the drop-in's train_f32x3_convs."""
import ctypes
import types

import numpy as np
import pytest
import torch

from eosv import _lib
from test_cpu_train_routes import ALL, NONE, PART, UNSUPPORTED, _expected, _fake_trainer
from test_cpu_train_x3 import _library, _stub_device, x3_terms

NAMES = ("eosv_conv2d_x3", "eosv_conv_wgrad_x3_workspace", "eosv_conv_wgrad_x3")
ARG = -1
P = 4096  # a non-null, 16-byte aligned address; never dereferenced: every call below returns before a launch


# ---------------------------------------------------------------- the gather, in numpy
def conv_dims(N, H, W, k, stride, pad):
    """(Ho, Wo, P) of the output map."""
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return Ho, Wo, N * Ho * Wo


def im2col(x, k, stride, pad):
    """col(X) [P][K] of NHWC x, K = (kh, kw, c): the implicit GEMM's gathered operand, padding as zeros."""
    N, H, W, C = x.shape
    Ho, Wo, P_ = conv_dims(N, H, W, k, stride, pad)
    xp = np.zeros((N, H + 2 * pad, W + 2 * pad, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    taps = [xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            for kh in range(k) for kw in range(k)]
    return np.ascontiguousarray(np.concatenate(taps, axis=-1).reshape(P_, k * k * C))


def flip_weights(w):
    """eosv_flip_weights in numpy: w [Cout][KH][KW][Cin] -> [Cin][KH][KW][Cout], rotated by 180 degrees."""
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


@pytest.mark.parametrize("shape", [(2, 5, 7, 32, 64, 3, 1, 1), (3, 9, 6, 64, 128, 3, 2, 1), (2, 7, 5, 128, 256, 1, 2, 0)])
def test_im2col_model_equals_f64_conv2d_on_bf16_exact_integers(shape):
    N, H, W, Cin, Cout, k, stride, pad = shape
    rng = np.random.default_rng(Cin + k)
    x = rng.integers(-127, 128, size=(N, H, W, Cin)).astype(np.float32)
    w = rng.integers(-127, 128, size=(Cout, k, k, Cin)).astype(np.float32)
    dy = rng.integers(-127, 128, size=(conv_dims(N, H, W, k, stride, pad)[2], Cout)).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_()
    wt = torch.from_numpy(w).double().permute(0, 3, 1, 2).requires_grad_()
    y = torch.nn.functional.conv2d(xt, wt, stride=stride, padding=pad)
    A = im2col(x, k, stride, pad)
    assert np.array_equal(x3_terms(A, np.ascontiguousarray(w.reshape(Cout, -1).T)),
                          y.detach().permute(0, 2, 3, 1).reshape(-1, Cout).numpy())
    g = torch.from_numpy(dy).double().reshape(N, y.shape[2], y.shape[3], Cout).permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (xt, wt), g)
    assert np.array_equal(x3_terms(np.ascontiguousarray(dy.T), A), dw.permute(0, 2, 3, 1).reshape(Cout, -1).numpy())
    if stride == 1:   # the input gradient is the conv of dY with the flipped weights
        Ag = im2col(dy.reshape(N, H, W, Cout), k, 1, pad)
        assert np.array_equal(x3_terms(Ag, np.ascontiguousarray(flip_weights(w).reshape(Cin, -1).T)),
                              dx.permute(0, 2, 3, 1).reshape(-1, Cin).numpy())


# ---------------------------------------------------------------- the C ABI
def _entries(L):
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    conv = L.eosv_conv2d_x3
    conv.restype, conv.argtypes = i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    ws = L.eosv_conv_wgrad_x3_workspace
    ws.restype, ws.argtypes = i64, [i32] * 9
    wg = L.eosv_conv_wgrad_x3
    wg.restype, wg.argtypes = i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, i64, vp]
    L.eosv_last_error.restype = ctypes.c_char_p
    return conv, ws, wg


GOOD = dict(N=2, H=9, W=6, Cin=64, Cout=128, k=3, stride=2, pad=1)


def _conv(conv, x=P, w=P, add=None, y=P, kw=None, **over):
    d = dict(GOOD, **over)
    return conv(x, d["N"], d["H"], d["W"], d["Cin"], w, d["Cout"], d["k"], d["k"] if kw is None else kw, d["stride"],
                d["pad"], add, y, None)


def _wgrad(wg, x=P, dy=P, dw=P, work=None, bytes_=0, **over):
    d = dict(GOOD, **over)
    return wg(x, d["N"], d["H"], d["W"], d["Cin"], dy, d["Cout"], d["k"], d["k"], d["stride"], d["pad"], dw, work,
              bytes_, None)


def test_library_binding_and_header_declare_the_entry_points():
    import os
    import re

    L = _library()
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eosv.h")
    with open(header) as fh:
        text = fh.read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", text), f"{name} is not declared in include/eosv.h"
    B = _lib.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert B.eosv_conv2d_x3.argtypes == [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    assert B.eosv_conv_wgrad_x3_workspace.restype is i64 and B.eosv_conv_wgrad_x3_workspace.argtypes == [i32] * 9
    assert B.eosv_conv_wgrad_x3.argtypes == [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, i64, vp]


BAD_SIZES = [dict(N=-1), dict(H=0), dict(W=-3), dict(Cin=0), dict(Cout=0), dict(k=0), dict(stride=0), dict(pad=-1),
             dict(H=1, W=6, k=5, pad=1),    # an empty output map: 1 + 2 - 5 < 0
             dict(H=9, W=2, k=3, pad=0)]


def test_bad_arguments_are_rejected_before_any_device_call():
    L = _library()
    conv, ws, wg = _entries(L)
    for kw in [dict(x=None), dict(w=None), dict(y=None)] + BAD_SIZES:
        assert _conv(conv, **kw) == ARG, kw
        assert b"eosv_conv2d_x3" in L.eosv_last_error(), kw
    assert _conv(conv, kw=0) == ARG
    for kw in [dict(x=None), dict(dy=None), dict(dw=None), dict(bytes_=-1), dict(work=None, bytes_=4096)] + BAD_SIZES:
        assert _wgrad(wg, **kw) == ARG, kw
        assert b"eosv_conv_wgrad_x3" in L.eosv_last_error(), kw
    # where the plan splits, a workspace that cannot hold one slice
    big = dict(N=2, H=17, W=16, Cin=64, Cout=64, k=3, stride=1, pad=1)
    assert ws(2, 17, 16, 64, 64, 3, 3, 1, 1) == 2 * 64 * 576 * 4
    assert _wgrad(wg, work=P, bytes_=64 * 576 * 4 - 1, **big) == ARG
    assert b"workspace" in L.eosv_last_error()


def test_unsupported_shapes_and_pointers_name_the_operand():
    L = _library()
    conv, ws, wg = _entries(L)
    mis = P + 4
    for kw, word in [(dict(Cin=48), b"Cin"), (dict(Cin=16), b"Cin"), (dict(Cout=72), b"Cout"), (dict(Cout=32), b"Cout"),
                     (dict(x=mis), b"d_x"), (dict(w=mis), b"d_w"), (dict(add=mis), b"d_add"), (dict(y=mis), b"d_y"),
                     (dict(N=1 << 20, H=1 << 12, W=1 << 12, stride=1), b"grid")]:
        assert _conv(conv, **kw) == UNSUPPORTED, kw
        assert b"eosv_conv2d_x3" in L.eosv_last_error() and word in L.eosv_last_error(), (kw, L.eosv_last_error())
    for kw, word in [(dict(Cin=48), b"Cin"), (dict(Cout=72), b"Cout"), (dict(x=mis), b"d_x"), (dict(dy=mis), b"d_dy"),
                     (dict(dw=mis), b"d_dw"), (dict(work=mis, bytes_=1 << 30), b"d_work")]:
        assert _wgrad(wg, **kw) == UNSUPPORTED, kw
        assert b"eosv_conv_wgrad_x3" in L.eosv_last_error() and word in L.eosv_last_error(), (kw, L.eosv_last_error())
    # other filters, strides and paddings with a non-empty map are shapes like any other: no status to
    # test without a device, but the workspace function takes them
    assert ws(4, 40, 33, 32, 64, 5, 3, 3, 2) >= 0


def test_an_empty_batch_is_nothing_to_do():
    L = _library()
    conv, ws, wg = _entries(L)
    assert _conv(conv, N=0) == 0 and _wgrad(wg, N=0) == 0
    assert _conv(conv, N=0, Cin=48, x=P + 4) == 0   # nothing would be read
    assert ws(0, 9, 6, 64, 128, 3, 3, 2, 1) == 0


def test_workspace_is_whole_slices_monotone_in_the_pixel_count_and_reads_no_device():
    L = _library()
    _, ws, _ = _entries(L)
    for bad in ((-1, 9, 6, 64, 128, 3, 3, 2, 1), (2, 0, 6, 64, 128, 3, 3, 2, 1), (2, 9, 6, 48, 128, 3, 3, 2, 1),
                (2, 9, 6, 64, 72, 3, 3, 2, 1), (2, 1, 6, 64, 128, 5, 5, 1, 1)):
        assert ws(*bad) == 0, bad
    for Cin, Cout, k, stride in ((64, 64, 3, 1), (64, 128, 3, 2), (256, 512, 1, 2), (512, 512, 3, 1), (32, 64, 3, 1)):
        one = Cout * k * k * Cin * 4
        sizes = [ws(N, 24, 23, Cin, Cout, k, k, stride, k // 2) for N in (1, 2, 3, 8, 32, 96, 400)]
        assert sizes == sorted(sizes), (Cin, Cout, k, sizes)
        assert all(b % one == 0 and b != one and b <= 1024 * one for b in sizes), (Cin, Cout, k, sizes)
        assert sizes[-1] > 0
    # under two slices' worth of pixels (2 x 256) the reduction is never split
    assert ws(1, 12, 11, 96, 64, 3, 3, 1, 1) == 0 and ws(2, 5, 7, 32, 64, 3, 3, 1, 1) == 0
    # fixed numbers: the plan's CU count is a constant, so no device is asked (this test runs without one)
    assert ws(96, 24, 23, 64, 64, 3, 3, 1, 1) == 154 * 64 * 576 * 4
    assert ws(2, 17, 16, 64, 64, 3, 3, 1, 1) == 2 * 64 * 576 * 4


# ---------------------------------------------------------------- the trainer's keyword and plans
def _expected_x3c(c, f32x3_convs, **switches):
    """The routes with the switch: today's rule, and `x3c` where the conv is eligible: first in the forward,
    after x3 in the weight gradient, before wino / conv in a stride-1 input gradient."""
    want = {job: list(r) for job, r in _expected(c, **switches).items()}
    stem = c.name == "convnet.0"
    stage = None if stem else int(c.name.split(".")[1]) - 4
    if stem or not (f32x3_convs >> stage & 1) or c.cin % 32 or (c.k == 1 and c.stride == 1):
        return {job: tuple(r) for job, r in want.items()}, False
    want["fwd"].insert(0, "x3c")
    want["wgrad"].insert(0, "x3c")
    if c.stride == 1 and c.k % 2 == 1 and c.pad == c.k // 2:
        want["dgrad"].insert(0, "x3c")
    return {job: tuple(r) for job, r in want.items()}, True


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
@pytest.mark.parametrize("switches", [NONE, ALL, PART], ids=["none", "all", "part"])
def test_plans_with_the_switch_off_and_on(monkeypatch, arch, switches):
    train = _stub_device(monkeypatch)
    for off in (dict(), dict(f32x3_convs=False), dict(f32x3_convs=0)):
        tr = train.NativeTrainer(arch, 4, **switches, **off)
        assert tr.x3c_mask == 0 and tr.x3c_launches == 0
        for c in tr._convs():
            assert c.x3c is False and c.routes == _expected(c, **switches), c.name
    for mask in (15, 6):
        tr = train.NativeTrainer(arch, 4, **switches, f32x3_convs=mask)
        assert tr.x3c_mask == mask
        on = 0
        for c in tr._convs():
            want, eligible = _expected_x3c(c, mask, **switches)
            assert c.routes == want and c.x3c is eligible, (c.name, c.routes, want)
            assert not (c.x3 and c.x3c), c.name
            assert ("x3c" in c.routes["fwd"]) == ("x3c" in c.routes["wgrad"]) == c.x3c
            on += c.x3c
        assert on == {15: 19, 6: 10 if arch == "resnet18" else 12}[mask]
        assert not tr.stem.x3c


def test_plans_by_name(monkeypatch):
    train = _stub_device(monkeypatch)

    def conv(tr, name):
        return next(c for c in tr._convs() if c.name == name)

    tr = train.NativeTrainer("resnet18", 4, f32x3_convs=15, winograd=15, winograd_wgrad=15)
    c = conv(tr, "convnet.4.0.conv2")   # doubly eligible: x3c first, Winograd takes what it refuses
    assert c.routes == {"fwd": ("x3c", "wino"), "wgrad": ("x3c", "wino", "conv", "gemm"), "dgrad": ("x3c", "wino")}
    c = conv(tr, "convnet.5.0.conv1")   # 3x3 stride 2: the input gradient stays on the GEMM
    assert c.routes == {"fwd": ("x3c", "conv", "gemm"), "wgrad": ("x3c", "conv", "gemm"), "dgrad": ("gemm",)}
    c = conv(tr, "convnet.5.0.downsample.0")
    assert c.routes == {"fwd": ("x3c", "conv", "gemm"), "wgrad": ("x3c", "conv", "gemm"), "dgrad": ("gemm",)}
    tr = train.NativeTrainer("resnet50", 4, f32x3=15, f32x3_convs=15)
    c = conv(tr, "convnet.5.0.conv3")   # f32x3 owns the stride-1 1x1 convs
    assert c.routes == {"fwd": ("x3", "conv", "gemm"), "wgrad": ("x3", "gemm"), "dgrad": ("x3", "conv", "gemm")}
    assert not conv(tr, "convnet.4.0.downsample.0").x3c and conv(tr, "convnet.4.0.downsample.0").x3
    c = conv(tr, "convnet.5.0.conv2")
    assert c.routes == {"fwd": ("x3c", "conv", "gemm"), "wgrad": ("x3c", "conv", "gemm"), "dgrad": ("gemm",)}
    c = conv(tr, "convnet.5.1.conv2")
    assert c.routes == {"fwd": ("x3c", "conv", "gemm"), "wgrad": ("x3c", "conv", "gemm"),
                        "dgrad": ("x3c", "conv", "gemm")}
    # f32x3 alone still leaves the stride-2 shortcut without any x3 route
    c = conv(train.NativeTrainer("resnet50", 4, f32x3=15), "convnet.5.0.downsample.0")
    assert not any("x3" in r or "x3c" in r for r in c.routes.values())


def test_stage_mask_parses_f32x3_convs(monkeypatch):
    train = _stub_device(monkeypatch)
    assert 0 <= train.TRAIN_X3C_DEFAULT <= 15
    assert train.NativeTrainer("resnet18", 4, f32x3_convs=True).x3c_mask == train.TRAIN_X3C_DEFAULT
    assert train.NativeTrainer("resnet18", 4, f32x3_convs=np.int64(9)).x3c_mask == 9
    for bad in (16, -1, 1.0, "15"):
        with pytest.raises(ValueError, match="f32x3_convs"):
            train.NativeTrainer("resnet18", 4, f32x3_convs=bad)
    # independent of the other four switches
    tr = train.NativeTrainer("resnet50", 4, f32x3_convs=3, winograd=4, winograd_wgrad=8, f32x3=2, stem_direct=True)
    assert (tr.x3c_mask, tr.wino_mask, tr.wino_wgrad_mask, tr.x3_mask, tr.stem_direct) == (3, 4, 8, 2, True)


COUNTERS = ("stem_direct_launches", "wino_launches", "wino_wgrad_launches", "x3_launches", "x3c_launches")


def _counts(tr):
    return {k: getattr(tr, k) for k in COUNTERS}


@pytest.mark.parametrize("job,statuses,winner,counter", [
    ("fwd", {"x3c": 0, "wino": 0}, "x3c", "x3c_launches"),
    ("fwd", {"x3c": UNSUPPORTED, "wino": 0}, "wino", "wino_launches"),
    ("wgrad", {"x3": UNSUPPORTED, "x3c": 0, "wino": 0, "conv": 0, "gemm": 0}, "x3c", "x3c_launches"),
    ("wgrad", {"x3c": UNSUPPORTED, "wino": 0, "conv": 0, "gemm": 0}, "wino", "wino_wgrad_launches"),
    ("dgrad", {"x3c": 0, "conv": 0, "gemm": 0}, "x3c", "x3c_launches"),
    ("dgrad", {"x3c": UNSUPPORTED, "conv": 0, "gemm": 0}, "conv", None),
])
def test_x3c_route_in_the_dispatcher(monkeypatch, job, statuses, winner, counter):
    tr, c, asked = _fake_trainer(monkeypatch, job, statuses)
    tr.x3c_launches = 3   # counted from where it stands
    before = _counts(tr)
    tr._run(job, c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(winner) + 1]
    want = dict(before)
    if counter:
        want[counter] += 1
    assert _counts(tr) == want


@pytest.mark.parametrize("job,statuses,culprit", [
    ("fwd", {"x3c": ARG, "conv": 0, "gemm": 0}, "x3c"),              # a failure is no refusal
    ("wgrad", {"x3c": -2, "wino": 0, "gemm": 0}, "x3c"),
    ("dgrad", {"x3c": UNSUPPORTED, "wino": UNSUPPORTED}, "wino"),    # Winograd's refusal still raises
])
def test_x3c_failures_raise_under_the_library_functions_name(monkeypatch, job, statuses, culprit):
    tr, c, asked = _fake_trainer(monkeypatch, job, statuses)
    before = _counts(tr)
    with pytest.raises(_lib.EosvError, match=f"eosv_fake_{culprit} failed"):
        tr._run(job, c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(culprit) + 1]
    assert _counts(tr) == before


def test_x3c_routes_call_the_library_with_the_convs_geometry(monkeypatch):
    """The three routes over a recording library: the forward passes no addend, the weight gradient asks
    for its workspace under the "splitk" key, the input gradient flips the weights and runs the conv over
    the output map with the residual gradient as the addend."""
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer("resnet18", 4, f32x3_convs=15)
    c = next(c for c in tr._convs() if c.name == "convnet.5.1.conv1")
    calls = []

    def rec(name, rc=0):
        def fn(*a):
            calls.append((name, a))
            return rc
        return fn

    tr.L = types.SimpleNamespace(eosv_conv2d_x3=rec("conv"), eosv_conv_wgrad_x3=rec("wgrad"),
                                 eosv_conv_wgrad_x3_workspace=rec("ws", 4096), eosv_flip_weights=rec("flip"))
    buf = types.SimpleNamespace(data_ptr=lambda: 64)
    monkeypatch.setattr(tr, "_buf", lambda key, n: calls.append(("buf", key)) or buf)
    t = lambda p: types.SimpleNamespace(data_ptr=lambda: p)   # noqa: E731
    c.w, c.g = t(1600), t(3200)
    shape = (2, 12, 11, c.cin)
    assert tr._fwd_x3c(c, t(16), shape, 264, None, t(32), None, 7) == (0, "eosv_conv2d_x3")
    assert calls.pop() == ("conv", (16, 2, 12, 11, 128, 1600, 128, 3, 3, 1, 1, None, 32, 7))
    assert tr._wgrad_x3c(c, t(16), shape, 264, t(48), None, None, 7) == (0, "eosv_conv_wgrad_x3")
    assert calls == [("ws", (2, 12, 11, 128, 128, 3, 3, 1, 1)), ("buf", "splitk"),
                     ("wgrad", (16, 2, 12, 11, 128, 48, 128, 3, 3, 1, 1, 3200, 64, 4096, 7))]
    del calls[:]
    assert tr._dgrad_x3c(c, None, shape, 264, t(48), t(80), t(96), 7) == (0, "eosv_conv2d_x3")
    assert calls == [("buf", "wflip"), ("flip", (1600, 128, 3, 3, 128, 64, 7)),
                     ("conv", (48, 2, 12, 11, 128, 64, 128, 3, 3, 1, 1, 96, 80, 7))]


def test_train_network_passes_train_f32x3_convs_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_f32x3_convs defaults to False and is read at finetune_model time; False passes no
    keyword at all."""
    import network_train

    assert network_train.TrainNetwork.train_f32x3_convs is False
    seen = []

    class Stub:
        def __init__(self, arch, num_classes, device=0, winograd=False, **kw):
            seen.append(kw)

        def load_state_dict(self, sd):
            pass

        def state_dict(self):
            return {}

    monkeypatch.setattr(network_train, "NativeTrainer", Stub)
    monkeypatch.setattr(network_train, "VideoDataset", lambda *a, **k: [])
    monkeypatch.setattr(network_train, "DataLoader", lambda *a, **k: [])
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    model = types.SimpleNamespace(state_dict=lambda: {}, load_state_dict=lambda sd: None)
    for value in (False, True, 6):
        tn = object.__new__(network_train.TrainNetwork)
        tn.__dict__.update(loss_path=str(tmp_path / "loss.txt"), ckp_path=str(tmp_path) + "/", epoch_nums=0,
                           batch_size=2, lr_1=1e-4, lr_2=1e-3, lr_step_size=10, resnet_model="resnet50",
                           num_classes=64, mymodel=model)
        if value is not False:
            tn.train_f32x3_convs = value
        tn.finetune_model()
    assert seen == [{}, {"f32x3_convs": True}, {"f32x3_convs": 6}]
