"""The opt-in f32x3 implicit GEMM of the stride-2 convs' input gradient (csrc/conv_dgrad_x3.hip), the
parts that need no device: the numpy model of the parity-class gather (dgrad_classes, dgrad_gather,
dgrad_weights + x3_terms, which tests/test_gpu_train_x3dgrad.py imports as the x3c tests import im2col),
the entry point's argument checks (every status below is returned before any device call),
NativeTrainer(f32x3_dgrad=...) and its plans, the dispatcher over an `x3d` route, and the drop-in's
train_f32x3_dgrad.

Shapes are (N, H, W, Cin, Cout, k, stride, pad), H, W, Cin the conv's input, i.e. dX."""
import ctypes
import types

import numpy as np
import pytest
import torch

from eosv import _lib
from test_cpu_train_routes import ALL, NONE, PART, UNSUPPORTED, _expected, _fake_trainer
from test_cpu_train_x3 import _library, _stub_device, x3_terms
from test_cpu_train_x3conv import _expected_x3c, conv_dims, flip_weights, im2col

ARG = -1
P = 4096  # a non-null, 16-byte aligned address; never dereferenced: every call below returns before a launch

# what each shape is there for: the docstring of tests/test_gpu_train_x3dgrad.py
SHAPES = {"a": (3, 9, 6, 64, 128, 3, 2, 1), "b": (2, 7, 5, 128, 256, 1, 2, 0), "c": (2, 8, 6, 64, 64, 3, 2, 1),
          "d": (1, 3, 2, 64, 64, 3, 2, 1), "e": (1, 2, 2, 64, 64, 3, 2, 1), "f": (1, 12, 11, 64, 32, 7, 2, 3),
          "g": (2, 6, 9, 64, 64, 3, 2, 0), "h": (2, 5, 4, 64, 32, 2, 2, 0), "i": (2, 17, 16, 64, 64, 3, 2, 1),
          "j": (1, 4, 4, 128, 512, 3, 2, 1),
          # strides 3 and 4: 9 and 16 classes, some without a tap along one axis
          "k": (2, 10, 7, 64, 32, 3, 3, 1), "l": (1, 9, 10, 64, 32, 3, 4, 1)}
# 512 tiles of the unhalved size keep the other three instantiations under the library's fixed plan: sid ->
# (shape, rows x columns of the tile eosv_conv_dgrad_x3_plan must report)
LARGE = {"m": ((1, 512, 512, 64, 32, 3, 2, 1), (128, 64)), "n": ((1, 512, 512, 128, 32, 3, 2, 1), (128, 128)),
         "o": ((1, 256, 256, 256, 32, 3, 2, 1), (64, 128))}
# per frame: pixels in classes no tap reaches, and pixels of the other classes whose taps all fall outside the map
TAPLESS_DEAD = {"a": (0, 0), "b": (23, 0), "c": (0, 0), "d": (0, 0), "e": (0, 0), "f": (0, 0), "g": (0, 9),
                "h": (0, 4), "i": (0, 0), "j": (0, 0)}


# ---------------------------------------------------------------- the gather, in numpy
def dgrad_classes(H, W, k, stride, pad):
    """The parity classes of one frame's input pixels, in the kernel's order (ph, pw): dicts with hs, ws (the
    class's rows and columns of dX), khs, kws (the taps that reach it, increasing)."""
    out = []
    for ph in range(stride):
        for pw in range(stride):
            out.append(dict(ph=ph, pw=pw, hs=np.arange((ph - pad) % stride, H, stride),
                            ws=np.arange((pw - pad) % stride, W, stride),
                            khs=list(range(ph, k, stride)), kws=list(range(pw, k, stride))))
    return out


def dgrad_gather(dy, H, W, k, stride, pad):
    """A [N H W][k k Cout], columns in (kh, kw, co) order: row (n, h, w) holds dY[n, (h + pad - kh) / stride,
    (w + pad - kw) / stride, :] at tap (kh, kw) where both quotients are exact and inside the output map, zeros
    elsewhere.  Filled class by class, as the kernel gathers: within a class tap jh reads output row oh0 - jh."""
    N, Ho, Wo, Cout = dy.shape
    A = np.zeros((N, H, W, k * k, Cout), dy.dtype)
    for c in dgrad_classes(H, W, k, stride, pad):
        oh0, ow0 = (c["hs"] + pad - c["ph"]) // stride, (c["ws"] + pad - c["pw"]) // stride
        for jh, kh in enumerate(c["khs"]):
            for jw, kw in enumerate(c["kws"]):
                oh, ow = oh0 - jh, ow0 - jw
                vh, vw = (oh >= 0) & (oh < Ho), (ow >= 0) & (ow < Wo)
                A[np.ix_(range(N), c["hs"][vh], c["ws"][vw], [kh * k + kw])] = \
                    dy[np.ix_(range(N), oh[vh], ow[vw])][:, :, :, None, :]
    return np.ascontiguousarray(A.reshape(N * H * W, k * k * Cout))


def dgrad_weights(w):
    """B [k k Cout][Cin] of w [Cout][k][k][Cin], rows in (kh, kw, co) order."""
    return np.ascontiguousarray(w.transpose(1, 2, 0, 3).reshape(-1, w.shape[3]))


def dgrad_untouched(N, H, W, k, stride, pad):
    """(tapless, dead): boolean [N H W] masks of the pixels in classes without a tap, and of the pixels of the
    other classes whose taps all fall outside the output map.  Both receive 0 + addend."""
    Ho, Wo, _ = conv_dims(1, H, W, k, stride, pad)
    tapless, reached = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for c in dgrad_classes(H, W, k, stride, pad):
        if not c["khs"] or not c["kws"]:
            tapless[np.ix_(c["hs"], c["ws"])] = True
    for h in range(H):
        for w in range(W):
            reached[h, w] = any((h + pad - kh) % stride == 0 and 0 <= (h + pad - kh) // stride < Ho and
                                (w + pad - kw) % stride == 0 and 0 <= (w + pad - kw) // stride < Wo
                                for kh in range(k) for kw in range(k))
    assert not (tapless & reached).any()
    dead = ~reached & ~tapless
    return np.tile(tapless.reshape(-1), N), np.tile(dead.reshape(-1), N)


def dgrad_plan(shape, expect=0):
    """(tile rows, tile columns, workgroups) the library would launch for `shape`: its own decision, asked of
    eosv_conv_dgrad_x3_plan, which reads no device."""
    N, H, W, Cin, Cout, k, stride, pad = shape
    fn = _library().eosv_conv_dgrad_x3_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.POINTER(ctypes.c_int64)]
    tm, tn, grid = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = fn(N, H, W, Cin, Cout, k, k, stride, pad, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(grid))
    assert rc == expect, (shape, rc)
    return tm.value, tn.value, grid.value


def ref_dx(w, dy, H, W, stride, pad):
    """dX [N H W][Cin] of conv2d in f64 by autograd, for w [Cout][k][k][Cin] and dY [N][Ho][Wo][Cout]."""
    N, Cin = dy.shape[0], w.shape[3]
    x = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x, torch.from_numpy(w).double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    dx, = torch.autograd.grad(y, x, torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    return dx.permute(0, 2, 3, 1).reshape(-1, Cin).numpy()


@pytest.mark.parametrize("sid", list(SHAPES))
def test_class_gather_equals_f64_autograd_on_bf16_exact_integers(sid):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    Ho, Wo, _ = conv_dims(N, H, W, k, stride, pad)
    rng = np.random.default_rng(ord(sid))
    w = rng.integers(-127, 128, size=(Cout, k, k, Cin)).astype(np.float32)
    dy = rng.integers(-127, 128, size=(N, Ho, Wo, Cout)).astype(np.float32)
    A, B = dgrad_gather(dy, H, W, k, stride, pad), dgrad_weights(w)
    ref = ref_dx(w, dy, H, W, stride, pad)
    assert np.array_equal(x3_terms(A, B), ref)
    # a row of the flipped copy, read at the kernel's k offset, is the column of B
    wf = flip_weights(w).reshape(Cin, k * k, Cout)
    for kh, kw in ((0, 0), (k - 1, 0), (k // 2, k - 1)):
        off = (k - 1 - kh) * k + (k - 1 - kw)
        assert np.array_equal(wf[:, off, :].T, B.reshape(k * k, Cout, Cin)[kh * k + kw])
    # the kernel's grid is the classes' row tiles x the column tiles, every class on the tile the plan picked
    tm, tn, grid = dgrad_plan(SHAPES[sid])
    assert grid == sum(-(-N * len(c["hs"]) * len(c["ws"]) // tm) for c in dgrad_classes(H, W, k, stride, pad)) * \
        -(-Cin // tn)
    # the pixels that receive nothing: exact zeros of the reference, and as many as the shape is there for
    tapless, dead = dgrad_untouched(N, H, W, k, stride, pad)
    assert not A[tapless | dead].any() and not ref[tapless | dead].any()
    if sid in TAPLESS_DEAD:
        assert (int(tapless.sum()) // N, int(dead.sum()) // N) == TAPLESS_DEAD[sid]
    # the classes' gathers together read what the forward's im2col writes: one slot per (output pixel, tap)
    # whose input pixel lies inside the image, so the MACs are the explicit GEMM's
    ones = dgrad_gather(np.ones((1, Ho, Wo, 1), np.float32), H, W, k, stride, pad)
    assert ones.sum() == im2col(np.ones((1, H, W, 1), np.float32), k, stride, pad).sum()
    slots = sum(len(c["hs"]) * len(c["ws"]) * len(c["khs"]) * len(c["kws"]) for c in dgrad_classes(H, W, k, stride, pad))
    assert ones.sum() <= slots <= H * W * ((k + stride - 1) // stride) ** 2


def test_the_shapes_reach_what_they_are_listed_for():
    def rows(sid):
        N, H, W, _, _, k, stride, pad = SHAPES[sid]
        return [len(c["hs"]) * len(c["ws"]) for c in dgrad_classes(H, W, k, stride, pad)], N

    def taps(sid):
        _, H, W, _, _, k, stride, pad = SHAPES[sid]
        return [len(c["khs"]) * len(c["kws"]) for c in dgrad_classes(H, W, k, stride, pad)]

    assert sorted(rows("a")[0]) == [12, 12, 15, 15]
    assert taps("b") == [1, 0, 0, 0]
    assert sorted(rows("d")[0]) == [1, 1, 2, 2] and sorted(rows("e")[0]) == [1, 1, 1, 1]
    assert sorted(taps("f")) == [9, 12, 12, 16] and SHAPES["f"][4] == 32
    assert sorted(r * rows("i")[1] for r in rows("i")[0]) == [128, 128, 144, 144]
    assert max(taps("j")) * SHAPES["j"][4] // 32 == 64
    assert len(taps("k")) == 9 and set(taps("k")) == {1}
    # which instantiation runs is the library's answer, not a model of its plan: the small shapes all take
    # the 64 x 64 tile, and m, n, o are there for the other three
    assert {dgrad_plan(s)[:2] for s in SHAPES.values()} == {(64, 64)}
    for shape, tile in LARGE.values():
        N, H, W, Cin, _, k, stride, pad = shape
        tm, tn, grid = dgrad_plan(shape)
        assert (tm, tn) == tile
        assert grid == sum(-(-N * len(c["hs"]) * len(c["ws"]) // tm) for c in dgrad_classes(H, W, k, stride, pad)) * \
            -(-Cin // tn) >= 512
    assert len(taps("l")) == 16 and sorted(taps("l")) == [0] * 7 + [1] * 9


# ---------------------------------------------------------------- the C ABI
def _entry(L):
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    fn = L.eosv_conv_dgrad_x3
    fn.restype, fn.argtypes = i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.eosv_last_error.restype = ctypes.c_char_p
    return fn


GOOD = dict(N=2, H=9, W=6, Cin=64, Cout=128, k=3, stride=2, pad=1)


def _dgrad(fn, dy=P, wf=P, add=None, dx=P, kw=None, **over):
    d = dict(GOOD, **over)
    return fn(dy, d["N"], d["H"], d["W"], d["Cin"], wf, d["Cout"], d["k"], d["k"] if kw is None else kw, d["stride"],
              d["pad"], add, dx, None)


def test_library_binding_and_header_declare_the_entry_point():
    import os
    import re

    L = _library()
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eosv.h")
    with open(header) as fh:
        text = fh.read()
    assert hasattr(L, "eosv_conv_dgrad_x3") and "eosv_conv_dgrad_x3" in _lib.EXPORTS
    assert hasattr(L, "eosv_conv_dgrad_x3_plan") and "eosv_conv_dgrad_x3_plan" in _lib.EXPORTS
    assert re.search(r"\bint\s+eosv_conv_dgrad_x3_plan\s*\(", text)
    m = re.search(r"/\*(?:(?!\*/).)*\*/\s*int\s+eosv_conv_dgrad_x3\s*\(", text, re.S)
    assert m, "eosv_conv_dgrad_x3 is not declared in include/eosv.h"
    assert "loss.backward()" in m.group(0) and "network_train.py:114" in m.group(0)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    B = _lib.lib()
    assert B.eosv_conv_dgrad_x3.restype is i32
    assert B.eosv_conv_dgrad_x3.argtypes == [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    assert B.eosv_conv_dgrad_x3_plan.argtypes == [i32] * 9 + [ctypes.POINTER(i32)] * 2 + [ctypes.POINTER(ctypes.c_int64)]


BAD_SIZES = [dict(N=-1), dict(H=0), dict(W=-3), dict(Cin=0), dict(Cout=0), dict(k=0), dict(stride=0), dict(stride=-2),
             dict(pad=-1),
             dict(H=1, W=6, k=5, pad=1),    # an empty output map: 1 + 2 - 5 < 0
             dict(H=9, W=2, k=3, pad=0)]


def test_bad_arguments_are_rejected_before_any_device_call():
    L = _library()
    fn = _entry(L)
    for kw in [dict(dy=None), dict(wf=None), dict(dx=None)] + BAD_SIZES:
        assert _dgrad(fn, **kw) == ARG, kw
        assert b"eosv_conv_dgrad_x3" in L.eosv_last_error(), kw
    assert _dgrad(fn, kw=0) == ARG
    # a bad argument is reported as such even where the shape would be refused too
    assert _dgrad(fn, dx=None, Cout=48, stride=1) == ARG


def test_unsupported_shapes_and_pointers_name_the_operand():
    L = _library()
    fn = _entry(L)
    mis = P + 4
    for kw, word in [(dict(Cout=48), b"Cout"), (dict(Cout=16), b"Cout"), (dict(Cin=96), b"Cin"), (dict(Cin=32), b"Cin"),
                     (dict(stride=1), b"stride"), (dict(stride=5), b"stride"),
                     (dict(dy=mis), b"d_dy"), (dict(wf=mis), b"d_wf"), (dict(add=mis), b"d_add"), (dict(dx=mis), b"d_dx"),
                     (dict(N=1 << 20, H=1 << 13, W=1 << 13), b"grid"), (dict(N=1, H=1 << 16, W=1 << 16), b"grid")]:
        assert _dgrad(fn, **kw) == UNSUPPORTED, kw
        assert b"eosv_conv_dgrad_x3" in L.eosv_last_error() and word in L.eosv_last_error(), (kw, L.eosv_last_error())
    # Cout needs 32 only (the reduction), not the forward's 64
    assert _dgrad(fn, Cout=32, dy=mis) == UNSUPPORTED and b"d_dy" in L.eosv_last_error()


def test_the_plan_query_returns_the_entrys_status_for_the_sizes():
    good = tuple(GOOD[k] for k in ("N", "H", "W", "Cin", "Cout", "k", "stride", "pad"))
    assert dgrad_plan(good) == (64, 64, 4)   # classes of 24 / 24 / 30 / 30 rows: one row tile each
    assert dgrad_plan((0,) + good[1:]) == (64, 64, 0)
    for i, bad in ((0, -1), (1, 0), (5, 0), (6, 0), (7, -1)):
        assert dgrad_plan(good[:i] + (bad,) + good[i + 1:], expect=ARG)[0] == -1   # outputs untouched
    for i, bad in ((4, 48), (3, 96), (6, 1), (6, 5)):
        assert dgrad_plan(good[:i] + (bad,) + good[i + 1:], expect=UNSUPPORTED)[0] == -1
        assert b"eosv_conv_dgrad_x3_plan" in _lib_error()
    fn = _library().eosv_conv_dgrad_x3_plan
    fn.argtypes = [ctypes.c_int] * 9 + [ctypes.c_void_p] * 3
    assert fn(*good[:5], good[5], *good[5:], None, None, None) == ARG


def _lib_error():
    L = _library()
    L.eosv_last_error.restype = ctypes.c_char_p
    return L.eosv_last_error()


def test_an_empty_batch_is_nothing_to_do():
    L = _library()
    fn = _entry(L)
    assert _dgrad(fn, N=0) == 0
    assert _dgrad(fn, N=0, Cin=96, dy=P + 4, stride=1) == 0   # nothing would be read or written


# ---------------------------------------------------------------- the trainer's keyword and plans
def _strided(arch_name, mask):
    """The names of the convs f32x3_dgrad takes: of the enabled stages 2-4, the 3x3 stride-2 conv and the
    stride-2 shortcut of the stage's first block."""
    which = "conv1" if arch_name == "resnet18" else "conv2"
    return sorted(f"convnet.{4 + li}.0.{n}" for li in (1, 2, 3) if mask >> li & 1 for n in (which, "downsample.0"))


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
@pytest.mark.parametrize("switches", [NONE, ALL, PART], ids=["none", "all", "part"])
def test_plans_with_the_switch_off_and_on(monkeypatch, arch, switches):
    train = _stub_device(monkeypatch)
    for off in (dict(), dict(f32x3_dgrad=False), dict(f32x3_dgrad=0), dict(f32x3_dgrad=None)):
        tr = train.NativeTrainer(arch, 4, **switches, **off)
        assert tr.x3d_mask == 0 and tr.x3d_launches == 0
        for c in tr._convs():
            assert c.x3d is False and c.routes == _expected(c, **switches), c.name
    # bit 0 selects nothing: layer 1 has no strided conv
    assert [c.routes for c in train.NativeTrainer(arch, 4, **switches, f32x3_dgrad=1)._convs()] == \
        [c.routes for c in train.NativeTrainer(arch, 4, **switches)._convs()]
    for mask in (15, 14, 6):
        for x3c in (0, 15):   # independent of f32x3_convs, which leaves these gradients on `gemm`
            tr = train.NativeTrainer(arch, 4, **switches, f32x3_dgrad=mask, f32x3_convs=x3c)
            assert tr.x3d_mask == mask
            names = _strided(arch, mask)
            assert len(names) == {15: 6, 14: 6, 6: 4}[mask]
            assert sorted(c.name for c in tr._convs() if c.x3d) == names
            for c in tr._convs():
                want = _expected_x3c(c, x3c, **switches)[0]
                if c.name in names:
                    assert (c.stride, c.cout % 32, c.cin % 64) == (2, 0, 0)
                    assert want["dgrad"] == ("gemm",)
                    want = dict(want, dgrad=("x3d", "gemm"))
                assert c.routes == want, (c.name, c.routes, want)
            assert not tr.stem.x3d


def test_stage_mask_parses_f32x3_dgrad(monkeypatch):
    train = _stub_device(monkeypatch)
    assert 0 <= train.TRAIN_X3D_DEFAULT <= 15
    assert train.NativeTrainer("resnet18", 4, f32x3_dgrad=True).x3d_mask == train.TRAIN_X3D_DEFAULT
    assert train.NativeTrainer("resnet18", 4, f32x3_dgrad=np.int64(9)).x3d_mask == 9
    for bad in (16, -1, 1.0, "15"):
        with pytest.raises(ValueError, match="f32x3_dgrad"):
            train.NativeTrainer("resnet18", 4, f32x3_dgrad=bad)
    # independent of the other switches
    tr = train.NativeTrainer("resnet50", 4, f32x3_dgrad=12, f32x3_convs=3, winograd=4, winograd_wgrad=8, f32x3=2,
                             stem_direct=True, fused_bn_stats=1)
    assert (tr.x3d_mask, tr.x3c_mask, tr.wino_mask, tr.wino_wgrad_mask, tr.x3_mask, tr.stem_direct, tr.bnstats_mask) == \
        (12, 3, 4, 8, 2, True, 1)


COUNTERS = ("stem_direct_launches", "wino_launches", "wino_wgrad_launches", "x3_launches", "x3c_launches", "x3d_launches")


def _counts(tr):
    return {k: getattr(tr, k) for k in COUNTERS}


@pytest.mark.parametrize("statuses,winner,counter", [
    ({"x3d": 0, "gemm": 0}, "x3d", "x3d_launches"),
    ({"x3d": UNSUPPORTED, "gemm": 0}, "gemm", None),
])
def test_x3d_route_in_the_dispatcher(monkeypatch, statuses, winner, counter):
    tr, c, asked = _fake_trainer(monkeypatch, "dgrad", statuses)
    tr.x3d_launches = 3   # counted from where it stands
    before = _counts(tr)
    tr._run("dgrad", c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(winner) + 1]
    want = dict(before)
    if counter:
        want[counter] += 1
    assert _counts(tr) == want


@pytest.mark.parametrize("statuses,culprit", [
    ({"x3d": ARG, "gemm": 0}, "x3d"),                        # a failure is no refusal
    ({"x3d": -2, "gemm": 0}, "x3d"),
    ({"x3d": UNSUPPORTED, "gemm": UNSUPPORTED}, "gemm"),     # the last route's refusal raises
])
def test_x3d_failures_raise_under_the_library_functions_name(monkeypatch, statuses, culprit):
    tr, c, asked = _fake_trainer(monkeypatch, "dgrad", statuses)
    before = _counts(tr)
    with pytest.raises(_lib.EosvError, match=f"eosv_fake_{culprit} failed"):
        tr._run("dgrad", c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(culprit) + 1]
    assert _counts(tr) == before


def test_x3d_route_calls_the_library_with_the_convs_geometry(monkeypatch):
    """The route over a recording library: it flips the weights into the `wflip` scratch and hands the kernel
    the conv's input shape, the flipped copy and the residual gradient as the addend."""
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer("resnet18", 4, f32x3_dgrad=2)
    c = next(c for c in tr._convs() if c.name == "convnet.5.0.conv1")
    calls = []

    def rec(name, rc=0):
        def fn(*a):
            calls.append((name, a))
            return rc
        return fn

    tr.L = types.SimpleNamespace(eosv_conv_dgrad_x3=rec("dgrad", UNSUPPORTED), eosv_flip_weights=rec("flip"))
    buf = types.SimpleNamespace(data_ptr=lambda: 64)
    monkeypatch.setattr(tr, "_buf", lambda key, n: calls.append(("buf", key, n)) or buf)
    t = lambda p: types.SimpleNamespace(data_ptr=lambda: p)   # noqa: E731
    c.w = t(1600)
    shape = (2, 24, 23, c.cin)
    assert tr._dgrad_x3d(c, None, shape, 2 * 12 * 12, t(48), t(80), t(96), 7) == (UNSUPPORTED, "eosv_conv_dgrad_x3")
    assert calls == [("buf", "wflip", 128 * 9 * 64), ("flip", (1600, 128, 3, 3, 64, 64, 7)),
                     ("dgrad", (48, 2, 24, 23, 64, 64, 128, 3, 3, 2, 1, 96, 80, 7))]
    del calls[:]
    assert tr._dgrad_x3d(c, None, shape, 2 * 12 * 12, t(48), t(80), None, 7)[1] == "eosv_conv_dgrad_x3"
    assert not calls[-1][1][11] and calls[-1][1][:11] == (48, 2, 24, 23, 64, 64, 128, 3, 3, 2, 1)   # no addend: NULL


def test_train_network_passes_train_f32x3_dgrad_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_f32x3_dgrad defaults to False and is read at finetune_model time; False passes no
    keyword at all."""
    import network_train

    assert network_train.TrainNetwork.train_f32x3_dgrad is False
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
    for value in (False, True, 14):
        tn = object.__new__(network_train.TrainNetwork)
        tn.__dict__.update(loss_path=str(tmp_path / "loss.txt"), ckp_path=str(tmp_path) + "/", epoch_nums=0,
                           batch_size=2, lr_1=1e-4, lr_2=1e-3, lr_step_size=10, resnet_model="resnet50",
                           num_classes=64, mymodel=model)
        if value is not False:
            tn.train_f32x3_dgrad = value
        tn.finetune_model()
    assert seen == [{}, {"f32x3_dgrad": True}, {"f32x3_dgrad": 14}]
