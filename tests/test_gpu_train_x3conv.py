"""GPU: the opt-in f32x3 implicit GEMMs of the training step's 3x3 and strided convs
(csrc/conv_x3.hip: eosv_conv2d_x3, eosv_conv_wgrad_x3) and NativeTrainer(f32x3_convs=mask).

Conventions of tests/test_gpu_train_x3.py, by import: inputs between NaN guards, outputs and
workspaces between sentinel guards, every launch twice with equal bytes.  The references are
torch.nn.functional.conv2d in f64 on the CPU (and its autograd for the two gradients) and a numpy
im2col (A = col(X) [P][K], K = (kh, kw, c)) fed to x3_terms: the split commutes with the gather,
because padding zeros split to zeros.

Shapes are (N, H, W, Cin, Cout, k, stride, pad); no map is square.
  a (2, 5, 7, 32, 64, 3, 1, 1)     P = 70: a ragged second row tile, a frame boundary inside a tile, one k-step per tap
  b (3, 9, 6, 64, 128, 3, 2, 1)    odd H at stride 2, a 5 x 3 output, padding hit on the top and left only
  c (2, 7, 5, 128, 256, 1, 2, 0)   the stride-2 shortcut: odd H and W, a 4 x 3 output
  d (1, 12, 11, 96, 64, 3, 1, 1)   P = 132 crosses 128; 3 k-steps per tap; wgrad K = 864, taps straddle a 128-column tile
  e (2, 17, 16, 64, 64, 3, 1, 1)   P = 544: wgrad splits into two slices, the last ragged
  f (1, 3, 2, 512, 512, 3, 1, 1)   the stage-4 map of a small frame: every output has padding taps; K = 4608
  g (8, 91, 90, 32, 128, 3, 1, 1)  P = 65520 = 512 row tiles of 128: the forward keeps the unhalved 128 x 128 tile
                                   under the fixed 256-CU plan (forward only)
  h (4, 64, 64, 32, 256, 3, 1, 1)  P = 16384: 128 x 128 would be 256 tiles, so m halves: the forward's 64 x 128 tile,
                                   512 of them (forward only)
  i (8, 91, 90, 32, 64, 3, 1, 1)   shape g with Cout 64: 512 row tiles of the forward's 128 x 64 tile (forward only)
  j (2, 7, 5, 64, 128, 1, 2, 0)    shape c with half the channels: Cout 128 and K = 64, the weight gradient's 128 x 64 tile
The input gradient through eosv_conv2d_x3 (dY as the input, flipped weights, stride 1) exists where the
conv's Cout % 32 == 0 and Cin % 64 == 0: shapes e and f.

Exactness: integer operands; every partial sum is an integer of magnitude at most
T max|a| max|b| < 2^24 (T the terms of an output), so f32 accumulation is exact in any order.
Largest err / bound seen on an MI355X: see DESIGN 3T.
"""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _expected_wino_launches, _oracle, _same_bytes, _small_case
from test_cpu_train_x3 import x3_terms
from test_cpu_train_x3conv import conv_dims, flip_weights, im2col
from test_gpu_train_x3 import SENTINEL, UNSUPPORTED, _check_random, _dev_in, _dev_out, _read_out

pytestmark = pytest.mark.gpu

SHAPES = {"a": (2, 5, 7, 32, 64, 3, 1, 1), "b": (3, 9, 6, 64, 128, 3, 2, 1), "c": (2, 7, 5, 128, 256, 1, 2, 0),
          "d": (1, 12, 11, 96, 64, 3, 1, 1), "e": (2, 17, 16, 64, 64, 3, 1, 1), "f": (1, 3, 2, 512, 512, 3, 1, 1),
          "g": (8, 91, 90, 32, 128, 3, 1, 1), "h": (4, 64, 64, 32, 256, 3, 1, 1), "i": (8, 91, 90, 32, 64, 3, 1, 1),
          "j": (2, 7, 5, 64, 128, 1, 2, 0)}
SMALL = "abcdefj"
LARGE = "ghi"   # forward only, and once
DGRAD = "ef"


# ---------------------------------------------------------------- launches
def _conv(x, w, stride, pad, add=None, expect_ok=True, off=None):
    """One eosv_conv2d_x3 launch: x [N][H][W][Cin], w [Cout][k][k][Cin] -> (rc, y [P][Cout]).
    off: the operand ("x", "w", "add", "y") whose pointer is moved 4 bytes on."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    N, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    P = conv_dims(N, H, W, k, stride, pad)[2]
    xb, xp = _dev_in(x)
    wb, wp = _dev_in(w)
    ab, ap = _dev_in(add) if add is not None else (None, None)
    yb, yp = _dev_out(P * Cout)
    if off:
        xp, wp, ap, yp = (p + 4 if name == off else p for name, p in (("x", xp), ("w", wp), ("add", ap), ("y", yp)))
    rc = L.eosv_conv2d_x3(xp, N, H, W, Cin, wp, Cout, k, k, stride, pad, ap, yp, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_conv2d_x3")
    return rc, _read_out(yb, P * Cout, "Y").reshape(P, Cout)


def _wgrad(x, dy, k, stride, pad, work="full", expect_ok=True, off=None):
    """One eosv_conv_wgrad_x3 launch -> (rc, dW [Cout][K]).  work: "full" the workspace the library
    asks for, "none" no workspace, "one" one slice's worth."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    N, H, W, Cin = x.shape
    Cout, K = dy.shape[1], k * k * Cin
    wbytes = {"full": int(L.eosv_conv_wgrad_x3_workspace(N, H, W, Cin, Cout, k, k, stride, pad)), "none": 0,
              "one": Cout * K * 4}[work]
    xb, xp = _dev_in(x)
    db, dp = _dev_in(dy)
    gb, gp = _dev_out(Cout * K)
    kb, kp = _dev_out(wbytes // 4) if wbytes else (None, None)
    if off:
        xp, dp, gp, kp = (p + 4 if name == off else p for name, p in (("x", xp), ("dy", dp), ("dw", gp), ("work", kp)))
    rc = L.eosv_conv_wgrad_x3(xp, N, H, W, Cin, dp, Cout, k, k, stride, pad, gp, kp, wbytes, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_conv_wgrad_x3")
    out = _read_out(gb, Cout * K, "dW").reshape(Cout, K)
    work_out = _read_out(kb, wbytes // 4, "the workspace") if wbytes else None
    return rc, out, work_out


def _twice(fn, *args, **kw):
    a, b = fn(*args, **kw)[1], fn(*args, **kw)[1]
    assert a.tobytes() == b.tobytes(), "two launches differ"
    return a


# ---------------------------------------------------------------- f64 references
def _ref_conv(x, w, stride, pad):
    """conv2d in f64 on the CPU -> [P][Cout]."""
    y = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2),
                                   torch.from_numpy(w).double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0]).numpy()


def _ref_grads(x, w, dy, stride, pad):
    """(dX [N][H][W][Cin], dW [Cout][K]) of conv2d in f64 by autograd, for dY [P][Cout]."""
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_()
    wt = torch.from_numpy(w).double().permute(0, 3, 1, 2).requires_grad_()
    y = torch.nn.functional.conv2d(xt, wt, stride=stride, padding=pad)
    g = torch.from_numpy(dy).double().reshape(y.shape[0], y.shape[2], y.shape[3], y.shape[1]).permute(0, 3, 1, 2)
    dx, dw = torch.autograd.grad(y, (xt, wt), g)
    return dx.permute(0, 2, 3, 1).numpy(), dw.permute(0, 2, 3, 1).reshape(w.shape[0], -1).numpy()


def _ints(rng, shape, bits):
    hi = (1 << bits) - 1
    return rng.integers(-hi, hi + 1, size=shape).astype(np.float32)


def _wide_narrow(T):
    """(bits of the wide operand, bound of the narrow one) for T terms per output."""
    bits = 12 if T * 4095 < 2 ** 24 else 11
    return bits, (7 if T * ((1 << bits) - 1) * 7 < 2 ** 24 else 1)


def _exact_pair(rng, shape_a, shape_b, T, wide_a):
    bits, bmax = _wide_narrow(T)
    a = _ints(rng, shape_a, bits) if wide_a else rng.integers(-bmax, bmax + 1, size=shape_a).astype(np.float32)
    b = rng.integers(-bmax, bmax + 1, size=shape_b).astype(np.float32) if wide_a else _ints(rng, shape_b, bits)
    assert T * float(np.abs(a).max()) * float(np.abs(b).max()) < 2 ** 24
    return a, b


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("sid", list(SHAPES))
def test_exact_forward_one_wide_operand_either_role(sid):
    """The large shapes run the wide input only."""
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    rng = np.random.default_rng(ord(sid))
    for wide_x in (True,) if sid in LARGE else (True, False):
        x, w = _exact_pair(rng, (N, H, W, Cin), (Cout, k, k, Cin), k * k * Cin, wide_x)
        got = _twice(_conv, x, w, stride, pad)
        assert np.array_equal(got.astype(np.float64), _ref_conv(x, w, stride, pad)), wide_x


@pytest.mark.parametrize("sid", list(SMALL))
def test_exact_weight_gradient_one_wide_operand_either_role(sid):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    P = conv_dims(N, H, W, k, stride, pad)[2]
    rng = np.random.default_rng(100 + ord(sid))
    for wide_x in (True, False):
        x, dy = _exact_pair(rng, (N, H, W, Cin), (P, Cout), P, wide_x)
        ref = _ref_grads(x, np.zeros((Cout, k, k, Cin), np.float32), dy, stride, pad)[1]
        for work in ("full", "none", "one"):
            got = _twice(_wgrad, x, dy, k, stride, pad, work=work)
            assert np.array_equal(got.astype(np.float64), ref), (wide_x, work)


@pytest.mark.parametrize("sid", list(DGRAD))
def test_exact_input_gradient_with_and_without_the_addend(sid):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    assert stride == 1 and pad == k // 2 and Cout % 32 == 0 and Cin % 64 == 0
    rng = np.random.default_rng(200 + ord(sid))
    for wide_dy in (True, False):
        dy, w = _exact_pair(rng, (N, H, W, Cout), (Cout, k, k, Cin), k * k * Cout, wide_dy)
        ref = _ref_grads(np.zeros((N, H, W, Cin), np.float32), w, dy.reshape(-1, Cout), 1, pad)[0].reshape(-1, Cin)
        add = _ints(rng, ref.shape, 10)
        assert float(np.abs(ref).max()) + 1023 < 2 ** 24
        wf = flip_weights(w)
        assert np.array_equal(_twice(_conv, dy, wf, 1, pad).astype(np.float64), ref), wide_dy
        assert np.array_equal(_twice(_conv, dy, wf, 1, pad, add=add).astype(np.float64), ref + add), wide_dy


def test_exact_both_operands_wide_drops_only_lo_lo():
    """Both operands wider than bf16 need T (2^bits)^2 <= 2^24.  A 1x1 stride-2 conv with Cin = 32 (T = 32)
    takes 9-bit operands.  Shape a has T = 288, which leaves no room for a ninth bit, so its weights are
    non-zero in 4 of the 32 channels only: 36 non-zero terms per output, 9-bit operands again; its
    weight gradient has T = P = 70, and dY is non-zero in the first 32 pixels only."""
    rng = np.random.default_rng(9)
    bits = 9
    for N, H, W, Cin, Cout, k, stride, pad, live in ((2, 7, 5, 32, 64, 1, 2, 0, 32), SHAPES["a"] + (4,)):
        assert k * k * live * (2 ** bits) ** 2 <= 2 ** 24
        x, w = _ints(rng, (N, H, W, Cin), bits), _ints(rng, (Cout, k, k, Cin), bits)
        w[..., live:] = 0
        A, B = im2col(x, k, stride, pad), np.ascontiguousarray(w.reshape(Cout, -1).T)
        model, full = x3_terms(A, B), A.astype(np.float64) @ B.astype(np.float64)
        assert not np.array_equal(model, full), "the case has no lo * lo term to drop"
        assert np.array_equal(_twice(_conv, x, w, stride, pad).astype(np.float64), model)
        P = A.shape[0]
        dy = _ints(rng, (P, Cout), bits)
        dy[32:] = 0
        assert 32 * (2 ** bits) ** 2 <= 2 ** 24
        At = np.ascontiguousarray(dy.T)
        model, full = x3_terms(At, A), At.astype(np.float64) @ A.astype(np.float64)
        assert not np.array_equal(model, full)
        for work in ("full", "none"):
            assert np.array_equal(_twice(_wgrad, x, dy, k, stride, pad, work=work).astype(np.float64), model), work


# ---------------------------------------------------------------- 2. random
@pytest.mark.parametrize("sid,scale", [(sid, sc) for sid in SMALL for sc in ((1.0, 1.0), (1e3, 1e-3))] +
                         [(sid, (1.0, 1.0)) for sid in LARGE],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]:g}")
def test_random_operands_against_the_model_and_f64(sid, scale):
    """The large shapes (g, h, i: the NT shapes of the 128 x 128, 64 x 128 and 128 x 64 tiles) run their forward only,
    and once."""
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    rng = np.random.default_rng(300 + ord(sid))
    x = (rng.standard_normal((N, H, W, Cin)) * scale[0]).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) * scale[1]).astype(np.float32)
    A, B = im2col(x, k, stride, pad), np.ascontiguousarray(w.reshape(Cout, -1).T)
    P = A.shape[0]
    tag = f"{sid} {SHAPES[sid]} x {scale[0]:g} / {scale[1]:g}"
    _check_random(tag + " forward", _twice(_conv, x, w, stride, pad), A, B)
    if sid in LARGE:
        return
    dy = (rng.standard_normal((P, Cout)) * scale[1]).astype(np.float32)
    At = np.ascontiguousarray(dy.T)
    for work in ("full", "none", "one"):
        _check_random(f"{tag} weight gradient, workspace: {work}", _twice(_wgrad, x, dy, k, stride, pad, work=work), At, A)
    if sid in DGRAD:
        g = (rng.standard_normal((N, H, W, Cout)) * scale[0]).astype(np.float32)
        wf = flip_weights(w)
        Ag, Bg = im2col(g, k, 1, pad), np.ascontiguousarray(wf.reshape(Cin, -1).T)
        add = rng.standard_normal((N * H * W, Cin)).astype(np.float32)
        _check_random(tag + " input gradient", _twice(_conv, g, wf, 1, pad), Ag, Bg)
        _check_random(tag + " input gradient + addend", _twice(_conv, g, wf, 1, pad, add=add), Ag, Bg,
                      extra=(add.astype(np.float64), np.abs(add)))


def test_weight_gradient_of_shape_e_splits_in_two():
    from eosv._lib import lib

    N, H, W, Cin, Cout, k, stride, pad = SHAPES["e"]
    assert int(lib().eosv_conv_wgrad_x3_workspace(N, H, W, Cin, Cout, k, k, stride, pad)) == 2 * Cout * k * k * Cin * 4
    for sid in "abcdfj":
        N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
        assert int(lib().eosv_conv_wgrad_x3_workspace(N, H, W, Cin, Cout, k, k, stride, pad)) == 0, sid


# ---------------------------------------------------------------- 3. bitwise against the GEMM
def test_1x1_stride_1_equals_the_x3_gemm_bitwise():
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    N, H, W, Cin, Cout = 2, 5, 7, 64, 256
    P = N * H * W
    rng = np.random.default_rng(3)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = rng.standard_normal((Cout, 1, 1, Cin)).astype(np.float32)
    add = rng.standard_normal((P, Cout)).astype(np.float32)
    for addend in (None, add):
        conv = _twice(_conv, x, w, 1, 0, add=addend)
        xb, xp = _dev_in(x)
        wb, wp = _dev_in(w)
        ab, ap = _dev_in(addend) if addend is not None else (None, None)
        yb, yp = _dev_out(P * Cout)
        check(L.eosv_sgemm_x3(0, 1, P, Cout, Cin, 1.0, xp, Cin, wp, Cin, 0.0, yp, Cout, ap, s), "eosv_sgemm_x3")
        torch.cuda.synchronize()
        gemm = _read_out(yb, P * Cout, "C").reshape(P, Cout)
        assert conv.tobytes() == gemm.tobytes(), "with the addend" if addend is not None else "without the addend"


# ---------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("what", ["Cin 48", "Cout 72", "x", "w", "add", "y"])
def test_refused_forward_writes_nothing(what):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES["a"]
    Cin, Cout = (48 if what == "Cin 48" else Cin), (72 if what == "Cout 72" else Cout)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = rng.standard_normal((Cout, k, k, Cin)).astype(np.float32)
    add = rng.standard_normal((N * H * W, Cout)).astype(np.float32)
    rc, y = _conv(x, w, stride, pad, add=add, expect_ok=False, off=what if len(what) < 4 else None)
    assert rc == UNSUPPORTED, rc
    assert bool((y == SENTINEL).all()), "a refused call wrote"


@pytest.mark.parametrize("what", ["Cin 48", "Cout 72", "x", "dy", "dw", "work"])
def test_refused_weight_gradient_writes_nothing(what):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES["e"]
    Cin, Cout = (48 if what == "Cin 48" else Cin), (72 if what == "Cout 72" else Cout)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    dy = rng.standard_normal((N * H * W, Cout)).astype(np.float32)
    # a refused shape asks for no workspace: the call still gets one slice's worth, which must stay untouched
    rc, dw, work = _wgrad(x, dy, k, stride, pad, work="one" if "C" in what else "full", expect_ok=False,
                          off=what if "C" not in what else None)
    assert rc == UNSUPPORTED, rc
    assert bool((dw == SENTINEL).all()) and bool((work == SENTINEL).all()), "a refused call wrote"


# ---------------------------------------------------------------- the trainer
def _eligible(name, mask=15):
    """[(conv name, layer index, stride)] of the convs f32x3_convs takes, from arch.SPECS: of the enabled
    stages, every 3x3 conv (cin % 32 == 0 for all of them) and the stride-2 1x1 downsample."""
    spec = arch.SPECS[name]
    out = []
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), spec.layers)):
        for bi in range(blocks):
            stride = 2 if (li > 0 and bi == 0) else 1
            cout = planes * spec.expansion
            p = f"convnet.{4 + li}.{bi}"
            if mask >> li & 1:
                assert inplanes % 32 == 0 and planes % 32 == 0
                if spec.block == "basic":
                    out += [(p + ".conv1", li, stride), (p + ".conv2", li, 1)]
                else:
                    out.append((p + ".conv2", li, stride))
                if bi == 0 and stride != 1:
                    out.append((p + ".downsample.0", li, stride))
            inplanes = cout
    return out


def _launches(name, mask=15):
    """Forward + weight gradient of every eligible conv, the input gradient of the stride-1 ones."""
    el = _eligible(name, mask)
    return 2 * len(el) + sum(1 for _, _, stride in el if stride == 1)


def test_eligible_conv_counts():
    for name in ("resnet18", "resnet50"):
        assert len(_eligible(name)) == 19 and _launches(name) == 19 + 19 + 13 == 51
        for mask in (15, 1, 6):
            tr = NativeTrainer(name, 64, device=0, f32x3_convs=mask)
            assert sorted(c.name for c in tr._convs() if c.x3c) == sorted(n for n, _, _ in _eligible(name, mask))
    assert _launches("resnet18", 1) == 12


@functools.lru_cache(maxsize=None)
def _wired_trainer(name, mask):
    tr = NativeTrainer(name, 64, device=0, f32x3_convs=mask)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    return tr


MAPS = [(24, 23), (12, 12), (6, 6), (3, 3)]   # the stages' maps of a 96 x 90 frame
WIRED = ([("resnet18", f"convnet.{4 + li}.1.conv1", li) for li in range(4)] +
         [("resnet18", "convnet.5.0.conv1", 1), ("resnet18", "convnet.5.0.downsample.0", 1)] +
         [("resnet50", f"convnet.{4 + li}.1.conv2", li) for li in range(4)] +
         [("resnet50", "convnet.6.0.conv2", 2), ("resnet50", "convnet.6.0.downsample.0", 2)])


@pytest.mark.parametrize("name,conv,li", WIRED)
def test_trainer_conv_calls_take_the_x3_kernels(name, conv, li):
    from eosv._lib import stream_ptr

    N = 2
    got = {}
    for mask in (15, False):
        tr = _wired_trainer(name, mask)
        c = next(c for c in tr._convs() if c.name == conv)
        assert c.x3c is (mask == 15)
        H, W = MAPS[li] if c.stride == 1 else MAPS[li - 1]
        shape = (N, H, W, c.cin)
        _, Ho, Wo, _ = c.out_shape(shape)
        P = N * Ho * Wo
        g = torch.Generator().manual_seed(H * 1000 + c.cin + c.k)
        x, dz, acc = torch.randn(*shape, generator=g), torch.randn(P, c.cout, generator=g), torch.randn(*shape, generator=g)
        s = stream_ptr()
        xd, dzd, accd = (t.cuda().reshape(-1) for t in (x, dz, acc))
        tr.x3c_launches = 0
        y, oshape = tr._conv_fwd(xd, shape, c, s)
        assert oshape == (N, Ho, Wo, c.cout)
        assert tr.x3c_launches == (1 if mask == 15 else 0)
        tr.x3c_launches = 0
        dx = tr._conv_bwd(dzd, xd, shape, c, s, need_dx=True, acc=accd)
        assert tr.x3c_launches == ((2 if c.stride == 1 else 1) if mask == 15 else 0)
        torch.cuda.synchronize()
        got[mask] = (y.cpu().numpy().reshape(P, c.cout), c.g.cpu().numpy().reshape(c.cout, c.K),
                     dx.cpu().numpy().reshape(-1, c.cin))
        w = c.w.cpu().numpy().reshape(c.cout, c.k, c.k, c.cin)
    y, gw, dx = got[15]
    A = im2col(x.numpy(), c.k, c.stride, c.pad)
    _check_random(f"{conv} forward", y, A, np.ascontiguousarray(w.reshape(c.cout, -1).T))
    _check_random(f"{conv} weight gradient", gw, np.ascontiguousarray(dz.numpy().T), A)
    accn = acc.numpy().reshape(-1, c.cin)
    if c.stride == 1:
        Ag = im2col(dz.numpy().reshape(N, Ho, Wo, c.cout), c.k, 1, c.pad)
        _check_random(f"{conv} input gradient + acc", dx, Ag, np.ascontiguousarray(flip_weights(w).reshape(c.cin, -1).T),
                      extra=(accn.astype(np.float64), np.abs(accn)))
    # the f32 path computes the same conv in another arithmetic: the x3c path really was taken
    for a, b, what in zip(got[15], got[False], ("y", "dW", "dx")):
        if what == "dx" and c.stride != 1:
            assert a.tobytes() == b.tobytes(), "the stride-2 input gradient stays on the f32 GEMM"
        else:
            assert a.tobytes() != b.tobytes(), what
        assert np.allclose(a, b, rtol=1e-2, atol=1e-2), what


@functools.lru_cache(maxsize=None)
def _one_step(name, f32x3_convs, fresh=0, **kw):
    """(loss, grads, x3c_launches, trainer) of one step of a fresh trainer on the small case; "default"
    builds the trainer without the keyword; `fresh` only separates cache entries."""
    frames, labels, T = _small_case()
    if f32x3_convs != "default":
        kw["f32x3_convs"] = f32x3_convs
    tr = NativeTrainer(name, 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr.x3c_launches, tr


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_launch_counts_follow_the_architecture(name):
    assert _one_step(name, 15)[2] == _launches(name) == 51
    if name == "resnet18":
        assert _one_step(name, 1)[2] == _launches(name, 1) == 12


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_default_step_untouched_by_the_keyword(name):
    a, b, z = _one_step(name, "default"), _one_step(name, False), _one_step(name, 0)
    assert a[2] == b[2] == z[2] == 0
    _same_bytes(a, b)
    _same_bytes(a, z)
    c = _one_step(name, 15)
    assert any(c[1][k].numpy().tobytes() != a[1][k].numpy().tobytes() for k in a[1])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_x3c_step_is_deterministic(name):
    a, b = _one_step(name, 15), _one_step(name, 15, fresh=1)
    assert a[2] == b[2] == 51
    _same_bytes(a, b)


def test_stacked_on_the_winograd_switches():
    """ResNet-18 with both Winograd switches on every stage and f32x3_convs on stages 1 and 3: x3c takes
    its stages' convs (the doubly eligible ones too), Winograd the stride-1 3x3 convs of stages 2 and 4."""
    loss, _, x3c, tr = _one_step("resnet18", 5, winograd=15, winograd_wgrad=15)
    assert x3c == _launches("resnet18", 5) == 12 + 13
    assert tr.wino_launches == _expected_wino_launches("resnet18", 10)
    assert tr.wino_wgrad_launches == _expected_wino_launches("resnet18", 10) // 2
    plain = _one_step("resnet18", "default")[0]
    assert abs(loss - plain) <= 1e-3 * abs(plain), (loss, plain)


@pytest.mark.parametrize("name,scaled,kw,need", [
    ("resnet18", ".bn2.weight", dict(f32x3_convs=15), dict(checked=55, x3c=16, x3=0)),
    ("resnet50", ".bn3.weight", dict(f32x3=15, f32x3_convs=15), dict(checked=70, x3c=8, x3=12))])
def test_two_steps_against_the_f64_replay(name, scaled, kw, need):
    """The form of test_gpu_train_x3.py's test: the synthetic net with every `scaled` tensor times 0.05,
    where torch's own f32 replay stays within 1e-4 (relative gradient norm) of f64 for most tensors.
    Per tensor yard = |g_f32 - g_f64| / |g_f64| from torch; every tensor with yard <= 1e-4 must have
    |g - g_f64| / |g_f64| <= max(1024 yard, 2e-2), both losses within max(1e-4, 1024 yard_loss), and at
    least `need` tensors, x3c weights and f32x3 weights must be checked."""
    from test_gpu_train_x3 import _eligible as _eligible_x3

    lr1, lr2 = 1e-3, 1e-2
    sd = dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    for k in sd:
        if k.endswith(scaled):
            sd[k] = (np.asarray(sd[k]) * np.float32(0.05)).astype(np.float32)
    frames, labels, T = _small_case()
    ref_losses, ref_g, _ = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float64)
    f32_losses, f32_g, _ = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float32)

    tr = NativeTrainer(name, 64, device=0, **kw)
    tr.load_state_dict(sd)
    l0, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    g0 = tr.grads()
    l1, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.x3c_launches == 51
    for got, ref, f32 in ((l0, ref_losses[0], f32_losses[0]), (l1, ref_losses[1], f32_losses[1])):
        yard = abs(f32 - ref) / abs(ref)
        err = abs(got - ref) / abs(ref)
        print(f"[x3c two steps {name}] loss {got:.7f} / f64 {ref:.7f}: relative error {err:.2e}, torch-f32 yardstick "
              f"{yard:.2e}")
        assert err <= max(1e-4, 1024 * yard), (got, ref, yard)
    x3c_weights = {n + ".weight" for n, _, _ in _eligible(name)}
    x3_weights = {n + ".weight" for n, _ in _eligible_x3(name)} if "f32x3" in kw else set()
    assert x3c_weights | x3_weights <= set(ref_g) and len(x3c_weights) == 19
    worst, ratio = (0.0, None, 0.0), (0.0, None)
    checked, checked_x3c, checked_x3, left_out = 0, 0, 0, []
    for k, gr in ref_g.items():
        norm = max(float(gr.norm()), 1e-12)
        yard = float((f32_g[k] - gr).norm()) / norm
        if yard > 1e-4:
            left_out.append(k)
            continue
        err = float((g0[k].double() - gr).norm()) / norm
        bound = max(1024 * yard, 2e-2)
        checked += 1
        checked_x3c += k in x3c_weights
        checked_x3 += k in x3_weights
        if err > worst[0]:
            worst = (err, k, yard)
        if err / bound > ratio[0]:
            ratio = (err / bound, k)
        assert err <= bound, (k, err, yard)
    print(f"[x3c two steps {name}] {checked} tensors checked ({checked_x3c} of the 19 x3c weights, {checked_x3} of the "
          f"{len(x3_weights)} f32x3 weights); worst relative gradient error {worst[0]:.2e} at {worst[1]} (yardstick "
          f"{worst[2]:.2e}); largest error / bound {ratio[0]:.3f} at {ratio[1]}; left out (yardstick > 1e-4): "
          f"{len(left_out)}: {', '.join(left_out)}")
    assert checked >= need["checked"] and checked_x3c >= need["x3c"] and checked_x3 >= need["x3"], \
        (checked, checked_x3c, checked_x3)
