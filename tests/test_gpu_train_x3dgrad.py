"""GPU: the opt-in f32x3 implicit GEMM of the strided convs' input gradient (csrc/conv_dgrad_x3.hip:
eosv_conv_dgrad_x3) and NativeTrainer(f32x3_dgrad=mask).

Conventions of tests/test_gpu_train_x3.py, by import: inputs between NaN guards, dX between sentinel guards
and itself all sentinel before the launch (the kernel must write every pixel exactly once), every launch
twice with equal bytes.  The references are conv2d's f64 autograd on the CPU and the numpy parity-class
gather of tests/test_cpu_train_x3dgrad.py (A = the gathered dY [N H W][k k Cout], B = W as [k k Cout][Cin])
fed to x3_terms.

Shapes are (N, H, W, Cin, Cout, k, stride, pad), H, W, Cin the conv's input.
  a (3, 9, 6, 64, 128, 3, 2, 1)     unequal classes: 12 / 12 / 15 / 15 pixels per frame
  b (2, 7, 5, 128, 256, 1, 2, 0)    the stride-2 shortcut: 23 of a frame's 35 pixels in classes without a tap
  c (2, 8, 6, 64, 64, 3, 2, 1)      an even map
  d (1, 3, 2, 64, 64, 3, 2, 1), e (1, 2, 2, 64, 64, 3, 2, 1)   classes of one pixel
  f (1, 12, 11, 64, 32, 7, 2, 3)    16 / 12 / 12 / 9 taps per class, Cout = 32: one step per tap
  g (2, 6, 9, 64, 64, 3, 2, 0)      9 pixels per frame whose taps all fall outside the map
  h (2, 5, 4, 64, 32, 2, 2, 0)      an even kernel, 4 such pixels per frame
  i (2, 17, 16, 64, 64, 3, 2, 1)    class rows 128 / 128 / 144 / 144: several row tiles in a class, a ragged last one
  j (1, 4, 4, 128, 512, 3, 2, 1)    64 k-steps in the 4-tap class
  k (2, 10, 7, 64, 32, 3, 3, 1), l (1, 9, 10, 64, 32, 3, 4, 1)   strides 3 and 4: 9 and 16 classes, 7 of l's without a tap
Under the library's fixed 256-CU plan all of these run the 64 x 64 tile.  The other three instantiations need
512 tiles of the unhalved size; one exact launch each, and eosv_conv_dgrad_x3_plan is asked which tile runs:
  m (1, 512, 512, 64, 32, 3, 2, 1)    65536 rows per class: the 128 x 64 tile
  n (1, 512, 512, 128, 32, 3, 2, 1)   the 128 x 128 tile
  o (1, 256, 256, 256, 32, 3, 2, 1)   16384 rows per class, 2 column tiles: the 64 x 128 tile

Exactness: integer operands; every partial sum is an integer of magnitude at most T max|a| max|b| < 2^24
(T = taps of the class x Cout terms), so f32 accumulation is exact in any order.
Largest err / bound seen on an MI355X: see DESIGN 3T.
"""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _same_bytes, _small_case
from test_cpu_train_x3conv import conv_dims, flip_weights
from test_cpu_train_x3dgrad import (LARGE, SHAPES, TAPLESS_DEAD, dgrad_classes, dgrad_gather, dgrad_plan,
                                    dgrad_untouched, dgrad_weights, ref_dx)
from test_gpu_train_x3 import SENTINEL, UNSUPPORTED, _check_random, _dev_in, _dev_out, _read_out
from test_gpu_train_x3conv import _exact_pair, _ints
from test_gpu_train_x3conv import test_two_steps_against_the_f64_replay as _x3c_replay
import test_gpu_train_x3conv as _x3c_tests

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- launches
def _dgrad(dy, w, H, W, stride, pad, add=None, expect_ok=True, off=None):
    """One eosv_conv_dgrad_x3 launch: dy [N][Ho][Wo][Cout], w [Cout][k][k][Cin] (flipped here, on the host) ->
    (rc, dX [N H W][Cin]).  off: the operand ("dy", "wf", "add", "dx") whose pointer is moved 4 bytes on."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    N, Cout = dy.shape[0], dy.shape[3]
    k, Cin = w.shape[1], w.shape[3]
    db, dp = _dev_in(dy)
    wb, wp = _dev_in(flip_weights(w))
    ab, ap = _dev_in(add) if add is not None else (None, None)
    xb, xp = _dev_out(N * H * W * Cin)
    if off:
        dp, wp, ap, xp = (p + 4 if name == off else p for name, p in (("dy", dp), ("wf", wp), ("add", ap), ("dx", xp)))
    rc = L.eosv_conv_dgrad_x3(dp, N, H, W, Cin, wp, Cout, k, k, stride, pad, ap, xp, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_conv_dgrad_x3")
    return rc, _read_out(xb, N * H * W * Cin, "dX").reshape(N * H * W, Cin)


def _twice(fn, *args, **kw):
    a, b = fn(*args, **kw)[1], fn(*args, **kw)[1]
    assert a.tobytes() == b.tobytes(), "two launches differ"
    return a


def _terms(H, W, Cout, k, stride, pad):
    """The most terms an output sums: the taps of the largest class x Cout."""
    return max(len(c["khs"]) * len(c["kws"]) for c in dgrad_classes(H, W, k, stride, pad)) * Cout


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("sid", list(SHAPES))
def test_exact_one_wide_operand_either_role_with_and_without_the_addend(sid):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    Ho, Wo, _ = conv_dims(N, H, W, k, stride, pad)
    tapless, dead = dgrad_untouched(N, H, W, k, stride, pad)
    if sid in TAPLESS_DEAD:   # a changed shape must not silently stop covering them
        assert (int(tapless.sum()) // N, int(dead.sum()) // N) == TAPLESS_DEAD[sid]
    none = tapless | dead
    rng = np.random.default_rng(ord(sid))
    for wide_dy in (True, False):
        dy, w = _exact_pair(rng, (N, Ho, Wo, Cout), (Cout, k, k, Cin), _terms(H, W, Cout, k, stride, pad), wide_dy)
        ref = ref_dx(w, dy, H, W, stride, pad)
        add = _ints(rng, ref.shape, 10)
        assert float(np.abs(ref).max()) + 1023 < 2 ** 24
        for addend in (None, add):
            got = _twice(_dgrad, dy, w, H, W, stride, pad, add=addend)
            assert not (got == SENTINEL).any(), "a pixel of dX was not written"
            want = ref if addend is None else ref + addend
            assert np.array_equal(got.astype(np.float64), want), (wide_dy, addend is not None)
            # the pixels no tap reaches: the addend's bytes, or +0.0
            fill = np.zeros_like(got[none]) if addend is None else addend[none]
            assert got[none].tobytes() == fill.tobytes(), (wide_dy, addend is not None)


@pytest.mark.parametrize("sid", list(LARGE))
def test_exact_on_the_larger_tiles(sid):
    """Wide dY, with the addend, once per shape; compared in f32, which holds every value exactly."""
    (N, H, W, Cin, Cout, k, stride, pad), tile = LARGE[sid]
    assert dgrad_plan(LARGE[sid][0])[:2] == tile and all(dgrad_plan(s)[:2] == (64, 64) for s in SHAPES.values())
    Ho, Wo, _ = conv_dims(N, H, W, k, stride, pad)
    rng = np.random.default_rng(ord(sid))
    dy, w = _exact_pair(rng, (N, Ho, Wo, Cout), (Cout, k, k, Cin), _terms(H, W, Cout, k, stride, pad), True)
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), torch.from_numpy(w).double().permute(0, 3, 1, 2),
                                     torch.from_numpy(dy).double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cin)
    add = _ints(rng, tuple(ref.shape), 10)
    assert float(ref.abs().max()) + 1023 < 2 ** 24
    want = (ref + torch.from_numpy(add).double()).float().numpy()
    got = _twice(_dgrad, dy, w, H, W, stride, pad, add=add)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- 2. random
@pytest.mark.parametrize("sid,scale", [(sid, sc) for sid in SHAPES for sc in ((1.0, 1.0), (1e3, 1e-3))],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]:g}")
def test_random_operands_against_the_model_and_f64(sid, scale):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES[sid]
    Ho, Wo, _ = conv_dims(N, H, W, k, stride, pad)
    rng = np.random.default_rng(300 + ord(sid))
    dy = (rng.standard_normal((N, Ho, Wo, Cout)) * scale[0]).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) * scale[1]).astype(np.float32)
    add = rng.standard_normal((N * H * W, Cin)).astype(np.float32)
    A, B = dgrad_gather(dy, H, W, k, stride, pad), dgrad_weights(w)
    tag = f"{sid} {SHAPES[sid]} dY x {scale[0]:g} / W x {scale[1]:g}"
    _check_random(tag + " input gradient", _twice(_dgrad, dy, w, H, W, stride, pad), A, B)
    _check_random(tag + " input gradient + addend", _twice(_dgrad, dy, w, H, W, stride, pad, add=add), A, B,
                  extra=(add.astype(np.float64), np.abs(add)))


# ---------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("what", ["Cout 48", "Cin 96", "stride 1", "dy", "wf", "add", "dx"])
def test_refused_call_writes_nothing(what):
    N, H, W, Cin, Cout, k, stride, pad = SHAPES["a"]
    Cout, Cin, stride = (48 if what == "Cout 48" else Cout), (96 if what == "Cin 96" else Cin), \
        (1 if what == "stride 1" else stride)
    Ho, Wo, _ = conv_dims(N, H, W, k, stride, pad)
    rng = np.random.default_rng(4)
    dy = rng.standard_normal((N, Ho, Wo, Cout)).astype(np.float32)
    w = rng.standard_normal((Cout, k, k, Cin)).astype(np.float32)
    add = rng.standard_normal((N * H * W, Cin)).astype(np.float32)
    rc, dx = _dgrad(dy, w, H, W, stride, pad, add=add, expect_ok=False, off=what if " " not in what else None)
    assert rc == UNSUPPORTED, rc
    assert bool((dx == SENTINEL).all()), "a refused call wrote"


# ---------------------------------------------------------------- the trainer
def _strided(name, mask=15):
    """[(conv name, layer index, has the shortcut's gradient as acc)] of the convs f32x3_dgrad takes, from
    arch.SPECS: of the enabled stages past the first, the 3x3 stride-2 conv and the stride-2 shortcut of the
    stage's first block.  The block's first conv is handed the shortcut's gradient: ResNet-18's conv1."""
    spec = arch.SPECS[name]
    out = []
    for li, blocks in enumerate(spec.layers):
        if li > 0 and blocks > 0 and mask >> li & 1:
            p = f"convnet.{4 + li}.0."
            out += [(p + ("conv1" if spec.block == "basic" else "conv2"), li, spec.block == "basic"),
                    (p + "downsample.0", li, False)]
    return out


def test_strided_conv_counts():
    for name in ("resnet18", "resnet50"):
        assert len(_strided(name)) == len(_strided(name, 14)) == 6 and len(_strided(name, 2)) == 2
        assert _strided(name, 1) == []
        for mask in (15, 14, 6, 1):
            tr = NativeTrainer(name, 64, device=0, f32x3_dgrad=mask)
            assert sorted(c.name for c in tr._convs() if c.x3d) == sorted(n for n, _, _ in _strided(name, mask))


@functools.lru_cache(maxsize=None)
def _wired_trainer(name, mask):
    tr = NativeTrainer(name, 64, device=0, f32x3_dgrad=mask)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    return tr


MAPS = [(24, 23), (12, 12), (6, 6), (3, 3)]   # the stages' maps of a 96 x 90 frame
WIRED = [(name,) + t for name in ("resnet18", "resnet50") for t in _strided(name)]


@pytest.mark.parametrize("name,conv,li,has_acc", WIRED, ids=[f"{w[0]}-{w[1]}" for w in WIRED])
def test_trainer_conv_bwd_takes_the_x3d_kernel(name, conv, li, has_acc):
    from eosv._lib import stream_ptr

    N = 2
    got = {}
    for mask in (14, False):
        tr = _wired_trainer(name, mask)
        c = next(c for c in tr._convs() if c.name == conv)
        assert c.x3d is (mask == 14) and c.stride == 2
        H, W = MAPS[li - 1]
        shape = (N, H, W, c.cin)
        _, Ho, Wo, _ = c.out_shape(shape)
        P = N * Ho * Wo
        g = torch.Generator().manual_seed(H * 1000 + c.cin + c.k)
        x, dz, acc = torch.randn(*shape, generator=g), torch.randn(P, c.cout, generator=g), torch.randn(*shape, generator=g)
        s = stream_ptr()
        xd, dzd = x.cuda().reshape(-1), dz.cuda().reshape(-1)
        accd = acc.cuda().reshape(-1) if has_acc else None
        tr.x3d_launches = 0
        dx = tr._conv_bwd(dzd, xd, shape, c, s, need_dx=True, acc=accd)
        assert tr.x3d_launches == (1 if mask == 14 else 0)
        torch.cuda.synchronize()
        got[mask] = (c.g.cpu().numpy().reshape(c.cout, c.K).copy(), dx.cpu().numpy().reshape(-1, c.cin))
        w = c.w.cpu().numpy().reshape(c.cout, c.k, c.k, c.cin)
    A = dgrad_gather(dz.numpy().reshape(N, Ho, Wo, c.cout), H, W, c.k, 2, c.pad)
    accn = acc.numpy().reshape(-1, c.cin)
    _check_random(f"{name} {conv} input gradient" + (" + acc" if has_acc else ""), got[14][1], A, dgrad_weights(w),
                  extra=(accn.astype(np.float64), np.abs(accn)) if has_acc else None)
    # the f32 GEMM computes the same gradient in another arithmetic: the x3d kernel really was taken
    assert got[14][1].tobytes() != got[False][1].tobytes()
    assert np.allclose(got[14][1], got[False][1], rtol=1e-2, atol=1e-2)
    assert got[14][0].tobytes() == got[False][0].tobytes(), "the weight gradient is not this switch's"


@functools.lru_cache(maxsize=None)
def _one_step(name, f32x3_dgrad, fresh=0, **kw):
    """(loss, grads, x3d_launches, trainer) of one step of a fresh trainer on the small case; "default"
    builds the trainer without the keyword; `fresh` only separates cache entries."""
    frames, labels, T = _small_case()
    if f32x3_dgrad != "default":
        kw["f32x3_dgrad"] = f32x3_dgrad
    tr = NativeTrainer(name, 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr.x3d_launches, tr


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_launch_counts_follow_the_architecture(name):
    assert _one_step(name, 15)[2] == len(_strided(name)) == 6
    assert _one_step(name, 14)[2] == len(_strided(name, 14)) == 6
    assert _one_step(name, 2)[2] == len(_strided(name, 2)) == 2
    _same_bytes(_one_step(name, 15), _one_step(name, 14))   # bit 0 selects nothing


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_default_step_untouched_by_the_keyword(name):
    a, b = _one_step(name, "default"), _one_step(name, False)
    assert a[2] == b[2] == 0
    _same_bytes(a, b)
    c = _one_step(name, 15)
    assert any(c[1][k].numpy().tobytes() != a[1][k].numpy().tobytes() for k in a[1])
    assert abs(c[0] - a[0]) <= 1e-3 * abs(a[0]), (c[0], a[0])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_x3d_step_is_deterministic(name):
    a, b = _one_step(name, 15), _one_step(name, 15, fresh=1)
    assert a[2] == b[2] == 6
    _same_bytes(a, b)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_stacked_on_f32x3_convs(name):
    """Every strided conv on x3c for its forward and weight gradient and on x3d for its input gradient: the x3c
    count is what it is without this switch."""
    loss, _, x3d, tr = _one_step(name, 15, f32x3_convs=15)
    assert x3d == 6 and tr.x3c_launches == 51
    plain = _one_step(name, "default")[0]
    assert abs(loss - plain) <= 1e-3 * abs(plain), (loss, plain)


@pytest.mark.parametrize("name,scaled,kw,need", [
    ("resnet18", ".bn2.weight", dict(f32x3_convs=15), dict(checked=55, x3c=16, x3=0)),
    ("resnet50", ".bn3.weight", dict(f32x3=15, f32x3_convs=15), dict(checked=70, x3c=8, x3=12))])
def test_two_steps_against_the_f64_replay(monkeypatch, name, scaled, kw, need):
    """The x3c tests' two-step replay, with its switch sets, tensor-count conditions and bounds as they are,
    and f32x3_dgrad=15 on top."""
    made = []

    def trainer(*a, **k):
        made.append(NativeTrainer(*a, **k))
        return made[-1]

    monkeypatch.setattr(_x3c_tests, "NativeTrainer", trainer)
    _x3c_replay(name, scaled, dict(kw, f32x3_dgrad=15), need)
    assert len(made) == 1 and made[0].x3d_mask == 15 and made[0].x3d_launches == 6
