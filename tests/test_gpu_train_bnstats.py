"""GPU: the BN batch statistics from the f32x3 forwards' epilogues (eosv_sgemm_x3_stats,
eosv_conv2d_x3_stats: the STATS instantiations of gemm_x3_kernel and conv_x3_kernel),
eosv_bn_train_forward_stats and NativeTrainer(fused_bn_stats=mask).

Conventions of tests/test_gpu_train_x3.py and tests/test_gpu_train_x3conv.py, by import: inputs between
NaN guards, outputs (the statistics buffer included) between sentinel guards, every launch twice with
equal bytes.

The statistics are part[tile][0][n] = sum of y, part[tile][1][n] = sum of y^2 over the rows of row tile
`tile` of the forward's plan, in f64, of the f32 values the launch stored.  R is the tile's height (64 or
128), chunks = ceil(rows / R) the value the _stats_chunks functions return; every case states its R and
asserts chunks, which pins the tile the plan chose.

Exactness: integer operands of magnitude <= 15, so every output is an integer of magnitude at most
T * 225 < 2^24 (T the terms of an output) and every partial sum of at most P outputs or squares stays
below P (T * 225)^2 < 2^53: f64 holds them all, whatever the order.
Random operands: the reference sums are taken in extended precision (np.longdouble) of the y the launch
wrote; a partial is R f64 additions of exactly converted values (y * y is exact in f64: 24-bit factors), so
|error| <= R 2^-53 sum|y| and R 2^-53 sum y^2.  Largest error / bound seen on an MI355X: 0.041 (printed).
"""
import collections
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _same_bytes, _small_case
from test_cpu_train_x3conv import conv_dims
from test_gpu_train_x3 import SENTINEL, UNSUPPORTED, _dev_in, _dev_out, _read_out
import test_gpu_train_x3conv as x3conv

pytestmark = pytest.mark.gpu

ARG = -1
AMAX = 15   # bound of the integer operands

# (m, n, k) -> R, the row-tile height
GEMMS = {(70, 64, 64): 64,            # 64 x 64 tile, ragged second row tile
         (40000, 128, 64): 64,        # 64 x 128
         (65530, 64, 64): 128,        # 128 x 64, last tile 122 rows
         (65530, 128, 64): 128,       # 128 x 128
         (300, 256, 128): 64}         # several column tiles: tn indexes the columns of part
# shape id of tests/test_gpu_train_x3conv.py -> R
CONVS = {"a": 64, "b": 64, "c": 64, "d": 64, "f": 64, "g": 128,   # 128 x 128
         "h": 64, "i": 128}                                      # 64 x 128, 128 x 64


def _tiles(rows, R):
    return -(-rows // R)


def _gemm_stats(a, b, stats=True, chunks=None, expect_ok=True, off=0, short=0, null=False):
    """One launch of eosv_sgemm_x3_stats (or, stats False, of eosv_sgemm_x3 NT): a [m][k], b [n][k] ->
    (rc, y [m][n], part [chunks][2][n] or None, the raw statistics floats).  off: bytes the statistics
    pointer is moved on; short: bytes taken off stats_bytes; null: no statistics pointer."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    (m, k), n = a.shape, b.shape[0]
    ab, ap = _dev_in(a)
    bb, bp = _dev_in(b)
    yb, yp = _dev_out(m * n)
    if not stats:
        rc = L.eosv_sgemm_x3(0, 1, m, n, k, 1.0, ap, k, bp, k, 0.0, yp, n, None, s)
        torch.cuda.synchronize()
        check(rc, "eosv_sgemm_x3")
        return rc, _read_out(yb, m * n, "Y").reshape(m, n), None, None
    if chunks is None:
        chunks = int(L.eosv_sgemm_x3_stats_chunks(m, n, k))
    sb, sp = _dev_out(4 * chunks * n)
    rc = L.eosv_sgemm_x3_stats(m, n, k, ap, k, bp, k, yp, n, None if null else sp + off, 16 * chunks * n - short, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_sgemm_x3_stats")
    raw = _read_out(sb, 4 * chunks * n, "the statistics")
    return rc, _read_out(yb, m * n, "Y").reshape(m, n), raw.view(np.float64).reshape(chunks, 2, n), raw


def _conv_stats(x, w, stride, pad, stats=True, chunks=None, expect_ok=True, off=0, short=0, null=False):
    """The same for eosv_conv2d_x3_stats / eosv_conv2d_x3 without an addend: x [N][H][W][Cin], w [Cout][k][k][Cin]."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    N, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    P = conv_dims(N, H, W, k, stride, pad)[2]
    xb, xp = _dev_in(x)
    wb, wp = _dev_in(w)
    yb, yp = _dev_out(P * Cout)
    if not stats:
        rc = L.eosv_conv2d_x3(xp, N, H, W, Cin, wp, Cout, k, k, stride, pad, None, yp, s)
        torch.cuda.synchronize()
        check(rc, "eosv_conv2d_x3")
        return rc, _read_out(yb, P * Cout, "Y").reshape(P, Cout), None, None
    if chunks is None:
        chunks = int(L.eosv_conv2d_x3_stats_chunks(N, H, W, Cin, Cout, k, k, stride, pad))
    sb, sp = _dev_out(4 * chunks * Cout)
    rc = L.eosv_conv2d_x3_stats(xp, N, H, W, Cin, wp, Cout, k, k, stride, pad, yp, None if null else sp + off,
                                16 * chunks * Cout - short, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_conv2d_x3_stats")
    raw = _read_out(sb, 4 * chunks * Cout, "the statistics")
    return rc, _read_out(yb, P * Cout, "Y").reshape(P, Cout), raw.view(np.float64).reshape(chunks, 2, Cout), raw


def _twice(fn, *args, **kw):
    a, b = fn(*args, **kw), fn(*args, **kw)
    assert a[1].tobytes() == b[1].tobytes(), "two launches differ in Y"
    assert a[3].tobytes() == b[3].tobytes(), "two launches differ in the statistics"
    return a


def _ref_partials(y, R, dtype):
    """[tiles][2][n] sums of y and y^2 over row tiles of R rows, summed in `dtype`."""
    rows, n = y.shape
    t = _tiles(rows, R)
    v = np.zeros((t * R, n), dtype)
    v[:rows] = y
    v = v.reshape(t, R, n)
    return np.stack([v.sum(axis=1), (v * v).sum(axis=1)], axis=1)


def _ints(rng, shape):
    return rng.integers(-AMAX, AMAX + 1, size=shape).astype(np.float32)


def _assert_exact_room(rows, T):
    ymax = T * AMAX * AMAX
    assert ymax < 2 ** 24 and rows * ymax * ymax < 2 ** 53, (rows, T)


# ---------------------------------------------------------------- 1. exact partials
@pytest.mark.parametrize("shape", list(GEMMS), ids=lambda s: "x".join(map(str, s)))
def test_exact_partials_of_the_gemm(shape):
    from eosv._lib import lib

    m, n, k = shape
    R = GEMMS[shape]
    _assert_exact_room(m, k)
    rng = np.random.default_rng(m + n + k)
    a, b = _ints(rng, (m, k)), _ints(rng, (n, k))
    chunks = int(lib().eosv_sgemm_x3_stats_chunks(m, n, k))
    assert chunks == _tiles(m, R), (chunks, R)
    _, y, part, _ = _twice(_gemm_stats, a, b)
    assert y.tobytes() == _gemm_stats(a, b, stats=False)[1].tobytes(), "Y differs from the plain entry's"
    assert np.array_equal(y.astype(np.float64), a.astype(np.float64) @ b.astype(np.float64).T)
    assert part.tobytes() == _ref_partials(y, R, np.float64).tobytes()


@pytest.mark.parametrize("sid", list(CONVS))
def test_exact_partials_of_the_conv(sid):
    from eosv._lib import lib

    N, H, W, Cin, Cout, k, stride, pad = x3conv.SHAPES[sid]
    R = CONVS[sid]
    P = conv_dims(N, H, W, k, stride, pad)[2]
    _assert_exact_room(P, k * k * Cin)
    rng = np.random.default_rng(500 + ord(sid))
    x, w = _ints(rng, (N, H, W, Cin)), _ints(rng, (Cout, k, k, Cin))
    chunks = int(lib().eosv_conv2d_x3_stats_chunks(N, H, W, Cin, Cout, k, k, stride, pad))
    assert chunks == _tiles(P, R), (chunks, R)
    _, y, part, _ = _twice(_conv_stats, x, w, stride, pad)
    assert y.tobytes() == _conv_stats(x, w, stride, pad, stats=False)[1].tobytes(), "Y differs from the plain entry's"
    if sid not in x3conv.LARGE:
        assert np.array_equal(y.astype(np.float64), x3conv._ref_conv(x, w, stride, pad))
    assert part.tobytes() == _ref_partials(y, R, np.float64).tobytes()


# ---------------------------------------------------------------- 2. random operands
def _check_partials(tag, y, part, R):
    ref = _ref_partials(y, R, np.longdouble)
    mag = _ref_partials(np.abs(y), R, np.longdouble)   # sum |y|, sum y^2
    u = np.longdouble(2.0) ** -53
    err = np.abs(part.astype(np.longdouble) - ref)
    bound = R * u * np.stack([mag[:, 0], mag[:, 1]], axis=1)
    assert not err[bound == 0].any(), tag   # a column of zeros sums to zero
    ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
    print(f"[bn stats {tag}] R = {R}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, (tag, ratio)


SCALES = ((1.0, 1.0), (1e3, 1e-3))


@pytest.mark.parametrize("scale", SCALES, ids=lambda v: f"{v[0]:g}")
@pytest.mark.parametrize("shape", list(GEMMS), ids=lambda s: "x".join(map(str, s)))
def test_random_partials_of_the_gemm(shape, scale):
    m, n, k = shape
    rng = np.random.default_rng(m + n + k + 1)
    a = (rng.standard_normal((m, k)) * scale[0]).astype(np.float32)
    b = (rng.standard_normal((n, k)) * scale[1]).astype(np.float32)
    _, y, part, _ = _twice(_gemm_stats, a, b)
    assert part.shape[0] == _tiles(m, GEMMS[shape])
    assert y.tobytes() == _gemm_stats(a, b, stats=False)[1].tobytes(), "Y differs from the plain entry's"
    _check_partials(f"gemm {shape} x {scale[0]:g} / {scale[1]:g}", y, part, GEMMS[shape])


@pytest.mark.parametrize("scale", SCALES, ids=lambda v: f"{v[0]:g}")
@pytest.mark.parametrize("sid", [s for s in CONVS if s not in x3conv.LARGE])
def test_random_partials_of_the_conv(sid, scale):
    N, H, W, Cin, Cout, k, stride, pad = x3conv.SHAPES[sid]
    rng = np.random.default_rng(600 + ord(sid))
    x = (rng.standard_normal((N, H, W, Cin)) * scale[0]).astype(np.float32)
    w = (rng.standard_normal((Cout, k, k, Cin)) * scale[1]).astype(np.float32)
    _, y, part, _ = _twice(_conv_stats, x, w, stride, pad)
    assert part.shape[0] == _tiles(y.shape[0], CONVS[sid])
    assert y.tobytes() == _conv_stats(x, w, stride, pad, stats=False)[1].tobytes(), "Y differs from the plain entry's"
    _check_partials(f"conv {sid} x {scale[0]:g} / {scale[1]:g}", y, part, CONVS[sid])


# ---------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("what,status", [("off", UNSUPPORTED), ("short", ARG), ("null", ARG)])
@pytest.mark.parametrize("entry", ["gemm", "conv"])
def test_refused_calls_write_nothing(entry, what, status):
    """A statistics pointer 8 bytes on (off 16), stats_bytes one row tile short, no statistics pointer."""
    rng = np.random.default_rng(7)
    if entry == "gemm":
        m, n, k = 70, 64, 64
        args = (_gemm_stats, rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((n, k)).astype(np.float32))
    else:
        N, H, W, Cin, Cout, k, stride, pad = x3conv.SHAPES["a"]
        n = Cout
        args = (_conv_stats, rng.standard_normal((N, H, W, Cin)).astype(np.float32),
                rng.standard_normal((Cout, k, k, Cin)).astype(np.float32), stride, pad)
    kw = {"off": dict(off=8), "short": dict(short=16 * n), "null": dict(null=True)}[what]
    rc, y, _, raw = args[0](*args[1:], expect_ok=False, **kw)
    assert rc == status, rc
    assert bool((y == SENTINEL).all()) and bool((raw == SENTINEL).all()), "a refused call wrote"


# ---------------------------------------------------------------- 4. eosv_bn_train_forward_stats
def _bn_ref(x, gamma, beta, rm, rv, res, relu):
    """nn.BatchNorm2d.train() in numpy f64 on x [P][C] -> (pre-activation, y, mean, invstd, running mean,
    running var); checked against torch.nn.functional.batch_norm where torch takes the shape (P > 1)."""
    P = x.shape[0]
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    invstd = 1.0 / np.sqrt(var + 1e-5)
    unb = var * P / (P - 1) if P > 1 else var
    pre = (x - mean) * invstd * gamma + beta + (res if res is not None else 0.0)
    nrm, nrv = 0.9 * rm + 0.1 * mean, 0.9 * rv + 0.1 * unb
    if P > 1:
        trm, trv = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
        ty = torch.nn.functional.batch_norm(torch.from_numpy(x), trm, trv, torch.from_numpy(gamma),
                                            torch.from_numpy(beta), True, 0.1, 1e-5).numpy()
        bn = (x - mean) * invstd * gamma + beta
        assert np.abs(ty - bn).max() <= 1e-12 * max(1.0, np.abs(ty).max())
        assert np.allclose(trm.numpy(), nrm, rtol=1e-12, atol=0) and np.allclose(trv.numpy(), nrv, rtol=1e-12, atol=0)
    return pre, (np.maximum(pre, 0.0) if relu else pre), mean, invstd, nrm, nrv


BN_CASES = [(37, 2048, 1), (75, 300, 3),
            (2100, 1024, 33),     # the finalize's second trip over its 32 chunk lanes
            (4704, 64, 2352),     # more chunks than the workspace's 1024: the layer-1 count, rows of two
            (1, 8, 1)]            # P = 1: the running variance takes the biased one


@pytest.mark.parametrize("relu,res,mask", [(True, False, True), (True, True, True), (False, False, False)])
@pytest.mark.parametrize("P,C,chunks", BN_CASES)
def test_bn_forward_from_caller_partials(P, C, chunks, relu, res, mask):
    """Against f64 (1e-6 relative by norm: y, running and saved statistics) and against eosv_bn_train_forward
    on the same x: the saved statistics within 1 f32 ulp (the two f64 sums differ by at most P 2^-52 relative
    to sum|x| and sum x^2, far below half an f32 ulp; measured on an MI355X: 0 ulp and equal y in every case), y
    within 1e-6."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    rng = np.random.default_rng(P + C + chunks)
    x = (rng.standard_normal((P, C)) + 0.5).astype(np.float32)
    r = rng.standard_normal((P, C)).astype(np.float32) if res else None
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
    rows = -(-P // chunks)
    x64 = x.astype(np.float64)
    part = np.zeros((chunks, 2, C))
    for t in range(chunks):
        part[t, 0], part[t, 1] = x64[t * rows:(t + 1) * rows].sum(axis=0), (x64[t * rows:(t + 1) * rows] ** 2).sum(axis=0)
    pre, yref, mean, invstd, nrm, nrv = _bn_ref(x64, *(v.astype(np.float64) for v in (gamma, beta, rm0, rv0)),
                                                None if r is None else r.astype(np.float64), relu)
    got = {}
    for fused in (True, False):
        xb, xp = _dev_in(x)
        rb, rp = _dev_in(r) if res else (None, None)
        gb, gp = _dev_in(gamma)
        bb, bp = _dev_in(beta)
        pb, pp = _dev_in(part.view(np.float32))
        yb, yp = _dev_out(P * C)
        mb, mp = _dev_out(C)
        ib, ip = _dev_out(C)
        rmb, rmp = _dev_out(C, rm0)
        rvb, rvp = _dev_out(C, rv0)
        mk = torch.full((P * C + 32,), 7, dtype=torch.uint8, device="cuda") if mask else None
        mkp = mk.data_ptr() + 16 if mask else None
        if fused:
            check(L.eosv_bn_train_forward_stats(xp, P, C, pp, chunks, gp, bp, 1e-5, 0.1, rmp, rvp, rp, int(relu), yp, mkp,
                                                mp, ip, s), "eosv_bn_train_forward_stats")
        else:
            work = torch.empty(int(L.eosv_bn_workspace_bytes(C)) // 4 + 4, device="cuda")
            check(L.eosv_bn_train_forward(xp, P, C, gp, bp, 1e-5, 0.1, rmp, rvp, rp, int(relu), yp, mkp, mp, ip,
                                          work.data_ptr(), s), "eosv_bn_train_forward")
        torch.cuda.synchronize()
        out = dict(y=_read_out(yb, P * C, "y").reshape(P, C), mean=_read_out(mb, C, "mean"),
                   invstd=_read_out(ib, C, "invstd"), rm=_read_out(rmb, C, "running mean"),
                   rv=_read_out(rvb, C, "running var"))
        if mask:
            h = mk.cpu().numpy()
            assert (h[:16] == 7).all() and (h[16 + P * C:] == 7).all(), "store outside the mask"
            out["mask"] = h[16:16 + P * C].reshape(P, C)
        got[fused] = out
    f, u = got[True], got[False]

    def rel(a, ref):
        return float(np.linalg.norm(a.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))

    for key, ref in (("y", yref), ("mean", mean), ("invstd", invstd), ("rm", nrm), ("rv", nrv)):
        assert rel(f[key], ref) < 1e-6, (key, rel(f[key], ref))
    if mask:
        sure = np.abs(pre) > 1e-5
        assert np.array_equal(f["mask"][sure] != 0, pre[sure] > 0) and int(f["mask"].max()) <= 1
    ulps = max(float(np.max(np.abs(f[key].astype(np.float64) - u[key]) / np.spacing(np.abs(u[key])))) for key in ("mean", "invstd"))
    print(f"[bn from partials P={P} C={C} chunks={chunks}] saved statistics against the unfused entry: {ulps:g} ulp; "
          f"y {rel(f['y'], u['y'].astype(np.float64)):.2e}")
    assert ulps <= 1.0
    assert rel(f["y"], u["y"].astype(np.float64)) < 1e-6


def test_bn_forward_stats_bad_arguments():
    from eosv._lib import lib

    L = lib()
    p = 4096
    for kw in (dict(part=None), dict(chunks=0), dict(chunks=-3)):
        a = dict(part=p, chunks=1)
        a.update(kw)
        assert L.eosv_bn_train_forward_stats(p, 8, 8, a["part"], a["chunks"], p, p, 1e-5, 0.1, None, None, None, 0, p,
                                             None, p, p, None) == ARG, kw


# ---------------------------------------------------------------- 5. the trainer
class _Counting:
    """The library with every call counted by name."""

    def __init__(self, L):
        self._L, self.calls = L, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._L, name)

        def call(*a):
            self.calls[name] += 1
            return fn(*a)
        return call


CONFIGS = {"resnet18": dict(f32x3_convs=15), "resnet50": dict(f32x3=15, f32x3_convs=15)}
FUSED = {"resnet18": 19, "resnet50": 52}


@functools.lru_cache(maxsize=None)
def _one_step(name, fused, fresh=0):
    """(loss, grads, trainer, call counts) of one step of a fresh trainer of CONFIGS[name] on the small
    case; fused "default" builds it without the keyword; `fresh` only separates cache entries."""
    frames, labels, T = _small_case()
    kw = dict(CONFIGS[name])
    if fused != "default":
        kw["fused_bn_stats"] = fused
    tr = NativeTrainer(name, 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    tr.L = _Counting(tr.L)
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr, tr.L.calls


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_call_counts_follow_the_architecture(name):
    _, _, tr, calls = _one_step(name, 15)
    _, _, off, off_calls = _one_step(name, 0)
    assert calls["eosv_bn_train_forward_stats"] == tr.bn_fused_launches == FUSED[name]
    assert calls["eosv_bn_train_forward"] == 1   # the stem's
    assert calls["eosv_sgemm_x3_stats"] + calls["eosv_conv2d_x3_stats"] == FUSED[name]
    assert (tr.x3_launches, tr.x3c_launches) == (off.x3_launches, off.x3c_launches)
    assert tr.x3c_launches == 51 and tr.x3_launches == (99 if name == "resnet50" else 0)
    assert off.bn_fused_launches == 0 and off_calls["eosv_bn_train_forward"] == FUSED[name] + 1
    if name == "resnet18":
        _, _, one, one_calls = _one_step(name, 1)
        assert one.bn_fused_launches == one_calls["eosv_bn_train_forward_stats"] == 4
        assert one_calls["eosv_bn_train_forward"] == 16


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_default_step_untouched_by_the_keyword(name):
    a, b, z = _one_step(name, "default"), _one_step(name, False), _one_step(name, 0)
    for r in (a, b, z):
        assert r[2].bn_fused_launches == 0 and not any("_stats" in k for k in r[3])
    _same_bytes(a, b)
    _same_bytes(a, z)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_fused_step_is_deterministic(name):
    a, b = _one_step(name, 15), _one_step(name, 15, fresh=1)
    assert a[2].bn_fused_launches == b[2].bn_fused_launches == FUSED[name]
    _same_bytes(a, b)


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_switch_on_against_off(name):
    """The bounds the project uses for BN outputs (1e-6) and for dx / dgamma / dbeta (1e-5): the loss within
    1e-6 relative, every gradient tensor within 1e-5 relative by norm."""
    on, off = _one_step(name, 15), _one_step(name, 0)
    err = abs(on[0] - off[0]) / abs(off[0])
    worst = (0.0, None)
    for k, g in off[1].items():
        e = float((on[1][k].double() - g.double()).norm()) / max(float(g.double().norm()), 1e-30)
        if e > worst[0]:
            worst = (e, k)
    print(f"[bn stats on / off {name}] loss relative difference {err:.2e}; worst gradient {worst[0]:.2e} at {worst[1]}")
    assert err <= 1e-6, (on[0], off[0])
    assert worst[0] <= 1e-5, worst


@pytest.mark.parametrize("name,scaled,need", [("resnet18", ".bn2.weight", dict(checked=55, x3c=16, x3=0)),
                                              ("resnet50", ".bn3.weight", dict(checked=70, x3c=8, x3=12))])
def test_two_steps_against_the_f64_replay(monkeypatch, name, scaled, need):
    """tests/test_gpu_train_x3conv.py's test itself (same state dicts, yardstick, bounds and minima), with the
    switch added to its trainer's keywords; the trainer it builds is caught to see that the BNs were fused."""
    built = []

    class Spy(NativeTrainer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    monkeypatch.setattr(x3conv, "NativeTrainer", Spy)
    x3conv.test_two_steps_against_the_f64_replay(name, scaled, dict(CONFIGS[name], fused_bn_stats=15), need)
    assert len(built) == 1 and built[0].bnstats_mask == 15 and built[0].bn_fused_launches == FUSED[name]
