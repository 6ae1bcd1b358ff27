"""GPU: the opt-in f32x3 GEMMs of the training step's stride-1 1x1 convs (csrc/gemm_x3.hip) and
NativeTrainer(f32x3=mask).

Every GEMM runs in guarded buffers (inputs between NaNs, outputs and workspaces between sentinels)
and twice, with equal bytes.  The numpy model of the arithmetic is tests/test_cpu_train_x3.py's.

1. Exact: integer operands whose every partial sum is an integer below 2^24, so f32 accumulation is
   exact in any order.  One operand wider than bf16 (|a| < 2^12: 8 bits in hi, 4 in lo; |b| <= 7, or
   less at a long reduction so that k max|a| max|b| < 2^24) must give the f64 product bitwise, in
   both roles: this pins hi*hi + lo*hi and hi*hi + hi*lo.  Both operands wider than bf16 must give
   the f64 value of sum (a_hi b_hi + a_hi b_lo + a_lo b_hi) bitwise: lo*lo is dropped and nothing
   else.  For that case 12-bit operands are exact only at k = 1 (4095^2 < 2^24; at k = 16 a sum of
   a 2^24 term and a 1 is no f32), so k = 1 runs 12-bit operands, k <= 16 runs 10-bit ones
   (16 * 2^20 = 2^24) and k = 64, the shortest reduction of NT and NN, 9-bit ones (64 * 2^18).
2. Random f32 operands against the numpy model in f64, |err| <= 1e-5 (1 + sum |terms|) (the conv rule
   of test_gpu_wino.py: room for f32 accumulation order only), and against the true f64 product,
   |err| <= 2^-14 sum |a||b| + 1e-5 (1 + sum |terms|).
3. Refused shapes: EOSV_ERR_UNSUPPORTED with the output still all sentinel, or a result inside 2.
4.-8. The trainer: per-conv wiring against f64, launch counts from arch.SPECS, the default step
   untouched, determinism, and two steps against the f64 replay.

Tile edges of the kernel: a workgroup takes 64 or 128 rows and columns.  TN reaches the four tile
shapes through its channel pairs; unsplit NT / NN halve the tile while the grid is under 512
workgroups, so their 128-row and 128-column tiles need the three LARGE shapes below.  P = 300 is
full tiles plus a ragged one, 100 is under one tile; TN's P = 33 is a second 32-row step with one
row, 1000 and 5000 split into 3 and 18 slices with a ragged last one.

Largest err / bound seen on an MI355X: see DESIGN 3T.
"""
import functools

import numpy as np
import pytest
import torch

from eosv import arch, synth
from eosv.train import NativeTrainer
from _common import _oracle, _same_bytes, _small_case
from test_cpu_train_x3 import split_bf16, x3_terms

pytestmark = pytest.mark.gpu

GUARD = 4096       # floats on each side of the guarded buffers (16 KiB: pointers stay 16-byte aligned)
SENTINEL = -7.25   # exact in f32; the integer cases never produce a fraction
UNSUPPORTED = -4

PAIRS = [(64, 64), (64, 256), (256, 64), (512, 128)]   # (Cin, Cout)
P_ROWS = [1, 100, 300]
P_TN = [1, 31, 33, 1000, 5000]
# (case, P, Cin, Cout): the 128 x 128, 64 x 128 and 128 x 64 tiles of the unsplit kernels, each with a ragged last row tile
LARGE = [("NT", 4100, 64, 2048), ("NN", 4100, 2048, 64), ("NT", 2050, 64, 2048), ("NN", 2050, 2048, 64),
         ("NT", 65540, 64, 64), ("NN", 65540, 64, 64)]


def _dims(case, P, cin, cout):
    """(m, n, k) of the conv's GEMM: NT forward, NN input gradient, TN weight gradient."""
    return {"NT": (P, cout, cin), "NN": (P, cin, cout), "TN": (cout, cin, P)}[case]


def _dev_in(a):
    """A numpy f32 array between NaN guards on the device -> (buffer, pointer of its first element)."""
    flat = torch.full((a.size + 2 * GUARD,), float("nan"))
    flat[GUARD:GUARD + a.size] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1))
    buf = flat.cuda()
    return buf, buf.data_ptr() + 4 * GUARD


def _dev_out(numel, init=None):
    flat = torch.full((numel + 2 * GUARD,), SENTINEL)
    if init is not None:
        flat[GUARD:GUARD + numel] = torch.from_numpy(np.ascontiguousarray(init, np.float32).reshape(-1))
    buf = flat.cuda()
    return buf, buf.data_ptr() + 4 * GUARD


def _read_out(buf, numel, what):
    h = buf.cpu()
    assert bool((h[:GUARD] == SENTINEL).all()) and bool((h[GUARD + numel:] == SENTINEL).all()), \
        f"store outside {what}"
    return h[GUARD:GUARD + numel].numpy().copy()


def _launch(case, A, B, alpha=1.0, beta=0.0, c0=None, add=None, split=None, expect_ok=True):
    """C of one launch.  A [m][k], B [k][n] (numpy, the logical operands) are stored as the case has
    them in memory.  split None: eosv_sgemm_x3; "none" / "work": eosv_sgemm_x3_tn_splitk without /
    with the workspace (TN only)."""
    from eosv._lib import check, lib, stream_ptr

    L, s = lib(), stream_ptr()
    m, k = A.shape
    n = B.shape[1]
    ta, tb = case == "TN", case == "NT"
    a_mem = A.T if ta else A
    b_mem = B.T if tb else B
    abuf, ap = _dev_in(a_mem)
    bbuf, bp = _dev_in(b_mem)
    addbuf, addp = _dev_in(add) if add is not None else (None, None)
    cbuf, cp = _dev_out(m * n, c0)
    if split is None:
        rc = L.eosv_sgemm_x3(int(ta), int(tb), m, n, k, alpha, ap, a_mem.shape[1], bp, b_mem.shape[1], beta, cp, n,
                             addp, s)
    else:
        assert case == "TN" and alpha == 1.0 and beta == 0.0 and add is None
        wb = int(L.eosv_sgemm_x3_tn_splitk_workspace(m, n, k)) if split == "work" else 0
        wbuf, wp = _dev_out(wb // 4) if wb else (None, None)
        rc = L.eosv_sgemm_x3_tn_splitk(m, n, k, ap, m, bp, n, cp, n, wp, wb, s)
    torch.cuda.synchronize()
    if expect_ok:
        check(rc, "eosv_sgemm_x3")
    out = _read_out(cbuf, m * n, "C").reshape(m, n)
    if split == "work" and wb:
        _read_out(wbuf, wb // 4, "the workspace")
    return rc, out


def _twice(*args, **kw):
    _, c1 = _launch(*args, **kw)
    _, c2 = _launch(*args, **kw)
    assert c1.tobytes() == c2.tobytes(), "two launches differ"
    return c1


def _ints(rng, shape, bits):
    hi = (1 << bits) - 1
    return rng.integers(-hi, hi + 1, size=shape).astype(np.float32)


def _narrow(rng, shape, k):
    """The bf16-exact operand of an exact case: |b| <= 7, less where k * 4095 * 7 would pass 2^24."""
    bmax = 7 if k * 4095 * 7 < 2 ** 24 else 1
    return rng.integers(-bmax, bmax + 1, size=shape).astype(np.float32)


def _wide_bits(k):
    return 12 if k * 4095 < 2 ** 24 else 11


EXACT = ([(c, P, ci, co) for c in ("NT", "NN") for ci, co in PAIRS for P in P_ROWS] +
         [("TN", P, ci, co) for ci, co in PAIRS for P in P_TN])


@pytest.mark.parametrize("case,P,cin,cout", EXACT, ids=lambda v: str(v))
def test_exact_one_wide_operand_either_role(case, P, cin, cout):
    m, n, k = _dims(case, P, cin, cout)
    rng = np.random.default_rng(m * 7 + n * 3 + k)
    for wide_a in (True, False):
        A = _ints(rng, (m, k), _wide_bits(k)) if wide_a else _narrow(rng, (m, k), k)
        B = _narrow(rng, (k, n), k) if wide_a else _ints(rng, (k, n), _wide_bits(k))
        ref = A.astype(np.float64) @ B.astype(np.float64)
        assert float(np.abs(A).astype(np.float64).max() * np.abs(B).astype(np.float64).max() * k) < 2 ** 24
        got = _twice(case, A, B)
        assert np.array_equal(got.astype(np.float64), ref), ("hi*hi + lo*hi" if wide_a else "hi*hi + hi*lo")
        if case == "TN":
            for split in ("none", "work"):
                got = _twice(case, A, B, split=split)
                assert np.array_equal(got.astype(np.float64), ref), split


@pytest.mark.parametrize("case,P,cin,cout,bits", [("TN", 1, 64, 64, 12), ("TN", 1, 512, 128, 12),
                                                    ("TN", 16, 64, 256, 10), ("TN", 13, 256, 64, 10),
                                                    ("NT", 100, 64, 64, 9), ("NT", 300, 64, 256, 9),
                                                    ("NN", 100, 64, 64, 9), ("NN", 300, 256, 64, 9)],
                         ids=lambda v: str(v))
def test_exact_both_operands_wide_drops_only_lo_lo(case, P, cin, cout, bits):
    m, n, k = _dims(case, P, cin, cout)
    assert k * (2 ** bits) ** 2 <= 2 ** 24
    rng = np.random.default_rng(bits * 1000 + m + n + k)
    A, B = _ints(rng, (m, k), bits), _ints(rng, (k, n), bits)
    model = x3_terms(A, B)
    full = A.astype(np.float64) @ B.astype(np.float64)
    assert not np.array_equal(model, full), "the case has no lo * lo term to drop"
    got = _twice(case, A, B)
    assert np.array_equal(got.astype(np.float64), model)
    if case == "TN":
        for split in ("none", "work"):
            assert np.array_equal(_twice(case, A, B, split=split).astype(np.float64), model), split


@pytest.mark.parametrize("case,P,cin,cout", [("NT", 100, 64, 256), ("NN", 300, 256, 64), ("TN", 33, 64, 64)],
                         ids=lambda v: str(v))
def test_exact_beta_and_addend_on_integer_c(case, P, cin, cout):
    m, n, k = _dims(case, P, cin, cout)
    rng = np.random.default_rng(m + 5 * n + 11 * k)
    A, B = _ints(rng, (m, k), 12), _narrow(rng, (k, n), k)
    c0, add = _ints(rng, (m, n), 10), _ints(rng, (m, n), 10)
    ref = A.astype(np.float64) @ B.astype(np.float64)
    assert np.array_equal(_twice(case, A, B, beta=1.0, c0=c0).astype(np.float64), ref + c0)
    assert np.array_equal(_twice(case, A, B, add=add).astype(np.float64), ref + add)
    assert np.array_equal(_twice(case, A, B, beta=1.0, c0=c0, add=add).astype(np.float64), ref + c0 + add)
    # beta = 0 does not read C: a NaN-filled C comes back clean
    nan_c = np.full((m, n), np.nan, np.float32)
    assert np.array_equal(_twice(case, A, B, c0=nan_c).astype(np.float64), ref)


def _check_random(tag, got, A, B, alpha=1.0, extra=None):
    """The two bounds of item 2; extra: the f64 sum of the epilogue's other terms (beta C + add)."""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    mag_ab = abs(alpha) * (np.abs(A64) @ np.abs(B64))
    model, true = alpha * x3_terms(A, B), alpha * (A64 @ B64)
    mag = mag_ab.copy()
    if extra is not None:
        model, true, mag = model + extra[0], true + extra[0], mag + extra[1]
    assert np.isfinite(got).all(), tag
    g = got.astype(np.float64)
    r_model = float((np.abs(g - model) / (1e-5 * (1.0 + mag))).max())
    r_true = float((np.abs(g - true) / (2.0 ** -14 * mag_ab + 1e-5 * (1.0 + mag))).max())
    print(f"x3 {tag}: max err / bound = {r_model:.3e} against the x3 model, {r_true:.3e} against f64")
    assert r_model <= 1.0, (tag, "against the x3 model", r_model)
    assert r_true <= 1.0, (tag, "against f64", r_true)
    return r_model, r_true


RANDOM = ([(c, P, ci, co) for c in ("NT", "NN") for ci, co in PAIRS for P in P_ROWS] +
          [("TN", P, ci, co) for ci, co in PAIRS for P in P_TN] + LARGE)


@pytest.mark.parametrize("case,P,cin,cout", RANDOM, ids=lambda v: str(v))
def test_random_operands_against_the_model_and_f64(case, P, cin, cout):
    m, n, k = _dims(case, P, cin, cout)
    rng = np.random.default_rng(m * 13 + n * 5 + k)
    A = rng.standard_normal((m, k)).astype(np.float32)
    B = rng.standard_normal((k, n)).astype(np.float32)
    tag = f"{case} m {m} n {n} k {k}"
    _check_random(tag, _twice(case, A, B), A, B)
    if case == "TN":
        for split in ("none", "work"):
            _check_random(f"{tag} split-K entry, workspace: {split}", _twice(case, A, B, split=split), A, B)


@pytest.mark.parametrize("case,P,cin,cout", [("NT", 300, 512, 128), ("NN", 300, 512, 128), ("TN", 1000, 64, 256)],
                         ids=lambda v: str(v))
def test_random_scaled_operands_and_epilogue(case, P, cin, cout):
    """Operands scaled by 1e3 and 1e-3; then alpha, beta and the addend together."""
    m, n, k = _dims(case, P, cin, cout)
    rng = np.random.default_rng(m + n + k)
    A = (rng.standard_normal((m, k)) * 1e3).astype(np.float32)
    B = (rng.standard_normal((k, n)) * 1e-3).astype(np.float32)
    tag = f"{case} m {m} n {n} k {k} scaled"
    _check_random(tag, _twice(case, A, B), A, B)
    if case == "TN":
        _check_random(tag + " split-K", _twice(case, A, B, split="work"), A, B)
    c0 = rng.standard_normal((m, n)).astype(np.float32)
    add = rng.standard_normal((m, n)).astype(np.float32)
    extra = (0.5 * c0.astype(np.float64) + add.astype(np.float64), 0.5 * np.abs(c0) + np.abs(add))
    _check_random(tag + " alpha -2 beta 0.5 + add", _twice(case, A, B, alpha=-2.0, beta=0.5, c0=c0, add=add), A, B,
                  alpha=-2.0, extra=extra)


@pytest.mark.parametrize("what", ["channels 72 (n)", "channels 72 (k)", "pointer off 16 bytes", "lda % 4 != 0"])
def test_refused_shapes_write_nothing_or_compute_correctly(what):
    """Either EOSV_ERR_UNSUPPORTED with the output buffer still all sentinel, or success with a
    result inside the bounds of the random cases; never anything else."""
    from eosv._lib import lib, stream_ptr

    L, s = lib(), stream_ptr()
    rng = np.random.default_rng(72)
    m, n, k = 100, 64, 64
    if what == "channels 72 (n)":
        n = 72
    if what == "channels 72 (k)":
        k = 72
    lda = k + 2 if what.startswith("lda") else k
    A = rng.standard_normal((m, k)).astype(np.float32)
    B = rng.standard_normal((k, n)).astype(np.float32)
    a_mem = np.zeros((m, lda), np.float32)
    a_mem[:, :k] = A
    off = 4 if what.startswith("pointer") else 0   # bytes: the same data, one float further
    abuf, ap = _dev_in(np.concatenate([np.zeros(off // 4, np.float32), a_mem.reshape(-1)]))
    bbuf, bp = _dev_in(B.T)
    cbuf, cp = _dev_out(m * n)
    rc = L.eosv_sgemm_x3(0, 1, m, n, k, 1.0, ap + off, lda, bp, k, 0.0, cp, n, None, s)
    torch.cuda.synchronize()
    got = _read_out(cbuf, m * n, "C").reshape(m, n)
    assert rc in (0, UNSUPPORTED), rc
    if rc == UNSUPPORTED:
        assert bool((got == SENTINEL).all()), "a refused call wrote"
    else:
        _check_random(what, got, A, B)


# ---------------------------------------------------------------- the trainer
def _eligible(name, mask=15):
    """[(conv name, layer index)] of the stride-1 1x1 convs of the enabled stages, from arch.SPECS:
    conv1 and conv3 of every bottleneck, and the downsample of a first block that keeps the stride."""
    spec = arch.SPECS[name]
    out = []
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), spec.layers)):
        for bi in range(blocks):
            stride = 2 if (li > 0 and bi == 0) else 1
            cout = planes * spec.expansion
            p = f"convnet.{4 + li}.{bi}"
            if spec.block != "basic" and mask >> li & 1:
                out += [(p + ".conv1", li), (p + ".conv3", li)]
                if bi == 0 and (stride != 1 or inplanes != cout) and stride == 1:
                    out.append((p + ".downsample.0", li))
            inplanes = cout
    return out


def test_eligible_conv_counts():
    assert len(_eligible("resnet50")) == 33 and len(_eligible("resnet50", 1)) == 7
    assert len(_eligible("resnet50", 8)) == 6 and _eligible("resnet18") == []
    # and the trainer marks exactly these
    for mask in (15, 1, 8):
        tr = NativeTrainer("resnet50", 64, device=0, f32x3=mask)
        assert sorted(c.name for c in tr._convs() if c.x3) == sorted(n for n, _ in _eligible("resnet50", mask))


def _conv_named(tr, name):
    return next(c for c in tr._convs() if c.name == name)


@functools.lru_cache(maxsize=None)
def _wired_trainer(f32x3):
    tr = NativeTrainer("resnet50", 64, device=0, f32x3=f32x3)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS["resnet50"], 64, 0))
    return tr


@pytest.mark.parametrize("name,hw", [("convnet.4.0.conv3", 24), ("convnet.4.0.downsample.0", 24),
                                     ("convnet.5.1.conv1", 12), ("convnet.6.0.conv3", 6), ("convnet.7.1.conv1", 3)])
def test_trainer_conv_calls_take_the_x3_gemms(name, hw):
    """_conv_fwd and _conv_bwd of one eligible conv per stage (and the layer-1 downsample) at N = 2 and
    the stage's map of a 96 x 96 frame, against the f64 GEMMs of the 1x1 conv."""
    from eosv._lib import stream_ptr

    N = 2
    P = N * hw * hw
    got = {}
    for mask in (15, False):
        tr = _wired_trainer(mask)
        c = _conv_named(tr, name)
        assert c.x3 is (mask == 15) and c.k == 1 and c.stride == 1
        g = torch.Generator().manual_seed(hw * 1000 + c.cin)
        x = torch.randn(P, c.cin, generator=g)
        dz = torch.randn(P, c.cout, generator=g)
        acc = torch.randn(P, c.cin, generator=g)
        s = stream_ptr()
        tr.x3_launches = 0
        xd, dzd, accd = (t.cuda().reshape(-1) for t in (x, dz, acc))
        y, oshape = tr._conv_fwd(xd, (N, hw, hw, c.cin), c, s)
        assert oshape == (N, hw, hw, c.cout)
        assert tr.x3_launches == (1 if mask == 15 else 0)
        tr.x3_launches = 0
        dx = tr._conv_bwd(dzd, xd, (N, hw, hw, c.cin), c, s, need_dx=True, acc=accd)
        assert tr.x3_launches == (2 if mask == 15 else 0)
        torch.cuda.synchronize()
        got[mask] = (y.cpu().numpy().reshape(P, c.cout), c.g.cpu().numpy().reshape(c.cout, c.cin),
                     dx.cpu().numpy().reshape(P, c.cin))
        w = c.w.cpu().numpy().reshape(c.cout, c.cin)
    y, gw, dx = got[15]
    xn, dzn, accn = x.numpy(), dz.numpy(), acc.numpy()
    _check_random(f"{name} forward", y, xn, np.ascontiguousarray(w.T))
    _check_random(f"{name} weight gradient", gw, np.ascontiguousarray(dzn.T), xn)
    _check_random(f"{name} input gradient + acc", dx, dzn, w, extra=(accn.astype(np.float64), np.abs(accn)))
    # the f32 path computes the same conv in another arithmetic: the x3 path really was taken
    for a, b, what in zip(got[15], got[False], ("y", "dW", "dx")):
        assert a.tobytes() != b.tobytes(), what
        assert np.allclose(a, b, rtol=1e-2, atol=1e-2), what


@functools.lru_cache(maxsize=None)
def _one_step(name, f32x3, fresh=0):
    """(loss, grads, x3_launches) of one step of a fresh trainer on the small case; f32x3 "default"
    builds the trainer without the keyword; `fresh` only separates cache entries."""
    frames, labels, T = _small_case()
    kw = {} if f32x3 == "default" else {"f32x3": f32x3}
    tr = NativeTrainer(name, 64, device=0, **kw)
    tr.load_state_dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    loss, _ = tr.step(frames.cuda(), labels, T, 1e-3, 1e-2)
    return loss, tr.grads(), tr.x3_launches


def test_launch_counts_follow_the_architecture():
    """Every eligible conv launches its forward, input gradient and weight gradient GEMM once."""
    assert 3 * len(_eligible("resnet50")) == 99
    assert _one_step("resnet50", 15)[2] == 3 * len(_eligible("resnet50")) == 99
    assert _one_step("resnet50", 1)[2] == 3 * len(_eligible("resnet50", 1)) == 21
    r18 = _one_step("resnet18", 15)
    assert r18[2] == 0
    _same_bytes(r18, _one_step("resnet18", "default"))


def test_default_step_untouched_by_the_keyword():
    a, b = _one_step("resnet50", "default"), _one_step("resnet50", False)
    assert a[2] == 0 and b[2] == 0
    _same_bytes(a, b)
    c = _one_step("resnet50", 15)
    assert any(c[1][k].numpy().tobytes() != a[1][k].numpy().tobytes() for k in a[1])


def test_x3_step_is_deterministic():
    a, b = _one_step("resnet50", 15), _one_step("resnet50", 15, fresh=1)
    assert a[2] == b[2] == 99
    _same_bytes(a, b)


def test_two_steps_against_the_f64_replay():
    """The synthetic ResNet-50 with every bn3.weight scaled by 0.05, where torch's own f32 replay stays
    within 1e-4 (relative gradient norm) of f64 for most tensors: an arithmetic with 2^8 times f32's
    unit roundoff can be judged there.  Per tensor yard = |g_f32 - g_f64| / |g_f64| from torch; every
    tensor with yard <= 1e-4 must have |g - g_f64| / |g_f64| <= max(1024 yard, 2e-2) (1024: the
    project's factor 4 times 2^-16 : 2^-24), both losses within max(1e-4, 1024 yard_loss); at least
    70 tensors and 12 eligible 1x1 weights must be checked."""
    name = "resnet50"
    lr1, lr2 = 1e-3, 1e-2
    sd = dict(synth.synth_state_dict(arch.SPECS[name], 64, 0))
    for k in sd:
        if k.endswith(".bn3.weight"):
            sd[k] = (np.asarray(sd[k]) * np.float32(0.05)).astype(np.float32)
    frames, labels, T = _small_case()
    ref_losses, ref_g, _ = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float64)
    f32_losses, f32_g, _ = _oracle(name, sd, frames, labels, T, lr1, lr2, 2, torch.float32)

    tr = NativeTrainer(name, 64, device=0, f32x3=15)
    tr.load_state_dict(sd)
    l0, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    g0 = tr.grads()
    l1, _ = tr.step(frames.cuda(), labels, T, lr1, lr2)
    assert tr.x3_launches == 99
    for got, ref, f32 in ((l0, ref_losses[0], f32_losses[0]), (l1, ref_losses[1], f32_losses[1])):
        yard = abs(f32 - ref) / abs(ref)
        err = abs(got - ref) / abs(ref)
        print(f"[x3 two steps] loss {got:.7f} / f64 {ref:.7f}: relative error {err:.2e}, torch-f32 yardstick {yard:.2e}")
        assert err <= max(1e-4, 1024 * yard), (got, ref, yard)
    x3_weights = {n + ".weight" for n, _ in _eligible(name)}
    assert x3_weights <= set(ref_g)
    worst, ratio = (0.0, None, 0.0), (0.0, None)
    checked, checked_x3, left_out = 0, 0, []
    for k, gr in ref_g.items():
        norm = max(float(gr.norm()), 1e-12)
        yard = float((f32_g[k] - gr).norm()) / norm
        if yard > 1e-4:
            left_out.append(k)
            continue
        err = float((g0[k].double() - gr).norm()) / norm
        bound = max(1024 * yard, 2e-2)
        checked += 1
        checked_x3 += k in x3_weights
        if err > worst[0]:
            worst = (err, k, yard)
        if err / bound > ratio[0]:
            ratio = (err / bound, k)
        assert err <= bound, (k, err, yard)
    print(f"[x3 two steps] {checked} tensors checked ({checked_x3} of the 33 f32x3 weights); worst relative gradient "
          f"error {worst[0]:.2e} at {worst[1]} (yardstick {worst[2]:.2e}); largest error / bound {ratio[0]:.3f} at "
          f"{ratio[1]}; left out (yardstick > 1e-4): {len(left_out)}: {', '.join(left_out)}")
    assert checked >= 70 and checked_x3 >= 12, (checked, checked_x3)
