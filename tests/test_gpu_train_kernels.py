"""GPU: the training step's kernels that are not convolutions (csrc/train.hip: batch norm, max pool,
average pool, broadcast, softmax cross-entropy, row sum, bias, SGD, axpy, layout changes), one by one
against plain torch in f64, at the smallest shapes that reach each path of the ResNet-50 step.

Conventions of every case:
  * inputs are f64 tensors from a seeded CPU generator holding f32-representable values (rounded once
    on the host), so the cast to f32 for the device is exact and an error is the kernel's alone;
  * the reference is plain torch in f64; errors are relative by norm (as in test_gpu_train.py) or, where
    a rounding count gives one, a bound per element; each case prints its measured error and bound;
  * outputs live in guarded buffers (as in test_gpu_wino_wgrad.py): GUARD elements on each side filled
    with a sentinel (SENTINEL for f32, a byte / int pattern for the mask and the indices), both guards
    bitwise intact after the call and no sentinel left inside.

Not covered: the grid-stride second trip of the elementwise kernels (grid_for caps at 2^20 blocks: more
than 2.7e8 elements, ten times the largest tensor of the 96-frame ResNet-50 step), and NaN in the max
pool (the kernel keeps the first tap and later larger values, `v > m`; torch propagates NaN).
"""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096       # elements on each side of the guarded buffers
SENTINEL = -7.25   # exact in f32, never a result of these inputs by chance
_SENT = {torch.float32: SENTINEL, torch.uint8: 0xA5, torch.int32: -7}
U = 2.0 ** -24     # f32 unit roundoff (one rounding, relative)
F64 = torch.float64


def _call(fn, *args):
    from eosv._lib import check, stream_ptr

    check(fn(*args, stream_ptr()), fn.__name__)
    torch.cuda.synchronize()


def _randn(g, *shape, scale=1.0, shift=0.0):
    """f64 normal values that f32 holds exactly."""
    return (torch.randn(*shape, generator=g, dtype=F64) * scale + shift).float().double()


def _rand(g, *shape, shift=0.0):
    return (torch.rand(*shape, generator=g, dtype=F64) + shift).float().double()


def _dev(t, off=0, dtype=torch.float32):
    """An input on the device, starting `off` elements into its allocation: (holder, pointer)."""
    flat = t.detach().reshape(-1).to(dtype)
    h = torch.zeros(flat.numel() + off, dtype=dtype)
    h[off:] = flat
    d = h.cuda()
    return d, d.data_ptr() + off * d.element_size()


def _guarded(n, dtype=torch.float32, off=0, init=None):
    """An output of n elements between two sentinel guards, `off` elements past the alignment of the
    allocation (GUARD elements keep it: 16 KiB of f32, 4 KiB of bytes): (buffer, pointer).  init: the
    values an in-place kernel starts from."""
    buf = torch.full((n + 2 * GUARD + off,), _SENT[dtype], dtype=dtype)
    if init is not None:
        buf[GUARD + off:GUARD + off + n] = init.detach().reshape(-1).to(dtype)
    buf = buf.cuda()
    return buf, buf.data_ptr() + (GUARD + off) * buf.element_size()


def _take(buf, n, off=0, what="output"):
    """The n values of a guarded buffer (CPU), after checking the guards and that every slot was written."""
    torch.cuda.synchronize()
    h = buf.cpu()
    lo = GUARD + off
    ref = torch.full((1,), _SENT[h.dtype], dtype=h.dtype)
    bits = (lambda t: t.view(torch.int32)) if h.dtype == torch.float32 else (lambda t: t)
    assert bool((bits(h[:lo]) == bits(ref)).all()), f"{what}: store below the buffer"
    assert bool((bits(h[lo + n:]) == bits(ref)).all()), f"{what}: store past the buffer"
    got = h[lo:lo + n].clone()
    assert bool((bits(got) != bits(ref)).all()), f"{what}: a slot was not written"
    return got


def _rel(got, ref):
    """Relative error by norm; a reference of norm zero asks for exact zeros."""
    ref = ref.detach().double().reshape(-1)
    got = got.double().reshape(-1)
    n = float(ref.norm())
    if n == 0.0:
        return 0.0 if not bool(got.any()) else float("inf")
    return float((got - ref).norm()) / n


# ---------------------------------------------------------------- a. batch norm
BN_EPS, BN_MOM = 1e-5, 0.1
BAND = 1e-5  # |pre-activation| below which f32 and f64 may disagree on the ReLU mask


@functools.lru_cache(maxsize=1)
def _bn_case(P, C):
    """Inputs and the f64 graph of train-mode batch norm over [P][C] rows, built once per shape: the
    pre-activation with and without the residual, the batch statistics and the running estimates."""
    g = torch.Generator().manual_seed(100003 * P + C)
    cs = types.SimpleNamespace()
    cs.x = _randn(g, P, C, scale=2.0, shift=0.5).requires_grad_()
    cs.r = _randn(g, P, C).requires_grad_()
    cs.dy = _randn(g, P, C)
    cs.gamma = _rand(g, C, shift=0.5).requires_grad_()
    cs.beta = _randn(g, C).requires_grad_()
    cs.rm0, cs.rv0 = _randn(g, C), _rand(g, C, shift=0.5)
    with torch.no_grad():
        cs.mean = cs.x.mean(0)
        var = ((cs.x - cs.mean) ** 2).mean(0)
        cs.invstd = 1.0 / torch.sqrt(var + BN_EPS)
    if P > 1:
        cs.rm, cs.rv = cs.rm0.clone(), cs.rv0.clone()
        cs.pre = torch.nn.functional.batch_norm(cs.x, cs.rm, cs.rv, cs.gamma, cs.beta, True, BN_MOM, BN_EPS)
    else:
        # torch refuses one value per channel; the kernel's P = 1 branch keeps the (zero) biased
        # variance as the running estimate's sample: the formula itself, in f64
        m = cs.x.mean(0)
        v = ((cs.x - m) ** 2).mean(0)
        cs.pre = (cs.x - m) / torch.sqrt(v + BN_EPS) * cs.gamma + cs.beta
        cs.rm = (1 - BN_MOM) * cs.rm0 + BN_MOM * m.detach()
        cs.rv = (1 - BN_MOM) * cs.rv0 + BN_MOM * v.detach()
    cs.pre_r = cs.pre + cs.r
    return cs


def _bn_run(P, C, relu, res, mask, want_dres, mis=None):
    """One forward and one backward call; every output guarded and returned on the CPU.
    mis: None (every operand 16-byte aligned), "all" (every f32 operand 4 bytes past a 16-byte
    boundary), "ydx" (only the forward's y and the backward's dx), "mask" (only the mask, by a byte)."""
    from eosv._lib import lib

    L = lib()
    cs = _bn_case(P, C)
    fo = 1 if mis == "all" else 0
    yo = 1 if mis in ("all", "ydx") else 0
    mo = 1 if mis == "mask" else 0
    n = P * C
    keep = []

    def inp(t):
        h, p = _dev(t, fo)
        keep.append(h)
        return p

    x_p, g_p, b_p, dy_p = inp(cs.x), inp(cs.gamma), inp(cs.beta), inp(cs.dy)
    r_p = inp(cs.r) if res else None
    rm, rm_p = _guarded(C, off=fo, init=cs.rm0)
    rv, rv_p = _guarded(C, off=fo, init=cs.rv0)
    y, y_p = _guarded(n, off=yo)
    mean, mean_p = _guarded(C, off=fo)
    inv, inv_p = _guarded(C, off=fo)
    mk, mk_p = _guarded(n, torch.uint8, off=mo) if mask else (None, None)
    # NaN workspace: a partial sum that is read was written by this call
    work = torch.full((int(L.eosv_bn_workspace_bytes(C)) // 8 + 2,), float("nan"), dtype=F64, device="cuda")
    _call(L.eosv_bn_train_forward, x_p, P, C, g_p, b_p, BN_EPS, BN_MOM, rm_p, rv_p, r_p, int(relu), y_p, mk_p,
          mean_p, inv_p, work.data_ptr())
    out = {"y": _take(y, n, yo, "y"), "mean": _take(mean, C, fo, "save_mean"), "inv": _take(inv, C, fo, "save_invstd"),
           "rm": _take(rm, C, fo, "running_mean"), "rv": _take(rv, C, fo, "running_var")}
    if mask and relu:
        out["mask"] = _take(mk, n, mo, "mask")
    y_in = None
    if not (mask and relu):  # the backward reads y
        if mis == "ydx":  # an aligned copy, so that the statistics pass stays on four channels per lane
            ycopy = out["y"].cuda()
            keep.append(ycopy)
            y_in = ycopy.data_ptr()
        else:
            y_in = y_p
    work.fill_(float("nan"))
    dx, dx_p = _guarded(n, off=yo)
    dg, dg_p = _guarded(C, off=fo)
    db, db_p = _guarded(C, off=fo)
    dres, dres_p = _guarded(n, off=fo) if want_dres else (None, None)
    _call(L.eosv_bn_train_backward, dy_p, y_in, mk_p, int(relu), x_p, P, C, g_p, mean_p, inv_p, dx_p, dg_p, db_p,
          dres_p, work.data_ptr())
    out.update(dx=_take(dx, n, yo, "dx"), dg=_take(dg, C, fo, "dgamma"), db=_take(db, C, fo, "dbeta"))
    if want_dres:
        out["dres"] = _take(dres, n, fo, "dres")
    # the backward left the forward's outputs alone
    assert torch.equal(_take(y, n, yo, "y"), out["y"]) and torch.equal(_take(mean, C, fo, "save_mean"), out["mean"])
    return out


def _bn_check(P, C, relu, res, mask, want_dres, out, tag):
    """The outputs of _bn_run against the f64 graph, the ReLU mask taken from the kernel: a
    pre-activation within f32 rounding of 0 may legitimately land on either side, and one flipped
    element moves dx far beyond 1e-5, so the mask is checked on its own (equal to pre > 0 outside a
    1e-5 band, six times f32's own distance from f64 here; at most 1e-4 of the elements inside it)
    and then used for the reference output and gradients."""
    cs = _bn_case(P, C)
    pre = cs.pre_r if res else cs.pre
    y = out["y"].view(P, C)
    share = 0.0
    if relu:
        keepm = y > 0
        if mask:
            m = out["mask"].view(P, C)
            assert int(m.max()) <= 1, "mask bytes other than 0 / 1"
            assert torch.equal(m.bool(), keepm), "mask bytes differ from y > 0"
        pd = pre.detach()
        band = pd.abs() <= BAND
        share = float(band.double().mean())
        assert torch.equal(keepm[~band], (pd > 0)[~band]), "ReLU mask wrong outside the rounding band"
        y_ref = pre * keepm.double()
    else:
        y_ref = pre
    wrt = [cs.x, cs.gamma, cs.beta] + ([cs.r] if res else [])
    grads = torch.autograd.grad(y_ref, wrt, cs.dy, retain_graph=True)
    checks = [("y", out["y"], y_ref, 1e-6), ("running_mean", out["rm"], cs.rm, 1e-6),
              ("running_var", out["rv"], cs.rv, 1e-6), ("save_mean", out["mean"], cs.mean, 1e-6),
              ("save_invstd", out["inv"], cs.invstd, 1e-6), ("dx", out["dx"], grads[0], 1e-5),
              ("dgamma", out["dg"], grads[1], 1e-5), ("dbeta", out["db"], grads[2], 1e-5)]
    if res and want_dres:
        checks.append(("dres", out["dres"], grads[3], 1e-6))
    errs = [(name, _rel(got, ref), bound) for name, got, ref, bound in checks]
    print(f"bn {tag} P={P} C={C} relu={relu} res={res} mask={mask} dres={want_dres}: "
          + ", ".join(f"{name} {e:.2e}/{b:.0e}" for name, e, b in errs)
          + (f"; share inside the {BAND:.0e} band {share:.2e} (bound 1e-4)" if relu else ""))
    assert share <= 1e-4
    for name, e, b in errs:
        assert e < b, (name, e, b)


# (relu, res, mask, want_dres): the trainer's conv1 / conv2 BN; the same reading y in the backward;
# the block's last BN with the residual gradient; plain BN (the downsample branch)
_F_MAIN = [(True, False, True, False), (True, False, False, False)]
_F_MORE = [(True, True, True, True), (False, False, False, False)]
# (P rows, C): the path only this shape reaches
BN_SHAPES = [
    (37, 2048, _F_MAIN + _F_MORE),   # two channel blocks in the partials, two c4 passes in apply4 / dx4, nr = 1
    (41, 1028, _F_MAIN + _F_MORE),   # C4 = 257: the second channel block and c4 pass have one live lane
    (2100, 1024, _F_MAIN),           # 131 chunks: a second trip of the finalize loop, most lanes idle
    (16500, 1024, _F_MAIN),          # bn_chunks capped at 1024; 17 rows per chunk, chunks 971..1023 empty
    (75, 300, _F_MAIN),              # aligned: C4 = 75 of 128 lanes, two row lanes (the base of the offset runs)
    (1, 8, _F_MAIN),                 # P = 1: the `P > 1 ? ... : var` branch of the running variance
    (3, 8, _F_MAIN),                 # fewer rows than row lanes
]
BN_CASES = [(P, C) + f for P, C, flags in BN_SHAPES for f in flags]
_ids = lambda v: str(int(v)) if not isinstance(v, bool) else "FT"[v]  # noqa: E731


@pytest.mark.parametrize("P,C,relu,res,mask,want_dres", BN_CASES, ids=_ids)
def test_bn_vs_f64(P, C, relu, res, mask, want_dres):
    """eosv_bn_train_forward / _backward against f64 at the shapes of BN_SHAPES, bounds of
    test_batchnorm_train_forward_backward_vs_torch (y, running estimates, saved statistics, residual
    gradient 1e-6; dx, dgamma, dbeta 1e-5)."""
    out = _bn_run(P, C, relu, res, mask, want_dres)
    _bn_check(P, C, relu, res, mask, want_dres, out, "aligned")


# the offset runs: (75, 300) with every operand offset is the scalar statistics pass (one channel per
# lane) with two channel blocks, the last one ragged (44 of 256 lanes); "mask" needs mask bytes
BN_MIS = [(P, C, mis) + f for P, C, flags in (BN_SHAPES[4], BN_SHAPES[0]) for mis in ("all", "ydx", "mask")
          for f in flags if mis != "mask" or f[2]]


@pytest.mark.parametrize("P,C,mis,relu,res,mask,want_dres", BN_MIS,
                         ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_bn_misaligned_operands(P, C, mis, relu, res, mask, want_dres):
    """The fallbacks of a float4-eligible shape (C % 4 == 0) whose operands are not 16-byte aligned
    (include/eosv.h is a C ABI; not every caller is torch's allocator): "all" sends everything down the
    scalar kernels, "ydx" feeds the four-channel statistics into the scalar apply / dx, "mask" offsets
    the mask bytes alone.  Same f64 bounds, and y, dx and the mask bitwise equal to the aligned call's:
    the elementwise passes are the same arithmetic per element, and the statistics differ between the
    paths only in the order of f64 partial sums, below the f32 rounding of mean, invstd and the two
    gradient sums.  (This test found dx one bit apart between bn_dx4 and bn_dx: the compiler fused
    xhat * mgx into the subtraction in one kernel and not in the other; bn_dx1 now writes the fma.)"""
    out = _bn_run(P, C, relu, res, mask, want_dres, mis)
    _bn_check(P, C, relu, res, mask, want_dres, out, mis)
    base = _bn_run(P, C, relu, res, mask, want_dres)
    for k in ("y", "dx") + (("mask",) if mask and relu else ()):
        assert out[k].numpy().tobytes() == base[k].numpy().tobytes(), f"{k} differs from the aligned call's"


# ---------------------------------------------------------------- b. head kernels, one by one
@pytest.mark.parametrize("N,HW,C", [(5, 49, 2048),   # layer4 of ResNet-50: 40 blocks of 256 lanes
                                    (3, 1, 64),      # a 1x1 map: the mean of one value is the value
                                    (2, 9, 37),      # odd C, less than one block
                                    (6, 16, 512)])   # the clip mean over T = 16 frames
def test_avgpool_vs_f64(N, HW, C):
    """eosv_avgpool_forward sums HW values in order and divides: HW roundings, each at most 2^-24 of the
    running sum of |x|, so |err| <= HW 2^-24 mean|x| per element."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(N * 1000 + HW * 10 + C)
    x = _randn(g, N, HW, C)
    xd, x_p = _dev(x)
    y, y_p = _guarded(N * C)
    _call(lib().eosv_avgpool_forward, x_p, N, HW, C, y_p)
    got = _take(y, N * C).view(N, C).double()
    bound = HW * U * x.abs().mean(1)
    use = float(((got - x.mean(1)).abs() / bound).max())
    print(f"avgpool {(N, HW, C)}: max err / bound = {use:.3f} (bound HW 2^-24 mean|x|)")
    assert use <= 1.0


@pytest.mark.parametrize("N,T,C,scale", [(3, 49, 2048, 1 / 49),  # the average pool's backward at layer4
                                         (2, 16, 512, 1 / 16),   # the clip mean's backward
                                         (4, 1, 5, 1.0),         # T = 1, C below a block
                                         (2, 7, 37, 1 / 7)])     # odd everything
def test_broadcast_rows_vs_f64(N, T, C, scale):
    """dx[(n, t)][c] = dy[n][c] * scale: one rounding (2^-24 relative) of the f64 product with the f32
    scale the ABI carries."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(N * 1000 + T * 10 + C)
    dy = _randn(g, N, C)
    dyd, dy_p = _dev(dy)
    dx, dx_p = _guarded(N * T * C)
    _call(lib().eosv_broadcast_rows, dy_p, N, T, C, scale, dx_p)
    got = _take(dx, N * T * C).view(N, T, C).double()
    ref = (dy[:, None, :] * float(np.float32(scale))).expand(N, T, C)
    err = (got - ref).abs()
    use = float((err / (U * ref.abs()).clamp_min(1e-300)).max())
    print(f"broadcast_rows {(N, T, C)}: max err / bound = {use:.3f} (bound 2^-24 |dx|)")
    assert bool((err <= U * ref.abs()).all())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows,C", [(6, 64),       # the fc bias gradient of the reference batch
                                    (1, 5),        # one row, C below a block
                                    (300, 1000),   # four blocks, the last ragged
                                    (17, 257)])    # one lane in the second block
def test_sum_rows_vs_f64(rows, C, accumulate):
    """y[c] = (accumulate ? y[c] : 0) + sum over rows, in row order: |err| <= rows 2^-24 sum|x| per
    column, the sequential-sum bound over every row summed into y.  accumulate = 0 starts from a y full
    of NaN, which must not be read; accumulate = 1 adds a second block of rows onto that call's result
    (the way a gradient is accumulated), and the bound counts both blocks' rows and values."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(rows * 1000 + C)
    blocks = [_randn(g, rows, C) for _ in range(1 + accumulate)]
    y, y_p = _guarded(C, init=torch.full((C,), float("nan"), dtype=F64))
    for i, xb in enumerate(blocks):
        xd, x_p = _dev(xb)
        _call(lib().eosv_sum_rows, x_p, rows, C, y_p, int(i > 0))
    got = _take(y, C).double()
    x = torch.cat(blocks)
    bound = x.shape[0] * U * x.abs().sum(0)
    use = float(((got - x.sum(0)).abs() / bound).max())
    print(f"sum_rows {(rows, C)} accumulate={accumulate}: max err / bound = {use:.3f} "
          f"(bound rows 2^-24 sum|x| over the {x.shape[0]} rows summed)")
    assert bool(torch.isfinite(got).all()) and use <= 1.0


@pytest.mark.parametrize("rows,C", [(6, 64), (1, 5), (3, 1000)])  # the fc logits; one row; several blocks
def test_add_bias_vs_f64(rows, C):
    """y[r][c] += b[c]: one rounding."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(rows * 1000 + C + 1)
    y0, b = _randn(g, rows, C), _randn(g, C)
    bd, b_p = _dev(b)
    y, y_p = _guarded(rows * C, init=y0)
    _call(lib().eosv_add_bias, y_p, rows, C, b_p)
    got = _take(y, rows * C).view(rows, C).double()
    ref = y0 + b
    err = (got - ref).abs()
    print(f"add_bias {(rows, C)}: max err / bound = {float((err / (U * ref.abs()).clamp_min(1e-300)).max()):.3f} "
          f"(bound 2^-24 |y|)")
    assert bool((err <= U * ref.abs()).all())


@pytest.mark.parametrize("N,C,H,W", [(2, 3, 5, 7),     # the frames' three channels, odd sizes
                                     (1, 3, 96, 96),   # one frame of the small training shape: 108 blocks
                                     (3, 5, 1, 9),     # H = 1
                                     (2, 64, 4, 4)])   # many channels over few pixels
def test_nchw_to_nhwc_bitwise(N, C, H, W):
    from eosv._lib import lib

    g = torch.Generator().manual_seed(N + 10 * C + 100 * H + W)
    x = _randn(g, N, C, H, W).float()
    xd, x_p = _dev(x)
    y, y_p = _guarded(x.numel())
    _call(lib().eosv_nchw_to_nhwc, x_p, N, C, H, W, y_p)
    got = _take(y, x.numel()).view(N, H, W, C)
    same = got.numpy().tobytes() == x.permute(0, 2, 3, 1).contiguous().numpy().tobytes()
    print(f"nchw_to_nhwc {(N, C, H, W)}: bitwise equal = {same} (bound: equality)")
    assert same


@pytest.mark.parametrize("Cout,KH,KW,Cin", [(64, 3, 3, 64),    # layer1's 3x3
                                            (8, 3, 3, 16),     # Cout != Cin: a swapped index shows
                                            (128, 1, 1, 64),   # 1x1: the flip is a transpose
                                            (5, 7, 7, 3)])     # the stem's kernel, odd channel counts
def test_flip_weights_bitwise(Cout, KH, KW, Cin):
    """W[co][kh][kw][ci] -> Wf[ci][KH-1-kh][KW-1-kw][co], until now seen only through the conv fed by it."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(Cout * 100 + KH * 10 + Cin)
    w = _randn(g, Cout, KH, KW, Cin).float()
    wd, w_p = _dev(w)
    wf, wf_p = _guarded(w.numel())
    _call(lib().eosv_flip_weights, w_p, Cout, KH, KW, Cin, wf_p)
    got = _take(wf, w.numel()).view(Cin, KH, KW, Cout)
    same = got.numpy().tobytes() == w.flip(1, 2).permute(3, 1, 2, 0).contiguous().numpy().tobytes()
    print(f"flip_weights {(Cout, KH, KW, Cin)}: bitwise equal = {same} (bound: equality)")
    assert same


ELEMENT_COUNTS = [1, 255, 256, 257, 1000003]  # one lane; around one block; 3907 blocks with a ragged last one


@pytest.mark.parametrize("alpha", [1.0, -0.5])
@pytest.mark.parametrize("n", ELEMENT_COUNTS)
def test_axpy_vs_f64(n, alpha):
    """y += alpha x: a multiply and an add, k = 2 roundings (one if fused), each at most 2^-24 of
    |y| + |alpha x|: |err| <= k 2^-23 (|y| + |alpha x|) holds with room."""
    from eosv._lib import lib

    K_OPS = 2
    g = torch.Generator().manual_seed(n)
    x, y0 = _randn(g, n), _randn(g, n)
    xd, x_p = _dev(x)
    y, y_p = _guarded(n, init=y0)
    _call(lib().eosv_axpy, y_p, x_p, n, alpha)
    got = _take(y, n).double()
    bound = K_OPS * 2.0 ** -23 * (y0.abs() + (alpha * x).abs())
    use = float(((got - (y0 + alpha * x)).abs() / bound).max())
    print(f"axpy n={n} alpha={alpha}: max err / bound = {use:.3f} (bound {K_OPS} 2^-23 (|y| + |alpha x|))")
    assert use <= 1.0


@pytest.mark.parametrize("n", ELEMENT_COUNTS)
def test_sgd_momentum_three_steps_vs_f64(n):
    """Three consecutive eosv_sgd_momentum steps (first = 1, 0, 0; the rate drops at the third, as the
    drop-in's StepLR does; the momentum buffer is NaN before the first step and must not be read)
    against the f64 recurrence of torch.optim.SGD(momentum=0.9): buf = g, then momentum buf + g;
    p -= lr buf, with the f32 lr and momentum the ABI carries.
    Rounding count: a step rounds twice for buf (multiply, add) and twice for p (multiply, subtract),
    k = 4, and an error made in one step is carried into the next with a factor of at most 1, so after
    s steps |err| <= 4 s 2^-23 (|p| + lr |buf|) for p and 2 s 2^-23 (momentum |buf| + |g|) for buf,
    magnitudes taken as the largest over the steps so far."""
    from eosv._lib import lib

    K_P, K_BUF = 4, 2
    g = torch.Generator().manual_seed(n + 7)
    p0 = _randn(g, n)
    grads = [_randn(g, n) for _ in range(3)]
    lrs = [float(np.float32(v)) for v in (1e-2, 1e-2, 1e-3)]
    mom = float(np.float32(0.9))
    p, p_p = _guarded(n, init=p0)
    buf, buf_p = _guarded(n, init=torch.full((n,), float("nan"), dtype=F64))
    p_ref, b_ref = p0.clone(), None
    p_mag, b_mag, t_mag = p0.abs(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    worst = 0.0
    for s, (gr, lr) in enumerate(zip(grads, lrs), 1):
        gd, g_p = _dev(gr)
        _call(lib().eosv_sgd_momentum, p_p, g_p, buf_p, n, lr, mom, int(s == 1))
        t_mag = torch.maximum(t_mag, gr.abs() + (0 if b_ref is None else mom * b_ref.abs()))
        b_ref = gr.clone() if b_ref is None else mom * b_ref + gr
        p_ref = p_ref - lr * b_ref
        p_mag, b_mag = torch.maximum(p_mag, p_ref.abs()), torch.maximum(b_mag, b_ref.abs())
        got_p, got_b = _take(p, n, what="p").double(), _take(buf, n, what="buf").double()
        assert bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(got_b).all())
        use_p = float(((got_p - p_ref).abs() / (K_P * s * 2.0 ** -23 * (p_mag + max(lrs) * b_mag))).max())
        use_b = float(((got_b - b_ref).abs() / (K_BUF * s * 2.0 ** -23 * t_mag)).max())
        print(f"sgd n={n} step {s} lr={lr:.0e}: max err / bound p {use_p:.3f}, buf {use_b:.3f} "
              f"(bounds {K_P} s 2^-23 (|p| + lr |buf|), {K_BUF} s 2^-23 (momentum |buf| + |g|))")
        worst = max(worst, use_p, use_b)
    assert worst <= 1.0


def _xent_labels(B, C, g):
    """Label vectors of a (B, C) case: every class for C = 5; the first, the last and index 256 (the
    first of the strided loop's second trip) for C >= 257; else the first, the last and random ones."""
    if C == 5:
        return [[j] * B for j in range(C)]
    if C >= 257:
        return [[j] * B for j in sorted({0, C - 1, 256})]
    return [[0] * B, [C - 1] * B, torch.randint(0, C, (B,), generator=g).tolist()]


@pytest.mark.parametrize("kind", ["unit", "x30", "edge"])
@pytest.mark.parametrize("B,C", [(1, 5),      # the bad-label test's class count, one clip
                                 (6, 64),     # the reference batch
                                 (3, 257),    # one class in the second trip of the 256-thread loops
                                 (2, 1000)])  # four trips, the last ragged; 256 live values in the LDS trees
def test_softmax_xent_vs_f64(B, C, kind):
    """eosv_softmax_xent's row losses and dlogits against f64 log_softmax and (softmax - onehot) / B,
    by norm within max(4 x torch-f32's own distance on the same f32 logits, 1e-6).  unit: logits ~ N(0, 1);
    x30: 30 times those (without the max subtraction expf overflows); edge: unit plus a row holding a
    +80 / -80 pair and a row of equal logits."""
    from eosv._lib import lib

    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = _randn(g, B, C)
    if kind == "x30":
        logits = (logits * 30).float().double()
    if kind == "edge":
        pair = _randn(g, 1, C)
        pair[0, 0], pair[0, C - 1] = 80.0, -80.0
        logits = torch.cat([logits, pair, torch.full((1, C), 3.5, dtype=F64)])
    R = logits.shape[0]
    ld, l_p = _dev(logits)
    l32 = logits.float()
    for labels in _xent_labels(R, C, g):
        lab = torch.tensor(labels, dtype=torch.long)
        labd, lab_p = _dev(lab, dtype=torch.int32)
        rl, rl_p = _guarded(R)
        dl, dl_p = _guarded(R * C)
        _call(lib().eosv_softmax_xent, l_p, lab_p, R, C, rl_p, dl_p)
        got_l, got_d = _take(rl, R, what="row_loss"), _take(dl, R * C, what="dlogits").view(R, C)
        onehot = torch.nn.functional.one_hot(lab, C)
        ref_l = -torch.log_softmax(logits, 1).gather(1, lab[:, None])[:, 0] / R
        ref_d = (torch.softmax(logits, 1) - onehot) / R
        f32_l = (torch.logsumexp(l32, 1) - l32.gather(1, lab[:, None])[:, 0]) / R
        f32_d = (torch.softmax(l32, 1) - onehot.float()) / R
        for name, got, ref, f32 in (("row_loss", got_l, ref_l, f32_l), ("dlogits", got_d, ref_d, f32_d)):
            err, yard = _rel(got, ref), _rel(f32, ref)
            print(f"softmax_xent {(R, C)} {kind} labels {labels[:3]}: {name} error {err:.2e}, torch-f32 yardstick "
                  f"{yard:.2e}, bound {max(4 * yard, 1e-6):.2e}")
            assert err <= max(4 * yard, 1e-6), (name, err, yard)


# ---------------------------------------------------------------- c. the head composed
@pytest.mark.parametrize("B,T,HW,D,classes", [(1, 1, 1, 64, 5),      # m = 1 logits, k = 1 weight gradient, 1x1 map
                                              (1, 4, 9, 512, 5),     # ResNet-18 width, one clip of 4 frames
                                              (2, 3, 49, 2048, 64),  # ResNet-50 layer4 at 224
                                              (6, 2, 4, 512, 101)])  # the reference batch, odd class count
def test_head_chain_vs_f64_autograd(B, T, HW, D, classes):
    """The calls NativeTrainer.step makes after layer4, in its order -- avgpool, clip mean, fc (eosv_sgemm
    NT), bias, cross-entropy; fc weight gradient (TN), bias gradient (row sum), dF (NN), the two
    broadcasts -- against f64 autograd on one graph: loss 1e-6, fc gradients and the gradient into the
    layer-4 map 1e-5 relative (the bounds of the conv / GEMM unit tests of test_gpu_train.py)."""
    from eosv._lib import lib

    L = lib()
    g = torch.Generator().manual_seed(B * 1000 + T * 100 + HW + D + classes)
    N4 = B * T
    h = torch.relu(_randn(g, N4, HW, D)).requires_grad_()   # a post-ReLU map
    w = _randn(g, classes, D, scale=D ** -0.5).requires_grad_()
    b = _randn(g, classes, scale=0.1).requires_grad_()
    labels = torch.randint(0, classes, (B,), generator=g)
    loss = torch.nn.functional.cross_entropy(h.mean(1).view(B, T, D).mean(1) @ w.T + b, labels)
    loss.backward()

    hd, h_p = _dev(h)
    wd, w_p = _dev(w)
    bd, b_p = _dev(b)
    labd, lab_p = _dev(labels, dtype=torch.int32)
    feat, feat_p = _guarded(N4 * D)
    fm, fm_p = _guarded(B * D)
    logits, logits_p = _guarded(B * classes)
    row_loss, rl_p = _guarded(B)
    dlog, dlog_p = _guarded(B * classes)
    gw, gw_p = _guarded(classes * D)
    gb, gb_p = _guarded(classes)
    dfm, dfm_p = _guarded(B * D)
    dfeat, dfeat_p = _guarded(N4 * D)
    dh, dh_p = _guarded(N4 * HW * D)
    _call(L.eosv_avgpool_forward, h_p, N4, HW, D, feat_p)
    _call(L.eosv_avgpool_forward, feat_p, B, T, D, fm_p)
    _call(L.eosv_sgemm, 0, 1, B, classes, D, 1.0, fm_p, D, w_p, D, 0.0, logits_p, classes)
    _call(L.eosv_add_bias, logits_p, B, classes, b_p)
    _call(L.eosv_softmax_xent, logits_p, lab_p, B, classes, rl_p, dlog_p)
    _call(L.eosv_sgemm, 1, 0, classes, D, B, 1.0, dlog_p, classes, fm_p, D, 0.0, gw_p, D)
    _call(L.eosv_sum_rows, dlog_p, B, classes, gb_p, 0)
    _call(L.eosv_sgemm, 0, 0, B, D, classes, 1.0, dlog_p, classes, w_p, D, 0.0, dfm_p, D)
    _call(L.eosv_broadcast_rows, dfm_p, B, T, D, 1.0 / T, dfeat_p)
    _call(L.eosv_broadcast_rows, dfeat_p, N4, HW, D, 1.0 / HW, dh_p)
    for buf, n, what in ((feat, N4 * D, "feat"), (fm, B * D, "fm"), (logits, B * classes, "logits"),
                         (dlog, B * classes, "dlogits"), (dfm, B * D, "dfm"), (dfeat, N4 * D, "dfeat")):
        _take(buf, n, what=what)
    got_loss = float(_take(row_loss, B, what="row_loss").double().sum())
    ref_loss = float(loss.detach())
    e_loss = abs(got_loss - ref_loss) / abs(ref_loss)
    e_w = _rel(_take(gw, classes * D, what="fc weight gradient"), w.grad)
    e_b = _rel(_take(gb, classes, what="fc bias gradient"), b.grad)
    e_h = _rel(_take(dh, N4 * HW * D, what="dh"), h.grad)
    print(f"head {(B, T, HW, D, classes)}: loss {e_loss:.2e}/1e-06, fc weight gradient {e_w:.2e}/1e-05, "
          f"fc bias gradient {e_b:.2e}/1e-05, layer-4 gradient {e_h:.2e}/1e-05")
    assert e_loss < 1e-6
    assert e_w < 1e-5 and e_b < 1e-5 and e_h < 1e-5


# ---------------------------------------------------------------- d. max pool with ties
@pytest.mark.parametrize("N,C,H,W", [(2, 8, 9, 8),    # four channels per lane
                                     (2, 5, 9, 8),    # the scalar kernels
                                     (1, 64, 7, 5)])  # odd H and W: the last window row / column is cut
def test_maxpool_with_tied_maxima(N, C, H, W):
    """The max pool's real input is ReLU(BN(stem)), about half zeros, where windows of equal maxima are
    common and the choice among them decides where the gradient goes: relu(randn - 0.8) ties at least a
    tenth of the windows.  Pooled values exact, indices torch-CPU's f64 return_indices (the first maximum
    in (kh, kw) order), dx autograd's within 1e-6 absolute."""
    from eosv._lib import lib

    L = lib()
    g = torch.Generator().manual_seed(N * 1000 + C * 100 + H * 10 + W)
    x = torch.relu(_randn(g, N, C, H, W) - 0.8).float().double().requires_grad_()
    y, ref_idx = torch.nn.functional.max_pool2d(x, 3, 2, 1, return_indices=True)
    dy = _randn(g, *y.shape)
    y.backward(dy)
    Ho, Wo = y.shape[2], y.shape[3]
    win = torch.nn.functional.unfold(torch.nn.functional.pad(x.detach(), (1, 1, 1, 1), value=float("-inf")), 3, stride=2)
    win = win.view(N, C, 9, Ho * Wo)
    tied = int(((win == win.max(2, keepdim=True)[0]).sum(2) >= 2).sum())
    total = N * C * Ho * Wo
    assert tied >= 0.1 * total, (tied, total)

    n_out, n_in = N * Ho * Wo * C, N * H * W * C
    xd, x_p = _dev(x.permute(0, 2, 3, 1))
    dyd, dy_p = _dev(dy.permute(0, 2, 3, 1))
    yd, y_p = _guarded(n_out)
    idx, idx_p = _guarded(n_out, torch.int32)
    dx, dx_p = _guarded(n_in)
    _call(L.eosv_maxpool_forward, x_p, N, H, W, C, y_p, idx_p)
    _call(L.eosv_maxpool_backward, dy_p, idx_p, N, H, W, C, dx_p)
    got_y = _take(yd, n_out, what="y").view(N, Ho, Wo, C).permute(0, 3, 1, 2)
    got_i = _take(idx, n_out, what="idx").view(N, Ho, Wo, C).permute(0, 3, 1, 2).long()
    got_dx = _take(dx, n_in, what="dx").view(N, H, W, C).permute(0, 3, 1, 2).double()
    wrong = int((got_i != ref_idx).sum())
    err = float((got_dx - x.grad).abs().max())
    print(f"maxpool {(N, C, H, W)}: {tied} of {total} windows tied; values exact = "
          f"{torch.equal(got_y, y.detach().float())}, {wrong} indices differ (bound 0), "
          f"dx max abs error {err:.2e} (bound 1e-06)")
    assert torch.equal(got_y, y.detach().float())
    assert wrong == 0
    assert err <= 1e-6
