"""The default conv route of the training step, entry by entry against plain torch in f64:
eosv_im2col, eosv_col2im (csrc/train.hip), eosv_conv2d_f32 (launch_conv_f32 of csrc/conv_f32_dma.hip:
row-strip kernel, DMA tiles, warp-specialised tiles, split-K sum) and eosv_conv_wgrad_f32
(csrc/wgrad_f32.hip: six tile shapes, slice sum), at the smallest shapes that reach each path.

Conventions, those of test_gpu_train_kernels.py (whose helpers are imported, not copied):
  * inputs are f64 tensors from a seeded CPU generator holding f32-representable values; the reference
    is plain torch in f64 on the CPU, computed once per shape (lru_cache) and never modified;
  * every output lives in a guarded buffer (4096 sentinel elements on each side, guards bitwise intact,
    no sentinel left inside); every workspace is NaN before the call;
  * maps are never square (H != W, Ho != Wo), so a swapped H / W, Ho / Wo or kh / kw index shows;
  * the path a case claims is asserted: the slice count from the workspace size the library reports,
    `total % 4` of the im2col tail, and, where the library does not report it (the tile of f32_tile,
    conv_rows_f32_ok), from mirrors of those functions fed with the device's CU count; a chip on which a
    case cannot reach its path skips with a message instead of passing on another path.

Per-element bound of every conv, weight-gradient and GEMM-composed case:
    |got - ref| <= (T + S + 3) 2^-23 A
T the number of terms summed per output (K = KH KW Cin, or the pixel count P for the weight gradient),
S the number of split slices, A the same operation on absolute values in f64 (|x| (*) |w| + |bias| +
|res|, or sum_p |x| |dy|): the any-order summation bound gamma_T sum|terms| with unit roundoff 2^-24,
so with a factor 2 of room; ReLU is 1-Lipschitz, so it holds after it.  The norm-relative 1e-5 of
test_gpu_train.py is kept as a second assertion.  test_f32_reference_clears_the_bounds (no GPU) shows
that torch's own f32 CPU results stay within these bounds.

Not covered: the `long long` instantiations of im2col4_kernel / col2im4_kernel (2^31 elements, an 8 GB
buffer) and the grid-stride second trips (more than 2^20 blocks).
"""
import functools
import itertools
import types
import zlib

import pytest
import torch

from test_gpu_train_kernels import GUARD, SENTINEL, _SENT, _call, _dev, _guarded, _rel, _take

gpu = pytest.mark.gpu
F64 = torch.float64
EPS = 2.0 ** -23
ERR_ARG, ERR_UNSUPPORTED = -1, -4  # eosv_status of include/eosv.h
Fn = torch.nn.functional


# ---------------------------------------------------------------- helpers
def _randn(g, *shape):
    """f64 normal values that f32 holds exactly."""
    return torch.randn(*shape, generator=g, dtype=F64).float().double()


def _seed(shape):
    """A generator seed from a case's shape, the same in every interpreter (hash() of a tuple is not)."""
    return zlib.crc32(repr(tuple(shape)).encode())


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _out_hw(H, W, KH, KW, s, p):
    return (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1


def _cdiv(a, b):
    return -(-a // b)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nan_ws(nfloats):
    """A NaN-filled workspace of at least nfloats floats (16-byte aligned)."""
    return torch.full((max(int(nfloats), 16) + 8,), float("nan"), dtype=torch.float32, device="cuda")


def _untouched(buf, what):
    """A guarded buffer no element of which was written."""
    torch.cuda.synchronize()
    h = buf.cpu()
    ref = torch.full((1,), _SENT[h.dtype], dtype=h.dtype)
    assert bool((h.view(torch.int32) == ref.view(torch.int32)).all()), f"{what}: written by a refused call"


def _take_near(buf, n, ref, bound, what):
    """_take for outputs among which the sentinel's value can be a correct result (millions of random
    sums: some references lie within their bound of it, and the kernel may round to exactly it).  A
    slot holding the sentinel passes only where the reference is within the bound of the sentinel, and
    is then read as the reference (the bound holds there by that very check); anywhere else it is a
    slot that was not written, as in _take."""
    torch.cuda.synchronize()
    inner = buf[GUARD:GUARD + n]
    hit = (inner == SENTINEL).nonzero().flatten().cpu()
    if hit.numel():
        r, b = ref.reshape(-1)[hit], bound.reshape(-1)[hit]
        assert bool(((r - SENTINEL).abs() <= b).all()), f"{what}: a slot was not written"
        print(f"{what}: {hit.numel()} of {n} results equal the sentinel's value, each within the bound of its reference")
        inner[hit.cuda()] = r.float().cuda()
    return _take(buf, n, what=what)


def _refused(fn, args, status, names, outs, works):
    """fn(*args) returns `status` with a message holding every string of `names`, and writes nothing."""
    from eosv._lib import lib, stream_ptr

    rc = fn(*args, stream_ptr())
    msg = lib().eosv_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    assert rc == status, (rc, msg)
    for n in names:
        assert n in msg, (n, msg)
    for what, buf in outs:
        _untouched(buf, what)
    for w in works:
        assert bool(torch.isnan(w).all()), "workspace written by a refused call"
    return msg


def _check(tag, got, ref, A, T, S, note=""):
    """The per-element bound (T + S + 3) 2^-23 A and the norm-relative 1e-5; prints the measured use."""
    got = got.double().reshape(-1)
    ref, A = ref.reshape(-1), A.reshape(-1)
    bound = (T + S + 3) * EPS * A
    err = (got - ref).abs()
    use = float((err / bound.clamp_min(1e-300)).max())
    rel = _rel(got, ref)
    print(f"{tag}: max err / bound = {use:.4f} (bound ({T} + {S} + 3) 2^-23 A), norm-relative {rel:.2e}/1e-05{note}")
    assert bool(torch.isfinite(got).all()), tag
    assert bool((err <= bound).all()), (tag, use)
    assert rel < 1e-5, (tag, rel)
    return use


# ---------------------------------------------------------------- a. / b. im2col, col2im
# (N, H, W, C, KH, KW, stride, pad): the path only this shape reaches
GATHER_SHAPES = [
    (1, 5, 5, 3, 7, 7, 2, 3),    # the stem's kernel, P = 9: total % 4 == 3, the im2col4 tail stores three
    (2, 5, 5, 3, 7, 7, 2, 3),    # P = 18: total % 4 == 2
    (1, 6, 9, 3, 7, 7, 2, 3),    # P = 15, non-square: total % 4 == 1
    (2, 5, 7, 8, 3, 3, 1, 1),    # 3x3 s1: every quad inside one tap (C % 4 == 0), col2im4
    (2, 6, 9, 8, 3, 3, 2, 1),    # 3x3 s2, even sizes: the last window is cut by the padding
    (2, 7, 10, 8, 3, 3, 2, 1),   # 3x3 s2, odd H: the last window fits
    (2, 5, 7, 16, 1, 1, 2, 0),   # 1x1 s2: the downsample gather; col2im writes zeros where no window reads
    (2, 4, 6, 8, 1, 3, 1, 1),    # KH != KW (the ABI takes one; the trainer never asks): Ho = 6 > H
]
TAIL = {GATHER_SHAPES[0]: 3, GATHER_SHAPES[1]: 2, GATHER_SHAPES[2]: 1}


def _im2col_ref(x, KH, KW, s, p):
    """col[n][oh][ow][kh][kw][c] = x[n][oh s - p + kh][ow s - p + kw][c] or 0, by indexing (x is NHWC)."""
    N, H, W, C = x.shape
    Ho, Wo = _out_hw(H, W, KH, KW, s, p)
    xp = torch.zeros(N, H + 2 * p, W + 2 * p, C, dtype=x.dtype)
    xp[:, p:p + H, p:p + W] = x
    col = torch.empty(N, Ho, Wo, KH, KW, C, dtype=x.dtype)
    for kh in range(KH):
        for kw in range(KW):
            col[:, :, :, kh, kw] = xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]
    return col


@gpu
@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_im2col_bitwise(shape):
    """eosv_im2col against the gather by indexing, bitwise (a gather rounds nothing), once with d_col
    16-byte aligned (im2col4_kernel: four elements per lane, the last lane's tail) and once 4 bytes off
    (im2col_kernel, one element per lane); the two results bitwise equal."""
    from eosv._lib import lib

    N, H, W, C, KH, KW, s, p = shape
    g = torch.Generator().manual_seed(_seed(shape))
    x = _randn(g, N, H, W, C).float()
    ref = _im2col_ref(x, KH, KW, s, p)
    total = ref.numel()
    if shape in TAIL:
        assert total % 4 == TAIL[shape], (total, "the im2col4 tail this case is here for")
    xd, x_p = _dev(x)
    outs = []
    for off in (0, 1):
        col, col_p = _guarded(total, off=off)
        _call(lib().eosv_im2col, x_p, N, H, W, C, KH, KW, s, p, col_p)
        outs.append(_take(col, total, off, "col").numpy().tobytes())
    same = [o == ref.numpy().tobytes() for o in outs]
    print(f"im2col {shape}: total % 4 = {total % 4}; bitwise equal aligned = {same[0]}, 4 bytes off = {same[1]} "
          f"(bound: equality)")
    assert all(same) and outs[0] == outs[1]


@functools.lru_cache(maxsize=None)
def _col2im_case(shape):
    """col, and in f64 the adjoint of the gather (fold), the same of |col|, and the tap count per pixel."""
    N, H, W, C, KH, KW, s, p = shape
    Ho, Wo = _out_hw(H, W, KH, KW, s, p)
    g = torch.Generator().manual_seed(_seed(shape) + 1)
    col = _randn(g, N, Ho, Wo, KH, KW, C)

    def fold(c):  # [N][Ho][Wo][KH][KW][C] -> fold's [N][C KH KW][Ho Wo] -> NHWC
        c = c.permute(0, 5, 3, 4, 1, 2).reshape(N, C * KH * KW, Ho * Wo)
        return _nhwc(Fn.fold(c, (H, W), (KH, KW), padding=p, stride=s))

    return types.SimpleNamespace(col=col, ref=fold(col), A=fold(col.abs()), taps=fold(torch.ones_like(col)), fold=fold)


def _col2im_check(tag, got, cs):
    bound = cs.taps * EPS * cs.A
    err = (got.double().view_as(cs.ref) - cs.ref).abs()
    use = float((err / bound.clamp_min(1e-300)).max())
    print(f"{tag}: max err / bound = {use:.3f} (bound taps 2^-23 sum|col|, taps <= {int(cs.taps.max())}), "
          f"pixels no window reads {int((cs.taps == 0).sum())}")
    assert bool((err <= bound).all()), (tag, use)
    return use


@gpu
@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_col2im_vs_f64(shape):
    """eosv_col2im against fold in f64, |err| <= taps 2^-23 sum|col| per element (taps: the (kh, kw)
    pairs that read the pixel; a pixel no window reads has bound 0 and must be written as 0, which the
    sentinel check of _take proves).  Three calls: every operand aligned (col2im4_kernel when
    C % 4 == 0, col2im_kernel at C = 3), d_x 4 bytes off and d_col 4 bytes off (col2im_kernel): same
    taps in the same order, so bitwise equal."""
    from eosv._lib import lib

    N, H, W, C, KH, KW, s, p = shape
    cs = _col2im_case(shape)
    n = N * H * W * C
    outs = []
    for xo, co in ((0, 0), (1, 0), (0, 1)):
        cd, col_p = _dev(cs.col, co)
        dx, dx_p = _guarded(n, off=xo)
        _call(lib().eosv_col2im, col_p, N, H, W, C, KH, KW, s, p, dx_p)
        got = _take(dx, n, xo, "dx")
        _col2im_check(f"col2im {shape} d_x+{4 * xo} d_col+{4 * co}", got, cs)
        outs.append(got.numpy().tobytes())
    assert outs[0] == outs[1] == outs[2], "the float4 and the scalar kernel differ"
    if s > 1 and KH == 1:
        assert int((cs.taps == 0).sum()) > 0


# ---------------------------------------------------------------- c. eosv_conv2d_f32
# mirrors of conv_f32_dma.hip's f32_tile / ksplit_count / launch_conv_f32 and conv_rows_f32_ok, for the
# choices the library does not report
_BM, _BN = {1: 256, 2: 128, 3: 128}, {1: 128, 2: 128, 3: 64}


def _tile(M, Cout, cus):
    if Cout <= 256 and _cdiv(M, 256) * _cdiv(Cout, 128) >= cus:
        return 1
    return 2 if _cdiv(M, 128) * _cdiv(Cout, 128) >= cus else 3


def _ks_mirror(M, Cout, K, cus):
    t = _tile(M, Cout, cus)
    blocks = _cdiv(M, _BM[t]) * _cdiv(Cout, _BN[t])
    return max(1, min(_cdiv(2 * cus, blocks), K // 16 // 32, 8))


def _path(shape, res, ws, cus):
    """The kernel launch_conv_f32 picks: rows | elem (128x64, per-element epilogue) | dma256x64 |
    ws1 / ws2 (warp-specialised 256x128 / 128x128) | dma1 / dma2 / dma3 (256x128 / 128x128 / 128x64)."""
    N, H, W, Cin, Cout, k, s, p = shape
    Ho, Wo = _out_hw(H, W, k, k, s, p)
    if Cin == 64 and Cout == 64 and k == 3 and s == 1 and p == 1 and (W == 56 or (W == 64 and not res)) and H % 2 == 0:
        return "rows"
    if Cout % 4:
        return "elem"
    if Cout <= 64:
        return "dma256x64"
    t = _tile(N * Ho * Wo, Cout, cus)
    return f"ws{t}" if not ws and t < 3 else f"dma{t}"


@functools.lru_cache(maxsize=4)
def _conv_case(shape):
    """Inputs (NCHW / OIHW f64), a bias of distinct values per channel, a residual, and in f64 the
    conv without epilogue and the conv of absolute values, as [M][Cout] rows (NHWC)."""
    N, H, W, Cin, Cout, k, s, p = shape
    g = torch.Generator().manual_seed(_seed(shape))
    cs = types.SimpleNamespace()
    cs.x, cs.w = _randn(g, N, Cin, H, W), _randn(g, Cout, Cin, k, k)
    cs.lin = _nhwc(Fn.conv2d(cs.x, cs.w, stride=s, padding=p)).reshape(-1, Cout)
    cs.A = _nhwc(Fn.conv2d(cs.x.abs(), cs.w.abs(), stride=s, padding=p)).reshape(-1, Cout)
    scale = float(cs.lin.std())  # about half of the pre-activations stay negative with bias and residual
    b = _randn(g, Cout) * scale
    cs.bias = (b - b.mean()).float().double()  # zero mean over the channels, also where there are five
    cs.res = (_randn(g, *cs.lin.shape) * scale).float().double()
    cs.M = cs.lin.shape[0]
    return cs


def _conv_ref(cs, bias, res, relu):
    pre = cs.lin + (cs.bias if bias else 0) + (cs.res if res else 0)
    A = cs.A + (cs.bias.abs() if bias else 0) + (cs.res.abs() if res else 0)
    return (pre.clamp_min(0) if relu else pre), A, pre


def _conv_run(shape, bias, res, relu, ws):
    """One eosv_conv2d_f32 call.  ws: "none" | "full" (the bytes the library asks for, or a token 64
    where it asks for none) | "short" (one float less) | "offset" (the pointer 4 bytes off).
    Returns the output rows, the slice count used, and checks the NaN workspace."""
    from eosv._lib import lib

    L = lib()
    N, H, W, Cin, Cout, k, s, p = shape
    cs = _conv_case(shape)
    xd, x_p = _dev(_nhwc(cs.x))
    wd, w_p = _dev(_nhwc(cs.w))
    bd, b_p = _dev(cs.bias) if bias else (None, None)
    rd, r_p = _dev(cs.res) if res else (None, None)
    y, y_p = _guarded(cs.M * Cout)
    need = int(L.eosv_conv2d_f32_workspace(N, H, W, Cin, Cout, k, k, s, p))
    assert need % (cs.M * Cout * 4) == 0
    ks = need // (cs.M * Cout * 4) if need else 1
    work = _nan_ws(need // 4)
    wp, wb = {"none": (None, 0), "full": (work.data_ptr(), need or 64), "short": (work.data_ptr(), need - 4),
              "offset": (work.data_ptr() + 4, need)}[ws]
    _call(L.eosv_conv2d_f32, x_p, N, H, W, Cin, w_p, Cout, k, k, s, p, b_p, r_p, int(relu), y_p, wp, wb)
    used = ks if ws == "full" else 1
    ref, A, _ = _conv_ref(cs, bias, res, relu)
    got = _take_near(y, cs.M * Cout, ref, (k * k * Cin + used + 3) * EPS * A, "y").view(cs.M, Cout)
    written = used * cs.M * Cout if used > 1 else 0
    assert bool(torch.isfinite(work[:written]).all()), "a slice of the workspace was not written"
    assert bool(torch.isnan(work[written:]).all()), "the workspace was written past the slices"
    return got, used, ks


def _big(cus, per_cu, Cout):
    """1x1 conv Cin = 32 over N maps of 31 x 65 with M >= per_cu * CUs rows (ragged against 128 / 256)."""
    return (_cdiv(per_cu * cus, 31 * 65), 31, 65, 32, Cout, 1, 1, 0)


# name: (shape or a function of the CU count, residual, workspace, the path asserted)
CONV_PATHS = {
    # conv_rows_f32_ok: Cin = Cout = 64, 3x3 s1 p1, H % 2 == 0, W == 56 or (W == 64 and no residual)
    "rows-one-strip": ((1, 2, 56, 64, 64, 3, 1, 1), False, "none", "rows"),          # one strip, one workgroup
    "rows56-res": ((2, 6, 56, 64, 64, 3, 1, 1), True, "none", "rows"),               # six strips, residual DMA
    "rows64": ((1, 4, 64, 64, 64, 3, 1, 1), False, "none", "rows"),                  # the 64-wide instance
    "rows64-res-falls-to-dma": ((1, 4, 64, 64, 64, 3, 1, 1), True, "none", "dma256x64"),  # LDS too small: not ok
    # Cout <= 64: the 256x64 DMA tile, M = 3 * 5 * 7 = 105 ragged against 256
    "dma256x64-cout64": ((3, 9, 13, 32, 64, 3, 2, 1), False, "none", "dma256x64"),
    "dma256x64-cout32": ((3, 9, 13, 32, 32, 3, 2, 1), False, "none", "dma256x64"),   # half of the N tile is past Cout
    # Cout % 4 != 0: rows not 16-byte aligned, 128x64 tile with the per-element epilogue (EPI = false)
    "elem-cout5": ((2, 3, 5, 64, 5, 1, 1, 0), False, "none", "elem"),
    "elem-cout101": ((2, 3, 5, 64, 101, 1, 1, 0), False, "none", "elem"),            # two N tiles, the last ragged
    # tile 3 (128x64): the grid is below the CU count; Cout = 96 leaves the second N tile half empty
    "tile3-cout96": ((1, 5, 7, 32, 96, 3, 1, 1), False, "none", "dma3"),
    "tile3-cout96-ws": ((1, 5, 7, 32, 96, 3, 1, 1), False, "full", "dma3"),          # K = 288: 18 k-steps, no split
    # tile 2 (128x128): Cout = 512 > 256 and ceil(M / 128) * 4 >= CUs
    "tile2-ws-kernel": (lambda cus: _big(cus, 32, 512), False, "none", "ws2"),       # launch_ws<128, 128>
    "tile2-dma": (lambda cus: _big(cus, 32, 512), False, "full", "dma2"),            # a workspace: launch_dma
    # tile 1 (256x128): Cout = 256 and ceil(M / 256) * 2 >= CUs
    "tile1-ws-kernel": (lambda cus: _big(cus, 128, 256), False, "none", "ws1"),      # launch_ws<256, 128>
    "tile1-dma": (lambda cus: _big(cus, 128, 256), False, "full", "dma1"),
}


@gpu
@pytest.mark.parametrize("name", list(CONV_PATHS))
def test_conv2d_path_vs_f64(name):
    """eosv_conv2d_f32 without bias and ReLU on each kernel launch_conv_f32 can pick (CONV_PATHS), the
    pick asserted from the mirror of its conditions; these shapes never split K (asserted)."""
    shape, res, ws, path = CONV_PATHS[name]
    cus = _cus()
    if callable(shape):
        shape = shape(cus)
    if _path(shape, res, ws != "none", cus) != path:
        pytest.skip(f"{name}: {cus} CUs send {shape} to {_path(shape, res, ws != 'none', cus)}, not {path}")
    N, H, W, Cin, Cout, k, s, p = shape
    Ho, Wo = _out_hw(H, W, k, k, s, p)
    assert H != W and Ho != Wo
    got, used, ks = _conv_run(shape, False, res, False, ws)
    assert ks == 1 and used == 1, (ks, used)
    ref, A, _ = _conv_ref(_conv_case(shape), False, res, False)
    _check(f"conv2d {name} {shape} path {path} ks = {ks}", got, ref, A, k * k * Cin, 1)


# (shape, the slice count claimed): M = 35 rows on the 128x64 tile, Cout / 64 blocks;
# slices = min(ceil(2 CUs / blocks), K / 16 / 32, 8)
SPLITK = {
    "ks2": ((1, 5, 7, 128, 256, 3, 1, 1), 2),   # K = 1152: 72 k-steps
    "ks4": ((1, 5, 7, 256, 128, 3, 1, 1), 4),   # K = 2304: 144 k-steps
    "ks8": ((1, 5, 7, 512, 128, 3, 1, 1), 8),   # K = 4608: 288 k-steps, capped at 8
}


def _splitk_shape(name):
    shape, claimed = SPLITK[name]
    N, H, W, Cin, Cout, k, s, p = shape
    mirror = _ks_mirror(N * H * W, Cout, k * k * Cin, _cus())
    if mirror != claimed:
        pytest.skip(f"{name}: {_cus()} CUs give {mirror} slices, not {claimed}")
    return shape, claimed


@gpu
@pytest.mark.parametrize("name", list(SPLITK))
def test_conv2d_splitk_vs_f64(name):
    """The split-K launch (raw partials per slice, ksplit_sum_kernel) at 2, 4 and 8 slices, the count
    read from eosv_conv2d_f32_workspace and asserted; every slice of the NaN workspace written, nothing
    past them.  S of the bound is the slice count."""
    shape, claimed = _splitk_shape(name)
    got, used, ks = _conv_run(shape, False, False, False, "full")
    assert ks == claimed and used == claimed, (ks, used, claimed)
    cs = _conv_case(shape)
    ref, A, _ = _conv_ref(cs, False, False, False)
    _check(f"conv2d split-K {name} {shape} ks = {ks}", got, ref, A, shape[5] ** 2 * shape[3], ks)


@gpu
@pytest.mark.parametrize("ws", ["short", "offset", "none"])
def test_conv2d_splitk_fallback(ws):
    """The 8-slice case with work_bytes one float short of the need (launch_dma falls back to one
    slice), with the workspace pointer 4 bytes off a 16-byte boundary (the entry ignores it) and with
    none: the result is right on one slice and the NaN workspace is untouched (checked in _conv_run)."""
    shape, claimed = _splitk_shape("ks8")
    got, used, ks = _conv_run(shape, True, True, True, ws)
    assert ks == claimed and used == 1
    ref, A, _ = _conv_ref(_conv_case(shape), True, True, True)
    _check(f"conv2d split-K fallback ({ws}) {shape} ks asked {ks}, used {used}", got, ref, A, shape[5] ** 2 * shape[3], 1)


# one case per kernel family: its in-kernel (or slice-sum) epilogue with every argument combination
EPILOGUE = {
    "rows": ("rows56-res", None),
    "dma": ("dma256x64-cout64", None),
    "ws": ("tile2-ws-kernel", None),
    "elem": ("elem-cout5", None),
    "ksum": (None, "ks2"),
}


@gpu
@pytest.mark.parametrize("bias,res,relu", list(itertools.product((False, True), repeat=3)),
                         ids=lambda v: "FT"[v])
@pytest.mark.parametrize("family", list(EPILOGUE))
def test_conv2d_epilogue_vs_f64(family, bias, res, relu):
    """y = relu(conv + bias + res) for every combination of the three, on the row kernel's register
    epilogue, the LDS-staged one of the DMA and the warp-specialised tiles, the per-element one
    (Cout % 4 != 0) and ksplit_sum_kernel's, whose bias index `i % C4` had never run: the bias holds
    distinct values per channel, and bias and residual are scaled like the conv so that about half of
    the pre-activations are negative (asserted between 0.3 and 0.7 where ReLU is on)."""
    cus = _cus()
    pname, sname = EPILOGUE[family]
    if sname:
        shape, claimed = _splitk_shape(sname)
        ws, path = "full", "dma3"
    else:
        shape, _, ws, path = CONV_PATHS[pname]
        shape = shape(cus) if callable(shape) else shape
        claimed = 1
    if _path(shape, res, ws != "none", cus) != path:
        pytest.skip(f"{family}: {cus} CUs send {shape} to another kernel than {path}")
    got, used, ks = _conv_run(shape, bias, res, relu, ws)
    assert used == claimed, (used, claimed)
    ref, A, pre = _conv_ref(_conv_case(shape), bias, res, relu)
    neg = float((pre < 0).double().mean())
    if relu:
        assert 0.3 < neg < 0.7, neg
    _check(f"conv2d epilogue {family} {shape} bias={int(bias)} res={int(res)} relu={int(relu)} ks = {used}", got, ref,
           A, shape[5] ** 2 * shape[3], used, f", negative pre-activations {neg:.2f}")


@gpu
def test_flipped_dgrad_nonsquare_vs_f64():
    """The trainer's stride-1 input gradient at a non-square map: eosv_flip_weights, then
    eosv_conv2d_f32 of dy with the flipped weights and the shortcut's gradient as residual, against
    autograd's x.grad + skip (Cin = 64, Cout = 128, 3x3 on 6 x 10; the conv runs 128 -> 64 channels on
    the 256x64 DMA tile).  A: the same gradient of absolute values + |skip|; T = 9 * 128 terms."""
    from eosv._lib import lib

    L = lib()
    N, H, W, Cin, Cout, k = 2, 6, 10, 64, 128, 3
    g = torch.Generator().manual_seed(610)
    x = _randn(g, N, Cin, H, W).requires_grad_()
    w, dy, skip = _randn(g, Cout, Cin, k, k), _randn(g, N, Cout, H, W), _randn(g, N, H, W, Cin)
    Fn.conv2d(x, w, padding=1).backward(dy)
    xa = x.detach().abs().requires_grad_()
    Fn.conv2d(xa, w.abs(), padding=1).backward(dy.abs())
    ref, A = _nhwc(x.grad) + skip, _nhwc(xa.grad) + skip.abs()
    wd, w_p = _dev(_nhwc(w))
    dyd, dy_p = _dev(_nhwc(dy))
    sd, s_p = _dev(skip)
    wf, wf_p = _guarded(w.numel())
    _call(L.eosv_flip_weights, w_p, Cout, k, k, Cin, wf_p)
    _take(wf, w.numel(), what="flipped weights")
    assert int(L.eosv_conv2d_f32_workspace(N, H, W, Cout, Cin, k, k, 1, 1)) == 0
    dx, dx_p = _guarded(N * H * W * Cin)
    _call(L.eosv_conv2d_f32, dy_p, N, H, W, Cout, wf_p, Cin, k, k, 1, 1, None, s_p, 0, dx_p, None, 0)
    _check(f"flipped dgrad {(N, H, W, Cin, Cout, k)} path dma256x64 ks = 1", _take(dx, N * H * W * Cin, what="dx"),
           ref, A, k * k * Cout, 1)


# ---------------------------------------------------------------- e. operand alignment of eosv_conv2d_f32
@gpu
@pytest.mark.parametrize("operand", ["d_x", "d_w", "d_y", "d_res", "d_bias"])
def test_conv2d_misaligned_operand_is_refused(operand):
    """No kernel behind eosv_conv2d_f32 has a path for an operand off a 16-byte boundary: x and w are
    read by 16-byte LDS-DMA pieces and float4 loads, and with Cout % 4 == 0 every epilogue stores y
    and loads the residual in float4s, the row kernel and the split-K sum the bias too.  The entry
    checked none of them (eosv_conv_wgrad_f32 and the BN entries do); it now returns
    EOSV_ERR_UNSUPPORTED naming the operand before any launch.  Only the refusal runs here: nothing
    written to y or the workspace."""
    from eosv._lib import lib

    L = lib()
    N, H, W, Cin, Cout, k = 1, 5, 7, 128, 256, 3   # the ks = 2 shape: the workspace would be used
    off = {n: int(n == operand) for n in ("d_x", "d_w", "d_y", "d_res", "d_bias")}
    M = N * H * W
    xd, x_p = _dev(torch.zeros(M * Cin), off["d_x"])
    wd, w_p = _dev(torch.zeros(Cout * k * k * Cin), off["d_w"])
    rd, r_p = _dev(torch.zeros(M * Cout), off["d_res"])
    bd, b_p = _dev(torch.zeros(Cout), off["d_bias"])
    y, y_p = _guarded(M * Cout, off=off["d_y"])
    need = int(L.eosv_conv2d_f32_workspace(N, H, W, Cin, Cout, k, k, 1, 1))
    work = _nan_ws(need // 4)
    msg = _refused(L.eosv_conv2d_f32, (x_p, N, H, W, Cin, w_p, Cout, k, k, 1, 1, b_p, r_p, 1, y_p, work.data_ptr(), need),
                   ERR_UNSUPPORTED, ("eosv_conv2d_f32", operand, "16-byte"), [("y", y)], [work])
    print(f"conv2d {operand} + 4 bytes: refused, \"{msg}\"")


# ---------------------------------------------------------------- d. eosv_conv_wgrad_f32
def _wgrad_plan(Cout, K, P, cus):
    """wgrad_f32.hip's wgrad_plan: (waves along Cout, waves along K), slices, rows per slice."""
    wm, wn = next(c for c in ((2, 2), (1, 4), (1, 3), (2, 1), (1, 2), (1, 1)) if Cout % (64 * c[0]) == 0 and K % (64 * c[1]) == 0)
    tiles = (Cout // (64 * wm)) * (K // (64 * wn))
    s = max(1, min(_cdiv(4 * cus, tiles), P // 256))
    rows = _cdiv(_cdiv(P, s), 16) * 16
    return (wm, wn), _cdiv(P, rows), rows


# (Cin, Cout, k): the smallest (Cout, K) that selects the tile
WGRAD_TILES = {
    (2, 2): (128, 128, 1),   # Cout 128, K 128
    (1, 4): (256, 64, 1),    # Cout 64, K 256
    (1, 3): (64, 64, 3),     # Cout 64, K 576 = 3 * 192: the only 3x3 among the smallest
    (2, 1): (64, 128, 1),    # Cout 128, K 64
    (1, 2): (128, 64, 1),    # Cout 64, K 128
    (1, 1): (64, 64, 1),     # Cout 64, K 64
}
# (N, H, W, stride): the path
WGRAD_SETTINGS = {
    "one-slice": (1, 9, 13, 1),    # P = 117 < 256: one slice straight into d_dw, the last step 5 of 16 pixels
    "sliced": (2, 19, 23, 1),      # P = 874: three slices of 304 rows, the last 266 = 16 * 16 + 10
    "stride2": (2, 17, 23, 2),     # stride 2 on odd H x W (3x3: pad 1, the first and last taps cut), P = 2 * 9 * 12 = 216
}


@functools.lru_cache(maxsize=4)
def _wgrad_case(Cin, Cout, k, N, H, W, s):
    p = k // 2
    g = torch.Generator().manual_seed(Cin * 1000 + Cout * 10 + k + N * H * W + s)
    x = _randn(g, N, Cin, H, W)
    w = torch.zeros(Cout, Cin, k, k, dtype=F64, requires_grad=True)
    y = Fn.conv2d(x, w, stride=s, padding=p)
    dy = _randn(g, *y.shape)
    ref, = torch.autograd.grad(y, w, dy)
    A, = torch.autograd.grad(Fn.conv2d(x.abs(), w, stride=s, padding=p), w, dy.abs())
    return types.SimpleNamespace(x=x, dy=dy, ref=_nhwc(ref), A=_nhwc(A), P=N * y.shape[2] * y.shape[3],
                                 Ho=y.shape[2], Wo=y.shape[3])


@gpu
@pytest.mark.parametrize("setting", list(WGRAD_SETTINGS))
@pytest.mark.parametrize("tile", list(WGRAD_TILES), ids=lambda t: f"{t[0]}x{t[1]}")
def test_wgrad_tile_vs_f64(tile, setting):
    """eosv_conv_wgrad_f32 on each of wgrad_plan's six tile shapes (asserted from the mirror of its
    selection) against autograd in f64, T = P pixels, S = the slice count read from the workspace size
    (asserted equal to the mirror's, > 1 with a ragged last slice in "sliced", 1 otherwise, where the
    NaN workspace stays untouched)."""
    from eosv._lib import lib

    L = lib()
    Cin, Cout, k = WGRAD_TILES[tile]
    N, H, W, s = WGRAD_SETTINGS[setting]
    p, K = k // 2, k * k * Cin
    cs = _wgrad_case(Cin, Cout, k, N, H, W, s)
    assert H != W and cs.Ho != cs.Wo
    need = int(L.eosv_conv_wgrad_f32_workspace(N, H, W, Cin, Cout, k, k, s, p))
    assert need % (Cout * K * 4) == 0
    slices = need // (Cout * K * 4) if need else 1
    mt, ms, rows = _wgrad_plan(Cout, K, cs.P, _cus())
    assert mt == tile and ms == slices, (mt, ms, slices)
    if setting == "sliced":
        if slices < 2:
            pytest.skip(f"{_cus()} CUs give one slice")
        assert (cs.P - (slices - 1) * rows) % 16 != 0, "the last slice is not ragged"
    else:
        assert slices == 1 and cs.P < 256 and cs.P % 16 != 0
    xd, x_p = _dev(_nhwc(cs.x))
    dyd, dy_p = _dev(_nhwc(cs.dy))
    dw, dw_p = _guarded(Cout * K)
    work = _nan_ws(need // 4)
    _call(L.eosv_conv_wgrad_f32, x_p, N, H, W, Cin, dy_p, Cout, k, k, s, p, dw_p, work.data_ptr(), need)
    got = _take(dw, Cout * K, what="dw")
    written = need // 4
    assert bool(torch.isfinite(work[:written]).all()) and bool(torch.isnan(work[written:]).all())
    _check(f"wgrad <{tile[0]},{tile[1]}> {setting} Cin={Cin} Cout={Cout} {k}x{k} s{s} on {N}x{H}x{W}: P = {cs.P}, "
           f"slices = {slices} of {rows} rows", got, cs.ref, cs.A, cs.P, slices)


@gpu
@pytest.mark.parametrize("what", ["Cin%4", "d_x", "d_dy", "d_dw", "short-workspace"])
def test_wgrad_refusals(what):
    """Cin % 4 != 0 and an operand 4 bytes off a 16-byte boundary: EOSV_ERR_UNSUPPORTED; a workspace
    one float short of the need: EOSV_ERR_ARG; each before any launch, d_dw and the workspace untouched."""
    from eosv._lib import lib

    L = lib()
    N, H, W, Cout, k = 2, 19, 23, 64, 1
    Cin = 62 if what == "Cin%4" else 64
    off = {n: int(n == what) for n in ("d_x", "d_dy", "d_dw")}
    P, K = N * H * W, k * k * Cin
    xd, x_p = _dev(torch.zeros(P * Cin), off["d_x"])
    dyd, dy_p = _dev(torch.zeros(P * Cout), off["d_dy"])
    dw, dw_p = _guarded(Cout * K, off=off["d_dw"])
    need = int(L.eosv_conv_wgrad_f32_workspace(N, H, W, 64, Cout, k, k, 1, 0))
    assert need > 0
    work = _nan_ws(need // 4)
    short = what == "short-workspace"
    msg = _refused(L.eosv_conv_wgrad_f32,
                   (x_p, N, H, W, Cin, dy_p, Cout, k, k, 1, 0, dw_p, work.data_ptr(), need - 4 * short),
                   ERR_ARG if short else ERR_UNSUPPORTED, ("eosv_conv_wgrad_f32",), [("dw", dw)], [work])
    print(f"wgrad {what}: refused, \"{msg}\"")


# ---------------------------------------------------------------- the reference alone clears the bounds (no GPU)
def test_f32_reference_clears_the_bounds():
    """torch's own f32 CPU results on the two smallest cases of each group stay within the bounds the
    GPU tests use against the same f64 references (S = 1): the bounds are not tighter than f32
    arithmetic allows, whatever the summation order of the CPU kernels."""
    for shape in (GATHER_SHAPES[0], GATHER_SHAPES[3]):
        cs = _col2im_case(shape)
        _col2im_check(f"torch f32 fold {shape}", cs.fold(cs.col.float()), cs)
    for name in ("elem-cout5", "tile3-cout96"):
        shape = CONV_PATHS[name][0]
        N, H, W, Cin, Cout, k, s, p = shape
        cs = _conv_case(shape)
        for bias, res, relu in ((False, False, False), (True, True, True)):
            y = Fn.conv2d(cs.x.float(), cs.w.float(), cs.bias.float() if bias else None, stride=s, padding=p)
            y = _nhwc(y).reshape(-1, Cout) + (cs.res.float() if res else 0)
            ref, A, _ = _conv_ref(cs, bias, res, relu)
            _check(f"torch f32 conv2d {shape} bias={int(bias)} res={int(res)} relu={int(relu)}",
                   y.clamp_min(0) if relu else y, ref, A, k * k * Cin, 1)
    for tile in ((1, 1), (2, 1)):
        Cin, Cout, k = WGRAD_TILES[tile]
        N, H, W, s = WGRAD_SETTINGS["one-slice"]
        cs = _wgrad_case(Cin, Cout, k, N, H, W, s)
        w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
        got, = torch.autograd.grad(Fn.conv2d(cs.x.float(), w, stride=s, padding=k // 2), w, cs.dy.float())
        _check(f"torch f32 weight gradient Cin={Cin} Cout={Cout} {k}x{k} P = {cs.P}", _nhwc(got), cs.ref, cs.A, cs.P, 1)
