"""conv_wino_f32_kernel (csrc/conv_wino_f32.hip) with the column stage of the output transform in
registers: wave w owns the position column q = w >> 1 (positions 4 p + q) and the output-channel
half j = w & 1, forms S = A^T M on its own accumulators and sends 8 values per (tile, channel)
through LDS instead of 16.

Bitwise against the parent on non-integer data.  tests/test_gpu_wino_exact.py cannot see a changed
association in the transform (integers add exactly in any order); here x, bias and residual are
normal, w is normal / sqrt(9 C), and every launch must equal, byte for byte, what the parent
commit's library gave for the same inputs (tests/golden/wino_otf_parent.npz, written once by
tools/record_wino_golden.py with EOSV_LIBRARY set to that library).  The file also holds a SHA-256
of the seeded inputs: if the regenerated inputs differ from the recorded ones the test fails (it
does not skip), naming the generator and not the kernel.  Each case runs uncapped and through
eosv_conv_wino_f32_grid with 1 and 3 workgroups, twice each, between guard bands.

Ownership probes: integer problems, exact against the f64 convolution (bounds as in
tests/test_gpu_wino_exact.py: |x| <= 3, w = 4 * [-2, 2], every intermediate an integer below
2^24).  The weights are non-zero for one output-channel half of every 64-channel block only, or
for one column of taps only (kw = 0: U's position columns 0..2, column 3 is zero; kw = 2: columns
1..3), so that a wave that writes S for the wrong half or column shows in the output; one case
has bias = nullptr and no residual.  Shapes (3, 3, 5, 64) and (5, 4, 4, 128) with one workgroup:
it walks two and four items, and the S pass overwrites V0 ahead of the rewritten chunk 0."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_wino_golden", os.path.join(REPO, "tools", "record_wino_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CAPS = (None, 1, 3)
GOLDEN_IDS = [rec.case_name(s, rr) for s, rr in rec.CASES]


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(rec.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("shape,rr", rec.CASES, ids=GOLDEN_IDS)
def test_bitwise_the_parent_on_normal_data(shape, rr):
    name = rec.case_name(shape, rr)
    g = _golden()
    got, want = rec.checksum(rec.problem(shape)), str(g["sum_" + name])
    assert got == want, f"{name}: the regenerated inputs are not the recorded ones ({got[:16]} != {want[:16]})"
    ref = g["y_" + name]
    assert ref.shape == shape and ref.dtype == np.float32
    for cap in CAPS:
        for run in range(2):
            y = rec.launch(shape, rr, cap)
            assert not (y == rec.SENTINEL).any(), "an output was not written"
            diff = y.view(np.uint32) != ref.view(np.uint32)
            n = int(diff.sum())
            print(f"wino otf {name} cap={cap} run {run}: {n} of {y.size} outputs differ from the parent's bits")
            if n:
                at = tuple(np.argwhere(diff)[0])
                pytest.fail(f"{name} cap={cap} run {run}: {n} outputs differ; first at (n, h, w, c) = {list(at)}: "
                            f"{y[at]!r} != {ref[at]!r}")


PROBE_SHAPES = [(3, 3, 5, 64), (5, 4, 4, 128)]
# (weights kept, bias given, residual + ReLU)
PROBES = [("half0", True, True), ("half1", True, True), ("kw0", True, True), ("kw2", True, True),
          ("all-nobias", False, False)]


@functools.lru_cache(maxsize=None)
def _integers(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(7919 + 1000 * C + 100 * N + 10 * H + W)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).float()
    w = 4.0 * torch.randint(-2, 3, (C, C, 3, 3), generator=g).float()
    b = torch.randint(-5, 6, (C,), generator=g).float()
    r = torch.randint(-9, 10, (N, C, H, W), generator=g).float()
    assert C * 12 * 18 * 9 + 5 + 9 < 2 ** 24
    xn = x.permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=w, b=b, r=r, xd=rec.guarded(xn.numpy()), bd=b.cuda(),
                rd=r.permute(0, 2, 3, 1).contiguous().cuda())


def _kept(w, keep):
    C = w.shape[0]
    out = torch.zeros_like(w)
    if keep in ("half0", "half1"):
        sel = (torch.arange(C) % 64) // 32 == int(keep[-1])
        out[sel] = w[sel]
    elif keep in ("kw0", "kw2"):
        kw = int(keep[-1])
        out[:, :, :, kw] = w[:, :, :, kw]
    else:
        out = w.clone()
    return out


@pytest.mark.parametrize("shape", PROBE_SHAPES, ids=["x".join(map(str, s)) for s in PROBE_SHAPES])
@pytest.mark.parametrize("keep,bias,rr", PROBES, ids=[p[0] for p in PROBES])
def test_ownership_probe_is_exact(shape, keep, bias, rr):
    from eosv._lib import check, lib

    N, H, W, C = shape
    p = _integers(shape)
    w = _kept(p["w"], keep)
    assert bool((w != 0).any())
    u = np.empty(16 * C * C, np.float32)
    check(lib().eosv_wino_weights_f32(w.numpy().ctypes.data, None, C, C, u.ctypes.data), "eosv_wino_weights_f32")
    assert np.array_equal(u, np.rint(u)) and float(np.abs(u).max()) <= 18.0
    if keep in ("kw0", "kw2"):   # the probe's premise: one position column of U is zero
        u4 = u.reshape(-1, 16, 8, 64)   # [block x chunk][pos][channel][cout]: wino_u_index
        zero = 3 if keep == "kw0" else 0
        assert not u4[:, zero::4].any() and u4[:, (zero + 1) % 4::4].any()
    ud = torch.from_numpy(u).cuda()
    ref = torch.nn.functional.conv2d(p["x"].double(), w.double(), padding=1)
    if bias:
        ref = ref + p["b"].double()[None, :, None, None]
    if rr:
        ref = torch.relu(ref + p["r"].double())
    ref = ref.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 2 ** 24
    ref = ref.float().numpy()
    ys = [rec.launch_arrays(shape, p["xd"], ud, p["bd"] if bias else None, p["rd"] if rr else None, rr, 1)
          for _ in range(2)]
    assert ys[0].tobytes() == ys[1].tobytes(), "two launches of one problem differ"
    y = ys[0]
    assert not (y == rec.SENTINEL).any(), "an output was not written"
    bad = np.argwhere(y != ref)
    print(f"wino otf probe {shape} {keep} bias={bias} res/relu={rr}: {len(bad)} of {y.size} outputs differ")
    if len(bad):
        at = tuple(bad[0])
        halves = sorted({int(c) % 64 // 32 for c in bad[:, 3]})
        pytest.fail(f"{len(bad)} outputs differ, in channel halves {halves}; first at (n, h, w, c) = {list(at)}: "
                    f"{y[at]} != {ref[at]}")
