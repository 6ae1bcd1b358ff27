"""The BN batch statistics from the f32x3 forwards' epilogues, the parts that need no device: the
_stats_chunks functions against the plan rule restated here, the entry points' argument checks (every
status below is returned before any device call), NativeTrainer(fused_bn_stats=...) and its plans, the
hand-off from the conv dispatcher to the BN forward over fake routes, and the drop-in's
train_fused_bn_stats."""
import ctypes
import types

import numpy as np
import pytest
import torch

from eosv import _lib, arch
from test_cpu_train_routes import ALL, NONE, PART, UNSUPPORTED
from test_cpu_train_x3 import _library, _stub_device
from test_cpu_train_x3conv import _expected_x3c, conv_dims

NAMES = ("eosv_sgemm_x3_stats_chunks", "eosv_conv2d_x3_stats_chunks", "eosv_sgemm_x3_stats", "eosv_conv2d_x3_stats",
         "eosv_bn_train_forward_stats")
ARG = -1
P = 4096  # a non-null, 16-byte aligned address; never dereferenced: every call below returns before a launch


def _entries(L):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = {"eosv_sgemm_x3_stats_chunks": (i32, [i32, i32, i32]),
           "eosv_conv2d_x3_stats_chunks": (i32, [i32] * 9),
           "eosv_sgemm_x3_stats": (i32, [i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i64, vp]),
           "eosv_conv2d_x3_stats": (i32, [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, i64, vp]),
           "eosv_bn_train_forward_stats": (i32, [vp, i64, i32, vp, i32, vp, vp, f32, f32, vp, vp, vp, i32, vp, vp, vp, vp,
                                                 vp])}
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    L.eosv_last_error.restype = ctypes.c_char_p
    return sig


# ---------------------------------------------------------------- the chunk counts
def _rule(rows, n):
    """Row tiles of the unsplit plan: the tile is 128 rows high only where ceil(rows / 128) x ceil(n / (64 wn))
    reaches 512 (two workgroups for each of the plan's 256 CUs), wn = 2 for n > 64; else 64."""
    wn = 2 if n > 64 else 1
    R = 128 if rows > 64 and -(-rows // 128) * -(-n // (64 * wn)) >= 512 else 64
    return -(-rows // R)


def _net_convs(name, frames=96, side=56):
    """[(kind, args, rows, cout)] of every non-stem conv at the reference batch (6 clips of 16 frames at
    224 x 224: a 56 x 56 map into layer 1): kind "gemm" (m, n, k) for the stride-1 1x1 convs, else "conv"."""
    spec = arch.SPECS[name]
    out = []
    inplanes, hw = 64, side
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), spec.layers)):
        for bi in range(blocks):
            stride = 2 if (li > 0 and bi == 0) else 1
            cout = planes * spec.expansion
            ohw = (hw - 1) // stride + 1
            if spec.block == "basic":
                convs = [(inplanes, planes, 3, stride, hw), (planes, planes, 3, 1, ohw)]
            else:
                convs = [(inplanes, planes, 1, 1, hw), (planes, planes, 3, stride, hw), (planes, cout, 1, 1, ohw)]
            if bi == 0 and (stride != 1 or inplanes != cout):
                convs.append((inplanes, cout, 1, stride, hw))
            for cin, co, k, s, h in convs:
                rows = frames * ((h + 2 * (k // 2) - k) // s + 1) ** 2
                if k == 1 and s == 1:
                    out.append(("gemm", (rows, co, cin), rows, co))
                else:
                    out.append(("conv", (frames, h, h, cin, co, k, k, s, k // 2), rows, co))
            inplanes, hw = cout, ohw
    return out


def test_chunk_counts_follow_the_plan_rule():
    L = _library()
    _entries(L)
    for name, count in (("resnet18", 19), ("resnet50", 52)):
        convs = _net_convs(name)
        assert len(convs) == count
        for kind, args, rows, cout in convs:
            got = (L.eosv_sgemm_x3_stats_chunks if kind == "gemm" else L.eosv_conv2d_x3_stats_chunks)(*args)
            assert got == _rule(rows, cout) >= 1, (name, kind, args, got)
    # layer 1 at the reference batch: more chunks than the BN workspace's 1024
    assert L.eosv_sgemm_x3_stats_chunks(96 * 56 * 56, 256, 64) == 2352
    assert L.eosv_conv2d_x3_stats_chunks(96, 56, 56, 64, 64, 3, 3, 1, 1) == 2352
    # the kernel tests' shapes (tests/test_gpu_train_bnstats.py)
    for (m, n, k), want in (((70, 64, 64), 2), ((40000, 128, 64), 625), ((65530, 64, 64), 512),
                            ((65530, 128, 64), 512), ((300, 256, 128), 5)):
        assert L.eosv_sgemm_x3_stats_chunks(m, n, k) == _rule(m, n) == want, (m, n, k)
    for shape, want in (((2, 5, 7, 32, 64, 3, 1, 1), 2), ((3, 9, 6, 64, 128, 3, 2, 1), 1), ((2, 7, 5, 128, 256, 1, 2, 0), 1),
                        ((1, 12, 11, 96, 64, 3, 1, 1), 3), ((1, 3, 2, 512, 512, 3, 1, 1), 1),
                        ((8, 91, 90, 32, 128, 3, 1, 1), 512)):
        N, H, W, Cin, Cout, k, stride, pad = shape
        rows = conv_dims(N, H, W, k, stride, pad)[2]
        assert L.eosv_conv2d_x3_stats_chunks(N, H, W, Cin, Cout, k, k, stride, pad) == _rule(rows, Cout) == want, shape
    # refused shapes
    assert L.eosv_conv2d_x3_stats_chunks(2, 5, 7, 48, 64, 3, 3, 1, 1) == 0
    assert L.eosv_conv2d_x3_stats_chunks(2, 5, 7, 32, 72, 3, 3, 1, 1) == 0
    assert L.eosv_conv2d_x3_stats_chunks(0, 5, 7, 32, 64, 3, 3, 1, 1) == 0
    assert L.eosv_conv2d_x3_stats_chunks(2, 1, 6, 32, 64, 5, 5, 1, 1) == 0
    assert L.eosv_sgemm_x3_stats_chunks(100, 96, 64) == 0 and L.eosv_sgemm_x3_stats_chunks(100, 64, 96) == 0
    assert L.eosv_sgemm_x3_stats_chunks(0, 64, 64) == 0 and L.eosv_sgemm_x3_stats_chunks(100, 64, 0) == 0


# ---------------------------------------------------------------- the C ABI
def test_library_binding_and_header_declare_the_entry_points():
    import os
    import re

    L = _library()
    sig = _entries(L)
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eosv.h")
    with open(header) as fh:
        text = fh.read()
    B = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/eosv.h"
        assert getattr(B, name).argtypes == sig[name][1] and getattr(B, name).restype is sig[name][0], name


def _gemm(L, m=70, n=64, k=64, a=P, b=P, c=P, st=P, nbytes=None):
    chunks = -(-m // 64)
    return L.eosv_sgemm_x3_stats(m, n, k, a, k, b, k, c, n, st, 16 * chunks * n if nbytes is None else nbytes, None)


def _conv(L, Cin=32, Cout=64, x=P, w=P, y=P, st=P, nbytes=None):
    return L.eosv_conv2d_x3_stats(x, 2, 5, 7, Cin, w, Cout, 3, 3, 1, 1, y, st, 16 * 2 * Cout if nbytes is None else nbytes,
                                  None)


def test_statuses_before_any_device_call():
    L = _library()
    _entries(L)
    for call, name in ((_gemm, b"eosv_sgemm_x3_stats"), (_conv, b"eosv_conv2d_x3_stats")):
        for kw in (dict(st=None), dict(nbytes=16 * 2 * 64 - 1), dict(nbytes=16 * 64), dict(nbytes=0), dict(nbytes=-1)):
            assert call(L, **kw) == ARG, (name, kw)
            assert name in L.eosv_last_error()
        assert call(L, st=P + 8) == UNSUPPORTED
        assert name in L.eosv_last_error() and b"d_stats" in L.eosv_last_error()
        assert call(L, **{"c" if call is _gemm else "y": P + 4}) == UNSUPPORTED
    assert _gemm(L, a=None) == ARG and _gemm(L, c=None) == ARG and _conv(L, x=None) == ARG and _conv(L, y=None) == ARG
    assert _gemm(L, n=96, nbytes=1 << 20) == UNSUPPORTED and _gemm(L, k=96, nbytes=1 << 20) == UNSUPPORTED
    assert _conv(L, Cin=48) == UNSUPPORTED and _conv(L, Cout=72, nbytes=1 << 20) == UNSUPPORTED
    bn = L.eosv_bn_train_forward_stats
    good = [P, 8, 8, P, 1, P, P, 1e-5, 0.1, None, None, None, 0, P, None, P, P, None]
    for i, bad in ((3, None), (4, 0), (4, -2), (0, None), (1, 0), (2, 0), (7, 0.0), (9, P)):
        a = list(good)
        a[i] = bad
        assert bn(*a) == ARG, (i, bad)
        assert b"eosv_bn_train_forward_stats" in L.eosv_last_error()


# ---------------------------------------------------------------- the trainer's keyword and plans
def test_stage_mask_parses_fused_bn_stats(monkeypatch):
    train = _stub_device(monkeypatch)
    assert 0 <= train.TRAIN_BNSTATS_DEFAULT <= 15
    assert train.NativeTrainer("resnet18", 4).bnstats_mask == 0
    assert train.NativeTrainer("resnet18", 4, fused_bn_stats=False).bnstats_mask == 0
    assert train.NativeTrainer("resnet18", 4, fused_bn_stats=True).bnstats_mask == train.TRAIN_BNSTATS_DEFAULT
    assert train.NativeTrainer("resnet18", 4, fused_bn_stats=np.int64(9)).bnstats_mask == 9
    for bad in (16, -1, "yes", 1.0):
        with pytest.raises(ValueError, match="fused_bn_stats"):
            train.NativeTrainer("resnet18", 4, fused_bn_stats=bad)
    tr = train.NativeTrainer("resnet50", 4, fused_bn_stats=5, f32x3=15, f32x3_convs=15)
    assert tr.bn_fused_launches == 0 and tr._fwd_stats is None and not tr.stem.stats
    for c in tr._convs():
        if c is not tr.stem:
            assert c.stats is bool(5 >> (int(c.name.split(".")[1]) - 4) & 1), c.name


@pytest.mark.parametrize("arch_name", ["resnet18", "resnet50"])
@pytest.mark.parametrize("switches", [NONE, ALL, PART], ids=["none", "all", "part"])
def test_plans_do_not_depend_on_the_switch(monkeypatch, arch_name, switches):
    """Off: the routes of a trainer built without the keyword, which are the rules of the routes test; on: the
    same tuples, since only the entry a forward route calls differs."""
    train = _stub_device(monkeypatch)
    for x3c in (0, 15, 6):
        want = [_expected_x3c(c, x3c, **switches)[0]
                for c in train.NativeTrainer(arch_name, 4, **switches, f32x3_convs=x3c)._convs()]
        for value in (False, 0, 15, 3, True):
            tr = train.NativeTrainer(arch_name, 4, **switches, f32x3_convs=x3c, fused_bn_stats=value)
            assert [c.routes for c in tr._convs()] == want, (x3c, value)
            assert [c.routes for c in train.NativeTrainer(arch_name, 4, **switches, f32x3_convs=x3c)._convs()] == want
            if not value:
                assert not any(c.stats for c in tr._convs())


# ---------------------------------------------------------------- the hand-off over fake routes
HAND = ("the statistics buffer", 7)


def _fake_forward(monkeypatch, statuses, conv=None, **kw):
    """The mechanism of tests/test_cpu_train_routes.py: a trainer whose forward routes of one conv are fakes
    answering `statuses` ({name: status}, in plan order); the x3 and x3c fakes return a hand-off as the real
    routes do with the switch on.  Returns it, the conv and the list the fakes log into."""
    train = _stub_device(monkeypatch)
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: None)
    tr = train.NativeTrainer("resnet18", 4, f32x3_convs=15, fused_bn_stats=15, **kw)
    c = conv(tr) if conv else tr.blocks[0].convs[0]
    c.routes = dict(c.routes, fwd=tuple(statuses))
    asked = []
    for name, rc in statuses.items():
        def route(cv, x, shape, P_, dz, out, acc, s, name=name, rc=rc):
            asked.append(name)
            return (rc, f"eosv_fake_{name}") + ((HAND,) if name in ("x3", "x3c") else ())
        monkeypatch.setattr(tr, f"_fwd_{name}", route)
    calls = []
    tr.L = types.SimpleNamespace(
        eosv_bn_train_forward=lambda *a: calls.append(("plain", a)) or 0,
        eosv_bn_train_forward_stats=lambda *a: calls.append(("stats", a)) or 0)
    return tr, c, asked, calls


@pytest.mark.parametrize("statuses,winner,handed", [
    ({"x3c": 0, "conv": 0, "gemm": 0}, "x3c", True),
    ({"x3": 0, "conv": 0, "gemm": 0}, "x3", True),
    ({"x3c": UNSUPPORTED, "conv": 0, "gemm": 0}, "conv", False),
    ({"x3c": UNSUPPORTED, "x3": UNSUPPORTED, "conv": UNSUPPORTED, "gemm": 0}, "gemm", False),
    ({"x3c": UNSUPPORTED, "wino": 0}, "wino", False),
])
def test_only_the_route_that_ran_hands_statistics_to_the_bn(monkeypatch, statuses, winner, handed):
    tr, c, asked, calls = _fake_forward(monkeypatch, statuses)
    tr._fwd_stats = ("stale", 1)
    y, oshape = tr._conv_fwd(None, (2, 8, 8, 64), c, 0)
    names = list(statuses)
    assert asked == names[:names.index(winner) + 1] and oshape == (2, 8, 8, 64)
    assert tr._fwd_stats == (HAND if handed else None)
    b = tr.blocks[0].bns[0]
    z = types.SimpleNamespace(data_ptr=lambda: 48, numel=lambda: 2 * 8 * 8 * 64)
    buf = types.SimpleNamespace(data_ptr=lambda: 64)
    stats = (buf, tr._fwd_stats[1]) if handed else None
    tr._bn_fwd(z, 128, b, True, None, 5, stats=stats)
    assert [k for k, _ in calls] == ["stats" if handed else "plain"]
    a = calls[0][1]
    if handed:   # (x, P, C, part, chunks, ...): no workspace
        assert a[:5] == (48, 128, 64, 64, 7) and len(a) == 18 and a[-1] == 5
    else:
        assert a[:3] == (48, 128, 64) and len(a) == 17
    assert tr.bn_fused_launches == (1 if handed else 0) and b.nbt == 1


def test_the_stem_never_hands_statistics(monkeypatch):
    for kw in (dict(), dict(stem_direct=True)):
        statuses = {"stem": 0, "conv": 0, "gemm": 0} if kw else {"conv": 0, "gemm": 0}
        tr, c, asked, calls = _fake_forward(monkeypatch, statuses, conv=lambda tr: tr.stem, **kw)
        assert c is tr.stem and not c.stats and not {"x3", "x3c"} & set(tr._plan(c)["fwd"])
        tr._x0 = "nhwc"   # the generic routes' copy of the frames: already made
        tr._fwd_stats = ("stale", 1)
        tr._conv_fwd(None, (2, 16, 16, 3), c, 0)
        assert asked == [next(iter(statuses))] and tr._fwd_stats is None


def test_forward_routes_call_the_stats_entries_with_the_convs_geometry(monkeypatch):
    train = _stub_device(monkeypatch)
    calls = []

    def rec(name, rc=0):
        def fn(*a):
            calls.append((name, a))
            return rc
        return fn

    t = lambda p: types.SimpleNamespace(data_ptr=lambda: p)   # noqa: E731
    buf = types.SimpleNamespace(data_ptr=lambda: 64)
    for chunks in (5, 0):
        tr = train.NativeTrainer("resnet50", 4, f32x3=15, f32x3_convs=15, fused_bn_stats=2)
        tr.L = types.SimpleNamespace(eosv_conv2d_x3_stats=rec("conv"), eosv_conv2d_x3_stats_chunks=rec("cchunks", chunks),
                                     eosv_sgemm_x3_stats=rec("gemm"), eosv_sgemm_x3_stats_chunks=rec("gchunks", chunks),
                                     eosv_conv2d_x3=rec("plain conv"), eosv_sgemm_x3=rec("plain gemm"))
        monkeypatch.setattr(tr, "_buf", lambda key, n: calls.append(("buf", key, n)) or buf)
        c2 = next(c for c in tr._convs() if c.name == "convnet.5.1.conv2")
        c3 = next(c for c in tr._convs() if c.name == "convnet.5.1.conv3")
        c2.w, c3.w = t(1600), t(3200)
        shape = (2, 12, 11, 128)
        del calls[:]
        got = tr._fwd_x3c(c2, t(16), shape, 264, None, t(32), None, 7)
        if chunks:
            assert got == (0, "eosv_conv2d_x3_stats", (buf, 5))
            assert calls == [("cchunks", (2, 12, 11, 128, 128, 3, 3, 1, 1)), ("buf", "bnstats", 5 * 2 * 128 * 2),
                             ("conv", (16, 2, 12, 11, 128, 1600, 128, 3, 3, 1, 1, 32, 64, 5 * 2 * 128 * 8, 7))]
        else:   # a shape the entry refuses: no launch, the dispatcher moves on
            assert got == (UNSUPPORTED, "eosv_conv2d_x3_stats") and [k for k, *_ in calls] == ["cchunks"]
        del calls[:]
        got = tr._fwd_x3(c3, t(16), shape, 264, None, t(32), None, 7)
        if chunks:
            assert got == (0, "eosv_sgemm_x3_stats", (buf, 5))
            assert calls == [("gchunks", (264, 512, 128)), ("buf", "bnstats", 5 * 2 * 512 * 2),
                             ("gemm", (264, 512, 128, 16, 128, 3200, 128, 32, 512, 64, 5 * 2 * 512 * 8, 7))]
        else:
            assert got == (UNSUPPORTED, "eosv_sgemm_x3_stats") and [k for k, *_ in calls] == ["gchunks"]
        # a conv of a stage the mask leaves out keeps the plain entries
        c1 = next(c for c in tr._convs() if c.name == "convnet.4.1.conv2")
        c1.w = t(1600)
        del calls[:]
        assert tr._fwd_x3c(c1, t(16), (2, 12, 11, 64), 264, None, t(32), None, 7) == (0, "eosv_conv2d_x3")
        assert [k for k, *_ in calls] == ["plain conv"]


def test_train_network_passes_train_fused_bn_stats_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_fused_bn_stats defaults to False and is read at finetune_model time; False passes
    no keyword at all."""
    import network_train

    assert network_train.TrainNetwork.train_fused_bn_stats is False
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
            tn.train_fused_bn_stats = value
        tn.finetune_model()
    assert seen == [{}, {"fused_bn_stats": True}, {"fused_bn_stats": 6}]
