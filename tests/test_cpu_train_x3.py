"""The opt-in f32x3 GEMMs of the training step's stride-1 1x1 convs (csrc/gemm_x3.hip), the parts
that need no device: eosv_sgemm_x3, eosv_sgemm_x3_tn_splitk and its workspace function are exported
and validate their arguments before any device call (bad arguments: EOSV_ERR_ARG; what the kernels do
not take: EOSV_ERR_UNSUPPORTED, the trainer's fall-back signal), the workspace function reads no
device, NativeTrainer parses `f32x3` as a stage mask and marks the eligible convs, and the drop-in
TrainNetwork hands `train_f32x3` on.

split_bf16 / x3_terms restate the kernel's arithmetic in numpy; tests/test_gpu_train_x3.py imports
them as its model."""
import ctypes
import types

import numpy as np
import pytest

from eosv import _lib

NAMES = ("eosv_sgemm_x3", "eosv_sgemm_x3_tn_splitk_workspace", "eosv_sgemm_x3_tn_splitk")
CHANNELS = (64, 128, 256, 512, 1024, 2048)
ARG, UNSUPPORTED = -1, -4
P = 4096  # a non-null, 16-byte aligned address; never dereferenced: every call below returns before a launch


# ---------------------------------------------------------------- the split, in numpy
def bf16_rne(x):
    """f32 -> the nearest bf16 (ties to even), as f32."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split_bf16(x):
    """(hi, lo) of the kernel's split: hi = bf16(x), lo = bf16(x - hi), the subtraction in f32 (exact)."""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def x3_terms(a, b):
    """The f64 value of sum_k (a_hi b_hi + a_hi b_lo + a_lo b_hi) for A [m][k], B [k][n]."""
    ah, al = (v.astype(np.float64) for v in split_bf16(a))
    bh, bl = (v.astype(np.float64) for v in split_bf16(b))
    return ah @ bh + ah @ bl + al @ bh


def test_split_reproduces_16_bit_integers():
    x = np.arange(-(1 << 16) + 1, 1 << 16, dtype=np.float32)
    hi, lo = split_bf16(x)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    # 12-bit integers: 8 bits in hi, the rest (at most 4 significant bits and a sign) in lo
    small = np.abs(x) < (1 << 12)
    assert float(np.abs(lo[small]).max()) <= 8.0


def test_split_residual_is_below_2_pow_minus_16():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000), rng.standard_normal(1000) * 1e30,
                        rng.standard_normal(1000) * 1e-30]).astype(np.float32)
    hi, lo = split_bf16(x)
    rho = x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert np.all(np.abs(rho) <= 2.0 ** -16 * np.abs(x.astype(np.float64)))
    # hi and lo are bf16 values: their low 16 bits are clear
    assert not np.any(hi.view(np.uint32) & 0xFFFF) and not np.any(lo.view(np.uint32) & 0xFFFF)
    # ties go to even: 1 + 2^-8 is halfway between 1 and 1 + 2^-7
    assert bf16_rne(np.float32(1 + 2.0 ** -8)) == 1.0 and bf16_rne(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6


# ---------------------------------------------------------------- the C ABI
def _library():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def _entries(L):
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    mm = L.eosv_sgemm_x3
    mm.restype, mm.argtypes = i32, [i32, i32, i32, i32, i32, f32, vp, i32, vp, i32, f32, vp, i32, vp, vp]
    ws = L.eosv_sgemm_x3_tn_splitk_workspace
    ws.restype, ws.argtypes = i64, [i32] * 3
    tn = L.eosv_sgemm_x3_tn_splitk
    tn.restype, tn.argtypes = i32, [i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i64, vp]
    L.eosv_last_error.restype = ctypes.c_char_p
    return mm, ws, tn


def _gemm(mm, ta, tb, m, n, k, a=P, lda=None, b=P, ldb=None, c=P, ldc=None, add=None):
    lda = (m if ta else k) if lda is None else lda
    ldb = (k if tb else n) if ldb is None else ldb
    ldc = n if ldc is None else ldc
    return mm(ta, tb, m, n, k, 1.0, a, lda, b, ldb, 0.0, c, ldc, add, None)


def test_library_exports_and_header_declares_the_entry_points():
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


def test_binding_declares_the_signatures():
    L = _lib.lib()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert L.eosv_sgemm_x3.argtypes == [i32, i32, i32, i32, i32, f32, vp, i32, vp, i32, f32, vp, i32, vp, vp]
    assert L.eosv_sgemm_x3_tn_splitk_workspace.restype is i64
    assert L.eosv_sgemm_x3_tn_splitk.argtypes == [i32, i32, i32, vp, i32, vp, i32, vp, i32, vp, i64, vp]


def test_sgemm_x3_rejects_bad_arguments_before_any_device_call():
    L = _library()
    mm, _, _ = _entries(L)
    calls = [dict(a=None), dict(b=None), dict(c=None), dict(ldc=63), dict(lda=60), dict(ldb=60), dict(lda=0),
             dict(ldb=-4)]
    for kw in calls:
        for ta, tb in ((0, 1), (0, 0), (1, 0)):
            assert _gemm(mm, ta, tb, 64, 64, 64, **kw) == ARG, (ta, tb, kw)
            assert b"eosv_sgemm_x3" in L.eosv_last_error(), kw
    for m, n, k in ((-1, 64, 64), (100, -64, 64), (100, 64, -64)):
        assert mm(0, 1, m, n, k, 1.0, P, 64, P, 64, 0.0, P, 64, None, None) == ARG, (m, n, k)
    # an empty result is nothing to do
    assert _gemm(mm, 0, 1, 0, 64, 64, lda=64) == 0


def test_sgemm_x3_reports_what_it_does_not_take():
    """Other channel counts, both transposes, a pointer off 16 bytes, a leading dimension that is
    no multiple of 4 and an empty reduction: EOSV_ERR_UNSUPPORTED before any launch."""
    L = _library()
    mm, _, _ = _entries(L)
    mis = P + 4
    refused = [
        (0, 1, dict(m=100, n=72, k=64)), (0, 1, dict(m=100, n=64, k=72)), (0, 1, dict(m=100, n=64, k=96)),
        (0, 0, dict(m=100, n=72, k=64)), (0, 0, dict(m=100, n=64, k=192)), (0, 0, dict(m=100, n=4096, k=64)),
        (1, 0, dict(m=72, n=64, k=100)), (1, 0, dict(m=64, n=32, k=100)),
        (1, 1, dict(m=64, n=64, k=64)),
        (0, 1, dict(m=100, n=64, k=0, lda=64, ldb=64)),
        (0, 1, dict(m=100, n=64, k=64, a=mis)), (0, 1, dict(m=100, n=64, k=64, b=mis)),
        (0, 1, dict(m=100, n=64, k=64, c=mis)), (0, 0, dict(m=100, n=64, k=64, add=mis)),
        (0, 1, dict(m=100, n=64, k=64, lda=66)), (0, 1, dict(m=100, n=64, k=64, ldb=65)),
        (0, 0, dict(m=100, n=64, k=64, ldc=70)), (1, 0, dict(m=64, n=64, k=100, lda=67)),
    ]
    for ta, tb, kw in refused:
        assert _gemm(mm, ta, tb, **kw) == UNSUPPORTED, (ta, tb, kw)
        assert b"eosv_sgemm_x3" in L.eosv_last_error(), kw


def test_tn_splitk_rejects_and_reports_before_any_device_call():
    L = _library()
    _, ws, tn = _entries(L)
    big = 1 << 40
    bad = [(0, 64, 100), (64, 0, 100), (64, 64, 0), (-64, 64, 100)]
    for m, n, k in bad:
        assert tn(m, n, k, P, max(m, 1), P, max(n, 1), P, max(n, 1), P, big, None) == ARG, (m, n, k)
    for args in [(64, 64, 100, None, 64, P, 64, P, 64, P, big), (64, 64, 100, P, 64, None, 64, P, 64, P, big),
                 (64, 64, 100, P, 64, P, 64, None, 64, P, big),
                 (64, 64, 100, P, 60, P, 64, P, 64, P, big), (64, 64, 100, P, 64, P, 60, P, 64, P, big),
                 (64, 64, 100, P, 64, P, 64, P, 60, P, big),
                 (64, 64, 100, P, 64, P, 64, P, 64, None, 4096),     # bytes without a buffer
                 (64, 64, 100, P, 64, P, 64, P, 64, P, -1)]:
        assert tn(*args, None) == ARG, args
        assert b"eosv_sgemm_x3_tn_splitk" in L.eosv_last_error(), args
    # where the plan splits, a workspace that cannot hold one slice
    assert ws(64, 64, 5000) > 0
    assert tn(64, 64, 5000, P, 64, P, 64, P, 64, P, 64 * 64 * 4 - 1, None) == ARG
    mis = P + 8
    for args in [(72, 64, 100, P, 72, P, 64, P, 64, P, big), (64, 96, 100, P, 64, P, 96, P, 96, P, big),
                 (64, 64, 100, mis, 64, P, 64, P, 64, P, big), (64, 64, 100, P, 64, mis, 64, P, 64, P, big),
                 (64, 64, 100, P, 64, P, 64, mis, 64, P, big), (64, 64, 100, P, 64, P, 64, P, 64, mis, big),
                 (64, 64, 100, P, 66, P, 64, P, 64, P, big), (64, 64, 100, P, 64, P, 70, P, 64, P, big),
                 (64, 64, 100, P, 64, P, 64, P, 65, P, big)]:
        assert tn(*args, None) == UNSUPPORTED, args
        assert b"eosv_sgemm_x3_tn_splitk" in L.eosv_last_error(), args


def test_tn_splitk_workspace_is_monotone_in_k_and_whole_slices():
    L = _library()
    _, ws, _ = _entries(L)
    for m, n, k in ((0, 64, 100), (64, -1, 100), (64, 64, 0), (64, 64, -5)):
        assert ws(m, n, k) == 0, (m, n, k)
    ks = [1, 31, 33, 255, 511, 512, 1000, 5000, 18816, 75264, 301056, 1 << 22]
    for m in CHANNELS:
        for n in CHANNELS:
            one = m * n * 4
            sizes = [ws(m, n, k) for k in ks]
            assert sizes == sorted(sizes), (m, n, sizes)
            assert all(b % one == 0 and b != one for b in sizes), (m, n, sizes)  # 0 or at least two slices
            assert all(b <= 1024 * one for b in sizes), (m, n)
            # a reduction under two slices' worth of rows is never split
            assert sizes[0] == sizes[1] == sizes[2] == sizes[3] == sizes[4] == 0, (m, n, sizes)
    # the shapes the GPU tests rely on: one slice at 33 rows, several at 1000 and 5000
    assert ws(64, 64, 33) == 0 and ws(64, 64, 1000) >= 2 * 64 * 64 * 4 and ws(64, 64, 5000) > ws(64, 64, 1000)


# ---------------------------------------------------------------- the trainer's keyword
def _stub_device(monkeypatch):
    import torch

    from eosv import train

    monkeypatch.setattr(train, "lib", lambda: types.SimpleNamespace(eosv_bn_workspace_bytes=lambda c: 64))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    return train


def test_stage_mask_parses_f32x3():
    from eosv import train

    assert train._stage_mask(False, train.TRAIN_X3_DEFAULT, "f32x3") == 0
    assert train._stage_mask(None, train.TRAIN_X3_DEFAULT, "f32x3") == 0
    assert train._stage_mask(True, train.TRAIN_X3_DEFAULT, "f32x3") == train.TRAIN_X3_DEFAULT
    assert 0 <= train.TRAIN_X3_DEFAULT <= 15
    for v in (0, 1, 6, 15, np.int64(9)):
        assert train._stage_mask(v, train.TRAIN_X3_DEFAULT, "f32x3") == int(v)
    for bad in (16, -1, 1.0, "15"):
        with pytest.raises(ValueError, match="f32x3"):
            train._stage_mask(bad, train.TRAIN_X3_DEFAULT, "f32x3")


def test_trainer_marks_the_eligible_convs_by_stage(monkeypatch):
    """Bit li enables layer{li+1}: conv1 and conv3 of its bottlenecks and, in layer 1, the stride-1
    downsample; the 3x3 convs, the stride-2 shortcuts and the stem never; ResNet-18 has none."""
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer("resnet50", 4)
    assert tr.x3_mask == 0 and tr.x3_launches == 0 and not any(c.x3 for c in tr._convs())
    assert not any(c.x3 for c in train.NativeTrainer("resnet50", 4, f32x3=False)._convs())
    with pytest.raises(ValueError, match="f32x3"):
        train.NativeTrainer("resnet50", 4, f32x3=16)
    tr = train.NativeTrainer("resnet50", 4, f32x3=15, winograd=3, stem_direct=True)
    assert tr.x3_mask == 15 and tr.wino_mask == 3 and tr.wino_wgrad_mask == 0 and tr.stem_direct is True
    on = [c.name for c in tr._convs() if c.x3]
    assert len(on) == 2 * 16 + 1
    assert "convnet.4.0.downsample.0" in on and "convnet.5.0.downsample.0" not in on and "convnet.0" not in on
    assert all(c.k == 1 and c.stride == 1 for c in tr._convs() if c.x3)
    assert all(c.x3 for c in tr._convs() if c.k == 1 and c.stride == 1)
    per_stage = {1: 7, 2: 8, 4: 12, 8: 6}   # 2 x (3, 4, 6, 3) blocks, + the layer-1 downsample
    for mask, count in per_stage.items():
        tr = train.NativeTrainer("resnet50", 4, f32x3=mask)
        on = [c.name for c in tr._convs() if c.x3]
        li = mask.bit_length() - 1
        assert len(on) == count and all(name.startswith(f"convnet.{4 + li}.") for name in on), (mask, on)
    assert not any(c.x3 for c in train.NativeTrainer("resnet18", 4, f32x3=15)._convs())


def test_train_network_passes_train_f32x3_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_f32x3 defaults to False and is read at finetune_model time; False passes no
    keyword at all."""
    import network_train
    import torch

    assert network_train.TrainNetwork.train_f32x3 is False
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
            tn.train_f32x3 = value
        tn.finetune_model()
    assert seen == [{}, {"f32x3": True}, {"f32x3": 6}]
