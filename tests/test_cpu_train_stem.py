"""The opt-in direct 7x7 stem kernels of the training step, the parts that need no device: the C ABI
exports eosv_stem_conv_f32, eosv_stem_wgrad_f32 and its workspace function and validates their
arguments before any device call, NativeTrainer takes `stem_direct` as a bool only, and the drop-in
TrainNetwork hands its `train_stem_direct` attribute to the trainer it builds."""
import ctypes
import types

import pytest

from eosv import _lib

NAMES = ("eosv_stem_conv_f32", "eosv_stem_wgrad_f32_workspace", "eosv_stem_wgrad_f32")


def _library():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def _entries(L):
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fwd = L.eosv_stem_conv_f32
    fwd.restype, fwd.argtypes = i32, [vp, i32, i32, i32, vp, vp, vp]
    ws = L.eosv_stem_wgrad_f32_workspace
    ws.restype, ws.argtypes = i64, [i32] * 3
    wg = L.eosv_stem_wgrad_f32
    wg.restype, wg.argtypes = i32, [vp, vp, i32, i32, i32, vp, vp, i64, vp]
    L.eosv_last_error.restype = ctypes.c_char_p
    return fwd, ws, wg


BAD_SIZES = [(0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, 8, -4)]
P = 4096        # a non-null, 16-byte aligned address (never dereferenced)
BIG = 1 << 40


def test_library_exports_the_stem_entry_points():
    L = _library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


def test_stem_conv_rejects_before_any_device_call():
    L = _library()
    fwd, _, _ = _entries(L)
    calls = [(None, 2, 8, 8, P, P), (P, 2, 8, 8, None, P), (P, 2, 8, 8, P, None)]
    calls += [(P, n, h, w, P, P) for n, h, w in BAD_SIZES]
    for args in calls:
        assert fwd(*args, None) == -1, args  # EOSV_ERR_ARG
        assert b"eosv_stem_conv_f32" in L.eosv_last_error(), args


def test_stem_wgrad_rejects_before_any_device_call():
    L = _library()
    _, ws, wg = _entries(L)
    calls = [(None, P, 2, 8, 8, P, P, BIG), (P, None, 2, 8, 8, P, P, BIG), (P, P, 2, 8, 8, None, P, BIG),
             (P, P, 2, 8, 8, P, None, BIG)]
    calls += [(P, P, n, h, w, P, P, BIG) for n, h, w in BAD_SIZES]
    # a workspace one byte short, and none
    calls += [(P, P, 2, 8, 8, P, P, ws(2, 8, 8) - 1), (P, P, 96, 224, 224, P, P, 0)]
    for args in calls:
        assert wg(*args, None) == -1, args
        assert b"eosv_stem_wgrad_f32" in L.eosv_last_error(), args


def test_stem_entries_report_unsupported_widths_and_alignment():
    """W % 4 != 0, a width past the cap, a misaligned pointer and sizes past 32-bit offsets are
    EOSV_ERR_UNSUPPORTED (the trainer's fall-back signal), returned before any launch."""
    L = _library()
    fwd, ws, wg = _entries(L)
    mis = P + 4
    for args in [(P, 2, 8, 30, P, P), (P, 2, 8, 260, P, P), (mis, 2, 8, 8, P, P), (P, 2, 8, 8, mis, P),
                 (P, 2, 8, 8, P, mis), (P, 4096, 224, 224, P, P)]:
        assert fwd(*args, None) == -4, args
        assert b"eosv_stem_conv_f32" in L.eosv_last_error(), args
    for args in [(P, P, 2, 8, 30, P, P, BIG), (P, P, 2, 8, 260, P, P, BIG), (mis, P, 2, 8, 8, P, P, BIG),
                 (P, mis, 2, 8, 8, P, P, BIG), (P, P, 2, 8, 8, mis, P, BIG), (P, P, 2, 8, 8, P, mis, BIG),
                 (P, P, 4096, 224, 224, P, P, BIG)]:
        assert wg(*args, None) == -4, args
        assert b"eosv_stem_wgrad_f32" in L.eosv_last_error(), args


def test_stem_wgrad_workspace_sizes():
    L = _library()
    _, ws, _ = _entries(L)
    for n, h, w in BAD_SIZES:
        assert ws(n, h, w) <= 0, (n, h, w)
    one = 64 * 147 * 4  # a partial dW
    for n, h, w in ((1, 8, 8), (96, 224, 224), (2, 64, 256)):
        b = ws(n, h, w)
        assert b >= one and b % one == 0, (n, h, w, b)
    assert ws(1, 8, 8) == one  # 4 output rows: one work item


def test_binding_declares_the_stem_signatures():
    L = _lib.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.eosv_stem_conv_f32.argtypes == [vp, i32, i32, i32, vp, vp, vp]
    assert L.eosv_stem_wgrad_f32_workspace.restype is i64
    assert L.eosv_stem_wgrad_f32.argtypes == [vp, vp, i32, i32, i32, vp, vp, i64, vp]


def test_trainer_stem_direct_argument_is_a_bool(monkeypatch):
    """Default / False -> off, True -> on, anything else raises; the other opt-ins are untouched.
    The constructor's device work is stubbed out."""
    import numpy as np
    import torch

    from eosv import train

    monkeypatch.setattr(train, "lib", lambda: types.SimpleNamespace(eosv_bn_workspace_bytes=lambda c: 64))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    tr = train.NativeTrainer("resnet18", 4)
    assert tr.stem_direct is False and tr.stem_direct_launches == 0
    assert train.NativeTrainer("resnet18", 4, stem_direct=False).stem_direct is False
    tr = train.NativeTrainer("resnet50", 4, stem_direct=True)
    assert tr.stem_direct is True and tr.stem_direct_launches == 0
    assert tr.wino_mask == 0 and tr.wino_wgrad_mask == 0
    tr = train.NativeTrainer("resnet18", 4, winograd=5, winograd_wgrad=True, stem_direct=np.True_)
    assert tr.stem_direct is True and tr.wino_mask == 5 and tr.wino_wgrad_mask == train.TRAIN_WINO_WGRAD_DEFAULT
    for bad in (1, 0, None, "yes", 1.0, 15):
        with pytest.raises(ValueError, match="stem_direct"):
            train.NativeTrainer("resnet18", 4, stem_direct=bad)


def test_train_network_passes_train_stem_direct_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_stem_direct defaults to False and is read at finetune_model time; False
    passes no keyword at all (a trainer without it keeps working)."""
    import network_train
    import torch

    assert network_train.TrainNetwork.train_stem_direct is False
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
    for value, wgrad in ((False, False), (True, False), (True, 6)):
        tn = object.__new__(network_train.TrainNetwork)
        tn.__dict__.update(loss_path=str(tmp_path / "loss.txt"), ckp_path=str(tmp_path) + "/", epoch_nums=0,
                           batch_size=2, lr_1=1e-4, lr_2=1e-3, lr_step_size=10, resnet_model="resnet18",
                           num_classes=64, mymodel=model)
        if value is not False:
            tn.train_stem_direct = value
        if wgrad is not False:
            tn.train_winograd_wgrad = wgrad
        tn.finetune_model()
    assert seen == [{}, {"stem_direct": True}, {"winograd_wgrad": 6, "stem_direct": True}]
    assert seen[1]["stem_direct"] is True
