"""The opt-in Winograd-domain weight gradient of the training step, the parts that need no device:
the C ABI exports eosv_conv_wgrad_wino_f32 and its workspace function and validates their arguments
before any device call, NativeTrainer resolves its `winograd_wgrad` argument to a stage mask
independently of `winograd`, and the drop-in TrainNetwork hands its `train_winograd_wgrad`
attribute to the trainer it builds."""
import ctypes
import types

import pytest

from eosv import _lib


def _library():
    import os

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def _entry(L):
    fn = L.eosv_conv_wgrad_wino_f32
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p,
                                                                            ctypes.c_int64, ctypes.c_void_p]
    ws = L.eosv_conv_wgrad_wino_f32_workspace
    ws.restype = ctypes.c_int64
    ws.argtypes = [ctypes.c_int] * 4
    L.eosv_last_error.restype = ctypes.c_char_p
    return fn, ws


# (N, H, W, C) no launch may see: C = 32, 72, 0 and an empty axis
BAD_SHAPES = [(2, 8, 8, 32), (2, 8, 8, 72), (2, 8, 8, 0), (0, 8, 8, 64), (2, 0, 8, 64), (2, 8, -1, 64)]


def test_library_exports_wino_wgrad():
    L = _library()
    for name in ("eosv_conv_wgrad_wino_f32_workspace", "eosv_conv_wgrad_wino_f32"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


def test_wino_wgrad_rejects_before_any_device_call():
    """Null pointers and bad shapes return EOSV_ERR_ARG with a message naming the function; the checks
    come before any launch, so this runs without a device (the pointers are never dereferenced)."""
    L = _library()
    fn, _ = _entry(L)
    p = 4096  # a non-null address
    big = 1 << 30
    calls = [(None, p, 2, 8, 8, 64, p, p, big), (p, None, 2, 8, 8, 64, p, p, big), (p, p, 2, 8, 8, 64, None, p, big),
             (p, p, 2, 8, 8, 64, p, None, big)]
    calls += [(p, p, n, h, w, c, p, p, big) for n, h, w, c in BAD_SHAPES]
    for args in calls:
        assert fn(*args, None) == -1, args  # EOSV_ERR_ARG
        assert b"eosv_conv_wgrad_wino_f32" in L.eosv_last_error(), args


def test_wino_wgrad_workspace_sizes():
    L = _library()
    _, ws = _entry(L)
    for shape in BAD_SHAPES:
        assert ws(*shape) <= 0, shape
    for n, h, w, c in ((1, 1, 1, 64), (3, 7, 5, 64), (2, 14, 14, 128), (96, 56, 56, 64), (96, 7, 7, 512)):
        b = ws(n, h, w, c)
        assert b >= 16 * c * c * 4, (n, h, w, c, b)


def test_trainer_winograd_wgrad_argument_resolves_to_a_mask(monkeypatch):
    """False / default -> 0, True -> TRAIN_WINO_WGRAD_DEFAULT, an int mask -> itself; anything else
    raises; `winograd` is resolved on its own.  The constructor's device work is stubbed out."""
    import torch

    from eosv import train

    monkeypatch.setattr(train, "lib", lambda: types.SimpleNamespace(eosv_bn_workspace_bytes=lambda c: 64))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    assert train.NativeTrainer("resnet18", 4).wino_wgrad_mask == 0
    assert train.NativeTrainer("resnet18", 4, winograd_wgrad=False).wino_wgrad_mask == 0
    assert train.NativeTrainer("resnet18", 4, winograd_wgrad=None).wino_wgrad_mask == 0
    assert train.NativeTrainer("resnet18", 4, winograd_wgrad=True).wino_wgrad_mask == train.TRAIN_WINO_WGRAD_DEFAULT
    assert 0 <= train.TRAIN_WINO_WGRAD_DEFAULT <= 15
    tr = train.NativeTrainer("resnet50", 4, winograd_wgrad=5)
    assert tr.wino_wgrad_mask == 5 and tr.wino_mask == 0 and tr.wino_wgrad_launches == 0 and tr.wino_launches == 0
    # the shared predicate on the new mask; the forward's eligibility follows `winograd` alone
    el = {c.name for c in tr._convs() if tr._wino_wgrad_eligible(c)}
    assert "convnet.4.0.conv2" in el and "convnet.6.1.conv2" in el
    assert "convnet.5.1.conv2" not in el and "convnet.6.0.conv2" not in el and "convnet.4.0.conv1" not in el
    assert not any(tr._wino_eligible(c) for c in tr._convs())
    tr = train.NativeTrainer("resnet18", 4, winograd=5, winograd_wgrad=0)
    assert tr.wino_mask == 5 and tr.wino_wgrad_mask == 0
    assert not any(tr._wino_wgrad_eligible(c) for c in tr._convs())
    tr = train.NativeTrainer("resnet18", 4, winograd=True, winograd_wgrad=9)
    assert tr.wino_mask == train.TRAIN_WINO_DEFAULT and tr.wino_wgrad_mask == 9
    for bad in (16, -1, "15", 1.0):
        with pytest.raises(ValueError):
            train.NativeTrainer("resnet18", 4, winograd_wgrad=bad)


def test_train_network_passes_train_winograd_wgrad_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_winograd_wgrad defaults to False and is read at finetune_model time; False
    passes no keyword at all (a trainer without it keeps working).  The instance is made without the
    constructor (it needs a device); the data set, the loader and NativeTrainer are recording stubs."""
    import network_train
    import torch

    assert network_train.TrainNetwork.train_winograd_wgrad is False
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
                           batch_size=2, lr_1=1e-4, lr_2=1e-3, lr_step_size=10, resnet_model="resnet18",
                           num_classes=64, mymodel=model)
        if value is not False:
            tn.train_winograd_wgrad = value
        tn.finetune_model()
    assert seen == [{}, {"winograd_wgrad": True}, {"winograd_wgrad": 6}]
    assert seen[1]["winograd_wgrad"] is True
