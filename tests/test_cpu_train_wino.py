"""The opt-in Winograd path of the training step, the parts that need no device: the C ABI exports
eosv_wino_weights_f32_device and validates its arguments before any device call, NativeTrainer
resolves its `winograd` argument to a stage mask, and the drop-in TrainNetwork hands its
`train_winograd` attribute to the trainer it builds."""
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


def test_library_exports_device_weight_transform():
    L = _library()
    assert hasattr(L, "eosv_wino_weights_f32_device")
    assert "eosv_wino_weights_f32_device" in _lib.EXPORTS


def test_device_weight_transform_rejects_before_any_device_call():
    """Bad shapes and null pointers return EOSV_ERR_ARG with a message; the checks come before the
    launch, so this runs without a device (the pointers are never dereferenced)."""
    L = _library()
    fn = L.eosv_wino_weights_f32_device
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.eosv_last_error.restype = ctypes.c_char_p
    p = 4096  # a non-null address
    for args in ((p, 32, 64, 0, p), (p, 64, 12, 0, p), (p, 64, 72, 1, p), (p, 12, 64, 1, p), (None, 64, 64, 0, p),
                 (p, 64, 64, 0, None), (p, 64, 64, 2, p), (p, 0, 64, 0, p)):
        assert fn(*args, None) == -1, args  # EOSV_ERR_ARG
        assert b"eosv_wino_weights_f32_device" in L.eosv_last_error(), args


def test_trainer_winograd_argument_resolves_to_a_mask(monkeypatch):
    """False / default -> 0, True -> TRAIN_WINO_DEFAULT, an int mask -> itself; anything else raises.
    The constructor's device work is stubbed out: only the argument handling runs."""
    import torch

    from eosv import train

    monkeypatch.setattr(train, "lib", lambda: types.SimpleNamespace(eosv_bn_workspace_bytes=lambda c: 64))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    assert train.NativeTrainer("resnet18", 4).wino_mask == 0
    assert train.NativeTrainer("resnet18", 4, winograd=False).wino_mask == 0
    assert train.NativeTrainer("resnet18", 4, winograd=True).wino_mask == train.TRAIN_WINO_DEFAULT
    assert 0 <= train.TRAIN_WINO_DEFAULT <= 15
    tr = train.NativeTrainer("resnet50", 4, winograd=5)
    assert tr.wino_mask == 5 and tr.wino_launches == 0
    # eligibility: stride-1 3x3 with cin = cout whose stage bit is set; R50 stage entries (stride 2) never
    el = {c.name for c in tr._convs() if tr._wino_eligible(c)}
    assert "convnet.4.0.conv2" in el and "convnet.6.1.conv2" in el
    assert "convnet.5.1.conv2" not in el and "convnet.6.0.conv2" not in el and "convnet.4.0.conv1" not in el
    for bad in (16, -1, "15", 1.0):
        with pytest.raises(ValueError):
            train.NativeTrainer("resnet18", 4, winograd=bad)


def test_train_network_passes_train_winograd_to_the_trainer(tmp_path, monkeypatch):
    """TrainNetwork.train_winograd defaults to False and is read at finetune_model time.  The
    constructor needs a device (model.cuda()), so the instance is made without it; the data set,
    the loader and NativeTrainer are recording stubs and no epoch runs."""
    import network_train
    import torch

    assert network_train.TrainNetwork.train_winograd is False
    seen = []

    class Stub:
        def __init__(self, arch, num_classes, device=0, winograd=False):
            seen.append((arch, num_classes, winograd))

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
            tn.train_winograd = value
        tn.finetune_model()
    assert seen == [("resnet18", 64, False), ("resnet18", 64, True), ("resnet18", 64, 6)]
