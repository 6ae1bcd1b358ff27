"""Host side of the Winograd F(2x2, 3x3) f32 path: eosv_wino_weights_f32 (no GPU needed)."""
import ctypes
import os

import numpy as np

from eosv import _lib

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


def _library():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.eosv_wino_weights_f32.restype = ctypes.c_int
    L.eosv_wino_weights_f32.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return L


def _transform(L, w, alpha):
    cout, cin = w.shape[:2]
    u = np.full(16 * cout * cin, np.nan, np.float32)
    rc = L.eosv_wino_weights_f32(w.ctypes.data, None if alpha is None else alpha.ctypes.data, cout, cin,
                                 u.ctypes.data)
    assert rc == 0
    return u


def _unpack(u, cout, cin):
    """The documented layout [cout / 64][cin / 8][16][8][64] -> [cout][cin][4][4]."""
    v = u.reshape(cout // 64, cin // 8, 16, 8, 64)      # (ob, ic, pos, i, o)
    return v.transpose(0, 4, 1, 3, 2).reshape(cout, cin, 4, 4)


def _reference(w, alpha):
    g = w if alpha is None else w * alpha[:, None, None, None]  # the float products of the fold
    assert g.dtype == np.float32
    return (G @ g.astype(np.float64) @ G.T).astype(np.float32)


def test_wino_weights_bitwise_equal_f64_transform():
    L = _library()
    rng = np.random.default_rng(7)
    w = rng.standard_normal((64, 64, 3, 3)).astype(np.float32)
    alpha = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    u = _unpack(_transform(L, w, alpha), 64, 64)
    ref = _reference(w, alpha)
    assert u.tobytes() == ref.tobytes()
    # no alpha: the weights themselves
    u1 = _unpack(_transform(L, w, None), 64, 64)
    assert u1.tobytes() == _reference(w, None).tobytes()


def test_wino_weights_layout_round_trip_128():
    """Every (cout, cin, position) of a 128-channel conv lands at its documented offset, once."""
    L = _library()
    cout = cin = 128
    # weight (o, i): centre tap = a code of (o, i), tap (0, 0) = -code; the corner positions
    # 0 / 3 / 12 / 15 of U are the corner taps, the others exact quarter sums
    code = (np.arange(cout)[:, None] * cin + np.arange(cin)[None, :] + 1).astype(np.float32)
    w = np.zeros((cout, cin, 3, 3), np.float32)
    w[:, :, 1, 1] = code
    w[:, :, 0, 0] = -code
    flat = _transform(L, w, None)
    assert not np.isnan(flat).any()          # every slot written
    u = _unpack(flat, cout, cin)
    assert np.array_equal(u[:, :, 0, 0], -code)          # position 0 = g[0][0]
    assert np.array_equal(u[:, :, 1, 1], np.zeros_like(code))  # (g00 + g11) / 4
    assert np.array_equal(u[:, :, 1, 2], -code / 2)            # (g00 - g11) / 4
    assert np.array_equal(u[:, :, 3, 3], np.zeros_like(code))  # g[2][2]
    assert u.tobytes() == _reference(w, None).tobytes()
    # explicit offsets of a few elements
    for o, i, pos in [(0, 0, 0), (63, 7, 15), (64, 8, 5), (127, 127, 10), (70, 33, 1)]:
        off = ((((o // 64) * (cin // 8) + i // 8) * 16 + pos) * 8 + i % 8) * 64 + o % 64
        assert flat[off] == _reference(w, None)[o, i, pos // 4, pos % 4]


def test_wino_weights_rejects_bad_shapes():
    L = _library()
    w = np.zeros((64, 64, 3, 3), np.float32)
    u = np.zeros(16 * 64 * 64, np.float32)
    assert L.eosv_wino_weights_f32(w.ctypes.data, None, 32, 64, u.ctypes.data) != 0
    assert L.eosv_wino_weights_f32(w.ctypes.data, None, 64, 12, u.ctypes.data) != 0
    assert L.eosv_wino_weights_f32(None, None, 64, 64, u.ctypes.data) != 0
