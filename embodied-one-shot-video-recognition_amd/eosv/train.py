"""Native training step for TrainNetwork.finetune_model.

Restates one iteration of the reference's loop (network_train.py:86-116) on the device:

    feature, output = model(video)                  # ResNet in train mode: batch-statistics BN
    feature = feature.view(b, T, -1).mean(dim=1)    # :100, :110
    output = model.fc(feature); loss = CrossEntropyLoss()(output, label)
    loss.backward(); optimizer_1.step(); optimizer_2.step()   # SGD(momentum=0.9): convnet / fc

with the f32 kernels of csrc/train.hip behind the C ABI (eosv_sgemm, eosv_im2col,
eosv_bn_train_forward, ...).  PyTorch only provides the device buffers; every arithmetic step
is a library call, and there is no CPU path.  Layouts: activations NHWC ([P][C] rows), conv
weights [Cout][KH][KW][Cin] (the state_dict's [Cout][Cin][KH][KW] permuted at load / export).

Each conv has three jobs, and each job an ordered tuple of routes, fixed at construction (_plan, c.routes)
and walked by _run: the first route the library does not refuse (EOSV_ERR_UNSUPPORTED) has done the job.
    fwd: stem, x3c, wino, x3, conv, gemm    wgrad: stem, x3, x3c, wino, conv, gemm    dgrad: x3, x3c, x3d, wino, conv, gemm

    route  forward                        weight gradient                 input gradient
    stem   eosv_stem_conv_f32 (NCHW)      eosv_stem_wgrad_f32             -
    wino   device U, eosv_conv_wino_f32   eosv_conv_wgrad_wino_f32        U with flip 1, shortcut gradient as residual
    x3     eosv_sgemm_x3 NT               eosv_sgemm_x3_tn_splitk         eosv_sgemm_x3 NN with the addend
    x3c    eosv_conv2d_x3                 eosv_conv_wgrad_x3              eosv_flip_weights, eosv_conv2d_x3 + residual (stride 1)
    x3d    -                              -                               eosv_flip_weights, eosv_conv_dgrad_x3 + residual (stride 2)
    conv   eosv_conv2d_f32 (split-K)      eosv_conv_wgrad_f32             eosv_flip_weights, eosv_conv2d_f32 + residual
    gemm   im2col*, eosv_sgemm            its buffer, eosv_sgemm_tn_splitk  eosv_sgemm NN, col2im*, axpy (*: not 1x1 s1)
stem, wino, x3, x3c and x3d are opt-in (the constants below); an eligible Winograd forward or input gradient is
its job's last route (alone, or after x3c where the caller asked for that arithmetic too); gemm takes every
conv and is last elsewhere.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from . import arch as _arch
from ._lib import EosvError, check, lib, stream_ptr
from ._lib import ptr as _f

BN_EPS = 1e-5
_UNSUPPORTED = -4  # EOSV_ERR_UNSUPPORTED
BN_MOMENTUM = 0.1
# NativeTrainer(winograd=True): the stages whose stride-1 3x3 convs take the Winograd F(2x2, 3x3)
# kernel (csrc/conv_wino_f32.hip) in the forward and the input gradient, one bit per channel count
# as the inference path's mask (1: 64, 2: 128, 4: 256, 8: 512).  A bit is set only where its stage
# beat the direct kernels at the training batch on both architectures: all four do (DESIGN 3T,
# profiles/train_wino_ab.txt).
TRAIN_WINO_DEFAULT = 15
_WINO_BIT = {64: 1, 128: 2, 256: 4, 512: 8}
# NativeTrainer(winograd_wgrad=True): the stages whose stride-1 3x3 convs take their weight gradient
# in the Winograd domain (csrc/conv_wgrad_wino_f32.hip), the same bits.  A bit is set only where its
# single-stage run beat the direct weight gradient at the training batch on both architectures
# (profiles/train_wino_wgrad_ab.txt); a stage that did not stays available through the mask.
# Stages 1-3 do; stage 4 (512 channels) wins on ResNet-18 but its two ResNet-50 convs gain less than
# the baseline's spread there.
TRAIN_WINO_WGRAD_DEFAULT = 7
# NativeTrainer(f32x3=True): the stages whose stride-1 1x1 convs (conv1 and conv3 of every bottleneck,
# the stride-1 downsample of layer 1) run their forward, input gradient and weight gradient on the
# f32x3 GEMMs (csrc/gemm_x3.hip).  Bit li is layer{li+1}: by stage, not by channel count (a stage's
# 1x1 convs have several).  A bit is set only where its single-stage run beat the f32 step by more
# than that step's run-to-run spread: all four do, plain and on top of the Winograd and stem
# switches (profiles/train_x3_ab.txt).
TRAIN_X3_DEFAULT = 15
# NativeTrainer(f32x3_convs=True): the stages whose other convs with cin % 32 == 0 (the 3x3 convs of
# either stride and the stride-2 1x1 shortcuts; never the stem, never a conv f32x3 owns) run their
# forward, weight gradient and stride-1 input gradient on the f32x3 implicit GEMMs (csrc/conv_x3.hip).
# Bit li is layer{li+1}.  A bit is set only where its single-stage run beat the f32 step by more than
# that step's run-to-run spread: all four do on both architectures.  On top of the Winograd switches
# stages 2-4 still gain and stage 1 does not (x3c takes the conv from Winograd there; DESIGN 3T,
# profiles/train_x3c_ab.txt).
TRAIN_X3C_DEFAULT = 15
# NativeTrainer(fused_bn_stats=True): the stages whose convs, where their forward runs on an f32x3 route
# (`x3`, `x3c`), take the first stage of the following BN (the per-channel sums in f64) in the conv's
# epilogue (the _stats entries of csrc/gemm_x3.hip and csrc/conv_x3.hip) instead of a pass of its own.
# Bit li is layer{li+1}.  A bit is set only where its single-stage run beat the run without the switch
# by more than that pair's run-to-run spread: stages 2-4 do on ResNet-50 (nothing leaves the spread on
# ResNet-18); stage 1, whose 1x1 GEMMs sit at their memory floor with two k-steps per tile, gains nothing
# alone.  All four together measured fastest (mask 15; DESIGN 3T, profiles/train_bnstats_ab.txt).
TRAIN_BNSTATS_DEFAULT = 14
# NativeTrainer(f32x3_dgrad=True): the stages whose stride-2 convs (the 3x3 entry conv and the 1x1 shortcut of
# layer{2,3,4}.0; layer 1 has none, so bit 0 selects nothing) run their input gradient on the f32x3
# implicit GEMM by parity class (csrc/conv_dgrad_x3.hip) instead of eosv_sgemm, the dcol buffer, col2im
# and axpy.  Bit li is layer{li+1}.  A bit is set only where that stage's slowest single-stage run beat
# the fastest run without the switch by more than the latter's three-run spread on both architectures
# (profiles/train_x3d_ab.txt); a stage that did not stays available through the mask.  Stages
# 2 and 3 do in the plain runs; stage 4 does on ResNet-50 but stays inside the spread on ResNet-18.  On top
# of every other switch no single stage cleared the spread of that session's parent runs, which was several
# times wider (one outlier), so those runs decide nothing either way.  The three together (mask 14) measured
# fastest, plain and stacked, well outside both spreads.
TRAIN_X3D_DEFAULT = 6


def _stage_mask(value, default, what):
    """A `winograd`-style argument as a stage mask: False / None -> 0, True -> default, an int 0..15."""
    if value is True:
        return default
    if value is False or value is None:
        return 0
    if not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 15:
        raise ValueError(f"NativeTrainer: {what} must be a bool or a stage mask 0..15, not {value!r}")
    return int(value)


@dataclass
class _Conv:
    name: str
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    w: torch.Tensor = None      # [Cout][K] with K = (kh, kw, cin)
    g: torch.Tensor = None
    buf: torch.Tensor = None
    x3: bool = False            # its GEMMs run in f32x3 (NativeTrainer(f32x3=...))
    x3c: bool = False           # its implicit GEMMs run in f32x3 (NativeTrainer(f32x3_convs=...))
    x3d: bool = False           # stride 2: its input gradient runs in f32x3 (NativeTrainer(f32x3_dgrad=...))
    stats: bool = False         # an f32x3 forward of it also writes its BN's batch sums (NativeTrainer(fused_bn_stats=...))
    routes: Dict[str, tuple] = None  # {"fwd", "wgrad", "dgrad"}: the routes it may take, in order (_plan)

    @property
    def K(self):
        return self.k * self.k * self.cin

    @property
    def direct(self):  # stride-1 1x1: the conv's im2col matrix is its input
        return self.k == 1 and self.stride == 1

    def out_shape(self, shape):  # NHWC, of the output over an NHWC input of `shape`
        N, H, W, _ = shape
        return (N, (H + 2 * self.pad - self.k) // self.stride + 1, (W + 2 * self.pad - self.k) // self.stride + 1,
                self.cout)


@dataclass
class _BN:
    name: str
    c: int
    gamma: torch.Tensor = None
    beta: torch.Tensor = None
    rm: torch.Tensor = None
    rv: torch.Tensor = None
    nbt: int = 0
    dgamma: torch.Tensor = None
    dbeta: torch.Tensor = None
    buf_g: torch.Tensor = None
    buf_b: torch.Tensor = None


@dataclass
class _Block:
    convs: List[_Conv]
    bns: List[_BN]
    ds: Optional[_Conv] = None
    ds_bn: Optional[_BN] = None
    saved: Dict[str, object] = field(default_factory=dict)


class NativeTrainer:
    """ResNet-18/50 + fc trained with the reference's recipe (network_train.py:75-79)."""

    def __init__(self, arch: str = "resnet50", num_classes: int = 64, device: int = 0, winograd=False,
                 winograd_wgrad=False, stem_direct=False, f32x3=False, f32x3_convs=False, fused_bn_stats=False,
                 f32x3_dgrad=False):
        """winograd: False (default) every conv on the direct kernels; True the stages of
        TRAIN_WINO_DEFAULT, or an int mask (1: 64, 2: 128, 4: 256, 8: 512 channels), on the Winograd
        kernel for the forward and the input gradient of their stride-1 3x3 convs.
        winograd_wgrad: the same form (True: TRAIN_WINO_WGRAD_DEFAULT) for the weight gradient of
        those convs; independent of `winograd`.
        stem_direct: a bool.  True runs the stem's forward and weight gradient on the direct 7x7
        kernels (csrc/stem_train_f32.hip) from the NCHW frames; a frame size they do not take
        (W % 4 != 0, W > 256) falls back to the im2col path, call by call.
        f32x3: False (default), True (the stages of TRAIN_X3_DEFAULT) or an int mask whose bit li
        enables layer{li+1}: the stride-1 1x1 convs of those stages run their forward, input gradient
        and weight gradient in f32x3 arithmetic (about 2^-16 relative per product instead of 2^-24);
        a call the f32x3 GEMM does not take falls back to the f32 path.  ResNet-18 has no such conv.
        f32x3_convs: the same form (True: TRAIN_X3C_DEFAULT) for the other convs of those stages with
        cin % 32 == 0, the 3x3 convs of either stride and the stride-2 1x1 shortcuts: forward, weight
        gradient and stride-1 input gradient on the f32x3 implicit GEMMs (the stride-2 input gradients
        are f32x3_dgrad's).  Independent of the other switches; where a conv is also Winograd-eligible, the
        f32x3 kernel takes it and Winograd only what that kernel refuses.
        fused_bn_stats: the same form (True: TRAIN_BNSTATS_DEFAULT).  A conv of an enabled stage whose
        forward runs on an f32x3 route (`x3` or `x3c`: set those switches too) writes the batch sums of
        the following BN from its epilogue, and that BN skips its first pass; the sums are the same
        f64 arithmetic in another order.  A conv on any other route, and the stem, are not affected.
        f32x3_dgrad: the same form (True: TRAIN_X3D_DEFAULT) for the input gradient of the stride-2 convs
        of those stages (cout % 32 == 0 and cin % 64 == 0: the 3x3 entry conv and the 1x1 shortcut of
        layer{2,3,4}.0, six per step in either architecture; bit 0 selects nothing): one f32x3 implicit
        GEMM by parity class with the residual gradient in its epilogue instead of the f32 GEMM, its
        dcol buffer, col2im and axpy.  Independent of every other switch; a call the kernel refuses falls
        back to that f32 path."""
        if not isinstance(stem_direct, (bool, np.bool_)):
            raise ValueError(f"NativeTrainer: stem_direct must be a bool, not {stem_direct!r}")
        self.stem_direct = bool(stem_direct)
        self.stem_direct_launches = 0  # direct stem launches (forward + weight gradient) of the last step
        self.wino_mask = _stage_mask(winograd, TRAIN_WINO_DEFAULT, "winograd")
        self.wino_wgrad_mask = _stage_mask(winograd_wgrad, TRAIN_WINO_WGRAD_DEFAULT, "winograd_wgrad")
        self.wino_launches = 0  # Winograd conv launches (forward + input gradient) of the last step
        self.wino_wgrad_launches = 0  # Winograd weight-gradient launches of the last step
        self.x3_mask = _stage_mask(f32x3, TRAIN_X3_DEFAULT, "f32x3")
        self.x3_launches = 0  # f32x3 GEMM launches of the last step (the slice sums not counted)
        self.x3c_mask = _stage_mask(f32x3_convs, TRAIN_X3C_DEFAULT, "f32x3_convs")
        self.x3c_launches = 0  # f32x3 implicit-GEMM launches of the last step (slice sums, weight flips not counted)
        self.bnstats_mask = _stage_mask(fused_bn_stats, TRAIN_BNSTATS_DEFAULT, "fused_bn_stats")
        self.x3d_mask = _stage_mask(f32x3_dgrad, TRAIN_X3D_DEFAULT, "f32x3_dgrad")
        self.x3d_launches = 0  # f32x3 strided input-gradient launches of the last step (weight flips not counted)
        self.bn_fused_launches = 0  # BN forwards of the last step that started from a conv epilogue's sums
        self._fwd_stats = None  # (buffer, chunks) of the last _conv_fwd when its route wrote the BN's sums
        self.spec = _arch.SPECS[arch]
        self.num_classes = num_classes
        self.dev = torch.device("cuda", device)
        self.L = lib()
        self.stem = _Conv("convnet.0", 3, 64, 7, 2, 3)
        self.stem_bn = _BN("convnet.1", 64)
        self.blocks: List[_Block] = []
        inplanes = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), self.spec.layers)):
            for bi in range(n):
                stride = 2 if (li > 0 and bi == 0) else 1
                p = f"convnet.{4 + li}.{bi}"
                if self.spec.block == "basic":
                    convs = [_Conv(p + ".conv1", inplanes, planes, 3, stride, 1),
                             _Conv(p + ".conv2", planes, planes, 3, 1, 1)]
                    bns = [_BN(p + ".bn1", planes), _BN(p + ".bn2", planes)]
                else:
                    convs = [_Conv(p + ".conv1", inplanes, planes, 1, 1, 0),
                             _Conv(p + ".conv2", planes, planes, 3, stride, 1),
                             _Conv(p + ".conv3", planes, planes * 4, 1, 1, 0)]
                    bns = [_BN(p + ".bn1", planes), _BN(p + ".bn2", planes), _BN(p + ".bn3", planes * 4)]
                cout = planes * self.spec.expansion
                blk = _Block(convs, bns)
                if bi == 0 and (stride != 1 or inplanes != cout):
                    blk.ds = _Conv(p + ".downsample.0", inplanes, cout, 1, stride, 0)
                    blk.ds_bn = _BN(p + ".downsample.1", cout)
                if self.x3_mask >> li & 1:
                    for c in convs + ([blk.ds] if blk.ds is not None else []):
                        c.x3 = c.direct
                if self.x3c_mask >> li & 1:
                    for c in convs + ([blk.ds] if blk.ds is not None else []):
                        c.x3c = c.cin % 32 == 0 and not c.direct
                if self.x3d_mask >> li & 1:
                    for c in convs + ([blk.ds] if blk.ds is not None else []):
                        c.x3d = c.stride == 2 and c.cout % 32 == 0 and c.cin % 64 == 0
                if self.bnstats_mask >> li & 1:
                    for c in convs + ([blk.ds] if blk.ds is not None else []):
                        c.stats = True
                self.blocks.append(blk)
                inplanes = cout
        self.D = inplanes
        for c in self._convs():
            c.routes = self._plan(c)
        self.fc_w = self.fc_b = None
        self.step_count = 0
        self._scratch: Dict[str, torch.Tensor] = {}
        self._col_key = None  # what the "col" scratch holds (_im2col); reset by every step
        self._x0 = None  # the NHWC copy of the step's frames (_nhwc_frames); lives for one step
        # the BN backward's ReLU mask from 1-byte forward masks (r05) or from y (EOSV_TRAIN_RELU_MASK=0, A/B)
        self._relu_mask = os.environ.get("EOSV_TRAIN_RELU_MASK", "1") != "0"
        self.work = torch.empty(int(self.L.eosv_bn_workspace_bytes(2048)) // 4 + 4, dtype=torch.float32,
                                device=self.dev)

    # ------------------------------------------------------------------ parameters
    def _convs(self):
        yield self.stem
        for b in self.blocks:
            yield from b.convs
            if b.ds is not None:
                yield b.ds

    def _bns(self):
        yield self.stem_bn
        for b in self.blocks:
            yield from b.bns
            if b.ds_bn is not None:
                yield b.ds_bn

    def load_state_dict(self, sd: Dict[str, object]):
        """The reference model's state_dict (numpy arrays or tensors, any device)."""
        def t(name):
            v = sd[name]
            v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            return v.detach().to(self.dev, torch.float32).contiguous()

        # optimizer_1's parameters (convnet: conv weights, BN gamma / beta) live in one flat buffer
        # (each tensor 16-byte aligned), with flat gradient and momentum buffers: one SGD launch
        sizes = [c.cout * c.K for c in self._convs()] + [b.c for b in self._bns() for _ in range(2)]
        total = sum((n + 3) // 4 * 4 for n in sizes)
        self.p_flat = torch.zeros(total, dtype=torch.float32, device=self.dev)
        self.g_flat = torch.zeros_like(self.p_flat)
        self.m_flat = torch.zeros_like(self.p_flat)
        off = [0]

        def views(n):
            o = off[0]
            off[0] += (n + 3) // 4 * 4
            return self.p_flat[o:o + n], self.g_flat[o:o + n], self.m_flat[o:o + n]

        for c in self._convs():
            w = t(c.name + ".weight")                       # [Cout][Cin][KH][KW]
            p, g, m = views(c.cout * c.K)
            p.copy_(w.permute(0, 2, 3, 1).reshape(-1))
            c.w, c.g, c.buf = p.view(c.cout, c.K), g.view(c.cout, c.K), m.view(c.cout, c.K)
        for b in self._bns():
            b.gamma, b.dgamma, b.buf_g = views(b.c)
            b.beta, b.dbeta, b.buf_b = views(b.c)
            b.gamma.copy_(t(b.name + ".weight"))
            b.beta.copy_(t(b.name + ".bias"))
            b.rm, b.rv = t(b.name + ".running_mean"), t(b.name + ".running_var")
            nbt = sd.get(b.name + ".num_batches_tracked", 0)
            b.nbt = int(nbt.item() if isinstance(nbt, torch.Tensor) else np.asarray(nbt))
        self.fc_w, self.fc_b = t("fc.weight"), t("fc.bias")
        self.fc_gw, self.fc_gb = torch.zeros_like(self.fc_w), torch.zeros_like(self.fc_b)
        self.fc_bw, self.fc_bb = torch.zeros_like(self.fc_w), torch.zeros_like(self.fc_b)
        self.step_count = 0

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's state_dict layout, on the CPU (torch.save, network_train.py:131)."""
        out = {}
        for c in self._convs():
            out[c.name + ".weight"] = c.w.view(c.cout, c.k, c.k, c.cin).permute(0, 3, 1, 2).contiguous().cpu()
        for b in self._bns():
            out[b.name + ".weight"] = b.gamma.cpu()
            out[b.name + ".bias"] = b.beta.cpu()
            out[b.name + ".running_mean"] = b.rm.cpu()
            out[b.name + ".running_var"] = b.rv.cpu()
            out[b.name + ".num_batches_tracked"] = torch.tensor(b.nbt, dtype=torch.int64)
        out["fc.weight"] = self.fc_w.cpu()
        out["fc.bias"] = self.fc_b.cpu()
        return out

    # ------------------------------------------------------------------ building blocks
    def _buf(self, key, n):
        t = self._scratch.get(key)
        if t is None or t.numel() < n:
            t = torch.empty(n, dtype=torch.float32, device=self.dev)
            self._scratch[key] = t
        return t[:n]

    def _ws(self, key, nbytes, pad=4):
        """(pointer, bytes) of a kernel's workspace of `nbytes`, kept under the scratch key `key`."""
        return _f(self._buf(key, int(nbytes) // 4 + pad)), int(nbytes)

    def _im2col(self, x, shape, c: _Conv, P, s):
        """The explicit im2col buffer of conv c over x (the stem: Cin = 3).  The forward's buffer is
        kept and the weight gradient of the same step reuses it instead of gathering it again
        (r05: 0.71 GB and one 0.2 ms pass per step at R50 / 96 frames): every write of the
        buffer goes through here and records what it holds."""
        col = self._buf("col", P * c.K)
        key = (id(c), x.data_ptr(), tuple(shape), col.data_ptr())
        if self._col_key != key:
            check(self.L.eosv_im2col(_f(x), *shape, c.k, c.k, c.stride, c.pad, _f(col), s), "eosv_im2col")
            self._col_key = key
        return col

    @staticmethod
    def _wino_shape(c: _Conv, mask: int) -> bool:
        """A stride-1 pad-1 3x3 conv with cin = cout whose stage bit is set in `mask`."""
        return (c.k == 3 and c.stride == 1 and c.pad == 1 and c.cin == c.cout and c.cin % 64 == 0
                and bool(mask & _WINO_BIT.get(c.cin, 0)))

    def _wino_eligible(self, c: _Conv) -> bool:
        return "wino" in c.routes["fwd"]

    def _wino_wgrad_eligible(self, c: _Conv) -> bool:
        return "wino" in c.routes["wgrad"]

    def _plan(self, c: _Conv):
        """Static eligibility, resolved once: per job the routes c may take, in the order _run tries them."""
        stem, wino = c is self.stem and self.stem_direct, self._wino_shape(c, self.wino_mask)
        same = c.stride == 1 and c.k % 2 == 1 and c.pad == c.k // 2  # the input gradient is a conv of dz
        cand = {"fwd": (("stem", stem), ("x3c", c.x3c), ("x3", c.x3), ("conv", True)),
                "wgrad": (("stem", stem), ("x3", c.x3), ("x3c", c.x3c),
                          ("wino", self._wino_shape(c, self.wino_wgrad_mask)), ("conv", c.cin % 4 == 0 and not c.direct)),
                "dgrad": (("x3", c.x3), ("x3c", c.x3c and same), ("x3d", c.x3d), ("conv", same))}
        plan = {job: tuple(name for name, ok in v if ok) + ("gemm",) for job, v in cand.items()}
        if wino:  # the Winograd forward and input gradient do not fall through: a refusal raises
            plan["fwd"] = plan["dgrad"] = (("x3c",) if c.x3c else ()) + ("wino",)
        return dict(plan, dgrad=()) if c is self.stem else plan

    def _run(self, job, c: _Conv, x, shape, dz, out, acc, s):
        """Does one job of conv c on the first of c.routes[job] that the library takes.  A route is
        _{job}_{name}(c, x, shape, P, dz, out, acc, s), P the output's rows, and returns (status, library
        function) of its deciding call: EOSV_ERR_UNSUPPORTED from any but the last moves on, any other
        failure raises.  A forward route that also wrote the following BN's batch sums returns them as a
        third item, (buffer, chunks); _run returns the winner's, or None.  The stem's x is the step's NCHW frames, which only its `stem` routes read as such."""
        names = c.routes[job]
        N, Ho, Wo, _ = c.out_shape(shape)
        for name in names:
            if c is self.stem and name != "stem":
                x = self._nhwc_frames(x, shape, s)
            rc, fn, *stats = getattr(self, f"_{job}_{name}")(c, x, shape, N * Ho * Wo, dz, out, acc, s)
            if rc != _UNSUPPORTED or name == names[-1]:
                check(rc, fn)
                n = {"stem": "stem_direct", "x3": "x3", "x3c": "x3c", "x3d": "x3d",
                     "wino": "wino_wgrad" if job == "wgrad" else "wino"}.get(name)
                if n:  # the launch counter of the family that ran; conv and gemm keep none
                    setattr(self, n + "_launches", getattr(self, n + "_launches") + 1)
                return stats[0] if stats else None
        raise EosvError(f"NativeTrainer: {c.name} has no {job} route")

    def _nhwc_frames(self, frames, shape, s):
        """The NHWC copy of the step's frames, made by the first generic stem route that needs it."""
        if self._x0 is None:
            N, H, W, C = shape
            self._x0 = torch.empty(N * H * W * C, dtype=torch.float32, device=self.dev)
            check(self.L.eosv_nchw_to_nhwc(_f(frames), N, C, H, W, _f(self._x0), s), "eosv_nchw_to_nhwc")
        return self._x0

    def _conv_fwd(self, x, shape, c: _Conv, s):
        oshape = c.out_shape(shape)
        y = torch.empty(oshape[0] * oshape[1] * oshape[2] * c.cout, dtype=torch.float32, device=self.dev)
        # what the BN behind this conv starts from: consumed at once (_bn_fwd), so one buffer serves the net
        self._fwd_stats = self._run("fwd", c, x, shape, None, y, None, s)
        return y, oshape

    def _conv_bwd(self, dz, x, shape, c: _Conv, s, need_dx=True, acc=None):
        """dW = dz^T . col(x); returns dx = col2im(dz . W) (NHWC, shape of x) when need_dx, plus
        acc (same shape) when given -- fused into the conv epilogue on the fast path."""
        self._run("wgrad", c, x, shape, dz, None, None, s)
        if not need_dx:
            return None
        dx = torch.empty(shape[0] * shape[1] * shape[2] * c.cin, dtype=torch.float32, device=self.dev)
        self._run("dgrad", c, None, shape, dz, dx, acc, s)
        return dx

    # ---- forward routes: y = conv(x, w); `shape` = (N, H, W, Cin) is the conv input's in every route
    def _fwd_stem(self, c, x, shape, P, dz, y, acc, s):
        return self.L.eosv_stem_conv_f32(_f(x), *shape[:3], _f(c.w), _f(y), s), "eosv_stem_conv_f32"

    def _fwd_wino(self, c, x, shape, P, dz, y, acc, s, flip=0):
        """y = conv3x3(x, w) (flip 0) or the input gradient conv3x3(x = dz, w rotated and transposed)
        + acc (flip 1) on the Winograd kernel.  U is transformed on the device from the current
        weights into one scratch buffer, used by this launch only (stream order) and never kept."""
        u = self._buf("wino_u", 16 * c.cin * c.cin)
        check(self.L.eosv_wino_weights_f32_device(_f(c.w), c.cout, c.cin, flip, _f(u), s),
              "eosv_wino_weights_f32_device")
        return self.L.eosv_conv_wino_f32(_f(x), _f(u), None, _f(acc), 0, _f(y), *shape, s), "eosv_conv_wino_f32"

    def _stats_buf(self, cout, chunks):
        """(pointer, bytes, hand-off) of the [chunks][2][cout] f64 batch sums a _stats entry writes."""
        st = self._buf("bnstats", chunks * 2 * cout * 2)
        return _f(st), chunks * 2 * cout * 8, (st, chunks)

    def _fwd_x3(self, c, x, shape, P, dz, y, acc, s):
        if c.stats:
            chunks = self.L.eosv_sgemm_x3_stats_chunks(P, c.cout, c.cin)
            if chunks < 1:  # a shape the entry refuses
                return _UNSUPPORTED, "eosv_sgemm_x3_stats"
            sp, sb, hand = self._stats_buf(c.cout, chunks)
            return self.L.eosv_sgemm_x3_stats(P, c.cout, c.cin, _f(x), c.cin, _f(c.w), c.cin, _f(y), c.cout, sp, sb,
                                              s), "eosv_sgemm_x3_stats", hand
        return self.L.eosv_sgemm_x3(0, 1, P, c.cout, c.cin, 1.0, _f(x), c.cin, _f(c.w), c.cin, 0.0, _f(y), c.cout,
                                    None, s), "eosv_sgemm_x3"

    def _fwd_x3c(self, c, x, shape, P, dz, y, acc, s):
        if c.stats:
            chunks = self.L.eosv_conv2d_x3_stats_chunks(*shape, c.cout, c.k, c.k, c.stride, c.pad)
            if chunks < 1:  # a shape the entry refuses
                return _UNSUPPORTED, "eosv_conv2d_x3_stats"
            sp, sb, hand = self._stats_buf(c.cout, chunks)
            return self.L.eosv_conv2d_x3_stats(_f(x), *shape, _f(c.w), c.cout, c.k, c.k, c.stride, c.pad, _f(y), sp,
                                               sb, s), "eosv_conv2d_x3_stats", hand
        return self.L.eosv_conv2d_x3(_f(x), *shape, _f(c.w), c.cout, c.k, c.k, c.stride, c.pad, None, _f(y),
                                     s), "eosv_conv2d_x3"

    def _fwd_conv(self, c, x, shape, P, dz, y, acc, s):
        # the inference conv kernels (exact-f32 MFMA) where they apply
        kw, kb = self._ws("ksplit", self.L.eosv_conv2d_f32_workspace(*shape, c.cout, c.k, c.k, c.stride, c.pad))
        return self.L.eosv_conv2d_f32(_f(x), *shape, _f(c.w), c.cout, c.k, c.k, c.stride, c.pad, None, None, 0, _f(y),
                                      kw, kb, s), "eosv_conv2d_f32"

    def _fwd_gemm(self, c, x, shape, P, dz, y, acc, s):
        col = x if c.direct else self._im2col(x, shape, c, P, s)
        return self.L.eosv_sgemm(0, 1, P, c.cout, c.K, 1.0, _f(col), c.K, _f(c.w), c.K, 0.0, _f(y), c.cout,
                                 s), "eosv_sgemm"

    # ---- weight-gradient routes: c.g = dz^T . col(x)
    def _wgrad_stem(self, c, x, shape, P, dz, out, acc, s):
        ws, wb = self._ws("stem_wgrad", self.L.eosv_stem_wgrad_f32_workspace(*shape[:3]))
        return self.L.eosv_stem_wgrad_f32(_f(x), _f(dz), *shape[:3], _f(c.g), ws, wb, s), "eosv_stem_wgrad_f32"

    def _wgrad_x3(self, c, x, shape, P, dz, out, acc, s):
        # dW = dz^T X in f32x3, the reduction over P split into slices
        ws, wb = self._ws("splitk", self.L.eosv_sgemm_x3_tn_splitk_workspace(c.cout, c.cin, P))
        return self.L.eosv_sgemm_x3_tn_splitk(c.cout, c.cin, P, _f(dz), c.cout, _f(x), c.cin, _f(c.g), c.cin,
                                              ws if wb else None, wb, s), "eosv_sgemm_x3_tn_splitk"

    def _wgrad_x3c(self, c, x, shape, P, dz, out, acc, s):
        # the implicit GEMM dW = dz^T col(x) in f32x3, the reduction over P split into slices
        ws, wb = self._ws("splitk", self.L.eosv_conv_wgrad_x3_workspace(*shape, c.cout, c.k, c.k, c.stride, c.pad))
        return self.L.eosv_conv_wgrad_x3(_f(x), *shape, _f(dz), c.cout, c.k, c.k, c.stride, c.pad, _f(c.g),
                                         ws if wb else None, wb, s), "eosv_conv_wgrad_x3"

    def _wgrad_wino(self, c, x, shape, P, dz, out, acc, s):
        ws, wb = self._ws("wino_wgrad", self.L.eosv_conv_wgrad_wino_f32_workspace(*shape))
        return self.L.eosv_conv_wgrad_wino_f32(_f(x), _f(dz), *shape, _f(c.g), ws, wb, s), "eosv_conv_wgrad_wino_f32"

    def _wgrad_conv(self, c, x, shape, P, dz, out, acc, s):
        # KxK and strided 1x1: implicit GEMM, no im2col buffer (a stride-1 1x1's X is the GEMM's operand as it is)
        ws, wb = self._ws("splitk", self.L.eosv_conv_wgrad_f32_workspace(*shape, c.cout, c.k, c.k, c.stride, c.pad))
        return self.L.eosv_conv_wgrad_f32(_f(x), *shape, _f(dz), c.cout, c.k, c.k, c.stride, c.pad, _f(c.g), ws, wb,
                                          s), "eosv_conv_wgrad_f32"

    def _wgrad_gemm(self, c, x, shape, P, dz, out, acc, s):
        col = x if c.direct else self._im2col(x, shape, c, P, s)
        ws, wb = self._ws("splitk", self.L.eosv_sgemm_tn_splitk_workspace(c.cout, c.K, P), pad=1)
        return self.L.eosv_sgemm_tn_splitk(c.cout, c.K, P, _f(dz), c.cout, _f(col), c.K, _f(c.g), c.K, ws, wb,
                                           s), "eosv_sgemm_tn_splitk"

    # ---- input-gradient routes: dx = col2im(dz . W) + acc; x is not read
    def _dgrad_x3(self, c, x, shape, P, dz, dx, acc, s):
        # dx = dz W + acc in f32x3, the residual gradient added in the epilogue
        return self.L.eosv_sgemm_x3(0, 0, P, c.cin, c.cout, 1.0, _f(dz), c.cout, _f(c.w), c.cin, 0.0, _f(dx), c.cin,
                                    _f(acc), s), "eosv_sgemm_x3"

    def _dgrad_x3c(self, c, x, shape, P, dz, dx, acc, s):
        # stride 1: dx = conv(dz, W flipped and transposed) + acc in f32x3, the residual gradient in the epilogue
        N, Ho, Wo, _ = c.out_shape(shape)
        wf = self._buf("wflip", c.cout * c.K)
        check(self.L.eosv_flip_weights(_f(c.w), c.cout, c.k, c.k, c.cin, _f(wf), s), "eosv_flip_weights")
        return self.L.eosv_conv2d_x3(_f(dz), N, Ho, Wo, c.cout, _f(wf), c.cin, c.k, c.k, 1, c.pad, _f(acc), _f(dx),
                                     s), "eosv_conv2d_x3"

    def _dgrad_x3d(self, c, x, shape, P, dz, dx, acc, s):
        # stride 2: dx = the parity-class gather of dz against the flipped weights + acc in f32x3, no dcol buffer
        wf = self._buf("wflip", c.cout * c.K)
        check(self.L.eosv_flip_weights(_f(c.w), c.cout, c.k, c.k, c.cin, _f(wf), s), "eosv_flip_weights")
        return self.L.eosv_conv_dgrad_x3(_f(dz), *shape, _f(wf), c.cout, c.k, c.k, c.stride, c.pad, _f(acc), _f(dx),
                                         s), "eosv_conv_dgrad_x3"

    def _dgrad_wino(self, c, x, shape, P, dz, dx, acc, s):
        # dx = conv(dz, W rotated and transposed) + acc: U comes straight from W, no flipped copy
        return self._fwd_wino(c, dz, c.out_shape(shape), P, None, dx, acc, s, flip=1)

    def _dgrad_conv(self, c, x, shape, P, dz, dx, acc, s):
        # stride 1: dx = conv(dz, W flipped and transposed) on the inference conv kernels
        N, Ho, Wo, _ = c.out_shape(shape)
        wf = self._buf("wflip", c.cout * c.K)
        check(self.L.eosv_flip_weights(_f(c.w), c.cout, c.k, c.k, c.cin, _f(wf), s), "eosv_flip_weights")
        kw, kb = self._ws("ksplit", self.L.eosv_conv2d_f32_workspace(N, Ho, Wo, c.cout, c.cin, c.k, c.k, 1, c.pad))
        return self.L.eosv_conv2d_f32(_f(dz), N, Ho, Wo, c.cout, _f(wf), c.cin, c.k, c.k, 1, c.pad, None, _f(acc),
                                      0, _f(dx), kw, kb, s), "eosv_conv2d_f32"

    def _dgrad_gemm(self, c, x, shape, P, dz, dx, acc, s):
        dcol = dx if c.direct else self._buf("dcol", P * c.K)
        check(self.L.eosv_sgemm(0, 0, P, c.K, c.cout, 1.0, _f(dz), c.cout, _f(c.w), c.K, 0.0, _f(dcol), c.K, s),
              "eosv_sgemm")
        if not c.direct:
            check(self.L.eosv_col2im(_f(dcol), *shape, c.k, c.k, c.stride, c.pad, _f(dx), s), "eosv_col2im")
        return (self.L.eosv_axpy(_f(dx), _f(acc), dx.numel(), 1.0, s) if acc is not None else 0), "eosv_axpy"

    def _bn_fwd(self, z, P, b: _BN, relu, res, s, stats=None):
        """Returns y and the backward's saved state: mean, 1/std and, with the ReLU, its mask (one
        byte per element: the backward reads it instead of y, r05).  stats: (buffer, chunks) of z's
        batch sums where the conv's epilogue wrote them (_conv_fwd): the first pass is then skipped."""
        y = torch.empty_like(z)
        mean = torch.empty(b.c, dtype=torch.float32, device=self.dev)
        invstd = torch.empty_like(mean)
        mask = torch.empty(z.numel(), dtype=torch.uint8, device=self.dev) if relu and self._relu_mask else None
        if stats is not None:
            check(self.L.eosv_bn_train_forward_stats(_f(z), P, b.c, _f(stats[0]), stats[1], _f(b.gamma), _f(b.beta),
                                                     BN_EPS, BN_MOMENTUM, _f(b.rm), _f(b.rv), _f(res), int(relu),
                                                     _f(y), _f(mask), _f(mean), _f(invstd), s),
                  "eosv_bn_train_forward_stats")
            self.bn_fused_launches += 1
        else:
            check(self.L.eosv_bn_train_forward(_f(z), P, b.c, _f(b.gamma), _f(b.beta), BN_EPS, BN_MOMENTUM, _f(b.rm),
                                               _f(b.rv), _f(res), int(relu), _f(y), _f(mask), _f(mean), _f(invstd),
                                               _f(self.work), s), "eosv_bn_train_forward")
        b.nbt += 1
        return y, (mean, invstd, mask)

    def _bn_bwd(self, dy, y, relu, z, P, b: _BN, stats, s, want_dres=False):
        dz = torch.empty_like(z)
        dres = torch.empty_like(z) if want_dres else None
        mask = stats[2] if relu else None  # None without the forward's mask: y is read
        check(self.L.eosv_bn_train_backward(_f(dy), None if mask is not None else _f(y), _f(mask), int(relu), _f(z),
                                            P, b.c, _f(b.gamma), _f(stats[0]), _f(stats[1]), _f(dz), _f(b.dgamma),
                                            _f(b.dbeta), _f(dres), _f(self.work), s), "eosv_bn_train_backward")
        return dz, dres

    # ------------------------------------------------------------------ one iteration
    def step(self, frames: torch.Tensor, labels, T: int, lr_conv: float, lr_fc: float, momentum: float = 0.9):
        """frames [B*T, 3, H, W] f32 (clip-major, as video.view(-1, 3, H, W)), labels [B] ints.
        Runs forward, loss, backward and both SGD updates; returns (loss, logits [B, C])."""
        if self.fc_w is None:
            raise RuntimeError("NativeTrainer.step: load_state_dict first")
        frames = frames.to(self.dev, torch.float32).contiguous()
        self._col_key = self._x0 = None  # new frames (possibly at the same address): the forward gathers afresh
        self.wino_launches = self.wino_wgrad_launches = self.stem_direct_launches = self.x3_launches = 0
        self.x3c_launches = self.bn_fused_launches = self.x3d_launches = 0
        NT, _, H, W = frames.shape
        if NT % T:
            raise ValueError("frames must be B*T clip-major rows")
        B = NT // T
        lab_h = np.asarray(labels).reshape(-1).astype(np.int64)
        if lab_h.size != B:
            raise ValueError("one label per clip")
        C = int(self.fc_w.shape[0])
        if lab_h.size and (lab_h.min() < 0 or lab_h.max() >= C):
            # nn.CrossEntropyLoss (network_train.py:85) raises on such a target
            raise ValueError(f"NativeTrainer.step: label out of range [0, {C}): "
                             f"min {int(lab_h.min())}, max {int(lab_h.max())} (num_classes too small for the list?)")
        lab = torch.as_tensor(lab_h.astype(np.int32), device=self.dev)
        s = stream_ptr()
        L = self.L
        # ---- forward
        shp0 = (NT, H, W, 3)  # the stem is handed the NCHW frames (_run)
        z0, shp1 = self._conv_fwd(frames, shp0, self.stem, s)
        P1 = shp1[0] * shp1[1] * shp1[2]
        a0, st0 = self._bn_fwd(z0, P1, self.stem_bn, True, None, s)
        Hq, Wq = (shp1[1] - 1) // 2 + 1, (shp1[2] - 1) // 2 + 1
        h = torch.empty(NT * Hq * Wq * 64, dtype=torch.float32, device=self.dev)
        idx = torch.empty(NT * Hq * Wq * 64, dtype=torch.int32, device=self.dev)
        check(L.eosv_maxpool_forward(_f(a0), shp1[0], shp1[1], shp1[2], 64, _f(h), _f(idx), s), "eosv_maxpool_forward")
        shp = (NT, Hq, Wq, 64)
        for blk in self.blocks:
            sv = blk.saved = {"x": h, "shape": shp, "z": [], "y": [], "st": [], "in": [], "inshape": []}
            cur, cshp = h, shp
            nl = len(blk.convs)
            if blk.ds is not None:
                zd, dshp = self._conv_fwd(h, shp, blk.ds, s)
                Pd = dshp[0] * dshp[1] * dshp[2]
                sc, std = self._bn_fwd(zd, Pd, blk.ds_bn, False, None, s, stats=self._fwd_stats)
                sv["ds"] = (zd, sc, std, Pd)
            else:
                sc = h
            for i, (c, b) in enumerate(zip(blk.convs, blk.bns)):
                z, oshp = self._conv_fwd(cur, cshp, c, s)
                P = oshp[0] * oshp[1] * oshp[2]
                last = i == nl - 1
                y, st = self._bn_fwd(z, P, b, True, sc if last else None, s, stats=self._fwd_stats)
                sv["in"].append(cur)
                sv["inshape"].append(cshp)
                sv["z"].append(z)
                sv["y"].append(y)
                sv["st"].append((st, P))
                cur, cshp = y, oshp
            h, shp = cur, cshp
        N4, H4, W4, D = shp
        feat = torch.empty(N4 * D, dtype=torch.float32, device=self.dev)
        check(L.eosv_avgpool_forward(_f(h), N4, H4 * W4, D, _f(feat), s), "eosv_avgpool_forward")
        fm = torch.empty(B * D, dtype=torch.float32, device=self.dev)
        check(L.eosv_avgpool_forward(_f(feat), B, T, D, _f(fm), s), "eosv_avgpool_forward")  # mean over the T frames
        C = self.num_classes
        logits = torch.empty(B * C, dtype=torch.float32, device=self.dev)
        check(L.eosv_sgemm(0, 1, B, C, D, 1.0, _f(fm), D, _f(self.fc_w), D, 0.0, _f(logits), C, s), "eosv_sgemm")
        check(L.eosv_add_bias(_f(logits), B, C, _f(self.fc_b), s), "eosv_add_bias")
        row_loss = torch.empty(B, dtype=torch.float32, device=self.dev)
        dlog = torch.empty(B * C, dtype=torch.float32, device=self.dev)
        check(L.eosv_softmax_xent(_f(logits), _f(lab), B, C, _f(row_loss), _f(dlog), s), "eosv_softmax_xent")
        # ---- backward
        check(L.eosv_sgemm(1, 0, C, D, B, 1.0, _f(dlog), C, _f(fm), D, 0.0, _f(self.fc_gw), D, s), "eosv_sgemm")
        check(L.eosv_sum_rows(_f(dlog), B, C, _f(self.fc_gb), 0, s), "eosv_sum_rows")
        dfm = torch.empty(B * D, dtype=torch.float32, device=self.dev)
        check(L.eosv_sgemm(0, 0, B, D, C, 1.0, _f(dlog), C, _f(self.fc_w), D, 0.0, _f(dfm), D, s), "eosv_sgemm")
        dfeat = torch.empty(N4 * D, dtype=torch.float32, device=self.dev)
        check(L.eosv_broadcast_rows(_f(dfm), B, T, D, 1.0 / T, _f(dfeat), s), "eosv_broadcast_rows")
        dh = torch.empty(N4 * H4 * W4 * D, dtype=torch.float32, device=self.dev)
        check(L.eosv_broadcast_rows(_f(dfeat), N4, H4 * W4, D, 1.0 / (H4 * W4), _f(dh), s), "eosv_broadcast_rows")
        for blk in reversed(self.blocks):
            sv = blk.saved
            nl = len(blk.convs)
            dres = None
            g = dh
            for i in reversed(range(nl)):
                c, b = blk.convs[i], blk.bns[i]
                st, P = sv["st"][i]
                dz, dr = self._bn_bwd(g, sv["y"][i], True, sv["z"][i], P, b, st, s, want_dres=(i == nl - 1))
                if i == nl - 1:
                    dres = dr
                skip = None
                if i == 0:
                    # the block input's gradient through the shortcut, added to the first conv's dx
                    if blk.ds is not None:
                        zd, sc, std, Pd = sv["ds"]
                        dzd, _ = self._bn_bwd(dres, None, False, zd, Pd, blk.ds_bn, std, s)
                        skip = self._conv_bwd(dzd, sv["x"], sv["shape"], blk.ds, s, need_dx=True)
                    else:
                        skip = dres
                g = self._conv_bwd(dz, sv["in"][i], sv["inshape"][i], c, s, need_dx=True, acc=skip)
            dh = g
            blk.saved = {}
        da0 = torch.empty(P1 * 64, dtype=torch.float32, device=self.dev)
        check(L.eosv_maxpool_backward(_f(dh), _f(idx), shp1[0], shp1[1], shp1[2], 64, _f(da0), s),
              "eosv_maxpool_backward")
        dz0, _ = self._bn_bwd(da0, a0, True, z0, P1, self.stem_bn, st0, s)
        self._conv_bwd(dz0, frames, shp0, self.stem, s, need_dx=False)
        self._x0 = None  # the NHWC frames are released with the step
        # ---- SGD (optimizer_1: convnet, optimizer_2: fc; first step initialises the momentum)
        first = int(self.step_count == 0)
        check(L.eosv_sgd_momentum(_f(self.p_flat), _f(self.g_flat), _f(self.m_flat), self.p_flat.numel(), lr_conv,
                                  momentum, first, s), "sgd")
        check(L.eosv_sgd_momentum(_f(self.fc_w), _f(self.fc_gw), _f(self.fc_bw), self.fc_w.numel(), lr_fc, momentum,
                                  first, s), "sgd")
        check(L.eosv_sgd_momentum(_f(self.fc_b), _f(self.fc_gb), _f(self.fc_bb), self.fc_b.numel(), lr_fc, momentum,
                                  first, s), "sgd")
        self.step_count += 1
        return float(row_loss.sum().item()), logits.view(B, C)

    def grads(self) -> Dict[str, torch.Tensor]:
        """The last step's gradients in the state_dict layout (CPU), for parity checks."""
        out = {}
        for c in self._convs():
            out[c.name + ".weight"] = c.g.view(c.cout, c.k, c.k, c.cin).permute(0, 3, 1, 2).contiguous().cpu()
        for b in self._bns():
            out[b.name + ".weight"] = b.dgamma.cpu()
            out[b.name + ".bias"] = b.dbeta.cpu()
        out["fc.weight"] = self.fc_gw.cpu()
        out["fc.bias"] = self.fc_gb.cpu()
        return out
