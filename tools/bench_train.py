#!/usr/bin/env python3
"""Training-step throughput: the reference's finetune recipe
(network_train.py:140: ResNet-50, batch 6 clips x 16 frames at 224x224, SGD momentum) on
synthetic frames, through eosv.train.NativeTrainer.  Prints one JSON line: clips/s, frames/s,
ms/step and the conv FLOP rate (forward + input gradient + weight gradient = 3 x the forward
conv FLOPs, the stem's input gradient excluded) against the f32 MFMA peak; with --cpu-steps, the
same step on torch-CPU (the oracle model, f32) for a CPU baseline.  --winograd [MASK] runs the
3x3 stride-1 convs' forward and input gradient on the Winograd kernel (NativeTrainer's opt-in);
--winograd-wgrad [MASK] runs their weight gradient in the Winograd domain (independent of
--winograd); the FLOP rate keeps counting direct-conv FLOPs.  --stem-direct runs the stem's
forward and weight gradient on the direct 7x7 kernels (no NHWC copy, no im2col buffer).
--f32x3 [MASK] runs the stride-1 1x1 convs' three GEMMs in f32x3 arithmetic (bit li: layer{li+1}).
--f32x3-convs [MASK] runs the 3x3 convs and the stride-2 1x1 shortcuts on the f32x3 implicit GEMMs
(forward, weight gradient, stride-1 input gradient; the same bits).
--fused-bn-stats [MASK] lets the f32x3 forwards of those stages write the following BN's batch sums
from their epilogue (the same bits; it acts only on convs that --f32x3 / --f32x3-convs enable).
--f32x3-dgrad [MASK] runs the input gradient of the stride-2 convs (layer{2,3,4}.0's 3x3 conv and 1x1
shortcut) on the f32x3 implicit GEMM by parity class (the same bits; bit 0 selects nothing).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "embodied-one-shot-video-recognition_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eosv import arch, synth  # noqa: E402
from eosv.train import NativeTrainer  # noqa: E402

GFLOP_FWD = {"resnet18": 3.6271, "resnet50": 8.1743}  # per 224x224 frame


def measure(arch_name="resnet50", batch=6, frames_per_clip=16, res=224, steps=5, warmup=1, device=0,
            winograd=False, winograd_wgrad=False, stem_direct=False, f32x3=False, f32x3_convs=False, fused_bn_stats=False,
            f32x3_dgrad=False):
    """One NativeTrainer on synthetic frames: warmup steps, then `steps` timed steps (synchronised
    on both sides).  Returns the JSON dict, plus the state dict, frames and labels for the CPU leg.
    winograd, winograd_wgrad: NativeTrainer's keywords (False, True = TRAIN_WINO_DEFAULT /
    TRAIN_WINO_WGRAD_DEFAULT, or a stage mask), stem_direct (a bool) and f32x3 (False, True =
    TRAIN_X3_DEFAULT, or a stage mask) and f32x3_convs (the same form, True = TRAIN_X3C_DEFAULT) and fused_bn_stats (the same form,
    True = TRAIN_BNSTATS_DEFAULT) and f32x3_dgrad (the same form, True = TRAIN_X3D_DEFAULT)."""
    sd = synth.synth_state_dict(arch.SPECS[arch_name], 64, 0)
    tr = NativeTrainer(arch_name, 64, device=device, winograd=winograd, winograd_wgrad=winograd_wgrad,
                       stem_direct=stem_direct, f32x3=f32x3, f32x3_convs=f32x3_convs,
                       fused_bn_stats=fused_bn_stats, f32x3_dgrad=f32x3_dgrad)
    tr.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    frames = torch.randn(batch * frames_per_clip, 3, res, res, generator=g).cuda(device)
    labels = np.arange(batch) % 64
    for _ in range(warmup):
        tr.step(frames, labels, frames_per_clip, 1e-4, 1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = tr.step(frames, labels, frames_per_clip, 1e-4, 1e-3)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    nf = batch * frames_per_clip
    flops = 3 * GFLOP_FWD[arch_name] * 1e9 * (res / 224.0) ** 2 * nf
    out = {"metric": "training clips/s (network_train.py finetune step)", "arch": arch_name, "batch": batch,
           "frames_per_clip": frames_per_clip, "res": res, "dtype": "f32", "clips_per_s": round(batch / dt, 2),
           "frames_per_s": round(nf / dt, 1), "ms_per_step": round(dt * 1e3, 2), "steps": steps, "warmup": warmup,
           "loss": round(loss, 4), "conv_tflops": round(flops / dt / 1e12, 2),
           "conv_frac_f32_peak": round(flops / dt / 157.3e12, 4),
           "winograd": tr.wino_mask, "wino_launches_per_step": tr.wino_launches,
           "winograd_wgrad": tr.wino_wgrad_mask, "wino_wgrad_launches_per_step": tr.wino_wgrad_launches,
           "stem_direct": tr.stem_direct, "stem_direct_launches_per_step": tr.stem_direct_launches,
           "f32x3": tr.x3_mask, "x3_launches_per_step": tr.x3_launches,
           "f32x3_convs": tr.x3c_mask, "x3c_launches_per_step": tr.x3c_launches,
           "fused_bn_stats": tr.bnstats_mask, "bn_fused_per_step": tr.bn_fused_launches,
           "f32x3_dgrad": tr.x3d_mask, "x3d_launches_per_step": tr.x3d_launches,
           "data": "synthetic frames, random-init weights of the reference architecture; conv_tflops counts "
                   "direct-conv FLOPs whatever the winograd mask (as roofline.frac, DESIGN 5)"}
    return out, sd, frames, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-steps", type=int, default=0)
    ap.add_argument("--winograd", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="Winograd kernel for the stride-1 3x3 convs' forward and input gradient: stage mask "
                         "(1: 64, 2: 128, 4: 256, 8: 512 channels); without a value, eosv.train.TRAIN_WINO_DEFAULT")
    ap.add_argument("--winograd-wgrad", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="Winograd-domain weight gradient of the same convs: stage mask as --winograd; without a "
                         "value, eosv.train.TRAIN_WINO_WGRAD_DEFAULT")
    ap.add_argument("--stem-direct", action="store_true",
                    help="the stem's forward and weight gradient on the direct 7x7 kernels (eosv_stem_conv_f32, "
                         "eosv_stem_wgrad_f32) instead of NHWC copy + im2col + GEMMs")
    ap.add_argument("--f32x3", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="f32x3 GEMMs for the stride-1 1x1 convs (forward, input and weight gradient): stage mask "
                         "(bit li: layer{li+1}); without a value, eosv.train.TRAIN_X3_DEFAULT")
    ap.add_argument("--f32x3-convs", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="f32x3 implicit GEMMs for the 3x3 convs and the stride-2 1x1 shortcuts (forward, weight "
                         "gradient, stride-1 input gradient): stage mask (bit li: layer{li+1}); without a value, "
                         "eosv.train.TRAIN_X3C_DEFAULT")
    ap.add_argument("--fused-bn-stats", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="the BN batch sums from the f32x3 forwards' epilogues (needs --f32x3 / --f32x3-convs): stage "
                         "mask (bit li: layer{li+1}); without a value, eosv.train.TRAIN_BNSTATS_DEFAULT")
    ap.add_argument("--f32x3-dgrad", nargs="?", type=int, const=-1, default=0, metavar="MASK",
                    help="f32x3 implicit GEMM by parity class for the stride-2 convs' input gradient: stage mask "
                         "(bit li: layer{li+1}; bit 0 selects nothing); without a value, eosv.train.TRAIN_X3D_DEFAULT")
    a = ap.parse_args()
    out, sd, frames, labels = measure(a.arch, a.batch, a.frames, a.res, a.steps, a.warmup,
                                      winograd=True if a.winograd < 0 else a.winograd,
                                      winograd_wgrad=True if a.winograd_wgrad < 0 else a.winograd_wgrad,
                                      stem_direct=a.stem_direct, f32x3=True if a.f32x3 < 0 else a.f32x3,
                                      f32x3_convs=True if a.f32x3_convs < 0 else a.f32x3_convs,
                                      fused_bn_stats=True if a.fused_bn_stats < 0 else a.fused_bn_stats,
                                      f32x3_dgrad=True if a.f32x3_dgrad < 0 else a.f32x3_dgrad)
    if a.cpu_steps:
        from oracle.resnet_ref import ModelResNetRef

        torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
        m = ModelResNetRef(a.arch, 64)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        m.train()
        o1 = torch.optim.SGD(m.convnet.parameters(), lr=1e-4, momentum=0.9)
        o2 = torch.optim.SGD(m.fc.parameters(), lr=1e-3, momentum=0.9)
        x = frames.cpu()
        lab = torch.as_tensor(labels, dtype=torch.long)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            o1.zero_grad()
            o2.zero_grad()
            f, _ = m(x)
            torch.nn.CrossEntropyLoss()(m.fc(f.view(a.batch, a.frames, -1).mean(1)), lab).backward()
            o1.step()
            o2.step()
        cdt = (time.perf_counter() - t0) / a.cpu_steps
        out["cpu_baseline"] = {"clips_per_s": round(a.batch / cdt, 3), "cores": torch.get_num_threads(),
                               "kind": "port", "sample": f"{a.cpu_steps} steps of the same batch, torch-CPU f32"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
