#!/usr/bin/env python3
"""Records tests/golden/launch_profile.json: per case, how many launches and how many algorithmic
FLOPs one forward records under every layer id (eosv_profile_read), for
tests/test_gpu_launch_profile.py to compare exactly.  The lists say which route every block took:
a fused launch is recorded under one of its block's layer ids with every fused conv's FLOPs, and
the convs it covers show 0 launches.

Run once on an MI355X with EOSV_LIBRARY set to the library of the commit whose routes are to be
held (the parent of a change to the host dispatch):

  EOSV_LIBRARY=/path/to/parent/libeosv.so python tools/record_launch_profile.py

Per case: Backbone(arch, dtype, res, res, max_frames), synthetic weights, one warm-up forward of
`frames` random frames, then the same forward with the profile on.  FLOPs are sums of products of
small integers, exact in a double at these sizes, and are written as integers.  The test imports
the cases and `measure` from here.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "embodied-one-shot-video-recognition_amd")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_profile.json")

# (arch, dtype, res, frames, max_frames)
CASES = [
    ("resnet18", "bf16", 224, 8, 8),     # bblock x2, s2rows, tap-shift
    ("resnet18", "bf16", 256, 8, 8),     # bblock at 64-wide maps
    ("resnet18", "f32", 224, 8, 8),      # Winograd, unfused-downsample route
    ("resnet18", "f32x3", 224, 8, 8),    # split stem, rows_x3
    ("resnet18", "f32", 112, 8, 8),      # the generic paths: no 56/64-wide map
    ("resnet50", "bf16", 224, 8, 8),     # bneck, bneck + next, conv2 + pair1x1r into stage 2, pairw
    ("resnet50", "bf16", 224, 5, 5),     # stage-2 M = 5 * 784, not a multiple of 64
    ("resnet50", "f32", 224, 8, 8),
    ("resnet50", "f32x3", 224, 8, 8),
    ("resnet50", "bf16", 112, 8, 8),     # no stage-1 fusion
    ("resnet101", "bf16", 256, 4, 4),    # bneck_tail at W 64
    ("resnet18", "bf16", 224, 20, 8),    # three chunks: every launched layer counts 3
]


def case_name(case):
    arch, dtype, res, frames, max_frames = case
    return f"{arch}-{dtype}-{res}-f{frames}" + (f"-max{max_frames}" if max_frames != frames else "")


def measure(case):
    """One case -> (launches, flops): two integer lists of n_layers entries (plan order: stem, every
    block's conv1, conv2[, conv3][, downsample], fc)."""
    import torch

    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from eosv import arch as archmod, engine, synth

    arch, dtype, res, frames, max_frames = case
    bb = engine.Backbone(arch, dtype, res, res, max_frames=max_frames)
    try:
        bb.load_state_dict(synth.synth_state_dict(archmod.SPECS[arch], 64, 0))
        x = torch.randn(frames, 3, res, res, generator=torch.Generator().manual_seed(7)).cuda()
        bb.forward(x)
        bb.profile(True)
        bb.forward(x)
        _, fl, n = bb.profile_read()
        bb.profile(False)
        torch.cuda.synchronize()
    finally:
        bb.close()
    flops = [int(v) for v in fl]
    assert all(float(i) == float(v) for i, v in zip(flops, fl)), "a FLOP count is not an integer"
    return [int(v) for v in n], flops


def main():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from eosv import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    print(f"library: {_lib.LIB_PATH}")
    data = {}
    for case in CASES:
        launches, flops = measure(case)
        data[case_name(case)] = {"launches": launches, "flops": flops}
        print(f"{case_name(case)}: {len(launches)} layers, {sum(launches)} launches, {sum(flops)} FLOPs")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in data.items()) + "\n}\n")
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
