"""arch.unfold_ds_bytes (applied by arch.fuse_bneck_bytes): the algorithmic bytes of a block whose
downsample ran as a launch of its own, recognised from the profile's launch counts; and the
Winograd launcher's check of the kernel's 32-bit patch offsets (host side, no device call)."""
import numpy as np

from eosv import arch

SPEC = arch.SPECS["resnet18"]


def _launch_counts(ds_launched):
    """Launch counts of an f32 R18 profile: every conv once per chunk, downsamples as asked."""
    n = 2 + 2 * sum(SPEC.layers) + 3
    nl = np.full(n, 4, np.int64)
    nl[-1] = 0  # the fc is not a conv launch
    for _, _, _, ds in arch.block_layer_ids(SPEC):
        if ds is not None:
            nl[ds] = 4 if ds_launched else 0
    return nl


def test_unfused_downsample_bytes_stage2_block():
    base = arch.conv_launch_bytes(SPEC, 224, 224, 4)
    L = arch.fuse_bneck_bytes(base, SPEC, _launch_counts(True))
    c1, c2, _, ds = arch.block_layer_ids(SPEC)[2]  # first block of stage 2: 56 x 56 x 64 -> 28 x 28 x 128
    assert (c1, c2, ds) == (5, 6, 7)
    px = 28 * 28
    # downsample: the block input at stride 2 (64 channels) + its output map (128) + 128 x 64 weights
    assert L[ds] == ((px * 64 + px * 128) * 4, 128 * 64 * 4, px * 64 * 4)
    # conv2: its input map + the residual map + the output map, 128 channels each; 3x3 weights only
    assert L[c2] == (3 * px * 128 * 4, 128 * 128 * 9 * 4, px * 128 * 4)
    # together: the folded launch's bytes plus the residual map written and read once
    pf, wb, _ = base[c2]
    assert L[ds][0] + L[c2][0] == pf + 2 * px * 128 * 4 == (px * 64 + 4 * px * 128) * 4
    assert L[ds][1] + L[c2][1] == wb
    # nothing else moves
    for i, e in enumerate(base):
        if i not in (6, 7, 11, 12, 16, 17):
            assert tuple(L[i]) == tuple(e)


def test_unfused_downsample_bytes_every_stage_and_bottleneck():
    for name in ("resnet18", "resnet50"):
        spec = arch.SPECS[name]
        base = arch.conv_launch_bytes(spec, 224, 224, 4)
        nl = np.ones(len(base) + 1, np.int64)
        L = arch.unfold_ds_bytes(base, spec, nl)
        for c1, c2, c3, ds in arch.block_layer_ids(spec):
            if ds is None:
                continue
            last = c2 if c3 is None else c3
            out = (L[last][0] - L[last][2]) // 2   # residual map = output map
            assert L[last][0] == L[last][2] + 2 * out
            assert L[ds][0] == L[ds][2] + out
            assert L[ds][0] + L[last][0] == base[last][0] + 2 * out
            assert L[ds][1] + L[last][1] == base[last][1] and L[ds][1] > 0


def test_wino_launcher_rejects_shapes_beyond_32_bit_offsets():
    """eosv_conv_wino_f32 addresses its patches with 32-bit byte offsets over the (at most) 65 frames
    a workgroup spans; a shape whose 65 frames exceed 2^32 bytes is refused before any device call."""
    from eosv import _lib

    L = _lib.lib()
    p = 4096  # never dereferenced: the launcher returns first
    # 65 * 512 * 512 * 64 * 4 B = 4.36e9 > 2^32
    assert L.eosv_conv_wino_f32(p, p, None, None, 0, p, 1, 512, 512, 64, None) == -4  # EOSV_ERR_UNSUPPORTED
    assert b"32-bit" in L.eosv_last_error()
    assert L.eosv_conv_wino_f32(p, p, None, None, 0, p, 1, 8, 8, 96, None) == -4  # C % 64, as before


def test_folded_downsample_list_is_unchanged():
    base = arch.conv_launch_bytes(SPEC, 224, 224, 4)
    L = arch.fuse_bneck_bytes(base, SPEC, _launch_counts(False))
    assert [tuple(e) for e in L] == [tuple(e) for e in base]
