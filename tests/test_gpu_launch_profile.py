"""Which route every block of the shipping configurations takes, held as the profile itself: the
launches and the algorithmic FLOPs that one forward records under every layer id
(eosv_profile_read) must equal, exactly, what tests/golden/launch_profile.json holds.

The fixture was written once by tools/record_launch_profile.py with EOSV_LIBRARY set to the library
of the commit before the host dispatch was rewritten on one launch bracket and one route function
(64b85ca), so a block that moves to another route, a fused launch recorded under another layer id
or a changed FLOP count fails here even where every output stays bitwise the same.  bench.py's
roofline accounting (arch.fuse_bneck_bytes, layer_bounds) reads exactly these lists.

The cases, the weights, the frames and the measurement are the recorder's."""
import functools
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_launch_profile",
                                               os.path.join(REPO, "tools", "record_launch_profile.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@functools.lru_cache(maxsize=None)
def _golden():
    with open(rec.GOLDEN) as fh:
        return json.load(fh)


def test_fixture_holds_every_case():
    assert sorted(_golden()) == sorted(rec.case_name(c) for c in rec.CASES)


@pytest.mark.parametrize("case", rec.CASES, ids=[rec.case_name(c) for c in rec.CASES])
def test_launches_and_flops_per_layer_are_the_recorded_ones(case):
    name = rec.case_name(case)
    want = _golden()[name]
    frames, max_frames = case[3], case[4]
    chunks = -(-frames // max_frames)
    # the fixture's own sanity: the fc layer is not part of a backbone forward, the stem is one
    # launch per chunk
    assert want["launches"][-1] == 0 and want["flops"][-1] == 0, f"{name}: the fixture counts the fc layer"
    assert want["launches"][0] == chunks, f"{name}: the fixture's stem has {want['launches'][0]} launches"
    launches, flops = rec.measure(case)
    print(f"launch profile {name}: {len(launches)} layers, {sum(launches)} launches, {sum(flops)} FLOPs")
    assert len(launches) == len(want["launches"]), f"{name}: {len(launches)} layers, recorded {len(want['launches'])}"
    moved = [(i, g, w) for i, (g, w) in enumerate(zip(launches, want["launches"])) if g != w]
    assert not moved, f"{name}: launches differ at (layer, got, recorded) {moved}"
    off = [(i, g, w) for i, (g, w) in enumerate(zip(flops, want["flops"])) if g != w]
    assert not off, f"{name}: FLOPs differ at (layer, got, recorded) {off}"
