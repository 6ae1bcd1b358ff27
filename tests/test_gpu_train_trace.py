"""GPU: the library calls one NativeTrainer.step() makes, against the recorded trace
(tests/golden/train_call_trace.json, written by tools/train_call_trace.py): the same calls, in the
same order, with the same arguments and statuses.  This pins which kernel each conv takes, the order
in which alternatives are asked and what follows a refusal (r18_w90: both direct stem kernels refuse
the 90-pixel width and the step falls through to the NHWC copy, im2col and the GEMMs); the numeric
tests and the launch counts do not.

A change that moves a call on purpose (a new route, another order) records the file again with the
tool and says so; a change of the Python glue alone must leave it as it is."""
import functools
import json
import os
import sys

import pytest

from _common import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import train_call_trace  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _recorded():
    with open(os.path.join(GOLDEN, "train_call_trace.json")) as fh:
        return json.load(fh)


def test_every_case_is_recorded():
    assert set(_recorded()) == set(train_call_trace.CASES)


@pytest.mark.parametrize("case", list(train_call_trace.CASES))
def test_step_makes_the_recorded_calls(case):
    want = _recorded()[case]
    first, second, _ = train_call_trace.record(case)
    diff = train_call_trace.first_difference(first, want)
    assert diff is None, f"{case}, step 1: {diff}"
    # the second step repeats the first but for the SGD launches' `first` flag (its 7th argument)
    assert len(second) == len(first)
    for i, (a, b) in enumerate(zip(second, first)):
        if b[0] == "eosv_sgd_momentum":
            assert b[1][6] == 1 and a == [b[0], b[1][:6] + [0] + b[1][7:], b[2]], (case, i, a, b)
        else:
            assert a == b, f"{case}, step 2: call {i}: {json.dumps(a)} where step 1 made {json.dumps(b)}"
