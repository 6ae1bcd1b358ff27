"""NativeTrainer's conv dispatch without a device: the plan (c.routes, fixed at construction) against
the eligibility rules restated here from (name, k, stride, pad, cin, cout, stage), and the dispatcher
(_run) over fake routes: the first route that does not refuse wins, later ones are not asked, only the
winner's family counts a launch, and every failure raises under the library function's name."""
import pytest

from eosv import _lib
from test_cpu_train_x3 import _stub_device

UNSUPPORTED, ARG = -4, -1
BIT = {64: 1, 128: 2, 256: 4, 512: 8}
NONE = dict(winograd=0, winograd_wgrad=0, f32x3=0, stem_direct=False)
ALL = dict(winograd=15, winograd_wgrad=15, f32x3=15, stem_direct=True)
PART = dict(winograd=5, winograd_wgrad=2, f32x3=9, stem_direct=True)


def _expected(c, winograd, winograd_wgrad, f32x3, stem_direct):
    stem = c.name == "convnet.0"
    stage = None if stem else int(c.name.split(".")[1]) - 4          # convnet.{4 + li}: layer{li + 1}
    wino_shape = c.k == 3 and c.stride == 1 and c.pad == 1 and c.cin == c.cout and c.cin in BIT
    one = c.k == 1 and c.stride == 1
    x3 = not stem and one and bool(f32x3 >> stage & 1)
    fwd, wgrad, dgrad = [], [], []
    if stem and stem_direct:
        fwd.append("stem")
        wgrad.append("stem")
    if x3:
        fwd.append("x3")
        wgrad.append("x3")
        dgrad.append("x3")
    if wino_shape and winograd_wgrad & BIT[c.cin]:
        wgrad.append("wino")
    fwd.append("conv")
    if c.cin % 4 == 0 and not one:
        wgrad.append("conv")
    if c.stride == 1 and c.k % 2 == 1 and c.pad == c.k // 2:
        dgrad.append("conv")
    for job in (fwd, wgrad, dgrad):
        job.append("gemm")
    if wino_shape and winograd & BIT[c.cin]:
        fwd = dgrad = ["wino"]                                      # no fall-through: the only entry
    if stem:
        dgrad = []
    return {"fwd": tuple(fwd), "wgrad": tuple(wgrad), "dgrad": tuple(dgrad)}


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
@pytest.mark.parametrize("switches", [NONE, ALL, PART], ids=["none", "all", "part"])
def test_plan_follows_the_rules(monkeypatch, arch, switches):
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer(arch, 4, **switches)
    convs = list(tr._convs())
    assert len(convs) == {"resnet18": 20, "resnet50": 53}[arch]
    for c in convs:
        assert c.routes == _expected(c, **switches), c.name
        assert all(r[-1:] == ("gemm",) or r in ((), ("wino",)) for r in c.routes.values()), c.name
        assert tr._wino_eligible(c) == ("wino" in c.routes["fwd"]) == ("wino" in c.routes["dgrad"])
        assert tr._wino_wgrad_eligible(c) == ("wino" in c.routes["wgrad"])
    if switches is NONE:   # the default constructor is the same trainer
        assert [c.routes for c in train.NativeTrainer(arch, 4)._convs()] == [c.routes for c in convs]
        assert not any(set(r) - {"conv", "gemm"} for c in convs for r in c.routes.values())


def _conv(tr, name):
    return next(c for c in tr._convs() if c.name == name)


def test_plan_of_three_convs_by_name(monkeypatch):
    train = _stub_device(monkeypatch)
    stem = train.NativeTrainer("resnet18", 4, stem_direct=True).stem
    assert stem.name == "convnet.0"
    assert stem.routes == {"fwd": ("stem", "conv", "gemm"), "wgrad": ("stem", "gemm"), "dgrad": ()}
    assert train.NativeTrainer("resnet18", 4).stem.routes == {"fwd": ("conv", "gemm"), "wgrad": ("gemm",), "dgrad": ()}
    c = _conv(train.NativeTrainer("resnet18", 4, winograd=1), "convnet.4.0.conv2")
    assert c.routes["fwd"] == ("wino",) and c.routes["dgrad"] == ("wino",)
    assert c.routes["wgrad"] == ("conv", "gemm")
    c = _conv(train.NativeTrainer("resnet50", 4, f32x3=15), "convnet.5.0.downsample.0")
    assert (c.k, c.stride) == (1, 2)
    assert not any("x3" in r for r in c.routes.values())
    assert c.routes == {"fwd": ("conv", "gemm"), "wgrad": ("conv", "gemm"), "dgrad": ("gemm",)}
    c = _conv(train.NativeTrainer("resnet50", 4, f32x3=15), "convnet.5.0.conv3")
    assert c.routes == {"fwd": ("x3", "conv", "gemm"), "wgrad": ("x3", "gemm"), "dgrad": ("x3", "conv", "gemm")}


COUNTERS = ("stem_direct_launches", "wino_launches", "wino_wgrad_launches", "x3_launches")


def _fake_trainer(monkeypatch, job, statuses):
    """A trainer whose routes of `job` are fakes answering `statuses` ({name: status}, in plan
    order); returns it, its stem-free first conv with that plan, and the list the fakes log into."""
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer("resnet18", 4)
    c = tr.blocks[0].convs[0]
    c.routes = dict(c.routes, **{job: tuple(statuses)})
    asked = []
    for name, rc in statuses.items():
        def route(conv, x, shape, P, dz, out, acc, s, name=name, rc=rc):
            assert conv is c and shape == (2, 8, 8, 64) and P == 2 * 8 * 8
            asked.append(name)
            return rc, f"eosv_fake_{name}"
        monkeypatch.setattr(tr, f"_{job}_{name}", route)
    return tr, c, asked


def _counts(tr):
    return {k: getattr(tr, k) for k in COUNTERS}


@pytest.mark.parametrize("job,statuses,winner,counter", [
    ("fwd", {"stem": UNSUPPORTED, "x3": UNSUPPORTED, "wino": 0, "conv": 0, "gemm": 0}, "wino", "wino_launches"),
    ("fwd", {"stem": 0, "conv": 0, "gemm": 0}, "stem", "stem_direct_launches"),
    ("wgrad", {"stem": UNSUPPORTED, "x3": 0, "wino": 0, "gemm": 0}, "x3", "x3_launches"),
    ("wgrad", {"x3": UNSUPPORTED, "wino": 0, "conv": 0, "gemm": 0}, "wino", "wino_wgrad_launches"),
    ("wgrad", {"stem": 0, "gemm": 0}, "stem", "stem_direct_launches"),
    ("dgrad", {"x3": UNSUPPORTED, "wino": 0}, "wino", "wino_launches"),
    ("dgrad", {"x3": UNSUPPORTED, "conv": 0, "gemm": 0}, "conv", None),
    ("fwd", {"x3": UNSUPPORTED, "conv": UNSUPPORTED, "gemm": 0}, "gemm", None),
])
def test_first_route_that_does_not_refuse_wins(monkeypatch, job, statuses, winner, counter):
    tr, c, asked = _fake_trainer(monkeypatch, job, statuses)
    tr.x3_launches = 5   # assignable, and counted from where it stands
    before = _counts(tr)
    tr._run(job, c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(winner) + 1]
    want = dict(before)
    if counter:
        want[counter] += 1
    assert _counts(tr) == want


@pytest.mark.parametrize("job,statuses,culprit", [
    ("fwd", {"x3": ARG, "conv": 0, "gemm": 0}, "x3"),                               # a failure is no refusal
    ("wgrad", {"x3": UNSUPPORTED, "wino": -2, "gemm": 0}, "wino"),
    ("dgrad", {"x3": UNSUPPORTED, "conv": UNSUPPORTED, "gemm": UNSUPPORTED}, "gemm"),  # the last one's refusal
    ("fwd", {"wino": UNSUPPORTED}, "wino"),
])
def test_failures_raise_under_the_library_functions_name(monkeypatch, job, statuses, culprit):
    tr, c, asked = _fake_trainer(monkeypatch, job, statuses)
    before = _counts(tr)
    with pytest.raises(_lib.EosvError, match=f"eosv_fake_{culprit} failed"):
        tr._run(job, c, None, (2, 8, 8, 64), None, None, None, 0)
    names = list(statuses)
    assert asked == names[:names.index(culprit) + 1]
    assert _counts(tr) == before


def test_a_job_without_routes_raises(monkeypatch):
    train = _stub_device(monkeypatch)
    tr = train.NativeTrainer("resnet18", 4)
    with pytest.raises(_lib.EosvError, match="convnet.0 has no dgrad route"):
        tr._run("dgrad", tr.stem, None, (2, 8, 8, 3), None, None, None, 0)
