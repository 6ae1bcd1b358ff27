"""Shared test helpers: load golden fixtures, synthesize the reference's inputs."""
import json
import os

import numpy as np
import torch

from eosv import arch, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(tag):
    with open(os.path.join(GOLDEN, tag + ".json")) as f:
        meta = json.load(f)
    npz = os.path.join(GOLDEN, tag + ".npz")
    arrays = dict(np.load(npz)) if os.path.exists(npz) else {}
    return meta, arrays


def load_video(video_info, support, T=16, H=224, W=224):
    """Frames the reference loader hands over (utils.py:96-136 query / 215-258 support)."""
    ids, n_all = synth.clip_frame_ids(video_info, T)
    cls = video_info.split("/")[0]
    v = torch.from_numpy(synth.synth_video(cls, video_info, ids, H, W))
    if support:
        n = min(T, n_all)
        if v.shape[0] < T:
            v = torch.cat([v, torch.zeros(T - v.shape[0], 3, H, W)])
        return v, n
    return v, v.shape[0]


# ---------------------------------------------------------------- shared by the training step's GPU tests
def _oracle(name, sd, frames, labels, T, lr1, lr2, steps, dtype):
    from oracle.resnet_ref import ModelResNetRef

    m = ModelResNetRef(name, 64)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(dtype).train()
    o1 = torch.optim.SGD(m.convnet.parameters(), lr=lr1, momentum=0.9)
    o2 = torch.optim.SGD(m.fc.parameters(), lr=lr2, momentum=0.9)
    crit = torch.nn.CrossEntropyLoss()
    B = frames.shape[0] // T
    losses, grads0 = [], None
    for it in range(steps):
        o1.zero_grad()
        o2.zero_grad()
        feature, _ = m(frames.to(dtype))
        feature = feature.view(B, T, -1).mean(dim=1)
        out = m.fc(feature)
        loss = crit(out, torch.as_tensor(labels, dtype=torch.long))
        loss.backward()
        if it == 0:
            grads0 = {k: p.grad.detach().double().clone() for k, p in m.named_parameters()}
        o1.step()
        o2.step()
        losses.append(float(loss.detach()))
    return losses, grads0, m.state_dict()


def _small_case():
    torch.manual_seed(0)
    T, B, H = 4, 2, 96
    return torch.randn(B * T, 3, H, H), [3, 17], T


def _expected_wino_launches(name, mask=15):
    """From the architecture alone: every stride-1 3x3 conv with cin = cout of an enabled stage runs
    once forward and once for its input gradient (every block conv's dx is needed; the stem's, the
    only one that is not, is 7x7)."""
    spec = arch.SPECS[name]
    n = 0
    inplanes = 64
    for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), spec.layers)):
        if not mask & (1 << li):
            inplanes = planes * spec.expansion
            continue
        for bi in range(blocks):
            stride = 2 if (li > 0 and bi == 0) else 1
            if spec.block == "basic":
                n += int(stride == 1 and inplanes == planes) + 1   # conv1 (3x3, stride), conv2 (3x3, 1)
            else:
                n += int(stride == 1)                               # conv2 is the 3x3 and carries the stride
            inplanes = planes * spec.expansion
    return 2 * n


def _same_bytes(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert a[1].keys() == b[1].keys()
    for k in a[1]:
        assert a[1][k].numpy().tobytes() == b[1][k].numpy().tobytes(), k
