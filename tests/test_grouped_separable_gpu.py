"""The separable EnhancedCNN with a grouped 3x3 (build_model(..., separable=True, group_width=16)) on the MI355X,
with the comparisons and constants of tests/test_separable_gpu.py."""
import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss, build_model, xavier_init

pytestmark = pytest.mark.gpu


def _model():
    return build_model("enhanced_cnn_small", separable=True, group_width=16)


def test_grouped_separable_cnn_matches_cpu_fp32():
    torch.manual_seed(0)
    m = _model()
    xavier_init(m)
    ref = _model()
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():  # same bf16-rounded weights as the kernels read
        for q in ref.parameters():
            q.copy_(q.bfloat16().float())
    ldnn.prepare(m, "cuda")
    ldnn.prepare(ref, "cpu")
    x, y = torch.randn(8, 3, 32, 32), torch.randint(0, 10, (8,))
    lo = CrossEntropyLoss()(m(x.cuda().bfloat16()), y.cuda())
    lo.backward()
    lr_ = CrossEntropyLoss()(ref(x.bfloat16().float()), y)
    lr_.backward()
    assert abs(lo.item() - lr_.item()) < 0.05 * max(1.0, lr_.item())
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        cos = torch.nn.functional.cosine_similarity(p.grad.float().cpu().flatten(), q.grad.flatten(), dim=0).item()
        print(n, cos)
        assert cos > 0.98, (n, cos)


def test_grouped_separable_graphed_step_matches_eager():
    """Two replays of a captured step against the same two eager steps of two more replicas."""
    from ldnn.optim import SGD
    from ldnn.train.graphed import GraphedStep

    torch.manual_seed(0)
    ms = [_model() for _ in range(3)]
    xavier_init(ms[0])
    for m in ms:
        m.load_state_dict(ms[0].state_dict())
        ldnn.prepare(m, "cuda")
    os_ = [SGD(m.parameters(), lr=0.05, momentum=0.9) for m in ms]
    crit = CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(32, 3, 32, 32, device="cuda", generator=g).bfloat16() for _ in range(3)]
    ys = [torch.randint(0, 10, (32,), device="cuda", generator=g) for _ in range(3)]
    for m, o in zip(ms, os_):
        o.zero_grad()
        crit(m(xs[0]), ys[0]).backward()
        o.step()
    p0 = [q.detach().clone() for q in ms[1].parameters()]
    gs = GraphedStep(ms[0], crit, os_[0], xs[1], ys[1], warmup=0)
    for i in (1, 2):
        gs(xs[i], ys[i])
        for m, o in zip(ms[1:], os_[1:]):
            o.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            o.step()
    torch.cuda.synchronize()
    for (n, p), q, s, r in zip(ms[0].named_parameters(), ms[1].parameters(), ms[2].parameters(), p0):
        d1, d2, d3 = ((t.detach() - r).flatten().double() for t in (p, q, s))
        eg, ee = (d1 - d2).norm().item(), (d3 - d2).norm().item()
        assert eg <= 3.0 * ee + 2e-3 * d2.norm().item(), (n, eg, ee, d2.norm().item())
        cos = torch.nn.functional.cosine_similarity(d1, d2, dim=0).item()
        cos_ee = torch.nn.functional.cosine_similarity(d3, d2, dim=0).item()
        assert cos > (0.9 if cos_ee >= 0.9 else cos_ee - 0.3), (n, cos, cos_ee)
