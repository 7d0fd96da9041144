"""Launch budget of the flat optimizers: which native calls ONE eager ``step()`` issues, in
order, for every optimizer form -- unsharded, and per rank under a 2-rank
``DataParallel(shard_optimizer=True)`` -- and that a captured step issues the same calls and
allocates nothing.

The expected sequences are literals recorded from the optimizers as they were before the step
became one pipeline (``_FlatStep``); they are not derived from the code under test.  A record
is the native function's name plus the keywords that were present (not None / not empty):
``clip`` ``lars`` ``ext`` ``sums_out`` ``zero`` (= ``zero_ranges``).  Pure host-side size
queries (``grad_sumsq_parts``, ``seg_sumsq_chunk``) launch nothing and are not recorded.

The model is a bias-carrying MLP 70-33-10: odd sizes (padded segments, alignment gaps), and
1-D biases that LARS leaves alone.  A world of one has nothing to shard (DataParallel keeps the
replicated update there), so the sharded sequences come from a 2-rank FakeWorld with two
sharded buckets and the replicated tail; the world-1 wrapper is checked to equal the plain
unsharded step with no all-reduce."""
import threading

import pytest
import torch

import ldnn
from ldnn.models import CrossEntropyLoss
from ldnn.models.mlp import MLP
from ldnn.ops import _ext
from ldnn.optim import SGD, Adam, AdamW
from ldnn.optim.optimizers import _Lars
from ldnn.parallel.comm import FakeWorld, LocalComm, _Done
from ldnn.parallel.ddp import DataParallel
from ldnn.train.graphed import GraphedDPStep

pytestmark = pytest.mark.gpu

_HOST_QUERIES = ("grad_sumsq_parts", "seg_sumsq_chunk")
_OPTIMIZER_CALLS = ("sgd_step", "adam_step", "bump_step", "grad_sumsq", "sumsq_total", "clip_finalize", "seg_sumsq",
                    "lars_finalize")
_KW = (("clip", "clip"), ("lars", "lars"), ("ext", "ext"), ("sums_out", "sums_out"), ("zero_ranges", "zero"))

CONFIGS = {
    "sgd_momentum": (lambda p: SGD(p, lr=0.05, momentum=0.9), {}),
    "sgd_clip": (lambda p: SGD(p, lr=0.05, momentum=0.9, max_grad_norm=1.0), {}),
    "sgd_lars": (lambda p: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4, lars_trust=0.02), {}),
    "sgd_clip_lars": (lambda p: SGD(p, lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0,
                                    lars_trust=0.02), {}),
    "adam": (lambda p: Adam(p, lr=1e-3), {}),
    "adam_clip": (lambda p: Adam(p, lr=1e-3, max_grad_norm=1.0), {}),
    "adamw_clear": (lambda p: AdamW(p, lr=1e-3), {"clear_grads": True}),
}

# ---- recorded before the refactor -------------------------------------------------------------
UNSHARDED = {
    "sgd_momentum": ["sgd_step"],
    "sgd_clip": ["grad_sumsq", "clip_finalize", "sgd_step[clip]"],
    "sgd_lars": ["seg_sumsq", "lars_finalize", "sgd_step[lars]"],
    "sgd_clip_lars": ["grad_sumsq", "clip_finalize", "seg_sumsq", "lars_finalize[clip]", "sgd_step[clip,lars]"],
    "adam": ["bump_step", "adam_step"],
    "adam_clip": ["grad_sumsq", "clip_finalize", "bump_step[clip]", "adam_step[clip]"],
    "adamw_clear": ["bump_step", "adam_step[zero]"],
}
# 2-rank world, two sharded buckets + the replicated tail: (rank 0, rank 1, all-reduces per rank).  Rank 0
# sums three ranges (its two shards and the tail), rank 1 its two shards; every rank updates three.
SHARDED = {
    "sgd_momentum": (["sgd_step"] * 3,
                     ["sgd_step"] * 3, 0),
    "sgd_clip": (["grad_sumsq"] * 3 + ["sumsq_total", "clip_finalize[ext]"] + ["sgd_step[clip]"] * 3,
                 ["grad_sumsq"] * 2 + ["sumsq_total", "clip_finalize[ext]"] + ["sgd_step[clip]"] * 3, 1),
    "sgd_lars": (["seg_sumsq", "lars_finalize[sums_out]", "lars_finalize[ext]"] + ["sgd_step[lars]"] * 3,
                 ["seg_sumsq", "lars_finalize[sums_out]", "lars_finalize[ext]"] + ["sgd_step[lars]"] * 3, 1),
    "sgd_clip_lars": (["grad_sumsq"] * 3 + ["sumsq_total", "seg_sumsq", "lars_finalize[sums_out]",
                                            "clip_finalize[ext]", "lars_finalize[clip,ext]"]
                      + ["sgd_step[clip,lars]"] * 3,
                      ["grad_sumsq"] * 2 + ["sumsq_total", "seg_sumsq", "lars_finalize[sums_out]",
                                            "clip_finalize[ext]", "lars_finalize[clip,ext]"]
                      + ["sgd_step[clip,lars]"] * 3, 1),
    "adam": (["bump_step"] + ["adam_step"] * 3,
             ["bump_step"] + ["adam_step"] * 3, 0),
    "adam_clip": (["grad_sumsq"] * 3 + ["sumsq_total", "clip_finalize[ext]", "bump_step[clip]"]
                  + ["adam_step[clip]"] * 3,
                  ["grad_sumsq"] * 2 + ["sumsq_total", "clip_finalize[ext]", "bump_step[clip]"]
                  + ["adam_step[clip]"] * 3, 1),
    "adamw_clear": (["bump_step"] + ["adam_step"] * 3,
                    ["bump_step"] + ["adam_step"] * 3, 0),
}
# -----------------------------------------------------------------------------------------------


class _Recorder:
    """Stands in for the native module: forwards every call, logs launches per thread."""

    def __init__(self, real):
        self._real, self.logs = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or name in _HOST_QUERIES:
            return fn

        def call(*a, **kw):
            tags = [tag for key, tag in _KW if kw.get(key) is not None and not (key == "zero_ranges" and not kw[key])]
            self.logs.setdefault(threading.get_ident(), []).append(name + ("[" + ",".join(tags) + "]" if tags else ""))
            return fn(*a, **kw)
        return call

    def take(self):
        return self.logs.pop(threading.get_ident(), [])


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder(_ext.C())
    monkeypatch.setattr(_ext, "C", lambda: r)
    return r


def _model():
    torch.manual_seed(0)
    m = MLP(70, (33,), 10)
    ldnn.prepare(m, "cuda")
    return m


def _fill_grad(flat, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat.grad.copy_(torch.randn(flat.numel, device="cuda", generator=g))


def _flat(opt):
    return opt._flat_for_group(opt.param_groups[0])


def _record_step(rec, opt, kw, comm=None):
    """One warm-up step, then the calls (and all-reduces on ``comm``) of the next one."""
    f = _flat(opt)
    _fill_grad(f, 1)
    opt.step(**kw)
    _fill_grad(f, 2)
    n = [0]
    if comm is not None:
        real = comm.all_reduce
        comm.all_reduce = lambda *a, **k: (n.__setitem__(0, n[0] + 1), real(*a, **k))[1]
    rec.take()
    opt.step(**kw)
    return rec.take(), n[0]


def _sharded_rank(comm, rec, name):
    mk, kw = CONFIGS[name]
    m = _model()
    dp = DataParallel(m, comm, bucket_cap_mb=0.005, shard_optimizer=True)
    assert dp.sharded and [b["sharded"] for b in dp.bucketer.buckets] == [True, True, False]
    out = _record_step(rec, mk(m.parameters()), kw, comm)
    dp.wait_gathers()
    torch.cuda.synchronize()
    return out


def record_unsharded(rec, name):
    mk, kw = CONFIGS[name]
    return _record_step(rec, mk(_model().parameters()), kw)[0]


def record_sharded(rec, name):
    return FakeWorld(2).run(_sharded_rank, rec, name)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_unsharded_step_launches(rec, name):
    assert record_unsharded(rec, name) == UNSHARDED[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_world1_wrapper_keeps_the_unsharded_step(rec, name):
    mk, kw = CONFIGS[name]
    m = _model()
    comm = FakeWorld(1).comm(0)
    dp = DataParallel(m, comm, shard_optimizer=True)
    assert not dp.sharded
    calls, reduces = _record_step(rec, mk(m.parameters()), kw, comm)
    assert calls == UNSHARDED[name] and reduces == 0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_sharded_step_launches_and_one_extra_collective(rec, name):
    res = record_sharded(rec, name)
    for r in range(2):
        assert res[r] == (SHARDED[name][r], SHARDED[name][2]), r


def _state_ids(opt):
    ids = {}
    for k, v in opt._ls().items():
        if torch.is_tensor(v):
            ids[k] = id(v)
        elif isinstance(v, _Lars):
            ids[k] = id(v)
            ids.update({f"{k}.{a}": id(t) for a, t in vars(v).items() if torch.is_tensor(t)})
            for key, tab in v.tables.items():
                ids.update({f"{k}.tables{key}.{a}": id(t) for a, t in tab.items() if torch.is_tensor(t)})
    return ids


@pytest.mark.parametrize("name", list(CONFIGS))
def test_captured_step_issues_the_eager_calls_and_allocates_nothing(rec, name):
    mk, kw = CONFIGS[name]
    opt = mk(_model().parameters())
    f = _flat(opt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager, _ = _record_step(rec, opt, kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    before = _state_ids(opt)
    _fill_grad(f, 3)
    graph = torch.cuda.CUDAGraph()
    opt._ldnn_capturing = True
    try:
        with torch.cuda.graph(graph, stream=s):
            opt.step(**kw)
    finally:
        opt._ldnn_capturing = False
    assert rec.take() == eager == UNSHARDED[name]
    assert _state_ids(opt) == before
    master = f.master.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(master, f.master)     # the graph holds the update


def test_capture_without_an_eager_step_is_refused(rec):
    opt = CONFIGS["sgd_clip_lars"][0](_model().parameters())
    _fill_grad(_flat(opt), 1)
    opt._ldnn_capturing = True
    with pytest.raises(RuntimeError, match="run an eager optimizer step before capturing"):
        opt.step()
    assert not any(torch.is_tensor(v) for v in opt._ls().values())


class _TwoRankEcho(LocalComm):
    """One process standing in for rank 0 of two (as tests/test_graphed_dp_gpu.py does)."""
    world_size = 2

    def reduce_scatter(self, out, inp, async_op=False):
        self.record("reduce_scatter", inp)
        out.copy_(inp[: out.numel()])
        return _Done() if async_op else None

    def all_gather_into(self, out, inp, async_op=False):
        self.record("all_gather_into", out)
        return _Done() if async_op else None


@pytest.mark.parametrize("name", list(CONFIGS))
def test_graphed_dp_capture_drives_the_sharded_step(rec, name):
    """GraphedDPStep's capture runs the sharded step through ``GradBucketer.step_driver``: the
    optimizer calls it captures are rank 0's eager ones, in per-bucket graphs (plain) or a norm
    and an update graph (clipping / LARS), and it allocates nothing."""
    m = _model()
    dp = DataParallel(m, _TwoRankEcho(), bucket_cap_mb=0.005, broadcast_init=False, shard_optimizer=True)
    assert dp.sharded and len(dp.bucketer.buckets) == 3
    opt = CONFIGS[name][0](m.parameters())
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(16, 70, device="cuda", generator=g).bfloat16()
    y = torch.randint(0, 10, (16,), device="cuda", generator=g)
    crit = CrossEntropyLoss()
    opt.zero_grad()
    crit(dp(x), y).backward()
    dp.finish_gradient_sync()
    opt.step()
    dp.wait_gathers()
    torch.cuda.synchronize()
    before = _state_ids(opt)
    rec.take()
    gd = GraphedDPStep(dp, crit, opt, x, y)
    calls = [c for c in rec.take() if c.split("[")[0] in _OPTIMIZER_CALLS]
    assert calls == SHARDED[name][0]
    assert _state_ids(opt) == before
    assert [i for _, i in gd.g_opts] == ([None, "clip"] if SHARDED[name][2] else [0, 1, 2])
    gd(x, y)
    dp.wait_gathers()
    torch.cuda.synchronize()
