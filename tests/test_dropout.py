"""Dropout with counter-hashed masks, on the CPU: the NumPy twin against the definition written out
element by element, its statistics, the functional / module / model / CLI layers on top of it.

The definition (csrc/kernels/dropout.hip, ops.functional.dropout_mask): a tensor is [R, N], four
neighbouring columns of a row share one hash, G = ceil(N / 4),
    key  = smix(smix(seed) ^ (module << 32 | counter))
    h    = smix(key ^ ((r * G + (c >> 2)) * 0xD1B54A32D192ED03))
    drop = ((h >> (16 * (c & 3))) & 0xFFFF) < thr,  thr = round(p * 65536)
    y    = drop ? 0 : x * (65536.0f / (65536 - thr))

Statistics: a mask of n = 2^20 elements keeps each with probability q = 1 - thr / 65536, so the kept
fraction has standard deviation sqrt(q (1 - q) / n); two independent masks agree on an element with
probability a = q^2 + (1 - q)^2, standard deviation sqrt(a (1 - a) / n).  The bound is 5 of them.
"""
import math

import numpy as np
import pytest
import torch

import ldnn
from ldnn import cli
from ldnn.data.autoaugment import smix, smix_np
from ldnn.models import REGISTRY, build_model
from ldnn.models.layers import Dropout, reseed_dropout
from ldnn.ops import functional as LF

M64 = (1 << 64) - 1


def loop_mask(seed, module, counter, thr, R, N):
    """The definition, literally."""
    key = smix(smix(seed & M64) ^ ((module << 32) | counter))
    G = (N + 3) // 4
    out = np.zeros((R, N), dtype=bool)
    for r in range(R):
        for c in range(N):
            h = smix(key ^ (((r * G + (c >> 2)) * 0xD1B54A32D192ED03) & M64))
            out[r, c] = ((h >> (16 * (c & 3))) & 0xFFFF) < thr
    return out


def test_smix_np_is_smix():
    z = np.array([0, 1, 0x9E3779B97F4A7C15, 1 << 63, M64, 123456789012345678], dtype=np.uint64)
    assert smix_np(z).tolist() == [smix(int(v)) for v in z]


@pytest.mark.parametrize("thr", [1, 32768, 65535, 65536])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (2, 9)], ids=str)
def test_twin_matches_the_definition(shape, thr):
    for seed, module, counter in ((0, 0, 0), (0xDEADBEEFCAFEF00D, 3, 7), (M64, 0xFFFFFFFF, 0xFFFFFFFF)):
        got = LF.dropout_mask(seed, module, counter, thr, *shape)
        assert got.dtype == bool and got.shape == shape
        assert np.array_equal(got, loop_mask(seed, module, counter, thr, *shape)), (seed, module, counter)
    if thr == 65536:
        assert LF.dropout_mask(1, 2, 3, thr, *shape).all()


def test_thr_and_scale():
    assert [LF.dropout_thr(p) for p in (0.0, 0.25, 0.5, 1.0)] == [0, 16384, 32768, 65536]
    assert LF.dropout_thr(0.1) == 6554 and LF.dropout_thr(1e-6) == 0
    assert LF.dropout_scale(32768) == np.float32(2.0) and LF.dropout_scale(65536) == np.float32(0.0)
    assert LF.dropout_scale(6554) == np.float32(65536.0) / np.float32(58982.0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            LF.dropout_thr(bad)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_fraction_and_decorrelation(p):
    R = N = 1024
    n = R * N
    thr = LF.dropout_thr(p)
    q = 1.0 - thr / 65536.0
    sd = math.sqrt(q * (1 - q) / n)
    base = LF.dropout_mask(2024, 0, 0, thr, R, N)
    others = {"counter": LF.dropout_mask(2024, 0, 1, thr, R, N), "module": LF.dropout_mask(2024, 1, 0, thr, R, N)}
    for name, m in [("base", base)] + list(others.items()):
        kept = 1.0 - m.mean()
        print(f"p={p} {name}: kept {kept:.6f}  expected {q:.6f}  ({abs(kept - q) / sd:.2f} sd)")
        assert abs(kept - q) <= 5 * sd
    a = q * q + (1 - q) * (1 - q)
    sda = math.sqrt(a * (1 - a) / n)
    for name, m in others.items():
        agree = (m == base).mean()
        print(f"p={p} {name}: agreement {agree:.6f}  expected {a:.6f}  ({abs(agree - a) / sda:.2f} sd)")
        assert abs(agree - a) <= 5 * sda


def _state(seed=11, module=2):
    return LF.DropoutState(torch.device("cpu"), seed, module)


@pytest.mark.parametrize("shape", [(6, 10), (4, 6, 20)], ids=str)
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_forward_and_backward_values(shape, p):
    g0 = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g0, requires_grad=True)
    g = torch.randn(*shape, generator=g0)
    st = _state()
    y = LF.dropout(x, p, True, st)
    y.backward(g)
    thr = LF.dropout_thr(p)
    N = shape[-1]
    drop = torch.from_numpy(LF.dropout_mask(11, 2, 0, thr, x.numel() // N, N)).view(shape)
    scale = float(LF.dropout_scale(thr))
    assert 0 < drop.sum() < drop.numel()
    assert torch.equal(y.detach(), torch.where(drop, torch.zeros(()), x.detach() * scale))
    assert torch.equal(x.grad, torch.where(drop, torch.zeros(()), g * scale))
    # bf16 in, bf16 out: one rounding of the fp32 product, as the kernel does
    xb = x.detach().bfloat16()
    yb = LF.dropout(xb, p, True, _state())
    assert yb.dtype == torch.bfloat16
    assert torch.equal(yb, torch.where(drop, torch.zeros(()), xb.float() * scale).bfloat16())


def test_shortcuts_and_checks():
    x = torch.randn(3, 7)
    st = _state()
    assert LF.dropout(x, 0.0, True, st) is x and LF.dropout(x, 0.5, False, st) is x
    assert LF.dropout(x, 0.0, True, None) is x and st.read()["counter"] == 0
    y = LF.dropout(x, 1.0, True, st)
    assert torch.equal(y, torch.zeros_like(x)) and not torch.signbit(y).any()
    with pytest.raises(ValueError):
        LF.dropout(x, 0.5, True, None)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError):
            LF.dropout(x, bad, True, st)
        with pytest.raises(ValueError):
            Dropout(bad)
    with pytest.raises(ValueError):
        Dropout(0.5, inplace=True)
    d = Dropout(0.5)
    assert d.eval()(x) is x
    d.train()
    d.p = 0.0
    assert d(x) is x and d.__dict__["_ldnn_drop"] is None      # nothing allocated
    d.p = 1.0
    assert torch.equal(d(x), torch.zeros_like(x))
    d.p = 1.5
    with pytest.raises(ValueError):
        d(x)


def test_module_state_is_no_parameter_or_buffer():
    d = Dropout(0.5)
    d(torch.randn(2, 4))
    assert d.__dict__["_ldnn_drop"] is not None
    assert list(d.state_dict()) == [] and list(d.buffers()) == [] and list(d.parameters()) == []


def test_counter_reseed_and_changed_rate():
    x = torch.ones(5, 12)
    d = Dropout(0.5)
    assert reseed_dropout(d, 77) == 1
    ys = []
    for k in range(3):
        assert d.__dict__["_ldnn_drop"] is None or d.__dict__["_ldnn_drop"].read()["counter"] == k
        ys.append(d(x))
    assert d.__dict__["_ldnn_drop"].read() == dict(seed=77, module_index=0, counter=3, thr=32768)
    for k, y in enumerate(ys):
        assert torch.equal(y == 0, torch.from_numpy(LF.dropout_mask(77, 0, k, 32768, 5, 12)))
    assert not torch.equal(ys[0], ys[1])
    reseed_dropout(d, 77)
    assert d.__dict__["_ldnn_drop"].read()["counter"] == 0 and torch.equal(d(x), ys[0])
    # a changed rate takes effect on the next call: mask and scale
    d.p = 0.25
    y = d(x)
    drop = torch.from_numpy(LF.dropout_mask(77, 0, 1, 16384, 5, 12))
    assert torch.equal(y, torch.where(drop, torch.zeros(()), x * float(np.float32(65536.0) / np.float32(49152.0))))
    # modules are numbered in modules() order, also through a wrapper module
    net = torch.nn.Sequential(Dropout(0.5), torch.nn.Sequential(torch.nn.Identity(), Dropout(0.5)), Dropout(0.5))
    wrapped = torch.nn.Sequential(net)
    assert ldnn.reseed_dropout(wrapped, 5) == 3
    outs = [m(x) for m in (net[0], net[1][1], net[2])]
    for k, y in enumerate(outs):
        assert torch.equal(y == 0, torch.from_numpy(LF.dropout_mask(5, k, 0, 32768, 5, 12))), k


# ---- models ------------------------------------------------------------------------------------
N_DROPOUTS = {"enhanced_cnn": 1, "enhanced_cnn_small": 1, "lenet5": 2, "mlp2": 1, "mlp3": 2, "mlp3_small": 2,
              "resnet18": 1, "resnet18_cifar": 1}
INPUT = {"cifar10": (2, 3, 32, 32), "mnist": (2, 1, 28, 28), "imagenet": (2, 3, 64, 64)}


@pytest.mark.parametrize("name", sorted(REGISTRY))
def test_models_take_the_rate(name):
    assert set(N_DROPOUTS) == set(REGISTRY)
    ctor, kind = REGISTRY[name]
    nc = 10
    plain = ctor(nc)
    zero = build_model(name, nc, dropout=0.0)
    half = build_model(name, nc, dropout=0.5)
    names = [n for n, _ in plain.named_modules()]
    assert [n for n, _ in zero.named_modules()] == names and [n for n, _ in ctor(nc, dropout=0.0).named_modules()] == names
    assert list(zero.state_dict()) == list(plain.state_dict()) == list(half.state_dict())
    assert not any(isinstance(m, Dropout) for m in zero.modules())
    drops = [m for m in half.modules() if isinstance(m, Dropout)]
    assert len(drops) == N_DROPOUTS[name] and all(m.p == 0.5 for m in drops)
    assert [n for n, _ in half.named_buffers()] == [n for n, _ in plain.named_buffers()]
    half.load_state_dict(plain.state_dict())
    ldnn.prepare(plain, "cpu")
    ldnn.prepare(half, "cpu")
    x = torch.randn(*INPUT[kind], generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert torch.equal(half.eval()(x), plain.eval()(x))
        if name.startswith("mlp") or name == "lenet5":    # (no BatchNorm: the training-mode outputs compare too)
            reseed_dropout(half, 1)
            assert not torch.equal(half.train()(x), plain.train()(x))


def test_mlp_places_dropout_after_each_hidden_activation():
    m = build_model("mlp3_small", dropout=0.5)
    ldnn.prepare(m, "cpu")
    reseed_dropout(m, 9)
    x = torch.randn(4, 784, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        h = x
        for k in (0, 1):
            h = torch.relu(torch.nn.functional.linear(h, m.layers[k].weight, m.layers[k].bias))
            h = torch.where(torch.from_numpy(LF.dropout_mask(9, k, 0, 32768, 4, 1024)), torch.zeros(()), h * 2.0)
        want = torch.nn.functional.linear(h, m.layers[2].weight, m.layers[2].bias)
        torch.testing.assert_close(m.train()(x), want, rtol=1e-5, atol=1e-5)


# ---- CLI ---------------------------------------------------------------------------------------
def test_cli_refuses_bad_rates_and_the_static_engine(monkeypatch):
    from ldnn.models.mlp import mlp3

    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit, match="--dropout"):
            cli.main(["--dropout", bad])
    p = cli.build_parser()
    assert p.parse_args([]).dropout == 0.0
    cpu = torch.device("cpu")
    with monkeypatch.context() as mp:
        mp.setattr(cli, "native_gpu", lambda dev: True)
        a = p.parse_args(["--model", "mlp3_small", "--engine", "static", "--dropout", "0.5"])
        with pytest.raises(SystemExit, match="--dropout runs on the autograd path"):
            cli.resolve_engine(a, mlp3(784, 64, 10, dropout=0.5), cpu, 1)
        a = p.parse_args(["--model", "mlp3_small", "--engine", "auto", "--dropout", "0.5"])
        assert cli.resolve_engine(a, mlp3(784, 64, 10, dropout=0.5), cpu, 1) is False
        a = p.parse_args(["--model", "mlp3_small", "--engine", "static"])
        assert cli.resolve_engine(a, mlp3(784, 64, 10), cpu, 1) is True


def _train(out, epochs, extra=()):
    res = cli.main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "320", "--n_test", "64", "--epochs_global",
                    str(epochs), "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(out), "--plots", "",
                    "--checkpoint_every", "1", "--partition_rule", "equal", "--time_limit", "0", "--lr", "0.01",
                    "--seed", "3", "--no_eval", "--batch_size", "32", "--dropout", "0.5", *extra])
    return res["histories"]


def _flat(h):
    out = []
    for v in h:
        out.extend(_flat(v) if isinstance(v, (list, tuple)) else [float(v)])
    return out


def test_cli_run_is_reproducible_and_resumes(tmp_path):
    ha = _train(tmp_path / "a", 2)
    assert len(ha) == 12 and len(ha[4]) == 2 and all(math.isfinite(v) for v in _flat(ha))
    hb = _train(tmp_path / "b", 2)
    assert _flat(ha) == _flat(hb)
    off = cli.main(["--model", "mlp2", "--dataset", "mnist", "--n_train", "320", "--n_test", "64", "--epochs_global",
                    "1", "--epochs_local", "1", "--device", "cpu", "--quiet", "--out_dir", str(tmp_path / "off"),
                    "--plots", "", "--partition_rule", "equal", "--time_limit", "0", "--lr", "0.01", "--seed", "3",
                    "--no_eval", "--batch_size", "32"])["histories"]
    assert off[4][0] != ha[4][0]          # the flag reached the model
    _train(tmp_path / "c", 1)
    hc = _train(tmp_path / "c", 2, ["--resume", "latest"])
    assert len(hc[4]) == 2 and _flat(hc) == _flat(ha)
