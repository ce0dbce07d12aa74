"""GPU tests for the multi-model LSTM recurrence (lstm_seq_*_multi in
ops/hip/lstm.hip) and the stacked model / service paths built on it.

The kernel tests are bitwise: a model's slab out of the multi launch must
equal the single-model launch on that model's inputs alone. Every model
gets different weights and biases, so a missing per-model stride shows.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 5), (3, 64, 5), (3, 128, 7)]      # (M, B, T)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ops():
    from ai_crypto_trader_amd.ops import require_hip_ops
    return require_hip_ops()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _inputs(H, M, B, T, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * H + M * B + T)
    dev = torch.device("cuda:0")
    xproj = torch.randn(M, T, B, 4 * H, generator=g).bfloat16().to(dev)
    w = (torch.randn(M, H, 4 * H, generator=g) * H ** -0.5).bfloat16()
    wt = w.transpose(1, 2).contiguous().to(dev)      # (M, 4H, H)
    w = w.contiguous().to(dev)                       # (M, H, 4H)
    bias = (torch.randn(M, 4 * H, generator=g) * 0.5).float().to(dev)
    dh_up = torch.randn(M, T, B, H, generator=g).float().to(dev)
    return xproj, wt, w, bias, dh_up


def _fwd_multi(xproj, wt, bias, save_mode=1):
    M, T, B, H4 = xproj.shape
    H, dev = H4 // 4, xproj.device
    h = torch.full((M, T, B, H), float("nan"), dtype=torch.bfloat16,
                   device=dev)
    if save_mode:
        gates = torch.full((M, T, B, H4), float("nan"),
                           dtype=torch.bfloat16, device=dev)
        c = torch.full((M, T, B, H), float("nan"), device=dev)
        gp, cp = gates.data_ptr(), c.data_ptr()
    else:
        gates = c = None
        gp = cp = 0
    _ops().lstm_seq_fwd_multi(xproj.data_ptr(), wt.data_ptr(),
                              bias.data_ptr(), h.data_ptr(), gp, cp, M, B, T,
                              H, save_mode, _stream(dev))
    return h, gates, c


def _fwd_single(xproj, wt, bias):
    T, B, H4 = xproj.shape
    H, dev = H4 // 4, xproj.device
    h = torch.empty((T, B, H), dtype=torch.bfloat16, device=dev)
    gates = torch.empty((T, B, H4), dtype=torch.bfloat16, device=dev)
    c = torch.empty((T, B, H), device=dev)
    _ops().lstm_seq_fwd(xproj.data_ptr(), wt.data_ptr(), bias.data_ptr(),
                        h.data_ptr(), gates.data_ptr(), c.data_ptr(), B, T,
                        H, 1, _stream(dev))
    return h, gates, c


def _bwd_multi(dh_up, gates, c, w):
    M, T, B, H = dh_up.shape
    dg = torch.full((M, T, B, 4 * H), float("nan"), dtype=torch.bfloat16,
                    device=dh_up.device)
    _ops().lstm_seq_bwd_multi(dh_up.data_ptr(), gates.data_ptr(),
                              c.data_ptr(), w.data_ptr(), dg.data_ptr(), M,
                              B, T, H, _stream(dh_up.device))
    return dg


def _bwd_single(dh_up, gates, c, w):
    T, B, H = dh_up.shape
    dg = torch.empty((T, B, 4 * H), dtype=torch.bfloat16,
                     device=dh_up.device)
    _ops().lstm_seq_bwd(dh_up.data_ptr(), gates.data_ptr(), c.data_ptr(),
                        w.data_ptr(), dg.data_ptr(), B, T, H,
                        _stream(dh_up.device))
    return dg


@functools.lru_cache(maxsize=None)
def _case(H, M, B, T):
    """Multi-launch results plus the per-model single-launch references,
    computed once per shape and shared by the forward and backward tests
    (read-only)."""
    xproj, wt, w, bias, dh_up = _inputs(H, M, B, T)
    h, gates, c = _fwd_multi(xproj, wt, bias)
    dg = _bwd_multi(dh_up, gates, c, w)
    singles = []
    for m in range(M):
        hs, gs, cs = _fwd_single(xproj[m].contiguous(), wt[m].contiguous(),
                                 bias[m].contiguous())
        dgs = _bwd_single(dh_up[m].contiguous(), gs, cs, w[m].contiguous())
        singles.append((hs, gs, cs, dgs))
    torch.cuda.synchronize()
    return dict(xproj=xproj, wt=wt, w=w, bias=bias, dh_up=dh_up, h=h,
                gates=gates, c=c, dg=dg, singles=singles)


@pytest.mark.parametrize("M,B,T", SHAPES)
@pytest.mark.parametrize("H", [64, 32])
def test_fwd_multi_bit_equal_to_single(dev, H, M, B, T):
    r = _case(H, M, B, T)
    for m, (hs, gs, cs, _) in enumerate(r["singles"]):
        assert torch.isfinite(hs.float()).all()
        assert torch.equal(r["h"][m], hs), f"h model {m}"
        assert torch.equal(r["gates"][m], gs), f"gates model {m}"
        assert torch.equal(r["c"][m], cs), f"c model {m}"
    if M > 1:       # different weights really give different models
        assert not torch.equal(r["h"][0], r["h"][1])


@pytest.mark.parametrize("H", [64, 32])
def test_fwd_multi_inference_mode(dev, H):
    """save_mode 0 with null save pointers: same h, nothing else stored."""
    M, B, T = SHAPES[2]
    r = _case(H, M, B, T)
    h, _, _ = _fwd_multi(r["xproj"], r["wt"], r["bias"], save_mode=0)
    torch.cuda.synchronize()
    assert torch.equal(h, r["h"])


@pytest.mark.parametrize("M,B,T", SHAPES)
@pytest.mark.parametrize("H", [64, 32])
def test_bwd_multi_bit_equal_to_single(dev, H, M, B, T):
    r = _case(H, M, B, T)
    for m, (_, _, _, dgs) in enumerate(r["singles"]):
        assert torch.isfinite(dgs.float()).all()
        assert torch.equal(r["dg"][m], dgs), f"dgates model {m}"


@pytest.mark.parametrize("H", [64, 32])
def test_models_independent_on_device(dev, H):
    M, B, T = SHAPES[2]
    r = _case(H, M, B, T)
    xproj, wt, w, bias = (r[k].clone() for k in ("xproj", "wt", "w", "bias"))
    xproj[1] += 1.0
    wt[1] *= 0.5
    w[1] *= 0.5
    bias[1] += 0.25
    h, gates, c = _fwd_multi(xproj, wt, bias)
    dg = _bwd_multi(r["dh_up"], gates, c, w)
    torch.cuda.synchronize()
    for m in (0, 2):
        assert torch.equal(h[m], r["h"][m])
        assert torch.equal(gates[m], r["gates"][m])
        assert torch.equal(c[m], r["c"][m])
        assert torch.equal(dg[m], r["dg"][m])
    assert not torch.equal(h[1], r["h"][1])


def test_bad_arguments_raise_before_launch(dev):
    ops = _ops()
    s = _stream(dev)
    for M, B, H in [(2, 32, 64), (2, 96, 64), (0, 64, 64), (2, 64, 48)]:
        with pytest.raises(RuntimeError, match="lstm_fwd_multi: "):
            ops.lstm_seq_fwd_multi(0, 0, 0, 0, 0, 0, M, B, 4, H, 0, s)
        with pytest.raises(RuntimeError, match="lstm_bwd_multi: "):
            ops.lstm_seq_bwd_multi(0, 0, 0, 0, 0, M, B, 4, H, s)


@pytest.mark.parametrize("B", [64, 40])      # 40: the pad-to-64 path
def test_stacked_layer_matches_f32_reference(dev, B):
    """Tolerances are test_lstm_fwd/bwd_matches_reference's: forward
    rtol=atol=5e-2, gradients max-relative 0.08, here per model."""
    from ai_crypto_trader_amd.models.lstm_multi import StackedLSTMLayer

    torch.manual_seed(1)
    M, T, F, H = 3, 12, 9, 64
    ref_layer = StackedLSTMLayer(M, F, H)
    with torch.no_grad():                     # non-trivial biases
        ref_layer.b_ih.uniform_(-0.1, 0.1)
        ref_layer.b_hh.uniform_(-0.1, 0.1)
    gpu_layer = StackedLSTMLayer(M, F, H)
    gpu_layer.load_state_dict(ref_layer.state_dict())
    gpu_layer = gpu_layer.to(dev)

    x = torch.randn(M, T, B, F, requires_grad=True)
    out_ref = ref_layer._forward_reference(x)
    (out_ref ** 2).mean().backward()

    xg = x.detach().clone().to(dev).requires_grad_(True)
    out_g = gpu_layer(xg)
    (out_g.float() ** 2).mean().backward()
    torch.cuda.synchronize()

    assert out_g.dtype == torch.bfloat16 and out_g.shape == (M, T, B, H)
    torch.testing.assert_close(out_g.float().cpu(), out_ref.detach(),
                               rtol=5e-2, atol=5e-2)

    def rel(a, b):
        return float((a - b).abs().max() / (b.abs().max() + 1e-8))

    pairs = [("x", xg.grad, x.grad),
             ("w_ih", gpu_layer.w_ih.grad, ref_layer.w_ih.grad),
             ("w_hh", gpu_layer.w_hh.grad, ref_layer.w_hh.grad),
             ("b_hh", gpu_layer.b_hh.grad, ref_layer.b_hh.grad)]
    for m in range(M):
        for name, got, want in pairs:
            r = rel(got[m].cpu().float(), want[m])
            print(f"B={B} model {m} d{name} max-rel {r:.4f}")
            assert r < 0.08, (m, name, r)

    with torch.no_grad():                     # inference path, same h
        out_inf = gpu_layer(xg.detach())
    torch.cuda.synchronize()
    assert torch.equal(out_inf, out_g.detach())


def test_stacked_predictor_trains(dev):
    """test_lstm_predictor_trains' bar (last < 0.7 x first), per model."""
    from ai_crypto_trader_amd.models.lstm_multi import (
        StackedLSTMPricePredictor,
    )

    torch.manual_seed(2)
    M, B = 3, 256
    model = StackedLSTMPricePredictor(M, n_features=9, seq_len=30).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    x = torch.randn(B, 30, 9, device=dev)
    y = torch.stack([x[:, -5:, k].mean(dim=1) for k in range(M)])
    xs = x.expand(M, B, 30, 9)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        per_model = ((model(xs) - y) ** 2).mean(dim=1)
        per_model.sum().backward()
        opt.step()
        losses.append(per_model.detach().cpu())
    for k in range(M):
        first, last = float(losses[0][k]), float(losses[-1][k])
        print(f"model {k}: loss {first:.4f} -> {last:.4f}")
        assert last < first * 0.7, (k, first, last)


def test_service_train_many_predict_many_on_device(dev):
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.neural_network import (
        NeuralNetworkService,
    )

    c = candles_chl_v(generate_ohlcv(600, 3, seed=5)).astype(np.float32)
    data = {f"S{i}USDC": c[i] for i in range(3)}
    svc = NeuralNetworkService(InProcessBus(), AppConfig(), device="cuda:0")
    torch.manual_seed(3)
    res = svc.train_many(data, epochs=2)
    assert set(res) == set(data)
    assert all(np.isfinite(v) for v in res.values()), res
    many = svc.predict_many(data)
    for sym in data:
        one = svc.predict(sym, data[sym])
        assert set(many[sym]) == set(one)
        d = abs(many[sym]["predicted_change_pct"]
                - one["predicted_change_pct"])
        print(f"{sym}: stacked vs single predicted_change_pct diff {d:.2e}")
        assert d < 5e-2
