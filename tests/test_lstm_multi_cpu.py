"""Stacked multi-model LSTM (models/lstm_multi.py) and the service's
train_many / predict_many on CPU: the stacked pass must be the arithmetic
of M separate single models."""

import asyncio
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

M, F, SEQ, HIDDEN = 3, 9, 8, (64, 32)


def _singles(seeds=(0, 1, 2)):
    from ai_crypto_trader_amd.models.lstm import LSTMPricePredictor

    out = []
    for s in seeds:
        torch.manual_seed(s)
        out.append(LSTMPricePredictor(F, SEQ, HIDDEN))
    return out


def _stacked(models):
    from ai_crypto_trader_amd.models.lstm_multi import (
        StackedLSTMPricePredictor,
    )
    return StackedLSTMPricePredictor.from_models(models)


def _market(lengths, seed=11):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    c = candles_chl_v(generate_ohlcv(max(lengths), len(lengths), seed=seed))
    return {f"S{i}USDC": c[i, -n:].astype(np.float32)
            for i, n in enumerate(lengths)}


def _service(**nn_cfg):
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.neural_network import (
        NeuralNetworkService,
    )
    cfg = AppConfig()
    for k, v in nn_cfg.items():
        setattr(cfg.neural_network, k, v)
    return NeuralNetworkService(InProcessBus(), cfg, device="cpu")


def test_forward_parity():
    models = _singles()
    stacked = _stacked(models)
    torch.manual_seed(10)
    x = torch.randn(M, 32, SEQ, F)
    with torch.no_grad():
        out = stacked(x)
        ref = torch.stack([m(x[i]) for i, m in enumerate(models)])
    assert out.shape == (M, 32)
    print("forward max diff", float((out - ref).abs().max()))
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-5)


def test_training_parity():
    models = _singles()
    stacked = _stacked(models)
    torch.manual_seed(11)
    N, B, steps = 256, 32, 40
    x = torch.randn(M, N, SEQ, F)
    y = torch.randn(M, N)
    g = torch.Generator().manual_seed(12)
    batches = [torch.randint(0, N, (B,), generator=g) for _ in range(steps)]

    opt = torch.optim.Adam(stacked.parameters(), lr=1e-3)
    for j in batches:
        opt.zero_grad()
        ((stacked(x[:, j]) - y[:, j]) ** 2).mean(dim=1).sum().backward()
        opt.step()

    opts = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in models]
    for j in batches:
        for i, (m, o) in enumerate(zip(models, opts)):
            o.zero_grad()
            ((m(x[i, j]) - y[i, j]) ** 2).mean().backward()
            o.step()

    worst = 0.0
    for i, m in enumerate(models):
        got = stacked.model_state_dict(i)
        for k, v in m.state_dict().items():
            worst = max(worst, float((got[k] - v).abs().max()))
            torch.testing.assert_close(got[k], v, rtol=0, atol=1e-5)
    print("training max param diff", worst)


def test_models_are_independent():
    stacked = _stacked(_singles())
    torch.manual_seed(13)
    x = torch.randn(M, 32, SEQ, F)
    x2 = x.clone()
    x2[2] += 1.0
    with torch.no_grad():
        a, b = stacked(x), stacked(x2)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert not torch.equal(a[2], b[2])


def test_export_load_round_trip(tmp_path):
    from ai_crypto_trader_amd.models.lstm import LSTMPricePredictor

    models = _singles()
    stacked = _stacked(models)
    fresh = LSTMPricePredictor(F, SEQ, HIDDEN).state_dict()
    for i in range(M):
        sd = stacked.export_model(i).state_dict()
        assert list(sd) == list(fresh)
        assert {k: v.shape for k, v in sd.items()} == \
            {k: v.shape for k, v in fresh.items()}
        for k, v in models[i].state_dict().items():
            assert torch.equal(sd[k], v), k
    # load_model then export_model is exact
    torch.manual_seed(99)
    other = LSTMPricePredictor(F, SEQ, HIDDEN)
    stacked.load_model(1, other.state_dict())
    back = stacked.export_model(1).state_dict()
    for k, v in other.state_dict().items():
        assert torch.equal(back[k], v), k
    # neighbours untouched
    for k, v in models[0].state_dict().items():
        assert torch.equal(stacked.model_state_dict(0)[k], v), k
    with pytest.raises(KeyError):
        stacked.load_model(0, {"l1.w_ih": fresh["l1.w_ih"]})

    # a checkpoint written after train_many loads through load()
    svc = _service()
    data = _market([300, 300])
    svc.train_many(data, epochs=1)
    svc.save(str(tmp_path))
    svc2 = _service()
    assert svc2.load(str(tmp_path)) == 2
    for sym in data:
        a, b = svc.models[sym].state_dict(), svc2.models[sym].state_dict()
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (sym, k)


def test_train_many_lengths_and_truncation():
    from ai_crypto_trader_amd.models.lstm import LSTMPricePredictor

    svc = _service()
    seq = svc.config.neural_network.seq_len
    data = _market([123, 400, 600])       # 63 / 340 / 540 windows
    short, mid, long_ = list(data)
    torch.manual_seed(0)
    res = svc.train_many(data, epochs=2)
    assert set(res) == set(data)
    assert math.isnan(res[short])
    assert short not in svc.models and short not in svc.scalers
    for sym in (mid, long_):
        assert np.isfinite(res[sym])
        assert type(svc.models[sym]) is LSTMPricePredictor
        assert sym in svc.scalers
        assert svc.val_loss[sym] == res[sym]
    # tail-aligned to the shortest trainable history
    info = svc.last_train_many
    assert info["symbols"] == [mid, long_]
    assert info["candles"] == 400
    assert info["windows"] == 400 - seq
    assert info["train_windows"] + info["val_windows"] == 400 - seq
    assert info["val_windows"] == (400 - seq) // 10
    assert svc.trained == 2
    # the long symbol's scaler saw only its most recent 400 candles
    from ai_crypto_trader_amd.services.neural_network import (
        MinMaxScaler, build_features,
    )
    ref = MinMaxScaler().fit(build_features(data[long_][-400:]))
    np.testing.assert_array_equal(svc.scalers[long_].lo, ref.lo)
    np.testing.assert_array_equal(svc.scalers[long_].hi, ref.hi)
    # the unchanged single-model paths work on the results
    assert svc.predict(long_, data[long_]) is not None
    assert svc.snapshot_for_regime(mid, "bull") == (mid, "bull")


def test_early_stopped_model_is_frozen():
    from ai_crypto_trader_amd.services.neural_network import (
        NeuralNetworkService,
    )

    stacked = _stacked(_singles())
    opt = torch.optim.Adam(stacked.parameters(), lr=1e-2)
    torch.manual_seed(14)
    x = torch.randn(M, 32, SEQ, F)
    y = torch.randn(M, 32)
    step = NeuralNetworkService._stacked_step
    for _ in range(3):                    # builds Adam momentum for all
        step(stacked, opt, x, y, {})
    before = [{k: v.clone() for k, v in stacked.model_state_dict(i).items()}
              for i in range(M)]
    frozen = {1: stacked.snapshot_model(1)}
    for _ in range(4):
        step(stacked, opt, x, y, frozen)
    after = [stacked.model_state_dict(i) for i in range(M)]
    for k in before[1]:
        assert torch.equal(before[1][k], after[1][k]), k
    for i in (0, 2):
        assert any(not torch.equal(before[i][k], after[i][k])
                   for k in before[i])


def test_predict_many_matches_predict_and_cache_invalidates():
    svc = _service()
    data = _market([400, 400, 400])
    torch.manual_seed(1)
    svc.train_many(data, epochs=1)
    data["NOMODEL"] = data[next(iter(data))]
    many = svc.predict_many(data)
    assert set(many) == set(data)
    assert many["NOMODEL"] is None
    for sym in list(data)[:3]:
        one = svc.predict(sym, data[sym])
        assert set(many[sym]) == set(one)
        assert abs(many[sym]["predicted_change_pct"]
                   - one["predicted_change_pct"]) < 1e-5
        for k in ("symbol", "current_price", "confidence",
                  "training_metrics", "features_used"):
            assert many[sym][k] == one[k], k
    # cached while nothing changes
    cached = svc._stacked_cache[2]
    svc.predict_many(data)
    assert svc._stacked_cache[2] is cached
    # retraining one symbol in place (train() keeps the model object)
    sym = next(iter(data))
    svc.config.neural_network.lr = 1e-2
    svc.train(sym, data[sym], epochs=1)
    again = svc.predict_many(data)
    assert svc._stacked_cache[2] is not cached
    assert again[sym]["predicted_change_pct"] != \
        many[sym]["predicted_change_pct"]
    assert abs(again[sym]["predicted_change_pct"]
               - svc.predict(sym, data[sym])["predicted_change_pct"]) < 1e-5


def test_serve_predict_many_cold_start_goes_through_train_many(tmp_path):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from serve import build_server

    app, nn = build_server(str(tmp_path), device="cpu")
    assert nn.config.neural_network.stacked
    data = _market([300, 300])
    body = {"candles": {s: c.tolist() for s, c in data.items()}}
    with TestClient(app) as c:
        out = c.post("/predict_many", json=body).json()
    assert nn.last_train_many["symbols"] == list(data)
    assert set(out) == set(data)
    for sym in data:
        assert np.isfinite(out[sym]["predicted_change_pct"])
        one = nn.predict(sym, data[sym])
        assert abs(out[sym]["predicted_change_pct"]
                   - one["predicted_change_pct"]) < 1e-5


@pytest.mark.parametrize("stacked,n_sym,expect_many",
                         [(True, 2, True), (True, 1, False),
                          (False, 2, False)])
def test_loop_routing(stacked, n_sym, expect_many):
    svc = _service(stacked=stacked)
    calls = {"train": 0, "train_many": 0, "predict": 0, "predict_many": 0}
    syms = [f"S{i}USDC" for i in range(n_sym)]
    for s in syms:
        svc.candles[s] = [[1.0, 1.0, 1.0, 1.0]] * 256

    def train(sym, candles, epochs=None, batch=None):
        calls["train"] += 1
        svc.models[sym] = object()
        return 0.0

    def train_many(data, epochs=None, batch=None):
        calls["train_many"] += 1
        assert sorted(data) == syms
        for s in data:
            svc.models[s] = object()
        return {s: 0.0 for s in data}

    def predict(sym, candles, regime=None):
        calls["predict"] += 1
        return None

    def predict_many(data, regime=None):
        calls["predict_many"] += 1
        return {s: None for s in data}

    async def stop_after_first_pass(_seconds):
        svc.running = False

    svc.train, svc.train_many = train, train_many
    svc.predict, svc.predict_many = predict, predict_many
    svc.sleep = stop_after_first_pass

    async def go():
        svc.running = True
        await svc._train_loop()
        svc.running = True
        await svc._predict_loop()

    asyncio.run(go())
    if expect_many:
        assert calls == {"train": 0, "train_many": 1, "predict": 0,
                         "predict_many": 1}
    else:
        assert calls == {"train": n_sym, "train_many": 0,
                         "predict": n_sym, "predict_many": 0}
