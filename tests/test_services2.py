"""Second service batch: social/news/order-book/arbitrage/grid/DCA/
registry/explainability/feature-importance/selection/patterns."""

import asyncio
import time

import numpy as np
import pytest

from ai_crypto_trader_amd.bus.message_bus import InProcessBus
from ai_crypto_trader_amd.config import AppConfig
from ai_crypto_trader_amd.services.arbitrage import PairGraph
from ai_crypto_trader_amd.services.news import (
    NewsAnalyzer, SyntheticNewsSource,
)
from ai_crypto_trader_amd.services.order_book import OrderBookAnalyzer
from ai_crypto_trader_amd.services.registry import (
    AIExplainabilityService, FeatureImportanceIntegrator,
)
from ai_crypto_trader_amd.services.social import SocialMetricsAnalyzer
from ai_crypto_trader_amd.services.strategy_selection import (
    StrategySelectionService,
)
from ai_crypto_trader_amd.utils.exchange import FakeExchange


# ------------------------------- social ------------------------------------

def test_lead_lag_recovers_known_lead():
    """Sentiment constructed to lead returns by 3 steps must be detected
    with a positive-lag peak."""
    rng = np.random.default_rng(0)
    an = SocialMetricsAnalyzer(max_lag=10)
    n = 600
    ret = rng.standard_normal(n) * 0.001
    price = np.exp(np.cumsum(ret))
    lead = 3
    for t in range(n - lead):
        sent = 0.5 + 40 * ret[t + lead] + rng.standard_normal() * 0.005
        an.record("X", float(sent), float(price[t]), ts=float(t))
    ll = an.lead_lag("X")
    # analyzer convention: lag k pairs s[t] with the return over candle
    # (t+k, t+k+1]; a sentiment coupled to the return INTO t+3 peaks at k=2
    assert ll["lag"] == lead - 1
    assert ll["pearson"] > 0.5
    assert abs(ll["spearman"]) > 0.3


def test_decayed_sentiment_weighting():
    an = SocialMetricsAnalyzer(half_life_h=1.0)
    now = 1_000_000.0
    an.record("X", 0.9, 1.0, ts=now - 7200)    # 2 half-lives old
    an.record("X", 0.1, 1.0, ts=now)
    s = an.decayed_sentiment("X", now=now)
    assert 0.1 < s < 0.5        # recent bearish dominates
    assert s < 0.3


# ------------------------------- news --------------------------------------

def test_news_sentiment_and_entities():
    na = NewsAnalyzer()
    assert na.sentiment("Bitcoin surges to record high on ETF approval") > 0.6
    assert na.sentiment("Massive hack triggers crash and liquidations") < 0.4
    assert abs(na.sentiment("Bitcoin trades sideways") - 0.5) < 0.15
    ents = na.entities("Ethereum and $SOL rally while Bitcoin dips")
    assert "ETH" in ents and "SOL" in ents and "BTC" in ents
    assert "regulation" in na.topics("SEC lawsuit threatens approval")
    assert na.relevance("Bitcoin surges", "BTCUSDC") >= 0.7


def test_synthetic_news_deterministic():
    a = SyntheticNewsSource(seed=1).headlines("BTCUSDC", 3)
    b = SyntheticNewsSource(seed=1).headlines("BTCUSDC", 3)
    assert a == b


# ----------------------------- order book ----------------------------------

def test_order_book_analyzer():
    ex = FakeExchange()
    ex.prices["BTCUSDC"] = 100.0
    book = ex.get_order_book("BTCUSDC", limit=50)
    a = OrderBookAnalyzer().analyze(book)
    assert a["ok"]
    assert a["spread_bps"] > 0
    assert -1 <= a["imbalance"] <= 1
    assert a["price_impact"]["10000"]["buy_impact_bps"] >= 0
    assert len(a["levels"]["support"]) >= 1
    assert 0 <= a["microstructure"]["gini"] <= 1
    assert a["signal"]["direction"] in ("bullish", "bearish", "neutral")

    # skewed book -> buy pressure
    book["bids"] = [[99.9, 100.0], [99.8, 100.0]]
    book["asks"] = [[100.1, 1.0], [100.2, 1.0]]
    a2 = OrderBookAnalyzer().analyze(book)
    assert a2["pressure"] == "buy" and a2["imbalance"] > 0.5


# ----------------------------- arbitrage -----------------------------------

def test_triangle_arbitrage_detection():
    g = PairGraph(fee=0.0)
    # consistent prices -> no profit
    g.add_pair("BTC", "USDC", 100.0)
    g.add_pair("ETH", "USDC", 10.0)
    g.add_pair("ETH", "BTC", 0.1)
    cycles = g.cycles("USDC")
    assert cycles, "triangle must be found"
    assert all(abs(g.cycle_profit(c) - 1.0) < 1e-9 for c in cycles)
    # mispriced ETH/BTC -> profitable cycle exists
    g.add_pair("ETH", "BTC", 0.095)
    profits = [g.cycle_profit(c) for c in g.cycles("USDC")]
    assert max(profits) > 1.02
    # fees eat it
    g.fee = 0.02
    assert max(g.cycle_profit(c) for c in g.cycles("USDC")) < 1.0


# ----------------------------- grid / dca ----------------------------------

def test_grid_strategy_fills():
    async def go():
        bus = InProcessBus()
        from ai_crypto_trader_amd.services.grid_dca import (
            GridTradingStrategy,
        )
        g = GridTradingStrategy(bus, FakeExchange(), "BTCUSDC", AppConfig())
        g.build_grid(1.0)
        assert len(g.levels) >= 8
        buys = [lv for lv in g.levels if lv["side"] == "BUY"]
        sells = [lv for lv in g.levels if lv["side"] == "SELL"]
        assert buys and sells
        fills = g.on_price(min(lv["price"] for lv in buys) - 1e-6)
        assert any(f["side"] == "BUY" for f in fills)
        fills = g.on_price(max(lv["price"] for lv in sells) + 1e-6)
        assert any(f["side"] == "SELL" for f in fills)
        assert g.pnl > 0
        # breakout rebuilds around the new price
        g.on_price(2.0)
        assert abs(g.center - 2.0) < 1e-9

    asyncio.run(go())


def test_dca_strategy_schedule_and_dip():
    async def go():
        bus = InProcessBus()
        from ai_crypto_trader_amd.services.grid_dca import DCAStrategy
        cfg = AppConfig()
        d = DCAStrategy(bus, FakeExchange(), "BTCUSDC", cfg,
                        candles_per_period=10)
        for i in range(1, 10):
            assert await d.maybe_buy(1.0, 0.5, "ranging") is None or i == 10
        rec = await d.maybe_buy(1.0, 0.5, "ranging")     # 10th tick
        assert rec is not None and not rec["dip"]
        # build history then dip
        for _ in range(130):
            d.recent.append(1.0)
        rec2 = await d.maybe_buy(1.0 * (1 - cfg.dca.dip_threshold_pct - 0.01),
                                 0.5, "ranging")
        assert rec2 is not None and rec2["dip"]
        assert rec2["usd"] > rec["usd"]                  # dip multiplier

    asyncio.run(go())


# ------------------------ registry / explainability ------------------------

def test_model_registry_roundtrip(tmp_path):
    async def go():
        bus = InProcessBus()
        from ai_crypto_trader_amd.services.registry import (
            ModelRegistryService,
        )
        reg = ModelRegistryService(bus, AppConfig(),
                                   store_path=str(tmp_path / "r.json"))
        a = await reg.register("lstm-btc", "lstm")
        b = await reg.register("ga-strat", "strategy")
        await reg.update_performance(a, {"sharpe": 1.5})
        await reg.update_performance(b, {"sharpe": 0.5})
        best = reg.best_model(metric="sharpe")
        assert best["id"] == a
        cmp_ = reg.compare([a, b])
        assert cmp_[0]["id"] == a
        await reg.set_status(a, "retired")
        assert reg.best_model(metric="sharpe")["id"] == b
        # persistence
        reg2 = ModelRegistryService(bus, AppConfig(),
                                    store_path=str(tmp_path / "r.json"))
        assert a in reg2.models

    asyncio.run(go())


def test_explanation_formatting():
    sig = {"symbol": "X", "decision": "BUY", "confidence": 0.8,
           "explanation": {"momentum": 0.5, "trend": -0.1},
           "factor_weights": {"momentum": 0.6, "trend": 0.4}}
    ex = AIExplainabilityService.format_explanation(sig)
    assert ex["factors"][0]["factor"] == "momentum"
    assert ex["factors"][0]["contribution"] == pytest.approx(0.3)


def test_feature_importance_integrator():
    fi = FeatureImportanceIntegrator()
    fi.update({"importances": {
        "rsi": {"permutation": 0.6, "impurity": 0.5},
        "macd": {"permutation": 0.2, "impurity": 0.3},
        "price_change_5m": {"permutation": 0.2, "impurity": 0.2},
    }, "at": time.time()})
    assert fi.weights["rsi"] == pytest.approx(0.6)
    p = fi.predict_outcome({"rsi": 40.0, "macd": 1.0})
    assert 0 <= p <= 1
    w = fi.adjust_factor_weights({"oscillators": 0.25, "momentum": 0.25,
                                  "trend": 0.25, "social_sentiment": 0.25})
    assert abs(sum(w.values()) - 1.0) < 1e-6


# -------------------------- strategy selection -----------------------------

def test_strategy_selection_scoring():
    bus = InProcessBus()
    svc = StrategySelectionService(bus, AppConfig())
    best_bull, _, scores = svc.select_optimal("bull", 0.8, 0.2, hour=14)
    assert best_bull == "momentum"
    best_vol, _, _ = svc.select_optimal("volatile", 0.5, 0.9, hour=14)
    assert best_vol in ("conservative", "dca_strategy")
    # hysteresis: small improvements don't switch
    svc.current = best_bull
    assert not svc.should_switch(best_bull, scores)
    low = {k: v * 0.99 for k, v in scores.items()}
    low[best_bull] = scores[best_bull]
    assert not svc.should_switch(max(low, key=low.get), low)


# ------------------------------ patterns -----------------------------------

def test_pattern_model_classifies_synthetic():
    from ai_crypto_trader_amd.models.patterns import (
        PATTERNS, PatternRecognitionModel, generate_pattern,
    )

    m = PatternRecognitionModel("cpu", seed=0)
    acc = m.train(epochs=6, n_per_class=48, seed=1)
    assert acc > 0.8, acc
    rng = np.random.default_rng(99)
    hits = 0
    trials = 20
    for i in range(trials):
        name = PATTERNS[i % (len(PATTERNS) - 1)]
        det = m.detect(generate_pattern(name, rng) * 100 + 50)
        hits += det["pattern"] == name
    assert hits / trials > 0.5
    det = m.detect(generate_pattern("double_top", rng) * 100 + 50)
    assert det["signal"] in ("bearish", "neutral", "bullish")


def test_generic_ga_optimizes():
    from ai_crypto_trader_amd.services.genetic_algorithm import (
        GeneticAlgorithm,
    )

    ranges = {"x": (-5.0, 5.0), "n": (1, 10, "int")}

    def fitness(ind):
        return -(ind["x"] - 2.0) ** 2 - (ind["n"] - 7) ** 2

    ga = GeneticAlgorithm(ranges, fitness, population_size=48,
                          generations=15, seed=3)
    best, fit = ga.run()
    assert abs(best["x"] - 2.0) < 0.5
    assert best["n"] == 7
    assert isinstance(best["n"], int)
    assert ga.diversity() >= 0
    assert len(ga.history) == 15

    # batched fitness path
    def fitness_batch(pop):
        import numpy as np
        return np.asarray([-(p["x"] - 1.0) ** 2 for p in pop])

    fitness_batch.batch = True
    ga2 = GeneticAlgorithm({"x": (-5.0, 5.0)}, fitness_batch,
                           population_size=32, generations=10, seed=1)
    best2, _ = ga2.run()
    assert abs(best2["x"] - 1.0) < 0.5


def test_serving_api():
    """serve.py ASGI surface: analyze/scan/backtest/predict on CPU."""
    import asyncio as _a

    import httpx

    from serve import build_server
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )

    async def go():
        app, nn = build_server("models_store_test_nonexistent", "cpu")
        candles = candles_chl_v(generate_ohlcv(400, 1, seed=9))[0]
        transport = httpx.ASGITransport(app=app)
        async with httpx.AsyncClient(transport=transport,
                                     base_url="http://t") as c:
            r = await c.get("/healthz")
            assert r.json()["ok"]
            r = await c.post("/analyze", json={
                "symbol": "X", "current_price": 1.0, "avg_volume": 1.0,
                "rsi": 25.0, "price_change_5m": 0.5})
            assert r.json()["decision"] in ("BUY", "SELL", "HOLD")
            r = await c.post("/scan", json={
                "AUSDC": candles.tolist(), "BUSDC": candles.tolist()})
            assert len(r.json()) == 2
            r = await c.post("/backtest", json={
                "candles": candles.tolist(),
                "params": {"entry_votes": 1}})
            assert "sharpe" in r.json()
            r = await c.post("/predict", json={
                "symbol": "AUSDC", "candles": candles.tolist()})
            out = r.json()
            assert "predicted_price" in out or "error" in out

    _a.run(go())


def test_grid_live_orders():
    """Live grid mode: resting LIMIT orders on the exchange, fills
    reconciled on tick."""
    async def go():
        from ai_crypto_trader_amd.services.grid_dca import (
            GridTradingStrategy,
        )
        ex = FakeExchange(initial_balance=100_000.0)
        ex.prices["BTCUSDC"] = 1.0
        # seed base-asset inventory so SELL limits can rest
        ex.balances["BTC"] = 100.0
        g = GridTradingStrategy(InProcessBus(), ex, "BTCUSDC",
                                AppConfig(), live=True, order_qty=1.0)
        g.build_grid(1.0)
        assert len(g._orders) >= 8          # resting LIMIT orders
        buy_prices = [lv["price"] for lv in g.levels
                      if lv["side"] == "BUY"]
        # price drops through the highest buy level -> exchange fills it
        ex.set_price("BTCUSDC", max(buy_prices) - 1e-6)
        fills = g.on_price(max(buy_prices) - 1e-6)
        assert any(f["side"] == "BUY" for f in fills)
        # price spikes through a sell level
        sell_prices = [lv["price"] for lv in g.levels
                       if lv["side"] == "SELL"]
        ex.set_price("BTCUSDC", min(sell_prices) + 1e-6)
        fills2 = g.on_price(min(sell_prices) + 1e-6)
        assert any(f["side"] == "SELL" for f in fills2)
        assert g.pnl > 0

    asyncio.run(go())


def test_strategy_evolution_service_cpu():
    """evolve_once on CPU: GA path runs, hot-swaps params, publishes the
    update + registry event; hybrid method selection prefers PPO only on
    GPU devices."""
    from ai_crypto_trader_amd.bus.schema import Channels, Keys
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.strategy_evolution import (
        StrategyEvolutionService,
    )

    candles = candles_chl_v(generate_ohlcv(1500, 2, seed=9))
    cfg = AppConfig()
    cfg.evolution.population_size = 16
    cfg.evolution.generations = 2

    async def go():
        bus = InProcessBus()
        svc = StrategyEvolutionService(bus, cfg, candles=candles,
                                       device="cpu")
        sub = bus.subscribe(Channels.STRATEGY_EVOLUTION_UPDATES)
        perf = await svc.evolve_once()
        assert perf["method"] in ("ga", "rl")
        assert perf["seconds"] > 0
        # hot swap happened: key set + channel published + version logged
        params = await bus.get_json(Keys.STRATEGY_PARAMS)
        assert params is not None and "stop_loss_pct" in params
        ch, msg = await asyncio.wait_for(sub.get(), timeout=2)
        assert msg["strategy_id"].startswith("evolved-")
        assert svc.model_versions and svc.evolutions == 1
        # live perf evaluation (the strategy_performance key content)
        d = svc.evaluate_params(svc.current_params)
        assert "win_rate" in d and "profit_factor" in d

    asyncio.run(go())

    # hybrid method selection: ppo only on cuda
    bus = InProcessBus()
    svc = StrategyEvolutionService(bus, cfg, candles=candles, device="cpu")
    svc.evolutions = 2
    assert svc.select_method("ranging", 0.2) == "rl"
    svc.device = "cuda:0"
    assert svc.select_method("ranging", 0.2) == "ppo"
    assert svc.select_method("volatile", 0.9) == "ga"


@pytest.mark.parametrize("cmd", [
    ["run_trader.py", "--minutes", "0.25", "--candles", "3000",
     "--symbols", "BTCUSDC,ETHUSDC", "--status-interval", "2"],
    ["auto_trader.py", "--minutes", "0.15", "--candles", "3000"],
    ["run_ai_model_services.py", "--model-registry", "--explainability",
     "--seconds", "5"],
])
def test_entrypoint_smoke(cmd):
    """The reference's three long-running entrypoints start, run a short
    window over the synthetic feed, and exit 0 (SURVEY §2.1 parity)."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable] + cmd, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])


def test_service_runner_cli():
    """Per-service runner (one-container-per-service topology): every
    registered service constructs; one runs end-to-end via the CLI."""
    import subprocess
    import sys

    from ai_crypto_trader_amd.services.runner import SERVICES

    assert len(SERVICES) == 21
    r = subprocess.run(
        [sys.executable, "-m", "ai_crypto_trader_amd.services.runner",
         "--service", "ai_analyzer", "--minutes", "0.02"],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]


def test_service_runner_builds_all():
    import argparse

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.runner import SERVICES, build_service

    args = argparse.Namespace(device="cpu", candles=600, speed=0.0, seed=0)
    cfg = AppConfig()
    cfg.trading.symbols = ["BTCUSDC", "ETHUSDC"]
    for name in SERVICES:
        svc = build_service(name, InProcessBus(), cfg, args)
        assert svc is not None, name


def test_dashboard_api():
    """Dashboard JSON API: every panel endpoint responds against a seeded
    bus (reference Dash callbacks -> data endpoints)."""
    import asyncio as _a

    import httpx

    from ai_crypto_trader_amd.bus.schema import Keys
    from dashboard import DataStore, build_app

    async def go():
        bus = InProcessBus()
        store = DataStore(bus)
        app = build_app(bus, store)
        await store.start()
        await bus.set(Keys.HOLDINGS, {"total_value": 1234.5})
        await bus.set(Keys.PORTFOLIO_RISK, {
            "portfolio_var_pct": 2.0, "avg_correlation": 0.4,
            "correlation_matrix": [[1.0, 0.4], [0.4, 1.0]],
            "symbols": ["BTCUSDC", "ETHUSDC"]})
        await bus.hset(Keys.SOCIAL_METRICS, "BTCUSDC",
                       {"sentiment": 0.7})
        transport = httpx.ASGITransport(app=app)
        async with httpx.AsyncClient(transport=transport,
                                     base_url="http://d") as c:
            for path in ("/api/portfolio", "/api/risk", "/api/signals",
                         "/api/trades", "/api/regime", "/api/monte_carlo",
                         "/api/predictions", "/api/patterns",
                         "/api/explanations", "/api/evolution",
                         "/api/social", "/api/correlation", "/api/models",
                         "/"):
                r = await c.get(path)
                assert r.status_code == 200, path
            r = await c.get("/api/correlation")
            assert r.json()["avg_correlation"] == 0.4
            r = await c.get("/api/social")
            assert r.json()["metrics"]["BTCUSDC"]["sentiment"] == 0.7

    asyncio.run(go())


def test_social_accuracy_and_adaptive_weights():
    """Direction-accuracy/IC self-assessment + adaptive source weights
    (reference social_metrics_analyzer.py:457-750)."""
    rng = np.random.default_rng(4)
    an = SocialMetricsAnalyzer()
    # sentiment that genuinely leads price by construction
    price = 100.0
    for t in range(400):
        s = float(np.clip(0.5 + 0.3 * np.sin(t / 9.0)
                          + 0.05 * rng.standard_normal(), 0, 1))
        an.record("BTCUSDC", s, price, ts=float(t * 60))
        price *= float(np.exp(0.004 * (s - 0.5)
                              + 0.0005 * rng.standard_normal()))
    d = an.direction_accuracy("BTCUSDC")
    assert d["n"] > 100
    assert d["accuracy"] > 0.6 and d["ic"] > 0.2

    # adaptive weights shift toward the accurate source, never below floor
    w0 = dict(an.source_weights)
    w1 = an.update_source_weights(
        {"twitter": 0.8, "reddit": 0.45, "news": 0.5})
    assert w1["twitter"] > w0["twitter"]
    assert abs(sum(w1.values()) - 1.0) < 1e-9
    for _ in range(50):
        w1 = an.update_source_weights(
            {"twitter": 0.9, "reddit": 0.1, "news": 0.5})
    # floored pre-normalization, so the post-normalized weight sits just
    # under the floor — but never collapses to zero
    assert w1["reddit"] >= 0.04


def test_dca_rebalance():
    """Periodic rebalancing trims an over-grown position back to the
    target allocation (reference dca_strategy.py:864-1022)."""
    from ai_crypto_trader_amd.config import AppConfig as _AC
    from ai_crypto_trader_amd.services.grid_dca import DCAStrategy

    svc = DCAStrategy(InProcessBus(), FakeExchange(), "BTCUSDC", _AC(),
                      candles_per_period=10)
    svc.units = 10.0
    svc.invested = 100.0          # value will dwarf invested
    svc.counter = 10 * 30         # exactly a rebalance tick
    rec = svc.maybe_rebalance(price=100.0)
    assert rec is not None and rec["action"] == "rebalance_sell"
    value = svc.units * 100.0
    capital = value + svc.banked
    assert abs(value / capital - 0.6) < 1e-6
    # off-tick: no rebalance
    svc.counter += 1
    assert svc.maybe_rebalance(price=100.0) is None


def test_dca_schedules():
    """All three DCA schedules behave distinctly (reference :347-451):
    regime_based buys more often in bear markets; value_averaging buys
    the gap to a growing target value."""
    from ai_crypto_trader_amd.config import AppConfig as _AC
    from ai_crypto_trader_amd.services.grid_dca import DCAStrategy

    async def run_sched(schedule, regime, price_fn):
        cfg = _AC()
        cfg.dca.schedule = schedule
        svc = DCAStrategy(InProcessBus(), FakeExchange(), "BTCUSDC", cfg,
                          candles_per_period=10)
        for t in range(100):
            await svc.maybe_buy(price_fn(t), 0.5, regime)
        return svc

    async def go():
        fixed = await run_sched("fixed", "bear", lambda t: 100.0)
        bear = await run_sched("regime_based", "bear", lambda t: 100.0)
        bull = await run_sched("regime_based", "bull", lambda t: 100.0)
        assert len(bear.purchases) > len(fixed.purchases) \
            > len(bull.purchases)

        va = await run_sched("value_averaging", "ranging", lambda t: 100.0)
        # flat price: each buy tops value up to base*periods -> invested
        # grows ~linearly and matches target at each tick
        assert len(va.purchases) >= 9
        assert abs(va.units * 100.0
                   - va.config.dca.base_order_usd * 10) < 1.0

        # rising market: value averaging buys LESS than fixed (the market
        # does the growing)
        va_up = await run_sched("value_averaging", "ranging",
                                lambda t: 100.0 * (1 + 0.01 * t))
        fixed_up = await run_sched("fixed", "ranging",
                                   lambda t: 100.0 * (1 + 0.01 * t))
        assert va_up.invested < fixed_up.invested

    asyncio.run(go())


def test_llm_evolution_seam():
    """method='gpt': an injected llm_fn proposing params (as a dict OR as
    strategy code text) drives the evolution (reference :364-511)."""
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.strategy_evolution import (
        StrategyEvolutionService,
    )

    candles = candles_chl_v(generate_ohlcv(1200, 2, seed=2))
    cfg = AppConfig()
    cfg.evolution.method = "gpt"

    def llm_fn(params, perf):
        assert "sharpe" in perf
        return "const stopLoss = 0.07;\nrsi_period = 9\n"

    async def go():
        bus = InProcessBus()
        svc = StrategyEvolutionService(bus, cfg, candles=candles,
                                       device="cpu", llm_fn=llm_fn)
        out = await svc.evolve_once()
        assert out["method"] == "gpt" and out["llm"]
        from ai_crypto_trader_amd.backtesting.strategy import params_to_dict
        d = params_to_dict(svc.current_params)
        assert abs(d["stop_loss_pct"] - 0.07) < 1e-6
        assert d["rsi_period"] == 9.0

    asyncio.run(go())


def test_code_strategy_cycle_improves_and_registers(tmp_path):
    """>=2 improvement iterations over strategy CODE
    (generate -> static eval -> simulate via strategy_tester -> suggest
    -> apply-to-code -> re-evaluate), report emitted, result round-trips
    through the model registry (reference
    ai_strategy_evaluator.py:732-1359)."""
    import asyncio
    import json as _json

    import numpy as np

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.registry import ModelRegistryService
    from ai_crypto_trader_amd.services.strategy_evaluator import (
        CodeStrategyCycle,
    )

    candles = candles_chl_v(generate_ohlcv(6000, 1, seed=4))[0]
    cyc = CodeStrategyCycle(report_dir=str(tmp_path), seed=1)

    # deliberately weak initial spec so suggestions have room to act
    res = cyc.cycle(candles, spec={"rsi_oversold": 12.0,
                                   "take_profit_pct": 0.02},
                    rounds=3)
    assert res["iterations"] >= 3          # initial + >=2 improvements
    assert res["best_eval"]["n_trades"] >= 0
    assert "def decide" in res["best_code"]
    # the improvement trail shows applied suggestions
    assert len(res["trail"]) == res["iterations"]
    assert res["trail"][1]["applied"] != "initial proposal"

    rp = cyc.report(res, name="cycle-test")
    assert rp.exists()
    md = list(tmp_path.glob("cycle-test-*.md"))
    assert md and "evaluate-improve" in md[0].read_text()

    # registry round-trip
    async def roundtrip():
        bus = InProcessBus()
        reg = ModelRegistryService(
            bus, store_path=str(tmp_path / "registry.json"))
        await reg.register(
            "code-cycle-best", "strategy_code",
            params={"quality": res["final_quality"],
                    "code": res["best_code"]})
        stored = await bus.get_json(
            __import__("ai_crypto_trader_amd.bus.schema",
                       fromlist=["Keys"]).Keys.MODEL_REGISTRY)
        return stored

    stored = asyncio.run(roundtrip())
    s = _json.dumps(stored)
    assert "code-cycle-best" in s and "def decide" in s


def test_code_static_eval_rejects_bad_code():
    from ai_crypto_trader_amd.services.strategy_evaluator import (
        CodeStrategyCycle,
    )

    ok, issues = CodeStrategyCycle.static_eval("x = 1")
    assert not ok and any("decide" in i for i in issues)
    # no stop loss -> risk-management gate
    code = CodeStrategyCycle._default_proposal({"stop_loss_pct": 0.0})
    ok2, issues2 = CodeStrategyCycle.static_eval(code)
    assert not ok2 and any("stop loss" in i for i in issues2)


def test_rf_supervised_regime_mode():
    """the supervised RandomForest regime classifier
    (reference market_regime_detector.py:156) behind config
    regime.method='rf'."""
    import numpy as np

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.market_regime import (
        MarketRegimeService, RandomForestRegime,
    )

    rng = np.random.default_rng(3)
    # clearly-trending market -> rule labels mostly 'bull'
    closes = 100 * np.cumprod(1 + 0.002 + 0.002 * rng.standard_normal(600))
    cfg = AppConfig()
    cfg.regime.method = "rf"
    svc = MarketRegimeService(InProcessBus(), cfg)
    regime, conf = svc.detect(closes)
    assert regime in ("bull", "bear", "ranging", "volatile")
    assert 0.0 <= conf <= 1.0
    assert isinstance(svc.model, RandomForestRegime)
    # the trained forest exposes feature importances over the 6 features
    fi = svc.model.feature_importances()
    assert len(fi) == 6 and abs(fi.sum() - 1.0) < 1e-6
    # trending data should not be labeled bear
    assert regime != "bear"


def test_nn_integrated_gradients_attribution():
    """integrated-gradients attribution on the fused
    LSTM predictor (SHAP DeepExplainer stand-in,
    neural_network_service.py:957-1003), published in the
    feature_importance report shape."""
    import numpy as np

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.neural_network import (
        NeuralNetworkService,
    )

    cfg = AppConfig()
    cfg.neural_network.seq_len = 16
    cfg.neural_network.attribution = "integrated_gradients"
    svc = NeuralNetworkService(InProcessBus(), cfg)
    candles = candles_chl_v(generate_ohlcv(600, 1, seed=7))[0]
    svc.train("BTCUSDC", candles, epochs=1)
    rep = svc.importance_report("BTCUSDC", candles)
    assert rep is not None
    assert rep["method"] == "integrated_gradients"
    imp = rep["feature_importance"]
    assert set(imp) == set(svc.FEATURE_NAMES)
    assert abs(sum(imp.values()) - 1.0) < 1e-5
    assert all(v >= 0 for v in imp.values())
    assert len(rep["top_features"]) == 5 and rep["recommendations"]

    # both methods behind config produce valid, differing attributions
    cfg.neural_network.attribution = "grad_input"
    rep2 = svc.importance_report("BTCUSDC", candles)
    assert rep2["method"] == "grad_input"
    assert abs(sum(rep2["feature_importance"].values()) - 1.0) < 1e-5


def test_regime_transition_drives_strategy_switch_with_hysteresis():
    """a regime transition (bull -> bear) propagates
    regime service -> selection service -> strategy_switch publication +
    strategy_params hot-swap, and the selection hysteresis blocks
    marginal switches (reference market_regime_service.py:637-1113,
    strategy_selection_service.py:884-935)."""
    import asyncio

    import numpy as np

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.bus.schema import Channels, Keys
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.market_regime import (
        MarketRegimeService,
    )
    from ai_crypto_trader_amd.services.strategy_selection import (
        STRATEGY_PRESETS, StrategySelectionService,
    )

    cfg = AppConfig()
    cfg.regime.method = "rule"
    bus = InProcessBus()
    regime_svc = MarketRegimeService(bus, cfg)
    sel = StrategySelectionService(bus, cfg)

    rng = np.random.default_rng(0)

    def market(drift, n=400):
        return 100 * np.cumprod(
            1 + drift + 0.001 * rng.standard_normal(n))

    async def run():
        switches = []
        sub = bus.subscribe(Channels.STRATEGY_SWITCH)

        async def pump_regime(closes):
            regime, conf = regime_svc.detect(closes)
            vol = float(np.diff(np.log(closes[-100:])).std()
                        * np.sqrt(525_600))
            await bus.set(Keys.CURRENT_MARKET_REGIME,
                          {"regime": regime, "confidence": conf,
                           "volatility": min(vol, 2.0)})
            return regime

        # establish bull
        r1 = await pump_regime(market(+0.003))
        assert r1 == "bull"
        sel.running = True
        task = asyncio.create_task(sel.run())
        try:
            await asyncio.sleep(0.1)
            base_strategy = sel.current
            # transition to bear
            r2 = await pump_regime(market(-0.003))
            assert r2 == "bear"
            for _ in range(50):
                try:
                    chan, msg = await asyncio.wait_for(sub.get(), 0.2)
                    switches.append(msg)
                    break
                except asyncio.TimeoutError:
                    continue
        finally:
            sel.running = False
            task.cancel()
        return base_strategy, switches

    base_strategy, switches = asyncio.run(run())
    assert switches, "regime transition produced no strategy_switch"
    sw = switches[-1]
    assert sw["market_regime"] == "bear"
    assert sw["new_strategy_id"] != base_strategy
    assert sel.current == sw["new_strategy_id"]
    assert sel.current in STRATEGY_PRESETS

    # hysteresis: equal/marginal scores must NOT switch
    cur = sel.current
    scores = {s: 1.0 for s in STRATEGY_PRESETS}
    best = [s for s in STRATEGY_PRESETS if s != cur][0]
    scores[best] = 1.0 + sel.min_improvement * 0.5     # below threshold
    assert not sel.should_switch(best, scores)
    scores[best] = 1.0 + sel.min_improvement * 2.0     # above threshold
    assert sel.should_switch(best, scores)
    # staying on the same strategy never switches
    assert not sel.should_switch(cur, scores)


def test_pattern_model_types_cnn_lstm_hybrid():
    """All three reference pattern-classifier architectures (cnn, lstm,
    cnn_lstm — pattern_recognition.py:94-196) train and detect behind
    patterns.model_type."""
    import numpy as np

    from ai_crypto_trader_amd.models.patterns import (
        PATTERN_MODELS, PatternRecognitionModel, generate_pattern,
    )

    assert set(PATTERN_MODELS) == {"cnn", "lstm", "cnn_lstm"}
    rng = np.random.default_rng(0)
    probe = generate_pattern("double_top", rng)
    # recurrent types are slow starters from scratch: give them a
    # higher lr + more epochs; the bar is "clearly learning" (random
    # chance over 15 classes is 0.067)
    plans = {"cnn": (6, 2e-3, 0.6), "lstm": (25, 5e-3, 0.25),
             "cnn_lstm": (25, 5e-3, 0.6)}
    for mt in PATTERN_MODELS:
        epochs, lr, bar = plans[mt]
        m = PatternRecognitionModel(seed=0, model_type=mt)
        acc = m.train(epochs=epochs, n_per_class=24, lr=lr)
        assert acc > bar, (mt, acc)
        det = m.detect(probe * 100.0)
        assert det["pattern"] in __import__(
            "ai_crypto_trader_amd.models.patterns",
            fromlist=["PATTERNS"]).PATTERNS
        assert 0.0 <= det["confidence"] <= 1.0


def test_cross_exchange_arbitrage_detection():
    """Cross-exchange spread scan (reference
    arbitrage_detection_service.py:434-522): a fee-surviving spread
    between two venues is detected; a sub-fee spread is not."""
    from ai_crypto_trader_amd.services.arbitrage import (
        CrossExchangeDetector,
    )
    from ai_crypto_trader_amd.utils.exchange import FakeExchange

    a = FakeExchange()
    b = FakeExchange()
    a.set_price("BTCUSDC", 100.0)
    b.set_price("BTCUSDC", 101.0)      # 1% spread >> 2x0.1% fees
    det = CrossExchangeDetector({"alpha": a, "beta": b},
                                min_profit_pct=0.05)
    opps = det.scan(["BTCUSDC"])
    assert opps and opps[0]["buy_on"] == "alpha" \
        and opps[0]["sell_on"] == "beta"
    assert opps[0]["net_profit_pct"] > 0.5

    b.set_price("BTCUSDC", 100.05)     # 0.05% spread < fees
    assert det.scan(["BTCUSDC"]) == []


def test_runner_tcp_health_endpoint():
    """The per-service TCP health endpoint (reference
    health_check_server + nc -z compose probes) responds with the
    service's health JSON."""
    import asyncio
    import json as _json

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.registry import ModelRegistryService
    from ai_crypto_trader_amd.services.runner import serve_health

    async def run():
        svc = ModelRegistryService(InProcessBus(), AppConfig())
        await svc.start()
        server = await serve_health(svc, 18943)
        try:
            reader, writer = await asyncio.open_connection(
                "127.0.0.1", 18943)
            line = await asyncio.wait_for(reader.readline(), 5)
            writer.close()
            return _json.loads(line)
        finally:
            server.close()
            await svc.stop()

    h = asyncio.run(run())
    assert h["service"] == "model_registry" and h["healthy"]


def test_regime_bucketed_performance_drives_selection():
    """The per-regime strategy performance table (reference
    market_regime_service.py:637-1113) blends into regime scoring:
    measured losses in a regime demote the statically-favored strategy."""
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.strategy_selection import (
        StrategySelectionService,
    )

    sel = StrategySelectionService(InProcessBus(), AppConfig())
    base = sel.score_regime("momentum", "bull")
    assert base == 1.0                     # static fit favors momentum
    # momentum keeps losing in bull markets
    for _ in range(10):
        sel.record_trade("momentum", "bull", -2.0)
    demoted = sel.score_regime("momentum", "bull")
    assert demoted < base - 0.2
    # and consistent wins promote a statically-weak strategy
    for _ in range(10):
        sel.record_trade("mean_reversion", "bull", +2.0)
    promoted = sel.score_regime("mean_reversion", "bull")
    assert promoted > sel.score_regime("conservative", "bull")
    # other regimes unaffected
    assert sel.score_regime("momentum", "bear") == \
        __import__("ai_crypto_trader_amd.services.strategy_selection",
                   fromlist=["REGIME_FIT"]).REGIME_FIT["bear"]["momentum"]
    # evolution performance reports feed score_history
    sel.record_performance("momentum", {"sharpe": 2.0})
    assert sel.score_history("momentum") == 1.0


def test_serving_endpoints_cpu_smoke(tmp_path):
    """serve.py's ASGI app responds on CPU: health, analyze, and a
    backtest request (the GPU latency profile is
    profiles/serve_latency.json)."""
    import pytest as _pytest
    _pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from serve import build_server

    app, _nn = build_server(str(tmp_path), device="cpu")
    with TestClient(app) as c:
        h = c.get("/healthz").json()
        assert h["ok"] and h["device"] == "cpu"
        r = c.post("/analyze", json={
            "symbol": "BTCUSDC", "current_price": 100.0, "rsi": 25.0,
            "stoch_k": 15.0, "williams_r": -85.0, "macd": 0.5,
            "trend": "uptrend", "trend_strength": 40.0,
            "price_change_1m": 0.4, "price_change_5m": 1.0,
            "price_change_15m": 2.0, "bb_position": 0.1,
        })
        assert r.status_code == 200
        out = r.json()
        assert out["decision"] in ("BUY", "SELL", "HOLD")
        assert 0 <= out["confidence"] <= 1


def test_strategy_version_similarity_dedup():
    """Near-duplicate evolved parameter sets reuse the existing version
    id (reference model-version similarity dedup,
    strategy_evolution_service.py:1295-1400); distinct sets register
    new versions."""
    import asyncio

    import numpy as np

    from ai_crypto_trader_amd.backtesting.strategy import (
        DEFAULT_PARAMS, clip_params,
    )
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.strategy_evolution import (
        StrategyEvolutionService,
    )

    candles = candles_chl_v(generate_ohlcv(2000, 1, seed=0))
    svc = StrategyEvolutionService(InProcessBus(), AppConfig(),
                                   candles=candles)

    async def run():
        p1 = DEFAULT_PARAMS.copy()
        await svc.hot_swap(p1, {"sharpe": 1.0}, "bull")
        n1 = len(svc.model_versions)
        # tiny perturbation -> same version reused
        p2 = p1.copy()
        p2[1] += 0.01
        await svc.hot_swap(clip_params(p2[None])[0],
                           {"sharpe": 1.1}, "bull")
        assert len(svc.model_versions) == n1
        assert svc.model_versions[-1]["performance"]["sharpe"] == 1.1
        # clearly different params -> new version
        p3 = p1.copy()
        p3[0] = 60.0
        p3[13] = 0.19
        p3[12] = 0.06
        await svc.hot_swap(clip_params(p3[None])[0],
                           {"sharpe": 0.5}, "bear")
        assert len(svc.model_versions) == n1 + 1

    asyncio.run(run())


def test_nn_regime_specific_model_snapshots():
    """Regime-tagged model snapshots (reference
    neural_network_service.py:1445-1473): predict() prefers the model
    trained under the matching regime; unknown regimes fall back to the
    live model."""
    import numpy as np

    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    from ai_crypto_trader_amd.services.neural_network import (
        NeuralNetworkService,
    )

    cfg = AppConfig()
    cfg.neural_network.seq_len = 16
    svc = NeuralNetworkService(InProcessBus(), cfg)
    candles = candles_chl_v(generate_ohlcv(500, 1, seed=1))[0]
    svc.train("BTCUSDC", candles, epochs=1)
    key = svc.snapshot_for_regime("BTCUSDC", "bull")
    assert key == ("BTCUSDC", "bull")
    # retrain changes the live model; the bull snapshot is frozen
    svc.train("BTCUSDC", candles, epochs=1)
    m_live, _ = svc.model_for("BTCUSDC")
    m_bull, _ = svc.model_for("BTCUSDC", "bull")
    assert m_bull is not m_live
    p_bull = svc.predict("BTCUSDC", candles, regime="bull")
    p_live = svc.predict("BTCUSDC", candles)
    assert p_bull is not None and p_live is not None
    # unknown regime -> live model path
    p_unknown = svc.predict("BTCUSDC", candles, regime="sideways")
    assert np.isclose(p_unknown["predicted_change_pct"],
                      p_live["predicted_change_pct"])
