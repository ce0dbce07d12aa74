"""GPU tests for the grid and DCA strategy families (run on MI355X:
pytest -m gpu). The HIP kernels (ops/hip/backtest_grid.hip,
backtest_dca.hip, ga.hip ga_evolve_generic) are validated against the
numpy twins on a deliberately volatile market, where every grid lane
trades and breaks out and most DCA lanes take profit."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from ai_crypto_trader_amd.backtesting.families import FAMILIES  # noqa: E402

SEEDS = {"grid": 11, "dca": 11}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def market():
    # T=4099: 16 full 256-candle tiles + a ragged 3-candle one
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(4099, 3, seed=7, sigma=3.0))


@pytest.fixture(scope="module")
def cpu_ref(market):
    """CPU-twin metrics at P=70 (ragged last block), computed once."""
    out = {}
    for name, fam in FAMILIES.items():
        pop = fam.random_population(70, SEEDS[name])
        out[name] = (pop, fam.run_cpu(market, pop))
    return out


def run_gpu(fam, dev, candles, pop):
    got = fam.run_gpu(torch.from_numpy(np.ascontiguousarray(candles)).to(dev),
                      torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    return got.cpu().numpy()


def assert_matches(got, ref):
    # integer-valued metrics must agree exactly (same decisions per
    # candle); tolerances of test_gpu_kernels.test_backtest_gpu_matches_cpu
    np.testing.assert_array_equal(got[..., 1], ref[..., 1])   # n_trades
    np.testing.assert_array_equal(got[..., 2], ref[..., 2])   # wins
    np.testing.assert_allclose(got[..., 0], ref[..., 0], rtol=2e-5)
    np.testing.assert_allclose(got[..., 5], ref[..., 5], rtol=1e-3,
                               atol=1e-6)
    np.testing.assert_allclose(got[..., 9], ref[..., 9], rtol=1e-3,
                               atol=1e-3)


def test_grid_gpu_matches_cpu(dev, market, cpu_ref):
    pop, ref = cpu_ref["grid"]
    # non-vacuity, on the twin alone
    assert (ref[..., 1] > 0).all()
    assert (ref[..., 2] < ref[..., 1]).mean() >= 0.5
    assert_matches(run_gpu(FAMILIES["grid"], dev, market, pop), ref)


def test_dca_gpu_matches_cpu(dev, market, cpu_ref):
    pop, ref = cpu_ref["dca"]
    assert (ref[..., 1] > 0).mean() >= 0.5
    assert_matches(run_gpu(FAMILIES["dca"], dev, market, pop), ref)


@pytest.mark.parametrize("name", ["grid", "dca"])
@pytest.mark.parametrize("P", [37, 256])
def test_family_gpu_pop_sizes_one_symbol(dev, market, name, P):
    """Less than one block, and exactly one, on a single symbol."""
    fam = FAMILIES[name]
    pop = fam.random_population(P, seed=5)
    one = market[:1, :1024]
    assert_matches(run_gpu(fam, dev, one, pop), fam.run_cpu(one, pop))


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_family_gpu_short_history(dev, market, name):
    """T=300: one full tile plus a ragged one."""
    fam = FAMILIES[name]
    pop = fam.random_population(70, seed=6)
    short = market[:, :300]
    assert_matches(run_gpu(fam, dev, short, pop), fam.run_cpu(short, pop))


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_family_gpu_segment_reshape(dev, market, name):
    """GAEngine's segment reshape: (nsym*4, T/4, 4) candles on the GPU
    equal the twin on the same reshape."""
    fam = FAMILIES[name]
    pop = fam.random_population(40, seed=8)
    nsym = market.shape[0]
    seg = np.ascontiguousarray(market[:, :4096]).reshape(nsym * 4, 1024, 4)
    assert_matches(run_gpu(fam, dev, seg, pop), fam.run_cpu(seg, pop))


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_ga_evolve_family_gpu_invariants(dev, name):
    from ai_crypto_trader_amd.ops.ga import ga_evolve_family_gpu

    fam = FAMILIES[name]
    P, elite_k = 300, 8
    pop = fam.random_population(P, seed=9)
    fit = np.random.default_rng(1).standard_normal(P).astype(np.float32)
    pop_t = torch.from_numpy(pop).to(dev)
    fit_t = torch.from_numpy(fit).to(dev)
    bounds_t = torch.from_numpy(np.ascontiguousarray(fam.bounds)).to(dev)

    def evolve(gen):
        out = ga_evolve_family_gpu(pop_t, fit_t, bounds_t, elite_k=elite_k,
                                   seed=3, gen=gen)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    child = evolve(4)
    assert child.shape == pop.shape
    order = np.argsort(-fit)
    np.testing.assert_array_equal(child[:elite_k], pop[order[:elite_k]])
    lo, hi, is_int = fam.bounds.T
    assert (child >= lo).all() and (child <= hi).all()
    ints = child[:, is_int > 0]
    assert (ints == np.rint(ints)).all()
    np.testing.assert_array_equal(child, evolve(4))      # same (seed, gen)
    assert not np.array_equal(child, evolve(5))
    assert not np.array_equal(child[elite_k:], pop[elite_k:])


@pytest.mark.parametrize("name", ["grid", "dca"])
def test_ga_engine_family_gpu(name):
    from ai_crypto_trader_amd.backtesting.ga_engine import GAEngine
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )

    fam = FAMILIES[name]
    candles = candles_chl_v(generate_ohlcv(8192, 2, seed=3, sigma=3.0))
    eng = GAEngine(candles, pop_per_rank=256, device="cuda:0", seed=2,
                   segments="auto", family=name)
    assert eng.segments == 2
    for _ in range(2):
        eng.step()
        torch.cuda.synchronize()
        assert torch.isfinite(eng.last_fitness_global).all()
    assert eng.last_metrics.shape == (256, 4, 10)
    pop = eng.pop_t.cpu().numpy()
    lo, hi, _ = fam.bounds.T
    assert pop.shape == (256, fam.nparam)
    assert (pop >= lo).all() and (pop <= hi).all()


def test_backtest_engine_grid_gpu_matches_cpu_engine(tmp_path):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine

    d = str(tmp_path / "d")
    cpu = BacktestEngine(d, device="cpu").run_backtest(
        "BTCUSDC", "grid", n_candles=3000)
    gpu = BacktestEngine(d, device="cuda").run_backtest(
        "BTCUSDC", "grid", n_candles=3000)
    assert gpu["engine"] == "cuda" and gpu["strategy"] == "grid"
    assert gpu["n_trades"] == cpu["n_trades"]
    assert gpu["final_equity"] == pytest.approx(cpu["final_equity"],
                                                rel=2e-5)
