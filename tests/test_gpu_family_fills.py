"""GPU tests for the fill ledgers of the grid and DCA families (run on
MI355X: pytest -m gpu). The HIP kernels (ops/hip/backtest_fills.hip) are
held to the numpy twins record for record and bit for bit, and to the
metrics-only kernels they share their state machines with, on the volatile
market where grid lanes fill hundreds of times and break out, and DCA lanes
take profit.

T = 700 is two full 256-candle tiles and a ragged 188, past the DCA
kernel's 128-candle halo; P = 41 is a partial block."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from ai_crypto_trader_amd.backtesting.families import FAMILIES  # noqa: E402
from ai_crypto_trader_amd.backtesting.fills import (  # noqa: E402
    FIELDS, FLOAT_FIELDS, INT_FIELDS,
)

P, SEED = 41, 11
NAMES = ["grid", "dca"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def market():
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(700, 3, seed=7, sigma=3.0))


@pytest.fixture(scope="module")
def ref(market):
    """Per family: the population and the twin's uncapped, stride-1 ledger,
    computed once and left unchanged."""
    out = {}
    for name in NAMES:
        fam = FAMILIES[name]
        pop = fam.random_population(P, SEED)
        n = fam.run_cpu_fills(market, pop, max_fills=1).n_records
        led = fam.run_cpu_fills(market, pop, max_fills=int(n.max()))
        if name == "dca" and not (led.kind == 6).any():
            # a lane whose schedule and dip cooldown coincide
            lane = fam.clip(np.array(
                [[15, 0.01, 0.01, 2.0, 15, 0.05, 0]], np.float32))
            pop = np.concatenate([pop, lane])
            n = fam.run_cpu_fills(market, pop, max_fills=1).n_records
            led = fam.run_cpu_fills(market, pop, max_fills=int(n.max()))
        out[name] = (pop, led)
    return out


def gpu_fills(name, dev, candles, pop, **kw):
    led = FAMILIES[name].run_gpu_fills(
        torch.from_numpy(np.ascontiguousarray(candles)).to(dev),
        torch.from_numpy(np.ascontiguousarray(pop)).to(dev), **kw)
    torch.cuda.synchronize()
    return led.numpy()


def differs(a, b):
    """Where two f32 (or i32) arrays are not the same numbers: equal
    values, or the same bits (a NaN against itself), pass."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return ~((a == b) | (a.view(np.int32) == b.view(np.int32)))


def assert_same_ledger(got, want, what=""):
    """Every field: integers equal, floats bit-equal."""
    np.testing.assert_array_equal(got.n_records, want.n_records,
                                  err_msg=what + "n_records")
    for f in INT_FIELDS:
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f),
                                      err_msg=what + f)
    for f in FLOAT_FIELDS + ("equity", "metrics"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape, what + f
        bad = differs(a, b)
        assert not bad.any(), (
            f"{what}{f}: {bad.sum()} of {bad.size} differ, first at "
            f"{np.argwhere(bad)[0].tolist()}: {a[bad][0]!r} vs {b[bad][0]!r}, "
            f"max rel {np.max(np.abs(a[bad] - b[bad]) / np.abs(b[bad]))!r}")
    assert got.equity_stride == want.equity_stride


def test_reference_is_not_vacuous(ref):
    """On the twin alone: the cases the GPU comparison is meant to cover
    are in the reference."""
    pop, led = ref["grid"]
    assert (pop[:, 0] == 16).any() and (pop[:, 2] > 0.5).any()
    assert set(np.unique(led.kind[led.kind >= 0])) == {0, 1, 2, 3}
    assert led.n_records.max() == led.max_fills > 1000
    pop, led = ref["dca"]
    assert {4, 5, 6, 7} <= set(np.unique(led.kind[led.kind >= 0]))
    assert led.n_records.max() == led.max_fills
    assert (led.slot.max(axis=2) > 0).any()        # a second cycle


@pytest.mark.parametrize("name", NAMES)
def test_fills_equal_the_twin(dev, market, ref, name):
    pop, want = ref[name]
    got = gpu_fills(name, dev, market, pop, max_fills=want.max_fills)
    assert_same_ledger(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_metrics_equal_the_metrics_kernel(dev, market, ref, name):
    """GPU against GPU: one state machine, two instantiations."""
    pop, want = ref[name]
    got = gpu_fills(name, dev, market, pop, max_fills=16, equity_stride=700)
    plain = FAMILIES[name].run_gpu(
        torch.from_numpy(market).to(dev), torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    plain = plain.cpu().numpy()
    assert not differs(got.metrics, plain).any()


@pytest.mark.parametrize("stride", [7, 256])
@pytest.mark.parametrize("name", NAMES)
def test_overflow_and_stride(dev, market, ref, name, stride):
    pop, full = ref[name]
    n = np.sort(full.n_records.ravel())
    cap = max(int(n[len(n) // 4]), 1)       # three lanes in four overflow
    over = full.n_records > cap
    assert 0.5 < over.mean() < 1.0
    got = gpu_fills(name, dev, market, pop, max_fills=cap,
                    equity_stride=stride)
    T = market.shape[1]
    ns = -(-T // stride)
    assert got.max_fills == cap and got.equity.shape[2] == ns
    np.testing.assert_array_equal(got.n_records, full.n_records)
    assert not differs(got.metrics, full.metrics).any()
    kept = np.minimum(full.n_records, cap)[..., None] > np.arange(cap)
    for f in FIELDS:
        a = getattr(got, f)
        assert not differs(a[kept], getattr(full, f)[..., :cap][
            kept]).any(), f
        assert (a[~kept] == (-1 if f in INT_FIELDS else 0)).all(), f
    at = np.minimum((np.arange(ns) + 1) * stride - 1, T - 1)
    assert not differs(got.equity, full.equity[..., at]).any()
    assert not differs(got.equity[..., -1], full.metrics[..., 0]).any()


@pytest.mark.parametrize("name", NAMES)
def test_launch_independence(dev, market, name):
    """P = 300: a full block plus 44 active lanes. One launch equals its
    rows [:256] and [256:] launched separately, on every field."""
    fam = FAMILIES[name]
    pop = fam.random_population(300, SEED + 1)
    kw = dict(max_fills=256, equity_stride=7)
    whole = gpu_fills(name, dev, market, pop, **kw)
    parts = [gpu_fills(name, dev, market, pop[a:b], **kw)
             for a, b in ((0, 256), (256, 300))]
    if name == "grid":
        assert (whole.n_records > 256).any()       # overflow in the launch
    for f in ("metrics", "n_records", "equity") + FIELDS:
        a = getattr(whole, f)
        b = np.concatenate([getattr(q, f) for q in parts])
        assert a.shape == b.shape and not differs(a, b).any(), f


@pytest.mark.parametrize("name", NAMES)
def test_engine_cuda_equals_cpu(tmp_path, name):
    from ai_crypto_trader_amd.backtesting.engine import BacktestEngine
    params = ({"half_levels": 6, "spacing_pct": 0.002} if name == "grid"
              else {"period": 30, "take_profit_pct": 0.004})
    stats = {}
    for device in ("cuda", "cpu"):
        eng = BacktestEngine(str(tmp_path / device), device=device)
        stats[device] = eng.run_backtest(
            "BTCUSDC", name, n_candles=3000, params=params,
            record_fills=True, record_equity=True, equity_stride=60)
    g, c = stats["cuda"], stats["cpu"]
    assert g["engine"] == "cuda" and c["engine"] == "cpu"
    assert len(c["fills"]) > 10 and c["n_trades"] > 0
    assert len(c["equity_curve"]) == 50
    for k in c:
        if k not in ("engine", "candles_per_sec"):
            assert g[k] == c[k], k
