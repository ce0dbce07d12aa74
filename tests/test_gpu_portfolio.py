"""bt_portfolio_kernel (ops/hip/backtest_portfolio.hip) against its numpy
twin, bit for bit: alone on random flag planes that make symbols contend
for slots and cash, end to end behind bt_flags, its argument checks, and
the flat-strategy skip. portfolio_cases.py has the inputs;
test_portfolio_cpu.py checks the twin itself."""

import numpy as np
import pytest

import portfolio_cases as pc
import tp_refs as tr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

bits = pc.bits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from ai_crypto_trader_amd.ops import require_hip_ops
    return require_hip_ops()


class Launch:
    """One bt_portfolio launch over given planes; every output starts as
    NaN / a sentinel, so a value the kernel did not write shows."""

    SENTINEL = -12345

    def __init__(self, dev, candles, pop, ef, xf, stride):
        self.dev = dev
        self.nsym, self.T, _ = candles.shape
        self.P = pop.shape[0]
        self.stride = stride
        self.n_samples = -(-self.T // stride) if stride else 0
        self.c_t = torch.from_numpy(np.array(candles)).to(dev)
        self.p_t = torch.from_numpy(np.array(pop)).to(dev)
        self.e_t = torch.from_numpy(tr.pack_flags(ef)).to(dev)
        self.x_t = torch.from_numpy(tr.pack_flags(xf)).to(dev)
        nan = float("nan")
        self.metrics = torch.full((self.P, 10), nan, device=dev)
        self.per_symbol = torch.full((self.P, self.nsym, 4), nan, device=dev)
        self.refused = torch.full((self.P, 2), self.SENTINEL,
                                  dtype=torch.int32, device=dev)
        self.equity = torch.full((self.P, max(self.n_samples, 1)), nan,
                                 device=dev)

    def run(self, ops, max_positions, initial_equity, **over):
        a = dict(nsym=self.nsym, T=self.T, P=self.P,
                 max_positions=max_positions, stride=self.stride,
                 n_samples=self.n_samples)
        a.update(over)
        ops.bt_portfolio(
            self.c_t.data_ptr(), self.p_t.data_ptr(), self.e_t.data_ptr(),
            self.x_t.data_ptr(), self.metrics.data_ptr(),
            self.per_symbol.data_ptr(), self.refused.data_ptr(),
            self.equity.data_ptr() if self.stride else 0, a["nsym"], a["T"],
            a["P"], a["max_positions"], float(initial_equity), a["stride"],
            a["n_samples"], torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize()
        return self

    def untouched(self):
        return (torch.isnan(self.metrics).all().item()
                and torch.isnan(self.per_symbol).all().item()
                and (self.refused == self.SENTINEL).all().item()
                and torch.isnan(self.equity).all().item())


def _assert_equal(got, ref, name):
    got, ref = bits(got), bits(ref)
    assert got.shape == ref.shape, name
    diff = np.argwhere(got != ref)
    assert len(diff) == 0, (
        f"{name}: {len(diff)} of {got.size} differ, first at "
        f"{diff[:5].tolist()}")


# ---------------------------------------------------------------------
# the kernel alone, on synthetic planes
# ---------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("shape", list(pc.CASES))
def test_kernel_equals_twin(ops, dev, shape, stride):
    nsym, P, T, max_positions = shape
    assert T % 64 != 0
    pc.assert_reaches_every_branch(shape)
    candles, pop, ef, xf, ref, trace = pc.case_with_twin(shape)
    run = Launch(dev, candles, pop, ef, xf, stride).run(
        ops, max_positions, pc.INITIAL_EQUITY)
    _assert_equal(run.metrics.cpu().numpy(), ref.metrics, "metrics")
    _assert_equal(run.per_symbol.cpu().numpy(), ref.per_symbol, "per_symbol")
    _assert_equal(run.refused.cpu().numpy(), ref.refused, "refused")
    _assert_equal(run.equity.cpu().numpy(),
                  pc.strided(trace["equity"], stride), "equity")


def test_no_equity_when_stride_is_zero(ops, dev):
    shape = (3, 65, 1000, 2)
    candles, pop, ef, xf, ref, _ = pc.case_with_twin(shape)
    run = Launch(dev, candles, pop, ef, xf, 0).run(
        ops, shape[3], pc.INITIAL_EQUITY)
    _assert_equal(run.metrics.cpu().numpy(), ref.metrics, "metrics")
    _assert_equal(run.refused.cpu().numpy(), ref.refused, "refused")
    assert torch.isnan(run.equity).all()


# ---------------------------------------------------------------------
# end to end: bt_flags + bt_portfolio against run_backtest_cpu + the twin
# ---------------------------------------------------------------------
def _market(T, nsym, seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, nsym, seed=seed))


def _end_to_end(dev, nsym, P, T, max_positions, stride, seed):
    from ai_crypto_trader_amd.backtesting.engine_portfolio_cpu import (
        run_portfolio_backtest_cpu,
    )
    from ai_crypto_trader_amd.backtesting.strategy import random_population
    from ai_crypto_trader_amd.ops.backtest import run_backtest_portfolio_gpu

    candles = _market(T, nsym, seed)
    pop = random_population(P, seed=seed + 1)
    ref = run_portfolio_backtest_cpu(
        candles, pop, max_positions=max_positions, equity_stride=stride)
    assert ref.metrics[:, 1].sum() > 0
    c_t = torch.from_numpy(candles).to(dev)
    p_t = torch.from_numpy(pop).to(dev)
    got = run_backtest_portfolio_gpu(
        c_t, p_t, max_positions=max_positions, equity_stride=stride)
    torch.cuda.synchronize()
    assert got.metrics.is_cuda and got.equity_stride == stride
    got = got.numpy()
    _assert_equal(got.metrics, ref.metrics, "metrics")
    _assert_equal(got.per_symbol, ref.per_symbol, "per_symbol")
    _assert_equal(got.refused, ref.refused, "refused")
    _assert_equal(got.equity, ref.equity, "equity")
    return c_t, p_t, got


def test_end_to_end_across_a_resnap_boundary(dev):
    """T = 17 000 > RESNAP: the Bollinger resnap candle fires at 16 384,
    inside the last tiles. (Still one flags shard: a shard body holds a
    whole RESNAP period, so two need T >= 2 * RESNAP.)"""
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP

    assert RESNAP < 17_000 < 2 * RESNAP
    _end_to_end(dev, 4, 8, 17_000, 2, 50, seed=61)


def test_end_to_end_single_symbol_is_the_continuous_backtest(dev):
    from ai_crypto_trader_amd.ops.backtest import run_backtest_continuous_gpu

    c_t, p_t, got = _end_to_end(dev, 1, 64, 1000, 1, 1, seed=71)
    cont = run_backtest_continuous_gpu(c_t, p_t)
    torch.cuda.synchronize()
    _assert_equal(got.metrics, cont[:, 0, :].cpu().numpy(), "continuous")
    assert (got.refused == 0).all()


# ---------------------------------------------------------------------
# argument checks: on the host, before anything is launched
# ---------------------------------------------------------------------
def test_bad_arguments_raise_before_launch(ops, dev):
    P, T = 3, 100
    candles = pc.walk_candles(65, T, seed=5)
    pop = pc.population(P, seed=6)
    flags = np.zeros((P, 65, T), bool)
    big = Launch(dev, candles, pop, flags, flags, 7)
    with pytest.raises(ValueError):
        big.run(ops, 1, 1.0)                         # nsym = 65
    small = Launch(dev, candles[:3], pop, flags[:, :3], flags[:, :3], 7)
    assert small.n_samples == 15
    bad = [
        dict(max_positions=0), dict(max_positions=4),
        dict(n_samples=14), dict(n_samples=16), dict(n_samples=0),
        dict(stride=0), dict(stride=-1),             # 15 samples, no stride
        dict(nsym=0), dict(T=0), dict(P=0),
    ]
    for over in bad:
        a = dict(max_positions=2)
        a.update(over)
        with pytest.raises(ValueError):
            small.run(ops, a.pop("max_positions"), 1.0, **a)
    torch.cuda.synchronize()
    assert big.untouched() and small.untouched()


# ---------------------------------------------------------------------
# the flat-strategy skip
# ---------------------------------------------------------------------
def test_flat_strategies_among_trading_neighbours(ops, dev):
    """Strategies 1 and 5 of 6 (two blocks of four) have no flag set: they
    end where they began, and their neighbours as the twin says."""
    from ai_crypto_trader_amd.backtesting.engine_portfolio_cpu import (
        run_portfolio_from_flags_cpu,
    )
    nsym, P, T, max_positions = 5, 6, 300, 2
    candles, pop, ef, xf = pc.make_case(nsym, P, T, seed=33)
    ef, xf = ef.copy(), xf.copy()
    for p in (1, 5):
        ef[p] = False
        xf[p] = False
    ref = run_portfolio_from_flags_cpu(
        candles, pop, ef, xf, max_positions=max_positions,
        initial_equity=pc.INITIAL_EQUITY, equity_stride=1)
    run = Launch(dev, candles, pop, ef, xf, 1).run(
        ops, max_positions, pc.INITIAL_EQUITY)
    metrics = run.metrics.cpu().numpy()
    equity = run.equity.cpu().numpy()
    for p in (1, 5):
        assert metrics[p, 0] == np.float32(pc.INITIAL_EQUITY)
        assert metrics[p, 9] == -1.0 and metrics[p, 1] == 0.0
        assert (equity[p] == np.float32(pc.INITIAL_EQUITY)).all()
    assert (ref.metrics[[0, 2, 3, 4], 1] > 0).all()
    _assert_equal(metrics, ref.metrics, "metrics")
    _assert_equal(run.per_symbol.cpu().numpy(), ref.per_symbol, "per_symbol")
    _assert_equal(run.refused.cpu().numpy(), ref.refused, "refused")
    _assert_equal(equity, ref.equity, "equity")
