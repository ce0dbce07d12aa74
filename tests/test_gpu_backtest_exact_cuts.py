"""The backtest kernels compute what they computed before two exact cuts:
the division-free guard on the drawdown divide (BtAccum::mark, shared by
the headline, ledger, grid and DCA kernels) and the stochastic / Williams
vote thresholds in the candle record (bt_shared_votes<true>).

P = 70, nsym = 3, T = 700 on three markets — one that slides for 520
candles, one with 40-candle stretches of high == low == close, and the
lane-loop market — at initial equities 1e-3, 1 and 1e4. Each case is held
bit for bit, all 10 metrics, against

  - run_backtest_continuous_gpu(nshards=1), whose flags kernel keeps the
    multiplies and whose trades kernel keeps the always-divide drawdown;
  - tests/golden/backtest_exact_cuts.npz, which the build of the commit
    BEFORE the cuts wrote on a GPU (tools/make_backtest_exact_cuts_golden.py;
    never regenerate it from the code under test).

The ledger, grid and DCA kernels run the falling market once each against
their CPU twins: the ledger bit for bit in every field, grid and DCA at
test_gpu_strategy_families' tolerances, and bit for bit against the golden.
"""

import functools
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tools import make_backtest_exact_cuts_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = (Path(__file__).resolve().parent / "golden"
          / "backtest_exact_cuts.npz")
METRICS = ("equity", "n_trades", "wins", "gross_p", "gross_l", "max_dd",
           "sum_ret", "sum_ret2", "sharpe", "fitness")
LEDGER_CAP = 256      # holds every lane of the falling market
CASES = [f"{m}_eq{gen.eq_name(eq)}" for m in gen.MARKETS
         for eq in gen.EQUITIES]


@functools.lru_cache(maxsize=None)
def _vote_cases():
    return gen.vote_cases()


@functools.lru_cache(maxsize=None)
def _family_cases():
    return gen.family_cases()


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    for k, metric in enumerate(METRICS):
        assert np.array_equal(got[..., k], want[..., k]), (
            f"{what}: {metric} differs in "
            f"{(got[..., k] != want[..., k]).sum()} of {want[..., k].size}")


def test_golden_file_is_complete():
    assert set(_golden()) == set(CASES) | {"grid_falling", "dca_falling"}
    for name in CASES:
        assert _golden()[name].shape == (gen.P_LANES, gen.NSYM, len(METRICS))


def test_markets_are_what_they_claim():
    fall = gen.falling_market()
    assert gen.FALL_TO - gen.FALL_FROM >= 500
    assert (fall[:, gen.FALL_TO, 0] < 0.5 * fall[:, gen.FALL_FROM, 0]).all()
    flat = gen.flat_market()
    t0 = gen.FLAT_AT + gen.FLAT_PERIOD
    stretch = flat[:, t0:t0 + gen.FLAT_LEN, :3]
    assert gen.FLAT_LEN == 40 and (stretch == stretch[:, :1, :1]).all()
    # drawdowns that matter: the golden's max_dd on the falling market
    assert np.median(_golden()["falling_eq1"][..., 5]) > 0.2


@pytest.mark.parametrize("name", CASES)
def test_vote_kernel(name):
    from ai_crypto_trader_amd.ops.backtest import (
        run_backtest_continuous_gpu, run_backtest_gpu,
    )
    dev = _dev()
    market, pop, eq = _vote_cases()[name]
    assert market.shape == (gen.NSYM, gen.T, 4) and len(pop) == gen.P_LANES
    m = torch.from_numpy(market).to(dev)
    p = torch.from_numpy(pop).to(dev)
    got = run_backtest_gpu(m, p, initial_equity=eq)
    cont = run_backtest_continuous_gpu(m, p, initial_equity=eq, nshards=1)
    torch.cuda.synchronize()
    got, cont = got.cpu().numpy(), cont.cpu().numpy()
    assert (got[..., 1].sum(axis=0) > 0).all()          # every symbol trades
    _assert_bits(got, cont, f"{name} vs continuous")
    _assert_bits(got, _golden()[name], f"{name} vs parent kernel")


def test_ledger_kernel_falling_market():
    from ledger_cases import assert_ledgers_equal
    from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
    from ai_crypto_trader_amd.ops.backtest import run_backtest_ledger_gpu
    dev = _dev()
    market, pop, eq = _vote_cases()["falling_eq1"]
    ref = run_backtest_cpu(market, pop, record_trades=True,
                           max_trades=LEDGER_CAP)
    assert ref.n_records.max() <= LEDGER_CAP
    assert np.median(ref.metrics[..., 5]) > 0.2
    led = run_backtest_ledger_gpu(torch.from_numpy(market).to(dev),
                                  torch.from_numpy(pop).to(dev),
                                  max_trades=LEDGER_CAP)
    torch.cuda.synchronize()
    got = led.numpy()
    assert_ledgers_equal(got, ref)
    _assert_bits(got.metrics, _golden()["falling_eq1"],
                 "ledger vs parent headline kernel")


@pytest.mark.parametrize("name", ["grid_falling", "dca_falling"])
def test_family_kernel_falling_market(name):
    dev = _dev()
    fam, market, pop = _family_cases()[name]
    ref = fam.run_cpu(market, pop)
    assert np.median(ref[..., 5]) > 0.02                # drawdowns happen
    got = fam.run_gpu(torch.from_numpy(market).to(dev),
                      torch.from_numpy(pop).to(dev))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    # the tolerances of test_gpu_strategy_families.assert_matches
    np.testing.assert_array_equal(got[..., 1], ref[..., 1])   # n_trades
    np.testing.assert_array_equal(got[..., 2], ref[..., 2])   # wins
    np.testing.assert_allclose(got[..., 0], ref[..., 0], rtol=2e-5)
    np.testing.assert_allclose(got[..., 5], ref[..., 5], rtol=1e-3,
                               atol=1e-6)
    np.testing.assert_allclose(got[..., 9], ref[..., 9], rtol=1e-3,
                               atol=1e-3)
    _assert_bits(got, _golden()[name], f"{name} vs parent kernel")
