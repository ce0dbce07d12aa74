"""Shared inputs and assertions of test_ledger_cpu.py / test_gpu_ledger.py
(a helper module, no tests of its own)."""

import numpy as np

from ai_crypto_trader_amd.backtesting.ledger import (
    FIELDS, FLOAT_FIELDS, INT_FIELDS,
)

T_SHORT = 700        # 2 tiles of 256 + 188: the history ends inside a tile
NSYM = 3             # not a multiple of 8: the non-XCD-affine block map
N_EAGER = 40
NEVER = N_EAGER      # index of the strategy that can never enter
CAP = 128            # holds every lane of short_inputs()
SMALL_CAP = 16       # overflows most of its lanes and not all


def market(T, nsym, seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, nsym, seed=seed, sigma=2.0))


def eager_population(P, seed):
    """Random strategies with entry/exit votes forced to 1/2 (as
    test_gpu_backtest_bbtable._windows_population does), so they trade
    often."""
    from ai_crypto_trader_amd.backtesting.strategy import random_population
    pop = random_population(P, seed=seed)
    pop[:, 10] = 1.0 + (np.arange(P) % 2)
    pop[:, 11] = 1.0 + ((np.arange(P) // 2) % 2)
    return pop


def short_inputs():
    """T=700 x 3 symbols x (40 eager strategies + one that never enters:
    seven entry votes of six)."""
    pop = eager_population(N_EAGER + 1, seed=17)
    pop[NEVER, 10] = 7.0
    return market(T_SHORT, NSYM, seed=31), pop


def assert_ledgers_equal(got, ref):
    """Every field of every slot, n_records, the equity samples and the
    metrics: bit for bit (the NaN-free arrays make array_equal exact)."""
    np.testing.assert_array_equal(got.n_records, ref.n_records)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        np.testing.assert_array_equal(a, b, err_msg=f)
    assert got.equity_stride == ref.equity_stride
    np.testing.assert_array_equal(got.equity, ref.equity)
    np.testing.assert_array_equal(got.metrics, ref.metrics)


def assert_filler(led):
    """Slots at or above min(n_records, max_trades): -1 / 0."""
    kept = np.minimum(led.n_records, led.max_trades)
    unused = np.arange(led.max_trades)[None, None, :] >= kept[..., None]
    for f in INT_FIELDS:
        assert (getattr(led, f)[unused] == -1).all(), f
    for f in FLOAT_FIELDS:
        assert (getattr(led, f)[unused] == 0).all(), f


def assert_prefix(small, full):
    """A smaller capacity keeps the first records and the whole count."""
    np.testing.assert_array_equal(small.n_records, full.n_records)
    assert (small.n_records > small.max_trades).any()      # overflow ...
    assert (small.n_records <= small.max_trades).any()     # ... not all
    for f in FIELDS:
        np.testing.assert_array_equal(
            getattr(small, f), getattr(full, f)[..., :small.max_trades],
            err_msg=f)
    assert_filler(small)
    np.testing.assert_array_equal(small.metrics, full.metrics)


def assert_sampled(led, curve, T):
    """led.equity is the stride-1 `curve` at the defined candles, and its
    last sample the final equity."""
    stride = led.equity_stride
    idx = [min((k + 1) * stride - 1, T - 1) for k in range(-(-T // stride))]
    assert led.equity.shape[-1] == len(idx)
    np.testing.assert_array_equal(led.equity, curve[..., idx])
    np.testing.assert_array_equal(led.equity[..., -1], led.metrics[..., 0])
