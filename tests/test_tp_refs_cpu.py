"""The references of test_gpu_tp_phases.py, checked without a GPU:
tp_refs.trades_ref against the engine's own numpy twin of the trades phase,
the directed inputs against the census of what they must reach, and every
deliberate deviation against the metrics it must move."""

import numpy as np
import pytest

import tp_refs as tr
from ai_crypto_trader_amd.backtesting.engine_cpu import (
    run_trades_from_flags_cpu,
)


@pytest.fixture(scope="module")
def directed():
    case = tr.directed_case()
    candles, pop, ef, xf, eq = case
    metrics, census = tr.trades_ref(candles, pop, ef, xf, eq,
                                    watch=(255, 511))
    return case, metrics, census


def _twin(case):
    candles, pop, ef, xf, eq = case
    return run_trades_from_flags_cpu(candles, pop, ef, xf,
                                     initial_equity=eq)


def test_directed_shape():
    candles, pop, ef, xf, eq = tr.directed_case()
    assert candles.shape == (3, 700, 4) and candles.dtype == np.float32
    assert pop.shape[0] == 300 and pop.dtype == np.float32
    assert ef.shape == xf.shape == (300, 3, 700)
    assert eq == 250.0
    assert np.isfinite(candles).all() and (candles[..., :3] > 0).all()
    assert (candles[..., 1] >= candles[..., 0]).all()      # high >= close
    assert (candles[..., 2] <= candles[..., 0]).all()      # low <= close
    script = pop[:32]
    assert (script[:, 13] == 0.125).all() and (script[:, 14] == 0.25).all()
    assert (script[:, 16] == 0.0625).all()
    assert (script[3::4, 15] == 0).all()
    assert (np.delete(script[:, 15], np.s_[3::4]) == 0.0625).all()
    assert (pop[:, 12] == 1.0).any() and (script[:, 12] == 1.0).any()
    assert ef[32:48].all() and xf[32:48].all()             # all-ones lanes
    assert not ef[64:128].any()                            # a wave, never
    assert not ef[128:192, :, :321].any() and ef[128:192, :, 321:].any()
    acandles, apop, aef, axf, _ = tr.affine_case()
    assert acandles.shape == (8, 300, 4) and aef.shape == (40, 8, 300)


def test_trades_ref_equals_engine_twin_directed(directed):
    case, metrics, _ = directed
    np.testing.assert_array_equal(metrics, _twin(case))
    assert not np.isnan(metrics).any()


def test_trades_ref_equals_engine_twin_affine():
    case = tr.affine_case()
    metrics, census = tr.trades_ref(*case)
    np.testing.assert_array_equal(metrics, _twin(case))
    assert census["both_hit"] > 0 and census["exit_trailed"] > 0


def test_trades_ref_equals_engine_twin_on_engine_flags():
    from ledger_cases import eager_population, market

    candles = market(1200, 2, seed=77)
    pop = eager_population(24, seed=5)
    ef, xf, m_engine = tr.cpu_flags(candles, pop)
    assert ef.any() and xf.any()
    metrics, _ = tr.trades_ref(candles, pop, ef, xf)
    np.testing.assert_array_equal(
        metrics, run_trades_from_flags_cpu(candles, pop, ef, xf))
    np.testing.assert_array_equal(metrics, m_engine)
    assert m_engine[..., 1].sum() > 0


def test_directed_case_reaches_every_class(directed):
    _, _, c = directed
    for name in ("exit_stop", "exit_trailed", "exit_tp", "exit_signal",
                 "both_hit", "exit_on_entry_bit", "entry_ignored",
                 "exit_ignored", "trail_off_at_arm", "open_at_T"):
        assert c[name] > 0, name
    for t in (255, 511):
        assert c["in_pos_at"][t] > 0, t
        assert c["armed_at"][t] > 0, t


def test_directed_script_on_symbol_zero():
    """The scripted lanes alone, on the scripted symbol alone, reach the
    classes the script is there for (the random lanes might by accident)."""
    candles, pop, ef, xf, eq = tr.directed_case()
    _, c = tr.trades_ref(candles[:1], pop[:32], ef[:32, :1], xf[:32, :1],
                         eq, watch=(0, 255, 511, 699))
    for name in ("exit_stop", "exit_trailed", "exit_tp", "exit_signal",
                 "both_hit", "exit_on_entry_bit", "entry_ignored",
                 "exit_ignored", "trail_off_at_arm"):
        assert c[name] > 0, name
    assert c["in_pos_at"][0] == 32          # entry at t = 0
    assert c["open_at_T"] == 32             # entry at t = T - 1
    for t in (255, 511):
        assert c["in_pos_at"][t] == 32
        assert c["armed_at"][t] == 24       # the lanes that trail


def test_directed_case_skip_pattern(directed):
    _, _, c = directed
    skip, entered = c["skip"], c["wave_entered"]
    assert skip.shape == entered.shape == (3, 2, 4, 22)
    blk0 = skip[:, 0]                                      # (sym, wave, half)
    mixed = blk0.any(axis=1) & ~blk0.all(axis=1)           # (sym, half)
    assert mixed.any()
    assert blk0[:, 1].all()                 # the wave that never enters
    assert blk0[:, 2, :10].all() and not blk0[:, 2, 10].any()
    # a skipped half-word, then an entry in the next one
    assert (skip[..., :-1] & entered[..., 1:]).any()
    # a wave that traded is skipped again once flat and settled
    traded_before = np.cumsum(entered, axis=-1) > 0
    assert (skip[:, 0, 3] & traded_before[:, 0, 3]).any()
    # the padding lanes of the second chunk never keep a wave busy
    assert skip[:, 1, 1:].all() and not skip[:, 1, 0].all()


@pytest.mark.parametrize("variant", tr.VARIANTS)
def test_variant_moves_a_metric(directed, variant):
    (candles, pop, ef, xf, eq), metrics, _ = directed
    wrong, _ = tr.trades_ref(candles, pop, ef, xf, eq, variant=variant)
    changed = (wrong != metrics).any(axis=-1)              # (P, nsym)
    assert changed.any(), variant
    # ... and on the scripted lanes of the scripted symbol
    assert changed[:32, 0].any(), variant


@pytest.mark.parametrize("T", [1, 63, 64, 65, 700])
def test_pack_unpack_round_trip(T):
    rng = np.random.default_rng(T)
    flags = rng.random((5, 3, T)) < 0.5
    flags[0] = True
    flags[1] = False
    words = tr.pack_flags(flags)
    nwords = (T + 63) // 64
    assert words.shape == (3, nwords, 5) and words.dtype == np.int64
    bits, pad = tr.unpack_flags(words, T)
    np.testing.assert_array_equal(bits, flags)
    assert pad.shape == (5, 3, nwords * 64 - T) and not pad.any()
    # bit t & 63 of word t >> 6, by plain integer arithmetic
    u = words.view(np.uint64)
    for t in {0, T // 2, T - 1}:
        got = (u[:, t >> 6, :] >> np.uint64(t & 63)) & np.uint64(1)
        np.testing.assert_array_equal(got.T.astype(bool), flags[:, :, t])
    # padding bits that are set come back as padding, not as flags
    if nwords * 64 > T:
        dirty = words.copy()
        dirty[:, -1, :] |= np.int64(-1) << np.int64(T & 63)
        bits2, pad2 = tr.unpack_flags(dirty, T)
        np.testing.assert_array_equal(bits2, flags)
        assert pad2.all()
