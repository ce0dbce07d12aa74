"""The two kernels of the continuous backtest (ops/hip/backtest_tp.hip),
each alone and bit for bit: bt_flags_kernel's bitmaps against the CPU
engine's votes at every (strategy, symbol, candle) — most of which the
position machine never looks at — and bt_trades_kernel against
tp_refs.trades_ref on directed flag planes, in one launch, resumed at tile
boundaries and split into symbol groups. test_tp_refs_cpu.py checks the
references themselves."""

import numpy as np
import pytest

import tp_refs as tr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = 0x5555555555555555
TILE = 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(dev):
    from ai_crypto_trader_amd.backtesting.strategy import RESNAP, WARMUP
    from ai_crypto_trader_amd.ops import require_hip_ops

    ops = require_hip_ops()
    assert ops.BT_RESNAP == RESNAP and ops.BT_WARMUP == WARMUP
    return ops


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------
class FlagsCase:
    """Inputs on the device plus the CPU engine's planes and metrics."""

    def __init__(self, dev, candles, pop):
        self.dev = dev
        self.candles, self.pop = candles, pop
        self.nsym, self.T, _ = candles.shape
        self.P = pop.shape[0]
        self.nwords = (self.T + 63) // 64
        self.ef, self.xf, self.metrics = tr.cpu_flags(candles, pop)
        self.c_t = torch.from_numpy(candles).to(dev)
        self.p_t = torch.from_numpy(pop).to(dev)

    def sentinel_buffers(self):
        shape = (self.nsym, self.nwords, self.P)
        return (torch.full(shape, SENTINEL, dtype=torch.int64,
                           device=self.dev),
                torch.full(shape, SENTINEL, dtype=torch.int64,
                           device=self.dev))

    def launch(self, ops, bufs, nshards, tail, shard0=0, nlaunch=0):
        ops.bt_flags(self.c_t.data_ptr(), self.p_t.data_ptr(),
                     bufs[0].data_ptr(), bufs[1].data_ptr(), self.nsym,
                     self.T, self.P, nshards, tail, shard0, nlaunch,
                     _stream(self.dev))
        torch.cuda.synchronize()
        return bufs[0].cpu().numpy(), bufs[1].cpu().numpy()

    def assert_planes(self, words, cpu_plane, name, first_word=0):
        """Words first_word.. hold the CPU plane, zero padding bits and no
        sentinel; the words before them still hold the sentinel."""
        words = words.view(np.uint64)
        assert (words[:, :first_word] == np.uint64(SENTINEL)).all(), name
        assert not (words[:, first_word:] == np.uint64(SENTINEL)).any(), name
        bits, pad = tr.unpack_flags(words, self.T)
        t0 = first_word * 64
        diff = np.argwhere(bits[:, :, t0:] != cpu_plane[:, :, t0:])
        assert len(diff) == 0, (
            f"{name}: {len(diff)} bits differ, first (p, sym, t - {t0}) "
            f"{diff[:5].tolist()}")
        assert not pad.any(), name


def _market(T, nsym, seed):
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(T, nsym, seed=seed))


@pytest.fixture(scope="module")
def long_case(dev):
    """T = 2 * RESNAP + 300: the resnap candle fires at 16384 and 32768,
    T % 64 = 44 leaves the last word partial."""
    from ai_crypto_trader_amd.backtesting.strategy import (
        RESNAP, random_population,
    )
    T = 2 * RESNAP + 300
    assert T == 33068 and T % 64 == 44
    case = FlagsCase(dev, _market(T, 2, seed=41),
                     random_population(70, seed=23))
    for plane in (case.ef, case.xf):
        assert 0.01 < plane.mean() < 0.5, plane.mean()
    return case


@pytest.mark.parametrize("tail", [2048, 1024])
@pytest.mark.parametrize("nshards", [1, 2])
def test_flags_equal_cpu_votes_everywhere(ops, long_case, nshards, tail):
    """Every bit of both planes, the ignored ones included. With two shards
    the second warm-starts `tail` candles before candle RESNAP. At half the
    default tail its reconvergence is empirical: a numpy march of the same
    recurrences on these inputs leaves the Wilder averages of 11 of the 140
    lanes not yet bit-equal at the boundary (equal within 100 candles), and
    no vote differs."""
    bufs = long_case.sentinel_buffers()
    ew, xw = long_case.launch(ops, bufs, nshards, tail)
    long_case.assert_planes(ew, long_case.ef, "entry")
    long_case.assert_planes(xw, long_case.xf, "exit")


def test_flags_launch_writes_only_its_own_shards(ops, long_case):
    """What the overlap schedule rests on: shard 1 of 2 writes the words
    from candle RESNAP on and nothing else; shard 0 then fills the rest."""
    first = ops.BT_RESNAP // 64
    bufs = long_case.sentinel_buffers()
    ew, xw = long_case.launch(ops, bufs, 2, 2048, shard0=1, nlaunch=1)
    long_case.assert_planes(ew, long_case.ef, "entry", first_word=first)
    long_case.assert_planes(xw, long_case.xf, "exit", first_word=first)
    ew, xw = long_case.launch(ops, bufs, 2, 2048, shard0=0, nlaunch=1)
    long_case.assert_planes(ew, long_case.ef, "entry")
    long_case.assert_planes(xw, long_case.xf, "exit")


@pytest.mark.parametrize("T", [1, 63, 64, 65, 127, 128, 129, 257])
def test_flags_short_histories(ops, dev, T):
    from ai_crypto_trader_amd.backtesting.strategy import (
        WARMUP, random_population,
    )
    case = FlagsCase(dev, _market(T, 1, seed=300 + T),
                     random_population(5, seed=T))
    ew, xw = case.launch(ops, case.sentinel_buffers(), 1, 2048)
    case.assert_planes(ew, case.ef, "entry")
    case.assert_planes(xw, case.xf, "exit")
    if T <= WARMUP:
        assert not ew.any() and not xw.any()


def test_flags_second_chunk_and_padding_lanes(ops, dev):
    """T = 700, 3 symbols, 300 strategies: two strategy chunks, 212 padding
    lanes in the second, a partial last word."""
    from ledger_cases import eager_population, market

    case = FlagsCase(dev, market(700, 3, seed=31),
                     eager_population(300, seed=17))
    assert case.ef.any() and case.xf.any()
    ew, xw = case.launch(ops, case.sentinel_buffers(), 1, 2048)
    case.assert_planes(ew, case.ef, "entry")
    case.assert_planes(xw, case.xf, "exit")


# ---------------------------------------------------------------------
# trades
# ---------------------------------------------------------------------
class TradesCase:
    def __init__(self, dev, candles, pop, ef, xf, equity):
        self.dev = dev
        self.nsym, self.T, _ = candles.shape
        self.P = pop.shape[0]
        self.nwords = (self.T + 63) // 64
        self.equity = float(equity)
        self.c_t = torch.from_numpy(candles).to(dev)
        self.p_t = torch.from_numpy(pop).to(dev)
        self.e_t = torch.from_numpy(tr.pack_flags(ef)).to(dev)
        self.x_t = torch.from_numpy(tr.pack_flags(xf)).to(dev)

    def nan_metrics(self, ops):
        return torch.full((self.P, self.nsym, ops.BT_NMETRIC), float("nan"),
                          dtype=torch.float32, device=self.dev)

    def launch(self, ops, metrics, t_lo=0, t_hi=None, state=None,
               sym0=0, nsym=None):
        """Symbols [sym0, sym0 + nsym) over candles [t_lo, t_hi)."""
        t_hi = self.T if t_hi is None else t_hi
        nsym = self.nsym if nsym is None else nsym
        ops.bt_trades(
            self.c_t.data_ptr() + sym0 * self.T * 4 * 4,
            self.p_t.data_ptr(),
            self.e_t.data_ptr() + sym0 * self.nwords * self.P * 8,
            self.x_t.data_ptr() + sym0 * self.nwords * self.P * 8,
            metrics.data_ptr(), nsym, self.T, self.P, self.equity, sym0,
            self.nsym, t_lo, t_hi,
            0 if state is None else state.data_ptr(), _stream(self.dev))

    def single(self, ops):
        m = self.nan_metrics(ops)
        self.launch(ops, m)
        torch.cuda.synchronize()
        return m.cpu().numpy()


@pytest.fixture(scope="module")
def directed(dev):
    case = tr.directed_case()
    ref, _ = tr.trades_ref(*case)
    return TradesCase(dev, *case), ref


def _assert_metrics(got, ref):
    diff = np.argwhere((got != ref).any(axis=-1))
    assert len(diff) == 0, (
        f"{len(diff)} lanes differ, first (p, sym) {diff[:5].tolist()}: "
        f"{got[tuple(diff[0])]} != {ref[tuple(diff[0])]}")


def test_trades_directed_equals_ref(ops, directed):
    case, ref = directed
    assert not np.isnan(ref).any()
    _assert_metrics(case.single(ops), ref)


def test_trades_affine_equals_ref(ops, dev):
    inputs = tr.affine_case()
    ref, _ = tr.trades_ref(*inputs)
    assert not np.isnan(ref).any()
    _assert_metrics(TradesCase(dev, *inputs).single(ops), ref)


@pytest.mark.parametrize("cuts", [(256, 512), (512,)])
def test_trades_resume_at_tile_boundaries(ops, directed, cuts):
    """Candle ranges cut at multiples of the 256-tile that are no RESNAP
    multiples, the state carried through a buffer that started as NaN:
    positions are open, with a trailing stop, across both cuts."""
    case, ref = directed
    carry = torch.full((case.P, case.nsym, ops.BT_NSTATE), float("nan"),
                       dtype=torch.float32, device=case.dev)
    m = case.nan_metrics(ops)
    bounds = (0, *cuts, case.T)
    for t_lo, t_hi in zip(bounds[:-1], bounds[1:]):
        assert t_lo % TILE == 0
        case.launch(ops, m, t_lo, t_hi, state=carry)
    torch.cuda.synchronize()
    got = m.cpu().numpy()
    _assert_metrics(got, case.single(ops))
    _assert_metrics(got, ref)


def test_trades_symbol_groups(ops, directed):
    """Symbols [0, 2) and then symbol 2 alone, each launch given its
    group's candles and flag words, both writing into the (P, 3, NMETRIC)
    tensor."""
    case, ref = directed
    assert case.nsym == 3
    m = case.nan_metrics(ops)
    case.launch(ops, m, sym0=0, nsym=2)
    torch.cuda.synchronize()
    part = m.cpu().numpy()
    assert np.isnan(part[:, 2]).all() and not np.isnan(part[:, :2]).any()
    case.launch(ops, m, sym0=2, nsym=1)
    torch.cuda.synchronize()
    got = m.cpu().numpy()
    assert not np.isnan(got).any()
    _assert_metrics(got, case.single(ops))
    _assert_metrics(got, ref)


def test_trades_on_cpu_planes_across_resnap(ops, long_case):
    """Phase 2 alone on the CPU engine's own planes, over a history that
    crosses the resnap candle twice: the engine's metrics."""
    lc = long_case
    case = TradesCase(lc.dev, lc.candles, lc.pop, lc.ef, lc.xf, 1.0)
    assert lc.metrics[..., 1].sum() > 0
    _assert_metrics(case.single(ops), lc.metrics)


# ---------------------------------------------------------------------
# argument checks: on the host, before anything is launched
# ---------------------------------------------------------------------
def test_bad_arguments_raise_before_launch(ops, dev, directed):
    case, _ = directed
    R = ops.BT_RESNAP
    nsym, T, P = case.nsym, case.T, case.P
    stream = _stream(dev)

    # bt_flags(nsym, T, P, nshards, tail, shard0, nlaunch)
    ebuf = torch.full((nsym, case.nwords, P), SENTINEL, dtype=torch.int64,
                      device=dev)
    xbuf = ebuf.clone()

    def flags(*a):
        ops.bt_flags(case.c_t.data_ptr(), case.p_t.data_ptr(),
                     ebuf.data_ptr(), xbuf.data_ptr(), *a, stream)

    bad_flags = [
        (0, T, P, 1, 2048, 0, 1), (nsym, 0, P, 1, 2048, 0, 1),
        (nsym, T, 0, 1, 2048, 0, 1), (-1, T, P, 1, 2048, 0, 1),
        (nsym, T, P, 0, 2048, 0, 0),          # no shard
        (nsym, T, P, 2, 2048, 0, 2),          # T < 2 * RESNAP
        (nsym, T, P, 1, 100, 0, 1),           # tail off the tile grid
        (nsym, T, P, 1, -256, 0, 1),
        (nsym, T, P, 1, R + 256, 0, 1),       # tail > RESNAP
        (nsym, T, P, 1, 2048, -1, 1),
        (nsym, T, P, 1, 2048, 1, 0),          # shard0 past the last shard
        (nsym, T, P, 1, 2048, 0, 2),          # more shards than there are
    ]
    for a in bad_flags:
        with pytest.raises(ValueError):
            flags(*a)

    # the shard count that put shard 1's warm tail in front of the candles:
    # T = 2 * RESNAP + 300 holds two RESNAP periods, not three
    T2 = 2 * R + 300
    c2 = torch.zeros((2, T2, 4), dtype=torch.float32, device=dev)
    e2 = torch.full((2, (T2 + 63) // 64, P), SENTINEL, dtype=torch.int64,
                    device=dev)
    x2 = e2.clone()
    with pytest.raises(ValueError):
        ops.bt_flags(c2.data_ptr(), case.p_t.data_ptr(), e2.data_ptr(),
                     x2.data_ptr(), 2, T2, P, 3, 2048, 0, 3, stream)
    with pytest.raises(ValueError):
        ops.bt_flags(c2.data_ptr(), case.p_t.data_ptr(), e2.data_ptr(),
                     x2.data_ptr(), 2, T2, P, 2, 2048, 1, 2, stream)

    # bt_trades(nsym, T, P, equity, sym0, nsym_stride, t_lo, t_hi, state)
    metrics = case.nan_metrics(ops)
    carry = torch.full((P, nsym, ops.BT_NSTATE), float("nan"),
                       dtype=torch.float32, device=dev)
    st = carry.data_ptr()

    def trades(*a):
        ops.bt_trades(case.c_t.data_ptr(), case.p_t.data_ptr(),
                      case.e_t.data_ptr(), case.x_t.data_ptr(),
                      metrics.data_ptr(), *a, stream)

    bad_trades = [
        (0, T, P, 1.0, 0, nsym, 0, T, st), (nsym, 0, P, 1.0, 0, nsym, 0, 0, st),
        (nsym, T, 0, 1.0, 0, nsym, 0, T, st),
        (nsym, T, P, 1.0, -1, nsym, 0, T, st),
        (nsym, T, P, 1.0, 1, nsym, 0, T, st),     # sym0 + nsym > stride
        (nsym, T, P, 1.0, 0, nsym - 1, 0, T, st),
        (nsym, T, P, 1.0, 0, nsym, 32, T, st),    # t_lo off the tile grid
        (nsym, T, P, 1.0, 0, nsym, -256, T, st),
        (nsym, T, P, 1.0, 0, nsym, 256, 256, st),  # empty range
        (nsym, T, P, 1.0, 0, nsym, 512, 256, st),
        (nsym, T, P, 1.0, 0, nsym, 0, T + 1, st),
        (nsym, T, P, 1.0, 0, nsym, 0, 256, 0),    # a partial range, no state
        (nsym, T, P, 1.0, 0, nsym, 256, T, 0),
    ]
    for a in bad_trades:
        with pytest.raises(ValueError):
            trades(*a)

    # nothing ran: every output still holds what it was filled with
    torch.cuda.synchronize()
    for buf in (ebuf, xbuf, e2, x2):
        assert (buf == SENTINEL).all()
    assert torch.isnan(metrics).all() and torch.isnan(carry).all()


def test_wrapper_rejects_a_tail_longer_than_resnap(dev):
    from ai_crypto_trader_amd.backtesting.strategy import (
        RESNAP, random_population,
    )
    from ai_crypto_trader_amd.ops.backtest import run_backtest_continuous_gpu

    c_t = torch.from_numpy(_market(512, 1, seed=1)).to(dev)
    p_t = torch.from_numpy(random_population(4, seed=1)).to(dev)
    with pytest.raises(AssertionError):
        run_backtest_continuous_gpu(c_t, p_t, tail=RESNAP + 256)
