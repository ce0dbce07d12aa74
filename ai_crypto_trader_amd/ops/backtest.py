"""GPU backtest op wrapper (HIP kernel: ops/hip/backtest.hip).

CPU golden reference: backtesting/engine_cpu.run_backtest_cpu — both
implement the per-candle state machine specified in
backtesting/strategy.py.
"""

from __future__ import annotations

import torch

from . import require_hip_ops
from ..backtesting.engine_cpu import NMETRIC
from ..backtesting.ledger import (
    DEFAULT_MAX_TRADES, FIELDS, INT_FIELDS, RECORD_BYTES, Ledger,
    n_equity_samples,
)
from ..backtesting.portfolio import (
    PortfolioResult, check_shape, n_portfolio_samples,
)
from ..backtesting.strategy import (
    MAX_WIN, NPARAM, RESNAP, SHARED_HALO, WARMUP,
)


def run_backtest_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, NPARAM) f32 cuda
    *,
    initial_equity: float = 1.0,
) -> torch.Tensor:             # (P, nsym, NMETRIC) f32 cuda
    ops = require_hip_ops()
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    assert candles.dim() == 3 and candles.shape[2] == 4
    assert population.dim() == 2 and population.shape[1] == NPARAM
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    metrics = torch.empty(
        (P, nsym, NMETRIC), dtype=torch.float32, device=candles.device
    )
    stream = torch.cuda.current_stream(candles.device).cuda_stream
    ops.backtest(
        candles.data_ptr(), population.data_ptr(), metrics.data_ptr(),
        nsym, T, P, float(initial_equity), stream,
    )
    return metrics


def run_backtest_ledger_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, NPARAM) f32 cuda
    *,
    max_trades: int = DEFAULT_MAX_TRADES,
    equity_stride: int = 1,
    initial_equity: float = 1.0,
) -> Ledger:
    """run_backtest_gpu plus what each lane did (HIP kernel:
    ops/hip/backtest_ledger.hip): up to `max_trades` trade records per
    (strategy, symbol) and the equity sampled every `equity_stride`
    candles, as a `Ledger` of cuda tensors (backtesting/ledger.py has the
    contract). CPU twin: run_backtest_cpu(record_trades=True), equal bit
    for bit. Meant for inspecting a few strategies, not a population:
    the output is P*nsym*(32*max_trades + 4*ceil(T/equity_stride)) bytes.
    """
    ops = require_hip_ops()
    _check_contract(ops)
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    assert candles.dim() == 3 and candles.shape[2] == 4
    assert population.dim() == 2 and population.shape[1] == NPARAM
    max_trades, equity_stride = int(max_trades), int(equity_stride)
    assert max_trades >= 1 and equity_stride >= 1
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    assert nsym >= 1 and T >= 1 and P >= 1
    n_samples = n_equity_samples(T, equity_stride)
    dev = candles.device
    nbytes = P * nsym * (RECORD_BYTES * max_trades + 4 * n_samples)
    free, _total = torch.cuda.mem_get_info(dev)
    assert nbytes <= free, (
        f"ledger output needs {nbytes / 2**30:.1f} GiB "
        f"({P} x {nsym} lanes x ({max_trades} records + {n_samples} equity "
        f"samples)), {free / 2**30:.1f} GiB free: lower max_trades, raise "
        f"equity_stride or run fewer strategies")
    metrics = torch.empty((P, nsym, NMETRIC), dtype=torch.float32,
                          device=dev)
    n_records = torch.zeros((P, nsym), dtype=torch.int32, device=dev)
    # lane-major records of 8 32-bit words: three ints, five floats. The
    # kernel writes whole records only, so unused slots keep this filler:
    # -1 in the integer fields, 0 in the float fields.
    words = torch.zeros((P, nsym, max_trades, len(FIELDS)),
                        dtype=torch.int32, device=dev)
    words[..., :len(INT_FIELDS)] = -1
    # time-major with the strategy fastest: a wave's stores coalesce
    equity = torch.empty((nsym, n_samples, P), dtype=torch.float32,
                         device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ops.backtest_ledger(
        candles.data_ptr(), population.data_ptr(), metrics.data_ptr(),
        n_records.data_ptr(), words.data_ptr(), equity.data_ptr(),
        nsym, T, P, max_trades, equity_stride, n_samples,
        float(initial_equity), stream,
    )
    fwords = words.view(torch.float32)
    cols = [words[..., i] if f in INT_FIELDS else fwords[..., i]
            for i, f in enumerate(FIELDS)]
    return Ledger(metrics, n_records, *cols, equity.permute(2, 0, 1),
                  equity_stride)


# Flag-bitmap buffers reused across GA generations (16.4 GB at the
# flagship 1024x64x1M shape — allocated once, not per step).
_flag_cache: dict = {}


def pick_nshards(nsym: int, T: int, P: int, *, target_blocks: int = 6144,
                 tail: int = 2048) -> int:
    """Time shards for bt_flags: enough blocks to oversubscribe every CU,
    bounded so each shard body is >= one RESNAP period and >= 4x the
    warm tail. 24 shards x 8 even time groups measured best end-to-end
    at the flagship shape (234 G/s; full sweep in
    profiles/backtest_continuous_pmc.json)."""
    chunks = (P + 255) // 256
    base = nsym * chunks
    want = max(1, -(-target_blocks // base))
    max_shards = max(1, T // max(RESNAP, 4 * tail))
    return min(want, max_shards, 64)


def _flag_buffers(ops, nsym: int, nwords: int, P: int, dev):
    """(eflags, xflags, carry) of this shape from _flag_cache, allocated
    on a miss — which drops the buffers of any other shape."""
    key = (nsym, nwords, P, dev.index)
    bufs = _flag_cache.get(key)
    if bufs is None or bufs[0].device != dev:
        eflags = torch.empty((nsym, nwords, P), dtype=torch.int64,
                             device=dev)
        xflags = torch.empty_like(eflags)
        carry = torch.empty((P, nsym, ops.BT_NSTATE),
                            dtype=torch.float32, device=dev)
        _flag_cache.clear()      # one shape live at a time (16 GB-class)
        bufs = _flag_cache[key] = (eflags, xflags, carry)
    return bufs


_pipe_streams: dict = {}

_contract_checked = False


def _check_contract(ops) -> None:
    """The constants compiled into the kernels (ops/hip/bt_vote.hpp) must
    be the ones backtesting/strategy.py specifies. Checked once."""
    global _contract_checked
    if _contract_checked:
        return
    got = (ops.BT_NPARAM, ops.BT_NMETRIC, ops.BT_MAXWIN, ops.BT_HALO,
           ops.BT_WARMUP, ops.BT_RESNAP)
    want = (NPARAM, NMETRIC, MAX_WIN, SHARED_HALO, WARMUP, RESNAP)
    assert got == want, f"kernel contract {got} != strategy.py {want}"
    _contract_checked = True


def run_backtest_continuous_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, NPARAM) f32 cuda
    *,
    initial_equity: float = 1.0,
    nshards: int = 0,          # 0 = auto
    tail: int = 2048,
    time_groups: int = 0,      # 0 = auto; 1 = serial two-launch path
) -> torch.Tensor:             # (P, nsym, NMETRIC) f32 cuda
    """Continuous (unsegmented) backtest via the time-parallel kernel
    pair (ops/hip/backtest_tp.hip): indicator/vote flags computed with
    the time axis split across shards (warm-tail reconverged EMA/RSI +
    RESNAP-exact Bollinger), then the exact sequential position state
    machine over packed flag words. Same metrics contract as
    run_backtest_gpu / engine_cpu.run_backtest_cpu.

    Overlap: the flags shards launch in `time_groups` groups on stream
    F; the trades kernel is resumable over candle ranges (bitwise state
    carry in HBM) and chunk g launches on stream T as soon as flags
    group g completes. The latency-bound trades chain (1 wave/SIMD,
    ~50% issue-idle) thus walks candles co-resident with the
    issue-bound flags waves instead of after them — the chip runs both
    at once and total time approaches max(flags, trades) + first-group
    latency. (Symbol-group pipelining was measured and rejected: the
    trades wall time is the length of the serial candle chain,
    independent of lane count, so symbol groups serialize G full-length
    chains.)"""
    ops = require_hip_ops()
    _check_contract(ops)
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    # a shard warm-starts `tail` candles before its RESNAP-aligned body,
    # and the first such body starts at RESNAP
    assert tail % 256 == 0 and 0 <= tail <= RESNAP
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    if nshards <= 0:
        nshards = pick_nshards(nsym, T, P, tail=tail)
    # shard bodies must be RESNAP-aligned (BB restart exactness)
    nshards = min(nshards, max(1, T // RESNAP))
    nwords = (T + 63) // 64
    dev = candles.device
    eflags, xflags, carry = _flag_buffers(ops, nsym, nwords, P, dev)
    metrics = torch.empty((P, nsym, NMETRIC), dtype=torch.float32,
                          device=dev)
    cptr = candles.data_ptr()
    pptr = population.data_ptr()

    if time_groups <= 0:
        time_groups = 8 if nshards >= 8 else 1
    time_groups = min(time_groups, nshards)
    if time_groups == 1:
        stream = torch.cuda.current_stream(dev).cuda_stream
        ops.bt_flags(cptr, pptr, eflags.data_ptr(), xflags.data_ptr(),
                     nsym, T, P, nshards, tail, 0, nshards, stream)
        ops.bt_trades(cptr, pptr, eflags.data_ptr(), xflags.data_ptr(),
                      metrics.data_ptr(), nsym, T, P,
                      float(initial_equity), 0, nsym, 0, T, 0, stream)
        return metrics

    ss = _pipe_streams.get(dev.index)
    if ss is None:
        # trades on the high-priority stream (measured neutral on
        # MI355X — CU arbitration ignores stream priority — but it
        # documents intent and costs nothing)
        ss = (torch.cuda.Stream(dev),
              torch.cuda.Stream(dev, priority=-1))
        _pipe_streams[dev.index] = ss
    sf, st = ss
    cur = torch.cuda.current_stream(dev)
    start_ev = torch.cuda.Event()
    start_ev.record(cur)
    sf.wait_event(start_ev)
    st.wait_event(start_ev)
    # balanced RESNAP-aligned shard boundaries (must match the kernel's
    # own formula: floor(s*T/S) to the RESNAP grid)
    def shard_lo(s):
        return (s * T // nshards) // RESNAP * RESNAP if s < nshards else T

    # even shard groups: trades chunks cover equal time slices and every
    # flags launch keeps full occupancy. Both a small-first-group and a
    # geometric schedule were measured WORSE (209 / 199 vs 234 G/s): a
    # 1-shard flags launch runs at poor occupancy and delays the whole
    # pipeline, and geometric sizing parks half the timeline behind the
    # final flags launch.
    sbounds = [nshards * g // time_groups for g in range(time_groups + 1)]
    evs = []
    for g in range(time_groups):
        s0, s1 = sbounds[g], sbounds[g + 1]
        ops.bt_flags(cptr, pptr, eflags.data_ptr(), xflags.data_ptr(),
                     nsym, T, P, nshards, tail, s0, s1 - s0,
                     sf.cuda_stream)
        ev = torch.cuda.Event()
        ev.record(sf)
        evs.append(ev)
    for g in range(time_groups):
        s0, s1 = sbounds[g], sbounds[g + 1]
        t_lo = shard_lo(s0)
        t_hi = T if s1 == nshards else shard_lo(s1)
        st.wait_event(evs[g])
        ops.bt_trades(cptr, pptr, eflags.data_ptr(), xflags.data_ptr(),
                      metrics.data_ptr(), nsym, T, P,
                      float(initial_equity), 0, nsym, t_lo, t_hi,
                      carry.data_ptr(), st.cuda_stream)
    done = torch.cuda.Event()
    done.record(st)
    cur.wait_event(done)
    return metrics


def run_backtest_portfolio_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda, 1 <= nsym <= 64
    population: torch.Tensor,  # (P, NPARAM) f32 cuda
    *,
    max_positions: int,
    initial_equity: float = 1.0,
    equity_stride: int = 0,    # 0 = no equity samples
    nshards: int = 0,          # 0 = auto
    tail: int = 2048,
) -> PortfolioResult:
    """Each strategy trades the whole basket from one cash account with at
    most `max_positions` open at once (contract: backtesting/portfolio.py):
    the vote flags by bt_flags (ops/hip/backtest_tp.hip), then the
    portfolio position machine (ops/hip/backtest_portfolio.hip) over them,
    both on the current stream. Returns a PortfolioResult of cuda tensors.
    CPU twin: engine_portfolio_cpu.run_portfolio_backtest_cpu, equal bit
    for bit. Shares the flag buffers of run_backtest_continuous_gpu."""
    ops = require_hip_ops()
    _check_contract(ops)
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    assert candles.dim() == 3 and candles.shape[2] == 4
    assert population.dim() == 2 and population.shape[1] == NPARAM
    assert tail % 256 == 0 and 0 <= tail <= RESNAP
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    max_positions, equity_stride = int(max_positions), int(equity_stride)
    check_shape(nsym, max_positions, equity_stride)
    assert T >= 1 and P >= 1
    if nshards <= 0:
        nshards = pick_nshards(nsym, T, P, tail=tail)
    nshards = min(nshards, max(1, T // RESNAP))
    nwords = (T + 63) // 64
    dev = candles.device
    eflags, xflags, _carry = _flag_buffers(ops, nsym, nwords, P, dev)
    n_samples = n_portfolio_samples(T, equity_stride)
    metrics = torch.empty((P, NMETRIC), dtype=torch.float32, device=dev)
    per_symbol = torch.empty((P, nsym, 4), dtype=torch.float32, device=dev)
    refused = torch.empty((P, 2), dtype=torch.int32, device=dev)
    equity = (torch.empty((P, n_samples), dtype=torch.float32, device=dev)
              if equity_stride else None)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ops.bt_flags(candles.data_ptr(), population.data_ptr(),
                 eflags.data_ptr(), xflags.data_ptr(), nsym, T, P, nshards,
                 tail, 0, nshards, stream)
    ops.bt_portfolio(
        candles.data_ptr(), population.data_ptr(), eflags.data_ptr(),
        xflags.data_ptr(), metrics.data_ptr(), per_symbol.data_ptr(),
        refused.data_ptr(), equity.data_ptr() if equity_stride else 0,
        nsym, T, P, max_positions, float(initial_equity), equity_stride,
        n_samples, stream)
    return PortfolioResult(metrics, per_symbol, refused, equity,
                           equity_stride)


def fitness_from_metrics(metrics: torch.Tensor) -> torch.Tensor:
    """Aggregate per-(param, symbol) fitness to per-param GA fitness:
    mean across symbols (the reference's GA evaluates one fitness per
    individual, strategy_evolution_service.py:525-694)."""
    return metrics[..., 9].mean(dim=1)
