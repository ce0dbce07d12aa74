"""GPU backtest op wrappers for the strategy families (HIP kernels:
ops/hip/backtest_grid.hip, ops/hip/backtest_dca.hip, and their recording
siblings in ops/hip/backtest_fills.hip).

CPU golden twins: backtesting/engine_grid_cpu.run_grid_backtest_cpu and
backtesting/engine_dca_cpu.run_dca_backtest_cpu — each pair implements the
per-candle state machine specified in backtesting/strategy_grid.py /
strategy_dca.py and emits the metrics tensor of ops/backtest.py.
"""

from __future__ import annotations

import torch

from . import require_hip_ops
from ..backtesting.engine_cpu import NMETRIC
from ..backtesting.fills import (
    DEFAULT_MAX_FILLS, FIELDS, INT_FIELDS, RECORD_BYTES, FillLedger,
    n_equity_samples,
)
from ..backtesting.strategy_dca import DCA_NPARAM
from ..backtesting.strategy_grid import GRID_NPARAM


def _run_family(op_name: str, nparam: int, candles: torch.Tensor,
                population: torch.Tensor,
                initial_equity: float) -> torch.Tensor:
    ops = require_hip_ops()
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    assert candles.dim() == 3 and candles.shape[2] == 4
    assert population.dim() == 2 and population.shape[1] == nparam
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    metrics = torch.empty(
        (P, nsym, NMETRIC), dtype=torch.float32, device=candles.device
    )
    stream = torch.cuda.current_stream(candles.device).cuda_stream
    getattr(ops, op_name)(
        candles.data_ptr(), population.data_ptr(), metrics.data_ptr(),
        nsym, T, P, float(initial_equity), stream,
    )
    return metrics


def run_grid_backtest_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, GRID_NPARAM) f32 cuda
    *,
    initial_equity: float = 1.0,
) -> torch.Tensor:             # (P, nsym, NMETRIC) f32 cuda
    return _run_family("backtest_grid", GRID_NPARAM, candles, population,
                       initial_equity)


def run_dca_backtest_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, DCA_NPARAM) f32 cuda
    *,
    initial_equity: float = 1.0,
) -> torch.Tensor:             # (P, nsym, NMETRIC) f32 cuda
    return _run_family("backtest_dca", DCA_NPARAM, candles, population,
                       initial_equity)


def _run_family_fills(op_name: str, nparam: int, candles: torch.Tensor,
                      population: torch.Tensor, max_fills: int,
                      equity_stride: int, initial_equity: float) -> FillLedger:
    ops = require_hip_ops()
    assert candles.is_cuda and population.is_cuda
    assert candles.dtype == torch.float32
    assert population.dtype == torch.float32
    assert candles.dim() == 3 and candles.shape[2] == 4
    assert population.dim() == 2 and population.shape[1] == nparam
    max_fills, equity_stride = int(max_fills), int(equity_stride)
    assert max_fills >= 1 and equity_stride >= 1
    candles = candles.contiguous()
    population = population.contiguous()
    nsym, T, _ = candles.shape
    P = population.shape[0]
    assert nsym >= 1 and T >= 1 and P >= 1
    n_samples = n_equity_samples(T, equity_stride)
    dev = candles.device
    nbytes = P * nsym * (RECORD_BYTES * max_fills + 4 * n_samples)
    free, _total = torch.cuda.mem_get_info(dev)
    assert nbytes <= free, (
        f"fill ledger output needs {nbytes / 2**30:.1f} GiB "
        f"({P} x {nsym} lanes x ({max_fills} records + {n_samples} equity "
        f"samples)), {free / 2**30:.1f} GiB free: lower max_fills, raise "
        f"equity_stride or run fewer strategies")
    metrics = torch.empty((P, nsym, NMETRIC), dtype=torch.float32,
                          device=dev)
    n_records = torch.zeros((P, nsym), dtype=torch.int32, device=dev)
    # lane-major records of 8 32-bit words: three ints, five floats. The
    # kernel writes whole records only, so unused slots keep this filler:
    # -1 in the integer fields, 0 in the float fields.
    words = torch.zeros((P, nsym, max_fills, len(FIELDS)),
                        dtype=torch.int32, device=dev)
    words[..., :len(INT_FIELDS)] = -1
    # time-major with the strategy fastest: a wave's stores coalesce
    equity = torch.empty((nsym, n_samples, P), dtype=torch.float32,
                         device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    getattr(ops, op_name)(
        candles.data_ptr(), population.data_ptr(), metrics.data_ptr(),
        n_records.data_ptr(), words.data_ptr(), equity.data_ptr(),
        nsym, T, P, max_fills, equity_stride, n_samples,
        float(initial_equity), stream,
    )
    fwords = words.view(torch.float32)
    cols = [words[..., i] if f in INT_FIELDS else fwords[..., i]
            for i, f in enumerate(FIELDS)]
    return FillLedger(metrics, n_records, *cols, equity.permute(2, 0, 1),
                      equity_stride)


def run_grid_fills_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, GRID_NPARAM) f32 cuda
    *,
    max_fills: int = DEFAULT_MAX_FILLS,
    equity_stride: int = 1,
    initial_equity: float = 1.0,
) -> FillLedger:
    """run_grid_backtest_gpu plus what each lane did (HIP kernel:
    ops/hip/backtest_fills.hip): up to `max_fills` fill records per
    (strategy, symbol) and the equity sampled every `equity_stride`
    candles, as a `FillLedger` of cuda tensors (backtesting/fills.py has
    the contract). CPU twin: run_grid_backtest_cpu(record_fills=True).
    Meant for inspecting a few strategies, not a population: the output
    is P*nsym*(32*max_fills + 4*ceil(T/equity_stride)) bytes."""
    return _run_family_fills("backtest_grid_fills", GRID_NPARAM, candles,
                             population, max_fills, equity_stride,
                             initial_equity)


def run_dca_fills_gpu(
    candles: torch.Tensor,     # (nsym, T, 4) f32 cuda
    population: torch.Tensor,  # (P, DCA_NPARAM) f32 cuda
    *,
    max_fills: int = DEFAULT_MAX_FILLS,
    equity_stride: int = 1,
    initial_equity: float = 1.0,
) -> FillLedger:
    """run_dca_backtest_gpu plus each order and take-profit, as
    run_grid_fills_gpu. CPU twin: run_dca_backtest_cpu(record_fills=True)."""
    return _run_family_fills("backtest_dca_fills", DCA_NPARAM, candles,
                             population, max_fills, equity_stride,
                             initial_equity)
