"""GPU backtest op wrappers for the strategy families (HIP kernels:
ops/hip/backtest_grid.hip, ops/hip/backtest_dca.hip).

CPU golden twins: backtesting/engine_grid_cpu.run_grid_backtest_cpu and
backtesting/engine_dca_cpu.run_dca_backtest_cpu — each pair implements the
per-candle state machine specified in backtesting/strategy_grid.py /
strategy_dca.py and emits the metrics tensor of ops/backtest.py.
"""

from __future__ import annotations

import torch

from . import require_hip_ops
from ..backtesting.engine_cpu import NMETRIC
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
