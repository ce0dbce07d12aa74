"""Registry of the non-vote strategy families.

Each family is a parameter layout plus a per-candle state machine with a
numpy twin and a HIP kernel, all emitting the (P, nsym, NMETRIC) metrics
tensor of the vote machine. GAEngine(family=...) and
BacktestEngine.run_backtest(strategy=...) look families up here; the vote
machine ("vote") keeps its own direct code paths and is not listed.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

from . import strategy_dca as _dca
from . import strategy_grid as _grid
from .engine_dca_cpu import run_dca_backtest_cpu
from .engine_grid_cpu import run_grid_backtest_cpu


def _run_grid_gpu(candles, population, **kw):
    from ..ops.backtest_families import run_grid_backtest_gpu

    return run_grid_backtest_gpu(candles, population, **kw)


def _run_dca_gpu(candles, population, **kw):
    from ..ops.backtest_families import run_dca_backtest_gpu

    return run_dca_backtest_gpu(candles, population, **kw)


def _run_grid_fills_cpu(candles, population, **kw):
    return run_grid_backtest_cpu(candles, population, record_fills=True,
                                 **kw)


def _run_dca_fills_cpu(candles, population, **kw):
    return run_dca_backtest_cpu(candles, population, record_fills=True, **kw)


def _run_grid_fills_gpu(candles, population, **kw):
    from ..ops.backtest_families import run_grid_fills_gpu

    return run_grid_fills_gpu(candles, population, **kw)


def _run_dca_fills_gpu(candles, population, **kw):
    from ..ops.backtest_families import run_dca_fills_gpu

    return run_dca_fills_gpu(candles, population, **kw)


@dataclass(frozen=True)
class Family:
    name: str
    nparam: int
    names: list
    bounds: np.ndarray                  # (nparam, 3): lo, hi, is_int
    clip: Callable                      # (P, nparam) -> f32 in bounds
    random_population: Callable         # (pop, seed) -> (pop, nparam)
    params_to_dict: Callable
    dict_to_params: Callable
    run_cpu: Callable                   # numpy twin
    run_gpu: Callable                   # HIP op (torch tensors)
    # the same runs with the fill ledger (backtesting/fills.py): keywords
    # max_fills, equity_stride, initial_equity; return a FillLedger
    run_cpu_fills: Callable
    run_gpu_fills: Callable


FAMILIES = {
    "grid": Family(
        "grid", _grid.GRID_NPARAM, _grid.GRID_PARAM_NAMES,
        _grid.GRID_PARAM_BOUNDS,
        _grid.clip_grid_params, _grid.random_grid_population,
        _grid.grid_params_to_dict, _grid.dict_to_grid_params,
        run_grid_backtest_cpu, _run_grid_gpu,
        _run_grid_fills_cpu, _run_grid_fills_gpu),
    "dca": Family(
        "dca", _dca.DCA_NPARAM, _dca.DCA_PARAM_NAMES,
        _dca.DCA_PARAM_BOUNDS,
        _dca.clip_dca_params, _dca.random_dca_population,
        _dca.dca_params_to_dict, _dca.dict_to_dca_params,
        run_dca_backtest_cpu, _run_dca_gpu,
        _run_dca_fills_cpu, _run_dca_fills_gpu),
}


def get_family(name: str) -> Family:
    try:
        return FAMILIES[name]
    except KeyError:
        raise ValueError(
            f"unknown strategy family {name!r} "
            f"(known: vote, {', '.join(sorted(FAMILIES))})") from None
