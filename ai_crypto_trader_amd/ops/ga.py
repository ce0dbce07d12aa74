"""GA evolution op wrapper (HIP kernel: ops/hip/ga.hip) + host-side GA.

The device kernel evolves a device-resident population in place;
GeneticAlgorithm (services side) uses these ops when a GPU is present and
the numpy path otherwise (genetic_algorithm.py:27-291 parity).
"""

from __future__ import annotations

import numpy as np

from . import require_hip_ops
from ..backtesting.strategy import NPARAM, PARAM_BOUNDS, clip_params


def ga_evolve_gpu(
    pop,                 # (P, NPARAM) f32 cuda
    fitness,             # (P,) f32 cuda
    *,
    elite_k: int = 8,
    tournament: int = 4,
    cx_rate: float = 0.5,
    mut_rate: float = 0.15,
    mut_scale: float = 0.1,
    seed: int = 0,
    gen: int = 0,
    bounds_t=None,
):
    """One generation: returns the next population (new tensor)."""
    import torch

    ops = require_hip_ops()
    P = pop.shape[0]
    assert pop.is_cuda and fitness.is_cuda
    order = torch.argsort(fitness, descending=True).to(torch.int32)
    if bounds_t is None:
        bounds_t = torch.from_numpy(np.ascontiguousarray(PARAM_BOUNDS)).to(
            pop.device
        )
    out = torch.empty_like(pop)
    stream = torch.cuda.current_stream(pop.device).cuda_stream
    ops.ga_evolve(
        pop.contiguous().data_ptr(), fitness.contiguous().data_ptr(),
        order.contiguous().data_ptr(), bounds_t.contiguous().data_ptr(),
        out.data_ptr(), P, elite_k, tournament, cx_rate, mut_rate, mut_scale,
        seed, gen, stream,
    )
    return out


def ga_evolve_cpu(
    pop: np.ndarray,
    fitness: np.ndarray,
    *,
    elite_k: int = 8,
    tournament: int = 4,
    cx_rate: float = 0.5,
    mut_rate: float = 0.15,
    mut_scale: float = 0.1,
    seed: int = 0,
    gen: int = 0,
) -> np.ndarray:
    """numpy GA generation (tournament + elitism + uniform crossover +
    gaussian mutation — genetic_algorithm.py:135-223 semantics). Not
    bit-identical to the GPU kernel (different RNG streams); tests check
    invariants on both."""
    rng = np.random.default_rng((seed * 1_000_003 + gen) & 0xFFFFFFFF)
    P = pop.shape[0]
    elite_k = min(elite_k, max(P // 4, 1))
    order = np.argsort(-fitness)
    out = np.empty_like(pop)
    out[:elite_k] = pop[order[:elite_k]]
    n_child = P - elite_k
    cand_a = rng.integers(0, P, size=(n_child, tournament))
    cand_b = rng.integers(0, P, size=(n_child, tournament))
    pa = cand_a[np.arange(n_child), np.argmax(fitness[cand_a], axis=1)]
    pb = cand_b[np.arange(n_child), np.argmax(fitness[cand_b], axis=1)]
    mask = rng.random((n_child, NPARAM)) < cx_rate
    child = np.where(mask, pop[pa], pop[pb])
    lo, hi = PARAM_BOUNDS[:, 0], PARAM_BOUNDS[:, 1]
    mut = rng.random((n_child, NPARAM)) < mut_rate
    noise = rng.standard_normal((n_child, NPARAM)) * mut_scale * (hi - lo)
    child = child + np.where(mut, noise, 0.0)
    out[elite_k:] = child.astype(np.float32)
    return clip_params(out)


def ga_evolve_family_gpu(
    pop,                 # (P, nparam) f32 cuda
    fitness,             # (P,) f32 cuda
    bounds_t,            # (nparam, 3) f32 cuda: lo, hi, is_int
    *,
    elite_k: int = 8,
    tournament: int = 4,
    cx_rate: float = 0.5,
    mut_rate: float = 0.15,
    mut_scale: float = 0.1,
    seed: int = 0,
    gen: int = 0,
):
    """One generation of any strategy family (backtesting/families.py):
    ga_evolve_gpu with the slot count and bounds taken from `bounds_t`
    and no slot-specific fix-ups (ga.hip ga_evolve_generic_kernel)."""
    import torch

    ops = require_hip_ops()
    P, nparam = pop.shape
    assert pop.is_cuda and fitness.is_cuda and bounds_t.is_cuda
    assert pop.dtype == torch.float32 and fitness.dtype == torch.float32
    assert bounds_t.dtype == torch.float32
    assert tuple(bounds_t.shape) == (nparam, 3)
    assert fitness.shape == (P,)
    assert 0 <= elite_k <= P
    order = torch.argsort(fitness, descending=True).to(torch.int32)
    out = torch.empty((P, nparam), dtype=torch.float32, device=pop.device)
    stream = torch.cuda.current_stream(pop.device).cuda_stream
    ops.ga_evolve_generic(
        pop.contiguous().data_ptr(), fitness.contiguous().data_ptr(),
        order.contiguous().data_ptr(), bounds_t.contiguous().data_ptr(),
        out.data_ptr(), P, nparam, elite_k, tournament, cx_rate, mut_rate,
        mut_scale, seed, gen, stream,
    )
    return out


def ga_evolve_family_cpu(
    pop: np.ndarray,
    fitness: np.ndarray,
    bounds: np.ndarray,      # (nparam, 3): lo, hi, is_int
    clip_fn,                 # the family's clip_*: (P, nparam) -> f32
    *,
    elite_k: int = 8,
    tournament: int = 4,
    cx_rate: float = 0.5,
    mut_rate: float = 0.15,
    mut_scale: float = 0.1,
    seed: int = 0,
    gen: int = 0,
) -> np.ndarray:
    """ga_evolve_cpu for any strategy family: same selection, crossover
    and mutation, with the slot count and bounds of `bounds` and the
    family's own clip."""
    rng = np.random.default_rng((seed * 1_000_003 + gen) & 0xFFFFFFFF)
    P, nparam = pop.shape
    elite_k = min(elite_k, max(P // 4, 1))
    order = np.argsort(-fitness)
    out = np.empty_like(pop)
    out[:elite_k] = pop[order[:elite_k]]
    n_child = P - elite_k
    cand_a = rng.integers(0, P, size=(n_child, tournament))
    cand_b = rng.integers(0, P, size=(n_child, tournament))
    pa = cand_a[np.arange(n_child), np.argmax(fitness[cand_a], axis=1)]
    pb = cand_b[np.arange(n_child), np.argmax(fitness[cand_b], axis=1)]
    mask = rng.random((n_child, nparam)) < cx_rate
    child = np.where(mask, pop[pa], pop[pb])
    lo, hi = bounds[:, 0], bounds[:, 1]
    mut = rng.random((n_child, nparam)) < mut_rate
    noise = rng.standard_normal((n_child, nparam)) * mut_scale * (hi - lo)
    child = child + np.where(mut, noise, 0.0)
    out[elite_k:] = child.astype(np.float32)
    return clip_fn(out)


def population_diversity(pop: np.ndarray) -> float:
    """Mean normalized per-param variance (genetic_algorithm.py:322-348)."""
    lo, hi = PARAM_BOUNDS[:, 0], PARAM_BOUNDS[:, 1]
    norm = (np.asarray(pop) - lo) / (hi - lo + 1e-12)
    return float(norm.var(axis=0).mean())
