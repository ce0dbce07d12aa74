"""GA evolution op wrapper (HIP kernel: ops/hip/ga.hip) + host-side GA.

The device kernel evolves a device-resident population in place;
GeneticAlgorithm (services side) uses these ops when a GPU is present and
the numpy path otherwise (genetic_algorithm.py:27-291 parity).
"""

from __future__ import annotations

import numpy as np

from . import require_hip_ops
from ..backtesting.strategy import NPARAM, PARAM_BOUNDS, clip_params


MAX_TOURNAMENT = 4
GEN_WRAP = 1 << 20


def check_tournament(tournament: int) -> int:
    """The evolve kernels draw eight Philox words per child and give
    tournament A words 0..3 and tournament B words 4..7. Above four
    contestants the two tournaments would share draws (at eight they are
    identical, both parents are the same individual and crossover does
    nothing), so a size outside 1..4 is refused, not run."""
    if not 1 <= int(tournament) <= MAX_TOURNAMENT:
        raise ValueError(
            f"tournament must be in 1..{MAX_TOURNAMENT}, got {tournament}: "
            "each child has eight Philox words for its two tournaments, "
            "four apiece; a larger tournament would make the two parents' "
            "draws overlap")
    return int(tournament)


def _check_evolve_args(pop, fitness, bounds_t, elite_k, tournament):
    """Shared checks of the two GPU wrappers. -> (P, nparam)."""
    import torch

    if pop.dim() != 2:
        raise ValueError(f"pop must be (P, nparam), got {tuple(pop.shape)}")
    P, nparam = pop.shape
    args = (("pop", pop, (P, nparam)), ("fitness", fitness, (P,)),
            ("bounds", bounds_t, (nparam, 3)))
    for name, t, shape in args:
        if tuple(t.shape) != shape:
            raise ValueError(
                f"{name} must have shape {shape}, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not 0 <= int(elite_k) <= P:
        raise ValueError(f"elite_k must be in 0..{P}, got {elite_k}")
    check_tournament(tournament)
    for name, t, _ in args:
        if not t.is_cuda or t.device != pop.device:
            raise ValueError(f"{name} must be on the GPU of pop")
    return P, nparam


def _rank(fitness):
    """(fitness with NaN -> -inf, its stable descending argsort as int32).
    A NaN fitness ranks last, as in the numpy path, and never wins a
    tournament; ties keep their index order, so every rank and every run
    picks the same elites."""
    import torch

    fitness = torch.nan_to_num(fitness.contiguous(), nan=float("-inf"),
                               posinf=float("inf"), neginf=float("-inf"))
    order = torch.argsort(fitness, descending=True, stable=True)
    return fitness, order.to(torch.int32)


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
    """One generation: returns the next population (new contiguous
    tensor). tournament must be in 1..4 (check_tournament); only the low
    20 bits of gen enter the Philox counter; NaN fitness counts as -inf."""
    import torch

    if bounds_t is None:
        bounds_t = torch.from_numpy(np.ascontiguousarray(PARAM_BOUNDS)).to(
            pop.device
        )
    if pop.dim() == 2 and pop.shape[1] != NPARAM:
        raise ValueError(
            f"pop must have {NPARAM} slots, got {pop.shape[1]}")
    P, nparam = _check_evolve_args(pop, fitness, bounds_t, elite_k,
                                   tournament)
    ops = require_hip_ops()
    fitness, order = _rank(fitness)
    out = torch.empty((P, NPARAM), dtype=torch.float32, device=pop.device)
    stream = torch.cuda.current_stream(pop.device).cuda_stream
    # named, so that a copy lives until the launch
    pop, bounds_t = pop.contiguous(), bounds_t.contiguous()
    ops.ga_evolve(
        pop.data_ptr(), fitness.data_ptr(),
        order.data_ptr(), bounds_t.data_ptr(),
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
    bit-identical to the GPU kernel (different RNG streams): the kernel's
    value-level reference is the exact twin in tests/ga_refs.py."""
    rng = np.random.default_rng((seed * 1_000_003 + gen) & 0xFFFFFFFF)
    P = pop.shape[0]
    elite_k = min(elite_k, max(P // 4, 1))
    order = np.argsort(-fitness, kind="stable")    # NaN last, ties by index
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
    and no slot-specific fix-ups (ga.hip ga_evolve_generic_kernel). The
    same limits hold: tournament in 1..4, gen modulo 2^20, NaN fitness
    counts as -inf."""
    import torch

    P, nparam = _check_evolve_args(pop, fitness, bounds_t, elite_k,
                                   tournament)
    ops = require_hip_ops()
    fitness, order = _rank(fitness)
    out = torch.empty((P, nparam), dtype=torch.float32, device=pop.device)
    stream = torch.cuda.current_stream(pop.device).cuda_stream
    pop, bounds_t = pop.contiguous(), bounds_t.contiguous()
    ops.ga_evolve_generic(
        pop.data_ptr(), fitness.data_ptr(),
        order.data_ptr(), bounds_t.data_ptr(),
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
    order = np.argsort(-fitness, kind="stable")    # NaN last, ties by index
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
