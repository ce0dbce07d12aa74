"""An exact twin of the two GA evolution kernels of ops/hip/ga.hip, its
error envelope, an independent f32 emulation and seeded mutants (a helper
module, no tests of its own).

Shared by test_ga_refs_cpu.py, which shows on a CPU that the envelope is
reachable by a correct kernel (a scalar f32 emulation sits inside it) and
rejects a subtly wrong one (every seeded mutant leaves it on a named case),
and by test_gpu_ga.py, which holds ga_evolve_kernel and
ga_evolve_generic_kernel to it through the raw bindings and the wrappers.

Semantics encoded once (evolve_twin):
  - child i of generation gen draws from the Philox counter
    ctr = (i << 20) | (gen & 0xFFFFF), passed as ctr_lo; ctr_hi is the
    stream. Only the low 20 bits of gen enter: generation 2^20 + 5 repeats
    the draws of generation 5 (GEN_WRAP; docs/KERNELS.md documents it).
  - streams 0 and 1 give eight words w[0..7]. Tournament A reads
    w[k & 7], tournament B reads w[(k + 4) & 7], k < tournament: the two
    are independent for tournament <= 4 and share draws above it, which is
    why the wrappers refuse tournament > 4.
  - a contestant is word % P; it replaces the best so far on a strict f32
    ">" starting from -1e30, so the first of tied contestants wins and a
    NaN or -inf fitness never wins. A tournament nobody wins falls back to
    the child's own slot i.
  - slot j draws stream 2 + j: .x the crossover uniform, .y the mutation
    uniform, (.z, .w) the Box-Muller pair of which the first component is
    used, that is component 2 of philox_normal4.
  - per slot, in this order: v = A's value if u_cx < cx_rate else B's; if
    u_mut < mut_rate add g * mut_scale * (hi - lo); clip to [lo, hi]; round
    integer slots with rint (ties to even); only then, in the fixed-slot
    kernel, ema_slow (slot 4) = ema_fast (slot 3) + 1 where it is not
    larger.
  - children i < elite_k are copies of pop[order[i]], with order the
    STABLE descending argsort of the fitness after NaN -> -inf.

What is exact. Philox words are integer arithmetic, the uniforms are two
exact f32 operations (_u32_to_unit), rates and fitness are compared in
f32: pa, pb, the crossover mask and the mutation mask carry no rounding.
A slot that is not mutated is an f32 copy, clipped: exact.

NORMALS ARE AN ARGUMENT. On the GPU the device's own box_muller output
(philox_probe), on the CPU philox_normal4_np, so the envelope holds only
the kernel's own arithmetic on a mutated slot: span = hi - lo is one f32
subtraction whose result feeds a multiply, so no contraction can touch it
and the twin takes it as the f32 difference; step = (g * mut_scale) * span
is two f32 multiplies and v + step one add, possibly contracted with the
second multiply into an fma. First order:
    |err| <= 2 U24 |step| + U24 |v + step|  (<= 3 U24 (|v| + |step|)),
zero where the slot is not mutated. Clipping is 1-Lipschitz and keeps it.

Integer slots. rint is not continuous: a mutated integer slot is
UNDECIDABLE when the two ends of [v - env, v + env], clipped, round to
different integers, that is when the clipped value lies within the
envelope of some k + 0.5. Such a slot is held to the two candidates only.
This is a condition on the case, not a measurement: at most UNDECIDABLE_CAP
of the mutated integer slots of a case may be undecidable
(test_ga_refs_cpu.py asserts it for the reference, test_gpu_ga.py for the
device's normals). The fix-up of slot 4 is applied per candidate.
"""

from dataclasses import dataclass

import numpy as np

from ai_crypto_trader_amd.backtesting.families import get_family
from ai_crypto_trader_amd.backtesting.strategy import (
    PARAM_BOUNDS, random_population,
)
from ai_crypto_trader_amd.ops.montecarlo import _u32_to_unit, philox4x32_np
from kernel_refs import U24
from mc_refs import philox4x32_int

f32 = np.float32
f64 = np.float64
u64 = np.uint64

GEN_BITS = 20
GEN_WRAP = 1 << GEN_BITS
MAX_TOURNAMENT = 4
UNDECIDABLE_CAP = 0.01
SEED_LO = 3
SEED_HI = (1 << 32) + 9
NEVER = f32(-1e30)


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------
FAMILIES = ("vote", "grid", "dca", "syn1", "syn40")
FITNESS = ("normal", "half_tied", "all_equal", "some_neginf", "all_nan")
AXES = dict(
    family=FAMILIES,
    P=(1, 9, 255, 256, 257, 600),
    elite=(0, 1, 8, "P"),
    tournament=(1, 2, 4),
    cx_rate=(0.0, 0.5, 1.0),
    mut_rate=(0.0, 0.15, 1.0),
    gen=(0, 5, GEN_WRAP + 5),
    seed=(SEED_LO, SEED_HI),
    fitness=FITNESS,
)


@dataclass(frozen=True)
class GaCase:
    family: str             # "vote": ga_evolve_kernel, else the generic one
    P: int
    elite: object           # 0 | 1 | 8 | "P"
    tournament: int
    cx_rate: float
    mut_rate: float
    gen: int
    seed: int
    fitness: str
    mut_scale: float = 0.1

    @property
    def elite_k(self):
        return self.P if self.elite == "P" else int(self.elite)

    @property
    def fixup(self):
        return self.family == "vote"

    @property
    def id(self):
        return (f"{self.family}-P{self.P}-e{self.elite}-t{self.tournament}"
                f"-cx{self.cx_rate}-mu{self.mut_rate}-g{self.gen}"
                f"-s{self.seed}-{self.fitness}")


def _feasible(c):
    return c.elite == "P" or int(c.elite) <= c.P


def _pairwise_cases():
    """A deterministic greedy all-pairs selection over AXES: every feasible
    pair of values of two axes appears in at least one case (elite 8 does
    not go with P = 1)."""
    names = list(AXES)
    idx = [(a, b) for a in range(len(names)) for b in range(a + 1, len(names))]
    need = set()
    for a, b in idx:
        for va in AXES[names[a]]:
            for vb in AXES[names[b]]:
                if (names[a], names[b]) == ("P", "elite") and \
                        (va, vb) == (1, 8):
                    continue
                need.add((a, va, b, vb))
    rng = np.random.default_rng(20)
    out = []
    while need:
        a0, va0, b0, vb0 = min(need, key=repr)     # a still-missing pair
        best, gain = None, -1
        for _ in range(60):
            vals = [AXES[n][rng.integers(len(AXES[n]))] for n in names]
            vals[a0], vals[b0] = va0, vb0
            if not _feasible(GaCase(*vals)):
                continue
            g = sum((a, vals[a], b, vals[b]) in need for a, b in idx)
            if g > gain:
                best, gain = vals, g
        out.append(GaCase(*best))
        for a, b in idx:
            need.discard((a, best[a], b, best[b]))
    return out


# the case the project's own GA test uses: P = 300, default rates
STANDARD = GaCase("vote", 300, 8, 4, 0.5, 0.15, 0, SEED_LO, "normal")
STANDARD_GENERIC = GaCase("grid", 300, 8, 4, 0.5, 0.15, 0, SEED_LO, "normal")
# named cases the mutants are shown on (beside STANDARD)
ALL_MUTATED = GaCase("vote", 257, 1, 2, 0.5, 1.0, 5, SEED_HI, "half_tied")
HALF_BOUNDS = GaCase("syn40", 255, 0, 4, 0.5, 1.0, GEN_WRAP + 5, SEED_LO,
                     "all_equal")
NO_WINNER = GaCase("vote", 256, 8, 4, 0.5, 0.15, 0, SEED_LO, "all_nan")
NO_WINNER_GENERIC = GaCase("dca", 257, 8, 4, 0.5, 0.15, 0, SEED_LO,
                           "all_nan")
CASES = [STANDARD, STANDARD_GENERIC, ALL_MUTATED, HALF_BOUNDS, NO_WINNER,
         NO_WINNER_GENERIC] + _pairwise_cases()


def case_id(c):
    return c.id


# tests/golden/ga_children.npz: children of P = 300 (random_population
# seed 1, the families' too; standard-normal fitness of default_rng(0),
# tie-free), recorded through ga_evolve_gpu / ga_evolve_family_gpu before
# the parent fallback, the NaN rule and the stable sort existed
GOLDEN_RUNS = {
    "a": dict(elite_k=8, tournament=4, seed=3, gen=0),
    "b": dict(elite_k=1, tournament=2, seed=(1 << 32) + 9, gen=5,
              cx_rate=0.3, mut_rate=0.4),
}
GOLDEN_DEFAULTS = dict(cx_rate=0.5, mut_rate=0.15, mut_scale=0.1)


def _synthetic_bounds(n):
    """Mixed int and float slots; some int slots have half-integer bounds
    (so that clip-then-round differs from round-then-clip), some slots have
    lo != 0 (so that the span hi - lo differs from hi)."""
    rows = []
    for j in range(n):
        kind = j % 4
        if kind == 0:
            rows.append((1.5 + j, 7.5 + 2 * j, 1))
        elif kind == 1:
            rows.append((-0.25 * (j + 1), 0.75 + 0.01 * j, 0))
        elif kind == 2:
            rows.append((2 + j, 40 + j, 1))
        else:
            rows.append((10.0 + j, 10.5 + j, 0))
    return np.array(rows, f32)


def bounds_for(family):
    if family == "vote":
        return np.ascontiguousarray(PARAM_BOUNDS, dtype=f32)
    if family in ("grid", "dca"):
        return np.ascontiguousarray(get_family(family).bounds, dtype=f32)
    return _synthetic_bounds({"syn1": 1, "syn40": 40}[family])


def population_for(c):
    if c.family == "vote":
        return random_population(c.P, seed=1)
    if c.family in ("grid", "dca"):
        return np.ascontiguousarray(
            get_family(c.family).random_population(c.P, seed=1), dtype=f32)
    b = bounds_for(c.family)
    rng = np.random.default_rng([31, c.P, b.shape[0]])
    pop = rng.uniform(b[:, 0], b[:, 1], (c.P, b.shape[0])).astype(f32)
    pop = np.clip(pop, b[:, 0], b[:, 1])
    isint = b[:, 2] > 0
    pop[:, isint] = np.rint(pop[:, isint])
    return pop.astype(f32)


def fitness_for(c):
    fit = np.random.default_rng(0).standard_normal(c.P).astype(f32)
    if c.fitness == "half_tied":
        # the backtest's score of a strategy that never trades
        fit[np.random.default_rng(1).permutation(c.P)[:(c.P + 1) // 2]] = -1.0
    elif c.fitness == "all_equal":
        fit[:] = 0.25
    elif c.fitness == "some_neginf":
        fit[::3] = -np.inf
    elif c.fitness == "all_nan":
        fit[:] = np.nan
    else:
        assert c.fitness == "normal"
    return fit


def sanitize_fitness(fit):
    """What the wrappers do before sorting and launching: NaN -> -inf."""
    fit = np.asarray(fit, f32).copy()
    fit[np.isnan(fit)] = -np.inf
    return fit


def stable_order(fit):
    """Stable descending argsort of the sanitized fitness, int32."""
    return np.argsort(-sanitize_fitness(fit).astype(f64),
                      kind="stable").astype(np.int32)


def case_inputs(c):
    """-> pop (P, n) f32, fitness (P,) f32 as given, order (P,) i32,
    bounds (n, 3) f32."""
    fit = fitness_for(c)
    return population_for(c), fit, stable_order(fit), bounds_for(c.family)


def cpu_normals(seed, lo, hi):
    from ai_crypto_trader_amd.ops.montecarlo import philox_normal4_np
    return philox_normal4_np(seed, np.asarray(lo, u64), np.asarray(hi, u64))


# ---------------------------------------------------------------------------
# The twin
# ---------------------------------------------------------------------------
def counters(P, elite_k, gen, mutant=None):
    i = np.arange(elite_k, P, dtype=u64)
    g = 0 if mutant == "gen_not_in_counter" else gen & (GEN_WRAP - 1)
    return i, (i << u64(GEN_BITS)) | u64(g)


def select_parents(fitness, P, words, tournament, child, mutant=None):
    """words (n, 8) u32 -> pa, pb (n,) int64. f32 compares throughout."""
    fit = np.asarray(fitness, f32)
    n = words.shape[0]
    out = []
    for off in (0, 4):
        if mutant == "tournament_b_reuses_a":
            off = 0
        best = np.full(n, -1, np.int64)
        fbest = np.full(n, NEVER, f32)
        for k in range(tournament):
            c = (words[:, (k + off) & 7].astype(np.int64)) % P
            with np.errstate(invalid="ignore"):
                win = (fit[c] >= fbest) if mutant == "ge_instead_of_gt" \
                    else (fit[c] > fbest)
            fbest = np.where(win, fit[c], fbest)
            best = np.where(win, c, best)
        out.append(best)
    pa, pb = out
    if mutant != "no_parent_fallback":
        pa = np.where(pa < 0, child, pa)
        pb = np.where(pb < 0, child, pb)
    return pa, pb


def _rint_ends(v, env, lo, hi):
    a = np.rint(np.clip(v - env, lo, hi))
    b = np.rint(np.clip(v + env, lo, hi))
    return a, b


def evolve_twin(pop, fitness, order, bounds, *, elite_k, tournament,
                cx_rate, mut_rate, mut_scale, seed, gen, fixup, normal_fn,
                mutant=None):
    """-> dict(pa, pb, cx, mut (children only), child (P, n) f64, env
    (P, n), cands (P, n, 4) the allowed values of an integer slot, isint
    (n,), undecidable (P, n) bool, n_mut_int)."""
    pop = np.asarray(pop, f32)
    P, n = pop.shape
    b = np.asarray(bounds, f32)
    lo, hi, isint = b[:, 0].astype(f64), b[:, 1].astype(f64), b[:, 2] > 0
    span = (b[:, 1] - b[:, 0]).astype(f64)            # one f32 subtraction
    if mutant == "span_hi":
        span = hi
    child = np.empty((P, n), f64)
    env = np.zeros((P, n))
    child[:elite_k] = pop[np.asarray(order)[:elite_k]]
    i, ctr = counters(P, elite_k, gen, mutant)
    nc = i.size
    res = dict(isint=isint, n_mut_int=0)
    if nc:
        w = [np.stack(philox4x32_np(seed, ctr, np.full(nc, s, u64)), -1)
             for s in (0, 1)]
        words = np.concatenate(w, axis=-1)
        pa, pb = select_parents(fitness, P, words, tournament,
                                i.astype(np.int64), mutant)
        s0 = 1 if mutant == "stream_1_plus_j" else 2
        lo_c = np.repeat(ctr, n)
        hi_c = np.tile(np.arange(s0, s0 + n, dtype=u64), nc)
        x, y, _, _ = philox4x32_np(seed, lo_c, hi_c)
        u_cx = _u32_to_unit(x).reshape(nc, n)
        u_mut = _u32_to_unit(y).reshape(nc, n)
        g = np.asarray(normal_fn(seed, lo_c, hi_c), f32)
        g = g[:, 3 if mutant == "gy_instead_of_gx" else 2]
        g = g.astype(f64).reshape(nc, n)
        cx = u_cx < f32(cx_rate)
        if mutant == "cx_compare_flipped":
            cx = ~cx
        mut = u_mut < f32(mut_rate)
        # a missing fallback reads before the buffer: whatever lies there
        padded = np.concatenate([pop, np.full((1, n), np.nan, f32)])
        v = np.where(cx, padded[pa], padded[pb]).astype(f64)
        step = np.where(mut, g * f64(f32(mut_scale)) * span, 0.0)
        e = np.where(mut, 2 * U24 * np.abs(step) + U24 * np.abs(v + step),
                     0.0)
        v = v + step
        if mutant == "round_before_clip":
            v = np.where(isint, np.rint(v), v)
        child[elite_k:] = np.clip(v, lo, hi)
        env[elite_k:] = e
        res.update(pa=pa, pb=pb, cx=cx, mut=mut,
                   n_mut_int=int((mut & isint).sum()))
        raw = np.full((P, n), np.nan)
        raw[elite_k:] = v
    # integer slots: candidates from the two ends of the envelope
    cands = np.repeat(child[:, :, None], 4, axis=2)
    und = np.zeros((P, n), bool)
    if nc:
        a, bb = _rint_ends(raw[elite_k:], env[elite_k:], lo, hi)
        a = np.where(isint, a, child[elite_k:])
        bb = np.where(isint, bb, child[elite_k:])
        cands[elite_k:] = np.stack([a, bb, a, bb], axis=-1)
        und[elite_k:] = a != bb
        if mutant != "round_before_clip":
            child[elite_k:] = np.where(isint, np.rint(child[elite_k:]),
                                       child[elite_k:])
        if fixup and mutant != "fixup_missing":
            c3 = cands[elite_k:, 3, :][:, [0, 0, 1, 1]]
            c4 = cands[elite_k:, 4, :][:, [0, 1, 0, 1]]
            cands[elite_k:, 4, :] = np.where(c4 <= c3, c3 + 1.0, c4)
            k = child[elite_k:]
            k[:, 4] = np.where(k[:, 4] <= k[:, 3], k[:, 3] + 1.0, k[:, 4])
    res.update(child=child, env=env, cands=cands, undecidable=und)
    return res


def run_case(c, normal_fn=cpu_normals, mutant=None, fitness=None):
    pop, fit, order, bounds = case_inputs(c)
    return evolve_twin(
        pop, fit if fitness is None else fitness, order, bounds,
        elite_k=c.elite_k, tournament=c.tournament, cx_rate=c.cx_rate,
        mut_rate=c.mut_rate, mut_scale=c.mut_scale, seed=c.seed, gen=c.gen,
        fixup=c.fixup, normal_fn=normal_fn, mutant=mutant)


def undecidable_share(res):
    """Share of the mutated integer slots that are undecidable."""
    n = int(res["undecidable"].sum())
    return n, res["n_mut_int"], (n / res["n_mut_int"] if n else 0.0)


def hold(got, res, rows=None):
    """Compare a child population with the twin. -> dict(worst: largest
    |got - ref| / envelope over the mutated float slots, bad: number of
    elements outside (an integer slot not among its candidates, a float
    slot outside its envelope, an exact slot that differs), first: index
    of the first bad element or None)."""
    got = np.asarray(got, f64)
    child, env, cands = res["child"], res["env"], res["cands"]
    if rows is not None:
        child, env, cands = child[rows], env[rows], cands[rows]
    isint = res["isint"][None, :]
    ok_int = (got[:, :, None] == cands).any(axis=2)
    err = np.abs(got - child)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok_flt = np.where(env > 0, err <= env, got == child)
        frac = np.where((env > 0) & ~isint, err / env, 0.0)
    ok = np.where(isint, ok_int, ok_flt)
    frac = np.where(np.isfinite(frac), frac, np.inf)
    bad = np.argwhere(~ok)
    return dict(worst=float(frac.max()) if frac.size else 0.0,
                bad=int(bad.shape[0]),
                first=tuple(int(x) for x in bad[0]) if bad.size else None)


# ---------------------------------------------------------------------------
# An independent scalar f32 emulation of the kernel (Python integers for
# Philox, numpy f32 scalars for the arithmetic)
# ---------------------------------------------------------------------------
def _unit(word):
    return (f32(word) + f32(1.0)) * f32(2.3283064e-10)


def emulate_rows(c, rows, normal_fn=cpu_normals, fma=False):
    """The children `rows` of case c, computed one at a time the way the
    kernel's thread does. fma: contract v + t * span into one rounding."""
    pop, fit, order, bounds = case_inputs(c)
    P, n = pop.shape
    out = np.empty((len(rows), n), f32)
    ms, cxr, mur = f32(c.mut_scale), f32(c.cx_rate), f32(c.mut_rate)
    for r, i in enumerate(rows):
        if i < c.elite_k:
            out[r] = pop[order[i]]
            continue
        ctr = (i << GEN_BITS) | (c.gen & 0xFFFFF)
        rnd = philox4x32_int(c.seed, ctr, 0) + philox4x32_int(c.seed, ctr, 1)
        pa = pb = -1
        fa = fb = NEVER
        for k in range(c.tournament):
            ca = rnd[k & 7] % P
            if fit[ca] > fa:
                fa, pa = fit[ca], ca
            cb = rnd[(k + 4) & 7] % P
            if fit[cb] > fb:
                fb, pb = fit[cb], cb
        pa = i if pa < 0 else pa
        pb = i if pb < 0 else pb
        streams = np.arange(2, 2 + n, dtype=u64)
        g = np.asarray(normal_fn(c.seed, np.full(n, ctr, u64), streams),
                       f32)[:, 2]
        for j in range(n):
            x, y, _, _ = philox4x32_int(c.seed, ctr, 2 + j)
            v = pop[pa, j] if _unit(x) < cxr else pop[pb, j]
            lo, hi = bounds[j, 0], bounds[j, 1]
            if _unit(y) < mur:
                t = f32(g[j] * ms)
                span = f32(hi - lo)
                if fma:
                    v = f32(f64(v) + f64(t) * f64(span))
                else:
                    v = f32(v + f32(t * span))
            v = min(max(v, lo), hi)
            if bounds[j, 2] > 0:
                v = np.rint(v)
            out[r, j] = v
        if c.fixup and out[r, 4] <= out[r, 3]:
            out[r, 4] = out[r, 3] + f32(1.0)
    return out


def sample_rows(c, cap=48):
    """Every row of a small case; for a larger one the elite edge, the
    256-lane block edges and both ends."""
    if c.P <= cap:
        return list(range(c.P))
    pick = set(range(6)) | set(range(c.P - 6, c.P))
    for edge in (c.elite_k, 256, 512):
        pick |= {r for r in range(edge - 4, edge + 4) if 0 <= r < c.P}
    rest = [r for r in range(c.P) if r not in pick]
    pick |= set(rest[::max(len(rest) // (cap - len(pick)), 1)][:cap])
    return sorted(pick)


# ---------------------------------------------------------------------------
# Mutants: each a defect a plausible edit could introduce, with the case
# on which it must leave the envelope
# ---------------------------------------------------------------------------
MUTANT_CASES = {
    "tournament_b_reuses_a": STANDARD,
    "ge_instead_of_gt": HALF_BOUNDS,          # all fitness equal
    "cx_compare_flipped": STANDARD,
    "gy_instead_of_gx": STANDARD,
    "span_hi": STANDARD,                      # vote slots with lo != 0
    "round_before_clip": HALF_BOUNDS,         # int slots, bounds k + 0.5
    "fixup_missing": ALL_MUTATED,
    "gen_not_in_counter": ALL_MUTATED,        # gen = 5
    "stream_1_plus_j": STANDARD,
    "no_parent_fallback": NO_WINNER,
}
MUTANTS = tuple(MUTANT_CASES)
