"""tests/ga_refs.py checked on a CPU: an independent scalar f32 emulation
of the evolve kernels sits inside the twin's envelope on every case (plain
and fma-contracted), every seeded mutant leaves it on its named case, the
undecidable cap holds for the reference on every case, the two tournaments
behave as independent draws for tournament 1, 2 and 4 (and stop doing so
above 4, which is why the wrappers refuse it), and the argument checks
raise before anything is launched."""

import dataclasses

import numpy as np
import pytest

import ga_refs as gr

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def refs():
    return {c.id: gr.run_case(c) for c in gr.CASES}


def test_every_axis_value_appears_in_a_case():
    for axis, values in gr.AXES.items():
        for v in values:
            assert any(getattr(c, axis) == v for c in gr.CASES), (axis, v)
    assert all(0 <= c.elite_k <= c.P for c in gr.CASES)
    assert len({c.id for c in gr.CASES}) == len(gr.CASES)
    # every pair of values of two axes too (elite 8 cannot go with P = 1)
    names = list(gr.AXES)
    for a in names:
        for b in names:
            if a >= b:
                continue
            for va in gr.AXES[a]:
                for vb in gr.AXES[b]:
                    if {a, b} == {"P", "elite"} and (va, vb) in ((1, 8),
                                                                 (8, 1)):
                        continue
                    assert any(getattr(c, a) == va and getattr(c, b) == vb
                               for c in gr.CASES), (a, va, b, vb)


@pytest.mark.parametrize("c", gr.CASES, ids=gr.case_id)
def test_f32_emulation_inside_envelope(refs, c):
    res = refs[c.id]
    rows = gr.sample_rows(c)
    worst = 0.0
    for fma in (False, True):
        got = gr.emulate_rows(c, rows, fma=fma)
        h = gr.hold(got, res, rows=rows)
        assert h["bad"] == 0, (c.id, fma, h)
        worst = max(worst, h["worst"])
    assert worst <= 1.0
    print(f"{c.id}: f32 emulation at {worst:.3g} of the envelope")


@pytest.mark.parametrize("c", gr.CASES, ids=gr.case_id)
def test_undecidable_cap_holds_for_the_reference(refs, c):
    n, total, share = gr.undecidable_share(refs[c.id])
    assert share <= gr.UNDECIDABLE_CAP, (c.id, n, total)


def test_standard_case_is_fully_decidable(refs):
    n, total, _ = gr.undecidable_share(refs[gr.STANDARD.id])
    assert n == 0 and total > 200, (n, total)


def test_envelope_is_zero_where_nothing_is_computed(refs):
    """Elite rows and slots that are not mutated are copies: no envelope.
    A mutated slot has a few ulps of the bounds' magnitude at most (the
    Box-Muller radius of an f32 uniform is below 6.7)."""
    for c in gr.CASES:
        res = refs[c.id]
        assert (res["env"][:c.elite_k] == 0).all()
        if "mut" not in res:
            continue
        env = res["env"][c.elite_k:]
        assert (env[~res["mut"]] == 0).all()
        assert (env[res["mut"]] > 0).all()
        b = np.abs(gr.bounds_for(c.family).astype(np.float64))
        reach = b[:, :2].max(axis=1) + 6.7 * c.mut_scale * (b[:, 0] + b[:, 1])
        assert (env <= 3 * gr.U24 * reach).all(), c.id


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_mutant_rejected(refs, mutant):
    c = gr.MUTANT_CASES[mutant]
    got = gr.run_case(c, mutant=mutant)["child"]
    h = gr.hold(got, refs[c.id])
    assert h["bad"] > 0, (mutant, c.id)
    print(f"{mutant}: {h['bad']} elements outside on {c.id}")


def test_generation_wraps_at_2_20(refs):
    """Only the low 20 bits of gen enter the counter."""
    seen = 0
    for c in gr.CASES:
        if c.gen != gr.GEN_WRAP + 5 or c.elite_k == c.P:
            continue
        low = gr.run_case(dataclasses.replace(c, gen=5))
        np.testing.assert_array_equal(low["child"], refs[c.id]["child"])
        if c.P > 8 and c.tournament > 1 and c.fitness in ("normal",
                                                          "half_tied"):
            other = gr.run_case(dataclasses.replace(c, gen=6))
            assert (other["pa"] != refs[c.id]["pa"]).any()
            seen += 1
    assert seen


def test_nan_fitness_counts_as_minus_inf(refs):
    """What the wrappers hand to the kernel (NaN -> -inf) gives the same
    children as the raw NaN: neither ever wins a tournament, the child's
    own slot is the fallback parent, and a stable sort ranks them last."""
    for c in (gr.NO_WINNER, gr.NO_WINNER_GENERIC):
        pop, fit, order, _ = gr.case_inputs(c)
        assert np.isnan(fit).all()
        np.testing.assert_array_equal(order, np.arange(c.P))
        res = refs[c.id]
        i = np.arange(c.elite_k, c.P)
        np.testing.assert_array_equal(res["pa"], i)
        np.testing.assert_array_equal(res["pb"], i)
        clean = gr.run_case(c, fitness=gr.sanitize_fitness(fit))
        np.testing.assert_array_equal(clean["child"], res["child"])
    fit = np.array([0.5, np.nan, 2.0, -np.inf, 2.0, np.nan], np.float32)
    np.testing.assert_array_equal(gr.stable_order(fit), [2, 4, 0, 1, 3, 5])


def test_twin_agrees_with_recorded_children():
    """The recorded children of the real kernels (tests/golden), against
    the twin on numpy normals: everything the twin calls exact, elites,
    parents through every slot that is not mutated, must match bit for
    bit. (The mutated slots need the device's own normals: the GPU test
    holds them.)"""
    from pathlib import Path

    g = np.load(Path(__file__).parent / "golden" / "ga_children.npz")
    seen = 0
    for tag, kw in gr.GOLDEN_RUNS.items():
        kw = {**gr.GOLDEN_DEFAULTS, **kw}
        for fam in ("vote", "grid", "dca"):
            pop, got = g[f"{fam}_pop"], g[f"{fam}_child_{tag}"]
            b = gr.bounds_for(fam)
            res = gr.evolve_twin(
                pop, g["fitness"], gr.stable_order(g["fitness"]), b,
                fixup=fam == "vote", normal_fn=gr.cpu_normals, **kw)
            exact = res["env"] == 0
            if fam == "vote":       # the fix-up couples slot 4 to slot 3
                exact[:, 4] &= exact[:, 3]
            np.testing.assert_array_equal(got[exact], res["child"][exact])
            seen += int(exact[kw["elite_k"]:].sum())
    assert seen > 10000


def _tournament_stats(P, tournament, n_child=20000):
    """pa == pb share and the mean fitness rank of parent A and B over
    n_child children (child indices beyond P only feed the counter)."""
    fit = np.random.default_rng(5).standard_normal(P).astype(np.float32)
    rank = np.empty(P, np.int64)
    rank[np.argsort(-fit, kind="stable")] = np.arange(P)
    i = np.arange(n_child, dtype=np.uint64)
    ctr = (i << np.uint64(20)) | np.uint64(3)
    words = np.concatenate(
        [np.stack(gr.philox4x32_np(11, ctr, np.full(n_child, s, np.uint64)),
                  -1) for s in (0, 1)], axis=-1)
    pa, pb = gr.select_parents(fit, P, words, tournament,
                               i.astype(np.int64) % P)
    return float((pa == pb).mean()), rank[pa].mean(), rank[pb].mean()


@pytest.mark.parametrize("tournament", [1, 2, 4])
def test_tournaments_are_independent_up_to_four(tournament):
    """Two independent tournaments of k draws with replacement from P:
    the best rank of one has P(rank >= r) = (1 - r / P)^k, which gives
    p_r = P(rank == r), P(pa == pb) = sum_r p_r^2 and
    E[rank] = sum_r r p_r; the measured share and means over n children
    must sit within five standard errors."""
    P, n = 300, 20000
    k = tournament
    r = np.arange(P + 1)
    surv = (1 - r / P) ** k                   # P(best rank >= r)
    p = surv[:-1] - surv[1:]
    share_exp = float((p ** 2).sum())
    mean_exp = float((np.arange(P) * p).sum())
    var = float((np.arange(P) ** 2 * p).sum()) - mean_exp ** 2
    share, ma, mb = _tournament_stats(P, k, n)
    se_share = np.sqrt(share_exp * (1 - share_exp) / n)
    se_mean = np.sqrt(var / n)
    print(f"tournament {k}: pa == pb {share:.4f} (independent: "
          f"{share_exp:.4f}), mean ranks {ma:.1f} {mb:.1f} "
          f"(independent: {mean_exp:.1f})")
    assert abs(share - share_exp) <= 5 * se_share
    assert abs(ma - mean_exp) <= 5 * se_mean
    assert abs(mb - mean_exp) <= 5 * se_mean


def test_tournaments_share_draws_above_four():
    """The hazard the limit exists for: at 5 the two tournaments overlap,
    at 8 they are one and the same."""
    s4, _, _ = _tournament_stats(300, 4)
    s5, _, _ = _tournament_stats(300, 5)
    s8, _, _ = _tournament_stats(300, 8)
    assert s4 < 0.02 and s5 > 0.15 and s8 == 1.0, (s4, s5, s8)


@pytest.mark.parametrize("tournament", [0, 5, 8, -1])
def test_tournament_outside_1_to_4_is_refused(tournament):
    from ai_crypto_trader_amd.backtesting.ga_engine import GAEngine
    from ai_crypto_trader_amd.ops.ga import check_tournament

    with pytest.raises(ValueError, match="eight Philox words"):
        check_tournament(tournament)
    candles = np.ones((1, 64, 4), np.float32)
    with pytest.raises(ValueError, match="eight Philox words"):
        GAEngine(candles, pop_per_rank=8, tournament=tournament)
    for ok in (1, 4):
        assert check_tournament(ok) == ok


def test_wrapper_argument_checks_raise_before_any_launch():
    from ai_crypto_trader_amd.ops.ga import (
        ga_evolve_family_gpu, ga_evolve_gpu,
    )

    P, n = 16, 19
    pop, fit = torch.zeros(P, n), torch.zeros(P)
    b = torch.zeros(n, 3)
    bad = [
        dict(pop=pop.double()), dict(fit=fit.double()), dict(b=b.double()),
        dict(fit=fit[:-1]), dict(b=b[:-1]), dict(pop=pop[0]),
        dict(elite_k=-1), dict(elite_k=P + 1), dict(tournament=5),
        dict(tournament=0), dict(),       # last: host tensors
    ]
    for kw in bad:
        a = dict(pop=pop, fit=fit, b=b, elite_k=2, tournament=4)
        a.update(kw)
        with pytest.raises(ValueError):
            ga_evolve_family_gpu(a["pop"], a["fit"], a["b"],
                                 elite_k=a["elite_k"],
                                 tournament=a["tournament"])
        with pytest.raises(ValueError):
            ga_evolve_gpu(a["pop"], a["fit"], bounds_t=a["b"],
                          elite_k=a["elite_k"], tournament=a["tournament"])
    with pytest.raises(ValueError, match="19 slots"):
        ga_evolve_gpu(torch.zeros(P, 5), fit, bounds_t=torch.zeros(5, 3))
