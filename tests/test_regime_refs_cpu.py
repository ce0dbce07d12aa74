"""The regime stack on a CPU: the envelopes of regime_refs.py are reachable
(f32 emulations of the kernels sit inside them with half the f32 part) and
sharp (seeded mutants sit outside); the numpy twins of ops/regime.py equal
the existing per-symbol code; the batched model, the service's universe
detection and the per-regime trade breakdown do what they say."""

import asyncio

import numpy as np
import pytest
import torch

import regime_refs as rr
from ai_crypto_trader_amd.backtesting.engine_cpu import run_backtest_cpu
from ai_crypto_trader_amd.backtesting.evaluation import (
    StrategyEvaluationSystem, label_regimes, regime_breakdown,
)
from ai_crypto_trader_amd.backtesting.ledger import FIELDS, Ledger
from ai_crypto_trader_amd.backtesting.result_analyzer import ResultAnalyzer
from ai_crypto_trader_amd.backtesting.strategy import (
    clip_params, dict_to_params,
)
from ai_crypto_trader_amd.bus.message_bus import InProcessBus
from ai_crypto_trader_amd.bus.schema import Keys
from ai_crypto_trader_amd.config import AppConfig
from ai_crypto_trader_amd.data.synthetic import (
    candles_chl_v, generate_ohlcv,
)
from ai_crypto_trader_amd.ops.regime import (
    hmm_estep_cpu, hmm_mstep, hmm_viterbi_cpu, regime_features_cpu,
)
from ai_crypto_trader_amd.services.market_regime import (
    REGIMES, GaussianHMMBatched, GaussianHMMTorch, KMeansTorch,
    MarketRegimeService, extract_features, kmeans_many,
)

EAGER = {"entry_votes": 1, "exit_votes": 1, "stop_loss_pct": 0.004,
         "take_profit_pct": 0.006, "trailing_stop_pct": 0.003,
         "trailing_act_pct": 0.002}
FEAT_NAMES = ("ret", "vol", "slope", "rsi", "macd", "bbw")


# ---------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------
FEAT_CPU_CASES = [(2, 2 + 257, 100.0), (12, 12 + 255, 100.0),
                  (26, 26 + 256, 100.0), (32, 600, 100.0),
                  (32, 600, 6e4), (256, 256 + 257, 6e4)]


@pytest.mark.parametrize("win,T,level", FEAT_CPU_CASES)
def test_feature_emulation_inside_envelope(win, T, level):
    c = rr.feat_closes(2, T, level)
    ref, env = rr.feat_ref(c, None, win)
    emu = rr.feat_emulate(c, None, win)
    for f, name in enumerate(FEAT_NAMES):
        w = rr.worst(emu[..., f], ref[..., f], 0.5 * env[..., f])
        print(f"{name}: worst err / half envelope = {w:.3f}, envelope "
              f"{env[..., f].max():.3e} on |ref| <= "
              f"{np.abs(ref[..., f]).max():.3e}")
        assert w <= 1.0, name
    # the envelope is an f32 one: a handful of ulps of the feature's scale
    scale = np.abs(ref).max(axis=(0, 1))
    big = scale > 0
    assert (env.max(axis=(0, 1))[big] <= 1e-3 * scale[big]).all()


def test_feature_envelope_holds_level_but_raw_moments_do_not():
    """At 6e4 with 0.1 % moves the pivoted emulation stays inside; std from
    raw second moments is off by orders of magnitude more."""
    c = rr.feat_closes(1, 400, 6e4)
    ref, env = rr.feat_ref(c, None, 32)
    W = np.lib.stride_tricks.sliding_window_view(c, 32, axis=1)[:, :368]
    s1 = W.sum(-1, dtype=np.float32) / np.float32(32)
    s2 = (W * W).sum(-1, dtype=np.float32) / np.float32(32)
    raw = np.sqrt(np.maximum(s2 - s1 * s1, 0)) / s1
    assert rr.worst(raw, ref[..., 5], env[..., 5]) > 100.0


def test_log1p_emulation_figure():
    """The recorded figure behind the log1pf allowance: numpy's f32 log1p
    against f64 on the log-return arguments the feature tests use."""
    worst = 0.0
    for level, T in ((100.0, 600), (6e4, 600), (100.0, 259), (6e4, 513)):
        c = rr.feat_closes(3, T, level)
        a = ((c[:, 1:] - c[:, :-1]) / c[:, :-1]).astype(np.float32)
        want = np.log1p(a.astype(np.float64))
        nz = want != 0
        rel = np.abs(np.log1p(a).astype(np.float64) - want)[nz] \
            / np.abs(want[nz])
        worst = max(worst, float(rel.max()))
    print(f"f32 log1p emulation: {worst / rr.U24:.3f} U24")
    assert worst <= rr.LOG1P_EMU_REL


def test_feature_constant_closes_are_exact_zero():
    c = np.full((1, 100), 123.456, np.float32)
    ref, env = rr.feat_ref(c, None, 32)
    emu = rr.feat_emulate(c, None, 32)
    assert np.isfinite(emu).all()
    assert (ref == 0).all() and (emu == 0).all()
    assert env.max() <= 2 * rr.RET_EPS      # only ret = 1 / 1 - 1 is charged


@pytest.mark.parametrize("mutant", rr.FEAT_MUTANTS)
def test_feature_mutants_fall_outside(mutant):
    col = {"slope_no_win": 2, "sample_std": 5, "macd_long12": 4}[mutant]
    c = rr.feat_closes(1, 300, 100.0)
    ref, env = rr.feat_ref(c, None, 32)
    bad = rr.feat_emulate(c, None, 32, mutant=mutant)
    w = rr.worst(bad[..., col], ref[..., col], env[..., col])
    print(f"{mutant}: {w:.1f} envelopes off")
    assert w > 10.0
    if mutant == "sample_std":
        assert rr.worst(bad[..., 1], ref[..., 1], env[..., 1]) > 10.0


@pytest.mark.parametrize("win", [32, 12])
def test_features_cpu_equals_extract_features(win):
    closes = candles_chl_v(generate_ohlcv(500, 3, seed=11))[:, :, 0]
    closes = closes.astype(np.float64)
    got = regime_features_cpu(closes, None, win)
    assert got.shape == (3, 500 - win, 6)
    for s in range(3):
        want = extract_features(closes[s], win)
        np.testing.assert_allclose(got[s], want, rtol=1e-5, atol=1e-12)
    # one window, and none
    one = regime_features_cpu(closes[:, :win + 1], None, win)
    np.testing.assert_allclose(
        one[0], extract_features(closes[0, :win + 1], win), rtol=1e-5,
        atol=1e-12)
    assert one.shape == (3, 1, 6)
    assert regime_features_cpu(closes[:, :win], None, win).shape == (3, 0, 6)
    assert extract_features(closes[0, :win], win).shape == (0, 6)
    # ragged: rows past lengths - win are zero, the others unchanged
    rag = regime_features_cpu(closes, [500, win, 300], win)
    np.testing.assert_array_equal(rag[0], got[0])
    assert (rag[1] == 0).all()
    np.testing.assert_array_equal(rag[2, :300 - win], got[2, :300 - win])
    assert (rag[2, 300 - win:] == 0).all()


@pytest.mark.parametrize("win", [1, 257])
def test_features_reject_unsupported_windows(win):
    with pytest.raises(RuntimeError):
        regime_features_cpu(np.ones((1, 600)), None, win)


# ---------------------------------------------------------------------------
# E-step
# ---------------------------------------------------------------------------
ESTEP_CPU_CASES = [
    dict(T=1, K=1, F=1), dict(T=2, K=2, F=1), dict(T=3, K=3, F=6),
    dict(T=65, K=4, F=6), dict(T=257, K=8, F=8),
    dict(T=257, K=4, F=6, clamp_var=True),
    dict(T=rr.HMM_LONG_T, K=4, F=6, far=True),
]


def _case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items())


@pytest.mark.parametrize("case", ESTEP_CPU_CASES, ids=_case_id)
def test_estep_emulation_inside_envelope(case):
    case = dict(case)
    T, K, F = case.pop("T"), case.pop("K"), case.pop("F")
    inp = rr.hmm_inputs(1, T, K, F, **case)
    emu = rr.hmm_estep_emulate(inp["X"][0], inp["mu"][0], inp["var"][0],
                               inp["logA"][0], inp["logpi"][0])
    ratios = rr.estep_ratios(inp, emu)
    print({k: round(v, 3) for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 0.5, k


def test_long_case_needs_the_scaling():
    """T = 2048 with the parameters far from the data: the unscaled f32
    forward pass dies within the first steps, the scaled emulation holds
    the figures recorded in regime_refs."""
    inp = rr.hmm_inputs(1, rr.HMM_LONG_T, 4, 6, far=True)
    args = (inp["X"][0], inp["mu"][0], inp["var"][0], inp["logA"][0],
            inp["logpi"][0])
    dead = rr.forward_unscaled_f32(*args)
    free = rr.hmm_logspace_ref(inp["X"][0].astype(np.float64),
                               *rr.params_of(inp, 0))
    emu = rr.hmm_estep_emulate(*args)
    a_err = np.abs(emu["alpha"] - free["alpha"]).max()
    ll_rel = abs(float(emu["ll"]) - free["ll"]) / abs(free["ll"])
    print(f"per-step log-likelihood {free['ll'] / rr.HMM_LONG_T:.1f}; "
          f"unscaled dead at t = {dead}; alpha err {a_err:.2e}, "
          f"ll rel {ll_rel:.2e}")
    assert free["ll"] / rr.HMM_LONG_T < -15
    assert dead <= 37
    assert a_err <= rr.HMM_LONG_ALPHA_ERR
    assert ll_rel <= rr.HMM_LONG_LL_REL


@pytest.mark.parametrize("mutant", rr.ESTEP_MUTANTS)
def test_estep_mutants_fall_outside(mutant):
    far = mutant == "no_shift"
    inp = rr.hmm_inputs(1, 257, 4, 6, far=far, sep=1.0 if not far else 3.0)
    bad = rr.hmm_estep_emulate(inp["X"][0], inp["mu"][0], inp["var"][0],
                               inp["logA"][0], inp["logpi"][0],
                               mutant=mutant)
    ratios = rr.estep_ratios(inp, bad)
    key = {"no_shift": "alpha", "head_with_last": "gamma_sum_head",
           "xi_alpha_next": "xi_sum"}[mutant]
    print(f"{mutant}: {key} {ratios[key]:.1f} envelopes off")
    assert ratios[key] > 10.0


@pytest.mark.parametrize("T", [1, 2, 3, 65])
def test_estep_cpu_twin_equals_logspace_reference(T):
    """The scaled recursion of hmm_estep_cpu in f64 against the log-space
    formulation, ragged batch included."""
    inp = rr.hmm_inputs(3, T, 4, 6)
    lens = [T, max(T - 1, 1), 1]
    st = hmm_estep_cpu(inp["X"], lens, inp["mu"], inp["var"], inp["logA"],
                       inp["logpi"], want_gamma=True)
    for b, n in enumerate(lens):
        free = rr.hmm_logspace_ref(inp["X"][b, :n].astype(np.float64),
                                   *rr.params_of(inp, b))
        for k in ("ll", "gamma0", "gamma_sum", "gamma_sum_head", "xi_sum",
                  "sx", "sxx"):
            np.testing.assert_allclose(st[k][b], free[k], rtol=1e-9,
                                       atol=1e-12, err_msg=k)
        np.testing.assert_allclose(st["gamma"][b, :n], free["gamma"],
                                   rtol=1e-9, atol=1e-12)
        assert (st["gamma"][b, n:] == 0).all()
    # a length-1 sequence: xi = 0, gamma the normalised first step
    assert (st["xi_sum"][2] == 0).all()
    np.testing.assert_allclose(st["gamma"][2, 0].sum(), 1.0, rtol=1e-12)
    with pytest.raises(RuntimeError):
        hmm_estep_cpu(np.zeros((1, 4, 9)), None, np.zeros((1, 2, 9)),
                      np.ones((1, 2, 9)), np.zeros((1, 2, 2)),
                      np.zeros((1, 2)))
    with pytest.raises(RuntimeError):
        hmm_estep_cpu(np.zeros((1, 4, 2)), None, np.zeros((1, 9, 2)),
                      np.ones((1, 9, 2)), np.zeros((1, 9, 9)),
                      np.zeros((1, 9)))


def test_estep_and_mstep_reproduce_one_torch_iteration():
    """hmm_estep_cpu + hmm_mstep for B = 1 against one iteration of
    GaussianHMMTorch.fit from the same starting parameters: the structural
    check that statistics and update fit together as they do in the torch
    class. Its bounds are the torch class's own worst-case f32 drift and
    are wide; the update's formulas and constants are pinned to f64
    rounding by test_mstep_is_fit_formulas_with_their_constants.

    The torch class runs log-space f32: every la[t] / lb[t] is a sum whose
    size grows to |ll|, each of its two f32 operations per step off by
    U24 |la[t]|, so after T steps a log-posterior is off by at most
    2 U24 T |ll| from each of the two passes, r = 4 U24 T |ll| relative on
    every gamma and xi. A ratio of two such sums moves by 2 r of its size:
    mu by 2 r max|x - mu|, var by 2 r max (x - mu)^2 (plus mu's own move),
    the rows of A and pi by 2 r."""
    T, K = 64, 3
    rng = np.random.default_rng(4)
    z = (np.arange(T) // 16) % K
    X = torch.from_numpy(
        (rng.normal(size=(T, 4)) + 3.0 * z[:, None]).astype(np.float32))
    start = GaussianHMMTorch(K, iters=0, seed=2).fit(X)
    one = GaussianHMMTorch(K, iters=1, seed=2).fit(X)
    st = hmm_estep_cpu(X.numpy()[None], None, start.mu.numpy()[None],
                       start.var.numpy()[None], start.logA.numpy()[None],
                       start.logpi.numpy()[None])
    new = hmm_mstep(st)
    r = 4 * rr.U24 * T * abs(float(st["ll"][0]))
    spread = np.abs(X.numpy()[:, None, :] - new["mu"][0][None]).max()
    checks = {
        "mu": (new["mu"][0], one.mu.numpy(), 2 * r * spread),
        "var": (new["var"][0], one.var.numpy(), 6 * r * spread ** 2),
        "A": (np.exp(new["logA"][0]), one.logA.exp().numpy(), 2 * r),
        "pi": (np.exp(new["logpi"][0]), one.logpi.exp().numpy(), 2 * r),
    }
    for name, (got, want, tol) in checks.items():
        err = np.abs(got - want).max()
        print(f"{name}: err {err:.2e}, bound {tol:.2e}")
        assert err <= tol, name
    assert r < 1e-2


def test_mstep_is_fit_formulas_with_their_constants():
    """hmm_mstep on f64 statistics against GaussianHMMTorch.fit's update
    written out per sequence and state, to f64 rounding: the +1e-9 on both
    denominators, the +1e-12 inside both logs, population variance and its
    1e-6 clamp. The statistics put each constant to work: a state nobody
    visits (all sums 0), a state visited once (variance exactly 0, head
    sum 0), and ordinary ones."""
    rng = np.random.default_rng(9)
    B, K, F, T = 2, 4, 3, 50
    X = rng.normal(size=(B, T, F)) * 2.0 + 1.0
    gamma = rng.dirichlet(np.ones(K - 2), size=(B, T))        # (B, T, K-2)
    gamma = np.concatenate([gamma, np.zeros((B, T, 2))], -1)
    gamma[:, -1] = 0.0
    gamma[:, -1, K - 2] = 1.0       # state K-2: the last step only
    xi = rng.uniform(0, 1, (B, K, K)) * gamma[:, :-1].sum(1)[:, :, None]
    st = {"gamma0": gamma[:, 0], "gamma_sum": gamma.sum(1),
          "gamma_sum_head": gamma[:, :-1].sum(1), "xi_sum": xi,
          "sx": np.einsum("btk,btf->bkf", gamma, X),
          "sxx": np.einsum("btk,btf->bkf", gamma, X * X)}
    got = hmm_mstep(st)
    clamped = 0
    for b in range(B):
        for i in range(K):
            nk = gamma[b, :, i].sum() + 1e-9
            mu = (gamma[b, :, i, None] * X[b]).sum(0) / nk
            raw = (gamma[b, :, i, None] * X[b] ** 2).sum(0) / nk - mu ** 2
            clamped += int((raw < 1e-6).sum())
            np.testing.assert_allclose(got["mu"][b, i], mu, rtol=1e-12,
                                       atol=1e-15)
            np.testing.assert_allclose(got["var"][b, i],
                                       np.maximum(raw, 1e-6), rtol=1e-9,
                                       atol=0)
            head = gamma[b, :-1, i].sum()
            np.testing.assert_allclose(
                got["logA"][b, i],
                np.log(xi[b, i] / (head + 1e-9) + 1e-12), rtol=1e-12)
            np.testing.assert_allclose(
                got["logpi"][b, i], np.log(gamma[b, 0, i] + 1e-12),
                rtol=1e-12)
    assert clamped >= 2 * B * F - F         # the two thin states, clamped
    assert (got["var"] >= 1e-6).all()
    # unvisited state: log(0 / 1e-9 + 1e-12) and mu = 0 / 1e-9
    assert np.allclose(got["logA"][:, K - 1], np.log(1e-12))
    assert np.allclose(got["logpi"][:, K - 2:], np.log(1e-12))
    assert (got["mu"][:, K - 1] == 0).all()
    # torch tensors go through the same code
    tt = hmm_mstep({k: torch.from_numpy(v) for k, v in st.items()})
    for k in got:
        np.testing.assert_allclose(tt[k].numpy(), got[k], rtol=1e-12,
                                   atol=1e-15)


# ---------------------------------------------------------------------------
# Viterbi
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,T", [(1, 1), (2, 2), (2, 257), (4, 65),
                                 (4, 2048), (8, 257)])
def test_viterbi_emulation(K, T):
    F = 1 if K <= 2 else 6
    inp = rr.hmm_inputs(1, T, K, F)
    X = inp["X"][0].astype(np.float64)
    prm = rr.params_of(inp, 0)
    path, best, env = rr.viterbi_ref(X, *prm)
    emu = rr.viterbi_emulate(inp["X"][0], inp["mu"][0], inp["var"][0],
                             inp["logA"][0], inp["logpi"][0])
    gap = best - rr.path_score(emu, X, *prm)
    print(f"score gap {gap:.3e}, envelope {env:.3e}, "
          f"{int((emu != path).sum())} mismatches")
    assert -1e-9 * abs(best) <= gap <= 0.5 * env
    if K in (2, 4) and F == 6 or K == 2:
        assert (emu == path).all()
    # the numpy twin, in f64, is the reference path
    twin = hmm_viterbi_cpu(inp["X"], None, inp["mu"], inp["var"],
                           inp["logA"], inp["logpi"])
    np.testing.assert_array_equal(twin[0], path)


def test_viterbi_ties_and_mutant():
    inp = rr.hmm_inputs(1, 65, 4, 6, tie=True)
    args = (inp["X"][0], inp["mu"][0], inp["var"][0], inp["logA"][0],
            inp["logpi"][0])
    assert (rr.viterbi_emulate(*args) == 0).all()
    assert (rr.viterbi_emulate(*args, mutant="tie_high") == 3).all()
    twin = hmm_viterbi_cpu(inp["X"], None, *(inp[k] for k in (
        "mu", "var", "logA", "logpi")))
    assert (twin == 0).all()
    # ragged: -1 past the length
    rag = hmm_viterbi_cpu(np.repeat(inp["X"], 2, 0), [65, 3], *(np.repeat(
        inp[k], 2, 0) for k in ("mu", "var", "logA", "logpi")))
    assert (rag[1, :3] == 0).all() and (rag[1, 3:] == -1).all()


# ---------------------------------------------------------------------------
# the batched model
# ---------------------------------------------------------------------------
def _blobs():
    g = torch.Generator().manual_seed(3)
    shift = torch.tensor([2.0, 0.0, 0.0, 0.0])
    a = torch.randn(120, 4, generator=g) * 0.2 + shift
    b = torch.randn(120, 4, generator=g) * 0.2 - shift
    return a, b


def test_kmeans_many_equals_kmeans_torch():
    a, b = _blobs()
    X = torch.stack([torch.cat([a, b]), torch.cat([b, a])])
    lens = [240, 200]
    got = kmeans_many(X, lens, 2, 20, seed=1)
    for i, n in enumerate(lens):
        want = KMeansTorch(2, 20, seed=1).fit(X[i, :n]).centers
        np.testing.assert_allclose(got[i].numpy(), want.numpy(), rtol=1e-5,
                                   atol=1e-6)


def test_fit_many_recovers_segments_and_climbs():
    """test_regime_models_recover_structure's criterion on the batched
    model (CPU twin), two sequences of different lengths; the
    log-likelihood never falls by more than its f32 envelope."""
    a, b = _blobs()
    seq = torch.cat([a[:80], b[:80], a[80:]])
    X = torch.stack([seq, torch.cat([seq[:160], torch.zeros(40, 4)])])
    lens = torch.tensor([200, 160])
    hmm = GaussianHMMBatched(2, iters=10, seed=1).fit_many(X, lens)
    paths = hmm.predict_many(X, lens)
    for i, n in enumerate(lens.tolist()):
        p = paths[i, :n]
        s0, s1 = p[:80], p[80:160]
        assert (s0 == s0.mode().values).float().mean() > 0.9
        assert (s1 == s1.mode().values).float().mean() > 0.9
        assert int(s0.mode().values) != int(s1.mode().values)
        if n > 160:
            s2 = p[160:]
            assert int(s2.mode().values) == int(s0.mode().values)
        assert (paths[i, n:] == -1).all()
    post = hmm.posterior_many(X, lens)
    np.testing.assert_allclose(post[0].sum(-1).numpy(), 1.0, rtol=1e-6)
    assert (post[1, 160:] == 0).all()
    hist = np.stack(hmm.ll_history)                       # (iters, B)
    assert hist.shape == (10, 2)
    ll = hmm.log_likelihood(X, lens).numpy()
    for i, n in enumerate(lens.tolist()):
        prm = tuple(getattr(hmm, k)[i].numpy().astype(np.float64)
                    for k in ("mu", "var", "logA", "logpi"))
        Xi = X[i, :n].numpy().astype(np.float64)
        free = rr.hmm_logspace_ref(Xi, *prm)
        fwd = rr.estep_forward_ref(Xi, *prm, free["alpha"])
        env = fwd["term"][1].sum()
        drop = -np.diff(np.r_[hist[:, i], ll[i]]).min()
        print(f"seq {i}: ll {hist[0, i]:.2f} -> {ll[i]:.2f}, largest drop "
              f"{max(drop, 0):.2e}, envelope {env:.2e}")
        assert drop <= env
        assert ll[i] > hist[0, i]


# ---------------------------------------------------------------------------
# the service
# ---------------------------------------------------------------------------
def _universe(n=5, T=600):
    closes = candles_chl_v(generate_ohlcv(T, n, seed=31))[:, :, 0]
    return {f"S{i}USDC": closes[i, :T - 100 * (i % 2)].astype(np.float64)
            for i in range(n)}


def test_detect_many_equals_detect_for_rule():
    cfg = AppConfig()
    cfg.regime.method = "rule"
    svc = MarketRegimeService(InProcessBus(), cfg)
    uni = _universe()
    uni["SHORT"] = uni["S0USDC"][:20]
    got = svc.detect_many(uni)
    assert list(got) == list(uni)
    for sym, closes in uni.items():
        assert got[sym] == svc.detect(closes)


@pytest.mark.parametrize("method", ["hmm", "kmeans", "gmm"])
def test_detect_many_labels_every_symbol(method):
    cfg = AppConfig()
    cfg.regime.method = method
    svc = MarketRegimeService(InProcessBus(), cfg)
    uni = _universe(3, 300)
    uni["SHORT"] = uni["S0USDC"][:150]              # < 200: the rules
    got = svc.detect_many(uni)
    assert set(got) == set(uni)
    for sym, (regime, conf) in got.items():
        assert regime in REGIMES
        assert 0.0 <= conf <= 1.0
    from ai_crypto_trader_amd.services.market_regime import (
        rule_based_regime,
    )
    assert got["SHORT"] == rule_based_regime(uni["SHORT"])
    if method != "hmm":
        # the per-symbol classes on the batched features: detect's answer
        for sym in ("S0USDC", "S1USDC"):
            assert got[sym][0] == svc.detect(uni[sym])[0]


def _one_loop_pass(per_symbol):
    cfg = AppConfig()
    cfg.trading.symbols = ["S0USDC", "S1USDC"]
    cfg.regime.method = "rule"
    cfg.regime.per_symbol = per_symbol
    bus = InProcessBus()
    svc = MarketRegimeService(bus, cfg)
    uni = _universe(3, 300)
    uni["TINY"] = uni["S0USDC"][:10]
    svc.prices = {s: list(c) for s, c in uni.items()}

    async def stop(_):
        svc.running = False

    svc.sleep = stop
    svc.running = True

    async def go():
        await svc._regime_loop()
        keys = sorted(await bus.keys())
        return keys, {k: await bus.get_json(k) for k in keys}

    keys, state = asyncio.run(go())
    return svc, uni, keys, state


def test_per_symbol_off_leaves_the_bus_as_today():
    assert AppConfig().regime.per_symbol is False
    assert Keys.MARKET_REGIMES == "market_regimes"
    _, _, keys, state = _one_loop_pass(False)
    assert keys == sorted([Keys.CURRENT_MARKET_REGIME,
                           Keys.MARKET_REGIME_HISTORY])
    assert set(state[Keys.CURRENT_MARKET_REGIME]) == {
        "regime", "confidence", "volatility", "at"}


def test_per_symbol_fallback_says_so():
    """detect_many failing leaves rule-based entries marked as such; a
    missing HIP extension on a GPU device is an error, not a fallback."""
    cfg = AppConfig()
    cfg.regime.method = "hmm"
    bus = InProcessBus()
    svc = MarketRegimeService(bus, cfg)
    svc.prices = {s: list(c) for s, c in _universe(2, 300).items()}

    def boom(_):
        raise ValueError("planted")

    svc.detect_many = boom

    async def go():
        await svc._publish_per_symbol()
        return await bus.get_json(Keys.MARKET_REGIMES)

    entries = asyncio.run(go())
    assert {e["method"] for e in entries.values()} == {"rule"}
    import ai_crypto_trader_amd.ops as ops_pkg
    gpu = MarketRegimeService(InProcessBus(), cfg, device="cuda:0")
    gpu.prices = svc.prices
    saved = ops_pkg._cached_mod, ops_pkg._try_load
    ops_pkg._cached_mod, ops_pkg._try_load = None, lambda: None
    try:
        with pytest.raises(RuntimeError, match="not built"):
            asyncio.run(gpu._publish_per_symbol())
    finally:
        ops_pkg._cached_mod, ops_pkg._try_load = saved


def test_per_symbol_on_adds_market_regimes():
    svc, uni, keys, state = _one_loop_pass(True)
    assert keys == sorted([Keys.CURRENT_MARKET_REGIME,
                           Keys.MARKET_REGIME_HISTORY, Keys.MARKET_REGIMES])
    regimes = state[Keys.MARKET_REGIMES]
    assert set(regimes) == {"S0USDC", "S1USDC", "S2USDC"}   # TINY: < 64
    for sym, entry in regimes.items():
        assert set(entry) == {"regime", "confidence", "volatility", "at",
                              "method"}
        assert entry["method"] == "rule"
        assert entry["regime"] == svc.detect(
            np.asarray(uni[sym], np.float64))[0]
    # the primary symbol's entry is what the single-symbol keys carry
    primary = state[Keys.CURRENT_MARKET_REGIME]
    assert regimes["S0USDC"]["regime"] == primary["regime"]
    assert regimes["S0USDC"]["confidence"] == primary["confidence"]


# ---------------------------------------------------------------------------
# per-regime breakdown
# ---------------------------------------------------------------------------
def test_label_regimes_shape_and_causality():
    mkt = candles_chl_v(generate_ohlcv(400, 2, seed=7))
    lab = label_regimes(mkt, method="kmeans", win=32)
    assert lab.shape == (2, 400) and lab.dtype == np.int8
    assert (lab[:, :32] == -1).all()
    assert ((lab[:, 32:] >= 0) & (lab[:, 32:] < len(REGIMES))).all()
    # alignment: candle win + i carries the regime of the cluster of feature
    # row i, whose window closes[i:i + win] ends at candle win + i - 1
    from ai_crypto_trader_amd.services.market_regime import (
        label_clusters, standardize_many,
    )
    for s in range(2):
        feats = extract_features(mkt[s, :, 0].astype(np.float64), 32)
        X = torch.from_numpy(feats)[None]
        Xn = standardize_many(X, torch.tensor([len(feats)]))[0]
        assign = KMeansTorch(4, seed=0).fit(Xn).predict(Xn).numpy()
        names = label_clusters(feats, assign, 4)
        want = np.asarray([REGIMES.index(names[c]) for c in assign])
        assert len(np.unique(want)) > 1
        assert (want[1:] != want[:-1]).sum() > 5     # a shift would show
        np.testing.assert_array_equal(lab[s, 32:], want)
    # the last close is in no window at all
    bumped = mkt.copy()
    bumped[:, -1, 0] *= 1.5
    np.testing.assert_array_equal(
        label_regimes(bumped, method="kmeans", win=32), lab)
    with pytest.raises(ValueError):
        label_regimes(mkt[:, :40], win=32)


def test_evaluate_by_regime_on_the_cpu_twin(small_market):
    mkt = np.ascontiguousarray(small_market[:2, :700])
    sys_ = StrategyEvaluationSystem("cpu")
    table = sys_.evaluate_by_regime(mkt, EAGER, method="hmm")
    assert list(table) == [*REGIMES, "unlabelled"]
    vec = clip_params(dict_to_params(EAGER)[None])
    led = run_backtest_cpu(mkt, vec, record_trades=True)
    closed = int(sum((led.exit_t[0, s, :led.n_kept(0, s)] >= 0).sum()
                     for s in range(2)))
    assert closed > 10
    assert sum(r["n_trades"] for r in table.values()) == closed
    assert sum(r["share_of_candles"] for r in table.values()) \
        == pytest.approx(1.0, abs=1e-12)
    assert table["unlabelled"]["share_of_candles"] \
        == pytest.approx(32 / 700)
    total = sum(float(led.pnl[0, s, :led.n_kept(0, s)][
        led.exit_t[0, s, :led.n_kept(0, s)] >= 0].astype(np.float64).sum())
        for s in range(2))
    assert sum(r["pnl"] for r in table.values()) == pytest.approx(total)


def test_regime_breakdown_by_hand():
    """One strategy, two symbols, hand-built labels and ledger."""
    labels = np.full((2, 10), -1, np.int8)
    labels[0, 3:] = [0, 0, 1, 1, 2, 2, 3]          # bull bull bear bear ...
    labels[1, 3:] = [1, 1, 1, 1, 1, 1, 1]
    cap = 4
    ints = {f: np.full((1, 2, cap), -1, np.int32)
            for f in ("entry_t", "exit_t", "reason")}
    flts = {f: np.zeros((1, 2, cap), np.float32)
            for f in FIELDS if f not in ints}
    # symbol 0: entry 1 (unlabelled) +2, entry 3 (bull) -1, entry 5 (bear)
    # +4, entry 9 (volatile) still open
    ints["entry_t"][0, 0] = [1, 3, 5, 9]
    ints["exit_t"][0, 0] = [2, 4, 6, -1]
    ints["reason"][0, 0] = [2, 1, 3, 0]
    flts["pnl"][0, 0] = [2.0, -1.0, 4.0, 0.0]
    # symbol 1: entry 4 (bear) +1, entry 6 (bear) -3
    ints["entry_t"][0, 1, :2] = [4, 6]
    ints["exit_t"][0, 1, :2] = [5, 8]
    ints["reason"][0, 1, :2] = [2, 1]
    flts["pnl"][0, 1, :2] = [1.0, -3.0]
    led = Ledger(np.zeros((1, 2, 1), np.float32),
                 np.asarray([[4, 2]], np.int32),
                 *(ints[f] if f in ints else flts[f] for f in FIELDS),
                 np.zeros((1, 2, 10), np.float32), 1)
    got = regime_breakdown(led, labels)
    want = {
        "bull": dict(n_trades=1, win_rate=0.0, pnl=-1.0, avg_pnl=-1.0,
                     share_of_candles=2 / 20),
        "bear": dict(n_trades=3, win_rate=2 / 3, pnl=2.0, avg_pnl=2 / 3,
                     share_of_candles=9 / 20),
        "ranging": dict(n_trades=0, win_rate=0.0, pnl=0.0, avg_pnl=0.0,
                        share_of_candles=2 / 20),
        "volatile": dict(n_trades=0, win_rate=0.0, pnl=0.0, avg_pnl=0.0,
                         share_of_candles=1 / 20),
        "unlabelled": dict(n_trades=1, win_rate=1.0, pnl=2.0, avg_pnl=2.0,
                           share_of_candles=6 / 20),
    }
    assert list(got) == list(want)
    for name in want:
        assert got[name] == pytest.approx(want[name]), name


def _cli(tmp_path, *extra):
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    return subprocess.run(
        [sys.executable, str(root / "run_backtest.py"), "--data-dir",
         str(tmp_path), "backtest", "--symbol", "BTCUSDC", "--cpu",
         "--params", json.dumps(EAGER), *extra],
        capture_output=True, text=True, cwd=tmp_path)


def test_cli_by_regime(tmp_path):
    """`backtest --trades --by-regime` prints one row per regime whose
    counts add up to the closed trades; without --trades it is refused,
    and a history too short to label ends with a message, not a trace."""
    r = _cli(tmp_path, "--candles", "700", "--trades", "--by-regime")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    head = next(i for i, ln in enumerate(lines)
                if ln.startswith("regime at entry"))
    rows = [ln.split() for ln in lines[head + 1:head + 6]]
    assert [row[0] for row in rows] == [*REGIMES, "unlabelled"]
    closed = next(int(ln.split()[1]) for ln in lines
                  if ln.startswith("closed"))
    assert sum(int(row[1]) for row in rows) == closed > 0
    bad = _cli(tmp_path, "--candles", "700", "--by-regime")
    assert bad.returncode == 2 and "--trades" in bad.stderr
    short = _cli(tmp_path, "--candles", "40", "--trades", "--by-regime")
    assert short.returncode != 0
    assert "--by-regime:" in short.stderr
    assert "Traceback" not in short.stderr


def test_trade_analysis_by_regime(tmp_path):
    ra = ResultAnalyzer(str(tmp_path))
    trades = [
        dict(reason="take_profit", pnl=2.0, duration=3),
        dict(reason="stop_loss", pnl=-1.0, duration=2),
        dict(reason="signal", pnl=0.5, duration=5),
        dict(reason="open", pnl=0.0, duration=-8),
    ]
    stats = {"n_trades": 3, "trades": trades}
    plain = ra.trade_analysis(stats)
    assert set(plain) == {
        "n_trades", "win_rate", "profit_factor", "expectancy_pct",
        "max_drawdown_pct", "n_closed", "n_open", "by_reason",
        "realized_pnl", "mean_duration", "median_duration", "avg_win",
        "avg_loss", "expectancy"}
    assert set(ra.trade_analysis({"n_trades": 3})) == {
        "n_trades", "win_rate", "profit_factor", "expectancy_pct",
        "max_drawdown_pct"}
    stats["regime_at_entry"] = ["bull", "bull", "bear", "bear"]
    with_regime = ra.trade_analysis(stats)
    assert set(with_regime) == set(plain) | {"by_regime"}
    assert {k: with_regime[k] for k in plain} == plain
    assert with_regime["by_regime"] == {
        "bull": {"count": 2, "pnl": 1.0, "win_rate": 0.5},
        "bear": {"count": 1, "pnl": 0.5, "win_rate": 1.0},
    }
