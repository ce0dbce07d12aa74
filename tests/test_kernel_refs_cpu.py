"""The envelopes of tests/kernel_refs.py, validated without a GPU.

For every case the GPU tests run, an emulation of the kernel's arithmetic
(f32 accumulation in the kernel's order, bf16 rounding at its rounding
points) has to sit inside the envelope with at least 2x room: the
tolerance is reachable by a correct kernel. Seeded mutants (the defects the
GPU tests exist to catch) have to sit outside it. This is where the
constants C_FWD, C_BWD and the lagged-correlation figures come from.
"""

import numpy as np
import pytest

import kernel_refs as kr

ROOM = 0.5      # emulation error / envelope


# --- covariance -----------------------------------------------------------

def test_cov_geometry_and_k():
    assert kr.cov_geometry(2) == (1, 1, 1)
    assert kr.cov_geometry(65) == (2, 2, 1)
    assert kr.cov_geometry(64 * 512 + 1) == (513, 512, 2)
    assert kr.cov_k(1037) == 64 + 1 + 17 + 4
    assert kr.cov_k(64 * 512 + 1) == 128 + 2 + 512 + 4


@pytest.mark.parametrize("T", kr.COV_TS)
@pytest.mark.parametrize("N", kr.COV_NS)
def test_cov_emulation_inside_envelope(N, T):
    X = kr.cov_inputs(T, N)
    ratio = kr.worst_ratio(kr.cov_emulate(X), kr.cov_ref(X),
                           kr.cov_envelope(X))
    assert ratio <= ROOM, ratio


@pytest.mark.parametrize("T", [65, 1037])
def test_cov_mutant_sx_double_counted(T):
    """The defect at N = 48: threads 240..255 add rows a second time."""
    X = kr.cov_inputs(T, 48)
    ref, tol = kr.cov_ref(X), kr.cov_envelope(X)
    assert kr.worst_ratio(kr.cov_emulate(X, double_count=True), ref,
                          tol) > 1.0
    # where N divides 256 the same loop is exact: nothing to double
    X = kr.cov_inputs(T, 32)
    np.testing.assert_array_equal(kr.cov_emulate(X, double_count=True),
                                  kr.cov_emulate(X))


@pytest.mark.parametrize("N", kr.COV_NS)
def test_cov_mutant_mean_term_dropped(N):
    X = kr.cov_inputs(1037, N)
    got = kr.cov_emulate(X, mean_term=False)
    assert kr.worst_ratio(got, kr.cov_ref(X), kr.cov_envelope(X)) > 1.0


def test_cov_envelope_sees_what_centred_data_hide():
    """On zero-mean data (the older GPU tests) the whole mean term is
    about 1/T of the result, so dropping it passes rtol = 1e-3; the
    envelope on non-centred data is what rejects it."""
    rng = np.random.default_rng(6)
    X = (rng.standard_normal((1037, 16)) * 0.02).astype(np.float32)
    np.testing.assert_allclose(kr.cov_emulate(X, mean_term=False),
                               kr.cov_ref(X), rtol=1e-3, atol=1e-6)


def test_cov_cpu_paths_48_columns():
    """cov_cpu, and PortfolioRiskService.compute_cov (which takes the CPU
    path on a machine without a GPU and the kernel with one), against
    np.cov on non-centred 48-column data."""
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.ops.covar import cov_cpu
    from ai_crypto_trader_amd.services.portfolio_risk import (
        PortfolioRiskService,
    )

    X = kr.cov_inputs(1037, 48)
    ref, tol = kr.cov_ref(X), kr.cov_envelope(X)
    svc = PortfolioRiskService(InProcessBus(), AppConfig())
    for got in (cov_cpu(X), svc.compute_cov(X)):
        assert got.shape == (48, 48)
        assert kr.worst_ratio(got, ref, tol) <= 1.0


# --- attention ------------------------------------------------------------

@pytest.mark.parametrize("case", kr.ATT_FWD_CASES, ids=kr.attn_case_id)
def test_attn_fwd_emulation_inside_envelope(case):
    Q, K, V, dO, scale = kr.attn_case(case)
    S = case[1]
    ref = kr.attn_ref(Q, K, V, dO, scale)
    emu = kr.attn_emulate(Q, K, V, dO, scale)
    assert kr.worst_ratio(emu["O"], ref["O"], ref["tol_O"]) <= ROOM
    assert kr.worst_ratio(emu["P"][:, :S, :S], ref["P"],
                          ref["tol_P"]) <= ROOM
    assert not emu["P"][:, :S, S:].any()
    rows = emu["P"][:, :S].astype(np.float64).sum(axis=-1)
    assert np.abs(rows - 1.0).max() <= ROOM * 64 * 2.0 ** -9
    if case[4]:                     # the max-subtraction case is what it says
        logits = scale * Q.astype(np.float64) @ K.astype(
            np.float64).transpose(0, 2, 1)
        assert 40.0 < np.abs(logits).max() < 60.0


@pytest.mark.parametrize("case", kr.ATT_BWD_CASES, ids=kr.attn_case_id)
def test_attn_bwd_emulation_inside_envelope(case):
    Q, K, V, dO, scale = kr.attn_case(case, backward=True)
    ref = kr.attn_ref(Q, K, V, dO, scale)
    emu = kr.attn_emulate(Q, K, V, dO, scale)
    for name in ("dQ", "dK", "dV"):
        assert kr.worst_ratio(emu[name], ref[name],
                              ref["tol_" + name]) <= ROOM, name
        # well-conditioned inputs: the bound means something
        assert kr.normwise(ref["tol_" + name],
                           ref[name]) <= kr.ATT_NORMWISE_MAX, name
    if case[1] == 1:                # one key: P = 1, dS = dQ = dK = 0
        assert not ref["dQ"].any() and not emu["dQ"].any()
        assert not ref["dK"].any() and not emu["dK"].any()


def test_attn_envelope_tighter_than_old_atol():
    """On the inputs of test_attn_fwd_matches_sdpa, whose allowance is
    3e-2 + 3e-2 |O| per element, the envelope is three times tighter on
    the median element and at least 1.75 times on every one (measured:
    3.1 and 1.77). With bf16's unit roundoff at 2^-8 and two roundings it
    cannot be much tighter than that and still hold a correct kernel."""
    rng = np.random.default_rng(7)
    for S, D in ((60, 16), (64, 32), (33, 64)):
        Q = kr.bf16_round(rng.standard_normal((32, S, D)))
        K = kr.bf16_round(rng.standard_normal((32, S, D)) * 0.7 + 0.1)
        V = kr.bf16_round(rng.standard_normal((32, S, D)))
        ref = kr.attn_ref(Q, K, V, V, kr.attn_scale(D))
        gain = kr.ATT_OLD_ATOL * (1.0 + np.abs(ref["O"])) / ref["tol_O"]
        assert gain.min() >= 1.75
        assert np.median(gain) >= 3.0


def _mutant_ratios(D, mutant, backward):
    case = (kr.ATT_BH, 60, D, None, None)
    Q, K, V, dO, scale = kr.attn_case(case, backward=backward)
    ref = kr.attn_ref(Q, K, V, dO, scale)
    emu = kr.attn_emulate(Q, K, V, dO, scale, mutant=mutant)
    return {n: kr.worst_ratio(emu[n], ref[n], ref["tol_" + n])
            for n in ("O", "dQ", "dK", "dV")}


@pytest.mark.parametrize("D", kr.ATT_DS)
@pytest.mark.parametrize("mutant,backward,caught", [
    ("key_off16", False, ("O",)),
    ("mask_weight", False, ("O",)),
    ("key_off16", True, ("dQ", "dK", "dV")),
    ("mask_weight", True, ("dQ", "dK", "dV")),
    ("no_scale_ds", True, ("dQ", "dK")),
    ("no_rowsum", True, ("dQ", "dK")),
    ("dk_no_transpose", True, ("dK",)),
])
def test_attn_mutants_outside_envelope(D, mutant, backward, caught):
    r = _mutant_ratios(D, mutant, backward)
    for name in caught:
        assert r[name] > 1.0, (name, r[name])


# --- lagged correlation ---------------------------------------------------

@pytest.mark.parametrize("mean,std,figure", kr.LAG_LEVELS)
def test_lag_level_figures(mean, std, figure):
    """The figures next to LAG_LEVELS are what the pivot-centred emulation
    achieves; the uncentred formula misses 4x the figure at both levels."""
    a, b = kr.lag_inputs(4000, mean, std)
    ref = kr.lagged_pearson_ref(a, b, 24)
    centred = np.abs(kr.lagged_corr_emulate(a, b, 24) - ref).max()
    raw = np.abs(kr.lagged_corr_emulate(a, b, 24, pivot=False) - ref).max()
    assert figure / 2 <= centred <= figure
    assert raw > 4 * figure


def test_lag_ref_matches_library_reference():
    from ai_crypto_trader_amd.ops.social_corr import lagged_pearson_cpu
    for n in kr.LAG_NS:
        a, b = kr.lag_inputs(n)
        np.testing.assert_allclose(kr.lagged_pearson_ref(a, b, 24),
                                   lagged_pearson_cpu(a, b, 24),
                                   rtol=0, atol=2 * kr.LAG_ULP)


def test_lag_short_windows_are_zero():
    a, b = kr.lag_inputs(5)
    for f in (kr.lagged_pearson_ref, kr.lagged_corr_emulate):
        out = f(a, b, 4)            # lags +-3, +-4 leave m < 3
        assert not out[[0, 1, 7, 8]].any()
        assert out[2:7].all()


def test_lag_tolerances_are_small():
    """Every tolerance the GPU test uses is the emulation's, times 4: a
    few ulp of the f32 result, nowhere near the old atol = 1e-4."""
    for n in kr.LAG_NS:
        for L in kr.LAG_MAX_LAGS:
            a, b = kr.lag_inputs(n)
            assert kr.lag_tolerance(a, b, L) <= 2e-6
    a, b = kr.lag_inputs(4000)
    assert kr.lag_tolerance(kr.ranks(a), kr.ranks(b), 24) <= 2e-6


# --- volume histogram -----------------------------------------------------

@pytest.mark.parametrize("n_bins", kr.VP_BINS)
def test_vp_ref_edges(n_bins):
    c = kr.vp_inputs(3, 257, flat_sym=1, top_sym=2)
    hist, tol, updown, tol_all, b = kr.vp_ref(c, n_bins)
    assert np.isfinite(hist).all() and b.min() >= 0 and b.max() < n_bins
    vol = c[..., 3].astype(np.float64)
    np.testing.assert_allclose(hist.sum(axis=1), vol.sum(axis=1),
                               rtol=1e-12)
    np.testing.assert_allclose(updown.sum(axis=1), vol[:, 1:].sum(axis=1),
                               rtol=1e-12)
    assert (b[1] == 0).all()                    # flat prices: one bin
    assert b[2, 257 // 2] == n_bins - 1         # close on the maximum
    assert (tol >= 0).all() and (tol[hist > 0] > 0).all()


# --- indicators -----------------------------------------------------------

def test_ind_edge_rows():
    assert kr.ind_edge_rows(2047).tolist() == [2046]
    assert kr.ind_edge_rows(2048).tolist() == [2046, 2047]
    assert kr.ind_edge_rows(2049).tolist() == [2046, 2047, 2048]
    assert kr.ind_edge_rows(4097).tolist() == [
        2046, 2047, 2048, 2049, 2050, 4094, 4095, 4096]
    assert kr.ind_edge_rows(20).size == 0
