"""cov, lagged_corr, vp_hist and indicators against f64 references, inside
the envelopes derived in tests/kernel_refs.py (validated on a CPU by
test_kernel_refs_cpu.py). Every test prints its figure before asserting.

What each is there to catch:
  cov            a row summed twice or not at all in Sx or Sxy at any of the
                 four N (N = 48 does not tile 256 threads), a wrong mean
                 term in the finalize step, a lost tail tile or grid-stride
                 wrap: visible because the data are not centred
  lagged_corr    cancellation in the raw f32 moments at price levels, the
                 tail of the strided loop at n around the block size, short
                 windows, constant input, the wrapper's truncation/dtypes
  vp_hist        a candle in the wrong bin (same f32 binning as the kernel,
                 so no allowance for one), lost or doubled volume at T
                 around the block size, flat prices, a close on the maximum
  indicators     a warm-up or off-by-one fault at the 2048-candle chunk edge
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# --- covariance -----------------------------------------------------------

@pytest.mark.parametrize("T", kr.COV_TS)
@pytest.mark.parametrize("N", kr.COV_NS)
def test_cov_inside_envelope(dev, N, T):
    from ai_crypto_trader_amd.ops.covar import cov_gpu

    X = kr.cov_inputs(T, N)
    got = cov_gpu(torch.from_numpy(X).to(dev))
    torch.cuda.synchronize()
    ratio = kr.worst_ratio(got.cpu().numpy(), kr.cov_ref(X),
                           kr.cov_envelope(X))
    print(f"cov N={N} T={T} K={kr.cov_k(T)}: error/envelope {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("N", kr.COV_BAD_NS)
def test_cov_rejects_unsupported_n(dev, N):
    from ai_crypto_trader_amd.ops.covar import cov_gpu

    X = torch.from_numpy(kr.cov_inputs(65, N)).to(dev)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        cov_gpu(X)
    torch.cuda.synchronize()        # nothing was launched, nothing pending


def test_cov_service_48_symbols(dev):
    """A 48-symbol portfolio reaches the kernel through the risk service."""
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.services.portfolio_risk import (
        PortfolioRiskService,
    )

    X = kr.cov_inputs(1037, 48)
    svc = PortfolioRiskService(InProcessBus(), AppConfig())
    ratio = kr.worst_ratio(svc.compute_cov(X), kr.cov_ref(X),
                           kr.cov_envelope(X))
    print(f"compute_cov 48 symbols: error/envelope {ratio:.3g}")
    assert ratio <= 1.0


# --- lagged correlation ---------------------------------------------------

def _lagged(dev, a, b, max_lag):
    from ai_crypto_trader_amd.ops.social_corr import lagged_corr_gpu

    got = lagged_corr_gpu(torch.from_numpy(a).to(dev),
                          torch.from_numpy(b).to(dev), max_lag)
    torch.cuda.synchronize()
    return got.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("max_lag", kr.LAG_MAX_LAGS)
@pytest.mark.parametrize("n", kr.LAG_NS)
def test_lagged_corr_inside_envelope(dev, n, max_lag):
    a, b = kr.lag_inputs(n)
    ref = kr.lagged_pearson_ref(a, b, max_lag)
    tol = kr.lag_tolerance(a, b, max_lag)
    got = _lagged(dev, a, b, max_lag)
    err = np.abs(got - ref).max()
    print(f"lagged_corr n={n} L={max_lag}: error {err:.3g} tol {tol:.3g}")
    assert err <= tol
    short = n - np.abs(np.arange(-max_lag, max_lag + 1)) < 3
    assert not got[short].any()     # n = 3, L = 24: every lag but 0
    if n == 3 and max_lag == 24:
        assert short.sum() == 48 and got[24] != 0.0


@pytest.mark.parametrize("mean,std,figure", kr.LAG_LEVELS)
def test_lagged_corr_level_data(dev, mean, std, figure):
    """Tolerance: 4x what the pivot-centred emulation achieves (the figure
    in kernel_refs.LAG_LEVELS). The raw-moment formula m*Sxy - Sx*Sy
    without the kernel's pivot is off by 1.8e-5 / 2.3e-3 here."""
    a, b = kr.lag_inputs(4000, mean, std)
    ref = kr.lagged_pearson_ref(a, b, 24)
    got = _lagged(dev, a, b, 24)
    err = np.abs(got - ref).max()
    print(f"lagged_corr mean={mean} std={std}: error {err:.3g} "
          f"tol {4 * figure:.3g}")
    assert err <= 4 * figure
    assert int(got.argmax()) == 24 - 5


def test_lagged_corr_spearman_values(dev):
    from ai_crypto_trader_amd.ops.social_corr import (
        lagged_corr_gpu, rank_transform_gpu,
    )

    a, b = kr.lag_inputs(4000)
    ra, rb = kr.ranks(a), kr.ranks(b)
    ra_g = rank_transform_gpu(torch.from_numpy(a).to(dev))
    rb_g = rank_transform_gpu(torch.from_numpy(b).to(dev))
    np.testing.assert_array_equal(ra_g.cpu().numpy(), ra)
    np.testing.assert_array_equal(rb_g.cpu().numpy(), rb)
    got = lagged_corr_gpu(ra_g, rb_g, 24)
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    ref = kr.lagged_pearson_ref(ra, rb, 24)     # f64 Pearson of f64 ranks
    tol = kr.lag_tolerance(ra, rb, 24)
    err = np.abs(got - ref).max()
    print(f"spearman: error {err:.3g} tol {tol:.3g}")
    assert err <= tol
    assert int(got.argmax()) == 24 - 5


def test_lagged_corr_constant_series_is_zero(dev):
    _, b = kr.lag_inputs(1000)
    const = np.full(1000, 0.3, np.float32)
    assert not _lagged(dev, const, b, 24).any()
    assert not _lagged(dev, b, const, 24).any()
    assert not _lagged(dev, const, const, 24).any()


def test_lagged_corr_wrapper_lengths_and_dtypes(dev):
    from ai_crypto_trader_amd.ops.social_corr import lagged_corr_gpu

    a, _ = kr.lag_inputs(300)
    _, b = kr.lag_inputs(257)
    ref = kr.lagged_pearson_ref(a[:257], b, 24)
    for x, y in ((a, b), (b, a)):
        got = _lagged(dev, x, y, 24)
        want = ref if x is a else kr.lagged_pearson_ref(b, a[:257], 24)
        tol = kr.lag_tolerance(x[:257], y[:257], 24)
        assert np.abs(got - want).max() <= tol
    # a wider dtype only: were the check missing, the kernel would read
    # f32 words inside the f64 buffer, never past it
    a_t = torch.from_numpy(a).to(dev)
    with pytest.raises(AssertionError):
        lagged_corr_gpu(a_t, a_t.double(), 4)
    with pytest.raises(AssertionError):
        lagged_corr_gpu(a_t.double(), a_t, 4)


# --- volume histogram -----------------------------------------------------

def _vp(dev, c, n_bins):
    from ai_crypto_trader_amd.utils.volume_profile import vp_hist_gpu

    hist, updown, lo, hi = vp_hist_gpu(torch.from_numpy(c).to(dev),
                                       n_bins=n_bins)
    torch.cuda.synchronize()
    return (hist.cpu().numpy().astype(np.float64),
            updown.cpu().numpy().astype(np.float64),
            lo.cpu().numpy(), hi.cpu().numpy())


@pytest.mark.parametrize("nsym", kr.VP_NSYMS)
@pytest.mark.parametrize("T", kr.VP_TS)
@pytest.mark.parametrize("n_bins", kr.VP_BINS)
def test_vp_hist_exact_binning(dev, n_bins, T, nsym):
    """nsym = 3 carries a flat symbol and one whose close hits the range
    maximum. No candle may sit in a neighbouring bin: an empty bin has
    tolerance zero."""
    edge = dict(flat_sym=1, top_sym=2) if nsym == 3 else {}
    c = kr.vp_inputs(nsym, T, **edge)
    ref, tol, ud_ref, tol_all, _ = kr.vp_ref(c, n_bins)
    hist, updown, lo, hi = _vp(dev, c, n_bins)
    lo_ref, hi_ref = kr.vp_range(c)
    np.testing.assert_array_equal(lo, lo_ref)
    np.testing.assert_array_equal(hi, hi_ref)
    assert np.isfinite(hist).all() and np.isfinite(updown).all()
    print(f"vp_hist bins={n_bins} T={T} nsym={nsym}: "
          f"hist {kr.worst_ratio(hist, ref, tol):.3g} "
          f"updown {kr.worst_ratio(updown, ud_ref, tol_all[:, None]):.3g}")
    assert (np.abs(hist - ref) <= tol).all()
    assert (np.abs(updown - ud_ref) <= tol_all[:, None]).all()
    total = c[..., 3].astype(np.float64).sum(axis=1)
    assert (np.abs(hist.sum(axis=1) - total) <= tol.sum(axis=1)).all()
    if T == 1:
        assert not updown.any()


def test_vp_hist_flat_and_top(dev):
    n_bins, T = 24, 257
    c = kr.vp_inputs(3, T, flat_sym=1, top_sym=2)
    _, _, _, _, b = kr.vp_ref(c, n_bins)
    hist, updown, _, _ = _vp(dev, c, n_bins)
    assert np.isfinite(hist).all() and np.isfinite(updown).all()
    assert hist[1, 0] > 0 and not hist[1, 1:].any()     # flat: one bin
    assert not updown[1, 1]                              # never a down tick
    assert b[2, T // 2] == n_bins - 1                    # close == maximum
    in_last = c[2, b[2] == n_bins - 1, 3].astype(np.float64).sum()
    assert abs(hist[2, -1] - in_last) <= T * kr.U24 * in_last


def test_vp_hist_rejects_too_many_bins(dev):
    from ai_crypto_trader_amd.utils.volume_profile import vp_hist_gpu

    c = torch.from_numpy(kr.vp_inputs(1, 255)).to(dev)
    with pytest.raises(RuntimeError, match="n_bins"):
        vp_hist_gpu(c, n_bins=kr.VP_MAXBINS + 1)
    torch.cuda.synchronize()


# --- indicators -----------------------------------------------------------

def _ind_gpu(dev, candles):
    from ai_crypto_trader_amd.ops.indicators import indicators_gpu

    got = indicators_gpu(
        torch.from_numpy(np.ascontiguousarray(candles)).to(dev))
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _ind_scaled(got, ref):
    """Error in units of the tolerance."""
    return np.abs(got - ref) / (kr.IND_ATOL + kr.IND_RTOL * np.abs(ref))


@pytest.fixture(scope="module")
def ind_case(dev):
    """Candles, the sequential reference (causal: the reference of a
    prefix is the prefix of the reference), and per indicator the largest
    scaled error away from every chunk edge over the whole 4097-candle
    series. The whole series is the yardstick for every T: in the first
    chunk the kernel replays the reference's own f32 rolling sums almost
    bit for bit, in later chunks it restarts them 512 candles earlier and
    their rounding drift differs by a few 1e-6 relative, so the first
    chunk alone would make the honest rows of the second stand out."""
    from ai_crypto_trader_amd.ops.indicators import indicators_cpu

    candles = kr.ind_inputs()
    ref = indicators_cpu(candles)
    T = candles.shape[1]
    rest = np.ones(T, bool)
    rest[kr.ind_edge_rows(T)] = False
    scaled = _ind_scaled(_ind_gpu(dev, candles), ref)
    return candles, ref, scaled[:, rest].max(axis=(0, 1))


@pytest.mark.parametrize("T", kr.IND_TS)
def test_indicators_chunk_edges(dev, ind_case, T):
    candles, ref_full, elsewhere = ind_case
    ref = ref_full[:, :T]
    got = _ind_gpu(dev, candles[:, :T])
    assert got.shape == ref.shape and np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=kr.IND_RTOL,
                               atol=kr.IND_ATOL)
    edge = kr.ind_edge_rows(T)
    if edge.size == 0:
        return
    # rows at a chunk edge must not stand out from the rest of the series,
    # per indicator (4 f32 ulp of slack, in the same units, where the rest
    # happens to be exact)
    at_edge = _ind_scaled(got, ref)[:, edge].max(axis=(0, 1))
    print(f"indicators T={T}: edge {at_edge.max():.3g} "
          f"rest {elsewhere.max():.3g}")
    slack = 4 * 2.0 ** -23 / kr.IND_RTOL
    assert (at_edge <= np.maximum(elsewhere, slack)).all(), (
        at_edge, elsewhere)
