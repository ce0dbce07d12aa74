"""f64 references, error envelopes and CPU emulations for the analytics and
attention kernels (a helper module, no tests of its own).

Shared by test_kernel_refs_cpu.py, which shows on a CPU that every envelope
is reachable by a correct kernel (an emulation of the kernel's arithmetic
sits inside it with 2x room) and rejects a subtly wrong one (seeded
mutants sit outside), and by test_gpu_analytics.py / test_gpu_attention.py,
which hold the HIP kernels to the same envelopes. No constant here was
fitted to a GPU result: each is derived below from the number formats and
the kernel's launch geometry, with its margin fixed by the CPU emulation.

Units: U24 = 2^-24 is the f32 unit roundoff and B8 = 2^-8 the bf16 one
(8 significant bits); a round-to-nearest bf16 store of x is off by up to
B8 |x|, reached just above a power of two.
"""

import numpy as np

U24 = 2.0 ** -24
B8 = 2.0 ** -8


def bf16_round(x):
    """f32 -> nearest-even bf16, returned as f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


def _fma32(acc, a, b):
    """f32 fma: the f64 product of two f32 is exact, so one f64 add and
    one rounding to f32 reproduce it (up to double rounding)."""
    return (acc.astype(np.float64)
            + a.astype(np.float64) * b.astype(np.float64)
            ).astype(np.float32)


# ---------------------------------------------------------------------------
# Covariance (ops/hip/covar.hip)
#
# The kernel is one-pass: Sxy_ij = sum_t x_ti x_tj and Sx_i = sum_t x_ti in
# f32, then (Sxy - Sx_i Sx_j / T) / (T - 1). A sum of n terms accumulated in
# f32 in any order is off by at most n * U24 * sum|terms| (first order), so
# per entry
#     tol_ij = K * U24 * (sum_t |x_ti x_tj| + |Sx_i||Sx_j| / T) / (T - 1)
# where K counts the f32 additions on the longest path into an entry:
#   - the MFMA fma chain: 64 rows per tile, continued in the same
#     accumulator over every tile the block owns,
#   - one per tile for the per-thread column sums,
#   - the atomic adds of the blocks, in any order,
#   - the four finalize operations (product, /T, subtract, /(T-1)).
# The mean term keeps the bound honest for data that are not centred: a
# relative error in Sx shows up as that fraction of Sx_i Sx_j / T.
# ---------------------------------------------------------------------------
COV_TILE_T = 64
COV_MAX_BLOCKS = 512
COV_THREADS = 256
COV_NS = (16, 32, 48, 64)
# 64*512 + 1: the grid-stride loop wraps, into a tile of a single row
COV_TS = (2, 63, 64, 65, 1037, 64 * 512 + 1)
COV_BAD_NS = (8, 40, 80)


def cov_inputs(T, N):
    """Per-column mean 0.02 (1 + j/N), comparable to the std; means and
    scales differ by column, so a shifted or transposed column shows."""
    rng = np.random.default_rng([11, T, N])
    j = np.arange(N)
    mean = 0.02 * (1.0 + j / N)
    std = 0.02 * (1.0 + 0.5 * ((5 * j + 3) % N) / N)
    return (mean + std * rng.standard_normal((T, N))).astype(np.float32)


def cov_ref(X):
    return np.atleast_2d(np.cov(X.astype(np.float64), rowvar=False))


def cov_geometry(T):
    """(ntiles, blocks, tiles per block) of launch_cov."""
    ntiles = -(-T // COV_TILE_T)
    nblocks = min(ntiles, COV_MAX_BLOCKS)
    return ntiles, nblocks, -(-ntiles // nblocks)


def cov_k(T):
    _, nblocks, tpb = cov_geometry(T)
    return COV_TILE_T * tpb + tpb + nblocks + 4


def cov_envelope(X):
    X64 = X.astype(np.float64)
    T = X64.shape[0]
    sx = np.abs(X64.sum(axis=0))
    a = np.abs(X64).T @ np.abs(X64)
    return cov_k(T) * U24 * (a + np.outer(sx, sx) / T) / (T - 1)


def _cov_emulate_sxy(X):
    T, N = X.shape
    ntiles, nblocks, tpb = cov_geometry(T)
    acc = np.zeros((nblocks, N, N), np.float32)
    for p in range(tpb):
        tiles = np.arange(nblocks) + p * nblocks
        for k in range(COV_TILE_T):
            rows = tiles * COV_TILE_T + k
            live = np.nonzero((tiles < ntiles) & (rows < T))[0]
            if live.size == 0:       # zero padding: fma(0, 0, acc) == acc
                continue
            xr = X[rows[live]]
            acc[live] = _fma32(acc[live], xr[:, :, None], xr[:, None, :])
    return np.cumsum(acc, axis=0, dtype=np.float32)[-1]


def _cov_emulate_sx(X, double_count):
    """Column sums in the kernel's geometry: thread tid sums column
    tid % N over rows tid / N, tid / N + 256 / N, ... of each tile.
    double_count=True is the seeded defect: all 256 threads run, and
    where N does not divide 256 those past N * (256 / N) add rows a
    second time."""
    T, N = X.shape
    ntiles, nblocks, _ = cov_geometry(T)
    rpp = COV_THREADS // N
    ngroups = -(-COV_THREADS // N) if double_count else rpp
    sx = np.zeros(N, np.float32)
    for b in range(nblocks):
        lds = np.zeros(N, np.float32)
        for g in range(ngroups):
            ncols = min(N, COV_THREADS - g * N)
            rows = np.concatenate([
                np.arange(t * COV_TILE_T + g,
                          min((t + 1) * COV_TILE_T, T), rpp)
                for t in range(b, ntiles, nblocks)])
            if rows.size:
                lds[:ncols] += np.cumsum(X[rows, :ncols], axis=0,
                                         dtype=np.float32)[-1]
        sx += lds
    return sx


def cov_emulate(X, double_count=False, mean_term=True):
    """The kernel's arithmetic in f32. The two flags are the mutants."""
    T = np.float32(X.shape[0])
    sxy = _cov_emulate_sxy(X)
    sx = _cov_emulate_sx(X, double_count)
    if not mean_term:
        return sxy / (T - np.float32(1))
    return (sxy - sx[:, None] * sx[None, :] / T) / (T - np.float32(1))


# ---------------------------------------------------------------------------
# Attention (ops/hip/attention.hip)
#
# bf16 keeps 8 significant bits: a round-to-nearest store is off by at most
# B8 = 2^-8 relative (half of its 2^-7 ulp).
#
# Forward. Inputs are bf16, products of two bf16 are exact in f32, scores
# and the softmax are f32 (relative error ~1e-5 with __expf and v_rcp, far
# below B8). The kernel rounds twice: P to bf16 before P @ V, and O to
# bf16 on store. With |P~ - P| <= B8 P,
#     |O~_id - O_id| <= B8 sum_j P_ij |V_jd| + B8 |O_id|
#                    <= 2 B8 * sum_j P_ij |V_jd|,
# so tol_id = C_FWD * B8 * sum_j P_ij |V_jd|. The worst case, 2, needs both
# roundings at their maximum, aligned, and no cancellation in O; rows where
# two keys share the weight come close, and the emulation reaches 1.56 on
# the cases below (1.38 for dV). C_FWD is twice that, rounded up, which
# leaves the emulation its 2x room and a correct kernel 1.75x over the
# worst case for f32 ordering and 1-ulp flips of __expf / v_rcp. The saved
# P is rounded once: |P~ - P| <= B8 P, which the emulation attains (0.996);
# it is held to the same C_FWD * B8 * P.
#
# Backward, from the saved P~ (bf16), dP = dO V^T (f32), r~_i = sum_j P~ dP:
#     dS~_ij = bf16(scale * P~_ij (dP_ij - r~_i)),
#     |r~_i - r_i| <= B8 R_i,   R_i = sum_j P_ij |dP_ij|,
#     |dS~_ij - dS_ij| <= 2 B8 |dS_ij| + B8 scale P_ij R_i
# (P's rounding, dS's rounding, and r~'s error carried through: the term
# that P's rounding induces in dS), then dQ = bf16(dS~ K),
# dK = bf16(dS~^T Q), dV = bf16(P~^T dO):
#     |dV~_jd - dV_jd| <= 2 B8 * sum_i P_ij |dO_id|               (as O)
#     |dQ~_id - dQ_id| <= 3 B8 * sum_j (|dS_ij| + scale P_ij R_i) |K_jd|
#     |dK~_jd - dK_jd| <= 3 B8 * sum_i (|dS_ij| + scale P_ij R_i) |Q_id|
# The worst case 3 takes three aligned roundings per term; with dozens of
# terms of both signs in every sum the emulation reaches 0.82 on the cases
# below. C_BWD is twice that, rounded up.
#
# Conditioning. sum_j dS_ij = 0 exactly, so dQ is a difference of terms and
# the R term is of the size of the |dS| term at best: the normwise bound
# ||tol||_F / ||ref||_F cannot be much below 2 * C_BWD * B8 for any input,
# and is several times that for sign-random ones. It has to stay within
# 2^-6 = 4 B8. ATT_BWD_KW (a weak common query direction, little noise)
# gives 0.84 * 2^-6 at worst; the sharper ATT_FWD_KW, which the forward
# cases use to exercise the softmax, would give 2 * 2^-6 and is not used
# for gradients.
# ---------------------------------------------------------------------------
ATT_S = 64
C_FWD = 3.5
C_BWD = 1.75
ATT_FWD_KW = dict(qamp=1.5, noise=0.25)
ATT_BWD_KW = dict(qamp=0.2, noise=0.05)
ATT_NORMWISE_MAX = 2.0 ** -6
ATT_DS = (16, 32, 64)
ATT_FWD_SS = (1, 16, 17, 33, 60, 64)
ATT_BWD_SS = (1, 17, 60, 64)
ATT_GUARD_SS = (1, 17, 60)
ATT_BH = 3
ATT_SCALE = 0.37           # the non-default scale
ATT_SENTINEL = -776.0      # bf16-representable, far outside every output
ATT_P_FLOOR = 1e-30        # below it exp() may flush; nothing depends on it
ATT_OLD_ATOL = 3e-2        # test_attn_fwd_matches_sdpa


def attn_inputs(BH, S, D, seed=0, logit_mag=None, scale=None, qamp=1.5,
                noise=0.25):
    """bf16-representable f32 (Q, K, V, dO), each (BH, S, D).

    Key/value row j carries its own offset a_j (a permutation of
    linspace(-1, 1)) along a direction k0 / v0; queries (amplitude qamp)
    and the upstream gradient share a direction, plus independent noise.
    The offsets make a permuted key index or a swapped fragment row
    visible, and they keep the backward sums from cancelling more than
    they must (see Conditioning above). dO is random and independent of
    the forward, not the gradient of a symmetric loss.
    logit_mag rescales Q so that max |scale * q.k| is about that value."""
    rng = np.random.default_rng([23, BH, S, D, seed])
    a = np.stack([rng.permutation(np.linspace(-1.0, 1.0, S)) if S > 1
                  else np.array([0.7]) for _ in range(BH)])

    def direction():
        v = rng.standard_normal((BH, 1, D))
        return v / np.sqrt((v ** 2).mean(axis=-1, keepdims=True))

    def jitter():
        return noise * rng.standard_normal((BH, S, D))

    K = a[:, :, None] * direction() + jitter()
    V = a[:, :, None] * direction() + jitter()
    Q = qamp * direction() + jitter()
    dO = direction() + jitter()
    if logit_mag is not None:
        sc = 1.0 / np.sqrt(D) if scale is None else scale
        Q = Q * (logit_mag / np.abs(sc * Q @ K.transpose(0, 2, 1)).max())
    return tuple(bf16_round(t) for t in (Q, K, V, dO))


def attn_scale(D, scale=None):
    return 1.0 / np.sqrt(D) if scale is None else scale


# (BH, S, D, scale or None, logit_mag or None)
ATT_FWD_CASES = (
    [(ATT_BH, S, D, None, None) for D in ATT_DS for S in ATT_FWD_SS]
    + [(1, 60, 16, None, None)]
    + [(ATT_BH, 60, D, ATT_SCALE, None) for D in ATT_DS]
    + [(ATT_BH, 60, D, None, 50.0) for D in ATT_DS])
ATT_BWD_CASES = (
    [(ATT_BH, S, D, None, None) for D in ATT_DS for S in ATT_BWD_SS]
    + [(ATT_BH, 60, D, ATT_SCALE, None) for D in ATT_DS])


def attn_case_id(case):
    BH, S, D, scale, mag = case
    return f"BH{BH}-S{S}-D{D}" + (f"-scale{scale}" if scale else "") + (
        f"-logit{mag:g}" if mag else "")


def attn_case(case, backward=False):
    """(Q, K, V, dO, scale) of a case; backward cases use ATT_BWD_KW."""
    BH, S, D, scale, mag = case
    kw = ATT_BWD_KW if backward else ATT_FWD_KW
    return attn_inputs(BH, S, D, logit_mag=mag, scale=scale, **kw) + (
        float(attn_scale(D, scale)),)


def attn_ref(Q, K, V, dO, scale):
    """f64 softmax attention and its gradients for the upstream dO, from
    the bf16-rounded inputs, P left unrounded. Returns a dict of arrays
    and of per-element tolerances (tol_*)."""
    Q, K, V, dO = (t.astype(np.float64) for t in (Q, K, V, dO))
    logits = scale * Q @ K.transpose(0, 2, 1)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    P = e / e.sum(axis=-1, keepdims=True)
    O = P @ V
    dV = P.transpose(0, 2, 1) @ dO
    dP = dO @ V.transpose(0, 2, 1)
    r = (P * dP).sum(axis=-1, keepdims=True)
    dS = scale * P * (dP - r)
    dQ = dS @ K
    dK = dS.transpose(0, 2, 1) @ Q
    R = (P * np.abs(dP)).sum(axis=-1, keepdims=True)
    E = np.abs(dS) + scale * P * R
    return dict(
        P=P, O=O, dQ=dQ, dK=dK, dV=dV,
        tol_P=C_FWD * B8 * P + ATT_P_FLOOR,
        tol_O=C_FWD * B8 * (P @ np.abs(V)),
        tol_dV=C_FWD * B8 * (P.transpose(0, 2, 1) @ np.abs(dO)),
        tol_dQ=C_BWD * B8 * (E @ np.abs(K)),
        tol_dK=C_BWD * B8 * (E.transpose(0, 2, 1) @ np.abs(Q)),
    )


ATTN_MUTANTS = ("key_off16", "mask_weight", "no_scale_ds", "no_rowsum",
                "dk_no_transpose")


def attn_emulate(Q, K, V, dO, scale, mutant=None):
    """The kernels' arithmetic: f32 accumulation over the 64-padded tile,
    bf16 rounding of P, O, dS and the three gradients. Returns f32
    O, P (BH, 64, 64), dQ, dK, dV. Mutants: a key index off by 16 in one
    column tile, masked columns given weight, scale omitted in dS, the
    rowsum correction dropped, dK built from dS instead of dS^T."""
    f32 = np.float32
    BH, S, D = Q.shape

    def pad(t):
        out = np.zeros((BH, ATT_S, D), f32)
        out[:, :S] = t
        return out

    Qp, Kp, Vp, dOp = pad(Q), pad(K), pad(V), pad(dO)
    kidx = np.arange(ATT_S)
    if mutant == "key_off16":
        kidx[16:32] += 16
    sc = (Qp @ Kp[:, kidx].transpose(0, 2, 1)) * f32(scale)
    if mutant != "mask_weight":
        sc[:, :, S:] = f32(-1e30)
    e = np.exp(sc - sc.max(axis=-1, keepdims=True), dtype=f32)
    Pb = bf16_round(e * (f32(1) / e.sum(axis=-1, dtype=f32,
                                        keepdims=True)))
    O = bf16_round(Pb @ Vp)[:, :S]

    dP = dOp @ Vp.transpose(0, 2, 1)
    rs = (dP * Pb).sum(axis=-1, dtype=f32, keepdims=True)
    if mutant == "no_rowsum":
        rs = np.zeros_like(rs)
    ds_scale = f32(1) if mutant == "no_scale_ds" else f32(scale)
    dSb = bf16_round(ds_scale * Pb * (dP - rs))
    dQ = bf16_round(dSb @ Kp)[:, :S]
    dSt = dSb if mutant == "dk_no_transpose" else dSb.transpose(0, 2, 1)
    dK = bf16_round(dSt @ Qp)[:, :S]
    dV = bf16_round(Pb.transpose(0, 2, 1) @ dOp)[:, :S]
    return dict(O=O, P=Pb, dQ=dQ, dK=dK, dV=dV)


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol; an exact match at tol == 0 counts as 0."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / tol)
    return float(q.max())


def normwise(tol, ref):
    """||tol||_F / ||ref||_F, or 0 where the reference is exactly zero
    (S = 1: dS, dQ and dK vanish identically, as does their bound)."""
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(tol) / n) if n > 0 else 0.0


# ---------------------------------------------------------------------------
# Lagged correlation (ops/hip/laggedcorr.hip)
#
# Reference: f64 two-pass Pearson per lag. The kernel's error is set by its
# f32 moment sums, whose cancellation depends on the data's level; the
# tolerance of a case is therefore what an emulation of the kernel's exact
# reduction order achieves on the same data when it first subtracts the
# pivot (x[0], y[0]) of each lag's window, times 4, and never below 4 ulp
# of an f32 result near 1 (2^-23): the result itself is stored in f32.
# ---------------------------------------------------------------------------
LAG_BLOCK = 256
LAG_NS = (3, 255, 256, 257, 4000)
LAG_MAX_LAGS = (0, 24)
LAG_ULP = 2.0 ** -23
# (mean, std, envelope of the pivot-centred emulation at n = 4000,
#  max_lag = 24). The envelope figures are asserted by
#  test_kernel_refs_cpu.py; the GPU tolerance is 4x the figure. The
#  uncentred f32 formula gives 1.8e-5 and 2.3e-3 on these.
LAG_LEVELS = ((1000.0, 100.0, 1.9e-7), (60000.0, 500.0, 1.3e-7))


def lag_inputs(n, mean=0.5, std=1.0, lead=5):
    """b random around `mean`; a follows b by `lead` samples plus noise."""
    rng = np.random.default_rng([51, n])
    zb = rng.standard_normal(n)
    za = np.roll(zb, lead) * 0.8 + rng.standard_normal(n) * 0.3
    return ((mean + std * za).astype(np.float32),
            (mean + std * zb).astype(np.float32))


def _lag_windows(a, b, lag):
    n = len(a)
    m = n - abs(lag)
    if lag >= 0:
        return a[:m], b[lag:lag + m]
    return a[-lag:-lag + m], b[:m]


def lagged_pearson_ref(a, b, max_lag):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out = np.zeros(2 * max_lag + 1)
    for j, lag in enumerate(range(-max_lag, max_lag + 1)):
        if len(a) - abs(lag) < 3:
            continue
        x, y = _lag_windows(a64, b64, lag)
        x, y = x - x.mean(), y - y.mean()
        den = np.sqrt((x * x).sum() * (y * y).sum())
        if den > 0:
            out[j] = (x * y).sum() / den
    return out


def _lag_block_sum(x, y=None):
    """sum(x) or sum(x*y) as the kernel's block does it: thread tid runs
    an f32 (fma) chain over i = tid, tid+256, ..., then the shfl_down tree
    of each wave, then the tree over the four waves."""
    m = len(x)
    rows = -(-m // LAG_BLOCK)
    xp = np.zeros(rows * LAG_BLOCK, np.float32)
    xp[:m] = x
    xp = xp.reshape(rows, LAG_BLOCK)
    if y is None:
        v = np.cumsum(xp, axis=0, dtype=np.float32)[-1]
    else:
        yp = np.zeros(rows * LAG_BLOCK, np.float32)
        yp[:m] = y
        yp = yp.reshape(rows, LAG_BLOCK)
        v = np.zeros(LAG_BLOCK, np.float32)
        for r in range(rows):
            v = _fma32(v, xp[r], yp[r])
    v = v.reshape(4, 64).copy()
    off = 32
    while off:
        v[:, :64 - off] = v[:, :64 - off] + v[:, off:]
        off //= 2
    w = v[:, 0]
    return np.float32(np.float32(w[0] + w[2]) + np.float32(w[1] + w[3]))


def lagged_corr_emulate(a, b, max_lag, pivot=True):
    f32 = np.float32
    out = np.zeros(2 * max_lag + 1, f32)
    for j, lag in enumerate(range(-max_lag, max_lag + 1)):
        m = len(a) - abs(lag)
        if m < 3:
            continue
        x, y = _lag_windows(a, b, lag)
        if pivot:
            x, y = x - x[0], y - y[0]
        sx, sy = _lag_block_sum(x), _lag_block_sum(y)
        sxy = _lag_block_sum(x, y)
        sxx, syy = _lag_block_sum(x, x), _lag_block_sum(y, y)
        fm = f32(m)
        cov = fm * sxy - sx * sy
        vx = fm * sxx - sx * sx
        vy = fm * syy - sy * sy
        den = np.sqrt(max(vx, f32(0))) * np.sqrt(max(vy, f32(0)))
        out[j] = cov / den if den > f32(1e-12) else f32(0)
    return out


def lag_tolerance(a, b, max_lag):
    ref = lagged_pearson_ref(a, b, max_lag)
    emu = lagged_corr_emulate(a, b, max_lag, pivot=True)
    return 4.0 * max(float(np.abs(emu - ref).max()), LAG_ULP)


def ranks(x):
    r = np.empty(len(x), np.float32)
    r[np.argsort(x, kind="stable")] = np.arange(len(x), dtype=np.float32)
    return r


# ---------------------------------------------------------------------------
# Volume histogram (ops/hip/histogram.hip)
#
# The bin of a candle is the kernel's own f32 expression,
#     int((close - lo) * (f32(n_bins) / max(hi - lo, 1e-12))), clamped,
# every step of which is a single IEEE operation (no a*b+c for the compiler
# to contract), so numpy in f32 gives the same integer. Only the f32 volume
# sums are inexact: n_b candles added in any order are off by at most
# n_b * U24 * sum|vol|.
# ---------------------------------------------------------------------------
VP_BINS = (1, 24, 32, 512)
VP_TS = (1, 255, 257, 5000)
VP_NSYMS = (1, 3)
VP_MAXBINS = 512


def vp_inputs(nsym, T, flat_sym=None, top_sym=None):
    """(nsym, T, 4) [close, high, low, vol] f32. flat_sym: a symbol whose
    prices never move; top_sym: one candle closes on the range maximum."""
    rng = np.random.default_rng([61, nsym, T])
    close = 100.0 * (1 + np.arange(nsym))[:, None] * np.exp(
        np.cumsum(0.01 * rng.standard_normal((nsym, T)), axis=1))
    high = close * (1 + 0.004 * rng.random((nsym, T)))
    low = close * (1 - 0.004 * rng.random((nsym, T)))
    vol = np.exp(rng.standard_normal((nsym, T)) + 3.0)
    c = np.stack([close, high, low, vol], axis=-1).astype(np.float32)
    c[..., 1] = np.maximum(c[..., 1], c[..., 0])
    c[..., 2] = np.minimum(c[..., 2], c[..., 0])
    if flat_sym is not None:
        c[flat_sym, :, :3] = np.float32(137.25)
    if top_sym is not None:
        t = T // 2
        c[top_sym, t, 1] = c[top_sym, :, 1].max() * np.float32(1.001)
        c[top_sym, t, 0] = c[top_sym, t, 1]
    return c


def vp_range(candles):
    """lo, hi as vp_hist_gpu forms them (f32: hi = max(high) + 1e-9)."""
    lo = candles[:, :, 2].min(axis=1)
    hi = candles[:, :, 1].max(axis=1) + np.float32(1e-9)
    return lo.astype(np.float32), hi.astype(np.float32)


def vp_ref(candles, n_bins):
    """hist f64 (nsym, n_bins), its tolerance, updown f64 (nsym, 2), its
    tolerance (nsym,), and the per-candle bin index."""
    f32 = np.float32
    nsym, T, _ = candles.shape
    lo, hi = vp_range(candles)
    close = candles[:, :, 0]
    vol = candles[:, :, 3].astype(np.float64)
    inv_w = f32(n_bins) / np.maximum(hi - lo, f32(1e-12))
    x = ((close - lo[:, None]) * inv_w[:, None]).astype(f32)
    b = np.clip(np.trunc(x).astype(np.int64), 0, n_bins - 1)
    hist = np.zeros((nsym, n_bins))
    tol = np.zeros((nsym, n_bins))
    for s in range(nsym):
        hist[s] = np.bincount(b[s], weights=vol[s], minlength=n_bins)
        cnt = np.bincount(b[s], minlength=n_bins)
        tol[s] = cnt * U24 * np.bincount(b[s], weights=np.abs(vol[s]),
                                         minlength=n_bins)
    up = close[:, 1:] >= close[:, :-1]
    updown = np.stack([(vol[:, 1:] * up).sum(axis=1),
                       (vol[:, 1:] * ~up).sum(axis=1)], axis=1)
    tol_all = T * U24 * np.abs(vol).sum(axis=1)
    return hist, tol, updown, tol_all, b


# ---------------------------------------------------------------------------
# Indicators (ops/hip/indicators.hip): shapes at the edges of the
# 2048-candle chunk, three symbols so the lanes do not fill a block.
# ---------------------------------------------------------------------------
IND_CHUNK = 2048
IND_TS = (1, 19, 20, 2047, 2048, 2049, 4097)
IND_NSYM = 3
IND_RTOL, IND_ATOL = 1e-3, 2e-4     # test_indicators_gpu_matches_cpu


def ind_inputs():
    from ai_crypto_trader_amd.data.synthetic import (
        candles_chl_v, generate_ohlcv,
    )
    return candles_chl_v(generate_ohlcv(max(IND_TS), IND_NSYM, seed=71))


def ind_edge_rows(T):
    """Rows within +-2 of each positive multiple of the chunk length."""
    rows = [r for k in range(1, T // IND_CHUNK + 2)
            for r in range(k * IND_CHUNK - 2, k * IND_CHUNK + 3)
            if 0 <= r < T]
    return np.array(rows, dtype=np.int64)
