"""f64 references, error envelopes, f32 CPU emulations and input generators
for the regime kernels (ops/hip/regime.hip): window features, the
Gaussian-HMM E-step and Viterbi. A helper module in the style of
kernel_refs.py / rnn_refs.py, no tests of its own.

Shared by test_regime_refs_cpu.py, which shows on a CPU that every envelope
is reachable (an f32 emulation of the kernel's arithmetic sits inside it
with half the f32 part) and that it rejects a subtly wrong kernel (seeded
mutants sit outside), and by test_gpu_regime.py, which holds the HIP
kernels to the same envelopes. No constant here was fitted to a GPU result.

Units and rules. U24 = 2^-24 is the f32 unit roundoff: +, -, *, fma, and
hipcc's default correctly rounded / and sqrtf are off by at most U24 of
their result, and that is what every operation is charged. Errors are
carried by running error analysis,
    a + b : e_a + e_b + U24 |a + b|
    a * b : |a| e_b + |b| e_a + e_a e_b + U24 |a b|
so cancellation is covered by absolute terms and fma contraction only
helps. A sum of n terms accumulated in f32 in any order is off by at most
n U24 sum|terms| on top of its terms' own errors (kernel_refs.py). The CPU
tests hold the emulation to half of every envelope. One output cannot
meet that at U24: `ret` = w[-1] / w[0] - 1 is one division and an exact
subtraction away from its inputs, so a correct kernel reaches the full
U24 bound; its two operations alone are charged RET_EPS = 2 U24.
Figures that do not come from the number format:
  * v_exp_f32, v_log_f32 and v_rcp_f32 are 1 ulp = 2 U24 each (the
    instruction set reference, as rnn_refs.py cites). exp(z) is
    v_exp_f32(z * log2e): the product and the constant's rounding move the
    argument by 2 U24 |z log2e|, which exp2 turns into a relative
    2 U24 |z|. v_exp_f32 flushes results below 2^-126, an absolute 2^-126.
  * log1pf is the compiler's library routine, not an instruction, and
    running error analysis cannot give its error. Following
    kernel_refs.LAG_LEVELS, its allowance is 4 times the error of the f32
    emulation's log1p against f64 on the same inputs, recorded as
    LOG1P_EMU_REL.
  * Input rounding is not charged: every reference takes the same
    f32-rounded inputs as the kernel.

Features. Reference: extract_features' formulas in f64 on the f32 closes.
The envelope follows the kernel's two passes about the pivot w[-1] term by
term (feat_ref). Nothing in it depends on the price level beyond the
level's own f32 spacing, which is what the 6e4 case is there to show.

E-step, forward: per step with teacher forcing. The kernel stores the
scaled alpha and c, so the f64 reference of step t starts from the
kernel's own alpha of step t - 1 and only one step's rounding lies between
the two (estep_forward_ref). The kernel's shift is the max of ITS emission
log-densities; c_t is relative to that shift, so c's envelope carries the
emission error of the max state, while alpha and log c_t + shift_t do not
depend on the shift at all.
Log-likelihood: (1) against the sum of the teacher-forced terms, a
reduction over t; (2) against a free-running log-space f64 forward pass,
where the kernel's alpha_{t-1} differs from the f64 one by an accumulated
error. A term log sum_j (a A)_j b_j moves by at most the Hilbert projective
distance d_H(a', a) = max_i log(a'_i / a_i) - min_i log(a'_i / a_i) when a
moves to a', so (2) adds the OBSERVED sum_t d_H(alpha'_{t-1}, alpha_{t-1})
(components floored at 2^-126) to the envelope of (1). The alphas
themselves are held per step, so this cannot hide a wrong recursion.

E-step, backward: beta is never stored. Anchored mode: the returned gamma
gives beta_{t+1}[j] up to a common factor as gamma'_{t+1}[j] /
alpha'_{t+1}[j] (3 roundings), so the f64 reference of gamma_t and of xi_t
starts from the kernel's own step t + 1 (estep_backward_ref); what a
denormal or zero stored value hides is bounded there and added.
Chain mode, for T <= HMM_CHAIN_MAX_T: against the free-running f64
forward-backward. Both recursions are a positive linear map, a positive
diagonal scaling and a normalisation per step, none of which expands d_H
(Birkhoff), and a per-component relative error r moves d_H by at most 2 r,
so the local envelopes add: gamma_t is within gamma_t (exp(D_t) - 1) of
the reference, D_t = sum_{s<=t} 2 max_i r_alpha,s + sum_{s>=t} 2 max_i
r_gamma,s. The bound grows with T, which is why it is used for small T
only. The reductions gamma_sum, gamma_sum_head, sx, sxx are held against
the f64 sums of the kernel's own returned gamma.

Viterbi. The kernel maximises the path score with every term rounded to
f32, i.e. a perturbed objective off by at most E = sum_t e_t for every
path, so the true (f64) score of its path is within 2 E of the f64 optimum
(viterbi_ref). On the planted inputs the path itself must match.
"""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view as _swv

from kernel_refs import U24, _fma32

GUARD = 64                  # NaN / sentinel tail behind every GPU output
RET_EPS = 2.0 * U24         # per operation of `ret` alone, see above
F32_MIN = 2.0 ** -126
# Relative error of the emulation's f32 log1p (numpy) against f64 on the
# log-return arguments of feat_closes at levels 100 and 6e4: 0.99 U24
# measured on the CPU, asserted by test_regime_refs_cpu.py. The kernel's
# log1pf is allowed 4 times this figure.
LOG1P_EMU_REL = 1.0 * U24
ALPHA_FLOOR = 1e-30         # chain mode: no relative envelope below this
HMM_CHAIN_MAX_T = 3
f32 = np.float32
LOG2E32 = f32(1.4426950408889634)
LN2_32 = f32(0.6931471805599453)

FEAT_WINS = (2, 12, 26, 32, 256)
FEAT_EXTRAS = (1, 255, 256, 257)        # T - win: the 256-window tile edge
FEAT_SS = (1, 3)
FEAT_MUTANTS = ("slope_no_win", "sample_std", "macd_long12")

HMM_KFS = ((1, 1), (2, 1), (3, 6), (4, 6), (8, 8))
HMM_TS = (1, 2, 3, 63, 64, 65, 257)
HMM_BS = (1, 5)
HMM_RAGGED = (1, 2, 65, 257, 64)
HMM_LONG_T = 2048
ESTEP_MUTANTS = ("no_shift", "head_with_last", "xi_alpha_next")
# The scaled f32 emulation against the free-running f64 reference on the
# long far-off case (hmm_inputs(1, 2048, 4, 6, far=True)): worst |alpha|
# error and relative log-likelihood error. Asserted (as upper figures) by
# test_regime_refs_cpu.py; the unscaled f32 forward pass is dead (zero or
# non-finite) within the first steps of that input.
HMM_LONG_ALPHA_ERR = 4.5e-7
HMM_LONG_LL_REL = 3.5e-8


def worst(got, ref, tol):
    """max |got - ref| / tol; an exact match at tol == 0 counts as 0 and a
    non-finite value as inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / tol)
    q = np.where(np.isfinite(got) & ~np.isnan(q), q, np.inf)
    return float(q.max()) if q.size else 0.0


# ---------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------
def feat_closes(S, T, level=100.0, move=1e-3, seed=0):
    """Geometric random walks at `level` with per-candle moves of `move`."""
    rng = np.random.default_rng([71, S, T, int(level), seed])
    return (level * np.exp(np.cumsum(rng.normal(0.0, move, (S, T)), axis=1))
            ).astype(f32)


def _sqrt_bound(v, e):
    return np.sqrt(v + e) - np.sqrt(np.maximum(v - e, 0.0))


def feat_ref(closes, lengths, win):
    """-> (ref, env), both (S, Tmax - win, 6) f64; rows at or past
    lengths[s] - win are 0 with envelope 0."""
    c = np.asarray(closes, f32).astype(np.float64)
    S, T = c.shape
    nw = max(T - win, 0)
    ref = np.zeros((S, nw, 6))
    env = np.zeros((S, nw, 6))
    if nw == 0:
        return ref, env
    u, n, m = U24, float(win), float(win - 1)
    W = _swv(c, win, axis=1)[:, :nw]
    p, w0 = W[..., -1], W[..., 0]

    ratio = p / w0
    ref[..., 0] = ratio - 1.0
    # one division and an exact subtraction from the inputs: see RET_EPS
    env[..., 0] = RET_EPS * (np.abs(ratio) + np.abs(ref[..., 0]))

    # log-returns: log1p(fl(fl(c1 - c0) / c0))
    a = np.diff(c, axis=1) / c[:, :-1]
    lr = np.log1p(a)
    e_lr = 2 * u * np.abs(a) / (1.0 + a) + 4 * LOG1P_EMU_REL * np.abs(lr)
    if win > 2:
        Lr = _swv(lr, win - 1, axis=1)[:, :nw]
        Elr = _swv(e_lr, win - 1, axis=1)[:, :nw]
        R = Lr.sum(-1)
        eR = Elr.sum(-1) + m * u * np.abs(Lr).sum(-1)
        rm = R / m
        e_rm = eR / m + u * np.abs(rm)
        q = Lr - rm[..., None]
        e_q = Elr + e_rm[..., None] + u * np.abs(q)
        t = q * q
        e_t = 2 * np.abs(q) * e_q + e_q ** 2 + u * t
        R2 = t.sum(-1)
        v = R2 / m
        e_v = (e_t.sum(-1) + m * u * R2) / m + u * v
        ref[..., 1] = np.sqrt(v)
        env[..., 1] = _sqrt_bound(v, e_v) + u * ref[..., 1]

    # pass 1 about the pivot p, pass 2 about the mean
    d = W - p[..., None]
    e_d = u * np.abs(d)
    Ssum = d.sum(-1)
    e_S = e_d.sum(-1) + n * u * np.abs(d).sum(-1)
    dm = Ssum / n
    e_dm = e_S / n + u * np.abs(dm)
    e = d - dm[..., None]
    e_e = e_d + e_dm[..., None] + u * np.abs(e)
    mean = p + dm
    e_mean = e_dm + u * np.abs(mean)

    t2 = e * e
    e_t2 = 2 * np.abs(e) * e_e + e_e ** 2 + u * t2
    E2 = t2.sum(-1)
    v = E2 / n
    e_v = (e_t2.sum(-1) + n * u * E2) / n + u * v
    sd = np.sqrt(v)
    e_sd = _sqrt_bound(v, e_v) + u * sd
    den = np.maximum(mean, 1e-9)
    ref[..., 5] = sd / den
    env[..., 5] = (e_sd / den + sd * e_mean / den ** 2
                   + u * np.abs(ref[..., 5]))

    x = np.arange(win) - 0.5 * (win - 1)
    tx = e * x
    XE = tx.sum(-1)
    e_XE = (np.abs(x) * e_e + u * np.abs(tx)).sum(-1) \
        + n * u * np.abs(tx).sum(-1)
    sxx = n * (n * n - 1.0) / 12.0
    ref[..., 2] = XE / sxx / mean * n
    # sxx in f32: exact integers times the rounded 1/12 (2 roundings), then
    # three more operations
    env[..., 2] = (e_XE / sxx / np.abs(mean) * n
                   + np.abs(ref[..., 2]) * (e_mean / np.abs(mean) + 5 * u))

    df = np.diff(W, axis=-1)
    e_df = u * np.abs(df)
    up, dn = np.maximum(df, 0), np.maximum(-df, 0)
    G, L = up.sum(-1), dn.sum(-1)
    e_G = np.where(df > 0, e_df, 0).sum(-1) + n * u * G
    e_L = np.where(df < 0, e_df, 0).sum(-1) + n * u * L
    g, l = G / m, L / m
    e_g, e_l = e_G / m + u * g, e_L / m + u * l
    gl = g + l
    e_gl = e_g + e_l + u * gl
    dd = np.maximum(gl, 1e-12)
    ref[..., 3] = 100 * g / dd
    env[..., 3] = (100 * e_g / dd + 100 * g * e_gl / dd ** 2
                   + 2 * u * ref[..., 3])

    nf = min(win, 12)
    ns = 26 if win >= 26 else win
    parts = []
    for k in (nf, ns):
        dk, ek = d[..., -k:], e_d[..., -k:]
        s = dk.sum(-1)
        e_s = ek.sum(-1) + k * u * np.abs(dk).sum(-1)
        parts.append((s / k, e_s / k + u * np.abs(s / k)))
    diff = parts[0][0] - parts[1][0]
    e_diff = parts[0][1] + parts[1][1] + u * np.abs(diff)
    ref[..., 4] = diff / p
    env[..., 4] = e_diff / np.abs(p) + u * np.abs(ref[..., 4])

    lengths = (np.full(S, T) if lengths is None
               else np.clip(np.asarray(lengths), 0, T))
    bad = np.arange(nw)[None] >= (lengths[:, None] - win)
    ref[bad] = 0.0
    env[bad] = 0.0
    return ref, env


def feat_emulate(closes, lengths, win, mutant=None):
    """The kernel's f32 arithmetic, window by window in its order."""
    c = np.ascontiguousarray(closes, f32)
    S, T = c.shape
    nw = max(T - win, 0)
    out = np.zeros((S, nw, 6), f32)
    if nw == 0:
        return out
    W = _swv(c, win, axis=1)[:, :nw]
    a = c[:, :-1]
    lr = np.log1p((c[:, 1:] - a) / a).astype(f32)
    Lr = _swv(lr, win - 1, axis=1)[:, :nw]
    p = W[..., -1]
    kf = win - min(win, 12)
    ks = win - 26 if win >= 26 else 0
    if mutant == "macd_long12":
        ks = kf
    z = np.zeros((S, nw), f32)
    Ssum, Sf, Ss, G, L, R = (z.copy() for _ in range(6))
    prev = W[..., 0]
    for k in range(win):
        wk = W[..., k]
        d = wk - p
        Ssum = Ssum + d
        if k >= kf:
            Sf = Sf + d
        if k >= ks:
            Ss = Ss + d
        df = wk - prev
        G = G + np.maximum(df, f32(0))
        L = L + np.maximum(-df, f32(0))
        if k < win - 1:
            R = R + Lr[..., k]
        prev = wk
    fwin, nr = f32(win), f32(win - 1)
    dm = Ssum / fwin
    rm = R / nr
    xbar = f32(0.5) * (fwin - f32(1))
    E2, XE, R2 = z.copy(), z.copy(), z.copy()
    for k in range(win):
        e = (W[..., k] - p) - dm
        E2 = _fma32(E2, e, e)
        XE = _fma32(XE, np.full_like(e, f32(k) - xbar), e)
        if k < win - 1:
            q = Lr[..., k] - rm
            R2 = _fma32(R2, q, q)
    mean = p + dm
    sxx = fwin * (fwin * fwin - f32(1)) * f32(1.0 / 12.0)
    g, l = G / nr, L / nr
    nvol, nstd = nr, fwin
    if mutant == "sample_std":
        nvol, nstd = max(nr - f32(1), f32(1)), fwin - f32(1)
    out[..., 0] = p / W[..., 0] - f32(1)
    out[..., 1] = np.sqrt(R2 / nvol)
    out[..., 2] = XE / sxx / mean
    if mutant != "slope_no_win":
        out[..., 2] = out[..., 2] * fwin
    out[..., 3] = f32(100) * g / np.maximum(g + l, f32(1e-12))
    out[..., 4] = (Sf / f32(win - kf) - Ss / f32(win - ks)) / p
    out[..., 5] = np.sqrt(E2 / nstd) / np.maximum(mean, f32(1e-9))
    lengths = (np.full(S, T) if lengths is None
               else np.clip(np.asarray(lengths), 0, T))
    out[np.arange(nw)[None] >= (lengths[:, None] - win)] = 0
    return out


# ---------------------------------------------------------------------------
# HMM inputs
# ---------------------------------------------------------------------------
def hmm_inputs(B, T, K, F, seed=0, far=False, clamp_var=False, block=37,
               sep=3.0, tie=False):
    """Planted blocky sequences (state = (t // block) % K, state means
    `sep` sigma apart) and parameters near the truth, as f32 arrays.
    far: the means are shifted so a step's likelihood is about e^-20.
    clamp_var: state 0 has every variance at the 1e-6 clamp and its rows
    sit within 1e-3 of its mean (log-densities near +40).
    tie: every state has the same parameters and uniform transitions."""
    rng = np.random.default_rng([83, B, T, K, F, seed])
    z = (np.arange(T) // block) % K
    X = rng.normal(size=(B, T, F)) + sep * z[None, :, None]
    mu = sep * np.arange(K)[None, :, None] + rng.normal(0, 0.3, (B, K, F))
    var = rng.uniform(0.5, 2.0, (B, K, F))
    A = rng.uniform(0.1, 1.0, (B, K, K)) + 4.0 * np.eye(K)
    A /= A.sum(-1, keepdims=True)
    pi = rng.uniform(0.5, 1.0, (B, K))
    pi /= pi.sum(-1, keepdims=True)
    if far:
        # across the direction the states differ in, so that no other
        # state's mean comes closer
        mu = mu + 2.6 * np.where(np.arange(F) % 2 == 0, 1.0, -1.0)
    if clamp_var:
        var[:, 0] = 1e-6
        rows = z == 0
        X[:, rows] = mu[:, None, 0] + 1e-3 * rng.normal(
            size=(B, int(rows.sum()), F))
    if tie:
        mu[:] = mu[:, :1]
        var[:] = var[:, :1]
        A[:] = 1.0 / K
        pi[:] = 1.0 / K
    return dict(X=X.astype(f32), mu=mu.astype(f32), var=var.astype(f32),
                logA=np.log(A).astype(f32), logpi=np.log(pi).astype(f32),
                z=z)


def params_of(inp, b):
    """Sequence b's parameters as f64 (of the f32 inputs)."""
    return tuple(inp[k][b].astype(np.float64)
                 for k in ("mu", "var", "logA", "logpi"))


# ---------------------------------------------------------------------------
# emissions
# ---------------------------------------------------------------------------
def logb_ref(X, mu, var):
    """(T, F), (K, F) f64 -> logb (T, K) and its envelope: the kernel's
    fma(-0.5, sum_f d^2 / var, -0.5 sum_f log var)."""
    u = U24
    F = X.shape[1]
    d = X[:, None, :] - mu[None]
    term = d * d / var[None]
    q = term.sum(-1)
    # d (twice), d * d, 1 / var, the fma's product side; then the sum
    e_q = (5 + F) * u * q
    lv = np.log(var)
    # v_log_f32 (2 U24), * ln2 and ln2's own rounding; then the sum
    e_hd = 0.5 * (4 + F) * u * np.abs(lv).sum(-1)
    logb = -0.5 * q - 0.5 * lv.sum(-1)[None]
    return logb, 0.5 * e_q + e_hd[None] + u * np.abs(logb)


def _shifted(logb, e_logb):
    """b = exp(logb - max), its relative envelope (without the flush) and
    the shift."""
    u = U24
    mx = logb.max(-1, keepdims=True)
    z = logb - mx
    e_z = e_logb + e_logb.max(-1, keepdims=True) + u * np.abs(z)
    return np.exp(z), e_z + (2 * np.abs(z) + 2) * u, mx[..., 0]


def _exp_param(logp):
    p = np.exp(logp)
    return p, p * (2 * np.abs(logp) + 2) * U24 + F32_MIN


# ---------------------------------------------------------------------------
# E-step references
# ---------------------------------------------------------------------------
def hmm_logspace_ref(X, mu, var, logA, logpi):
    """Free-running log-space forward-backward in f64 (GaussianHMMTorch's
    formulation): dict of ll, alpha (normalised), gamma, xi_sum and the
    statistics."""
    def lse(a, axis):
        m = a.max(axis, keepdims=True)
        return (m + np.log(np.exp(a - m).sum(axis, keepdims=True))
                ).squeeze(axis)

    T, K = X.shape[0], mu.shape[0]
    logb, _ = logb_ref(X, mu, var)
    la = np.empty((T, K))
    lb = np.zeros((T, K))
    la[0] = logpi + logb[0]
    for t in range(1, T):
        la[t] = logb[t] + lse(la[t - 1][:, None] + logA, 0)
    for t in range(T - 2, -1, -1):
        lb[t] = lse(logA + (logb[t + 1] + lb[t + 1])[None], 1)
    ll = lse(la[-1], 0)
    lg = la + lb
    gamma = np.exp(lg - lse(lg, 1)[:, None])
    xi = np.zeros((K, K))
    for t in range(T - 1):
        xi += np.exp(la[t][:, None] + logA
                     + (logb[t + 1] + lb[t + 1])[None] - ll)
    return dict(ll=ll, alpha=np.exp(la - lse(la, 1)[:, None]), gamma=gamma,
                gamma0=gamma[0], gamma_sum=gamma.sum(0),
                gamma_sum_head=gamma[:-1].sum(0), xi_sum=xi,
                sx=gamma.T @ X, sxx=gamma.T @ (X * X))


def estep_forward_ref(X, mu, var, logA, logpi, alpha_k):
    """Teacher-forced forward pass. X (T, F) f64 of the f32 input, alpha_k
    (T, K) the kernel's stored alpha. -> dict of (value, envelope) pairs
    for alpha (T, K), c (T,), and term (T,) = log c_t + shift_t."""
    u = U24
    T, K = alpha_k.shape
    alpha_k = np.asarray(alpha_k, np.float64)
    logb, e_logb = logb_ref(X, mu, var)
    b, rel_b, mx = _shifted(logb, e_logb)
    e_b = b * rel_b + F32_MIN
    A, e_A = _exp_param(logA)
    pi, e_pi = _exp_param(logpi)
    pred = np.empty((T, K))
    e_pred = np.empty((T, K))
    pred[0], e_pred[0] = pi, e_pi
    if T > 1:
        pred[1:] = alpha_k[:-1] @ A
        e_pred[1:] = alpha_k[:-1] @ e_A + (1 + K) * u * pred[1:]
    au = pred * b
    e_au = pred * e_b + b * e_pred + e_pred * e_b + u * au
    c = au.sum(-1)
    e_c = e_au.sum(-1) + K * u * c
    alpha = au / c[:, None]
    e_alpha = (e_au / c[:, None] + au * (e_c / c ** 2)[:, None]
               + 3 * u * alpha + F32_MIN)
    logc = np.log(c)
    term = logc + mx
    e_term = e_c / c + 4 * u * np.abs(logc) + u * np.abs(term)
    return dict(alpha=(alpha, e_alpha), c=(c, e_c), term=(term, e_term))


def hilbert(a, b):
    """Projective distance of two positive vectors per row, components
    floored at 2^-126."""
    r = np.log(np.maximum(a, F32_MIN)) - np.log(np.maximum(b, F32_MIN))
    return r.max(-1) - r.min(-1)


def ll_refs(fwd, free, alpha_k, ll_k):
    """The two log-likelihood checks: [(ref, env)] for the teacher-forced
    sum and for the free-running f64 value."""
    term, e_term = fwd["term"]
    env1 = e_term.sum() + U24 * abs(float(ll_k))
    drift = hilbert(np.asarray(alpha_k, np.float64)[:-1],
                    free["alpha"][:-1]).sum()
    return [(term.sum(), env1), (free["ll"], env1 + drift)]


def estep_backward_ref(X, mu, var, logA, logpi, alpha_k, gamma_k):
    """Anchored backward pass: gamma_t and xi_t from the kernel's own
    alpha and gamma of step t + 1. -> dict of (value, envelope) pairs for
    gamma (T, K), xi_sum (K, K) and the reductions over the kernel's own
    gamma: gamma_sum, gamma_sum_head, sx, sxx."""
    u = U24
    alpha_k = np.asarray(alpha_k, np.float64)
    gamma_k = np.asarray(gamma_k, np.float64)
    T, K = alpha_k.shape
    logb, e_logb = logb_ref(X, mu, var)
    b, rel_b, _ = _shifted(logb, e_logb)
    A = np.exp(logA)
    rel_A = (2 * np.abs(logA) + 2) * u

    gamma = np.empty((T, K))
    e_gamma = np.empty((T, K))
    s = alpha_k[-1].sum()
    gamma[-1] = alpha_k[-1] / s
    e_gamma[-1] = gamma[-1] * (K + 3) * u + F32_MIN
    xi, e_xi = np.zeros((K, K)), np.zeros((K, K))
    if T > 1:
        ok = alpha_k[1:] >= F32_MIN
        safe = np.where(ok, alpha_k[1:], 1.0)
        beta = np.where(ok, gamma_k[1:] / safe, 0.0)        # (T-1, K)
        # what the reconstruction cannot see: a stored gamma below 2^-126
        # is denormal (off by 2^-149), and a state whose stored alpha is
        # denormal or zero is left out. Its beta is at most the largest
        # known one over min A, since beta_j / beta_j' <= max_k A_jk / A_j'k
        lost = np.where(ok, 2.0 ** -149 / safe,
                        beta.max(-1, keepdims=True) / A.min())
        w = A[None] * (b[1:] * beta)[:, None, :]            # (T-1, i, j)
        w_lost = A[None] * (b[1:] * lost)[:, None, :]
        rel = rel_A[None] + rel_b[1:, None, :]
        br = w.sum(-1)
        gu = alpha_k[:-1] * br
        # beta's reconstruction (3), b * beta, A *, rcp (2) and its product,
        # the sum over j (K), alpha *
        e_gu = (alpha_k[:-1] * ((w * rel).sum(-1) + w_lost.sum(-1))
                + gu * (9 + K) * u)
        g = gu.sum(-1)
        e_g = e_gu.sum(-1) + K * u * g
        gamma[:-1] = gu / g[:, None]
        # results below 2^-126 are denormal or flushed: an absolute 2^-126
        e_gamma[:-1] = (e_gu / g[:, None] + gu * (e_g / g ** 2)[:, None]
                        + 2 * u * gamma[:-1] + F32_MIN)
        xt = alpha_k[:-1, :, None] * w / g[:, None, None]
        e_xt = (xt * (rel + 10 * u + (e_g / g)[:, None, None])
                + alpha_k[:-1, :, None] * w_lost / g[:, None, None])
        xi = xt.sum(0)
        e_xi = e_xt.sum(0) + (T - 1) * (u * xi + F32_MIN)
    gx = np.abs(gamma_k.T @ np.abs(X))
    gxx = gamma_k.T @ (X * X)
    return dict(
        gamma=(gamma, e_gamma), xi_sum=(xi, e_xi),
        gamma_sum=(gamma_k.sum(0), T * (u * gamma_k.sum(0) + F32_MIN)),
        gamma_sum_head=(gamma_k[:-1].sum(0),
                        T * (u * gamma_k[:-1].sum(0) + F32_MIN)),
        sx=(gamma_k.T @ X, (2 + T) * (u * gx + F32_MIN)),
        sxx=(gxx, (3 + T) * (u * gxx + F32_MIN)))


def gamma_chain_env(fwd, bwd, free):
    """Chain-mode envelope of gamma (T, K) against the free-running
    reference `free`: gamma_t (exp(D_t) - 1), see the module docstring."""
    a, e_a = fwd["alpha"]
    g, e_g = bwd["gamma"]
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = np.where(a > ALPHA_FLOOR, e_a / a, 0).max(-1)
        rg = np.where(g > ALPHA_FLOOR, e_g / g, 0).max(-1)
    D = 2 * np.cumsum(ra) + 2 * np.cumsum(rg[::-1])[::-1]
    return free["gamma"] * np.expm1(D)[:, None] + F32_MIN


def estep_ratios(inp, got, b=0, T=None):
    """Worst error / envelope of every E-step output of sequence b of
    hmm_inputs' `inp`; `got` holds that sequence's (T, ...) slices and
    statistics. gamma0 must be gamma[0] bit for bit."""
    T = T or inp["X"].shape[1]
    X = inp["X"][b, :T].astype(np.float64)
    prm = params_of(inp, b)
    fwd = estep_forward_ref(X, *prm, got["alpha"])
    bwd = estep_backward_ref(X, *prm, got["alpha"], got["gamma"])
    free = hmm_logspace_ref(X, *prm)
    out = {k: worst(got[k], *fwd[k]) for k in ("alpha", "c")}
    out.update({k: worst(got[k], *bwd[k]) for k in (
        "gamma", "xi_sum", "gamma_sum", "gamma_sum_head", "sx", "sxx")})
    out["gamma0"] = 0.0 if np.array_equal(
        np.asarray(got["gamma0"]), np.asarray(got["gamma"])[0]) else np.inf
    for name, (ref, env) in zip(("ll_forced", "ll_free"), ll_refs(
            fwd, free, got["alpha"], got["ll"])):
        out[name] = worst(got["ll"], ref, env)
    if T <= HMM_CHAIN_MAX_T:
        out["gamma_chain"] = worst(
            got["gamma"], free["gamma"], gamma_chain_env(fwd, bwd, free))
    return out


# ---------------------------------------------------------------------------
# E-step emulation
# ---------------------------------------------------------------------------
def _bfly(v, op):
    """An 8-lane xor butterfly (offsets 1, 2, 4) in f32: what the kernel's
    __shfl_xor reductions compute, in their order."""
    idx = np.arange(8)
    for off in (1, 2, 4):
        v = op(v, v[idx ^ off]).astype(f32)
    return v[0]


def _pad8(v, fill=0.0):
    out = np.full(8, fill, f32)
    out[:len(v)] = v
    return out


def _emu_emission(mu, var):
    iv = (f32(1) / var).astype(f32)
    ld = np.zeros(len(mu), f32)
    for f in range(mu.shape[1]):
        ld = ld + (np.log2(var[:, f]).astype(f32) * LN2_32).astype(f32)
    return iv, (f32(-0.5) * ld).astype(f32)


def _emu_logb(x, mu, iv, hd):
    q = np.zeros(len(mu), f32)
    for f in range(mu.shape[1]):
        d = (x[f] - mu[:, f]).astype(f32)
        q = _fma32(q, (d * d).astype(f32), iv[:, f])
    return (f32(-0.5) * q + hd).astype(f32)


def _emu_exp(z):
    return np.exp2((z * LOG2E32).astype(f32)).astype(f32)


def hmm_estep_emulate(X, mu, var, logA, logpi, mutant=None):
    """One sequence through the kernel's f32 arithmetic (f32 inputs)."""
    X, mu, var = (np.asarray(v, f32) for v in (X, mu, var))
    logA, logpi = np.asarray(logA, f32), np.asarray(logpi, f32)
    T, K = X.shape[0], mu.shape[0]
    iv, hd = _emu_emission(mu, var)
    A = _emu_exp(logA)
    tiny = f32(F32_MIN)

    def shifted_b(t):
        lb = _emu_logb(X[t], mu, iv, hd)
        mx = f32(0) if mutant == "no_shift" else _bfly(
            _pad8(lb, -np.inf), np.maximum)
        return _emu_exp((lb - mx).astype(f32)), mx

    def sum_i(M):                       # (K, K) -> sum over rows, per column
        P = np.zeros((8, 8), f32)
        P[:K, :K] = M
        return np.array([_bfly(P[:, j], np.add) for j in range(K)], f32)

    alpha = np.zeros((T, K), f32)
    c = np.zeros(T, f32)
    ll = 0.0
    a = np.zeros(K, f32)
    with np.errstate(all="ignore"):
        for t in range(T):
            bj, mx = shifted_b(t)
            pred = _emu_exp(logpi) if t == 0 else sum_i(a[:, None] * A)
            au = (pred * bj).astype(f32)
            ct = max(_bfly(_pad8(au), np.add), tiny)
            a = (au * (f32(1) / ct)).astype(f32)
            ll += float(f32(f32(np.log2(ct)) * LN2_32) + mx)
            alpha[t], c[t] = a, ct

        gamma = np.zeros((T, K), f32)
        xi = np.zeros((K, K), f32)
        gs, gh = np.zeros(K, f32), np.zeros(K, f32)
        ax = np.zeros((K, X.shape[1]), f32)
        axx = np.zeros_like(ax)

        def take(t, gam, head):
            nonlocal gs, gh, ax, axx
            gs = gs + gam
            if head:
                gh = gh + gam
            ax = _fma32(ax, gam[:, None], X[t][None])
            axx = _fma32(axx, (gam[:, None] * X[t][None]).astype(f32),
                         X[t][None])
            gamma[t] = gam

        at = alpha[T - 1]
        gam = (at / max(_bfly(_pad8(at), np.add), tiny)).astype(f32)
        take(T - 1, gam, mutant == "head_with_last")
        bc = np.ones(K, f32)
        for t in range(T - 1, 0, -1):
            bj, _ = shifted_b(t)
            rc = f32(1) / c[t]
            w = ((A * (bj * bc).astype(f32)[None]).astype(f32)
                 * rc).astype(f32)
            P = np.zeros((8, 8), f32)
            P[:K, :K] = w
            br = np.array([_bfly(P[i], np.add) for i in range(K)], f32)
            ap = alpha[t - 1]
            gu = (ap * br).astype(f32)
            rg = f32(1) / max(_bfly(_pad8(gu), np.add), tiny)
            gam = (gu * rg).astype(f32)
            lead = alpha[t] if mutant == "xi_alpha_next" else ap
            xi = _fma32(xi, (lead[:, None] * w).astype(f32),
                        np.full_like(w, rg))
            take(t - 1, gam, True)
            bc = br
    return dict(ll=f32(ll), alpha=alpha, c=c, gamma=gamma, gamma0=gamma[0],
                gamma_sum=gs, gamma_sum_head=gh, xi_sum=xi, sx=ax, sxx=axx)


def forward_unscaled_f32(X, mu, var, logA, logpi):
    """A raw-probability f32 forward pass; returns the first step at which
    it holds a zero row or a non-finite value (T if none)."""
    X, mu, var = (np.asarray(v, f32) for v in (X, mu, var))
    iv, hd = _emu_emission(mu, var)
    A = _emu_exp(np.asarray(logA, f32))
    a = None
    with np.errstate(all="ignore"):
        for t in range(X.shape[0]):
            bj = _emu_exp(_emu_logb(X[t], mu, iv, hd))
            a = ((_emu_exp(np.asarray(logpi, f32)) if t == 0
                  else (a @ A).astype(f32)) * bj).astype(f32)
            if not np.isfinite(a).all() or a.sum() == 0:
                return t
    return X.shape[0]


# ---------------------------------------------------------------------------
# Viterbi
# ---------------------------------------------------------------------------
def path_score(path, X, mu, var, logA, logpi):
    """The joint log-probability of a state path, in f64."""
    logb, _ = logb_ref(X, mu, var)
    path = np.asarray(path)
    t = np.arange(len(path))
    return float(logpi[path[0]] + logb[t, path].sum()
                 + logA[path[:-1], path[1:]].sum())


def viterbi_ref(X, mu, var, logA, logpi):
    """-> (f64 path with ties to the lowest state, its score, envelope
    2 E of a kernel path's score)."""
    u = U24
    T, K = X.shape[0], mu.shape[0]
    logb, e_logb = logb_ref(X, mu, var)
    back = np.zeros((T, K), np.int64)
    delta = logpi + logb[0]
    E = e_logb[0].max() + 2 * u * np.abs(delta).max()
    delta = delta - delta.max()
    amax = np.abs(logA).max()
    for t in range(1, T):
        spread = -delta.min()
        s = delta[:, None] + logA
        back[t] = s.argmax(0)
        delta = s.max(0) + logb[t]
        # the three additions of a step, each on values of this size
        E += e_logb[t].max() + u * (3 * (spread + amax)
                                    + 2 * np.abs(logb[t]).max())
        delta = delta - delta.max()
    path = np.empty(T, np.int64)
    path[-1] = delta.argmax()
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path, path_score(path, X, mu, var, logA, logpi), 2 * E


def viterbi_emulate(X, mu, var, logA, logpi, mutant=None):
    """The kernel's f32 max-plus recursion; mutant "tie_high" sends ties
    to the highest state."""
    X, mu, var = (np.asarray(v, f32) for v in (X, mu, var))
    logA, logpi = np.asarray(logA, f32), np.asarray(logpi, f32)
    T, K = X.shape[0], mu.shape[0]
    iv, hd = _emu_emission(mu, var)

    def argbest(v, axis):
        if mutant == "tie_high":
            n = v.shape[axis]
            return n - 1 - np.flip(v, axis).argmax(axis)
        return v.argmax(axis)

    back = np.zeros((T, K), np.int64)
    delta = (logpi + _emu_logb(X[0], mu, iv, hd)).astype(f32)
    delta = (delta - delta.max()).astype(f32)
    for t in range(1, T):
        s = (delta[:, None] + logA).astype(f32)
        back[t] = argbest(s, 0)
        delta = (s.max(0) + _emu_logb(X[t], mu, iv, hd)).astype(f32)
        delta = (delta - delta.max()).astype(f32)
    path = np.empty(T, np.int64)
    path[-1] = argbest(delta, 0)
    for t in range(T - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    return path
