"""Market-regime ops: window features, the Gaussian-HMM E-step / M-step and
Viterbi for B sequences at once (ops/hip/regime.hip; the math of
services/market_regime.py::extract_features and GaussianHMMTorch).

Each op has a numpy CPU twin, vectorised over the batch, and a GPU wrapper
over require_hip_ops(). Sequences are padded to a common Tmax and carry
their own `lengths`; the HMM parameters are per sequence:

    mu, var (B, K, F)   logA (B, K, K)   logpi (B, K)      K, F <= 8

E-step statistics (a dict, numpy or torch alike):

    ll (B,)  gamma0 (B, K)  gamma_sum (B, K)  gamma_sum_head (B, K)
    xi_sum (B, K, K)  sx (B, K, F)  sxx (B, K, F)
    alpha (B, Tmax, K)  c (B, Tmax)         the scaled forward pass
    gamma (B, Tmax, K)                      on request, 0 past lengths[b]

The forward pass is the scaled (Rabiner) recursion with each step's
emission log-densities shifted by their max over states, so c_t is the
scale of the shifted step and ll = sum_t (log c_t + shift_t).
"""

from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from . import require_hip_ops

N_FEATURES = 6
MIN_WIN, MAX_WIN = 2, 256
MAX_K = MAX_F = 8
STAT_KEYS = ("ll", "gamma0", "gamma_sum", "gamma_sum_head", "xi_sum", "sx",
             "sxx")
_TINY = float(np.finfo(np.float32).tiny)


def _check_win(win: int):
    if not MIN_WIN <= win <= MAX_WIN:
        raise RuntimeError(
            f"regime_features: win must be in [{MIN_WIN}, {MAX_WIN}], "
            f"got {win}")


def _check_kf(K: int, F: int):
    if not (1 <= K <= MAX_K and 1 <= F <= MAX_F):
        raise RuntimeError(
            f"hmm: needs 1 <= K <= {MAX_K} and 1 <= F <= {MAX_F}, "
            f"got K={K} F={F}")


# ---------------------------------------------------------------------------
# features
# ---------------------------------------------------------------------------
def regime_features_cpu(closes: np.ndarray, lengths=None,
                        win: int = 32) -> np.ndarray:
    """(S, Tmax) closes -> (S, Tmax - win, 6) f32, extract_features per
    symbol in closed form over sliding windows; rows at or past
    lengths[s] - win are 0. A 1-D input is one symbol."""
    _check_win(win)
    c = np.asarray(closes, np.float64)
    if c.ndim == 1:
        c = c[None]
    S, Tmax = c.shape
    nw = max(Tmax - win, 0)
    out = np.zeros((S, nw, N_FEATURES), np.float32)
    if nw == 0:
        return out
    lengths = (np.full(S, Tmax) if lengths is None
               else np.clip(np.asarray(lengths), 0, Tmax))
    valid = np.arange(nw)[None] < (lengths[:, None] - win)       # (S, nw)
    # padding must not poison the valid rows' neighbours with log(0)
    safe = np.where(np.arange(Tmax)[None] < lengths[:, None], c, 1.0)
    W = sliding_window_view(safe, win, axis=1)[:, :nw]           # (S,nw,win)
    lr = np.diff(np.log(safe), axis=1)
    with np.errstate(all="ignore"):
        mean = W.mean(-1)
        feats = np.empty((S, nw, N_FEATURES))
        feats[..., 0] = W[..., -1] / W[..., 0] - 1.0
        if win > 2:
            feats[..., 1] = sliding_window_view(
                lr, win - 1, axis=1)[:, :nw].std(-1)
        else:
            feats[..., 1] = 0.0
        x = np.arange(win) - 0.5 * (win - 1)
        sxx = win * (win * win - 1.0) / 12.0
        feats[..., 2] = ((W - mean[..., None]) @ x) / sxx / mean * win
        d = np.diff(W, axis=-1)
        g = np.maximum(d, 0).mean(-1)
        l = np.maximum(-d, 0).mean(-1)
        feats[..., 3] = 100 * g / np.maximum(g + l, 1e-12)
        slow = W[..., -26:].mean(-1) if win >= 26 else mean
        feats[..., 4] = (W[..., -12:].mean(-1) - slow) / W[..., -1]
        feats[..., 5] = W.std(-1) / np.maximum(mean, 1e-9)
    out[valid] = feats[valid]
    return out


def regime_features_gpu(closes, lengths=None, win: int = 32, out=None):
    """closes (S, Tmax) f32 cuda, lengths (S,) i32 cuda (default: all Tmax)
    -> (S, Tmax - win, 6) f32. `out`: a preallocated contiguous buffer of
    at least that many elements to write into."""
    import torch

    _check_win(win)
    ops = require_hip_ops()
    assert closes.is_cuda and closes.dtype == torch.float32
    if closes.dim() == 1:
        closes = closes[None]
    closes = closes.contiguous()
    S, Tmax = closes.shape
    nw = max(Tmax - win, 0)
    if lengths is None:
        lengths = torch.full((S,), Tmax, dtype=torch.int32,
                             device=closes.device)
    lengths = lengths.to(device=closes.device,
                         dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty(S * nw * N_FEATURES, dtype=torch.float32,
                          device=closes.device)
    assert out.is_contiguous() and out.numel() >= S * nw * N_FEATURES
    if nw > 0 and S > 0:
        stream = torch.cuda.current_stream(closes.device).cuda_stream
        ops.regime_features(closes.data_ptr(), lengths.data_ptr(),
                            out.data_ptr(), S, Tmax, win, stream)
    return out.view(-1)[:S * nw * N_FEATURES].view(S, nw, N_FEATURES)


# ---------------------------------------------------------------------------
# HMM, CPU twins
# ---------------------------------------------------------------------------
def _emission_logb(X, mu, var):
    """(B, T, F), (B, K, F) -> (B, T, K) diagonal-Gaussian log-densities
    (without the constant -F/2 log 2 pi, as GaussianHMMTorch)."""
    d = X[:, :, None, :] - mu[:, None]
    return (-0.5 * ((d * d) / var[:, None]).sum(-1)
            - 0.5 * np.log(var).sum(-1)[:, None])


def _prep(X, lengths, mu, var, logA, logpi, dtype):
    X = np.asarray(X, dtype)
    if X.ndim == 2:
        X = X[None]
    B, Tmax, F = X.shape
    mu = np.asarray(mu, dtype).reshape(B, -1, F)
    K = mu.shape[1]
    _check_kf(K, F)
    var = np.asarray(var, dtype).reshape(B, K, F)
    logA = np.asarray(logA, dtype).reshape(B, K, K)
    logpi = np.asarray(logpi, dtype).reshape(B, K)
    lengths = (np.full(B, Tmax) if lengths is None
               else np.clip(np.asarray(lengths), 0, Tmax)).astype(np.int64)
    return X, lengths, mu, var, logA, logpi, B, Tmax, K, F


def hmm_estep_cpu(X, lengths, mu, var, logA, logpi, want_gamma=False,
                  dtype=np.float64) -> dict:
    """One E-step for B sequences, the kernel's recursion in `dtype`."""
    X, lengths, mu, var, logA, logpi, B, Tmax, K, F = _prep(
        X, lengths, mu, var, logA, logpi, dtype)
    tiny = dtype(_TINY)
    with np.errstate(all="ignore"):
        logb = _emission_logb(X, mu, var)
        shift = logb.max(-1)                                 # (B, T)
        bs = np.exp(logb - shift[..., None])                 # (B, T, K)
        A = np.exp(logA)
        alpha = np.zeros((B, Tmax, K), dtype)
        c = np.ones((B, Tmax), dtype)
        ll = np.zeros(B, np.float64)
        a = np.zeros((B, K), dtype)
        for t in range(Tmax):
            live = t < lengths
            if not live.any():
                break
            pred = (np.exp(logpi) if t == 0
                    else np.einsum("bi,bij->bj", a, A))
            au = pred * bs[:, t]
            ct = np.maximum(au.sum(-1), tiny)
            an = au / ct[:, None]
            a = np.where(live[:, None], an, a)
            alpha[live, t] = an[live]
            c[live, t] = ct[live]
            ll[live] += (np.log(ct) + shift[:, t])[live]

        gamma = np.zeros((B, Tmax, K), dtype)
        xi = np.zeros((B, K, K), dtype)
        beta = np.ones((B, K), dtype)
        for t in range(Tmax - 1, -1, -1):
            last = t == lengths - 1
            inner = t < lengths - 1
            if not (last | inner).any():
                continue
            if inner.any():
                # w[i, j] = A[i, j] b_{t+1}[j] beta_{t+1}[j] / c_{t+1}
                w = A * (bs[:, t + 1] * beta / c[:, t + 1, None])[:, None]
                br = w.sum(-1)
                gu = alpha[:, t] * br
                rg = 1.0 / np.maximum(gu.sum(-1), tiny)
                xi += np.where(inner[:, None, None],
                               alpha[:, t, :, None] * w
                               * rg[:, None, None], 0)
                gamma[inner, t] = (gu * rg[:, None])[inner]
                beta = np.where(inner[:, None], br, beta)
            if last.any():
                al = alpha[:, t]
                gl = al / np.maximum(al.sum(-1), tiny)[:, None]
                gamma[last, t] = gl[last]
        idx = np.maximum(lengths - 1, 0)
        g_last = np.where((lengths > 0)[:, None],
                          gamma[np.arange(B), idx], 0)
        gsum = gamma.sum(1)
    out = {
        "ll": ll.astype(dtype), "gamma0": gamma[:, 0].copy(),
        "gamma_sum": gsum, "gamma_sum_head": gsum - g_last,
        "xi_sum": xi,
        "sx": np.einsum("btk,btf->bkf", gamma, X),
        "sxx": np.einsum("btk,btf->bkf", gamma, X * X),
        "alpha": alpha, "c": c,
    }
    if want_gamma:
        out["gamma"] = gamma
    return out


def hmm_viterbi_cpu(X, lengths, mu, var, logA, logpi,
                    dtype=np.float64) -> np.ndarray:
    """Viterbi paths (B, Tmax) i32, -1 past lengths[b]; ties go to the
    lowest state index."""
    X, lengths, mu, var, logA, logpi, B, Tmax, K, F = _prep(
        X, lengths, mu, var, logA, logpi, dtype)
    path = np.full((B, Tmax), -1, np.int32)
    if Tmax == 0:
        return path
    with np.errstate(all="ignore"):
        logb = _emission_logb(X, mu, var)
        back = np.zeros((B, Tmax, K), np.int64)
        delta = logpi + logb[:, 0]
        delta = delta - delta.max(-1, keepdims=True)
        final = delta.copy()
        for t in range(1, Tmax):
            s = delta[:, :, None] + logA                     # (B, i, j)
            back[:, t] = s.argmax(1)
            delta = s.max(1) + logb[:, t]
            delta = delta - delta.max(-1, keepdims=True)
            live = t < lengths
            final = np.where(live[:, None], delta, final)
    state = final.argmax(-1)
    rows = np.arange(B)
    for t in range(Tmax - 1, -1, -1):
        on = t < lengths
        path[on, t] = state[on]
        state = np.where(on & (t >= 1), back[rows, t, state], state)
    return path


def hmm_mstep(stats: dict) -> dict:
    """GaussianHMMTorch.fit's M-step on batched statistics (torch tensors
    or numpy arrays alike): its +1e-9, +1e-12 and the 1e-6 variance clamp."""
    xi, g0 = stats["xi_sum"], stats["gamma0"]
    is_torch = hasattr(xi, "clamp")
    logf = (lambda v: v.log()) if is_torch else np.log
    logA = logf(xi / (stats["gamma_sum_head"][..., None] + 1e-9) + 1e-12)
    logpi = logf(g0 + 1e-12)
    nk = (stats["gamma_sum"] + 1e-9)[..., None]
    mu = stats["sx"] / nk
    var = stats["sxx"] / nk - mu * mu
    var = var.clamp(min=1e-6) if is_torch else np.maximum(var, 1e-6)
    return {"mu": mu, "var": var, "logA": logA, "logpi": logpi}


# ---------------------------------------------------------------------------
# HMM, GPU wrappers
# ---------------------------------------------------------------------------
def _prep_gpu(X, lengths, mu, var, logA, logpi):
    import torch

    assert X.is_cuda and X.dtype == torch.float32
    if X.dim() == 2:
        X = X[None]
    B, Tmax, F = X.shape
    K = mu.shape[-2]
    _check_kf(K, F)
    dev = X.device

    def f32(t, shape):
        t = t.to(device=dev, dtype=torch.float32).reshape(shape)
        return t.contiguous()

    if lengths is None:
        lengths = torch.full((B,), Tmax, dtype=torch.int32, device=dev)
    lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
    assert lengths.numel() == B
    return (X.contiguous(), lengths, f32(mu, (B, K, F)), f32(var, (B, K, F)),
            f32(logA, (B, K, K)), f32(logpi, (B, K)), B, Tmax, K, F)


def _buffer(buffers, name, shape, dtype, dev):
    """A view of shape `shape` on buffers[name] (a flat preallocated
    tensor), or a fresh tensor."""
    import torch

    n = int(np.prod(shape))
    if buffers is not None and name in buffers:
        buf = buffers[name]
        assert buf.is_contiguous() and buf.dtype == dtype \
            and buf.numel() >= n, name
        return buf.view(-1)[:n].view(shape)
    return torch.empty(shape, dtype=dtype, device=dev)


def hmm_estep_gpu(X, lengths, mu, var, logA, logpi, want_gamma=False,
                  buffers: dict | None = None) -> dict:
    """One E-step for B sequences in one launch (hmm_estep_kernel). All
    arguments are cuda tensors; returns the statistics dict of the module
    docstring as f32 cuda tensors. `buffers` maps output names to flat
    preallocated tensors to write into."""
    import torch

    ops = require_hip_ops()
    X, lengths, mu, var, logA, logpi, B, Tmax, K, F = _prep_gpu(
        X, lengths, mu, var, logA, logpi)
    dev, f32 = X.device, torch.float32
    shapes = {"ll": (B,), "gamma0": (B, K), "gamma_sum": (B, K),
              "gamma_sum_head": (B, K), "xi_sum": (B, K, K),
              "sx": (B, K, F), "sxx": (B, K, F), "alpha": (B, Tmax, K),
              "c": (B, Tmax)}
    if want_gamma:
        shapes["gamma"] = (B, Tmax, K)
    out = {k: _buffer(buffers, k, s, f32, dev) for k, s in shapes.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    ops.hmm_estep(
        X.data_ptr(), lengths.data_ptr(), mu.data_ptr(), var.data_ptr(),
        logA.data_ptr(), logpi.data_ptr(), out["alpha"].data_ptr(),
        out["c"].data_ptr(), out["ll"].data_ptr(), out["gamma0"].data_ptr(),
        out["gamma_sum"].data_ptr(), out["gamma_sum_head"].data_ptr(),
        out["xi_sum"].data_ptr(), out["sx"].data_ptr(),
        out["sxx"].data_ptr(),
        out["gamma"].data_ptr() if want_gamma else 0, B, Tmax, K, F, stream)
    return out


def hmm_viterbi_gpu(X, lengths, mu, var, logA, logpi,
                    buffers: dict | None = None):
    """Viterbi paths (B, Tmax) i32 cuda, -1 past lengths[b], in one launch
    (hmm_viterbi_kernel, backtrack included)."""
    import torch

    ops = require_hip_ops()
    X, lengths, mu, var, logA, logpi, B, Tmax, K, F = _prep_gpu(
        X, lengths, mu, var, logA, logpi)
    dev = X.device
    bp = _buffer(buffers, "bp", (B, Tmax, K), torch.uint8, dev)
    path = _buffer(buffers, "path", (B, Tmax), torch.int32, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ops.hmm_viterbi(X.data_ptr(), lengths.data_ptr(), mu.data_ptr(),
                    var.data_ptr(), logA.data_ptr(), logpi.data_ptr(),
                    bp.data_ptr(), path.data_ptr(), B, Tmax, K, F, stream)
    return path
