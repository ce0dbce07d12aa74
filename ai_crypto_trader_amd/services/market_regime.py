"""Market regime service (reference parity:
services/market_regime_service.py + services/utils/market_regime_detector.py).

Features per window: return, volatility, trend strength (rolling slope),
RSI, MACD, BB width (market_regime_detector.py:64-110). Detectors: KMeans
/ GMM / Gaussian HMM (torch, GPU-capable) and the reference's heuristic
cluster->label
mapping by mean return & volatility (:226-296), plus the rule-based
fallback (market_regime_service.py:503-604). Publishes `strategy_switch`
on regime changes; maintains `current_market_regime` /
`market_regime_history` keys.

For the whole universe: `detect_many` runs the features, the HMM's
Baum-Welch and Viterbi for every symbol at once (kmeans_many,
GaussianHMMBatched over ops/regime.py's HIP kernels or their numpy twins);
with `regime.per_symbol` the loop also maintains `market_regimes`."""

from __future__ import annotations

import time

import numpy as np
import torch

from ..bus.schema import Channels, Keys, StrategySwitch
from .base import Service

REGIMES = ("bull", "bear", "ranging", "volatile")


def extract_features(closes: np.ndarray, win: int = 32) -> np.ndarray:
    """(T,) closes -> (n_win, 6) features [ret, vol, slope, rsi, macd, bbw]
    over trailing windows (market_regime_detector.py:64-110 semantics)."""
    T = len(closes)
    n = T - win
    if n <= 0:
        return np.zeros((0, 6), np.float32)
    out = np.zeros((n, 6), np.float32)
    lr = np.diff(np.log(closes))
    for i in range(n):
        w = closes[i:i + win]
        r = lr[i:i + win - 1]
        out[i, 0] = w[-1] / w[0] - 1.0
        out[i, 1] = r.std()
        x = np.arange(win)
        out[i, 2] = np.polyfit(x, w / w.mean(), 1)[0] * win
        g = np.maximum(np.diff(w), 0).mean()
        l = np.maximum(-np.diff(w), 0).mean()
        out[i, 3] = 100 * g / max(g + l, 1e-12)
        ema_f = w[-12:].mean()
        ema_s = w[-26:].mean() if win >= 26 else w.mean()
        out[i, 4] = (ema_f - ema_s) / w[-1]
        out[i, 5] = w.std() / max(w.mean(), 1e-9)
    return out


class KMeansTorch:
    """Plain torch KMeans (runs on GPU when tensors are cuda) — the
    detector's default model (market_regime_detector.py:138)."""

    def __init__(self, k: int = 4, iters: int = 50, seed: int = 0):
        self.k = k
        self.iters = iters
        self.seed = seed
        self.centers: torch.Tensor | None = None

    def fit(self, X: torch.Tensor):
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        idx = torch.randperm(X.shape[0], generator=g)[: self.k]
        self.centers = X[idx.to(X.device)].clone()
        for _ in range(self.iters):
            d = torch.cdist(X, self.centers)
            assign = d.argmin(dim=1)
            for c in range(self.k):
                m = assign == c
                if m.any():
                    self.centers[c] = X[m].mean(dim=0)
        return self

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        return torch.cdist(X, self.centers).argmin(dim=1)


class GMMTorch:
    """Diagonal-covariance GMM via EM (market_regime_detector.py:144)."""

    def __init__(self, k: int = 4, iters: int = 60, seed: int = 0):
        self.k = k
        self.iters = iters
        self.seed = seed

    def fit(self, X: torch.Tensor):
        km = KMeansTorch(self.k, 20, self.seed).fit(X)
        self.mu = km.centers.clone()
        self.var = torch.ones_like(self.mu) * X.var(dim=0, keepdim=True)
        self.pi = torch.full((self.k,), 1.0 / self.k, device=X.device)
        for _ in range(self.iters):
            logp = self._log_prob(X)                       # (N, k)
            logr = logp - torch.logsumexp(logp, dim=1, keepdim=True)
            r = logr.exp()
            nk = r.sum(dim=0) + 1e-9
            self.mu = (r.T @ X) / nk[:, None]
            self.var = (r.T @ (X ** 2)) / nk[:, None] - self.mu ** 2
            self.var = torch.clamp(self.var, min=1e-8)
            self.pi = nk / nk.sum()
        return self

    def _log_prob(self, X):
        d = X[:, None, :] - self.mu[None]
        return (torch.log(self.pi)[None]
                - 0.5 * ((d ** 2) / self.var[None]).sum(-1)
                - 0.5 * torch.log(self.var[None]).sum(-1))

    def predict(self, X):
        return self._log_prob(X).argmax(dim=1)

    def predict_proba(self, X):
        lp = self._log_prob(X)
        return (lp - torch.logsumexp(lp, 1, keepdim=True)).exp()


class GaussianHMMTorch:
    """Diagonal-covariance Gaussian HMM via Baum-Welch EM, log-space
    forward-backward (market_regime_detector.py:150 — hmmlearn GaussianHMM
    equivalent; data is tiny so a per-timestep torch loop is fine)."""

    def __init__(self, k: int = 4, iters: int = 30, seed: int = 0):
        self.k = k
        self.iters = iters
        self.seed = seed

    def _emission_logp(self, X):
        d = X[:, None, :] - self.mu[None]                    # (T, k, F)
        return (-0.5 * ((d ** 2) / self.var[None]).sum(-1)
                - 0.5 * torch.log(self.var[None]).sum(-1))

    def fit(self, X: torch.Tensor):
        T = X.shape[0]
        k = self.k
        km = KMeansTorch(k, 20, self.seed).fit(X)
        self.mu = km.centers.clone()
        self.var = torch.ones_like(self.mu) * X.var(dim=0, keepdim=True)
        self.var = torch.clamp(self.var, min=1e-6)
        dev = X.device
        # sticky prior: regimes persist (diag-heavy transition init)
        self.logA = torch.log(torch.full((k, k), 0.05 / (k - 1), device=dev)
                              .fill_diagonal_(0.95))
        self.logpi = torch.full((k,), -np.log(k), device=dev)
        for _ in range(self.iters):
            logb = self._emission_logp(X)                    # (T, k)
            # forward / backward in log space
            la = torch.empty(T, k, device=dev)
            lb = torch.zeros(T, k, device=dev)
            la[0] = self.logpi + logb[0]
            for t in range(1, T):
                la[t] = logb[t] + torch.logsumexp(
                    la[t - 1][:, None] + self.logA, dim=0)
            for t in range(T - 2, -1, -1):
                lb[t] = torch.logsumexp(
                    self.logA + (logb[t + 1] + lb[t + 1])[None], dim=1)
            lg = la + lb
            lg = lg - torch.logsumexp(lg, dim=1, keepdim=True)
            g = lg.exp()                                     # (T, k) gammas
            # xi sums for the transition update
            xi = torch.zeros(k, k, device=dev)
            ll = torch.logsumexp(la[-1], dim=0)
            for t in range(T - 1):
                lx = (la[t][:, None] + self.logA
                      + (logb[t + 1] + lb[t + 1])[None] - ll)
                xi += lx.exp()
            self.logA = torch.log(xi / (g[:-1].sum(0)[:, None] + 1e-9)
                                  + 1e-12)
            self.logpi = torch.log(g[0] + 1e-12)
            nk = g.sum(0) + 1e-9
            self.mu = (g.T @ X) / nk[:, None]
            self.var = torch.clamp(
                (g.T @ (X ** 2)) / nk[:, None] - self.mu ** 2, min=1e-6)
        return self

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """Viterbi path."""
        T = X.shape[0]
        logb = self._emission_logp(X)
        delta = self.logpi + logb[0]
        back = torch.zeros(T, self.k, dtype=torch.long, device=X.device)
        for t in range(1, T):
            s = delta[:, None] + self.logA
            best = s.max(dim=0)
            delta = best.values + logb[t]
            back[t] = best.indices
        path = torch.empty(T, dtype=torch.long, device=X.device)
        path[-1] = delta.argmax()
        for t in range(T - 2, -1, -1):
            path[t] = back[t + 1, path[t + 1]]
        return path


def kmeans_many(X: torch.Tensor, lengths, k: int = 4, iters: int = 20,
                seed: int = 0) -> torch.Tensor:
    """KMeansTorch for B padded sequences at once: X (B, N, F), lengths
    (B,) -> centres (B, k, F). Seeded per sequence like KMeansTorch
    (randperm(n) from a CPU generator at `seed`); an empty cluster keeps
    its centre. Every sequence needs at least k rows."""
    B, N, F = X.shape
    lengths = torch.as_tensor(lengths, device=X.device).long()
    assert int(lengths.min()) >= k, "kmeans_many: a sequence has < k rows"
    idx = torch.stack([
        torch.randperm(int(n), generator=torch.Generator(
            device="cpu").manual_seed(seed))[:k]
        for n in lengths.tolist()]).to(X.device)                  # (B, k)
    centers = torch.gather(X, 1, idx[:, :, None].expand(B, k, F)).clone()
    valid = torch.arange(N, device=X.device)[None] < lengths[:, None]
    for _ in range(iters):
        assign = torch.cdist(X, centers).argmin(dim=2)            # (B, N)
        onehot = (torch.nn.functional.one_hot(assign, k)
                  * valid[:, :, None]).to(X.dtype)                # (B, N, k)
        count = onehot.sum(1)                                     # (B, k)
        mean = (onehot.transpose(1, 2) @ X) / count.clamp(min=1)[:, :, None]
        centers = torch.where((count > 0)[:, :, None], mean, centers)
    return centers


class GaussianHMMBatched:
    """GaussianHMMTorch for B sequences at once: the same init (KMeans
    centres, global variance, sticky 0.95 transitions) and M-step, with the
    E-step and Viterbi as one HIP launch each on cuda tensors
    (ops/regime.py::hmm_estep_gpu / hmm_viterbi_gpu) and their numpy twins
    otherwise. Parameters are per sequence: mu, var (B, k, F), logA
    (B, k, k), logpi (B, k); `ll_history` holds the (B,) log-likelihood
    of every EM iteration."""

    def __init__(self, k: int = 4, iters: int = 30, seed: int = 0):
        self.k = k
        self.iters = iters
        self.seed = seed
        self.ll_history: list[np.ndarray] = []

    def _params(self):
        return self.mu, self.var, self.logA, self.logpi

    @staticmethod
    def _lengths(X, lengths):
        if lengths is None:
            return torch.full((X.shape[0],), X.shape[1], dtype=torch.int32,
                              device=X.device)
        return torch.as_tensor(lengths, device=X.device).to(torch.int32)

    def _estep(self, X, lengths, want_gamma=False) -> dict:
        from ..ops.regime import hmm_estep_cpu, hmm_estep_gpu

        if X.is_cuda:
            return hmm_estep_gpu(X, lengths, *self._params(),
                                 want_gamma=want_gamma)
        st = hmm_estep_cpu(X.numpy(), lengths.numpy(),
                           *(p.numpy() for p in self._params()),
                           want_gamma=want_gamma)
        return {key: torch.from_numpy(np.ascontiguousarray(v))
                for key, v in st.items()}

    def init_params(self, X: torch.Tensor, lengths):
        B, N, F = X.shape
        k = self.k
        valid = (torch.arange(N, device=X.device)[None]
                 < lengths[:, None])[:, :, None].to(X.dtype)
        n = lengths.to(X.dtype)[:, None]
        mean = (X * valid).sum(1) / n
        var = (((X - mean[:, None]) ** 2) * valid).sum(1) \
            / (n - 1).clamp(min=1)
        self.mu = kmeans_many(X, lengths, k, 20, self.seed)
        self.var = torch.clamp(var[:, None, :].expand(B, k, F), min=1e-6)
        self.var = self.var.contiguous()
        if k > 1:
            A = torch.full((k, k), 0.05 / (k - 1), device=X.device,
                           dtype=X.dtype).fill_diagonal_(0.95)
        else:
            A = torch.ones(1, 1, device=X.device, dtype=X.dtype)
        self.logA = torch.log(A)[None].expand(B, k, k).contiguous()
        self.logpi = torch.full((B, k), -float(np.log(k)), device=X.device,
                                dtype=X.dtype)

    def fit_many(self, X: torch.Tensor, lengths=None):
        """X (B, Tmax, F), lengths (B,): Baum-Welch for every sequence."""
        from ..ops.regime import hmm_mstep

        lengths = self._lengths(X, lengths)
        self.init_params(X, lengths)
        self.ll_history = []
        for _ in range(self.iters):
            st = self._estep(X, lengths)
            self.ll_history.append(st["ll"].cpu().numpy().copy())
            p = hmm_mstep(st)
            self.mu, self.var = p["mu"].to(X.dtype), p["var"].to(X.dtype)
            self.logA = p["logA"].to(X.dtype)
            self.logpi = p["logpi"].to(X.dtype)
        return self

    def predict_many(self, X: torch.Tensor, lengths=None) -> torch.Tensor:
        """Viterbi paths (B, Tmax), -1 past lengths[b]."""
        from ..ops.regime import hmm_viterbi_cpu, hmm_viterbi_gpu

        lengths = self._lengths(X, lengths)
        if X.is_cuda:
            return hmm_viterbi_gpu(X, lengths, *self._params())
        return torch.from_numpy(hmm_viterbi_cpu(
            X.numpy(), lengths.numpy(),
            *(p.numpy() for p in self._params())))

    def posterior_many(self, X: torch.Tensor, lengths=None) -> torch.Tensor:
        """State posteriors gamma (B, Tmax, k), 0 past lengths[b]."""
        return self._estep(X, self._lengths(X, lengths),
                           want_gamma=True)["gamma"]

    def log_likelihood(self, X: torch.Tensor, lengths=None) -> torch.Tensor:
        return self._estep(X, self._lengths(X, lengths))["ll"]


def standardize_many(feats: torch.Tensor, nwin: torch.Tensor) -> torch.Tensor:
    """Per-sequence (x - mean) / (std + 1e-9) over each sequence's first
    nwin[b] rows, as `detect` standardises one symbol; padding rows are 0."""
    valid = (torch.arange(feats.shape[1], device=feats.device)[None]
             < nwin[:, None])[:, :, None].to(feats.dtype)
    n = nwin.to(feats.dtype)[:, None]
    mean = (feats * valid).sum(1) / n
    std = ((((feats - mean[:, None]) ** 2) * valid).sum(1)
           / (n - 1).clamp(min=1)).sqrt()
    return ((feats - mean[:, None]) / (std[:, None] + 1e-9)) * valid


def cluster_many(Xn: torch.Tensor, nwin: torch.Tensor, method: str, k: int,
                 seed: int):
    """Cluster every sequence of Xn (B, N, F): -> (assign (B, N) numpy,
    -1 past nwin[b]; posteriors (B, N, k) numpy for `hmm`, else None; the
    model). `hmm` is one batched model; `kmeans` / `gmm` loop the
    per-symbol classes."""
    if method == "hmm":
        model = GaussianHMMBatched(k, seed=seed).fit_many(Xn, nwin)
        return (model.predict_many(Xn, nwin).cpu().numpy(),
                model.posterior_many(Xn, nwin).cpu().numpy(), model)
    assign = np.full(Xn.shape[:2], -1, np.int64)
    model = None
    for i, m in enumerate(nwin.tolist()):
        cls = GMMTorch if method == "gmm" else KMeansTorch
        model = cls(k, seed=seed).fit(Xn[i, :m])
        assign[i, :m] = model.predict(Xn[i, :m]).cpu().numpy()
    return assign, None, model


def label_clusters(X: np.ndarray, assign: np.ndarray, k: int) -> dict:
    """Heuristic cluster -> regime mapping by mean return & volatility
    (market_regime_detector.py:226-296)."""
    stats = []
    for c in range(k):
        m = assign == c
        if not m.any():
            stats.append((0.0, 0.0))
            continue
        stats.append((float(X[m, 0].mean()), float(X[m, 1].mean())))
    vols = [s[1] for s in stats]
    vol_hi = np.percentile(vols, 75)
    labels = {}
    for c, (ret, vol) in enumerate(stats):
        if vol >= vol_hi and vol > 0:
            labels[c] = "volatile"
        elif ret > 0.002:
            labels[c] = "bull"
        elif ret < -0.002:
            labels[c] = "bear"
        else:
            labels[c] = "ranging"
    return labels


class RandomForestRegime:
    """Supervised RandomForest regime classifier — the reference's 4th
    detector mode (market_regime_detector.py:156): trained on labeled
    historical windows, predicts the regime of the latest one.

    Labels come from `label_windows` (rule-based labeling of each
    historical window — the offline stand-in for the reference's
    collected outcome labels, market_regime_data_collector.py:44-241);
    a caller with real labeled data passes them straight to fit()."""

    def __init__(self, n_estimators: int = 100, seed: int = 0):
        from sklearn.ensemble import RandomForestClassifier

        self.clf = RandomForestClassifier(
            n_estimators=n_estimators, random_state=seed, n_jobs=1)
        self.classes_: list[str] = []

    @staticmethod
    def label_windows(closes: np.ndarray, win: int = 32) -> np.ndarray:
        """Rule-label each feature window (bull/bear/ranging/volatile)."""
        n = len(closes) - win + 1
        labels = np.empty(n, dtype=object)
        for i in range(n):
            labels[i] = rule_based_regime(closes[i:i + win])[0]
        return labels

    def fit(self, X: np.ndarray, y: np.ndarray):
        self.clf.fit(X, y)
        self.classes_ = list(self.clf.classes_)
        return self

    def predict(self, X: np.ndarray) -> np.ndarray:
        return self.clf.predict(X)

    def predict_proba(self, X: np.ndarray) -> np.ndarray:
        return self.clf.predict_proba(X)

    def feature_importances(self) -> np.ndarray:
        return self.clf.feature_importances_


def rule_based_regime(closes: np.ndarray) -> tuple[str, float]:
    """Rule-based thresholds (market_regime_service.py:503-604)."""
    if len(closes) < 30:
        return "ranging", 0.0
    r = np.diff(np.log(closes[-100:]))
    ret = closes[-1] / closes[-min(len(closes), 100)] - 1.0
    vol = float(r.std() * np.sqrt(525_600))
    if vol > 1.2:
        return "volatile", min(vol / 2.0, 1.0)
    if ret > 0.01:
        return "bull", min(abs(ret) * 20, 1.0)
    if ret < -0.01:
        return "bear", min(abs(ret) * 20, 1.0)
    return "ranging", 0.3


class MarketRegimeService(Service):
    name = "market_regime"

    def __init__(self, bus, config=None, device="cpu"):
        super().__init__(bus, config)
        self.device = device
        self.prices: dict[str, list[float]] = {}
        self.model = None
        self.labels: dict[int, str] = {}
        self.current = "ranging"
        self.history: list[dict] = []

    def run_tasks(self):
        return [self._consume_market(), self._regime_loop()]

    async def _consume_market(self):
        sub = self.bus.subscribe(Channels.MARKET_UPDATES)

        def on_msg(_, m):
            if m.get("symbol"):
                h = self.prices.setdefault(m["symbol"], [])
                h.append(m["current_price"])
                if len(h) > 4096:
                    del h[:2048]

        await self.consume(sub, on_msg)

    def _primary_closes(self) -> np.ndarray | None:
        if not self.prices:
            return None
        sym = self.config.trading.symbols[0] \
            if self.config.trading.symbols[0] in self.prices \
            else next(iter(self.prices))
        h = self.prices[sym]
        return np.asarray(h, np.float64) if len(h) >= 64 else None

    def detect(self, closes: np.ndarray) -> tuple[str, float]:
        method = self.config.regime.method
        if method == "rule" or len(closes) < 200:
            return rule_based_regime(closes)
        X_np = extract_features(closes)
        if len(X_np) < 4 * self.config.regime.n_regimes:
            return rule_based_regime(closes)
        if method == "rf":
            # supervised mode (market_regime_detector.py:156): rule
            # labels over historical windows -> RandomForest -> predict
            # the latest window with a class-probability confidence
            y = RandomForestRegime.label_windows(closes)
            n = min(len(X_np), len(y))
            rf = RandomForestRegime(seed=self.config.seed)
            rf.fit(X_np[:n - 1], y[:n - 1])
            proba = rf.predict_proba(X_np[n - 1:n])[0]
            i = int(np.argmax(proba))
            self.model = rf
            return str(rf.classes_[i]), float(proba[i])
        X = torch.from_numpy(X_np)
        if self.device != "cpu":
            X = X.to(self.device)
        Xn = (X - X.mean(0)) / (X.std(0) + 1e-9)
        cls = {"gmm": GMMTorch, "hmm": GaussianHMMTorch}.get(
            method, KMeansTorch)
        self.model = cls(self.config.regime.n_regimes,
                         seed=self.config.seed).fit(Xn)
        assign = self.model.predict(Xn).cpu().numpy()
        self.labels = label_clusters(X_np, assign, self.config.regime.n_regimes)
        regime = self.labels.get(int(assign[-1]), "ranging")
        conf = float((assign == assign[-1]).mean())
        return regime, conf

    def detect_many(self, closes_by_symbol: dict) -> dict:
        """`detect` for a universe: {symbol: closes} -> {symbol: (regime,
        confidence)}. Features come from one batched pass; `hmm` fits and
        decodes every symbol in one batched model (GaussianHMMBatched) and
        takes as confidence the posterior of the Viterbi state at the last
        step; `kmeans` / `gmm` run the per-symbol classes over the batched
        features. Symbols `detect` would hand to the rules get the rules
        here too."""
        from ..ops.regime import regime_features_cpu, regime_features_gpu

        method = self.config.regime.method
        k = self.config.regime.n_regimes
        win = 32
        out, todo = {}, []
        for sym, closes in closes_by_symbol.items():
            closes = np.asarray(closes, np.float64)
            if method == "rf" and len(closes) >= 200:
                out[sym] = self.detect(closes)
            elif (method == "rule" or len(closes) < 200
                  or len(closes) - win < 4 * k):
                out[sym] = rule_based_regime(closes)
            else:
                todo.append((sym, closes))
        if not todo:
            return out
        S = len(todo)
        lens = np.asarray([len(c) for _, c in todo], np.int32)
        padded = np.ones((S, int(lens.max())), np.float32)
        for i, (_, c) in enumerate(todo):
            padded[i, :len(c)] = c
        if self.device != "cpu":
            feats = regime_features_gpu(
                torch.from_numpy(padded).to(self.device),
                torch.from_numpy(lens).to(self.device), win)
        else:
            feats = torch.from_numpy(regime_features_cpu(padded, lens, win))
        nwin = torch.from_numpy(lens - win).to(feats.device)
        paths, post, self.model = cluster_many(
            standardize_many(feats, nwin), nwin, method, k,
            self.config.seed)
        feats_np = feats.cpu().numpy()
        for i, (sym, _) in enumerate(todo):
            m = int(lens[i]) - win
            assign = paths[i, :m]
            if post is not None:
                conf = float(post[i, m - 1, assign[-1]])
            else:
                conf = float((assign == assign[-1]).mean())
            labels = label_clusters(feats_np[i, :m], assign, k)
            out[sym] = (labels.get(int(assign[-1]), "ranging"), conf)
        return {sym: out[sym] for sym in closes_by_symbol}

    async def _regime_loop(self):
        while self.running:
            closes = self._primary_closes()
            if closes is not None:
                closes = closes[-self.config.regime.lookback:]
                try:
                    regime, conf = self.detect(closes)
                except Exception as e:
                    self.log.warning("detect failed: %s", e)
                    regime, conf = rule_based_regime(closes)
                vol = float(np.diff(np.log(closes[-100:])).std()
                            * np.sqrt(525_600)) if len(closes) > 2 else 0.0
                entry = {"regime": regime, "confidence": conf,
                         "volatility": min(vol, 2.0), "at": time.time()}
                await self.bus.set(Keys.CURRENT_MARKET_REGIME, entry)
                self.history.append(entry)
                await self.bus.set(Keys.MARKET_REGIME_HISTORY,
                                   self.history[-100:])
                if regime != self.current:
                    await self.bus.publish(
                        Channels.STRATEGY_SWITCH,
                        StrategySwitch(regime, f"for-{self.current}",
                                       f"for-{regime}",
                                       "regime change").to_dict())
                    self.current = regime
            if self.config.regime.per_symbol:
                await self._publish_per_symbol()
            await self.sleep(5.0)

    async def _publish_per_symbol(self):
        """`market_regimes`: {symbol: entry} for every tracked symbol with
        enough history, next to the primary symbol's keys. An entry says
        which method produced it: the configured one, or "rule" when
        detect_many failed and the rules stood in. A missing HIP extension
        on a GPU device is not such a failure: it raises."""
        if self.device != "cpu":
            from ..ops import require_hip_ops
            require_hip_ops()
        lookback = self.config.regime.lookback
        universe = {sym: np.asarray(h[-lookback:], np.float64)
                    for sym, h in self.prices.items() if len(h) >= 64}
        if not universe:
            return
        method = self.config.regime.method
        try:
            found = self.detect_many(universe)
        except Exception as e:
            self.log.warning("detect_many failed, rules for all: %s", e)
            found = {sym: rule_based_regime(c) for sym, c in universe.items()}
            method = "rule"
        now = time.time()
        entries = {}
        for sym, (regime, conf) in found.items():
            c = universe[sym]
            vol = float(np.diff(np.log(c[-100:])).std()
                        * np.sqrt(525_600)) if len(c) > 2 else 0.0
            entries[sym] = {"regime": regime, "confidence": conf,
                            "volatility": min(vol, 2.0), "at": now,
                            "method": method}
        await self.bus.set(Keys.MARKET_REGIMES, entries)

    async def run(self):
        pass
