"""f64 references, envelopes, f32 emulations and seeded mutants for the
kernels of ops/hip/rl_env.hip: env_reset_kernel, env_step_kernel and
gae_kernel (a helper module, no tests of its own).

Shared by test_rl_refs_cpu.py (on a CPU: the existing f32 twin
TradingVecEnvCPU follows the reference's discrete trajectory exactly and
its floats sit under the recorded floors; an f32 emulation of the GAE scan
sits inside its envelope with 2x room; every GAE mutant leaves it) and by
test_gpu_rl_env.py, which holds the HIP kernels to the same references.

The environment (EnvRef)
------------------------
One lane per env, vectorised here over envs, all floats f64, the kernel's
f32 constants (2/13, 2/27, 2/10, 0.01, 0.001, 1 - fee) taken at their f32
values. Per step, in the kernel's order: t += 1, EMAs, signal, RSI
averages, the action, equity, reward, ep_left -= 1,
done = ep_left <= 0 or t + 2 >= T, the observation, and on done an
in-place restart drawn from philox(seed, e, 2^32 epoch + t):
sym = x % nsym, t0 = 16 + y % max(T - ep_len - 32, 1). reset() draws
philox(seed, e, epoch) after epoch += 1. Actions: 1 enters (all-in) when
flat, 2 closes when long, EVERYTHING ELSE HOLDS, 0 as well as the
out-of-range -1 and 3.

The discrete trajectory, symbol, t, ep_left, done, the in-position flag
and the restart (sym, t0), does not depend on rounding (units is exactly 0
or a positive quotient) and is compared exactly, with the range check
16 <= t0 < 16 + max(T - ep_len - 32, 1).

The reward and the twelve observation fields are held to
    |got - ref| <= C_field * U24 * scale_field
where scale is the magnitude of the operands before cancellation:
  reward   log(eq / prev_eq): both equities carry the roundings of the
           trades of the episode (three per trade on cash or units, then
           the product and the sum), the quotient one more, the logarithm
           an absolute error of its own: 2 (1 + trades) + 1 + |reward|;
  obs 0    rsi / 100 = 1 - 1 / (1 + rs) lies in [0, 1] and a relative
           error e of rs moves it by rs e / (1 + rs)^2 <= e / 4: 1;
  obs 1    100 (ema_f - ema_s - sig) / close:
           100 (|ema_f| + |ema_s| + |sig|) / close;
  obs 2-4  100 (close / c_k - 1): 100 (close / c_k + 1);
  obs 5    the flag: exact;
  obs 6    10 (close / entry - 1) in a position: 10 (close / entry + 1),
           and exactly 0 outside one;
  obs 7    equity - 1: equity (1 + trades) + 1;
  obs 8-9  1000 avg, avg += (x - avg) / 14: 1000 (avg_prev + x + avg);
  obs 10   100 (ema_f / ema_s - 1): 100 (ema_f / ema_s + 1);
  obs 11   0.001 ep_left, one product: |obs 11|.
The recurrences (EMAs with gain 2/13 .. 2/10, averages with 1/14) damp an
old error geometrically, so a static scale holds at every step; the factor
that the accumulation costs is part of C. C is not guessed: ENV_FLOOR
records, per field, a power of two above the worst ratio that the existing
f32 numpy twin TradingVecEnvCPU needs against this reference over all
cases (test_rl_refs_cpu.py prints the measured ratios and asserts them
under the floor); the device gets ENV_C = 4 x floor, the rule of
mc_refs.C_Z: its __logf, divisions and fma contraction are 1-ulp where
numpy rounds to half an ulp.

An identity that needs no reference: over one episode of one env the
rewards sum to log(final equity), to within the summed reward envelopes
and that of the final equity.

GAE (gae_f64)
-------------
A_t = delta_t + gamma lam nonterm_t A_{t+1},
delta_t = r_t + gamma v_{t+1} nonterm_t - v_t, returns A_t + v_t, with
gamma and lam at their f32 values and a running first-order envelope
    err_t = gamma lam nonterm err_{t+1}
            + GAE_C U24 (|r_t| + gamma |v_{t+1}| + |v_t|
                         + gamma lam |A_{t+1}| + |A_t|),
    err_ret_t = err_t + U24 (|A_t| + |v_t|).
GAE_C = 3 is the largest number of roundings any term passes before the
final add, counted from the kernel: gamma v_{t+1} is rounded as a product,
in the sum with r_t and in the difference with v_t (nonterm is 0 or 1, its
products are exact); gamma lam A_{t+1} is rounded in gamma * lam and in the
product; the final add is the |A_t| term.
"""

from dataclasses import dataclass

import numpy as np

from ai_crypto_trader_amd.ops.montecarlo import philox4x32_np
from kernel_refs import U24

f32 = np.float32
f64 = np.float64
u64 = np.uint64

N_OBS = 12
FIELDS = ("reward",) + tuple(f"obs{k}" for k in range(N_OBS))
# worst ratio of TradingVecEnvCPU (f32 numpy) against EnvRef over ENV_CASES,
# as test_rl_refs_cpu.py measures it, in the order of FIELDS:
#   reward 0.53, obs0 2.11, obs1 1.45, obs2 0.50, obs3 0.50, obs4 0.50,
#   obs5 0 (exact), obs6 0.50, obs7 0.76, obs8 2.11, obs9 2.05, obs10 3.24,
#   obs11 0.89
ENV_FLOOR = np.array([1, 4, 2, 1, 1, 1, 1, 1, 1, 4, 4, 4, 1], f64)
ENV_C = 4.0 * ENV_FLOOR
GAE_C = 3.0


# ---------------------------------------------------------------------------
# Environment cases
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class EnvCase:
    name: str
    n_envs: int
    nsym: int
    T: int
    ep_len: int
    steps: int
    fee: float
    seed: int
    cpu_envs: int           # envs the slow per-env f32 twin is run for

    @property
    def id(self):
        return f"{self.name}-fee{self.fee}"


ENV_CASES = [
    # crosses the 256-lane block edge; every env restarts several times
    EnvCase("main", 300, 3, 400, 37, 120, 0.001, 5, 300),
    EnvCase("main", 300, 3, 400, 37, 120, 0.0, (1 << 32) + 5, 48),
    EnvCase("main", 300, 3, 400, 37, 120, 0.01, 6, 48),
    # max_start clamps to 1 and the episode ends on t + 2 >= T
    EnvCase("short", 257, 2, 60, 128, 100, 0.01, 7, 48),
    # every step is terminal
    EnvCase("shortest", 257, 1, 18, 5, 6, 0.0, 8, 48),
]


def case_id(c):
    return c.id


def env_market(c):
    """(nsym, T, 4) f32: close, high, low, volume; a 1 % random walk
    around a level that differs per symbol."""
    rng = np.random.default_rng([41, c.nsym, c.T])
    ret = 0.01 * rng.standard_normal((c.nsym, c.T))
    close = 50.0 * (1 + np.arange(c.nsym))[:, None] * np.exp(np.cumsum(ret, 1))
    out = np.empty((c.nsym, c.T, 4), f32)
    out[..., 0] = close
    out[..., 1] = close * 1.003
    out[..., 2] = close * 0.997
    out[..., 3] = rng.uniform(1, 2, (c.nsym, c.T))
    return out


def env_actions(c):
    """(steps, n_envs) int32 drawn from {-1, 0, 1, 2, 3}."""
    rng = np.random.default_rng([43, c.n_envs, c.steps])
    return rng.integers(-1, 4, (c.steps, c.n_envs)).astype(np.int32)


A_F, A_S, A_SIG = (f64(f32(2) / f32(13)), f64(f32(2) / f32(27)),
                   f64(f32(2) / f32(10)))
K001, K0001 = f64(f32(0.01)), f64(f32(0.001))


class EnvRef:
    """The f64 state machine. reset() and step(actions) return a dict:
    obs (E, 12) f64 and scale_obs; step adds reward, scale_reward, done,
    and after it sym, t, ep_left, in_pos hold the state the kernel leaves
    behind (after an in-place restart), restart the envs that restarted."""

    def __init__(self, candles, n_envs, ep_len, fee, seed):
        self.c = np.asarray(candles, f32).astype(f64)[..., 0]
        self.nsym, self.T = self.c.shape
        self.E, self.ep_len, self.seed = n_envs, ep_len, seed
        self.keep = f64(f32(1.0) - f32(fee))
        self.epoch = 0
        self.e = np.arange(n_envs, dtype=u64)

    @property
    def n_start(self):
        return max(self.T - self.ep_len - 32, 1)

    def _restart(self, mask, ctr_hi):
        x, y, _, _ = philox4x32_np(self.seed, self.e, ctr_hi)
        sym = (x.astype(np.int64) % self.nsym)
        t0 = 16 + (y.astype(np.int64) % self.n_start)
        assert ((t0 >= 16) & (t0 < 16 + self.n_start)).all()
        c0 = self.c[sym, t0]
        new = dict(sym=sym, t=t0, ema_f=c0, ema_s=c0, sig=0 * c0,
                   ag=0 * c0, al=0 * c0, prev=c0, cash=1 + 0 * c0,
                   units=0 * c0, entry=c0, equity=1 + 0 * c0,
                   ep_left=np.full(self.E, self.ep_len, np.int64),
                   trades=np.zeros(self.E, np.int64))
        for k, v in new.items():
            cur = getattr(self, k, None)
            setattr(self, k, v if cur is None else np.where(mask, v, cur))

    def _obs(self, rsi, hist, r1, r5, r15, close, s_rest):
        in_pos = self.units > 0
        upnl = np.where(in_pos, close / self.entry - 1.0, 0.0)
        obs = np.stack([
            rsi * K001, hist / close * 100.0, r1 * 100.0, r5 * 100.0,
            r15 * 100.0, in_pos.astype(f64), upnl * 10.0,
            self.equity - 1.0, self.ag * 1000.0, self.al * 1000.0,
            (self.ema_f / self.ema_s - 1.0) * 100.0,
            self.ep_left * K0001], axis=1)
        s2, s3, s4, s8, s9 = s_rest
        scale = np.stack([
            np.ones(self.E),
            100.0 * (np.abs(self.ema_f) + np.abs(self.ema_s)
                     + np.abs(self.sig)) / close,
            s2, s3, s4, np.zeros(self.E),
            np.where(in_pos, 10.0 * (close / self.entry + 1.0), 0.0),
            self.equity * (1 + self.trades) + 1.0, s8, s9,
            100.0 * (self.ema_f / self.ema_s + 1.0),
            np.abs(self.ep_left * K0001)], axis=1)
        return obs, scale

    def reset(self):
        self.epoch += 1
        self._restart(np.ones(self.E, bool),
                      np.full(self.E, self.epoch, u64))
        z = np.zeros(self.E)
        obs, scale = self._obs(50.0 + z, z, z, z, z, self.prev,
                               (200 + z, 200 + z, 200 + z, z, z))
        return dict(obs=obs, scale_obs=scale)

    def step(self, actions):
        act = np.asarray(actions)
        t = self.t + 1
        row = self.c[self.sym]
        idx = np.arange(self.E)
        close = row[idx, t]
        self.ema_f = self.ema_f + A_F * (close - self.ema_f)
        self.ema_s = self.ema_s + A_S * (close - self.ema_s)
        macd = self.ema_f - self.ema_s
        self.sig = self.sig + A_SIG * (macd - self.sig)
        change = close - self.prev
        gain, loss = np.maximum(change, 0), np.maximum(-change, 0)
        ag0, al0 = self.ag, self.al
        self.ag = ag0 + (gain - ag0) / 14.0
        self.al = al0 + (loss - al0) / 14.0
        rsi = 100.0 - 100.0 / (1.0 + self.ag / np.maximum(self.al, 1e-9))
        enter = (act == 1) & (self.units == 0)
        close_ = (act == 2) & (self.units > 0)
        units = np.where(enter, self.cash * self.keep / close, self.units)
        entry = np.where(enter, close, self.entry)
        cash = np.where(enter, 0.0, self.cash)
        cash = np.where(close_, cash + units * close * self.keep, cash)
        units = np.where(close_, 0.0, units)
        self.units, self.entry, self.cash = units, entry, cash
        self.trades = self.trades + enter + close_
        equity = cash + units * close
        prev_eq = self.equity
        reward = np.log(np.maximum(equity, 1e-9) / np.maximum(prev_eq, 1e-9))
        self.equity = equity
        self.ep_left = self.ep_left - 1
        done = (self.ep_left <= 0) | (t + 2 >= self.T)
        c5 = row[idx, np.maximum(t - 5, 0)]
        c15 = row[idx, np.maximum(t - 15, 0)]
        r1 = close / self.prev - 1.0
        s_rest = (100 * (close / self.prev + 1), 100 * (close / c5 + 1),
                  100 * (close / c15 + 1), 1000 * (ag0 + gain + self.ag),
                  1000 * (al0 + loss + self.al))
        self.prev = close
        self.t = t
        obs, scale = self._obs(rsi, macd - self.sig, r1, close / c5 - 1.0,
                               close / c15 - 1.0, close, s_rest)
        out = dict(obs=obs, scale_obs=scale, reward=reward, done=done,
                   scale_reward=2.0 * (1 + self.trades) + 1.0
                   + np.abs(reward),
                   t_step=t.copy(), equity=equity.copy())
        self._restart(done, (u64(1) << u64(32)) * u64(self.epoch)
                      + t.astype(u64))
        out["restart"] = done
        return out

    def discrete(self):
        """What the kernel's state buffer must hold exactly."""
        return dict(sym=self.sym.copy(), t=self.t.copy(),
                    ep_left=self.ep_left.copy(), in_pos=self.units > 0)


def ratio(got, ref, env):
    """|got - ref| / env elementwise; 0 where they agree exactly, inf
    where only the envelope vanishes or the result is not finite."""
    err = np.abs(np.asarray(got, f64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / env)
    return np.where(np.isfinite(q), q, np.inf)


def env_ratios(got_reward, got_obs, ref):
    """Worst |got - ref| / (U24 scale) per field of FIELDS (13,);
    got_reward None for a reset."""
    q = ratio(got_obs, ref["obs"], U24 * ref["scale_obs"]).max(axis=0)
    r = 0.0 if got_reward is None else \
        ratio(got_reward, ref["reward"], U24 * ref["scale_reward"]).max()
    return np.concatenate([[r], q])


# ---------------------------------------------------------------------------
# GAE
# ---------------------------------------------------------------------------
GAE_SHAPES = ((1, 1), (7, 255), (128, 257), (64, 600))
GAE_PARAMS = ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0))
GAE_DONES = ("none", "all", "random", "first", "last")
GAE_MUTANTS = ("nonterm_missing_from_bootstrap", "nonterm_missing_from_carry",
               "values_t_for_values_t1", "returns_without_v")


def gae_inputs(T, E, dones):
    rng = np.random.default_rng([47, T, E])
    rew = rng.standard_normal((T, E)).astype(f32)
    val = (rng.standard_normal((T + 1, E)) + 0.5).astype(f32)
    d = np.zeros((T, E), f32)
    if dones == "all":
        d[:] = 1.0
    elif dones == "random":
        d[rng.random((T, E)) < 0.05] = 1.0
    elif dones == "first":
        d[0] = 1.0
    elif dones == "last":
        d[-1] = 1.0
    else:
        assert dones == "none"
    return rew, val, d


def gae_f64(rew, val, dones, gamma, lam, mutant=None):
    """-> adv, ret, env_adv, env_ret, all (T, E) f64."""
    g, gl = f64(f32(gamma)), f64(f32(gamma)) * f64(f32(lam))
    r, v, d = (np.asarray(x, f32).astype(f64) for x in (rew, val, dones))
    T, E = r.shape
    adv, ret = np.empty((T, E)), np.empty((T, E))
    ea, er = np.empty((T, E)), np.empty((T, E))
    a, err = np.zeros(E), np.zeros(E)
    for t in range(T - 1, -1, -1):
        nt = 1.0 - d[t]
        nt_b = 1.0 if mutant == "nonterm_missing_from_bootstrap" else nt
        nt_c = 1.0 if mutant == "nonterm_missing_from_carry" else nt
        v1 = v[t] if mutant == "values_t_for_values_t1" else v[t + 1]
        a1 = a
        a = r[t] + g * v1 * nt_b - v[t] + gl * nt_c * a1
        err = gl * nt * err + GAE_C * U24 * (
            np.abs(r[t]) + g * np.abs(v[t + 1]) + np.abs(v[t])
            + gl * np.abs(a1) + np.abs(a))
        adv[t], ea[t] = a, err
        ret[t] = a if mutant == "returns_without_v" else a + v[t]
        er[t] = err + U24 * (np.abs(a) + np.abs(v[t]))
    return adv, ret, ea, er


def gae_emulate(rew, val, dones, gamma, lam, fma=False):
    """The kernel's scan in f32, plain or with the contractions a compiler
    may apply (a * b + c in one rounding)."""
    g, l_ = f32(gamma), f32(lam)
    rew, val, dones = (np.asarray(x, f32) for x in (rew, val, dones))
    T, E = rew.shape
    adv, ret = np.empty((T, E), f32), np.empty((T, E), f32)
    a = np.zeros(E, f32)
    gl = f32(g * l_)
    for t in range(T - 1, -1, -1):
        nt = (f32(1.0) - dones[t]).astype(f32)
        gv = (g * val[t + 1]).astype(f32)
        if fma:
            s = (rew[t].astype(f64) + gv.astype(f64) * nt).astype(f32)
            delta = (s - val[t]).astype(f32)
            a = (delta.astype(f64)
                 + (gl * nt).astype(f64) * a.astype(f64)).astype(f32)
        else:
            delta = ((rew[t] + (gv * nt).astype(f32)).astype(f32)
                     - val[t]).astype(f32)
            a = (delta + ((gl * nt).astype(f32) * a).astype(f32)).astype(f32)
        adv[t] = a
        ret[t] = (a + val[t]).astype(f32)
    return adv, ret


def gae_worst(adv, ret, ref, room=1.0):
    """Largest fraction of the envelope, for adv and for ret."""
    ra, rr, ea, er = ref
    return (float(ratio(adv, ra, room * ea).max()),
            float(ratio(ret, rr, room * er).max()))
