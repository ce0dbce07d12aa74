"""tests/rl_refs.py checked on a CPU: the existing f32 numpy twin
TradingVecEnvCPU follows the f64 reference's discrete trajectory exactly
and its floats stay under the recorded floors from which the device
constants derive; the GAE envelope is reachable (an f32 emulation sits
inside with 2x room) and has teeth (every seeded mutant leaves it); the
argument checks of the env classes and of gae_gpu raise before anything is
launched."""

import numpy as np
import pytest

import rl_refs as rr
from rl_refs import U24

torch = pytest.importorskip("torch")

from ai_crypto_trader_amd.models import rl  # noqa: E402


def _sub(ref, k):
    return {key: (v[:k] if isinstance(v, np.ndarray) else v)
            for key, v in ref.items()}


@pytest.fixture(scope="module")
def env_floor_runs():
    """Every case once: TradingVecEnvCPU (its first cpu_envs envs: an env's
    draws depend on its index alone) in lockstep with EnvRef. -> worst
    ratio per field (13,), per case."""
    out = {}
    for c in rr.ENV_CASES:
        market, acts = rr.env_market(c), rr.env_actions(c)
        k = c.cpu_envs
        ref = rr.EnvRef(market, c.n_envs, c.ep_len, c.fee, c.seed)
        cpu = rl.TradingVecEnvCPU(market, n_envs=k, ep_len=c.ep_len,
                                  fee=c.fee, seed=c.seed)
        worst = rr.env_ratios(None, cpu.reset(), _sub(ref.reset(), k))
        n_done = 0
        for s in range(c.steps):
            o, r, d = cpu.step(acts[s, :k])
            res = ref.step(acts[s])
            np.testing.assert_array_equal(d, res["done"][:k].astype(float))
            disc = ref.discrete()
            st = cpu.state
            np.testing.assert_array_equal(st[:, 0], disc["sym"][:k])
            np.testing.assert_array_equal(st[:, 1], disc["t"][:k])
            np.testing.assert_array_equal(st[:, 12], disc["ep_left"][:k])
            np.testing.assert_array_equal(st[:, 9] > 0, disc["in_pos"][:k])
            np.testing.assert_array_equal(o[:, 5], res["obs"][:k, 5])
            worst = np.maximum(worst, rr.env_ratios(r, o, _sub(res, k)))
            n_done += int(res["done"].sum())
        out[c.id] = (worst, n_done)
    return out


def test_env_cpu_twin_under_recorded_floors(env_floor_runs):
    total = np.zeros(len(rr.FIELDS))
    for cid, (worst, _) in env_floor_runs.items():
        print(cid, " ".join(f"{f}={w:.3g}" for f, w in
                            zip(rr.FIELDS, worst)))
        total = np.maximum(total, worst)
    print("worst per field:", " ".join(
        f"{f}={w:.3g}" for f, w in zip(rr.FIELDS, total)))
    assert (total <= rr.ENV_FLOOR).all(), dict(zip(rr.FIELDS, total))
    # a floor is a power of two, and no more than 4x what is needed
    # (obs 5, the flag, is exact and keeps the smallest floor)
    assert (np.log2(rr.ENV_FLOOR) % 1 == 0).all()
    assert (rr.ENV_FLOOR <= np.maximum(4 * total, 1.0)).all()
    np.testing.assert_array_equal(rr.ENV_C, 4 * rr.ENV_FLOOR)


def test_env_cases_restart_and_end_of_data(env_floor_runs):
    """The cases do what they are there for."""
    by = {c.id: c for c in rr.ENV_CASES}
    for cid, (_, n_done) in env_floor_runs.items():
        c = by[cid]
        if c.name == "main":
            assert n_done >= 3 * c.n_envs           # several restarts each
        if c.name == "shortest":
            assert n_done == c.steps * c.n_envs     # every step terminal
    c = next(c for c in rr.ENV_CASES if c.name == "short")
    ref = rr.EnvRef(rr.env_market(c), c.n_envs, c.ep_len, c.fee, c.seed)
    ref.reset()
    assert ref.n_start == 1 and (ref.t == 16).all()
    acts = rr.env_actions(c)
    for s in range(c.T - 16 - 2):
        res = ref.step(acts[s])
        # ends on t + 2 >= T, long before ep_len runs out
        assert res["done"].all() == (s == c.T - 16 - 3), s


def test_env_second_reset_gives_new_starts():
    c = rr.ENV_CASES[0]
    ref = rr.EnvRef(rr.env_market(c), c.n_envs, c.ep_len, c.fee, c.seed)
    ref.reset()
    first = (ref.sym.copy(), ref.t.copy())
    ref.reset()
    assert ref.epoch == 2
    assert ((ref.sym != first[0]) | (ref.t != first[1])).mean() > 0.9


def test_env_episode_rewards_sum_to_log_equity():
    """The identity the GPU test uses, on the reference itself."""
    c = rr.ENV_CASES[2]
    ref = rr.EnvRef(rr.env_market(c), c.n_envs, c.ep_len, c.fee, c.seed)
    ref.reset()
    acts = rr.env_actions(c)
    acc = np.zeros(c.n_envs)
    checked = 0
    for s in range(c.steps):
        res = ref.step(acts[s])
        acc += res["reward"]
        d = res["done"]
        np.testing.assert_allclose(acc[d], np.log(res["equity"][d]),
                                   rtol=0, atol=1e-12)
        checked += int(d.sum())
        acc[d] = 0.0
    assert checked > c.n_envs


@pytest.mark.parametrize("shape", [
    (3, 400), (3, 400, 3), (0, 400, 4), (2, 17, 4), (1, (1 << 24) + 1, 4)])
def test_env_shape_checks(shape):
    with pytest.raises(ValueError):
        rl._check_env_args(shape, 8, 16)


def test_env_argument_checks_raise_before_any_launch():
    ok = np.ones((2, 18, 4), np.float32)
    rl.TradingVecEnvCPU(ok, n_envs=1, ep_len=1)
    rl._check_env_args((1, 1 << 24, 4), 1, 1)
    for kw in (dict(n_envs=0), dict(ep_len=0)):
        with pytest.raises(ValueError):
            rl.TradingVecEnvCPU(ok, **kw)
    with pytest.raises(ValueError):
        rl.TradingVecEnvCPU(ok[:, :17])
    # the GPU class refuses a host tensor, f64, and a short history
    for bad in (torch.from_numpy(ok), torch.from_numpy(ok).double()):
        with pytest.raises(ValueError):
            rl.TradingVecEnv(bad)


def test_gae_gpu_argument_checks_raise_before_any_launch():
    T, E = 4, 3
    r, v, d = torch.zeros(T, E), torch.zeros(T + 1, E), torch.zeros(T, E)
    for args in ((r, v[:-1], d), (r, v, d[:, :-1]), (r.double(), v, d),
                 (r, v, d.bool()), (r[0], v, d), (r, v, d)):   # last: host
        with pytest.raises(ValueError):
            rl.gae_gpu(*args)


# --- GAE ------------------------------------------------------------------

GAE_COMBOS = [(p, dn) for p in rr.GAE_PARAMS for dn in rr.GAE_DONES]


@pytest.mark.parametrize("shape", rr.GAE_SHAPES, ids=str)
def test_gae_emulation_inside_envelope_with_room(shape):
    worst = 0.0
    for (gamma, lam), dn in GAE_COMBOS:
        rew, val, d = rr.gae_inputs(*shape, dn)
        ref = rr.gae_f64(rew, val, d, gamma, lam)
        for fma in (False, True):
            adv, ret = rr.gae_emulate(rew, val, d, gamma, lam, fma=fma)
            wa, wr = rr.gae_worst(adv, ret, ref)
            assert max(wa, wr) <= 0.5, (shape, gamma, lam, dn, fma, wa, wr)
            worst = max(worst, wa, wr)
    print(f"gae {shape}: f32 emulation at {worst:.3g} of the envelope")


def test_gae_envelope_is_tight_enough_to_matter():
    """Median envelope relative to |A| stays within a few hundred ulps at
    the longest scan: it cannot hide a wrong term."""
    rew, val, d = rr.gae_inputs(128, 257, "random")
    adv, _, ea, _ = rr.gae_f64(rew, val, d, 0.99, 0.95)
    assert np.median(ea / np.abs(adv)) < 512 * U24


@pytest.mark.parametrize("mutant", rr.GAE_MUTANTS)
def test_gae_mutants_rejected(mutant):
    """On the 5 % random dones of the (128, 257) shape, gamma 0.99,
    lam 0.95."""
    rew, val, d = rr.gae_inputs(128, 257, "random")
    ref = rr.gae_f64(rew, val, d, 0.99, 0.95)
    adv, ret, _, _ = rr.gae_f64(rew, val, d, 0.99, 0.95, mutant=mutant)
    wa, wr = rr.gae_worst(adv, ret, ref)
    assert max(wa, wr) > 1000.0, (mutant, wa, wr)


def test_gae_closed_forms():
    """lam = 0 gives the one-step TD error; all dones cut every bootstrap
    (A_t = r_t - v_t); gamma = lam = 1 without dones telescopes to the
    reward-to-go plus the bootstrap minus v_t."""
    rew, val, d = rr.gae_inputs(7, 255, "none")
    r, v = rew.astype(np.float64), val.astype(np.float64)
    g = np.float64(np.float32(0.9))
    adv, _, _, _ = rr.gae_f64(rew, val, d, 0.9, 0.0)
    np.testing.assert_allclose(adv, r + g * v[1:] - v[:-1], atol=1e-14)
    adv, ret, _, _ = rr.gae_f64(rew, val, np.ones_like(d), 0.99, 0.95)
    np.testing.assert_allclose(adv, r - v[:-1], atol=1e-14)
    np.testing.assert_allclose(ret, r, atol=1e-14)
    adv, _, _, _ = rr.gae_f64(rew, val, d, 1.0, 1.0)
    togo = np.cumsum(r[::-1], axis=0)[::-1]
    np.testing.assert_allclose(adv, togo + v[-1] - v[:-1], atol=1e-12)
