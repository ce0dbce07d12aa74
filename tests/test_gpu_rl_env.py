"""env_reset_kernel, env_step_kernel and gae_kernel against the f64
references of tests/rl_refs.py (validated on a CPU by
test_rl_refs_cpu.py).

The environment runs through TradingVecEnv with its state, obs, reward and
done tensors replaced by views into one NaN-guarded buffer, so the wrapper's
argument handling and the kernels' writes are both under test. The discrete
trajectory (symbol, t, ep_left, done, the in-position flag, the restart) is
compared exactly after every step; the reward and the observation fields
are held to ENV_C * U24 * scale per field. GAE runs through the raw binding
into guarded outputs and through gae_gpu. Each test prints its worst
fraction of the envelope.
"""

import numpy as np
import pytest

import rl_refs as rr
from rl_refs import U24

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
N_STATE = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from ai_crypto_trader_amd.ops import require_hip_ops
    return require_hip_ops()


class _Guarded:
    """Several f32 tensors as views into one buffer, NaN slack before,
    between and after them."""

    def __init__(self, dev, **shapes):
        self.spans, off = {}, GUARD
        for name, shape in shapes.items():
            n = int(np.prod(shape))
            self.spans[name] = (off, n, shape)
            off += n + GUARD
        self.buf = torch.full((off,), float("nan"), dtype=torch.float32,
                              device=dev)

    def view(self, name):
        off, n, shape = self.spans[name]
        return self.buf[off:off + n].view(*shape)

    def read(self):
        """-> {name: ndarray}; asserts every guard word is still NaN."""
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        keep = np.ones(b.size, bool)
        out = {}
        for name, (off, n, shape) in self.spans.items():
            keep[off:off + n] = False
            out[name] = b[off:off + n].reshape(shape).copy()
        assert np.isnan(b[keep]).all(), "write outside the outputs"
        return out


def _guarded_env(dev, c, market):
    from ai_crypto_trader_amd.models.rl import TradingVecEnv
    env = TradingVecEnv(torch.from_numpy(market).to(dev), n_envs=c.n_envs,
                        ep_len=c.ep_len, fee=c.fee, seed=c.seed)
    g = _Guarded(dev, state=(c.n_envs, N_STATE), obs=(c.n_envs, rr.N_OBS),
                 reward=(c.n_envs,), done=(c.n_envs,))
    g.view("state").zero_()
    env.state, env.obs = g.view("state"), g.view("obs")
    env.reward, env.done = g.view("reward"), g.view("done")
    return env, g


def _check_discrete(tag, st, ref):
    d = ref.discrete()
    np.testing.assert_array_equal(st[:, 0], d["sym"], err_msg=tag)
    np.testing.assert_array_equal(st[:, 1], d["t"], err_msg=tag)
    np.testing.assert_array_equal(st[:, 12], d["ep_left"], err_msg=tag)
    np.testing.assert_array_equal(st[:, 9] > 0, d["in_pos"], err_msg=tag)
    assert (st[:, 9] >= 0).all(), tag


@pytest.mark.parametrize("c", rr.ENV_CASES, ids=rr.case_id)
def test_env_matches_reference(dev, c):
    market, acts = rr.env_market(c), rr.env_actions(c)
    env, g = _guarded_env(dev, c, market)
    ref = rr.EnvRef(market, c.n_envs, c.ep_len, c.fee, c.seed)
    env.reset()
    got, res = g.read(), ref.reset()
    _check_discrete("reset", got["state"], ref)
    first = (ref.sym.copy(), ref.t.copy())
    worst = rr.env_ratios(None, got["obs"], res)
    assert (worst <= rr.ENV_C).all(), ("reset", dict(zip(rr.FIELDS, worst)))
    acc = np.zeros(c.n_envs)          # rewards of the running episode
    acc_env = np.zeros(c.n_envs)
    n_done, worst_id = 0, 0.0
    for s in range(c.steps):
        env.step(torch.from_numpy(acts[s]).to(dev))
        got, res = g.read(), ref.step(acts[s])
        tag = f"step {s}"
        np.testing.assert_array_equal(got["done"], res["done"].astype(float),
                                      err_msg=tag)
        _check_discrete(tag, got["state"], ref)
        np.testing.assert_array_equal(got["obs"][:, 5], res["obs"][:, 5],
                                      err_msg=tag)
        q = rr.env_ratios(got["reward"], got["obs"], res)
        assert (q <= rr.ENV_C).all(), (tag, dict(zip(rr.FIELDS, q)))
        worst = np.maximum(worst, q)
        # identity: an episode's rewards sum to log(final equity)
        acc += got["reward"].astype(np.float64)
        acc_env += rr.ENV_C[0] * U24 * res["scale_reward"]
        d = res["done"]
        eq = got["obs"][:, 7].astype(np.float64) + 1.0
        slack = acc_env + rr.ENV_C[8] * U24 * res["scale_obs"][:, 7] / eq
        qi = rr.ratio(acc[d], np.log(eq[d]), slack[d])
        if qi.size:
            assert (qi <= 1.0).all(), (tag, "identity", float(qi.max()))
            worst_id = max(worst_id, float(qi.max()))
        acc[d], acc_env[d] = 0.0, 0.0
        n_done += int(d.sum())
    if c.name == "main":
        assert n_done >= 3 * c.n_envs
    # a second reset() is a new epoch: new starts, the reference's
    env.reset()
    got, res = g.read(), ref.reset()
    _check_discrete("second reset", got["state"], ref)
    if ref.n_start > 1:
        assert ((ref.sym != first[0]) | (ref.t != first[1])).mean() > 0.9
    q = rr.env_ratios(None, got["obs"], res)
    assert (q <= rr.ENV_C).all(), ("second reset", dict(zip(rr.FIELDS, q)))
    frac = np.maximum(worst, q) / rr.ENV_C
    print(f"{c.id}: worst fraction of the envelope "
          + " ".join(f"{f}={x:.3g}" for f, x in zip(rr.FIELDS, frac))
          + f"; reward-sum identity {worst_id:.3g}; {n_done} restarts")


def test_env_refuses_bad_arguments_on_device(dev):
    from ai_crypto_trader_amd.models.rl import TradingVecEnv
    ok = torch.ones(2, 18, 4, device=dev)
    TradingVecEnv(ok, n_envs=1, ep_len=1)
    for bad, kw in ((ok[:, :17], {}), (ok.double(), {}), (ok[..., :3], {}),
                    (ok[0], {}), (ok[:0], {}), (ok, dict(n_envs=0)),
                    (ok, dict(ep_len=0)), (ok.cpu(), {})):
        with pytest.raises(ValueError):
            TradingVecEnv(bad, **kw)


# --- GAE ------------------------------------------------------------------

def _gae_raw(ops, dev, rew, val, d, gamma, lam):
    T, E = rew.shape
    g = _Guarded(dev, adv=(T, E), ret=(T, E))
    t = [torch.from_numpy(x).to(dev) for x in (rew, val, d)]
    ops.gae(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
            g.view("adv").data_ptr(), g.view("ret").data_ptr(), T, E,
            gamma, lam, torch.cuda.current_stream(dev).cuda_stream)
    out = g.read()
    return out["adv"], out["ret"]


@pytest.mark.parametrize("shape", rr.GAE_SHAPES, ids=str)
def test_gae_matches_reference(dev, ops, shape):
    from ai_crypto_trader_amd.models.rl import gae_gpu
    worst = 0.0
    for gamma, lam in rr.GAE_PARAMS:
        for dn in rr.GAE_DONES:
            rew, val, d = rr.gae_inputs(*shape, dn)
            ref = rr.gae_f64(rew, val, d, gamma, lam)
            adv, ret = _gae_raw(ops, dev, rew, val, d, gamma, lam)
            wa, wr = rr.gae_worst(adv, ret, ref)
            assert max(wa, wr) <= 1.0, (shape, gamma, lam, dn, wa, wr)
            worst = max(worst, wa, wr)
            # the wrapper on a transposed (dense, not contiguous) rewards
            # and dones: same bits, contiguous outputs
            rew_t = torch.from_numpy(np.ascontiguousarray(rew.T)).to(dev).t()
            d_t = torch.from_numpy(np.ascontiguousarray(d.T)).to(dev).t()
            a2, r2 = gae_gpu(rew_t, torch.from_numpy(val).to(dev), d_t,
                             gamma, lam)
            torch.cuda.synchronize()
            assert a2.is_contiguous() and r2.is_contiguous()
            assert tuple(a2.shape) == shape and tuple(r2.shape) == shape
            np.testing.assert_array_equal(a2.cpu().numpy(), adv)
            np.testing.assert_array_equal(r2.cpu().numpy(), ret)
    print(f"gae {shape}: worst {worst:.3g} of the envelope")


def test_gae_gpu_refuses_bad_arguments_on_device(dev):
    from ai_crypto_trader_amd.models.rl import gae_gpu
    T, E = 4, 3
    r = torch.zeros(T, E, device=dev)
    v = torch.zeros(T + 1, E, device=dev)
    d = torch.zeros(T, E, device=dev)
    for args in ((r, v[:-1], d), (r, v, d[:, :-1]), (r.double(), v, d),
                 (r, v, d.bool()), (r, v.half(), d), (r, v, d.cpu())):
        with pytest.raises(ValueError):
            gae_gpu(*args)
