"""The Monte-Carlo kernels and the device RNG against the f64 references
and per-path envelopes of tests/mc_refs.py (validated on a CPU by
test_mc_refs_cpu.py).

The path references consume the device's own normals, read through the
philox_probe binding, so a path envelope holds only the arithmetic of the
kernel under test; the normals themselves are held to C_Z separately.
Every path and both outputs are compared elementwise, the raw bindings are
called so that path_base, seed and the true n_paths reach the kernel as
given, and every output buffer has NaN slack on both sides that must stay
untouched. Each test prints the worst fraction of its envelope.
"""

import dataclasses

import numpy as np
import pytest

import mc_refs as mr
from mc_refs import U24

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from ai_crypto_trader_amd.ops import require_hip_ops
    return require_hip_ops()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _u64(a, dev):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(dev)


def _u32(a, dev):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).to(dev)


def _philox_probe(ops, dev, seed, lo, hi):
    """-> words (n, 4) u32, normals (n, 4) f32 of the device."""
    n = int(np.asarray(lo).size)
    t_lo, t_hi = _u64(lo, dev), _u64(hi, dev)
    words = torch.empty((n, 4), dtype=torch.int32, device=dev)
    normals = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ops.philox_probe(seed, t_lo.data_ptr(), t_hi.data_ptr(),
                     words.data_ptr(), normals.data_ptr(), n, _stream(dev))
    torch.cuda.synchronize()
    return (words.cpu().numpy().view(np.uint32), normals.cpu().numpy())


def _device_normals(ops, dev):
    return lambda seed, lo, hi: _philox_probe(ops, dev, seed, lo, hi)[1]


class _Guarded:
    """Two output vectors with NaN slack on both sides."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((2, n + 2 * GUARD), float("nan"),
                              dtype=torch.float32, device=dev)
        self.fv = self.buf[0, GUARD:]
        self.dd = self.buf[1, GUARD:]

    def results(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:, :GUARD]).all(), "write below the outputs"
        assert np.isnan(b[:, GUARD + self.n:]).all(), \
            "write past the outputs"
        return b[0, GUARD:GUARD + self.n], b[1, GUARD:GUARD + self.n]


def _run_gbm(ops, dev, c, terms):
    cvol, drift, wS0, v0 = terms
    t_c = torch.from_numpy(cvol).to(dev)
    t_d = torch.from_numpy(drift).to(dev)
    t_w = torch.from_numpy(wS0).to(dev)
    out = _Guarded(c.n_paths, dev)
    if c.kernel == "mfma":
        ops.mc_paths_mfma(t_c.data_ptr(), t_d.data_ptr(), t_w.data_ptr(),
                          out.fv.data_ptr(), out.dd.data_ptr(), c.A,
                          c.n_steps, c.n_paths, float(v0), c.seed,
                          c.path_base, int(c.antithetic), _stream(dev))
    else:
        ops.mc_paths(t_c.data_ptr(), t_d.data_ptr(), t_w.data_ptr(), 0,
                     out.fv.data_ptr(), out.dd.data_ptr(), c.A, c.n_steps,
                     c.n_paths, float(v0), c.seed, c.path_base,
                     int(c.antithetic), _stream(dev))
    return out.results()


def _run_boot(ops, dev, c, terms):
    lr2, wS0, v0 = terms
    t_lr = torch.from_numpy(lr2).to(dev)
    t_w = torch.from_numpy(wS0).to(dev)
    out = _Guarded(c.n_paths, dev)
    ops.mc_bootstrap(t_lr.data_ptr(), t_w.data_ptr(), out.fv.data_ptr(),
                     out.dd.data_ptr(), c.A, c.t_hist, c.n_steps, c.n_paths,
                     float(v0), c.seed, c.path_base, _stream(dev))
    return out.results()


def _hold(tag, fv, dd, res):
    rf, rd = mr.worst(fv, dd, res)
    print(f"{tag}: fv {rf:.3g} dd {rd:.3g} of the envelope")
    qf = mr.ratio(fv, res["fv"], res["env_fv"])
    qd = mr.ratio(dd, res["dd"], res["env_dd"])
    assert (qf <= 1.0).all(), (tag, "fv", rf, int(qf.argmax()))
    assert (qd <= 1.0).all(), (tag, "dd", rd, int(qd.argmax()))


def _gbm_inside(ops, dev, c):
    terms = mr.gbm_terms(mr.gbm_inputs(c.A, c.kind))
    fv, dd = _run_gbm(ops, dev, c, terms)
    res = mr.gbm_run(c, _device_normals(ops, dev), terms=terms)
    _hold(c.id, fv, dd, res)
    return fv, dd, res


# --- RNG ------------------------------------------------------------------

@pytest.mark.parametrize("seed", [mr.SEED_LO, mr.SEED_HI])
def test_philox_words_bit_equal(dev, ops, seed):
    from ai_crypto_trader_amd.ops.montecarlo import philox4x32_np

    los = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 3]
    his = [0, 3, (2 << 32) | 1, (6 << 32) | 15, mr.BOOT_TAG,
           mr.BOOT_TAG | 1, mr.BOOT_TAG | ((1 << 32) - 1)]
    lo = np.array([a for a in los for _ in his], np.uint64)
    hi = np.array([b for _ in los for b in his], np.uint64)
    words, _ = _philox_probe(ops, dev, seed, lo, hi)
    want = np.stack(philox4x32_np(seed, lo, hi), axis=-1)
    np.testing.assert_array_equal(words, want)
    for i in (0, len(his) + 2, lo.size - 1):        # and the integer twin
        assert tuple(int(x) for x in words[i]) == \
            mr.philox4x32_int(seed, int(lo[i]), int(hi[i]))


def test_normals_within_c_z(dev, ops):
    seed, lo, hi = mr.rng_sample()
    words, z = _philox_probe(ops, dev, seed, lo, hi)
    z_ref, r_ref = mr.normals_ref(seed, lo, hi)
    q = mr.z_ratio(z, z_ref, r_ref)
    i = np.unravel_index(int(q.argmax()), q.shape)
    print(f"normals: worst |z - z_ref| / (U24 r) = {q.max():.3g} at draw "
          f"{i} (z_ref {z_ref[i]:.6g}, r {r_ref[i]:.6g}), C_Z = {mr.C_Z:g}")
    assert np.isfinite(z).all()
    assert (q <= mr.C_Z).all(), (float(q.max()), i)


def test_box_muller_edges(dev, ops):
    a_words = [0xFFFFFFFF, 0, 0x7FFFFFFF]          # u1 = 1, 2^-32, 1/2
    # turns 2^-32, 1/4, 1/2, 3/4, 1
    b_words = [0, (1 << 30) - 1, (1 << 31) - 1, 3 * (1 << 30) - 1,
               0xFFFFFFFF]
    a = np.array([x for x in a_words for _ in b_words], np.uint32)
    b = np.array([y for _ in a_words for y in b_words], np.uint32)
    t_a, t_b = _u32(a, dev), _u32(b, dev)
    out = torch.empty((a.size, 2), dtype=torch.float32, device=dev)
    ops.box_muller_probe(t_a.data_ptr(), t_b.data_ptr(), out.data_ptr(),
                         a.size, _stream(dev))
    torch.cuda.synchronize()
    z = out.cpu().numpy()
    z_ref, r = mr.box_muller_ref(a, b)
    q = mr.ratio(z, z_ref, U24 * r[:, None])
    print("box_muller edges: |z - z_ref| / (U24 r) per (u1, turns):\n",
          np.where(np.isfinite(q), q, -1).max(axis=1).reshape(3, 5))
    assert np.isfinite(z).all()
    assert (z[r == 0.0] == 0.0).all()              # u1 = 1: z = +-0 exactly
    assert abs(float(np.abs(z[5:10]).max()) - 6.66) < 0.01   # smallest u1
    assert (q <= mr.C_Z).all(), q


# --- VALU -----------------------------------------------------------------

@pytest.mark.parametrize("c", mr.VALU_CASES, ids=mr.case_id)
def test_valu_inside_envelope(dev, ops, c):
    fv, dd, _ = _gbm_inside(ops, dev, c)
    if c.kind == "monotone":
        assert (dd == 0.0).all()


def test_valu_grid_wrap(dev, ops):
    """More paths than the capped grid covers in one pass: the paths at
    the start, around the mirror boundary and across the wrap are held to
    the envelope, every other one must be finite."""
    c, paths = mr.WRAP_CASE, mr.wrap_paths()
    terms = mr.gbm_terms(mr.gbm_inputs(c.A, c.kind))
    fv, dd = _run_gbm(ops, dev, c, terms)
    assert np.isfinite(fv).all() and np.isfinite(dd).all()
    res = mr.gbm_run(c, _device_normals(ops, dev), paths, terms=terms)
    _hold(c.id, fv[paths], dd[paths], res)


# --- MFMA -----------------------------------------------------------------

@pytest.mark.parametrize("c", mr.MFMA_CASES, ids=mr.case_id)
def test_mfma_inside_envelope(dev, ops, c):
    _gbm_inside(ops, dev, c)
    if c.n_steps == 1:
        # the f32 kernel on the same counters: both inside their own
        # envelopes around one set of draws, so they agree on which
        # counter each path used
        _gbm_inside(ops, dev, dataclasses.replace(c, kernel="valu"))


# --- bootstrap ------------------------------------------------------------

@pytest.mark.parametrize("c", mr.BOOT_CASES, ids=mr.case_id)
def test_bootstrap_inside_envelope(dev, ops, c):
    terms = mr.boot_terms(*mr.boot_inputs(c.A, c.t_hist))
    fv, dd = _run_boot(ops, dev, c, terms)
    res = mr.boot_run(c, terms)
    _hold(c.id, fv, dd, res)
    if c.t_hist == 1:
        assert (fv == fv[0]).all() and (dd == dd[0]).all()
        closed = np.full(c.n_paths, mr.boot_closed_form(c, terms))
        assert (mr.ratio(fv, closed, res["env_fv"]) <= 1.0).all()


# --- sharding -------------------------------------------------------------

@pytest.mark.parametrize("kernel,lo", [("valu", 300), ("mfma", 256)])
def test_gbm_shards_are_the_single_run(dev, ops, kernel, lo):
    A = 64 if kernel == "mfma" else 8
    c = mr.GbmCase(kernel, A, 1000, 2, False, mr.BASE_HI, mr.SEED_HI)
    terms = mr.gbm_terms(mr.gbm_inputs(A))
    fv, dd = _run_gbm(ops, dev, c, terms)
    parts = [
        _run_gbm(ops, dev, dataclasses.replace(c, n_paths=lo), terms),
        _run_gbm(ops, dev, dataclasses.replace(
            c, n_paths=c.n_paths - lo, path_base=c.path_base + lo), terms),
    ]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), fv)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), dd)


def test_bootstrap_shards_are_the_single_run(dev, ops):
    c, lo = mr.BootCase(8, 33, 5, 1000, mr.BASE_HI, mr.SEED_HI), 300
    terms = mr.boot_terms(*mr.boot_inputs(c.A, c.t_hist))
    fv, dd = _run_boot(ops, dev, c, terms)
    parts = [
        _run_boot(ops, dev, dataclasses.replace(c, n_paths=lo), terms),
        _run_boot(ops, dev, dataclasses.replace(
            c, n_paths=c.n_paths - lo, path_base=c.path_base + lo), terms),
    ]
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), fv)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), dd)


# 64 assets select the MFMA kernel: its shard boundary sits on a block
@pytest.mark.parametrize("A,n", [(8, 1001), (64, 1024)])
def test_mc_paths_sharded_slices_are_the_single_run(dev, A, n):
    from ai_crypto_trader_amd.ops.montecarlo import (
        mc_paths_gpu, mc_paths_sharded,
    )

    inp = mr.gbm_inputs(A)
    args = (inp["chol"], inp["mu"], inp["sigma"], inp["w"])
    kw = dict(n_steps=3, dt=inp["dt"], s0=inp["s0"], seed=mr.SEED_HI,
              device=dev)
    fv, dd = mc_paths_gpu(*args, n_paths=n, **kw)
    got = [mc_paths_sharded(*args, n_paths_total=n, world=2, rank=r, **kw)
           for r in range(2)]
    torch.cuda.synchronize()
    assert [g[0].shape[0] for g in got] == [(n + 1) // 2, n // 2]
    assert torch.equal(torch.cat([g[0] for g in got]), fv)
    assert torch.equal(torch.cat([g[1] for g in got]), dd)


# --- the risk service's call -----------------------------------------------

def test_service_inputs_inside_envelope(dev, ops):
    """Three symbols as MonteCarloService.simulate prepares them (clipped
    estimates, padded to four assets with the zero-weight dummy), through
    mc_paths_gpu as the service calls it: antithetic, a path count that is
    no multiple of 256, dt = 1/365."""
    from ai_crypto_trader_amd.bus.message_bus import InProcessBus
    from ai_crypto_trader_amd.config import AppConfig
    from ai_crypto_trader_amd.ops.montecarlo import mc_paths_gpu
    from ai_crypto_trader_amd.services.monte_carlo import MonteCarloService

    svc = MonteCarloService(InProcessBus(), AppConfig())
    rng = np.random.default_rng(6)
    syms = ["AUSDC", "BUSDC", "CUSDC"]
    for s, (m, sd) in zip(syms, [(2e-3, 8e-3), (-2e-3, 7e-3), (0.0, 1e-3)]):
        svc.prices[s] = list(np.exp(np.cumsum(
            m + sd * rng.standard_normal(300))))
    mu, sigma, chol = svc._estimate_params(syms)
    assert mu[0] == 2.0 and mu[1] == -2.0 and sigma[0] == 4.0
    mu = np.concatenate([mu, [0.0]])
    sigma = np.concatenate([sigma, [1e-4]])
    w = np.array([1 / 3, 1 / 3, 1 / 3, 0.0])
    c4 = np.eye(4)
    c4[:3, :3] = chol
    inp = dict(chol=c4, mu=mu, sigma=sigma, w=w, s0=1.0, dt=1.0 / 365.0)
    c = mr.GbmCase("valu", 4, 1000, 7, True, 0, 13, "service")
    fv, dd = mc_paths_gpu(c4, mu, sigma, w, antithetic=True,
                          n_steps=c.n_steps, n_paths=c.n_paths, dt=inp["dt"],
                          seed=c.seed, device=dev)
    torch.cuda.synchronize()
    res = mr.gbm_run(c, _device_normals(ops, dev), terms=mr.gbm_terms(inp))
    _hold("service " + c.id, fv.cpu().numpy(), dd.cpu().numpy(), res)


def test_mfma_wrapper_pairs_on_the_true_path_count(dev, ops):
    """mc_paths_gpu at the service's default size: 64 assets select the
    MFMA kernel, antithetic, 10 000 paths (no multiple of 256). Path
    p >= 5000 mirrors p - 5000."""
    from ai_crypto_trader_amd.ops.montecarlo import mc_paths_gpu

    c = mr.GbmCase("mfma", 64, 10_000, 2, True, 0, mr.SEED_LO)
    inp = mr.gbm_inputs(64)
    fv, dd = mc_paths_gpu(inp["chol"], inp["mu"], inp["sigma"], inp["w"],
                          antithetic=True, n_steps=c.n_steps,
                          n_paths=c.n_paths, dt=inp["dt"], s0=inp["s0"],
                          seed=c.seed, device=dev)
    torch.cuda.synchronize()
    assert fv.shape == (c.n_paths,) and dd.shape == (c.n_paths,)
    res = mr.gbm_run(c, _device_normals(ops, dev))
    _hold("wrapper " + c.id, fv.cpu().numpy(), dd.cpu().numpy(), res)


# --- launch parameters are rejected before any launch -----------------------

def test_launchers_reject_bad_parameters(dev, ops):
    buf = torch.zeros(64 * 64 + 1024, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _stream(dev)

    def paths(A=8, n_steps=2, n_paths=256):
        ops.mc_paths(p, p, p, 0, p, p, A, n_steps, n_paths, 1.0, 1, 0, 0, s)

    def mfma(A=64, n_steps=2, n_paths=256):
        ops.mc_paths_mfma(p, p, p, p, p, A, n_steps, n_paths, 1.0, 1, 0, 0,
                          s)

    def boot(A=8, t_hist=4, n_steps=2, n_paths=256):
        ops.mc_bootstrap(p, p, p, p, A, t_hist, n_steps, n_paths, 1.0, 1, 0,
                         s)

    for fn in (paths, mfma, boot):
        for bad in (dict(n_paths=0), dict(n_paths=-5), dict(n_steps=-1),
                    dict(A=12), dict(A=0)):
            with pytest.raises(RuntimeError):
                fn(**bad)
    with pytest.raises(RuntimeError):
        mfma(A=32)
    for t_hist in (0, -3):
        with pytest.raises(RuntimeError):
            boot(t_hist=t_hist)
    torch.cuda.synchronize()
    assert (buf == 0).all()
