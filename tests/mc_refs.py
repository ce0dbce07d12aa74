"""f64 references, error envelopes, CPU emulations and seeded mutants for
the Monte-Carlo kernels of ops/hip/montecarlo.hip and the device RNG of
ops/hip/common.hpp (a helper module, no tests of its own).

Shared by test_mc_refs_cpu.py, which shows on a CPU that every envelope is
reachable by a correct kernel (an f32 / bf16 emulation of the kernel sits
inside it with 2x room) and rejects a subtly wrong one (seeded mutants of
the semantics sit outside), and by test_gpu_montecarlo.py, which holds the
HIP kernels to the same envelopes.

The path references consume NORMALS AS AN ARGUMENT: on the GPU the device's
own philox_normal4 output (read through the philox_probe binding), on the
CPU the numpy twin philox_normal4_np. The path envelopes therefore contain
only the arithmetic of the kernel under test; the RNG is judged separately
(normals_ref, C_Z). For the MFMA kernel the bf16 rounding of z * zsign and
of cvol is part of the reference (kernel_refs.bf16_round, nearest-even, is
what the hardware conversion does), so its envelope too is f32-only.

Semantics encoded once (gbm_draws / gbm_run / boot_run):
  - counters (ctr_lo = zsrc, ctr_hi = step << 32 | k4), component d of the
    draw is normal k = 4 k4 + d;
  - half = n_paths // 2; with antithetic a path p >= half takes
    zsrc = p - half + path_base and negated normals, else p + path_base;
  - per step: logS, then V, then vmax, then dd; v0 is the f32 sum of wS0;
  - bootstrap: ctr_hi = 2^63 | s4, component j is step 4 s4 + j, row index
    word % t_hist.

Envelopes, first-order running error analysis, nothing fitted to a GPU
result. U24 = 2^-24 is the f32 unit roundoff.
  - every f32 fma or add contributes U24 |its result| (VALU logS: A fma and
    one drift add per step; bootstrap: one add per step), accumulated next
    to the f64 recurrence across steps;
  - MFMA logS: bf16 x bf16 products are exact in f32; a 32-deep MFMA plus
    its C input is a 33-term sum in unspecified order, bounded by
    33 U24 (sum |products| + |C|), twice per step, then the drift add;
  - V = sum_a w_a 2^L_a: each term is off by w_a 2^L_a (ln2 dL_a + EPS_EXP)
    and the fma chain adds U24 |partial sum| per term (VALU, bootstrap: A
    terms in order; MFMA: four 16-term chains and three pairwise adds);
  - dd_t = (vmax - V) rcp(vmax): (dV + dvmax) / vmax + (3 U24 + EPS_RCP)
    dd_t, with dvmax the running max of dV (max is 1-Lipschitz), and the
    max drawdown inherits the max over steps.
EPS_EXP = EPS_RCP = 2 * 2^-23: docs/KERNELS.md documents the raw v_exp_f32
and v_rcp_f32 as 1 ulp (2^-23 relative); the factor 2 is room.
"""

from dataclasses import dataclass

import numpy as np

from ai_crypto_trader_amd.ops.montecarlo import (
    _LOG2E, _gbm_terms, _u32_to_unit, philox4x32_np,
)
from kernel_refs import U24, _fma32, bf16_round

EPS_EXP = 2.0 * 2.0 ** -23
EPS_RCP = 2.0 * 2.0 ** -23
LN2 = float(np.log(2.0))
MC_AS = (4, 8, 16, 32, 64)
MAX_GRID_PATHS = 8192 * 256          # grid cap of the VALU / bootstrap kernels
BOOT_TAG = 1 << 63
# the envelope must be useful: median of envelope(fv) / |fv| over all cases
USEFUL_CAP = 64 * U24

f32 = np.float32
f64 = np.float64
u64 = np.uint64


# ---------------------------------------------------------------------------
# RNG: Philox words -> f32 uniforms (bit-exact in numpy) -> f64 Box-Muller
# ---------------------------------------------------------------------------
RNG_SAMPLE_SEED = 77
RNG_SAMPLE_HI = 5
RNG_SAMPLE_N = 1 << 18
# Device normals are allowed |z - z_ref| <= C_Z * U24 * r_ref with r_ref the
# Box-Muller radius of the draw: the error of r (v_log, v_sqrt) and that of
# the angle (v_sin / v_cos on turns) both scale with r. The floor is what
# the f32 numpy twin philox_normal4_np itself needs against the f64
# reference over the fixed sample (test_mc_refs_cpu measures 7.1 and asserts
# it stays under C_Z_CPU_FLOOR); the device gets 4x the floor, rounded up to
# a power of two, because its natives are 1-ulp rather than half-ulp and it
# reduces the turns input itself.
C_Z_CPU_FLOOR = 8.0
C_Z = 32.0


def philox4x32_int(seed, ctr_lo, ctr_hi, rounds=7):
    """Philox4x32 on Python integers, independent of numpy dtypes."""
    M = 0xFFFFFFFF
    k0, k1 = seed & M, (seed >> 32) & M
    c0, c1, c2, c3 = ctr_lo & M, (ctr_lo >> 32) & M, ctr_hi & M, \
        (ctr_hi >> 32) & M
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, \
            (p0 >> 32) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def box_muller_ref(a, b):
    """f64 Box-Muller on the device's f32 uniforms. -> z (n, 2), r (n,)."""
    u1 = _u32_to_unit(np.asarray(a, np.uint32)).astype(f64)
    u2 = _u32_to_unit(np.asarray(b, np.uint32)).astype(f64)
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1), r


def normals_ref(seed, ctr_lo, ctr_hi):
    """-> z_ref (n, 4) f64, r_ref (n, 4) f64 (the radius of each draw)."""
    a, b, c, d = philox4x32_np(seed, ctr_lo, ctr_hi)
    z0, r0 = box_muller_ref(a, b)
    z1, r1 = box_muller_ref(c, d)
    return (np.concatenate([z0, z1], axis=-1),
            np.stack([r0, r0, r1, r1], axis=-1))


def rng_sample():
    lo = np.arange(RNG_SAMPLE_N, dtype=u64)
    return RNG_SAMPLE_SEED, lo, np.full(RNG_SAMPLE_N, RNG_SAMPLE_HI, u64)


def ratio(got, ref, env):
    """|got - ref| / env elementwise; 0 where both vanish, inf where only
    the envelope does, inf for a non-finite result."""
    err = np.abs(np.asarray(got, f64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / env)
    return np.where(np.isfinite(q), q, np.inf)


def z_ratio(z, z_ref, r_ref):
    return ratio(z, z_ref, U24 * r_ref)


# ---------------------------------------------------------------------------
# Inputs: asymmetric everywhere
# ---------------------------------------------------------------------------
def _random_chol(rng, A):
    W = rng.standard_normal((A, A + 2)) + 0.8 * rng.standard_normal((A, 1))
    S = W @ W.T
    d = np.sqrt(np.diag(S))
    return np.linalg.cholesky(S / d[:, None] / d[None, :])


def gbm_inputs(A, kind="general"):
    """-> dict(chol, mu, sigma, w, s0, dt). Dense L with distinct entries,
    per-asset mu and sigma, unequal weights with one exact zero, s0 != 1.
    kind "service": 3 real assets padded to 4 as MonteCarloService.simulate
    pads them, mu and sigma at its clip values, dt = 1/365, s0 = 1 as it
    passes. kind "monotone": tiny sigma, mu > 0, so V only rises."""
    rng = np.random.default_rng([23, A])
    if kind == "service":
        assert A == 4
        chol = np.eye(4)
        chol[:3, :3] = _random_chol(rng, 3)
        return dict(chol=chol, mu=np.array([2.0, -2.0, 0.7, 0.0]),
                    sigma=np.array([4.0, 4.0, 0.9, 1e-4]),
                    w=np.array([1 / 3, 1 / 3, 1 / 3, 0.0]), s0=1.0,
                    dt=1.0 / 365.0)
    chol = _random_chol(rng, A)
    w = rng.uniform(0.5, 1.5, A)
    w[2] = 0.0
    w /= w.sum()
    if kind == "monotone":
        return dict(chol=chol, mu=np.linspace(0.5, 0.8, A),
                    sigma=1e-5 * (1.0 + np.arange(A)), w=w, s0=37.5,
                    dt=1.0 / 252.0)
    assert kind == "general"
    return dict(chol=chol, mu=rng.uniform(-0.5, 0.8, A),
                sigma=rng.uniform(0.2, 1.2, A), w=w, s0=37.5, dt=1.0 / 252.0)


def gbm_terms(inp):
    """(cvol [k][a], drift, wS0, v0), all f32, exactly what mc_paths_gpu
    hands to the kernels."""
    cvol, drift = _gbm_terms(inp["chol"], inp["mu"], inp["sigma"], inp["dt"])
    wS0 = (np.asarray(inp["w"]) * inp["s0"]).astype(f32)
    return cvol, drift, wS0, f32(wS0.sum())


def boot_inputs(A, t_hist):
    """-> (lr natural-log rows (t_hist, A) f32, weights, s0): per-asset
    means and scales differ, one weight is exactly zero."""
    rng = np.random.default_rng([29, A, t_hist])
    j = np.arange(A)
    lr = (0.0004 * (1 + j) / A
          + 0.01 * (1 + 0.5 * ((3 * j + 1) % A) / A)
          * rng.standard_normal((t_hist, A))).astype(f32)
    w = rng.uniform(0.5, 1.5, A)
    w[1] = 0.0
    return lr, w / w.sum(), 12.25


def boot_terms(lr, w, s0):
    """(logret base-2 (t_hist, A), wS0, v0) f32 as mc_bootstrap_gpu builds
    them."""
    lr2 = np.ascontiguousarray(np.asarray(lr, f32) * f32(_LOG2E), dtype=f32)
    wS0 = (np.asarray(w) * s0).astype(f32)
    return lr2, wS0, f32(wS0.sum())


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------
SEED_LO = 9
SEED_HI = (1 << 32) + 9
BASE_HI = (1 << 32) + 5


@dataclass(frozen=True)
class GbmCase:
    kernel: str             # "valu" | "mfma"
    A: int
    n_paths: int
    n_steps: int
    antithetic: bool
    path_base: int
    seed: int
    kind: str = "general"

    @property
    def id(self):
        return (f"{self.kernel}-A{self.A}-P{self.n_paths}-T{self.n_steps}"
                f"-anti{int(self.antithetic)}-base{self.path_base}"
                f"-seed{self.seed}-{self.kind}")


@dataclass(frozen=True)
class BootCase:
    A: int
    t_hist: int
    n_steps: int
    n_paths: int
    path_base: int
    seed: int

    @property
    def id(self):
        return (f"boot-A{self.A}-H{self.t_hist}-T{self.n_steps}"
                f"-P{self.n_paths}-base{self.path_base}-seed{self.seed}")


def _valu_cases():
    out = []
    for A in MC_AS:
        out += [
            GbmCase("valu", A, 1, 1, False, 0, SEED_LO),
            GbmCase("valu", A, 255, 2, True, 777, SEED_HI),      # odd n
            GbmCase("valu", A, 257, 7, False, BASE_HI, SEED_LO),
            GbmCase("valu", A, 1000, 7, True, BASE_HI, SEED_HI),
            GbmCase("valu", A, 257, 1, True, 0, SEED_HI),        # odd n
            GbmCase("valu", A, 1000, 2, False, 777, SEED_LO),
        ]
    out += [
        GbmCase("valu", 4, 257, 7, True, 777, SEED_HI, "service"),
        GbmCase("valu", 4, 257, 7, False, 0, SEED_LO, "monotone"),
    ]
    return out


VALU_CASES = _valu_cases()
MFMA_CASES = [
    GbmCase("mfma", 64, 256, 1, False, 0, SEED_LO),
    GbmCase("mfma", 64, 512, 2, False, 777, SEED_HI),
    GbmCase("mfma", 64, 768, 7, True, BASE_HI, SEED_LO),   # half in a block
    GbmCase("mfma", 64, 1000, 2, True, 0, SEED_HI),
    GbmCase("mfma", 64, 1000, 7, False, 777, SEED_LO),
    GbmCase("mfma", 64, 1000, 1, True, BASE_HI, SEED_HI),
    GbmCase("mfma", 64, 10_000, 2, True, BASE_HI, SEED_HI),
    GbmCase("mfma", 64, 256, 7, False, BASE_HI, SEED_LO),
    GbmCase("mfma", 64, 999, 1, True, 777, SEED_LO),       # odd n
]
# the grid-stride wrap of the VALU kernel: only the listed paths are held to
# the envelope (the probe is called for their counters alone)
WRAP_CASE = GbmCase("valu", 4, MAX_GRID_PATHS + 300, 2, True, 777, SEED_HI)


def wrap_paths(c=WRAP_CASE):
    half = c.n_paths // 2
    return np.concatenate([
        np.arange(256),
        np.arange(half - 128, half + 128),
        np.arange(MAX_GRID_PATHS - 256, c.n_paths),
    ])


def _boot_cases():
    out = []
    for A in MC_AS:
        out += [
            BootCase(A, 1, 5, 257, 0, SEED_LO),
            BootCase(A, 2, 3, 1, BASE_HI, SEED_HI),
            BootCase(A, 33, 7, 257, BASE_HI, SEED_LO),
            BootCase(A, 300, 4, 257, 0, SEED_HI),
            BootCase(A, 300, 1, 1, 0, SEED_LO),
        ]
    return out


BOOT_CASES = _boot_cases()


def case_id(c):
    return c.id


# ---------------------------------------------------------------------------
# GBM semantics: counters, then the f64 recurrence with its running envelope
# ---------------------------------------------------------------------------
def pad256(n):
    return -(-n // 256) * 256


def gbm_draws(c, paths=None, mutant=None):
    """-> seed, ctr_lo, ctr_hi (P, T, A/4) u64, sign (P, A) f32."""
    n, A, T = c.n_paths, c.A, c.n_steps
    p = (np.arange(n, dtype=np.int64) if paths is None
         else np.asarray(paths, np.int64))
    half = n // 2
    if mutant == "half_from_padded_count":
        half = pad256(n) // 2
    if mutant == "half_off_by_one_at_odd_n":
        half = (n + 1) // 2
    mirror = (p >= half) if c.antithetic else np.zeros(p.shape, bool)
    base_m = 0 if mutant == "path_base_not_added_on_mirror" else c.path_base
    zsrc = np.where(mirror, p - half + base_m, p + c.path_base)
    if mutant == "path_high_word_dropped":
        zsrc = zsrc & 0xFFFFFFFF
    seed = c.seed & 0xFFFFFFFF if mutant == "seed_high_word_dropped" \
        else c.seed
    step = np.arange(T, dtype=u64)[None, :, None]
    k4 = np.arange(A // 4, dtype=u64)[None, None, :]
    if mutant == "k4_off_by_one":
        k4 = k4 + u64(1)
    if mutant == "counter_words_swapped":
        hi = (k4 << u64(32)) | step
    else:
        hi = (step << u64(32)) | k4
    shape = (p.size, T, A // 4)
    lo = np.broadcast_to(zsrc.astype(u64)[:, None, None], shape)
    hi = np.broadcast_to(hi, shape)
    sign = np.where(mirror, f32(-1), f32(1))[:, None].repeat(A, axis=1)
    if mutant == "sign_not_applied_to_one_component":
        sign[:, 3::4] = 1.0
    return seed, lo, hi, sign.astype(f32)


def draw_normals(normal_fn, seed, lo, hi):
    """normal_fn(seed, ctr_lo (n,), ctr_hi (n,)) -> (n, 4) f32; returns the
    normals as (P, T, A)."""
    P, T, K4 = lo.shape
    z = normal_fn(seed, np.ascontiguousarray(lo).ravel(),
                  np.ascontiguousarray(hi).ravel())
    return np.asarray(z, f32).reshape(P, T, K4 * 4)


def bf16_trunc(x):
    x = np.ascontiguousarray(x, dtype=f32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def _rd(x, e):
    """One f32 rounding of a result x known to within e."""
    return U24 * (np.abs(x) + e)


def _chain(term, eterm, rows):
    """f32 fma chain acc += term[a] over rows, from 0: value, error."""
    S = np.zeros(term.shape[0])
    E = np.zeros(term.shape[0])
    for a in rows:
        S = S + term[:, a]
        E = E + eterm[:, a]
        E = E + _rd(S, E)
    return S, E


def _pair(S0, E0, S1, E1):
    S = S0 + S1
    E = E0 + E1
    return S, E + _rd(S, E)


def _mfma_rows(fq):
    return [mt * 16 + fq * 4 + r for mt in range(4) for r in range(4)]


def _drawdown(state, V, eV, mutant):
    vmax, evmax, mdd, emdd = state
    if mutant == "dd_before_vmax_update":
        ddt = (vmax - V) / vmax
        vmax = np.maximum(vmax, V)
        evmax = np.maximum(evmax, eV)
    else:
        vmax = np.maximum(vmax, V)
        evmax = np.maximum(evmax, eV)
        ddt = (vmax - V) / vmax
    edd = (eV + evmax) / (vmax - evmax) \
        + (3 * U24 + EPS_RCP) * np.abs(ddt)
    return vmax, evmax, np.maximum(mdd, ddt), np.maximum(emdd, edd)


def gbm_f64(c, terms, z, sign, paths, mutant=None):
    """The f64 recurrence on given normals z (P, T, A) f32 (unsigned), with
    the running envelope. -> dict(fv, dd, env_fv, env_dd)."""
    cvol, drift, wS0, v0 = terms
    A, P = c.A, z.shape[0]
    mfma = c.kernel == "mfma"
    if mutant == "z_xy_swapped":
        idx = np.arange(A)
        idx[0::4], idx[1::4] = np.arange(A)[1::4], np.arange(A)[0::4]
        z = z[:, :, idx]
    zs = (z * sign[:, None, :]).astype(f32)
    cv = np.asarray(cvol, f32)
    if mfma:
        rnd = bf16_trunc if mutant == "bf16_truncation" else bf16_round
        zs, cv = rnd(zs), rnd(cv)
        if mutant == "zhalf_halves_swapped":
            zs = np.concatenate([zs[..., 32:], zs[..., :32]], axis=-1)
    cv = cv.astype(f64)                                  # [k][a]
    if mutant == "cvol_untransposed":
        cv = cv.T
    d = drift.astype(f64)
    w = wS0.astype(f64)
    if mutant == "drift_shifted_one_asset":
        d = np.roll(d, 1)
    if mutant == "two_weights_swapped":
        w = w.copy()
        w[[0, 1]] = w[[1, 0]]
    d = np.broadcast_to(d, (P, A))
    w = np.broadcast_to(w, (P, A))
    if mutant == "fr_instead_of_fq4_r":
        row = (np.arange(A) // 16 * 16)[None, :] \
            + (np.asarray(paths) % 16)[:, None]
        d, w = drift.astype(f64)[row], wS0.astype(f64)[row]

    L = np.zeros((P, A))
    eL = np.zeros((P, A))
    V = np.full(P, f64(v0))
    eV = np.zeros(P)
    Vprev = V
    dds = (V.copy(), np.zeros(P), np.zeros(P), np.zeros(P))
    for t in range(c.n_steps):
        zt = zs[:, t, :].astype(f64)
        if mfma:
            for ks in range(2):
                sl = slice(32 * ks, 32 * ks + 32)
                cin = np.abs(L) + eL
                L = L + zt[:, sl] @ cv[sl]
                eL = eL + 33 * U24 * (np.abs(zt[:, sl]) @ np.abs(cv[sl])
                                      + cin)
        else:
            for k in range(A):
                L = L + zt[:, k, None] * cv[k][None, :]
                eL = eL + _rd(L, eL)
        L = L + d
        eL = eL + _rd(L, eL)
        term = w * (np.exp(L) if mutant == "exp_instead_of_exp2"
                    else np.exp2(L))
        eterm = np.abs(term) * (np.expm1(LN2 * eL) + EPS_EXP)
        Vprev = V
        if mfma:
            parts = [_chain(term, eterm, _mfma_rows(fq)) for fq in range(4)]
            s01 = _pair(*parts[0], *parts[1])
            if mutant == "one_shuffle_missing":
                V, eV = s01
            else:
                V, eV = _pair(*s01, *_pair(*parts[2], *parts[3]))
        else:
            V, eV = _chain(term, eterm, range(A))
        dds = _drawdown(dds, V, eV, mutant)
    fv = Vprev if mutant == "final_value_one_step_early" else V
    return dict(fv=fv, dd=dds[2], env_fv=eV, env_dd=dds[3])


def gbm_run(c, normal_fn, paths=None, mutant=None, terms=None):
    """Reference (mutant=None) or a seeded mutant of it, on the normals
    normal_fn yields for the counters the semantics ask for."""
    if terms is None:
        terms = gbm_terms(gbm_inputs(c.A, c.kind))
    p = (np.arange(c.n_paths, dtype=np.int64) if paths is None
         else np.asarray(paths, np.int64))
    if mutant == "ct_tiles_swapped":
        p = p ^ 16
    seed, lo, hi, sign = gbm_draws(c, p, mutant)
    z = draw_normals(normal_fn, seed, lo, hi)
    return gbm_f64(c, terms, z, sign, p, mutant)


def _exp2_32(x):
    return np.exp2(x.astype(f32)).astype(f32)


def _dd32(vmax, mdd, V):
    vmax = np.maximum(vmax, V)
    dd = ((vmax - V).astype(f32) * (f32(1) / vmax).astype(f32)).astype(f32)
    return vmax, np.maximum(mdd, dd)


def gbm_emulate(c, normal_fn, paths=None, terms=None):
    """Step-for-step f32 (VALU) / bf16 + f32 (MFMA, the 32-deep chain in
    sequential order) twin of the kernel. -> fv, dd f32."""
    if terms is None:
        terms = gbm_terms(gbm_inputs(c.A, c.kind))
    cvol, drift, wS0, v0 = terms
    seed, lo, hi, sign = gbm_draws(c, paths)
    z = draw_normals(normal_fn, seed, lo, hi)
    zs = (z * sign[:, None, :]).astype(f32)
    cv = np.asarray(cvol, f32)
    mfma = c.kernel == "mfma"
    if mfma:
        zs, cv = bf16_round(zs), bf16_round(cv)
    P, A = zs.shape[0], c.A
    L = np.zeros((P, A), f32)
    V = np.full(P, v0, f32)
    vmax = np.full(P, v0, f32)
    mdd = np.zeros(P, f32)
    for t in range(c.n_steps):
        for k in range(A):
            L = _fma32(L, zs[:, t, k, None], cv[k][None, :])
        L = (L + drift[None, :]).astype(f32)
        ex = _exp2_32(L)
        if mfma:
            part = []
            for fq in range(4):
                acc = np.zeros(P, f32)
                for a in _mfma_rows(fq):
                    acc = _fma32(acc, wS0[a], ex[:, a])
                part.append(acc)
            V = ((part[0] + part[1]).astype(f32)
                 + (part[2] + part[3]).astype(f32)).astype(f32)
        else:
            V = np.zeros(P, f32)
            for a in range(A):
                V = _fma32(V, wS0[a], ex[:, a])
        vmax, mdd = _dd32(vmax, mdd, V)
    return V, mdd


# ---------------------------------------------------------------------------
# Bootstrap semantics
# ---------------------------------------------------------------------------
def boot_counters(c, paths=None, mutant=None):
    """-> seed, ctr_lo, ctr_hi (P, S4) u64."""
    p = (np.arange(c.n_paths, dtype=np.int64) if paths is None
         else np.asarray(paths, np.int64))
    src = p + c.path_base
    if mutant == "path_high_word_dropped":
        src = src & 0xFFFFFFFF
    seed = c.seed & 0xFFFFFFFF if mutant == "seed_high_word_dropped" \
        else c.seed
    s4 = np.arange((c.n_steps + 3) // 4, dtype=u64)
    tag = u64(0) if mutant == "tag_bit_missing" else u64(BOOT_TAG)
    shape = (p.size, s4.size)
    return (seed, np.broadcast_to(src.astype(u64)[:, None], shape),
            np.broadcast_to((tag | s4)[None, :], shape))


def boot_indices(c, words_fn=philox4x32_np, paths=None, mutant=None):
    """Row index per (path, step); the mutant "tail_steps_executed" runs
    all four steps of the last Philox call."""
    seed, lo, hi = boot_counters(c, paths, mutant)
    P, S4 = lo.shape
    w = words_fn(seed, np.ascontiguousarray(lo).ravel(),
                 np.ascontiguousarray(hi).ravel())
    w = np.stack([np.asarray(x, np.uint32) for x in w], axis=-1)
    if mutant == "philox_components_reversed":
        w = w[:, ::-1]
    mod = c.t_hist - 1 if mutant == "mod_t_hist_minus_1" else c.t_hist
    t = (w.astype(np.int64) % mod).reshape(P, S4 * 4)
    return t if mutant == "tail_steps_executed" else t[:, :c.n_steps]


def _boot_rows(lr2, A, t, mutant):
    if mutant == "row_stride_a_minus_1":
        flat = np.concatenate([lr2.ravel(), np.zeros(A, lr2.dtype)])
        return flat[(t * (A - 1))[:, None] + np.arange(A)[None, :]]
    return lr2[t]


def boot_run(c, terms=None, words_fn=philox4x32_np, paths=None,
             mutant=None):
    if terms is None:
        terms = boot_terms(*boot_inputs(c.A, c.t_hist))
    lr2, wS0, v0 = terms
    idx = boot_indices(c, words_fn, paths, mutant)
    P, A = idx.shape[0], c.A
    w = wS0.astype(f64)
    if mutant == "two_weights_swapped":
        w[[0, 1]] = w[[1, 0]]
    w = np.broadcast_to(w, (P, A))
    L = np.zeros((P, A))
    eL = np.zeros((P, A))
    V = np.full(P, f64(v0))
    eV = np.zeros(P)
    Vprev = V
    dds = (V.copy(), np.zeros(P), np.zeros(P), np.zeros(P))
    for s in range(idx.shape[1]):
        L = L + _boot_rows(lr2, A, idx[:, s], mutant).astype(f64)
        eL = eL + _rd(L, eL)
        term = w * (np.exp(L) if mutant == "exp_instead_of_exp2"
                    else np.exp2(L))
        eterm = np.abs(term) * (np.expm1(LN2 * eL) + EPS_EXP)
        Vprev = V
        V, eV = _chain(term, eterm, range(A))
        dds = _drawdown(dds, V, eV, mutant)
    fv = Vprev if mutant == "final_value_one_step_early" else V
    return dict(fv=fv, dd=dds[2], env_fv=eV, env_dd=dds[3])


def boot_emulate(c, terms=None, words_fn=philox4x32_np, paths=None):
    if terms is None:
        terms = boot_terms(*boot_inputs(c.A, c.t_hist))
    lr2, wS0, v0 = terms
    idx = boot_indices(c, words_fn, paths)
    P, A = idx.shape[0], c.A
    L = np.zeros((P, A), f32)
    V = np.full(P, v0, f32)
    vmax = np.full(P, v0, f32)
    mdd = np.zeros(P, f32)
    for s in range(idx.shape[1]):
        L = (L + lr2[idx[:, s]]).astype(f32)
        ex = _exp2_32(L)
        V = np.zeros(P, f32)
        for a in range(A):
            V = _fma32(V, wS0[a], ex[:, a])
        vmax, mdd = _dd32(vmax, mdd, V)
    return V, mdd


def boot_closed_form(c, terms):
    """t_hist = 1: every path adds row 0 n_steps times."""
    lr2, wS0, _ = terms
    return float((wS0.astype(f64)
                  * np.exp2(c.n_steps * lr2[0].astype(f64))).sum())


# ---------------------------------------------------------------------------
# Mutants: each a defect a plausible edit could introduce
# ---------------------------------------------------------------------------
COMMON_MUTANTS = (
    "cvol_untransposed", "drift_shifted_one_asset", "two_weights_swapped",
    "z_xy_swapped", "k4_off_by_one", "counter_words_swapped",
    "seed_high_word_dropped", "path_high_word_dropped",
    "exp_instead_of_exp2", "final_value_one_step_early",
)
ANTITHETIC_MUTANTS = (
    "half_from_padded_count", "half_off_by_one_at_odd_n",
    "sign_not_applied_to_one_component", "path_base_not_added_on_mirror",
)
MFMA_MUTANTS = (
    "zhalf_halves_swapped", "ct_tiles_swapped", "one_shuffle_missing",
    "fr_instead_of_fq4_r", "bf16_truncation",
)
GBM_MUTANTS = COMMON_MUTANTS + ANTITHETIC_MUTANTS
BOOT_MUTANTS = (
    "two_weights_swapped", "seed_high_word_dropped",
    "path_high_word_dropped", "exp_instead_of_exp2",
    "final_value_one_step_early", "mod_t_hist_minus_1",
    "tail_steps_executed", "row_stride_a_minus_1", "tag_bit_missing",
    "philox_components_reversed",
)
# "dd computed before vmax is updated" cannot be told from the kernel by
# its outputs: where V exceeds the old vmax the early dd is negative and
# max(mdd, dd) with mdd >= 0 drops it, elsewhere vmax does not change. It
# is kept as a mutant that must be bit-equal to the reference.
EQUIVALENT_MUTANTS = ("dd_before_vmax_update",)


def worst(got_fv, got_dd, res, room=1.0):
    """Largest |got - ref| / (room * envelope) over every path, for both
    outputs."""
    return (float(ratio(got_fv, res["fv"], room * res["env_fv"]).max()),
            float(ratio(got_dd, res["dd"], room * res["env_dd"]).max()))


def useful(res):
    """envelope(fv) / |fv_ref| per path."""
    return res["env_fv"] / np.abs(res["fv"])
