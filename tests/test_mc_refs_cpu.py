"""The envelopes of tests/mc_refs.py, validated without a GPU.

For every case the GPU tests run, an f32 / bf16 emulation of the kernel's
arithmetic sits inside the per-path envelope of both outputs with 2x room
(ROOM; the whole envelope is f32 arithmetic, the bf16 roundings of the MFMA
kernel are part of its reference). Every seeded mutant falls outside on at
least one path of at least one case; no case is dropped and no percentile
is taken, every path and both outputs are compared elementwise. The
envelope is useful: the median of envelope(fv) / |fv| over all cases is at
most 64 U24. On the CPU the normals are philox_normal4_np, whose integer
core is checked here against Python-integer vectors, because on the GPU it
judges the device. Each test prints its figures.
"""

import functools

import numpy as np
import pytest

import mc_refs as mr
from ai_crypto_trader_amd.ops.montecarlo import (
    philox4x32_np, philox_normal4_np,
)
from mc_refs import U24

ROOM = 0.5
GBM_CASES = mr.VALU_CASES + mr.MFMA_CASES


@functools.lru_cache(maxsize=None)
def _gbm_ref(c):
    return mr.gbm_run(c, philox_normal4_np)


@functools.lru_cache(maxsize=None)
def _boot_ref(c):
    return mr.boot_run(c)


# --- RNG ------------------------------------------------------------------

# Philox4x32-10 known answers of the Random123 distribution: they validate
# the Python-integer implementation, which then judges the 7-round twin.
KAT10 = [
    ((0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    (((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
]
# 7 rounds, from the Python-integer implementation: every counter and key
# word non-zero in the second, the bootstrap tag bit set in the third
VEC7 = [
    ((9, 0, 0), (0x82CB025C, 0xED82D7CD, 0xCC8490F6, 0x249CDCBB)),
    (((1 << 32) + 9, (1 << 40) + 3, (2 << 32) | 1),
     (0xEE2039CC, 0x49DE6391, 0x2580599A, 0x0592DD34)),
    ((9, (1 << 32) + 5, (1 << 63) | 3),
     (0x5BEF2586, 0x892B16E5, 0x2AE3FF0A, 0x7B2D0ABA)),
]


def test_philox_np_matches_integer_vectors():
    for (seed, lo, hi), want in KAT10:
        assert mr.philox4x32_int(seed, lo, hi, rounds=10) == want
    for (seed, lo, hi), want in VEC7:
        assert mr.philox4x32_int(seed, lo, hi) == want
        got = philox4x32_np(seed, np.array([lo], np.uint64),
                            np.array([hi], np.uint64))
        assert tuple(int(x[0]) for x in got) == want
    rng = np.random.default_rng(41)
    raw = rng.integers(0, 1 << 64, (64, 3), dtype=np.uint64)
    for seed, lo, hi in raw.tolist():
        got = philox4x32_np(seed, np.array([lo], np.uint64),
                            np.array([hi], np.uint64))
        assert tuple(int(x[0]) for x in got) == \
            mr.philox4x32_int(seed, lo, hi)


def test_normals_floor_fixes_c_z():
    """The f32 twin against the f64 reference, reference against
    reference: the floor that C_Z is derived from."""
    seed, lo, hi = mr.rng_sample()
    z_ref, r_ref = mr.normals_ref(seed, lo, hi)
    q = mr.z_ratio(philox_normal4_np(seed, lo, hi), z_ref, r_ref)
    floor = float(q.max())
    print(f"normals: f32 twin worst |z - z_ref| / (U24 r) = {floor:.3g} "
          f"over {q.size} draws, C_Z = {mr.C_Z:g}")
    assert floor <= mr.C_Z_CPU_FLOOR
    assert mr.C_Z == 2.0 ** np.ceil(np.log2(4 * floor))
    assert np.abs(z_ref).max() > 4.5         # the sample reaches the tails


def test_box_muller_ref_edges():
    z, r = mr.box_muller_ref([0xFFFFFFFF, 0, 0x7FFFFFFF],
                             [0x3FFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF])
    assert r[0] == 0.0 and (z[0] == 0.0).all()
    assert abs(r[1] - np.sqrt(64 * np.log(2.0))) < 1e-12     # u = 2^-32
    assert np.isfinite(z).all()


# --- emulations inside ----------------------------------------------------

def _inside(c, fv, dd, res):
    rf, rd = mr.worst(fv, dd, res, room=ROOM)
    med = float(np.median(mr.useful(res)))
    print(f"{c.id}: emulation fv {rf:.3g} dd {rd:.3g} of the envelope / 2, "
          f"median envelope(fv)/|fv| {med / U24:.3g} U24")
    assert rf <= 1.0 and rd <= 1.0, (rf, rd)
    assert np.isfinite(res["env_fv"]).all()
    assert np.isfinite(res["env_dd"]).all()


@pytest.mark.parametrize("c", GBM_CASES, ids=mr.case_id)
def test_gbm_emulation_inside_envelope(c):
    fv, dd = mr.gbm_emulate(c, philox_normal4_np)
    res = _gbm_ref(c)
    _inside(c, fv, dd, res)
    if c.kind == "monotone":
        assert (res["dd"] == 0.0).all() and (dd == 0.0).all()
        v0 = float(mr.gbm_terms(mr.gbm_inputs(c.A, c.kind))[3])
        assert (res["fv"] > v0).all()


def test_gbm_wrap_emulation_inside_envelope():
    c, paths = mr.WRAP_CASE, mr.wrap_paths()
    assert c.n_paths > mr.MAX_GRID_PATHS and c.n_paths % 2 == 0
    half = c.n_paths // 2
    assert paths.min() == 0 and paths.max() == c.n_paths - 1
    assert ((paths >= half).sum() > 128) and ((paths < half).sum() > 128)
    fv, dd = mr.gbm_emulate(c, philox_normal4_np, paths)
    _inside(c, fv, dd, mr.gbm_run(c, philox_normal4_np, paths))


@pytest.mark.parametrize("c", mr.BOOT_CASES, ids=mr.case_id)
def test_boot_emulation_inside_envelope(c):
    fv, dd = mr.boot_emulate(c)
    res = _boot_ref(c)
    _inside(c, fv, dd, res)
    if c.t_hist == 1:
        terms = mr.boot_terms(*mr.boot_inputs(c.A, 1))
        closed = mr.boot_closed_form(c, terms)
        assert (fv == fv[0]).all() and (dd == dd[0]).all()
        assert (mr.ratio(np.full_like(res["fv"], closed), res["fv"],
                         res["env_fv"]) <= 1.0).all()


def test_envelopes_are_useful():
    """Held by the reference alone: no kernel result enters."""
    u = [mr.useful(_gbm_ref(c)) for c in GBM_CASES]
    u += [mr.useful(_boot_ref(c)) for c in mr.BOOT_CASES]
    worst_case = max(float(np.median(x)) for x in u)
    med = float(np.median(np.concatenate(u)))
    print(f"median envelope(fv)/|fv| over all cases {med / U24:.3g} U24, "
          f"largest per-case median {worst_case / U24:.3g} U24")
    assert med <= mr.USEFUL_CAP


# --- mutants outside ------------------------------------------------------

VALU_MUTANT_CASES = [c for c in mr.VALU_CASES if c.kind == "general"
                     and c.A in (4, 8) and c.antithetic]
MFMA_MUTANT_CASES = [c for c in mr.MFMA_CASES
                     if c.antithetic and c.n_paths <= 1000]
BOOT_MUTANT_CASES = [c for c in mr.BOOT_CASES
                     if c.A in (4, 8) and c.t_hist > 1]


@functools.lru_cache(maxsize=None)
def _mutant_ratio(family, mutant):
    """Largest |mutant - ref| / envelope over both outputs, every path and
    every case of the family."""
    best = 0.0
    if family == "boot":
        for c in BOOT_MUTANT_CASES:
            m = mr.boot_run(c, mutant=mutant)
            best = max(best, *mr.worst(m["fv"], m["dd"], _boot_ref(c)))
        return best
    cases = VALU_MUTANT_CASES if family == "valu" else MFMA_MUTANT_CASES
    for c in cases:
        m = mr.gbm_run(c, philox_normal4_np, mutant=mutant)
        best = max(best, *mr.worst(m["fv"], m["dd"], _gbm_ref(c)))
    return best


ALL_MUTANTS = ([("valu", m) for m in mr.GBM_MUTANTS]
               + [("mfma", m) for m in mr.GBM_MUTANTS + mr.MFMA_MUTANTS]
               + [("boot", m) for m in mr.BOOT_MUTANTS])


@pytest.mark.parametrize("family,mutant", ALL_MUTANTS,
                         ids=[f"{f}-{m}" for f, m in ALL_MUTANTS])
def test_mutant_outside_envelope(family, mutant):
    r = _mutant_ratio(family, mutant)
    print(f"{family} mutant {mutant}: {r:.3g} envelopes")
    assert r > 1.0, (family, mutant, r)


def test_weakest_mutant():
    r = {fm: _mutant_ratio(*fm) for fm in ALL_MUTANTS}
    fm = min(r, key=r.get)
    print(f"weakest mutant: {fm[0]} {fm[1]} at {r[fm]:.3g} envelopes")
    assert r[fm] > 1.0


@pytest.mark.parametrize("mutant", mr.EQUIVALENT_MUTANTS)
def test_equivalent_mutant_is_bit_equal(mutant):
    """A defect the outputs cannot show is recorded as such, not counted
    as caught."""
    for c in VALU_MUTANT_CASES + MFMA_MUTANT_CASES:
        m, res = mr.gbm_run(c, philox_normal4_np, mutant=mutant), _gbm_ref(c)
        assert (m["fv"] == res["fv"]).all() and (m["dd"] == res["dd"]).all()
    for c in BOOT_MUTANT_CASES:
        m, res = mr.boot_run(c, mutant=mutant), _boot_ref(c)
        assert (m["fv"] == res["fv"]).all() and (m["dd"] == res["dd"]).all()
