"""ga_evolve_kernel and ga_evolve_generic_kernel against the exact twin of
tests/ga_refs.py (validated on a CPU by test_ga_refs_cpu.py).

The twin consumes the device's own normals, read through the philox_probe
binding (component 2 of the four is box_muller(z, w).x), so its envelope
holds only the kernel's arithmetic on a mutated slot. Everything else is
compared bit for bit: elite rows against a stable order, every slot that
is not mutated, every integer slot outside the undecidable set. Each case
runs through the raw binding (NaN fitness reaches the kernel as given) and
through the wrapper (which maps NaN to -inf and sorts itself); the output
of the raw call has NaN guard rows on both sides that must stay untouched.
Each test prints its worst fraction of the envelope.
"""

from pathlib import Path

import numpy as np
import pytest

import ga_refs as gr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD_ROWS = 4
GOLDEN = Path(__file__).parent / "golden" / "ga_children.npz"


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


def _device_normals(ops, dev):
    def fn(seed, lo, hi):
        n = int(np.asarray(lo).size)
        t_lo, t_hi = _u64(lo, dev), _u64(hi, dev)
        words = torch.empty((n, 4), dtype=torch.int32, device=dev)
        normals = torch.empty((n, 4), dtype=torch.float32, device=dev)
        ops.philox_probe(seed, t_lo.data_ptr(), t_hi.data_ptr(),
                         words.data_ptr(), normals.data_ptr(), n,
                         _stream(dev))
        torch.cuda.synchronize()
        return normals.cpu().numpy()
    return fn


def _raw(ops, dev, c, pop, fit, order, bounds):
    """The kernel through its binding, into a guarded buffer."""
    P, n = pop.shape
    buf = torch.full((P + 2 * GUARD_ROWS, n), float("nan"),
                     dtype=torch.float32, device=dev)
    out = buf[GUARD_ROWS:GUARD_ROWS + P]
    assert out.is_contiguous()
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev)
         for x in (pop, fit, order, bounds)]
    tail = (c.elite_k, c.tournament, c.cx_rate, c.mut_rate, c.mut_scale,
            c.seed, c.gen, _stream(dev))
    if c.family == "vote":
        ops.ga_evolve(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                      t[3].data_ptr(), out.data_ptr(), P, *tail)
    else:
        ops.ga_evolve_generic(t[0].data_ptr(), t[1].data_ptr(),
                              t[2].data_ptr(), t[3].data_ptr(),
                              out.data_ptr(), P, n, *tail)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.isnan(b[:GUARD_ROWS]).all(), "write before the output"
    assert np.isnan(b[GUARD_ROWS + P:]).all(), "write past the output"
    return b[GUARD_ROWS:GUARD_ROWS + P]


def _wrapper(dev, c, pop, fit, bounds, transpose=False):
    from ai_crypto_trader_amd.ops.ga import (
        ga_evolve_family_gpu, ga_evolve_gpu,
    )
    if transpose:       # dense, not contiguous: column-major storage
        pop_t = torch.from_numpy(np.ascontiguousarray(pop.T)).to(dev).t()
        assert pop_t.shape == pop.shape and (
            not pop_t.is_contiguous() or min(pop.shape) == 1)
    else:
        pop_t = torch.from_numpy(pop).to(dev)
    fit_t = torch.from_numpy(fit).to(dev)
    b_t = torch.from_numpy(bounds).to(dev)
    kw = dict(elite_k=c.elite_k, tournament=c.tournament, cx_rate=c.cx_rate,
              mut_rate=c.mut_rate, mut_scale=c.mut_scale, seed=c.seed,
              gen=c.gen)
    if c.family == "vote":
        out = ga_evolve_gpu(pop_t, fit_t, bounds_t=b_t, **kw)
    else:
        out = ga_evolve_family_gpu(pop_t, fit_t, b_t, **kw)
    torch.cuda.synchronize()
    assert out.is_contiguous() and out.dtype == torch.float32
    assert tuple(out.shape) == pop.shape
    return out.cpu().numpy()


def _hold(tag, got, res):
    h = gr.hold(got, res)
    assert h["bad"] == 0, (tag, h)
    assert h["worst"] <= 1.0
    return h["worst"]


@pytest.mark.parametrize("c", gr.CASES, ids=gr.case_id)
def test_evolve_matches_twin(dev, ops, c):
    pop, fit, order, bounds = gr.case_inputs(c)
    res = gr.run_case(c, normal_fn=_device_normals(ops, dev))
    n_und, n_mut, share = gr.undecidable_share(res)
    assert share <= gr.UNDECIDABLE_CAP, (n_und, n_mut)
    raw = _raw(ops, dev, c, pop, fit, order, bounds)
    w_raw = _hold("raw", raw, res)
    wrapped = _wrapper(dev, c, pop, fit, bounds)
    w_wrap = _hold("wrapper", wrapped, res)
    # same kernel, same inputs up to NaN -> -inf: same bits
    np.testing.assert_array_equal(raw, wrapped)
    print(f"{c.id}: raw {w_raw:.3g} wrapper {w_wrap:.3g} of the envelope, "
          f"{n_und} of {n_mut} mutated integer slots undecidable")


@pytest.mark.parametrize("c", [gr.STANDARD, gr.STANDARD_GENERIC,
                               gr.HALF_BOUNDS], ids=gr.case_id)
def test_wrapper_takes_a_transposed_population(dev, ops, c):
    """A dense non-contiguous pop: the output is allocated contiguous, not
    with the input's strides."""
    pop, fit, order, bounds = gr.case_inputs(c)
    plain = _wrapper(dev, c, pop, fit, bounds)
    np.testing.assert_array_equal(
        _wrapper(dev, c, pop, fit, bounds, transpose=True), plain)


def test_wrapper_refuses_bad_arguments_on_device(dev):
    from ai_crypto_trader_amd.ops.ga import (
        ga_evolve_family_gpu, ga_evolve_gpu,
    )
    pop = torch.zeros(16, 19, device=dev)
    fit = torch.zeros(16, device=dev)
    b = torch.zeros(19, 3, device=dev)
    for kw in (dict(tournament=5), dict(tournament=8), dict(tournament=0),
               dict(elite_k=17), dict(elite_k=-1)):
        with pytest.raises(ValueError):
            ga_evolve_gpu(pop, fit, bounds_t=b, **kw)
        with pytest.raises(ValueError):
            ga_evolve_family_gpu(pop, fit, b, **kw)
    with pytest.raises(ValueError):
        ga_evolve_gpu(pop.double(), fit, bounds_t=b)
    with pytest.raises(ValueError):
        ga_evolve_family_gpu(pop, fit.cpu(), b)
    with pytest.raises(ValueError):
        ga_evolve_family_gpu(pop, fit[:-1], b)


def test_children_bit_identical_to_recorded_population(dev):
    """tests/golden/ga_children.npz holds children that the kernels
    produced before the parent fallback, the NaN rule and the stable sort
    went in, for finite tie-free fitness and tournament <= 4: those
    changes must not move a single bit of such a generation."""
    from ai_crypto_trader_amd.ops.ga import (
        ga_evolve_family_gpu, ga_evolve_gpu,
    )
    g = np.load(GOLDEN)
    fit_t = torch.from_numpy(g["fitness"]).to(dev)
    for tag, kw in gr.GOLDEN_RUNS.items():
        got = ga_evolve_gpu(torch.from_numpy(g["vote_pop"]).to(dev), fit_t,
                            **kw)
        np.testing.assert_array_equal(got.cpu().numpy(),
                                      g[f"vote_child_{tag}"])
        for name in ("grid", "dca"):
            b = torch.from_numpy(gr.bounds_for(name)).to(dev)
            got = ga_evolve_family_gpu(
                torch.from_numpy(g[f"{name}_pop"]).to(dev), fit_t, b, **kw)
            np.testing.assert_array_equal(got.cpu().numpy(),
                                          g[f"{name}_child_{tag}"])
