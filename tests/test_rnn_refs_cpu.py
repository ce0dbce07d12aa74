"""The envelopes of tests/rnn_refs.py, validated without a GPU.

For every case the GPU tests run, an f32 / bf16 emulation of the kernel's
arithmetic sits inside every per-step envelope, with 2x room on the part
that comes from f32 arithmetic (ROOM) and none on the B8 |value| part,
which is a hard bound. Every seeded mutant falls outside at some element.
Sharpness is a cap, not a measurement: per bf16 output, step and case the
median of envelope / (B8 |reference|) is at most 4, so a defect of a few
bf16 ulps in a typical element cannot hide. Each test prints its figures.
"""

import functools

import numpy as np
import pytest

import kernel_refs as kr
import rnn_refs as rr

torch = pytest.importorskip("torch")

ROOM = 0.5
BF16_OUTPUTS = ("gates", "h", "dgates")


@functools.lru_cache(maxsize=None)
def _lstm(case):
    xproj, W, b, dh_up = rr.rnn_inputs(4, case)
    gates, c, h = rr.lstm_forward_f64(xproj, W, b)
    return xproj, W, b, dh_up, gates, c


@functools.lru_cache(maxsize=None)
def _gru(case):
    xproj, W, b, dh_up = rr.rnn_inputs(3, case)
    gates, hpn, h = rr.gru_forward_f64(xproj, W, b)
    return xproj, W, b, dh_up, gates, hpn, h


def _inside(tag, case, got, res):
    H = case[0]
    for name, triple in res.items():
        r, idx = rr.worst(got[name], triple, room=ROOM)
        line = f"{tag} {rr.case_id(case)} {name}: emulation {r:.3g}"
        if name in BF16_OUTPUTS:
            med = max(rr.sharpness(triple))
            line += f", sharpness median {med:.3g}"
            assert med <= rr.SHARPNESS_CAP, (name, med)
        print(line + f" at {idx}")
        assert r <= 1.0, (name, r, idx)
        assert np.isfinite(triple[1]).all()


def _outside(tag, case, mutant, got, res):
    worst = {n: rr.worst(got[n], t)[0] for n, t in res.items()}
    print(f"{tag} {rr.case_id(case)} mutant {mutant}: "
          + " ".join(f"{n} {r:.3g}" for n, r in worst.items()))
    assert max(worst.values()) > 1.0, (mutant, worst)


MUTANT_CASES = [(H, 128, T, False) for H in rr.RNN_HS
                for T in rr.MUTANT_CASE_TS]


# --- LSTM -----------------------------------------------------------------

@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_lstm_fwd_emulation_inside_envelope(case):
    xproj, W, b = _lstm(case)[:3]
    emu = rr.lstm_fwd_emulate(xproj, W, b)
    _inside("lstm_fwd", case, emu,
            rr.lstm_fwd_ref(xproj, W, b, emu["h"], emu["c"]))
    if case[3]:         # saturated: both ends of every gate are reached
        g = emu["gates"][:, rr.sat_rows(case), :].reshape(-1, 4, case[0])
        for k in (0, 1, 3):
            assert set(np.unique(g[:, k])) == {0.0, 1.0}
        assert set(np.unique(g[:, 2])) == {-1.0, 1.0}


@pytest.mark.parametrize("mutant", rr.LSTM_FWD_MUTANTS)
@pytest.mark.parametrize("case", MUTANT_CASES, ids=rr.case_id)
def test_lstm_fwd_mutant_outside(case, mutant):
    xproj, W, b = _lstm(case)[:3]
    emu = rr.lstm_fwd_emulate(xproj, W, b, mutant=mutant)
    _outside("lstm_fwd", case, mutant, emu,
             rr.lstm_fwd_ref(xproj, W, b, emu["h"], emu["c"]))


@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_lstm_bwd_emulation_inside_envelope(case):
    _, W, _, dh_up, gates, c = _lstm(case)
    dg = rr.lstm_bwd_emulate(dh_up, gates, c, W)
    _inside("lstm_bwd", case, dict(dgates=dg),
            rr.lstm_bwd_ref(dh_up, gates, c, W, dg))


@pytest.mark.parametrize("mutant", rr.LSTM_BWD_MUTANTS)
@pytest.mark.parametrize("case", MUTANT_CASES, ids=rr.case_id)
def test_lstm_bwd_mutant_outside(case, mutant):
    _, W, _, dh_up, gates, c = _lstm(case)
    dg = rr.lstm_bwd_emulate(dh_up, gates, c, W, mutant=mutant)
    _outside("lstm_bwd", case, mutant, dict(dgates=dg),
             rr.lstm_bwd_ref(dh_up, gates, c, W, dg))


# --- GRU ------------------------------------------------------------------

@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_gru_fwd_emulation_inside_envelope(case):
    xproj, W, b = _gru(case)[:3]
    emu = rr.gru_fwd_emulate(xproj, W, b)
    _inside("gru_fwd", case, emu, rr.gru_fwd_ref(xproj, W, b, emu["h"]))
    if case[3]:
        g = emu["gates"][:, rr.sat_rows(case), :].reshape(-1, 3, case[0])
        for k in (0, 1):
            assert set(np.unique(g[:, k])) == {0.0, 1.0}
        assert set(np.unique(g[:, 2])) == {-1.0, 1.0}


@pytest.mark.parametrize("mutant", rr.GRU_FWD_MUTANTS)
@pytest.mark.parametrize("case", MUTANT_CASES, ids=rr.case_id)
def test_gru_fwd_mutant_outside(case, mutant):
    xproj, W, b = _gru(case)[:3]
    emu = rr.gru_fwd_emulate(xproj, W, b, mutant=mutant)
    _outside("gru_fwd", case, mutant, emu,
             rr.gru_fwd_ref(xproj, W, b, emu["h"]))


@pytest.mark.parametrize("case", rr.GRU_BWD_CASES, ids=rr.case_id)
def test_gru_bwd_emulation_inside_envelope(case):
    _, W, _, dh_up, gates, hpn, h = _gru(case)
    dg = rr.gru_bwd_emulate(dh_up, gates, hpn, h, W)
    anchored = case[2] > rr.GRU_CHAIN_MAX_T
    _inside("gru_bwd " + ("anchored" if anchored else "chain"), case,
            dict(dgates=dg),
            rr.gru_bwd_ref(dh_up, gates, hpn, h, W, dg, anchored))


@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("mutant", rr.GRU_BWD_MUTANTS)
@pytest.mark.parametrize("H", rr.RNN_HS)
def test_gru_bwd_mutant_outside(H, mutant, anchored):
    """Chain mode at its longest (T = 3), anchored mode at T = 7: a defect
    in the carried dh (drop_direct) shows in both."""
    case = (H, 128, 7 if anchored else rr.GRU_CHAIN_MAX_T, False)
    xproj, W, _, dh_up, gates, hpn, h = _gru(case)
    dg = rr.gru_bwd_emulate(dh_up, gates, hpn, h, W, mutant=mutant,
                            xproj=xproj)
    _outside("gru_bwd " + ("anchored" if anchored else "chain"), case,
             mutant, dict(dgates=dg),
             rr.gru_bwd_ref(dh_up, gates, hpn, h, W, dg, anchored))


def test_gru_bwd_chain_mode_loses_sharpness_beyond_three_steps():
    """Why anchored mode exists: at T = 7 the running bound on the carried
    dh already breaks the cap at the early steps."""
    case = (64, 64, 7, False)
    _, W, _, dh_up, gates, hpn, h = _gru(case)
    dg = rr.gru_bwd_emulate(dh_up, gates, hpn, h, W)
    chain = rr.sharpness(rr.gru_bwd_ref(dh_up, gates, hpn, h, W, dg,
                                        False)["dgates"])
    anch = rr.sharpness(rr.gru_bwd_ref(dh_up, gates, hpn, h, W, dg,
                                       True)["dgates"])
    print("gru_bwd H64 T7 sharpness by step, chain:",
          " ".join(f"{x:.2g}" for x in chain), "anchored:",
          " ".join(f"{x:.2g}" for x in anch))
    assert max(chain) > rr.SHARPNESS_CAP >= max(anch)


# --- torch side and number formats ----------------------------------------

def test_weight_grad_reference_shapes_and_bound():
    case = (32, 128, 7, False)
    _, W, _, dh_up, gates, c = _lstm(case)
    dg = rr.lstm_bwd_emulate(dh_up, gates, c, W)
    h = rr.lstm_forward_f64(*rr.rnn_inputs(4, case)[:3])[2]
    (dw, tol_w, _), (db, tol_b, _) = rr.weight_grad_ref(h, dg)
    assert dw.shape == (32, 128) and db.shape == (128,)
    # a bf16 GEMM with f32 accumulation, emulated: inside
    hp = np.concatenate([np.zeros_like(h[:1]), h[:-1]]).reshape(-1, 32)
    got = kr.bf16_round((hp.astype(np.float64).T
                         @ dg.reshape(-1, 128).astype(np.float64)
                         ).astype(np.float32))
    assert kr.worst_ratio(got, dw, tol_w) <= 1.0
    # the sum over t = 1.. only (h_prev not shifted) is far outside
    bad = h.reshape(-1, 32).astype(np.float64).T @ dg.reshape(-1, 128)
    assert kr.worst_ratio(bad, dw, tol_w) > 1.0


def test_gru_h_side_n_column():
    case = (32, 64, 2, False)
    _, _, _, _, gates, _, _ = _gru(case)
    dgx = kr.bf16_round(np.random.default_rng(3).standard_normal(
        gates.shape))
    out = rr.gru_h_side(dgx, gates, 32)
    np.testing.assert_array_equal(out[..., :64], dgx[..., :64])
    want = (torch.from_numpy(dgx[..., 64:]).bfloat16()
            * torch.from_numpy(gates[..., :32]).bfloat16())
    np.testing.assert_array_equal(out[..., 64:], want.float().numpy())


def test_bf16_round_ties_and_store_error():
    """bf16_round against torch.bfloat16 on exact ties (to even, both
    parities), their neighbours, signs, and random values; and the store
    error reaches but never exceeds B8 |x|, not B8 / 2."""
    base = np.array([0x3F80, 0x3F81, 0x4000, 0x7F7E, 0x0080, 0x3EFF],
                    np.uint32) << 16
    bits = np.concatenate([base + d for d in
                           (0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF)])
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])
    x = bits.astype(np.uint32).view(np.float32)
    rnd = np.random.default_rng(1).standard_normal(100_000).astype(
        np.float32)
    x = np.concatenate([x, rnd])
    want = torch.from_numpy(x).bfloat16().float().numpy()
    np.testing.assert_array_equal(kr.bf16_round(x), want)
    rel = np.abs(kr.bf16_round(rnd).astype(np.float64) - rnd) / np.abs(rnd)
    print(f"bf16 store error / |x|: max {rel.max() / kr.B8:.4f} of B8")
    assert kr.B8 / 2 < rel.max() <= kr.B8
    just_above_one = np.float32(1.0 + 2.0 ** -8 - 2.0 ** -20)
    assert kr.bf16_round(just_above_one) == 1.0
