"""lstm_seq_fwd / _bwd and gru_seq_fwd / _bwd (ops/hip/lstm.hip, gru.hip)
against per-step f64 references, per element, inside the envelopes derived
in tests/rnn_refs.py (validated on a CPU by test_rnn_refs_cpu.py). The
kernels are called through the raw bindings; every test prints its worst
error / envelope and where it sits before asserting.

What each is there to catch:
  forward     b_hh indexing per gate and column (non-zero, all different),
              an error confined to one gate, one column, one 16-row slab,
              t = 0 or the last step, the second batch tile's offsets,
              T = 1, T = 60, gates saturated to exactly 0 / 1 / +-1
  backward    <32> and <64> alike, second batch tile, c_prev / h_prev at
              t = 0, the dc and dh chains, the recurrent GEMM; the saved
              tensors come from an f64 forward, so a forward defect can
              neither cause nor hide a failure here
  guard bands a store past T * B rows, or an element never written
  inference   save_mode 0 with null save pointers: the same h, bit for bit
  autograd    what models/{lstm,gru}.py build around the kernels: dgates
              passed through, dW_hh and db_hh, the GRU's h-side n column
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rnn_refs as rr  # noqa: E402
from kernel_refs import bf16_round  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ops():
    from ai_crypto_trader_amd.ops import require_hip_ops
    return require_hip_ops()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dev():
    return torch.device("cuda:0")


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(_dev()).bfloat16()


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(_dev())


def _guarded(T, B, width, dtype):
    """(T * B + 64, width), all NaN: the kernel gets the data_ptr."""
    return torch.full((T * B + rr.GUARD_ROWS, width), float("nan"),
                      dtype=dtype, device=_dev())


def _body(buf, T, B, name):
    body, tail = buf[:T * B].float(), buf[T * B:].float()
    assert torch.isnan(tail).all(), f"{name}: wrote past T * B rows"
    assert torch.isfinite(body).all(), f"{name}: element not written"
    return body.reshape(T, B, -1).cpu().numpy()


def _fwd(G, xproj, W, b, save_mode):
    """Forward launch of family G (4: LSTM, 3: GRU) on guarded outputs."""
    T, B, GH = xproj.shape
    H = GH // G
    bf = torch.bfloat16
    xp, wt, bias = _bf16(xproj), _bf16(W.T), _f32(b)
    h = _guarded(T, B, H, bf)
    if save_mode:
        gates = _guarded(T, B, GH, bf)
        aux = _guarded(T, B, H, torch.float32)
        gp, ap = gates.data_ptr(), aux.data_ptr()
    else:
        gates = aux = None
        gp = ap = 0
    fn = _ops().lstm_seq_fwd if G == 4 else _ops().gru_seq_fwd
    fn(xp.data_ptr(), wt.data_ptr(), bias.data_ptr(), h.data_ptr(), gp, ap,
       B, T, H, save_mode, _stream(_dev()))
    torch.cuda.synchronize()
    return h, gates, aux


@functools.lru_cache(maxsize=None)
def _fwd_case(G, case):
    """Kernel outputs of one forward case in both save modes (read-only,
    shared by the tests that need them)."""
    H, B, T, _ = case
    xproj, W, b, _ = rr.rnn_inputs(G, case)
    h, gates, aux = _fwd(G, xproj, W, b, 1)
    h0, _, _ = _fwd(G, xproj, W, b, 0)
    out = dict(h=_body(h, T, B, "h"), gates=_body(gates, T, B, "gates"),
               aux=_body(aux, T, B, "c / hp_n"),
               h_infer=_body(h0, T, B, "h (inference)"))
    out["infer_equal"] = torch.equal(h[:T * B], h0[:T * B])
    return xproj, W, b, out


def _report(tag, case, got, res):
    H = case[0]
    worst = {}
    for name, triple in res.items():
        r, idx = rr.worst(got[name], triple)
        worst[name] = r
        print(f"{tag} {rr.case_id(case)} {name}: {r:.3g} of the envelope "
              f"at {rr.where_str(idx, H)}")
    for name, r in worst.items():
        assert r <= 1.0, (tag, name, r)


# --- forward --------------------------------------------------------------

@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_lstm_fwd_inside_envelope(dev, case):
    xproj, W, b, out = _fwd_case(4, case)
    res = rr.lstm_fwd_ref(xproj, W, b, out["h"], out["aux"])
    _report("lstm_fwd", case,
            dict(gates=out["gates"], c=out["aux"], h=out["h"]), res)
    assert out["infer_equal"], "save_mode 0 changed h"


@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_gru_fwd_inside_envelope(dev, case):
    xproj, W, b, out = _fwd_case(3, case)
    res = rr.gru_fwd_ref(xproj, W, b, out["h"])
    _report("gru_fwd", case,
            dict(gates=out["gates"], hpn=out["aux"], h=out["h"]), res)
    assert out["infer_equal"], "save_mode 0 changed h"


@pytest.mark.parametrize("G", [4, 3], ids=["lstm", "gru"])
@pytest.mark.parametrize("H", rr.RNN_HS)
def test_saturated_gates_are_exact(dev, G, H):
    """exp overflows to inf on one side and underflows on the other:
    v_rcp(inf) = 0, and the gates land on 0, 1 and +-1 exactly."""
    case = (H, 128, 2, True)
    out = _fwd_case(G, case)[3]
    g = out["gates"][:, rr.sat_rows(case), :].reshape(-1, G, H)
    tanh_gate = 2
    for k in range(G):
        want = {-1.0, 1.0} if k == tanh_gate else {0.0, 1.0}
        assert set(np.unique(g[:, k])) == want, (k, np.unique(g[:, k]))


# --- backward -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lstm_bwd_case(case):
    H, B, T, _ = case
    xproj, W, b, dh_up = rr.rnn_inputs(4, case)
    gates, c, _ = rr.lstm_forward_f64(xproj, W, b)
    dg = _guarded(T, B, 4 * H, torch.bfloat16)
    args = (_f32(dh_up), _bf16(gates), _f32(c), _bf16(W))
    _ops().lstm_seq_bwd(*(a.data_ptr() for a in args), dg.data_ptr(), B, T,
                        H, _stream(_dev()))
    torch.cuda.synchronize()
    return dh_up, gates, c, W, _body(dg, T, B, "dgates")


@pytest.mark.parametrize("case", rr.RNN_CASES, ids=rr.case_id)
def test_lstm_bwd_inside_envelope(dev, case):
    dh_up, gates, c, W, dg = _lstm_bwd_case(case)
    _report("lstm_bwd", case, dict(dgates=dg),
            rr.lstm_bwd_ref(dh_up, gates, c, W, dg))


@functools.lru_cache(maxsize=None)
def _gru_bwd_case(case):
    H, B, T, _ = case
    xproj, W, b, dh_up = rr.rnn_inputs(3, case)
    gates, hpn, h = rr.gru_forward_f64(xproj, W, b)
    dg = _guarded(T, B, 3 * H, torch.bfloat16)
    args = (_f32(dh_up), _bf16(gates), _f32(hpn), _bf16(h), _bf16(W))
    _ops().gru_seq_bwd(*(a.data_ptr() for a in args), dg.data_ptr(), B, T,
                       H, _stream(_dev()))
    torch.cuda.synchronize()
    return dh_up, gates, hpn, h, W, _body(dg, T, B, "dgates")


@pytest.mark.parametrize("case", rr.GRU_BWD_CASES, ids=rr.case_id)
def test_gru_bwd_inside_envelope(dev, case):
    """Chain mode at T <= 3, anchored mode at T = 7 and 60."""
    dh_up, gates, hpn, h, W, dg = _gru_bwd_case(case)
    anchored = case[2] > rr.GRU_CHAIN_MAX_T
    _report("gru_bwd " + ("anchored" if anchored else "chain"), case,
            dict(dgates=dg),
            rr.gru_bwd_ref(dh_up, gates, hpn, h, W, dg, anchored))


# --- the torch side of the autograd functions -----------------------------

def _check_torch_side(tag, H, h_out, dg_for_gemm, w_grad, b_grad):
    (dw, tol_w, _), (db, tol_b, _) = rr.weight_grad_ref(h_out, dg_for_gemm)
    r_w = rr.worst(w_grad, (dw, tol_w, 0.0))
    r_b = rr.worst(b_grad, (db, tol_b, 0.0))
    print(f"{tag} H{H}: w_hh.grad {r_w[0]:.3g} at {r_w[1]}, b_hh.grad "
          f"{r_b[0]:.3g} at {r_b[1]} of the envelope")
    assert r_w[0] <= 1.0
    assert r_b[0] <= 1.0


@pytest.mark.parametrize("G", [4, 3], ids=["lstm", "gru"])
@pytest.mark.parametrize("H", rr.RNN_HS)
def test_autograd_function_torch_side(dev, G, H):
    from ai_crypto_trader_amd.models.gru import _FusedGRUSeq
    from ai_crypto_trader_amd.models.lstm import _FusedLSTMSeq

    case = (H, 128, 7, False)
    _, B, T, _ = case
    xproj, W, b, dh_up = rr.rnn_inputs(G, case)
    dh_up = bf16_round(dh_up)           # the output, and so its grad, is bf16
    xp = _bf16(xproj).requires_grad_(True)
    w_hh = _f32(W).requires_grad_(True)
    b_hh = _f32(b).requires_grad_(True)
    fn = _FusedLSTMSeq if G == 4 else _FusedGRUSeq
    h = fn.apply(xp, w_hh, b_hh)
    h.backward(_bf16(dh_up))
    torch.cuda.synchronize()

    # the same launches through the raw bindings
    _, _, _, out = _fwd_case(G, case)
    assert torch.equal(h.detach().float().cpu(),
                       torch.from_numpy(out["h"]))
    ops, s = _ops(), _stream(dev)
    dg = torch.empty((T, B, G * H), dtype=torch.bfloat16, device=dev)
    gates, aux, hk = _bf16(out["gates"]), _f32(out["aux"]), _bf16(out["h"])
    up, w = _f32(dh_up), _bf16(W)
    if G == 4:
        ops.lstm_seq_bwd(up.data_ptr(), gates.data_ptr(), aux.data_ptr(),
                         w.data_ptr(), dg.data_ptr(), B, T, H, s)
    else:
        ops.gru_seq_bwd(up.data_ptr(), gates.data_ptr(), aux.data_ptr(),
                        hk.data_ptr(), w.data_ptr(), dg.data_ptr(), B, T,
                        H, s)
    torch.cuda.synchronize()
    assert xp.grad.dtype == torch.bfloat16
    assert torch.equal(xp.grad, dg)
    dg = dg.float().cpu().numpy()
    if G == 3:
        dg = rr.gru_h_side(dg, out["gates"], H)
    assert w_hh.grad.dtype == torch.float32 and w_hh.grad.shape == (H, G * H)
    _check_torch_side("lstm" if G == 4 else "gru", H, out["h"], dg,
                      w_hh.grad.cpu().numpy(), b_hh.grad.cpu().numpy())


# --- arguments ------------------------------------------------------------

def test_gru_bad_arguments_raise_before_launch(dev):
    ops = _ops()
    s = _stream(dev)
    # one shared guard: every message names its caller
    for B, H in [(32, 64), (96, 64), (0, 64), (-64, 64), (64, 48)]:
        with pytest.raises(RuntimeError, match="gru_fwd: "):
            ops.gru_seq_fwd(0, 0, 0, 0, 0, 0, B, 4, H, 0, s)
        with pytest.raises(RuntimeError, match="gru_bwd: "):
            ops.gru_seq_bwd(0, 0, 0, 0, 0, 0, B, 4, H, s)
        with pytest.raises(RuntimeError, match="lstm_fwd: "):
            ops.lstm_seq_fwd(0, 0, 0, 0, 0, 0, B, 4, H, 0, s)
        with pytest.raises(RuntimeError, match="lstm_bwd: "):
            ops.lstm_seq_bwd(0, 0, 0, 0, 0, B, 4, H, s)
