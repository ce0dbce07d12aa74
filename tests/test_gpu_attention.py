"""attn_fwd / attn_bwd (ops/hip/attention.hip) against f64 softmax
attention and its f64 gradients, per element, inside the bf16 envelopes
derived in tests/kernel_refs.py (validated on a CPU by
test_kernel_refs_cpu.py). Every test prints its figures before asserting.

What each is there to catch:
  forward        an error confined to one 16-row wave slab, one fragment
                 column tile or the padded tail (the envelope is per
                 element, and key/value rows carry distinct offsets), a
                 wrong scale, overflow without max-subtraction, BH = 1
  saved P        weight on masked columns, unnormalised rows, a P that
                 differs from the one the output was built from
  backward       every D instantiation (32 and 64 had never run), scale
                 missing in dS, the rowsum correction, dS vs dS^T, padded
                 rows leaking into dK/dV
  guard bands    a store past row S (the `row < s_len` guards) or a row
                 never written, forward and backward
  independence   a block reading or writing another block's slab
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kernel_refs as kr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf16(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).bfloat16()


def _np(t):
    return t.float().cpu().numpy()


def _forward(dev, case, backward=False):
    from ai_crypto_trader_amd.models.attention import attn_fwd_hip

    Q, K, V, dO, scale = kr.attn_case(case, backward=backward)
    ref = kr.attn_ref(Q, K, V, dO, scale)
    q, k, v, go = (_bf16(dev, t) for t in (Q, K, V, dO))
    # scale=None takes the wrapper's default 1/sqrt(D)
    o, p = attn_fwd_hip(q, k, v, scale=case[3], save_p=True)
    torch.cuda.synchronize()
    return ref, (q, k, v, go, scale), o, p


@pytest.mark.parametrize("case", kr.ATT_FWD_CASES, ids=kr.attn_case_id)
def test_attn_fwd_inside_envelope(dev, case):
    from ai_crypto_trader_amd.models.attention import attn_fwd_hip

    S = case[1]
    ref, (q, k, v, _, _), o, p = _forward(dev, case)
    o_plain = attn_fwd_hip(q, k, v, scale=case[3])      # P_out == nullptr
    torch.cuda.synchronize()
    assert torch.equal(o, o_plain)
    p = _np(p).astype(np.float64)
    r_o = kr.worst_ratio(_np(o), ref["O"], ref["tol_O"])
    r_p = kr.worst_ratio(p[:, :S, :S], ref["P"], ref["tol_P"])
    rows = np.abs(p[:, :S].sum(axis=-1) - 1.0).max()
    print(f"attn_fwd {kr.attn_case_id(case)}: O {r_o:.3g} P {r_p:.3g} "
          f"of the envelope, rowsum off by {rows:.3g}")
    assert r_o <= 1.0
    assert r_p <= 1.0
    assert not p[:, :S, S:].any()           # masked keys: exactly zero
    assert rows <= 64 * 2.0 ** -9


@pytest.mark.parametrize("case", kr.ATT_BWD_CASES, ids=kr.attn_case_id)
def test_attn_bwd_inside_envelope(dev, case):
    from ai_crypto_trader_amd.models.attention import attn_bwd_hip

    ref, (q, k, v, go, scale), _, p = _forward(dev, case, backward=True)
    dq, dk, dv = attn_bwd_hip(q, k, v, p, go, scale)
    torch.cuda.synchronize()
    r = {n: kr.worst_ratio(_np(g), ref[n], ref["tol_" + n])
         for n, g in (("dQ", dq), ("dK", dk), ("dV", dv))}
    print(f"attn_bwd {kr.attn_case_id(case)}: " + " ".join(
        f"{n} {x:.3g}" for n, x in r.items()) + " of the envelope")
    for n, x in r.items():
        assert x <= 1.0, n


@pytest.mark.parametrize("D", kr.ATT_DS)
def test_fused_attention_autograd(dev, D):
    """One pass through fused_attention(...).backward per instantiation,
    (B, H, S, D) layout, the same envelopes."""
    from ai_crypto_trader_amd.models.attention import fused_attention

    B, H, S = 1, kr.ATT_BH, 60
    case = (B * H, S, D, None, None)
    Q, K, V, dO, scale = kr.attn_case(case, backward=True)
    ref = kr.attn_ref(Q, K, V, dO, scale)
    q, k, v = (torch.from_numpy(t).to(dev).reshape(B, H, S, D)
               .requires_grad_(True) for t in (Q, K, V))
    o = fused_attention(q, k, v)
    o.backward(torch.from_numpy(dO).to(dev).reshape(B, H, S, D).to(o.dtype))
    torch.cuda.synchronize()
    r = {"O": kr.worst_ratio(_np(o.detach()).reshape(B * H, S, D),
                             ref["O"], ref["tol_O"])}
    for n, t in (("dQ", q), ("dK", k), ("dV", v)):
        assert t.grad.dtype == torch.float32
        r[n] = kr.worst_ratio(_np(t.grad).reshape(B * H, S, D), ref[n],
                              ref["tol_" + n])
    print(f"fused_attention D={D}: " + " ".join(
        f"{n} {x:.3g}" for n, x in r.items()) + " of the envelope")
    for n, x in r.items():
        assert x <= 1.0, n


def _guarded(dev, BH, S, D):
    """A (BH, S, D) bf16 buffer followed by a 64 * D guard band, all
    sentinel. Returns the flat tensor; the kernel gets its data_ptr."""
    n = BH * S * D + kr.ATT_S * D
    return torch.full((n,), kr.ATT_SENTINEL, dtype=torch.bfloat16,
                      device=dev)


def _check_guard(buf, BH, S, D, name):
    body = buf[:BH * S * D].float()
    tail = buf[BH * S * D:].float()
    assert (tail == kr.ATT_SENTINEL).all(), f"{name}: wrote past row S"
    assert (body != kr.ATT_SENTINEL).all(), f"{name}: rows not written"
    return body.reshape(BH, S, D)


@pytest.mark.parametrize("S", kr.ATT_GUARD_SS)
@pytest.mark.parametrize("D", kr.ATT_DS)
def test_attn_store_guards(dev, D, S):
    """Raw bindings, outputs allocated 64 * D elements longer than
    (BH, S, D) and filled with a sentinel: the tail stays untouched and
    every row below S is written, in O and in dQ / dK / dV. The results
    equal the wrappers' bit for bit."""
    from ai_crypto_trader_amd.models.attention import (
        attn_bwd_hip, attn_fwd_hip,
    )
    from ai_crypto_trader_amd.ops import require_hip_ops

    ops = require_hip_ops()
    BH = kr.ATT_BH
    Q, K, V, dO, scale = kr.attn_case((BH, S, D, None, None),
                                      backward=True)
    q, k, v, go = (_bf16(dev, t) for t in (Q, K, V, dO))
    stream = torch.cuda.current_stream(dev).cuda_stream
    o = _guarded(dev, BH, S, D)
    p = torch.empty((BH, kr.ATT_S, kr.ATT_S), dtype=torch.bfloat16,
                    device=dev)
    ops.attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                 p.data_ptr(), BH, S, D, scale, stream)
    dq, dk, dv = (_guarded(dev, BH, S, D) for _ in range(3))
    ops.attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), p.data_ptr(),
                 go.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                 dv.data_ptr(), BH, S, D, scale, stream)
    torch.cuda.synchronize()
    o_w, p_w = attn_fwd_hip(q, k, v, save_p=True)
    grads_w = attn_bwd_hip(q, k, v, p_w, go, scale)
    torch.cuda.synchronize()
    assert torch.equal(_check_guard(o, BH, S, D, "O"), o_w.float())
    assert torch.equal(p, p_w)
    for name, buf, want in zip(("dQ", "dK", "dV"), (dq, dk, dv), grads_w):
        assert torch.equal(_check_guard(buf, BH, S, D, name), want.float())


@pytest.mark.parametrize("D", kr.ATT_DS)
def test_attn_block_independence(dev, D):
    """bh = 1 alone and as the middle block of BH = 3: bit-equal."""
    from ai_crypto_trader_amd.models.attention import (
        attn_bwd_hip, attn_fwd_hip,
    )

    S = 60
    Q, K, V, dO, scale = kr.attn_case((kr.ATT_BH, S, D, None, None),
                                      backward=True)
    q, k, v, go = (_bf16(dev, t) for t in (Q, K, V, dO))
    o3, p3 = attn_fwd_hip(q, k, v, save_p=True)
    g3 = attn_bwd_hip(q, k, v, p3, go, scale)
    q1, k1, v1, go1 = (t[1:2].contiguous() for t in (q, k, v, go))
    o1, p1 = attn_fwd_hip(q1, k1, v1, save_p=True)
    g1 = attn_bwd_hip(q1, k1, v1, p1, go1, scale)
    torch.cuda.synchronize()
    assert torch.equal(o1, o3[1:2]) and torch.equal(p1, p3[1:2])
    for a, b in zip(g1, g3):
        assert torch.equal(a, b[1:2])
