"""Per-step f64 references, error envelopes and CPU emulations for the LSTM
and GRU sequence kernels (ops/hip/lstm.hip, ops/hip/gru.hip). A helper
module in the style of kernel_refs.py, no tests of its own.

Why per step. A free-running comparison over T steps cannot be sharp: the
bf16 rounding of h at step 1 is amplified through the recurrence, so an
honest bound is far above what a subtle defect produces. In training mode
the kernels store every intermediate (gates, c or hp_n, h going forward,
dgates going back), so the f64 reference of step t takes the kernel's OWN
stored outputs of step t-1 (forward) or t+1 (backward) as its inputs
(teacher forcing), and only one step's rounding lies between the two.

How an envelope is built. Every reference value is carried as a triple
(v, e, h): the f64 value, a bound e on what f32 arithmetic may add (the
"soft" part) and a bound h on what bf16 roundings upstream may add (the
"hard" part). Both are propagated by running error analysis:
    a + b : e_a + e_b            plus one f32 rounding U24 |a + b|
    a * b : |a| e_b + |b| e_a + e_a e_b     plus U24 |a b|
so cancellation is covered by absolute terms, and fma contraction (one
rounding where two are budgeted) only helps. A bf16 store of x adds
B8 |x|: round-to-nearest at 8 significant bits is off by up to 2^-9 of the
binade's upper end, i.e. up to 2^-8 |x| just above a power of two. The
envelope of a stored value is e + h + B8 (|v| + e + h). The CPU tests hold
an emulation to h-part + B8 |v| + HALF of e (2x room on the f32 part, none
needed on the bf16 part), and seeded mutants have to fall outside.

Figures that do not come from the number formats:
  * MFMA / f32 accumulation of n exact bf16 products in any order: off by
    at most n U24 sum|terms| (first order), as in kernel_refs.py.
  * sigmoid(x) = v_rcp_f32(1 + v_exp_f32(-x * log2e)). The instruction set
    reference gives v_exp_f32 and v_rcp_f32 1 ulp = 2 U24 each. The
    argument y = -x * log2e carries one rounding of the product and the
    f32 rounding of log2e (1.3e-8 relative, below U24): |dy| <= 2 U24 |y|,
    which exp2 turns into a relative 2 U24 ln2 |y| = 2 U24 |x|. With
    e = exp(-x), s = 1 / (1 + e) and ds/s = -de / (1 + e):
        |ds| <= s ((1 - s) (2 |x| + 2) + 3) U24
    (3 = one rounding of 1 + e and the 2 of v_rcp). v_exp_f32 flushes
    results below 2^-126; that moves s by less than 2^-126 and sits under
    every other term. tanh(x) = 2 sigmoid(2x) - 1 doubles the figure at 2x
    (2x and 2s are exact) and adds the rounding of the subtraction.
  * An input error passes through sigmoid with its Lipschitz constant 1/4
    and through tanh with 1.
No constant here was fitted to a GPU result.
"""

import numpy as np

from kernel_refs import B8, U24, _fma32, bf16_round

BM = 64                     # batch tile of every kernel
GUARD_ROWS = 64             # NaN tail behind every output in the GPU tests
SAT = 100.0                 # exact in bf16; exp(100) overflows f32

RNN_HS = (64, 32)
# (H, B, T, saturated)
RNN_CASES = tuple(
    [(H, B, T, False) for H in RNN_HS for B in (64, 128) for T in (1, 2, 7)]
    + [(H, 64, 60, False) for H in RNN_HS]
    + [(H, 128, 2, True) for H in RNN_HS])
# GRU backward: the carried dh is never stored, so its running bound grows
# geometrically; chain mode up to 3 steps, anchored mode beyond
GRU_BWD_CASES = tuple(
    [(H, B, T, False) for H in RNN_HS for B in (64, 128)
     for T in (1, 2, 3, 7)]
    + [(H, 64, 60, False) for H in RNN_HS]
    + [(H, 128, 2, True) for H in RNN_HS])
GRU_CHAIN_MAX_T = 3
SHARPNESS_CAP = 4.0         # median envelope / (B8 |ref|), a cap
MUTANT_CASE_TS = (7,)       # mutants run at B = 128, T = 7, both H


def case_id(case):
    H, B, T, sat = case
    return f"H{H}-B{B}-T{T}" + ("-sat" if sat else "")


def rnn_inputs(G, case):
    """xproj (T, B, G H) and W_hh (H, G H) on the bf16 grid, b_hh f32
    different for every gate and column, dh_up f32 independent of h.
    Every batch row differs. Saturated variant: rows 5 and B - 11 carry
    +-100 in every gate, the sign alternating by column and gate."""
    H, B, T, sat = case
    rng = np.random.default_rng([29, G, H, B, T, int(sat)])
    xproj = bf16_round(rng.standard_normal((T, B, G * H)))
    W = bf16_round(rng.standard_normal((H, G * H)) * H ** -0.5)
    b = (0.5 * rng.standard_normal(G * H)).astype(np.float32)
    dh_up = rng.standard_normal((T, B, H)).astype(np.float32)
    if sat:
        col = np.arange(G * H)
        sign = np.where((col + col // H) % 2 == 0, SAT, -SAT)
        for k, row in enumerate((5, B - 11)):
            xproj[:, row, :] = sign if k == 0 else -sign
    return xproj, W, b, dh_up


def sat_rows(case):
    return (5, case[1] - 11)


# --- values with error bounds ---------------------------------------------

def _abs(x):
    return np.abs(x)


class E:
    """(v, e, h), see the module header."""
    __slots__ = ("v", "e", "h")
    __array_ufunc__ = None      # ndarray (+|*) E defers to E

    def __init__(self, v, e=0.0, h=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)
        self.h = np.asarray(h, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    def _rounded(self, v, e, h):
        return E(v, e + U24 * (_abs(v) + e + h), h)

    def __add__(self, o):
        o = E.of(o)
        return self._rounded(self.v + o.v, self.e + o.e, self.h + o.h)

    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.e, self.h)

    def __sub__(self, o):
        return self + (-E.of(o))

    def __rsub__(self, o):
        return E.of(o) + (-self)

    def __mul__(self, o):
        o = E.of(o)
        a, b = _abs(self.v), _abs(o.v)
        e = a * o.e + b * self.e + self.e * o.e
        h = (a * o.h + b * self.h + self.h * o.h
             + self.e * o.h + self.h * o.e)
        return self._rounded(self.v * o.v, e, h)

    __rmul__ = __mul__

    def stored_bf16(self):
        """(ref, envelope, soft part) of the value stored as bf16."""
        tol = self.e + self.h + B8 * (_abs(self.v) + self.e + self.h)
        return self.v, tol, np.broadcast_to(self.e, self.v.shape)

    def stored_f32(self):
        return (self.v, np.broadcast_to(self.e + self.h, self.v.shape),
                np.broadcast_to(self.e, self.v.shape))

    def after_bf16(self):
        """The same value once it has been rounded to bf16 (the kernel
        goes on computing with the rounded one)."""
        return E(self.v, self.e,
                 self.h + B8 * (_abs(self.v) + self.e + self.h))


def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _sig_budget(x):
    s = _sigmoid64(x)
    return s * ((1.0 - s) * (2.0 * _abs(x) + 2.0) + 3.0) * U24


def sig_e(x):
    s = _sigmoid64(x.v)
    return E(s, 0.25 * x.e + _sig_budget(x.v), 0.25 * x.h)


def tanh_e(x):
    t = np.tanh(x.v)
    return E(t, x.e + 2.0 * _sig_budget(2.0 * x.v) + U24 * _abs(t), x.h)


def _preact(x, b, hp, W, nops):
    """x + b + hp @ W accumulated in f32 from exact inputs, any order."""
    hp = hp.astype(np.float64)
    W = W.astype(np.float64)
    v = x + b + hp @ W
    return E(v, nops * U24 * (_abs(x) + _abs(b) + _abs(hp) @ _abs(W)))


class Result(dict):
    """name -> (ref, tol, soft), each (T, ...)."""

    def put(self, name, t, triple, T):
        if name not in self:
            self[name] = tuple(np.zeros((T,) + triple[0].shape)
                               for _ in range(3))
        for dst, src in zip(self[name], triple):
            dst[t] = src


def worst(got, triple, room=0.0):
    """(max |got - ref| / (tol - room * soft), its index). An exact match
    counts as 0 also where the envelope is 0."""
    ref, tol, soft = triple
    err = _abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / (tol - room * soft))
    q = np.where(np.isnan(q), np.inf, q)
    k = np.unravel_index(np.argmax(q), q.shape)
    return float(q[k]), tuple(int(i) for i in k)


def sharpness(triple):
    """Per step, the median of envelope / (B8 |ref|). Elements whose
    reference and envelope are both exactly zero (a gradient through a
    gate at exactly 0 or 1, or through c_prev = 0 at t = 0) carry no
    rounding at all and are left out; a step of nothing else counts 0."""
    ref, tol, _ = triple
    out = []
    for t in range(ref.shape[0]):
        r, e = _abs(ref[t]).ravel(), tol[t].ravel()
        live = ~((r == 0.0) & (e == 0.0))
        with np.errstate(divide="ignore"):
            out.append(float(np.median(e[live] / (B8 * r[live])))
                       if live.any() else 0.0)
    return out


def where_str(idx, H):
    t, row, col = idx
    return f"t={t} row={row} gate={col // H} col={col % H}"


# --- f32 / bf16 emulation primitives --------------------------------------

_ONE = np.float32(1.0)
_TWO = np.float32(2.0)


def _sig32(x):
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(np.float64)).astype(np.float32)
        return (_ONE / (_ONE + e)).astype(np.float32)


def _tanh32(x):
    with np.errstate(over="ignore"):
        e = np.exp(-2.0 * x.astype(np.float64)).astype(np.float32)
        return (_TWO * (_ONE / (_ONE + e)) - _ONE).astype(np.float32)


def _mm32(acc, A, Bm):
    """acc + A @ Bm as a chain of f32 fmas over k."""
    acc = acc.astype(np.float32)
    for k in range(A.shape[1]):
        acc = _fma32(acc, A[:, k, None], Bm[None, k, :])
    return acc


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ===========================================================================
# LSTM
# ===========================================================================
LSTM_FWD_MUTANTS = ("drop_bias_o", "gate_order", "swap_w_rows", "stale_h",
                    "tile_offset")
LSTM_BWD_MUTANTS = ("cprev_t", "dc_wrong_gate", "drop_rec", "swap_w_cols",
                    "tile_offset")


def lstm_forward_f64(xproj, W, b):
    """Free-running f64 forward; gates on the bf16 grid, c in f32, h bf16:
    the saved tensors handed to the backward kernel, so that a forward
    defect can neither cause nor hide a backward failure."""
    T, B, H4 = xproj.shape
    H = H4 // 4
    h = np.zeros((B, H))
    c = np.zeros((B, H))
    W64 = W.astype(np.float64)
    gates, cs, hs = [], [], []
    for t in range(T):
        a = (xproj[t].astype(np.float64) + b + h @ W64).reshape(B, 4, H)
        gi, gf, go = (_sigmoid64(a[:, k]) for k in (0, 1, 3))
        gg = np.tanh(a[:, 2])
        c = gf * c + gi * gg
        h = go * np.tanh(c)
        gates.append(np.concatenate([gi, gf, gg, go], axis=1))
        cs.append(c)
        hs.append(h)
    return (bf16_round(np.stack(gates)), np.stack(cs).astype(np.float32),
            bf16_round(np.stack(hs)))


def lstm_fwd_ref(xproj, W, b, h_out, c_out):
    """Step references from the kernel's own h_out[t-1], c_out[t-1]."""
    T, B, H4 = xproj.shape
    H = H4 // 4
    res = Result()
    for t in range(T):
        hp = h_out[t - 1] if t else np.zeros((B, H), np.float32)
        cp = c_out[t - 1].astype(np.float64) if t else np.zeros((B, H))
        # one add of the bias and H fma steps, any order: H + 2 roundings
        pre = _preact(xproj[t].astype(np.float64), b.astype(np.float64),
                      hp, W, H + 2)
        g = [E(pre.v[:, k * H:(k + 1) * H], pre.e[:, k * H:(k + 1) * H])
             for k in range(4)]
        gi, gf, go = sig_e(g[0]), sig_e(g[1]), sig_e(g[3])
        gg = tanh_e(g[2])
        # c and h are formed from the unrounded gates: no bf16 term in c
        c = gf * cp + gi * gg
        h = go * tanh_e(c)
        trip = [x.stored_bf16() for x in (gi, gf, gg, go)]
        res.put("gates", t, tuple(np.concatenate([p[k] for p in trip],
                                                 axis=1)
                                  for k in range(3)), T)
        res.put("c", t, c.stored_f32(), T)
        res.put("h", t, h.stored_bf16(), T)
    return res


def lstm_fwd_emulate(xproj, W, b, mutant=None):
    T, B, H4 = xproj.shape
    H = H4 // 4
    W = W.copy()
    b = b.copy()
    if mutant == "drop_bias_o":
        b[3 * H:] = 0.0
    if mutant == "swap_w_rows":
        W[[3, 5]] = W[[5, 3]]
    order = (0, 2, 1, 3) if mutant == "gate_order" else (0, 1, 2, 3)
    h = np.zeros((B, H), np.float32)
    h_old = h
    c = np.zeros((B, H), np.float32)
    hs, cs, gs = [], [], []
    for t in range(T):
        x = xproj[t]
        if mutant == "tile_offset" and B > BM:
            x = np.concatenate([x[:BM], x[:B - BM]])
        a = _mm32(x + b, h_old if mutant == "stale_h" else h, W)
        a = a.reshape(B, 4, H)
        gi = _sig32(a[:, order[0]])
        gf = _sig32(a[:, order[1]])
        gg = _tanh32(a[:, order[2]])
        go = _sig32(a[:, order[3]])
        c = _f32(gf * c + gi * gg)
        h_old = h
        h = bf16_round(go * _tanh32(c))
        gs.append(bf16_round(np.concatenate([gi, gf, gg, go], axis=1)))
        cs.append(c)
        hs.append(h)
    return dict(h=np.stack(hs), c=np.stack(cs), gates=np.stack(gs))


def lstm_bwd_ref(dh_up, gates, c, W, dgates_out):
    """Step references. The recurrent term of step t is formed from the
    kernel's own dgates_out[t+1] (exactly the bf16 values its MFMA read
    from LDS): 4H products, 4H U24 (|dg| |W^T|). dc is carried here in
    f64 with its running bound; its gain is gf <= 1 and only f32-level
    terms enter it."""
    T, B, H = dh_up.shape
    W64 = W.astype(np.float64)
    dc = E(np.zeros((B, H)))
    res = Result()
    for t in range(T - 1, -1, -1):
        g = gates[t].astype(np.float64).reshape(B, 4, H)
        gi, gf, gg, go = (g[:, k] for k in range(4))
        cprev = c[t - 1].astype(np.float64) if t else np.zeros((B, H))
        if t < T - 1:
            dg = dgates_out[t + 1].astype(np.float64)
            rec = E(dg @ W64.T, 4 * H * U24 * (_abs(dg) @ _abs(W64.T)))
        else:
            rec = E(np.zeros((B, H)))
        tc = tanh_e(E(c[t]))
        dh = dh_up[t].astype(np.float64) + rec
        do_ = dh * tc
        dcv = dc + dh * go * (1.0 - tc * tc)
        dai = dcv * gg * gi * (1.0 - E(gi))
        daf = dcv * cprev * gf * (1.0 - E(gf))
        dag = dcv * gi * (1.0 - E(gg) * gg)
        dao = do_ * go * (1.0 - E(go))
        dc = dcv * gf
        trip = [x.stored_bf16() for x in (dai, daf, dag, dao)]
        res.put("dgates", t, tuple(np.concatenate([p[k] for p in trip],
                                                  axis=1)
                                   for k in range(3)), T)
    return res


def lstm_bwd_emulate(dh_up, gates, c, W, mutant=None):
    T, B, H = dh_up.shape
    W = W.copy()
    if mutant == "swap_w_cols":
        W[:, [3, 5]] = W[:, [5, 3]]
    dc = np.zeros((B, H), np.float32)
    dhrec = np.zeros((B, H), np.float32)
    out = np.zeros((T, B, 4 * H), np.float32)
    for t in range(T - 1, -1, -1):
        g = gates[t].reshape(B, 4, H)
        gi, gf, gg, go = (g[:, k] for k in range(4))
        cprev = c[t - 1] if t else np.zeros((B, H), np.float32)
        if mutant == "cprev_t":
            cprev = c[t]
        up = dh_up[t]
        if mutant == "tile_offset" and B > BM:
            up = np.concatenate([up[:BM], up[:B - BM]])
        tc = _tanh32(c[t])
        dh = _f32(up + dhrec)
        do_ = dh * tc
        dcv = _f32(dc + dh * go * (_ONE - tc * tc))
        di, df, dgg = dcv * gg, dcv * cprev, dcv * gi
        dc = _f32(dcv * (go if mutant == "dc_wrong_gate" else gf))
        dg = bf16_round(np.concatenate(
            [di * gi * (_ONE - gi), df * gf * (_ONE - gf),
             dgg * (_ONE - gg * gg), do_ * go * (_ONE - go)], axis=1))
        out[t] = dg
        dhrec = _mm32(np.zeros((B, H), np.float32), dg,
                      np.ascontiguousarray(W.T))
        if mutant == "drop_rec" and t == T - 1:
            dhrec[:, 5] = 0.0
    return out


# ===========================================================================
# GRU
# ===========================================================================
GRU_FWD_MUTANTS = ("drop_bias_n", "bias_n_outside", "gate_order",
                   "swap_w_rows", "stale_h", "tile_offset")
GRU_BWD_MUTANTS = ("dz_sign", "drop_direct", "n_cols_swapped", "dr_from_xn",
                   "hprev_t", "tile_offset")


def gru_forward_f64(xproj, W, b):
    """Free-running f64 forward: saved gates (bf16), hp_n (f32), h (bf16)
    for the backward kernel."""
    T, B, H3 = xproj.shape
    H = H3 // 3
    h = np.zeros((B, H))
    W64 = W.astype(np.float64)
    gates, hpns, hs = [], [], []
    for t in range(T):
        x = xproj[t].astype(np.float64).reshape(B, 3, H)
        hp = (b + h @ W64).reshape(B, 3, H)
        r = _sigmoid64(x[:, 0] + hp[:, 0])
        z = _sigmoid64(x[:, 1] + hp[:, 1])
        n = np.tanh(x[:, 2] + r * hp[:, 2])
        h = (1.0 - z) * n + z * h
        gates.append(np.concatenate([r, z, n], axis=1))
        hpns.append(hp[:, 2])
        hs.append(h)
    return (bf16_round(np.stack(gates)), np.stack(hpns).astype(np.float32),
            bf16_round(np.stack(hs)))


def gru_fwd_ref(xproj, W, b, h_out):
    """Step references from the kernel's own h_out[t-1]. One trap: the
    kernel blends with its unrounded f32 register h_prev, the reference
    only sees bf16(h_prev) = h_out[t-1], so |h_prev - h_out[t-1]| <=
    B8 |h_prev| <= B8 (1 + 2 B8) |h_out[t-1]| enters h[t] through z. It is
    fresh each step and does not accumulate."""
    T, B, H3 = xproj.shape
    H = H3 // 3
    res = Result()
    zero = np.zeros((B, H3))
    for t in range(T):
        hp_b = h_out[t - 1] if t else np.zeros((B, H), np.float32)
        # accumulator starts at the bias: H fma steps on top, H + 1
        hp = _preact(zero, b.astype(np.float64), hp_b, W, H + 1)
        x = xproj[t].astype(np.float64)
        s = [slice(k * H, (k + 1) * H) for k in range(3)]
        hpn = E(hp.v[:, s[2]], hp.e[:, s[2]])
        r = sig_e(x[:, s[0]] + E(hp.v[:, s[0]], hp.e[:, s[0]]))
        z = sig_e(x[:, s[1]] + E(hp.v[:, s[1]], hp.e[:, s[1]]))
        n = tanh_e(x[:, s[2]] + r * hpn)
        hprev = E(hp_b, 0.0, B8 * (1.0 + 2.0 * B8) * _abs(hp_b))
        h = (1.0 - z) * n + z * hprev
        trip = [v.stored_bf16() for v in (r, z, n)]
        res.put("gates", t, tuple(np.concatenate([p[k] for p in trip],
                                                 axis=1)
                                  for k in range(3)), T)
        res.put("hpn", t, hpn.stored_f32(), T)
        res.put("h", t, h.stored_bf16(), T)
    return res


def gru_fwd_emulate(xproj, W, b, mutant=None):
    T, B, H3 = xproj.shape
    H = H3 // 3
    W = W.copy()
    b = b.copy()
    if mutant == "drop_bias_n":
        b[2 * H:] = 0.0
    if mutant == "swap_w_rows":
        W[[3, 5]] = W[[5, 3]]
    bn = b[2 * H:]
    h32 = np.zeros((B, H), np.float32)      # the f32 register
    hb = np.zeros((B, H), np.float32)       # its bf16 copy in LDS
    hb_old = hb
    hs, gs, hpns = [], [], []
    for t in range(T):
        x = xproj[t]
        if mutant == "tile_offset" and B > BM:
            x = np.concatenate([x[:BM], x[:B - BM]])
        x = x.reshape(B, 3, H)
        acc = _mm32(np.broadcast_to(b, (B, H3)),
                    hb_old if mutant == "stale_h" else hb, W)
        acc = acc.reshape(B, 3, H)
        kr_, kz = (1, 0) if mutant == "gate_order" else (0, 1)
        gr = _sig32(_f32(x[:, kr_] + acc[:, kr_]))
        gz = _sig32(_f32(x[:, kz] + acc[:, kz]))
        hpn = acc[:, 2]
        if mutant == "bias_n_outside":      # b_hh_n not multiplied by r
            gn = _tanh32(_f32(x[:, 2] + gr * _f32(hpn - bn) + bn))
        else:
            gn = _tanh32(_f32(x[:, 2] + gr * hpn))
        h32 = _f32((_ONE - gz) * gn + gz * h32)
        hb_old = hb
        hb = bf16_round(h32)
        gs.append(bf16_round(np.concatenate([gr, gz, gn], axis=1)))
        hpns.append(hpn)
        hs.append(hb)
    return dict(h=np.stack(hs), hpn=np.stack(hpns), gates=np.stack(gs))


def gru_bwd_ref(dh_up, gates, hpn, h_out, W, dgates_out, anchored):
    """Step references for the x-side dgates (da_r, da_z, da_n).

    dh[t] = dh_up[t] + dh[t+1] z[t+1] + dg_h[t+1] @ W^T. The r and z
    columns of dg_h that the MFMA reads are the stored outputs; its n
    column bf16(da_n r) is not stored: it is formed here from dh[t+1] and
    carries its own error plus B8 |da_n r|. dh itself is loop-carried and
    never stored.
      chain mode     dh[t+1] is this reference's own value with its
                     running bound (grows geometrically: T <= 3).
      anchored mode  dh[t+1] is recovered from the kernel's stored
                     da_n[t+1] or da_z[t+1] divided by its f64
                     coefficient, whichever coefficient is larger per
                     element: the kernel's dh[t+1] to within the bf16
                     rounding of that store, B8 |dh[t+1]|, plus the f32
                     roundings of the coefficient (at most 8 U24). The
                     uncertainty enters step t once, through z and the n
                     column, and is discarded. Where both coefficients are
                     exactly zero the chain value is used.
    A defect in the carried dh still shows in anchored mode: step t is
    predicted with the correct recurrence from the recovered dh[t+1]."""
    T, B, H = dh_up.shape
    W64 = W.astype(np.float64)
    Wn = _abs(W64[:, 2 * H:].T)
    res = Result()
    dh_next = None
    for t in range(T - 1, -1, -1):
        g = gates[t].astype(np.float64).reshape(B, 3, H)
        gr, gz, gn = (g[:, k] for k in range(3))
        hprev = (h_out[t - 1].astype(np.float64) if t
                 else np.zeros((B, H)))
        if t < T - 1:
            g1 = gates[t + 1].astype(np.float64).reshape(B, 3, H)
            r1, z1, n1 = (g1[:, k] for k in range(3))
            d1 = dgates_out[t + 1].astype(np.float64)
            if anchored:
                cn = (1.0 - z1) * (1.0 - n1 * n1)
                cz = (h_out[t].astype(np.float64) - n1) * z1 * (1.0 - z1)
                use_n = _abs(cn) >= _abs(cz)
                coef = np.where(use_n, cn, cz)
                num = np.where(use_n, d1[:, 2 * H:], d1[:, H:2 * H])
                ok = coef != 0.0
                rec = num / np.where(ok, coef, 1.0)
                dh1 = E(np.where(ok, rec, dh_next.v),
                        np.where(ok, 8 * U24 * _abs(rec), dh_next.e),
                        np.where(ok, B8 * (1.0 + 2.0 * B8) * _abs(rec),
                                 dh_next.h))
            else:
                dh1 = dh_next
            nh = (dh1 * (1.0 - E(z1)) * (1.0 - E(n1) * n1) * r1
                  ).after_bf16()
            A = np.concatenate([d1[:, :2 * H], nh.v], axis=1)
            Ae = np.concatenate([np.zeros((B, 2 * H)), nh.e + nh.h], axis=1)
            gemm = E(A @ W64.T,
                     nh.e @ Wn + 3 * H * U24 * ((_abs(A) + Ae) @ _abs(W64.T)),
                     nh.h @ Wn)
            dhrec = dh1 * z1 + gemm
        else:
            dhrec = E(np.zeros((B, H)))
        dh = dh_up[t].astype(np.float64) + dhrec
        da_n = dh * (1.0 - E(gz)) * (1.0 - E(gn) * gn)
        da_r = da_n * hpn[t].astype(np.float64) * gr * (1.0 - E(gr))
        da_z = dh * (E(hprev) - gn) * gz * (1.0 - E(gz))
        dh_next = dh
        trip = [x.stored_bf16() for x in (da_r, da_z, da_n)]
        res.put("dgates", t, tuple(np.concatenate([p[k] for p in trip],
                                                  axis=1)
                                   for k in range(3)), T)
    return res


def gru_bwd_emulate(dh_up, gates, hpn, h_out, W, mutant=None, xproj=None):
    T, B, H = dh_up.shape
    dhrec = np.zeros((B, H), np.float32)
    out = np.zeros((T, B, 3 * H), np.float32)
    Wt = np.ascontiguousarray(W.T)
    for t in range(T - 1, -1, -1):
        g = gates[t].reshape(B, 3, H)
        gr, gz, gn = (g[:, k] for k in range(3))
        hprev = h_out[t - 1] if t else np.zeros((B, H), np.float32)
        if mutant == "hprev_t":
            hprev = h_out[t]
        up = dh_up[t]
        if mutant == "tile_offset" and B > BM:
            up = np.concatenate([up[:BM], up[:B - BM]])
        dh = _f32(up + dhrec)
        dz = dh * ((gn - hprev) if mutant == "dz_sign" else (hprev - gn))
        da_n = _f32(dh * (_ONE - gz) * (_ONE - gn * gn))
        src = (xproj[t][:, 2 * H:] if mutant == "dr_from_xn" else hpn[t])
        da_r = _f32(da_n * src * gr * (_ONE - gr))
        da_z = _f32(dz * gz * (_ONE - gz))
        nx, nh = da_n, _f32(da_n * gr)
        if mutant == "n_cols_swapped":
            nx, nh = nh, nx
        out[t] = bf16_round(np.concatenate([da_r, da_z, nx], axis=1))
        dgh = bf16_round(np.concatenate([da_r, da_z, nh], axis=1))
        direct = dh * gz
        if mutant == "drop_direct" and t == T - 1:
            direct = np.zeros_like(direct)
        dhrec = _f32(direct + _mm32(np.zeros((B, H), np.float32), dgh, Wt))
    return out


# ===========================================================================
# Torch side of the autograd functions: dW_hh and db_hh from the kernel's
# own h_out and dgates (tests call these with what the kernel returned)
# ===========================================================================

def weight_grad_ref(h_out, dg):
    """dW_hh = h_prev^T @ dg over T B rows, f32 accumulation in any order,
    returned by the GEMM as bf16: B8 |value| + T B U24 (|h_prev|^T |dg|).
    db_hh = column sums in f32, any order: T B U24 sum|dg|."""
    T, B, H = h_out.shape
    hp = np.concatenate([np.zeros((1, B, H)), h_out[:-1].astype(np.float64)])
    hp = hp.reshape(T * B, H)
    dg = dg.astype(np.float64).reshape(T * B, -1)
    n = T * B
    dw = E(hp.T @ dg, n * U24 * (_abs(hp).T @ _abs(dg)))
    db = E(dg.sum(axis=0), n * U24 * _abs(dg).sum(axis=0))
    return dw.stored_bf16(), db.stored_f32()


def gru_h_side(dgates_x, gates, H):
    """dg_h as models/gru.py forms it: the n column is
    bf16(bf16(da_n) * bf16(r)), the rest is the x side."""
    out = np.array(dgates_x, dtype=np.float32)
    out[..., 2 * H:] = bf16_round(out[..., 2 * H:] * gates[..., :H])
    return out
