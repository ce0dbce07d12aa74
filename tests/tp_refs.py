"""References and directed inputs for the two phases of the continuous
backtest, ops/hip/backtest_tp.hip (a helper module, no tests of its own;
test_tp_refs_cpu.py and test_gpu_tp_phases.py use it).

  pack_flags / unpack_flags   the kernels' flag-word layout
  cpu_flags                   phase 1 by the CPU engine
  trades_ref                  phase 2: a numpy position machine written from
                              backtesting/strategy.py sections 3-4, with a
                              census of which branches the inputs reached and
                              deliberate deviations (`variant`) that show the
                              inputs tell a wrong machine from the right one
  directed_case, affine_case  scripted candles and flag planes that reach
                              every branch and equality edge of the machine
"""

import numpy as np

from ai_crypto_trader_amd.backtesting.engine_cpu import (
    finalize_metrics, run_backtest_cpu,
)
from ai_crypto_trader_amd.backtesting.strategy import FEE, random_population

f32 = np.float32

VARIANTS = ("sl_strict", "tp_strict", "arm_strict", "tp_over_sl",
            "reenter_same_candle", "trail_ignores_zero", "fill_at_low")

LANES_PER_BLOCK = 256       # strategies per bt_trades_kernel block
LANES_PER_WAVE = 64
HALF = 32                   # candles per equity hand-off (half a flag word)


# ---------------------------------------------------------------------
# flag words: (nsym, nwords, P) int64, bit t & 63 of word t >> 6
# ---------------------------------------------------------------------
def pack_flags(flags):
    """(P, nsym, T) bool -> (nsym, nwords, P) int64, padding bits zero."""
    flags = np.asarray(flags, bool)
    P, nsym, T = flags.shape
    nwords = (T + 63) // 64
    bits = np.zeros((P, nsym, nwords * 64), bool)
    bits[:, :, :T] = flags
    by = np.packbits(bits.reshape(P, nsym, nwords, 64), axis=-1,
                     bitorder="little")                 # (P, nsym, nwords, 8)
    words = np.ascontiguousarray(by).view("<u8")[..., 0]
    return np.ascontiguousarray(words.transpose(1, 2, 0)).view(np.int64)


def unpack_flags(words, T):
    """(nsym, nwords, P) int64 -> ((P, nsym, T) bool, the bits at t >= T of
    the last word as (P, nsym, nwords * 64 - T) bool)."""
    words = np.ascontiguousarray(words).view(np.uint64)
    nsym, nwords, P = words.shape
    assert nwords == (T + 63) // 64
    by = words.astype("<u8").view(np.uint8).reshape(nsym, nwords, P, 8)
    bits = np.unpackbits(by, axis=-1, bitorder="little")
    bits = bits.transpose(2, 0, 1, 3).reshape(P, nsym, nwords * 64)
    return bits[:, :, :T].astype(bool), bits[:, :, T:].astype(bool)


def cpu_flags(candles, pop):
    """Phase 1 by the CPU engine: (entry plane, exit plane, metrics); the
    planes are (P, nsym, T) bool."""
    metrics, nets = run_backtest_cpu(candles, pop, record_net=True)
    entry_v = pop[:, 10].astype(np.int32)[:, None, None]
    exit_v = pop[:, 11].astype(np.int32)[:, None, None]
    return nets >= entry_v, nets <= -exit_v, metrics


# ---------------------------------------------------------------------
# phase 2 reference
# ---------------------------------------------------------------------
def trades_ref(candles, pop, eflags, xflags, initial_equity=1.0,
               variant=None, watch=()):
    """The position machine of strategy.py sections 3-4 over given flag
    planes, every lane at once; lane = (strategy, symbol), symbol fastest.

    Returns (metrics (P, nsym, NMETRIC) f32, census). census holds counts
    over all lanes and candles:
      exit_stop, exit_trailed, exit_tp, exit_signal   exits by reason (a
                          stop is `trailed` once it stands above the
                          entry's own stop)
      both_hit            candles in position with low <= stop and
                          high >= tp
      exit_on_entry_bit   exits on a candle whose entry bit is set
      entry_ignored       entry bits on a candle that began in position
      exit_ignored        exit bits on a candle that began flat
      trail_off_at_arm    candles in position at or past the trailing arm
                          with trailing_stop_pct == 0
      open_at_T           lanes still in position after the last candle
    and
      in_pos_at[t], armed_at[t]   for t in `watch`: lanes in position after
                          candle t, and those of them whose stop trails
      skip, wave_entered  (nsym, blocks of 256 strategies, 4 waves of 64,
                          half-words of 32 candles) bool: all of the wave's
                          lanes flat when the half-word starts and no entry
                          bit inside it (bt_trades_kernel's skip condition),
                          and whether a lane of the wave entered inside it

    `variant` is one of VARIANTS: a machine that is wrong in that one way.
    """
    assert variant is None or variant in VARIANTS, variant
    candles = np.asarray(candles, f32)
    pop = np.asarray(pop, f32)
    nsym, T, _ = candles.shape
    P = pop.shape[0]
    L = P * nsym
    ebits = np.asarray(eflags, bool).reshape(L, T)
    xbits = np.asarray(xflags, bool).reshape(L, T)
    sym = np.tile(np.arange(nsym), P)
    par = np.repeat(pop, nsym, axis=0)
    size = par[:, 12]
    keep = f32(1.0) - f32(FEE)
    sl_mul = f32(1.0) - par[:, 13]
    tp_mul = f32(1.0) + par[:, 14]
    trail_mul = f32(1.0) - par[:, 15]
    arm_mul = f32(1.0) + par[:, 16]
    trails = par[:, 15] > 0
    if variant == "trail_ignores_zero":
        trails = np.ones(L, bool)

    init = f32(initial_equity)
    cash = np.full(L, init, f32)
    units = np.zeros(L, f32)
    held = np.zeros(L, bool)
    paid = np.zeros(L, f32)
    stop = np.zeros(L, f32)
    stop0 = np.zeros(L, f32)        # the stop as the entry set it
    target = np.zeros(L, f32)
    arm = np.zeros(L, f32)
    peak = np.zeros(L, f32)
    equity = np.full(L, init, f32)
    top = np.full(L, init, f32)
    max_dd = np.zeros(L, f32)
    n_trades = np.zeros(L, f32)
    wins = np.zeros(L, f32)
    gross_p = np.zeros(L, f32)
    gross_l = np.zeros(L, f32)
    sum_ret = np.zeros(L, f32)
    sum_ret2 = np.zeros(L, f32)

    names = ("exit_stop", "exit_trailed", "exit_tp", "exit_signal",
             "both_hit", "exit_on_entry_bit", "entry_ignored",
             "exit_ignored", "trail_off_at_arm", "open_at_T")
    census = dict.fromkeys(names, 0)
    census["in_pos_at"] = {}
    census["armed_at"] = {}
    nhalf = (T + HALF - 1) // HALF
    held_at_half = np.zeros((nhalf, L), bool)
    entered_in_half = np.zeros((nhalf, L), bool)

    def count(name, mask):
        census[name] += int(np.count_nonzero(mask))

    for t in range(T):
        close = candles[sym, t, 0]
        high = candles[sym, t, 1]
        low = candles[sym, t, 2]
        eb, xb = ebits[:, t], xbits[:, t]
        was = held.copy()
        if t % HALF == 0:
            held_at_half[t // HALF] = was
        count("entry_ignored", was & eb)
        count("exit_ignored", ~was & xb)

        # section 3, in position: peak, trailing stop, the three exits
        peak[was] = np.maximum(peak, high)[was]
        reached = (peak > arm) if variant == "arm_strict" else (peak >= arm)
        count("trail_off_at_arm", was & (peak >= arm) & (par[:, 15] == 0))
        trailing = was & trails & reached
        stop[trailing] = np.maximum(stop, peak * trail_mul)[trailing]

        below = (low < stop) if variant == "sl_strict" else (low <= stop)
        above = (high > target) if variant == "tp_strict" \
            else (high >= target)
        count("both_hit", was & below & above)
        if variant == "tp_over_sl":
            by_tp = was & above
            by_stop = was & ~by_tp & below
        else:
            by_stop = was & below
            by_tp = was & ~by_stop & above
        by_signal = was & ~by_stop & ~by_tp & xb
        leaving = by_stop | by_tp | by_signal
        fill = np.where(by_stop, stop, np.where(by_tp, target, close))
        if variant == "fill_at_low":
            fill = np.where(by_stop, low, np.where(by_tp, high, close))
        count("exit_stop", by_stop & ~(stop > stop0))
        count("exit_trailed", by_stop & (stop > stop0))
        count("exit_tp", by_tp)
        count("exit_signal", by_signal)
        count("exit_on_entry_bit", leaving & eb)

        proceeds = units * fill * keep
        pnl = proceeds - paid
        cash[leaving] = (cash + proceeds)[leaving]
        n_trades[leaving] += f32(1.0)
        wins[leaving & (pnl > 0)] += f32(1.0)
        gross_p[leaving] += np.maximum(pnl, f32(0.0))[leaving]
        gross_l[leaving] += np.maximum(-pnl, f32(0.0))[leaving]
        units[leaving] = f32(0.0)
        held = was & ~leaving

        # section 3, flat: enter at the close. A lane that left on this
        # candle began it in position, so it waits for the next one.
        flat = ~held if variant == "reenter_same_candle" else ~was
        entering = flat & eb
        cost = np.minimum(size * equity, cash)
        units[entering] = (cost * keep / close)[entering]
        cash[entering] = (cash - cost)[entering]
        paid[entering] = cost[entering]
        stop[entering] = (close * sl_mul)[entering]
        stop0[entering] = stop[entering]
        target[entering] = (close * tp_mul)[entering]
        arm[entering] = (close * arm_mul)[entering]
        peak[entering] = close[entering]
        held = held | entering
        entered_in_half[t // HALF] |= entering

        # section 4: mark to market
        value = cash + units * close
        r = value / equity - f32(1.0)
        sum_ret += r
        sum_ret2 += r * r
        equity = value
        top = np.maximum(top, equity)
        max_dd = np.maximum(max_dd, (top - equity) / top)

        if t in watch:
            census["in_pos_at"][t] = int(np.count_nonzero(held))
            census["armed_at"][t] = int(np.count_nonzero(
                held & trails & (peak >= arm)))

    census["open_at_T"] = int(np.count_nonzero(held))

    # the kernel's view: block = (symbol, 256 strategies), wave = 64 of
    # them; lanes past P hold no position and no bits
    nblk = (P + LANES_PER_BLOCK - 1) // LANES_PER_BLOCK
    ent_bit = np.zeros((nhalf, L), bool)
    for h in range(nhalf):
        ent_bit[h] = ebits[:, h * HALF:(h + 1) * HALF].any(axis=1)

    def per_wave(a):
        full = np.zeros((nhalf, nblk * LANES_PER_BLOCK, nsym), bool)
        full[:, :P] = a.reshape(nhalf, P, nsym)
        full = full.reshape(nhalf, nblk, 4, LANES_PER_WAVE, nsym)
        return full.any(axis=3).transpose(3, 1, 2, 0)

    census["skip"] = ~per_wave(held_at_half | ent_bit)
    census["wave_entered"] = per_wave(entered_in_half)

    metrics = finalize_metrics(
        T, equity, n_trades, wins, gross_p, gross_l, max_dd, sum_ret,
        sum_ret2).reshape(P, nsym, -1)
    return metrics, census


# ---------------------------------------------------------------------
# directed inputs
# ---------------------------------------------------------------------
# Scripted lanes enter at close 1.0 with stop_loss 1/8, take_profit 1/4,
# trailing arm 1/16 and trailing distance 1/16 (0 on every fourth lane),
# all exact in f32: stop 0.875, take-profit 1.25, arm 1.0625.
STOP, TP, ARM = f32(0.875), f32(1.25), f32(1.0625)
UP, DOWN = f32(np.inf), f32(-np.inf)

# (candle offset, (close, high, low), entry bit, exit bit). A candle that is
# not listed is quiet: (1, 1, 1) with no bits. Every episode ends flat: its
# last candle closes at 1.0 with the exit bit set.
_Q = (1.0, 1.0, 1.0)
_OPENING = [
    # entry at t = 0; stop and take-profit both hit, far through both
    (0, _Q, 1, 0), (1, (1.0, 1.3, 0.8), 0, 0), (2, _Q, 0, 1),
    # a gap through the take-profit. With a trailing stop the same candle
    # arms it (peak 1.5 -> stop 1.40625) and fills it (low 1.0).
    (4, _Q, 1, 0), (5, (1.4, 1.5, 1.0), 0, 0), (6, _Q, 0, 1),
    # low == stop
    (8, _Q, 1, 0), (9, (1.0, 1.0, STOP), 0, 0), (10, _Q, 0, 1),
    # low one ulp above the stop: holds, then leaves on the signal
    (12, _Q, 1, 0), (13, (1.0, 1.0, np.nextafter(STOP, UP)), 0, 0),
    (14, _Q, 0, 1),
    # high == take-profit (a trailing stop rises to 1.171875 < low)
    (16, _Q, 1, 0), (17, (1.2, TP, 1.2), 0, 0), (18, _Q, 0, 1),
    # high one ulp below the take-profit
    (20, _Q, 1, 0), (21, (1.2, np.nextafter(TP, DOWN), 1.2), 0, 0),
    (22, _Q, 0, 1),
    # peak == arm: the stop rises to 0.99609375 and the next low fills it
    (24, _Q, 1, 0), (25, (1.05, ARM, 1.05), 0, 0),
    (26, (0.99, 1.0, 0.99), 0, 0), (27, _Q, 0, 1),
    # peak one ulp below the arm: the same low fills nothing
    (28, _Q, 1, 0), (29, (1.05, np.nextafter(ARM, DOWN), 1.05), 0, 0),
    (30, (0.99, 1.0, 0.99), 0, 0), (31, _Q, 0, 1),
    # a stop that ratchets three times, rests a candle, then fills
    (32, _Q, 1, 0), (33, (1.1, 1.1, 1.05), 0, 0),
    (34, (1.15, 1.15, 1.1), 0, 0), (35, (1.2, 1.2, 1.15), 0, 0),
    (36, (1.15, 1.2, 1.13), 0, 0), (37, (1.1, 1.15, 1.1), 0, 0),
    (38, (1.0, 1.1, 1.0), 0, 1),
    # an entry bit on the exit candle and on the next: the lane enters on
    # the next. Re-entering on the exit candle would meet candle 42's low.
    (40, _Q, 1, 0), (41, (1.0, 1.0, 0.8), 1, 0),
    (42, (1.0, 1.0, 0.8), 1, 0), (43, _Q, 0, 1),
    (44, _Q, 0, 1),
]
OPENING_LEN = 48


def _crossing(b):
    """A position entered at b - 6, its stop trailing from b - 5 on, held
    across candle b - 1 / b, ratcheted again at b + 1 and filled at b + 3
    (offsets from b - 12; the first two candles clear the lane)."""
    held = (1.08, 1.08, 1.05)
    ev = [(0, _Q, 0, 1), (1, _Q, 0, 1), (6, _Q, 1, 0),
          (7, held, 0, 0), (8, (1.1, 1.1, 1.05), 0, 0)]
    ev += [(k, held, 0, 0) for k in range(9, 13)]
    ev += [(13, (1.15, 1.15, 1.1), 0, 0), (14, (1.12, 1.12, 1.1), 0, 0),
           (15, (1.05, 1.1, 1.05), 0, 0), (16, (1.0, 1.05, 1.0), 0, 1),
           (17, _Q, 0, 1)]
    return b - 12, 20, ev


def _closing(T):
    """Entry on the last candle (the first two candles clear the lane)."""
    return T - 6, 6, [(0, _Q, 0, 1), (1, _Q, 0, 1), (5, _Q, 1, 0)]


def _windows(T):
    out = [(0, OPENING_LEN, _OPENING)]
    b = 256
    while b + 8 <= T - 6:
        out.append(_crossing(b))
        b += 256
    out.append(_closing(T))
    return out


def _case(T, nsym, P, groups, seed):
    """groups: name -> slice of strategies. `script` lanes follow the script
    on symbol 0; elsewhere, and on every other lane, planes are random at
    20 % unless the group says otherwise."""
    from ledger_cases import market

    rng = np.random.default_rng(seed)
    candles = market(T, nsym, seed=seed + 1).copy()
    pop = random_population(P, seed=seed + 2)
    eflags = rng.random((P, nsym, T)) < 0.2
    xflags = rng.random((P, nsym, T)) < 0.2

    sc = groups["script"]
    n_sc = sc.stop - sc.start
    k = np.arange(n_sc)
    pop[sc, 12] = np.where(k % 8 < 4, 0.5, 1.0)
    pop[sc, 13] = 0.125
    pop[sc, 14] = 0.25
    pop[sc, 15] = np.where(k % 4 == 3, 0.0, 0.0625)
    pop[sc, 16] = 0.0625
    for t0, n, events in _windows(T):
        candles[0, t0:t0 + n, :3] = 1.0
        eflags[sc, 0, t0:t0 + n] = False
        xflags[sc, 0, t0:t0 + n] = False
        for dt, (c, h, lo), eb, xb in events:
            candles[0, t0 + dt, :3] = (c, h, lo)
            eflags[sc, 0, t0 + dt] = bool(eb)
            xflags[sc, 0, t0 + dt] = bool(xb)

    pop[groups["all_in"], 12] = 1.0
    eflags[groups["ones"]] = True
    xflags[groups["ones"]] = True
    sparse = groups["sparse"]
    eflags[sparse] = rng.random(eflags[sparse].shape) < 0.02
    xflags[sparse] = rng.random(xflags[sparse].shape) < 0.02
    eflags[groups["never"]] = False
    if "late" in groups:
        # no entry bit up to candle 320; all of them enter at 321
        eflags[groups["late"], :, :321] = False
        eflags[groups["late"], :, 321] = True
    if "bursts" in groups:
        # two short bursts of entries under all-ones exit planes: the wave
        # trades, is flat and settled again, and is skipped again
        b = groups["bursts"]
        burst = np.zeros(eflags[b].shape, bool)
        for t0 in (40, 400):
            burst[:, :, t0:t0 + 4] = rng.random(burst[:, :, :4].shape) < 0.5
        eflags[b] = burst
        xflags[b] = True
    return (np.ascontiguousarray(candles, f32), pop.astype(f32),
            eflags, xflags)


DIRECTED_EQUITY = 250.0


def directed_case():
    """T = 700 (two 256-tiles plus 188; 21 half-words plus 28 candles),
    3 symbols, 300 strategies (a 256-chunk plus 44): (candles, pop, eflags,
    xflags, initial_equity). Symbol 0 is scripted, symbols 1-2 are
    ledger_cases.market at sigma = 2."""
    groups = {
        "script": slice(0, 32), "ones": slice(32, 48),
        "sparse": slice(48, 64),
        "never": slice(64, 128),        # a whole wave that never enters
        "late": slice(128, 192),        # a wave flat until candle 321
        "bursts": slice(192, 256),
        "all_in": slice(256, 270),      # second chunk: 20 % planes
    }
    return (*_case(700, 3, 300, groups, seed=4100), DIRECTED_EQUITY)


def affine_case():
    """The same script at T = 300, 8 symbols, 40 strategies: the shape of
    bt_block_map's XCD-affine branch."""
    groups = {
        "script": slice(0, 16), "ones": slice(16, 20),
        "never": slice(20, 24), "sparse": slice(32, 40),
        "all_in": slice(24, 28),
    }
    return (*_case(300, 8, 40, groups, seed=4200), DIRECTED_EQUITY)
