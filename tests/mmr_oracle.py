"""MMR selection (include/mvdb.h "MMR SEARCH") restated in float64, and the adjudicator of a device pick sequence.

Given the candidates of one query — rel[F] (fp32 search scores, best first) and their stored rows [F, d] — step 0 picks
position 0 and step t >= 1 the unpicked position that maximises lambda * rel[j] - (1 - lambda) * max_p s(p, j), s the inner
product of two stored rows, ties to the lower position, a NaN objective ranking as -inf.

The adjudicator does not ask the device for the float64 sequence: two fp32 summation orders may rank a near-tie either
way, and one such swap changes every later step.  It follows the DEVICE's prefix instead: at every step t >= 1 it recomputes
the objective in float64 from the picks the device made before t and requires

    max_j obj64[j] - obj64[pick_t] <= tau,        tau = (d + 4) * 2^-23 * max(1, B^2),

B the largest norm among the candidate rows: an fp32 dot product of d terms in any order is within d * 2^-24 * |x| |y| of the
true value, the objective adds three roundings (two products, one difference) and 1 - lambda one more on the similarity
term, and two candidates are compared.  Wherever the float64 margin exceeds tau the pick is forced to be the float64 argmax.
"""
import numpy as np

NEG = -np.inf


def _sims(rows64, p):
    """float64 inner products of row p with every row (inf * 0 and inf - inf give NaN, as on the device)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return rows64 @ rows64[p]


def _objective(lam, rel64, maxsim):
    lam = float(np.float32(lam))            # the device takes lambda as fp32
    with np.errstate(invalid="ignore", over="ignore"):
        obj = lam * rel64 - (1.0 - lam) * maxsim
    return np.where(np.isnan(obj), NEG, obj)


def _fold(maxsim, s):
    """max with a sticky NaN: a NaN similarity makes the objective NaN (= -inf) from then on."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s) | np.isnan(maxsim), np.nan, np.maximum(maxsim, s))


def select(rel, rows, k, lam, dtype=np.float64):
    """The pick sequence (positions) for candidates rel[F] / rows[F, d]; every position is valid.  dtype=np.float32 runs the
    same loop in numpy fp32 (one more summation order, for comparison)."""
    rel = np.asarray(rel)
    F = rel.shape[0]
    if F == 0:
        return []
    x = np.asarray(rows).astype(dtype)
    r = rel.astype(dtype)
    lam_t = dtype(np.float32(lam))
    mu_t = dtype(1) - lam_t
    picks, picked = [0], np.zeros(F, bool)
    picked[0] = True
    maxsim = np.full(F, NEG, dtype)
    for _ in range(1, min(int(k), F)):
        with np.errstate(invalid="ignore", over="ignore"):
            s = x @ x[picks[-1]]
            maxsim = np.where(np.isnan(s) | np.isnan(maxsim), dtype(np.nan), np.maximum(maxsim, s))
            obj = lam_t * r - mu_t * maxsim
        obj = np.where(np.isnan(obj), dtype(NEG), obj)
        obj[picked] = NEG
        best = obj.max()
        j = int(np.flatnonzero((obj == best) & ~picked)[0])   # ties (and an all -inf remainder): the lower position
        picks.append(j)
        picked[j] = True
    return picks


def tau(rows):
    rows64 = np.asarray(rows, np.float64)
    norms = np.sqrt((rows64 * rows64).sum(axis=1))
    norms = norms[np.isfinite(norms)]
    B = float(norms.max()) if norms.size else 1.0
    return (rows64.shape[1] + 4) * 2.0 ** -23 * max(1.0, B * B)


def adjudicate(rel, rows, picks, k, lam):
    """(ok, message, worst deficit) for a device pick sequence over the candidates rel[F] / rows[F, d] (every position
    valid): min(k, F) distinct positions, position 0 first, and every later pick within tau of the float64 best given the
    device's own earlier picks."""
    rel64 = np.asarray(rel, np.float64)
    rows64 = np.asarray(rows, np.float64)
    F = rel64.shape[0]
    picks = [int(p) for p in picks]
    if len(picks) != min(int(k), F):
        return False, f"{len(picks)} picks for k = {k}, {F} candidates", np.inf
    if not picks:
        return True, "", 0.0
    if picks[0] != 0:
        return False, f"step 0 picked position {picks[0]}", np.inf
    if len(set(picks)) != len(picks) or min(picks) < 0 or max(picks) >= F:
        return False, f"picks are not distinct positions in [0, {F}): {picks}", np.inf
    t_ = tau(rows)
    worst = 0.0
    maxsim = np.full(F, NEG)
    picked = np.zeros(F, bool)
    picked[0] = True
    for t in range(1, len(picks)):
        maxsim = _fold(maxsim, _sims(rows64, picks[t - 1]))
        obj = _objective(lam, rel64, maxsim)
        obj[picked] = NEG
        best, got = obj.max(), obj[picks[t]]
        if np.isfinite(best) and np.isfinite(got):
            deficit = float(best - got)
        else:
            deficit = 0.0 if got == best else np.inf   # an infinite best must be matched exactly
        worst = max(worst, deficit)
        if deficit > t_:
            return False, (f"step {t}: picked position {picks[t]} with objective {got!r}, position {int(obj.argmax())} has "
                           f"{best!r}: deficit {deficit:.3e} > tau {t_:.3e}"), worst
        picked[picks[t]] = True
    return True, "", worst


def objective_trace(rel, rows, picks, lam):
    """obj64 of every pick t >= 1 given the prefix before it (NaN already mapped to -inf)."""
    rel64 = np.asarray(rel, np.float64)
    rows64 = np.asarray(rows, np.float64)
    maxsim = np.full(rel64.shape[0], NEG)
    out = []
    for t in range(1, len(picks)):
        maxsim = _fold(maxsim, _sims(rows64, int(picks[t - 1])))
        out.append(float(_objective(lam, rel64, maxsim)[int(picks[t])]))
    return out
