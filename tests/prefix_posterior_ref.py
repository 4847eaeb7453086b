"""float64 oracles of the per-token posteriors (csrc/prefix_posterior.hip) and brute-force enumerations to check them against.

Psi_i = log P(the output starts with y1 .. yi | x); factors log c_i = Psi_i - Psi_{i-1}, log c_end = total - Psi_U."""
import itertools

import numpy as np


def ctc_prefix_oracle(x, L, y, blank):
    """x: (>= L, V) float64 log-probs.  Returns (psi [U], total): psi[i] = Psi_{i+1}, total = log P(y | x)."""
    U = len(y)
    S = 2 * U + 1
    if L == 0:
        return np.full(U, -np.inf), (0.0 if U == 0 else -np.inf)
    lab = np.array([blank if s % 2 == 0 else y[s // 2] for s in range(S)])
    allow2 = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        allow2[s] = lab[s] != lab[s - 2]
    a = np.full(S, -np.inf)
    a[0] = x[0, blank]
    psi = np.full(U, -np.inf)
    if S > 1:
        a[1] = x[0, lab[1]]
        psi[0] = a[1]
    for t in range(1, L):
        c1 = np.concatenate([[-np.inf], a])[:S]
        c2 = np.concatenate([[-np.inf, -np.inf], a])[:S]
        c2[~allow2] = -np.inf
        enter = np.logaddexp(c1, c2) + x[t, lab]  # the mass that moves INTO each state at frame t
        psi = np.logaddexp(psi, enter[1::2])
        a = np.logaddexp(a + x[t, lab], enter)
    total = np.logaddexp(a[S - 1], a[S - 2] if S > 1 else -np.inf)
    return psi, float(total)


def rnnt_prefix_oracle(lpb, lpy, Tb, Ub):
    """lpb / lpy: (>= Tb, >= Ub + 1) float64 (ea_rnnt_scan's meaning).  Returns (psi [Ub], total)."""
    if Tb <= 0:
        return np.full(Ub, -np.inf), -np.inf
    alpha = np.full((Tb, Ub + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                continue
            a = alpha[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
            c = alpha[t, u - 1] + lpy[t, u - 1] if u > 0 else -np.inf
            alpha[t, u] = np.logaddexp(a, c)
    psi = np.array([np.logaddexp.reduce(alpha[:, u] + lpy[:Tb, u]) for u in range(Ub)]).reshape(Ub)
    return psi, float(alpha[Tb - 1, Ub] + lpb[Tb - 1, Ub])


def factors(psi, total):
    """(logc [U + 1], total): the factors with the kernels' conventions — clamped to <= 0, -inf (never NaN) from the first
    Psi = -inf on."""
    chain = np.concatenate([[0.0], np.asarray(psi, dtype=np.float64), [total]])
    out = np.empty(len(chain) - 1)
    for i in range(1, len(chain)):
        out[i - 1] = -np.inf if chain[i] == -np.inf else min(chain[i] - chain[i - 1], 0.0)
    return out, total


# ------------------------------------------------------------------------------------------------ brute force
def ctc_collapse(path, blank):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(p)
        prev = p
    return tuple(out)


def ctc_brute_sequences(x, L, blank):
    """{label sequence: probability} by enumeration of all V**L frame labellings (linear domain)."""
    V = x.shape[1]
    probs = {}
    for path in itertools.product(range(V), repeat=L):
        p = float(np.exp(sum(x[t, k] for t, k in enumerate(path))))
        y = ctc_collapse(path, blank)
        probs[y] = probs.get(y, 0.0) + p
    return probs


def prefix_mass(probs, prefix):
    n = len(prefix)
    return sum(p for y, p in probs.items() if y[:n] == tuple(prefix))


def rnnt_lattice_of(logp_fn, T, y, blank):
    """(lpb, lpy) float64 [T][U + 1] of label sequence y under a prefix-dependent model logp_fn(t, prefix) -> log-probs [V]."""
    U = len(y)
    lpb, lpy = np.full((T, U + 1), -np.inf), np.full((T, U + 1), -np.inf)
    for t in range(T):
        for u in range(U + 1):
            row = logp_fn(t, tuple(y[:u]))
            lpb[t, u] = row[blank]
            if u < U:
                lpy[t, u] = row[y[u]]
    return lpb, lpy


def rnnt_brute_sequence(logp_fn, T, y, blank):
    """P(y) (linear) by enumeration of every alignment: the positions of the U emits among the T - 1 + U moves before the
    final blank."""
    U = len(y)
    lpb, lpy = rnnt_lattice_of(logp_fn, T, y, blank)
    n = T - 1 + U
    tot = 0.0
    for pos in itertools.combinations(range(n), U):
        ps = set(pos)
        t = u = 0
        sc = 0.0
        for i in range(n):
            if i in ps:
                sc += lpy[t, u]
                u += 1
            else:
                sc += lpb[t, u]
                t += 1
        tot += float(np.exp(sc + lpb[T - 1, U]))
    return tot
