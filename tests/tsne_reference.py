"""Brute-force dense longdouble evaluation of the t-SNE definitions of include/insider_hip.h: the reference of
tests/test_tsne_cpu.py and tests/test_gpu_tsne.py.  Nothing here is shared with posthoc.tsne_host(): P is a dense N x N matrix
and every sum runs over all pairs."""
import numpy as np

LD = np.longdouble


def entropy_ld(idx, d2, beta):
    """Per row at the given beta, in longdouble: H(beta), the conditionals p (N x k, 0 at open slots) and the moment sum
    1 + E[beta d] + E[(beta d)^2] under p (rows without a filled slot: H = NaN, moment 1)."""
    N, k = idx.shape
    H, mom = np.full(N, np.nan, dtype=LD), np.ones(N, dtype=LD)
    p = np.zeros((N, k), dtype=LD)
    for i in range(N):
        m = int((idx[i] >= 0).sum())
        if m == 0 or not np.isfinite(beta[i]):
            continue
        d = d2[i, :m].astype(LD)
        bd = LD(beta[i]) * (d - d.min())
        e = np.exp(-bd)
        S = e.sum()
        p[i, :m] = e / S
        H[i] = np.log(S) + (bd * e).sum() / S
        mom[i] = 1 + (bd * p[i, :m]).sum() + (bd * bd * p[i, :m]).sum()
    return H, p, mom


def dense_p(idx, p_cond, alive):
    """The N x N joint P in longdouble from the conditionals (N x k)."""
    N = idx.shape[0]
    Pc = np.zeros((N, N), dtype=LD)
    for i in range(N):
        for s in range(idx.shape[1]):
            if idx[i, s] >= 0:
                Pc[i, idx[i, s]] = LD(p_cond[i, s])
    return (Pc + Pc.T) / (2 * LD(int(alive.sum())))


def dense_eval(idx, p_cond, Y, alive, a=1.0):
    """Z, KL and the gradient (under exaggeration a; NaN rows for dead points) at the map Y (N x 2) in longdouble, and what the
    bounds are made of: kl_abs (sum |KL terms|), kl_terms (their number), p_sum, and per component the sums of the absolute
    attractive terms (attr_abs, under a), of |w^2 delta| (rep_abs), the repulsive sums (rep) and the attractive terms per row."""
    N = idx.shape[0]
    P = dense_p(idx, p_cond, alive)
    Yl = Y.astype(LD)
    dlt = Yl[:, None, :] - Yl[None, :, :]
    w = 1 / (1 + (dlt * dlt).sum(axis=2))
    pair = alive[:, None] & alive[None, :] & ~np.eye(N, dtype=bool)
    w = np.where(pair, w, LD(0))
    z = w.sum()
    attr = ((P * w)[:, :, None] * dlt).sum(axis=1)
    rep = ((w * w)[:, :, None] * dlt).sum(axis=1)
    grad = 4 * (LD(a) * attr - rep / z)
    grad[~alive] = np.nan
    pos = P > 0
    terms = P[pos] * np.log(P[pos] * z / w[pos])
    return dict(z=z, kl=terms.sum(), grad=grad, kl_abs=np.abs(terms).sum(), kl_terms=int(pos.sum()), p_sum=P.sum(),
                attr_abs=LD(a) * ((P * w)[:, :, None] * np.abs(dlt)).sum(axis=1), rep_abs=((w * w)[:, :, None] * np.abs(dlt)).sum(axis=1),
                rep=rep, terms=pos.sum(axis=1).astype(np.float64))
