"""fp64 numpy restatement of the linear layer on CBSR features (cbsr_linear.hip): only the terms a
row selects exist, so a non-finite weight column reaches only the rows that select it."""
import numpy as np


def _slots(idx, D):
    """(j, rows, columns) of the slots whose selector is < D, slot by slot."""
    for j in range(idx.shape[1]):
        d = idx[:, j].astype(np.int64)
        rows = np.flatnonzero(d < D)
        yield j, rows, d[rows]


def forward(val, idx, W, bias=None, prior=None):
    W = W.astype(np.float64)
    y = np.zeros((idx.shape[0], W.shape[0])) if prior is None else prior.astype(np.float64)
    if bias is not None:
        y = y + bias.astype(np.float64)
    with np.errstate(invalid="ignore"):
        for j, rows, d in _slots(idx, W.shape[1]):
            y[rows] += val[rows, j, None].astype(np.float64) * W[:, d].T
    return y


def grad_values(g, idx, W):
    out = np.zeros(idx.shape)
    with np.errstate(invalid="ignore"):
        for j, rows, d in _slots(idx, W.shape[1]):
            out[rows, j] = (g[rows].astype(np.float64) * W[:, d].T.astype(np.float64)).sum(1)
    return out


def grad_weight(g, val, idx, D):
    gwt = np.zeros((D, g.shape[1]))
    with np.errstate(invalid="ignore"):
        for j, rows, d in _slots(idx, D):
            np.add.at(gwt, d, g[rows].astype(np.float64) * val[rows, j, None].astype(np.float64))
    return gwt.T
