"""fp64 numpy restatement of the fused linear + MaxK (linear_maxk.hip): the dense product, then
each row's k winners in the project's top-k order -- value descending, column ascending on ties,
NaN largest."""
import numpy as np


def hidden(x, W, b=None):
    with np.errstate(invalid="ignore", over="ignore"):
        h = x.astype(np.float64) @ W.T.astype(np.float64)
        return h if b is None else h + b.astype(np.float64)


def topk(h, k):
    """(values [V, k], columns [V, k]) of h's rows."""
    nan = np.isnan(h)
    cols = np.broadcast_to(np.arange(h.shape[1]), h.shape)
    order = np.lexsort((cols, -np.where(nan, 0.0, h), ~nan))[:, :k]  # the last key ranks first
    return np.take_along_axis(h, order, 1), order.astype(np.uint8)
