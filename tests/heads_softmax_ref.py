"""Expected values and bounds of the multi-head GAT edge softmax (edge_softmax_heads.hip): the
single-head reference of tests/edge_softmax_ref.py on each head's slice, stacked head-major.  The
heads share the graph and nothing else, so there is nothing to add: no new formula, no new
constant.  test_heads_softmax_cpu.py pins the stacking against float64 torch autograd of a
multi-head composition."""
from collections import namedtuple

import numpy as np

import edge_softmax_ref as ER

#: per head: the Fwd / Bwd of edge_softmax_ref; stacked [H, ...]: what the kernels are checked on
HeadsFwd = namedtuple("HeadsFwd", "heads w bound")
HeadsBwd = namedtuple("HeadsBwd", "heads g_dst g_dst_bound g_src g_src_bound")


def gat_forward_heads(rp, col, s_dst, s_src, slope):
    """s_dst [H, R], s_src [H, C] (fp32) -> w [H, E] in float64 with its per-element bound."""
    fs = [ER.gat_forward(rp, col, s_dst[h], s_src[h], slope) for h in range(s_dst.shape[0])]
    return HeadsFwd(fs, np.stack([f.w for f in fs]), np.stack([f.bound for f in fs]))


def backward_heads(rp, col, fwd, gw, slope, num_cols, gw_bound=None):
    """Both score gradients [H, R] / [H, C] of gw [H, E] with their bounds; gw_bound [H, E]: the
    bound of a gw that was itself computed."""
    bs = [ER.backward(rp, col, f, gw[h], slope, num_cols,
                      gw_bound=None if gw_bound is None else gw_bound[h])
          for h, f in enumerate(fwd.heads)]
    st = lambda name: np.stack([getattr(b, name) for b in bs])  # noqa: E731
    return HeadsBwd(bs, st("g_dst"), st("g_dst_bound"), st("g_src"), st("g_src_bound"))


def heads_slice(x, H):
    """The first H heads of a HeadsFwd / HeadsBwd."""
    return type(x)(x.heads[:H], *(a[:H] for a in x[1:]))
