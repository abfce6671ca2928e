"""Frames for the robust / cluster-robust one-model GLM report tests (tests/test_glm_sandwich_gpu.py, tests/test_glm_sandwich_cpu.py).

ONE beta for the whole frame: glm_cases.family_frame with a single group of all the rows, then from the same generator, in the order
of glm_weighted_cases.frame_for_sizes, the weights, the offset, beta and y (draw_weights / draw_offset / draw_y).  The clusters cut
the rows afterwards.

The ragged frame: cluster sizes RAGGED (661 rows) sit on every edge of the 4-row matrix instruction, the 64-row step and two steps;
default_rng(77 + p), integer weights with zeros plus an offset.  At p = 16, gamma, the one-row cluster draws weight 0, so G = 9 there:
the case that pins "G counts the clusters with a row of positive weight" (tests/test_glm_sandwich_cpu.py asserts the draw).
"""
import numpy as np

import glm_cases as gc
import glm_weighted_cases as wc

RAGGED = (1, 3, 4, 5, 63, 64, 65, 127, 129, 200)
WIDTHS = (1, 7, 16)
KINDS = ("hc0", "hc1", "cluster", "cluster0")
TOL, MAX_ITER = 1e-10, 100


def one_model_frame(rng, family, n, p, weighted=True, with_offset=True):
    """(X [n, p], y [n], pw or None, o or None): one beta for all the rows"""
    X, y, _, pw, o = wc.frame_for_sizes(rng, family, [n], p, "integer", with_offset)
    return X, y, (pw if weighted else None), (o if with_offset else None)


def plain_frame(rng, family, n, p):
    """(X, y) of family_frame with one group: no weights, no offset"""
    X, y, _ = gc.family_frame(rng, family, [n], p)
    return X, y


def ragged(family, p, weighted=True):
    """(X, y, off, codes, pw, o) of the ragged frame"""
    rng = np.random.default_rng(77 + p)
    X, y, pw, o = one_model_frame(rng, family, int(sum(RAGGED)), p, weighted, True)
    off = gc.offsets(RAGGED)
    return X, y, off, codes_of(off), pw, o


def codes_of(off):
    """the cluster index of every row of contiguous clusters"""
    off = np.asarray(off)
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.int64)


def lopsided(family, p, big=500, small=(3, 7, 2, 11, 5, 64, 9)):
    """one long cluster among small ones: (X, y, off, codes); no weights, no offset"""
    rng = np.random.default_rng(501 + p)
    sizes = list(small[:3]) + [big] + list(small[3:])
    X, y = plain_frame(rng, family, int(sum(sizes)), p)
    off = gc.offsets(sizes)
    return X, y, off, codes_of(off)
