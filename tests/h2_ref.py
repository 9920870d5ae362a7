"""The scale rule of the f16 forward scatter (H2Scale / h2_decide_uniform of csrc/mma.h, driven by strip_main_h of
csrc/aggregate.hip) restated in plain Python integers.

Written from the documented rule, never calling the library: the host program tests/split_cpu.hip runs the header's own
statements and must give THIS trajectory, and the GPU tests take from here which path a wave took and at which exponent a
block was split, so a defect cannot sit in the rule and in its reference alike.

A wave streams blocks of 16 rows x 32 columns; it multiplies the two f16 pieces of x * 2^e.  State: e = 120, e_floor = -110,
seen = False.  Block b with finite magnitude maximum m (infinities and NaNs left out; has_inf[b]: it holds an infinity):

  asked   = b == 0  or  m > 2^(15 - e)  or  has_inf[b]        (the kernel looks only at a block that does not fit)
  asked and m > 0:
     fe = floor(log2 m) + 1;   en = min(max(13 - fe, -110), e)
     not seen            -> FIRST:     e = en, e_floor = en - 10, seen
     en >= e_floor       -> LOWER:     e = en (accumulators times 2^(en - e); NOTHING if en == e)
     fe + e >= 100       -> REANCHOR:  e = en, e_floor = en - 10
     otherwise           -> OUTLIER:   the block alone as three exact bf16 pieces, e unchanged
  otherwise              -> NOTHING

The block is split at the e AFTER its decision (OUTLIER: exact at the unchanged e).
"""
import numpy as np

E_INIT, E_MIN, E_DROP, E_REANCHOR = 120, -110, 10, 100
NOTHING, FIRST, LOWER, OUTLIER, REANCHOR = 0, 1, 2, 3, 4
PATH_NAMES = ("nothing", "first", "lower", "outlier", "reanchor")


def frexp_exp(m):
    """floor(log2 m) + 1 of a finite float32 m > 0 (denormals included)."""
    return int(np.frexp(np.float32(m))[1])


def walk(maxima, has_inf=None):
    """maxima: the finite block maxima of one wave (float32, >= 0), in streaming order -> (e per block, path per block,
    e_out): int arrays of len(maxima) and the exponent the accumulators are left in."""
    maxima = np.asarray(maxima, dtype=np.float32)
    n = len(maxima)
    es, paths = np.empty(n, np.int64), np.empty(n, np.int64)
    e, e_floor, seen = E_INIT, E_MIN, False
    for b in range(n):
        m = float(maxima[b])
        path = NOTHING
        asked = b == 0 or m > 2.0 ** (15 - e) or (has_inf is not None and bool(has_inf[b]))
        if asked and m > 0.0:
            fe = frexp_exp(m)
            en = min(max(13 - fe, E_MIN), e)
            if not seen:
                seen, e_floor, e, path = True, en - E_DROP, en, FIRST
            elif en >= e_floor:
                path = LOWER if en != e else NOTHING
                e = en
            elif fe + e >= E_REANCHOR:
                e_floor, e, path = en - E_DROP, en, REANCHOR
            else:
                path = OUTLIER
        es[b], paths[b] = e, path
    return es, paths, e


def floor_exponents(es, paths):
    """-> per block, the exponent e of the ABSOLUTE floor 2^-25 * 2^-e of a term of that block: the e it was split at, or
    the e of a LATER re-anchor of the wave if that is lower.  Lowering inside e_floor multiplies the accumulators by at most
    2^-10 in all: exact.  A re-anchor multiplies them by as little as 2^-126 (by 2^max(d, -126): a sum more than 2^126 below
    the new scale is then a small wrong number, further down it is flushed), so what was summed before it is kept exactly
    only while it lies within 2^100 of the new scale, and within the new floor otherwise."""
    es, paths = np.asarray(es), np.asarray(paths)
    out, lowest = np.empty(len(es), np.int64), 1 << 20
    for b in range(len(es) - 1, -1, -1):
        out[b] = min(int(es[b]), lowest)
        if paths[b] == REANCHOR:
            lowest = min(lowest, int(es[b]))
    return out


def block_maxima(x_abs_finite, rows_per_block=16):
    """|x| with the non-finite entries zeroed, [n_rows (a multiple of 16 is not required), 32] -> maxima per block of 16 rows."""
    a = np.asarray(x_abs_finite, dtype=np.float32)
    pad = (-a.shape[0]) % rows_per_block
    if pad:
        a = np.concatenate([a, np.zeros((pad,) + a.shape[1:], np.float32)])
    return a.reshape(a.shape[0] // rows_per_block, -1).max(axis=1)
