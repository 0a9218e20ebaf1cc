"""numpy restatement of row-keyed noise (``mc_ctx_set_row_seeds``), on ``oracle/philox_oracle``: the way the kernels walk it.

The kernels walk FLAT groups of four elements of ``[B, T, C]`` (so every other operand keeps its f32x4 form) and look the noise up per
element: flat element ``i`` is element ``r = i % (T C)`` of row ``b = i // (T C)`` and takes lane ``r % 4`` of the Philox block with
key ``seeds[b]`` and counter ``(r // 4, draw)``.  Where ``T C % 4 != 0`` a flat group straddles two rows, or sits askew of the row's own
blocks; the lookup does not care.  The definition it must meet: row ``b`` equals ``draw_normal(T C, seeds[b], draw)``.
"""
import numpy as np

from oracle import philox_oracle as P


def draw_rows(seeds, T, C, draw):
    """[B, T, C] float32, walked in flat groups of four as ``philox_rows_fill_k`` / ``sampler_update_k<.., RowNoise>`` do"""
    B, TC = len(seeds), T * C
    n = B * TC
    blocks = {}                    # row -> its stream as [blocks, 4]: block c = the Philox call with key seeds[b], counter (c, draw)
    out = np.zeros(n, dtype=np.float32)
    for i0 in range(0, n, 4):
        for i in range(i0, min(i0 + 4, n)):
            b, r = divmod(i, TC)
            if b not in blocks:
                blocks[b] = P.draw_normal(4 * ((TC + 3) // 4), int(seeds[b]), int(draw)).reshape(-1, 4)
            out[i] = blocks[b][r // 4, r % 4]
    return out.reshape(B, T, C)


def straddling_groups(B, T, C):
    """how many flat groups of four hold elements of two rows"""
    TC, n = T * C, B * T * C
    return sum(1 for i0 in range(0, n - 3, 4) if i0 // TC != (i0 + 3) // TC)
