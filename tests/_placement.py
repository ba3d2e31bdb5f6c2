"""Operands of the direct kernel tests as sub-blocks of larger parents (the placement of test_gpu_gemm_core.place, with
an optional leading dimension of the caller's choice): a wrong leading dimension, a tail that runs past the block or an
aligned-load assumption then reads the NaN around an input or overwrites the sentinel around an output."""
import numpy as np

SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison


def place(ctx, block, sub=True, fill=np.nan, ld=None, row0=2):
    """Upload `block` (r x c). sub=False: a matrix of its own (ld = r). sub=True: inside a parent with leading dimension
    `ld` (default: the smallest odd number >= r + 3), starting at row `row0` (2, or 1) of column 1. The element offset
    is ld + row0: with an odd ld and row0 = 2, or an even ld and row0 = 1, it is odd and the block's first element is 8-
    but not 16-byte aligned; with an even ld and row0 = 2 it is 16-byte aligned. The rest of the parent holds `fill`.
    Returns (parent DeviceMatrix, pointer, ld, r0, c0)."""
    r, c = block.shape
    if not sub:
        d = ctx.from_numpy(np.asfortranarray(block))
        return d, d.ptr, r, 0, 0
    assert row0 in (1, 2)
    if ld is None:
        ld = r + 3 if (r + 3) % 2 else r + 4
    assert ld >= r + row0 + 1
    host = np.full((ld, c + 2), fill, order="F")
    host[row0:row0 + r, 1:1 + c] = block
    d = ctx.from_numpy(host)
    assert (d.t.data_ptr() + 8 * (ld + row0)) % 16 == (8 if (ld + row0) % 2 else 0)
    return d, d.col_ptr(1, row0), ld, row0, 1


def placements(r):
    """The three placements of a block of r rows, as keyword arguments of place(). odd: odd ld, first element 8- but not
    16-byte aligned; even-aligned: even ld > r, 16-byte aligned; even-misaligned: the same even ld, 8- but not 16-byte
    aligned."""
    even = r + 4 if r % 2 == 0 else r + 5
    return {"odd": dict(ld=None, row0=2), "even-aligned": dict(ld=even, row0=2), "even-misaligned": dict(ld=even, row0=1)}


def take(parent, r0, c0, r, c, what):
    """The r x c block of a placed output, after checking that everything around it still holds the sentinel."""
    out = np.array(parent.to_numpy())
    blk = out[r0:r0 + r, c0:c0 + c].copy()
    out[r0:r0 + r, c0:c0 + c] = SENT
    assert (out == SENT).all(), (what, "wrote outside its block")
    return blk
