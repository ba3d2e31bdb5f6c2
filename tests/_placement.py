"""Operands of the direct kernel tests as sub-blocks of larger parents (the placement of test_gpu_gemm_core.place, with
an optional leading dimension of the caller's choice): a wrong leading dimension, a tail that runs past the block or an
aligned-load assumption then reads the NaN around an input or overwrites the sentinel around an output."""
import numpy as np

SENT = -98765.4321          # finite and non-zero: `==` on it is a bitwise comparison


def place(ctx, block, sub=True, fill=np.nan, ld=None):
    """Upload `block` (r x c). sub=False: a matrix of its own (ld = r). sub=True: inside a parent with leading dimension
    `ld` (default: the smallest odd number >= r + 3), starting at row 2 of column 1; with an odd ld that is an odd
    element offset, so the block's first element is 8- but not 16-byte aligned. The rest of the parent holds `fill`.
    Returns (parent DeviceMatrix, pointer, ld, r0, c0)."""
    r, c = block.shape
    if not sub:
        d = ctx.from_numpy(np.asfortranarray(block))
        return d, d.ptr, r, 0, 0
    if ld is None:
        ld = r + 3 if (r + 3) % 2 else r + 4
    assert ld >= r + 3
    host = np.full((ld, c + 2), fill, order="F")
    host[2:2 + r, 1:1 + c] = block
    d = ctx.from_numpy(host)
    if ld % 2:
        assert (d.t.data_ptr() + 8 * (ld + 2)) % 16 == 8
    return d, d.col_ptr(1, 2), ld, 2, 1


def take(parent, r0, c0, r, c, what):
    """The r x c block of a placed output, after checking that everything around it still holds the sentinel."""
    out = np.array(parent.to_numpy())
    blk = out[r0:r0 + r, c0:c0 + c].copy()
    out[r0:r0 + r, c0:c0 + c] = SENT
    assert (out == SENT).all(), (what, "wrote outside its block")
    return blk
