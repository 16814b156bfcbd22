"""numpy restatement of the orientation codes of the oriented entries (include/acf_hip.h: ACF_HIP_ORIENT_*): code = rot + 4 * mirror,
the upright frame is the source mirrored left-right first, then turned rot quarter turns clockwise."""
import numpy as np


def orient(S, code, axes=(0, 1)):
    """The upright frame(s) of source S; axes: where (rows, columns) are in S."""
    rot, mirror = code & 3, code >> 2
    return np.rot90(np.flip(S, axes[1]) if mirror else S, k=-rot, axes=axes)


def inverse_code(code):
    """The code that turns the upright frame back into the source: a mirrored code undoes itself, a rotation by the opposite one."""
    return code if code >> 2 else (4 - code) & 3


def unorient(U, code, axes=(0, 1)):
    """The source of upright U: the inverse permutation of orient()."""
    return orient(U, inverse_code(code), axes)


def dims(rows, cols, code):
    return (cols, rows) if code & 1 else (rows, cols)


def source_index(code, rows, cols):
    """(rs, cs): for every upright pixel (r, c) the source pixel it reads — the table of the header, written out."""
    rot, mirror = code & 3, code >> 2
    h, w = dims(rows, cols, code)
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rs, cs = [(r, c), (rows - 1 - c, r), (rows - 1 - r, cols - 1 - c), (c, cols - 1 - r)][rot]
    return rs, (cols - 1 - cs if mirror else cs)


def unorient_box(code, rows, cols, box):
    """The documented closed form of acf_hip_unorient_rect: upright {x, y, w, h} -> source {x, y, w, h}, any box."""
    x, y, w, h = box
    rot, mirror = code & 3, code >> 2
    swap, rev_r, rev_c = rot & 1, rot in (1, 2), (rot >= 2) != bool(mirror)
    r0, nr = (x, w) if swap else (y, h)     # along the source rows
    c0, nc = (y, h) if swap else (x, w)     # along the source columns
    return [cols - c0 - nc if rev_c else c0, rows - r0 - nr if rev_r else r0, nc, nr]


def box_of_mask(m):
    """{x, y, w, h} of the bounding box of a boolean mask."""
    ys, xs = np.nonzero(m)
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]
