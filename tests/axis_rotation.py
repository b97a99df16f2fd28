"""The same membrane with its normal along x or y — TEST HELPER, numpy only, no test functions.

`rotate(tables, xyz, box9, dim)` relabels the coordinates CYCLICALLY: old z becomes `dim`, old x becomes (dim + 1) % 3,
old y becomes (dim + 2) % 3.  Cyclic, because the local-leaflet code sums `da * da + db * db` with da = (dim + 1) % 3,
db = (dim + 2) % 3, dn = dim: under this relabelling the first in-plane, second in-plane and normal coordinate of the
rotated system ARE the x, y and z of the original one, in that order, so every leaflet distance and flag of the rotated
run can be compared bit for bit with the z run.  (A plain x <-> z swap would hand the two in-plane terms over in the
other order.)  The frames are permuted, never regenerated: jitter, wrapping and every float stay what they were.

Everything of the tables that names an axis follows: `normal`, `leaflets.normal_dim`, the geometry's point, extents,
orientation and structure box, and the ordermap's plane.  The plane codes are 0 = (x, y), 1 = (x, z), 2 = (z, y)
(Plane::projection2plane); the image of a plane may be one of them with its two axes exchanged — (x, y) becomes (y, z)
for dim = 0 and (z, x) for dim = 1 — and then span_x / span_y and the two bin sizes are exchanged and the maps come out
TRANSPOSED: `maps_transposed(plane, dim)` tells, `maps_like_z(maps, plane, dim)` undoes it.

dim = 2 returns its arguments unchanged (the same objects): the control of every parametrisation.
"""
import copy

import numpy as np

PLANE_AXES = {0: (0, 1), 1: (0, 2), 2: (2, 1)}          # plane code -> (first axis, second axis)
_PLANE_OF = {v: k for k, v in PLANE_AXES.items()}


def dest(dim):
    """dest[old axis] = the axis it becomes."""
    return [(dim + 1) % 3, (dim + 2) % 3, dim]


def source(dim):
    """source[new axis] = the old axis it holds: rotated[..., j] = original[..., source(dim)[j]]."""
    src = [0, 0, 0]
    for old, new in enumerate(dest(dim)):
        src[new] = old
    return src


def rotate_vectors(v, dim):
    """Coordinates, normals, box edges, points: anything whose last axis is (x, y, z)."""
    if dim == 2 or v is None:
        return v
    return np.ascontiguousarray(np.asarray(v)[..., source(dim)])


def unrotate_vectors(v, dim):
    """The inverse of rotate_vectors: a rotated run's vectors in the axes of the z run."""
    if dim == 2 or v is None:
        return v
    return np.ascontiguousarray(np.asarray(v)[..., dest(dim)])


def rotate_box9(box9, dim):
    if dim == 2 or box9 is None:
        return box9
    src = source(dim)
    b = np.asarray(box9)
    return np.ascontiguousarray(b[..., src, :][..., :, src])


def rotate_plane(plane, dim):
    """-> (plane code of the image, whether its two axes are exchanged)."""
    d = dest(dim)
    a, b = PLANE_AXES[plane]
    image = (d[a], d[b])
    if image in _PLANE_OF:
        return _PLANE_OF[image], False
    return _PLANE_OF[(image[1], image[0])], True


def maps_transposed(plane, dim):
    return rotate_plane(plane, dim)[1]


def maps_like_z(maps, plane, dim):
    """Ordermaps [..., nx, ny] of a rotated run in the layout of the z run (`plane` = the z run's plane)."""
    return np.swapaxes(maps, -1, -2) if maps_transposed(plane, dim) else maps


def rotate_tables(tables, dim):
    if dim == 2:
        return tables
    t = copy.deepcopy(tables)
    src, d = source(dim), dest(dim)
    t.normal = tuple(float(tables.normal[s]) for s in src)
    # the leaflet normal is an axis of its own: whatever it was, it moves with the coordinates
    t.leaflets.normal_dim = d[int(tables.leaflets.normal_dim)]
    g = tables.geometry
    dims = (g.xdim, g.ydim, g.zdim)
    t.geometry.point = tuple(float(g.point[s]) for s in src)
    t.geometry.xdim, t.geometry.ydim, t.geometry.zdim = (tuple(dims[s]) for s in src)
    t.geometry.orientation = d[int(g.orientation)]
    t.geometry.structure_box = tuple(float(g.structure_box[s]) for s in src)
    om = tables.ordermap
    t.ordermap.plane, swapped = rotate_plane(int(om.plane), dim)
    if swapped:
        t.ordermap.span_x, t.ordermap.span_y = tuple(om.span_y), tuple(om.span_x)
        t.ordermap.bin = (om.bin[1], om.bin[0])
    return t


def rotate(tables, xyz, box9, dim, normals=None):
    """-> (tables', xyz', box9'), or with manual normals / a table of normals [..., 3]: (tables', xyz', box9', normals')."""
    out = (tables, xyz, box9) if dim == 2 else (rotate_tables(tables, dim), rotate_vectors(xyz, dim), rotate_box9(box9, dim))
    return out if normals is None else out + (rotate_vectors(normals, dim),)
