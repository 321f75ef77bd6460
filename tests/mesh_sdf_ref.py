"""The yardstick of the mesh -> SDF tests: a plain numpy float64 restatement of textbook formulas, independent of the kernel's
formulation (csrc/es_mesh_sdf.hip selects between the foot of the perpendicular and three edge segments from precomputed edge frames;
this walks Ericson's Voronoi regions of the triangle, Real-Time Collision Detection section 5.1.5), plus the meshes the tests run on.
Helper module: no tests here.

Conventions (the inverse of postprocess.sdf_to_mesh): voxel (i, j, k) of an n^3 grid is the point (i/n - 0.5, j/n - 0.5, k/n - 0.5),
array axes x, y, z, negative inside, inside = generalized winding number > 0.5, value clamped to [-trunc, trunc]; triangles of zero
area are dropped."""
import numpy as np


# ------------------------------------------------------------------------------------------------ the reference
def grid_points(n):
    """[n^3, 3] float64 in the order of a C-contiguous [n, n, n] array"""
    g = np.arange(n, dtype=np.float64) / n - 0.5
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)


def _rows(a, b):
    return np.einsum('ij,ij->i', a, b)


def drop_zero_area(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    l2 = np.maximum(np.maximum(_rows(b - a, b - a), _rows(c - b, c - b)), _rows(a - c, a - c))
    return f[area2 > 1e-14 * l2]


def closest_point_on_triangle(p, a, b, c):
    """Ericson's region walk for points p [N, 3] against ONE triangle (a, b, c): the closest points [N, 3]"""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = ap @ ab, ap @ ac
    d3, d4 = bp @ ab, bp @ ac
    d5, d6 = cp @ ab, cp @ ac
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    out = np.empty_like(p)
    todo = np.ones(len(p), bool)

    def take(mask, q):
        m = todo & mask
        out[m] = q[m] if q.ndim == 2 else q
        todo[m] = False

    with np.errstate(divide='ignore', invalid='ignore'):
        take((d1 <= 0) & (d2 <= 0), a)                                                        # vertex region A
        take((d3 >= 0) & (d4 <= d3), b)                                                       # vertex region B
        take((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)           # edge AB
        take((d6 >= 0) & (d5 <= d6), c)                                                       # vertex region C
        take((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)           # edge AC
        take((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))   # edge BC
        den = 1.0 / (va + vb + vc)
        take(np.ones(len(p), bool), a + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac)  # the face
    return out


def distance(points, verts, faces):
    """unsigned distance of points [N, 3] to the mesh, float64 [N]"""
    p = np.asarray(points, np.float64)
    v = np.asarray(verts, np.float64)
    best = np.full(len(p), np.inf)
    for f in drop_zero_area(v, faces):
        q = closest_point_on_triangle(p, v[f[0]], v[f[1]], v[f[2]])
        best = np.minimum(best, np.linalg.norm(p - q, axis=1))
    return best


def winding(points, verts, faces):
    """generalized winding number: (1 / 4 pi) sum 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), float64 [N]"""
    p = np.asarray(points, np.float64)
    v = np.asarray(verts, np.float64)
    w = np.zeros(len(p))
    for f in drop_zero_area(v, faces):
        a, b, c = v[f[0]] - p, v[f[1]] - p, v[f[2]] - p
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        num = _rows(a, np.cross(b, c))
        den = la * lb * lc + _rows(a, b) * lc + _rows(b, c) * la + _rows(c, a) * lb
        w += 2.0 * np.arctan2(num, den)
    return w / (4.0 * np.pi)


def sdf_ref(verts, faces, n, trunc=0.2):
    """dict: 'sdf' float64 [n, n, n] (clamped), 'd' the raw distance [n, n, n], 'w' the winding number [n, n, n]"""
    p = grid_points(n)
    d, w = distance(p, verts, faces), winding(p, verts, faces)
    s = np.clip(np.where(w > 0.5, -d, d), -trunc, trunc)
    return {'sdf': s.reshape(n, n, n), 'd': d.reshape(n, n, n), 'w': w.reshape(n, n, n)}


def fit_transform(verts, fit):
    """centre (of the bounding box) and scale (longest side -> fit) in float64: fitted = (v - centre) * scale"""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    return 0.5 * (lo + hi), fit / (hi - lo).max()


# ------------------------------------------------------------------------------------------------ the meshes (float64, int64)
_QUADS = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # -x +x -y +y -z +z, outward


def cube(half=0.3, centre=(0.01, -0.02, 0.03)):
    """12 triangles, outward; vertex 4 ix + 2 iy + iz; the last two triangles are the +z face"""
    v = np.array([[2 * ix - 1, 2 * iy - 1, 2 * iz - 1] for ix in (0, 1) for iy in (0, 1) for iz in (0, 1)], np.float64) * half + np.asarray(centre)
    f = np.array([t for q in _QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)
    return v, f


def open_cube():
    v, f = cube()
    return v, f[:-2]


def octa(radius=0.37, rx=0.4, rz=0.7, shift=(0.02, 0.01, -0.03)):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * radius
    f = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                t = (sx, 2 + sy, 4 + sz)
                f.append(t if (sx + sy + sz) % 2 == 0 else (t[0], t[2], t[1]))
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    return v @ (Rz @ Rx).T + np.asarray(shift), np.array(f, np.int64)


def subdivide(verts, faces, rounds=1):
    """midpoint subdivision: every triangle -> 4, orientation kept, midpoints shared"""
    v, f = [tuple(x) for x in np.asarray(verts, np.float64)], np.asarray(faces, np.int64)
    for _ in range(rounds):
        mid = {}

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                mid[key] = len(v)
                v.append(tuple(0.5 * (np.array(v[i]) + np.array(v[j]))))
            return mid[key]
        out = []
        for a, b, c in f.tolist():
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = np.array(out, np.int64)
    return np.array(v, np.float64), f


def cube768():
    return subdivide(*cube(), rounds=3)


def cube767():
    v, f = cube768()
    return v, f[:-1]


def two():
    (v0, f0), (v1, f1) = cube(0.12, (-0.21, -0.19, -0.2)), cube(0.15, (0.21, 0.16, 0.11))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])


def sphere(radius=0.3, rounds=4):
    """an octahedron subdivided `rounds` times with every vertex pushed onto the sphere: 8 * 4^rounds triangles, inscribed"""
    v, f = octa(1.0, 0.0, 0.0, (0, 0, 0))
    for _ in range(rounds):
        v, f = subdivide(v, f)
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v * radius, f


MESHES = {'cube': cube, 'open_cube': open_cube, 'octa': octa, 'cube768': cube768, 'cube767': cube767, 'two': two}


def as_f32(verts):
    """the mesh the device sees: vertices rounded to float32 (returned as float64 values)"""
    return np.asarray(verts, np.float32).astype(np.float64)
