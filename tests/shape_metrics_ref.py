"""The float64 yardstick of the shape-set metrics tests (echoscene_amd/shape_metrics.py, csrc/es_shape_metrics.hip) and the clouds
those tests run on.  The matrix is restated by brute force from its definition, with direct differences and no expansion:

    out[i, j] = mean_p min_q |a_ip - b_jq|^2 + mean_q min_p |a_ip - b_jq|^2

tests/test_shape_metrics_cpu.py pins it to closed forms and to the matrices the reference's _pairwise_EMD_CD_ recorded
(tests/golden/shape_metrics.npz, written by tests/golden/make_golden_shape_metrics.py, which also runs on these clouds)."""
import numpy as np

# the seams of the kernel's tiling (csrc/es_shape_metrics.hip: CM_WQ, CM_PASS, CM_CHUNK)
WAVE_QUERIES = 64          # queries a wave holds per pass: four 16-query tiles
PASS_QUERIES = 256         # queries the four waves of a workgroup take per pass
LDS_CHUNK = 2048           # candidates per LDS stage


def pair_sq_dists(x, y):
    """[P, Q] float64: |x_p - y_q|^2 as the sum of the three squared differences"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = np.zeros((x.shape[0], y.shape[0]))
    for c in range(3):
        d += (x[:, c, None] - y[None, :, c]) ** 2
    return d


def chamfer_pair(x, y):
    d = pair_sq_dists(x, y)
    return d.min(1).mean() + d.min(0).mean()


def chamfer_matrix(a, b=None):
    """float64 [Na, Nb]; a, b: sequences of [P, 3] clouds (b None: a against itself, every entry computed)"""
    b = a if b is None else b
    return np.array([[chamfer_pair(x, y) for y in b] for x in a])


def normalize(pc):
    """the normalisation of the metric script in float64: minus the mean per axis, over the largest absolute coordinate that remains"""
    pc = np.asarray(pc, np.float64)
    pc = pc - pc.mean(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return pc / np.abs(pc).max()


def normalize_f32(pc):
    """the same formula evaluated in float32 throughout: the base of the normalisation test's error bar"""
    pc = np.asarray(pc, np.float32)
    pc = pc - pc.mean(axis=0, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        return pc / np.abs(pc).max()


# ------------------------------------------------------------------------------------------------ clouds
def _family(rs, kind, P):
    if kind == 0:                                                   # gaussian, axes of different width
        return rs.standard_normal((P, 3)) * (0.5 + rs.rand(3))
    if kind == 1:                                                   # an anisotropic box, off centre
        return (rs.rand(P, 3) - 0.5) * np.array([1.0, 0.6, 0.3]) * (0.5 + rs.rand(3)) + rs.standard_normal(3)
    u = rs.standard_normal((P, 3))                                  # points on an ellipsoid
    return u / np.linalg.norm(u, axis=1, keepdims=True) * (0.4 + rs.rand(3))


def clouds(seed, N, P):
    """N clouds of P points, float32 [N, P, 3]: the three families in turn, each cloud normalised (a single point cannot be: it is
    taken from [-1, 1]^3 as it is).  The float32 values ARE the clouds: yardstick, reference and kernel all start from them."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(N):
        pc = _family(rs, (seed + i) % 3, P)
        out.append(normalize(pc) if P > 1 else np.clip(0.5 * pc, -1, 1))
    return np.stack(out).astype(np.float32)


# (Na, Nb, P, Q) of the matrix tests: every Na, Nb in {1, 2, 3}; P, Q around the 16-point tile, the wave's query block, the pass of a
# workgroup and the LDS chunk; P != Q in most
MATRIX_CASES = (
    (1, 1, 1, 1), (2, 3, 1, 17), (3, 2, 15, 16), (1, 2, 16, 16), (2, 1, 17, 15), (2, 2, 64, 1), (3, 1, 16, 64),
    (3, 3, WAVE_QUERIES - 1, WAVE_QUERIES + 1), (2, 2, WAVE_QUERIES, WAVE_QUERIES), (1, 3, WAVE_QUERIES + 1, WAVE_QUERIES - 1),
    (1, 2, PASS_QUERIES - 1, PASS_QUERIES + 1), (2, 1, PASS_QUERIES, PASS_QUERIES), (1, 1, PASS_QUERIES + 1, PASS_QUERIES - 1),
    (1, 1, LDS_CHUNK - 1, LDS_CHUNK + 1), (1, 2, LDS_CHUNK, LDS_CHUNK), (1, 1, LDS_CHUNK + 1, LDS_CHUNK - 1), (2, 2, LDS_CHUNK + 1, 17),
)


def matrix_case(n):
    Na, Nb, P, Q = MATRIX_CASES[n]
    return clouds(1000 + 2 * n, Na, P), clouds(1001 + 2 * n, Nb, Q)


# Clouds on the lattice of multiples of 1/64 in [-1, 1]^3: every product, |x|^2, |y|^2 and every partial sum of the expanded form is a
# multiple of 1/4096 below 2^24 / 4096, so fp32 computes each distance exactly in any order, the double sums are exact, and the only
# rounding is the last one: the kernel must return float32(yardstick) bit for bit.  At each seam index s of the tiling, a[s] is b[s]
# moved by one lattice step, far closer than random lattice points lie: b[s] is the nearest neighbour of a[s] and the other way round,
# so a point lost, doubled or misplaced at a seam -- as a query or as a candidate -- changes the sum.
SEAM_INDICES = (0, 15, 16, 31, 32, 47, 48, WAVE_QUERIES - 1, WAVE_QUERIES, PASS_QUERIES - 1, PASS_QUERIES, LDS_CHUNK - 1, LDS_CHUNK)
LATTICE_CASES = ((1, 1), (15, 17), (33, 31), (WAVE_QUERIES + 1, PASS_QUERIES + 1), (PASS_QUERIES, WAVE_QUERIES), (LDS_CHUNK + 1, LDS_CHUNK + 1),
                 (LDS_CHUNK, PASS_QUERIES - 1), (2 * LDS_CHUNK + 1, LDS_CHUNK - 1))


def lattice_case(n):
    P, Q = LATTICE_CASES[n]
    for attempt in range(100):                                      # (the first seed whose planted pairs are unique nearest neighbours)
        rs = np.random.RandomState(4000 + n + 100 * attempt)
        a, b = rs.randint(-63, 64, size=(P, 3)), rs.randint(-63, 64, size=(Q, 3))
        seams = [s for s in SEAM_INDICES if s < min(P, Q)]
        for s in seams:
            a[s] = b[s] + (1, 0, 0)
        d = pair_sq_dists(a, b)
        if all((d[s] <= 1).sum() == 1 and (d[:, s] <= 1).sum() == 1 for s in seams) or min(P, Q) == 1:
            return (a / 64.0).astype(np.float32)[None], (b / 64.0).astype(np.float32)[None]
    raise AssertionError('no seed found')


# the sets of the end-to-end metrics test and of the bitwise tests
def metric_sets():
    return clouds(77, 6, 64), clouds(78, 6, 64)                     # (sample, ref)


def golden_sets(P):
    return clouds(500 + P, 5, P), clouds(600 + P, 4, P)


# vertex arrays of the sampling / normalisation goldens: (n vertices, number)
SAMPLE_CASES = ((100, 64), (64, 64), (40, 64), (300, 257), (10, 65), (7, 1), (3, 63))


def sample_verts(n):
    rs = np.random.RandomState(900 + n)
    return (_family(rs, n % 3, n) * 3.0 + 5.0).astype(np.float32)   # far from the origin and not unit sized: the normalisation has work to do


def two_smallest_gap(m, axis):
    """the smallest difference between the two smallest entries along ``axis`` (inf entries allowed): the margin a rank-based result has"""
    s = np.sort(m, axis=axis)
    s = s[:2] if axis == 0 else s[:, :2].T
    return float((s[1] - s[0]).min())


def rank_margins(y_rs, y_rr, y_ss):
    """(COV, k-NN) margins of the metric matrices: for COV every sample's two nearest references, for k-NN every column of the block
    matrix with its diagonal excluded (k = 1: the two nearest; k = 3 with two sets of six also rests on the third and fourth, so all
    adjacent gaps among the four nearest count)"""
    cov = two_smallest_gap(y_rs, 0)
    m = np.block([[y_rr, y_rs], [y_rs.T, y_ss]])
    np.fill_diagonal(m, np.inf)
    s = np.sort(m, axis=0)[:4]
    return cov, float(np.diff(s, axis=0).min())
