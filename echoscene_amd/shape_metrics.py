"""Shape-set metrics of the reference's ``scripts/compute_mmd_cov_1nn.py`` on the device -- SURVEY.md section 8(f) rank 4: generated
SDF -> mesh (``postprocess.marching_cubes_batch``) -> point cloud (``point_clouds``) -> matrix of Chamfer distances
(``pairwise_chamfer``, csrc/es_shape_metrics.hip) and of earth mover's distances (``pairwise_emd``, csrc/es_emd.hip) -> MMD, COV and
1-NN accuracy by either distance (``compute_all_metrics``).  The matrices are the expensive part and stay on the device; the N x N
statistics after them are bookkeeping and run in numpy on one copy of the matrices.

``lgan_mmd_cov``, ``knn`` and ``compute_all_metrics`` take the call shapes of the reference's functions of those names and return the
same keys; they are written from the formulas (Achlioptas et al. 2018 for MMD / COV, Lopez-Paz & Oquab 2017 for the 1-NN two-sample
test).  The six EMD entries are computed on request (``emd=True``): they are the values of the reference's exact route (``emd_approx``,
an assignment solver on the host, once per pair) within ``EMD_EPS`` per matrix entry, from an auction kernel that solves one pair per
workgroup; the approximate values of the reference's accelerated route, an extension outside its tree, are not reproduced."""
import ctypes as C
import numpy as np
import torch

from . import hip

_CD_KEYS = ('lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc')
_EMD_KEYS = tuple(k.replace('CD', 'EMD') for k in _CD_KEYS)

# |pairwise_emd - exact optimum| per entry for clouds whose joint bounding box has every extent below 4 (normalised clouds: at most 2);
# the derivation is in the header of csrc/es_emd.hip.  Larger clouds: times 2^(e - 3), e the scale exponent derived there.
EMD_EPS = 4e-6


def __getattr__(name):
    if name == 'EMD_MAX_POINTS':                                    # read from the library on first use, a plain attribute from then on
        globals()[name] = int(hip.lib().es_emd_max_points())
        return globals()[name]
    raise AttributeError('module %r has no attribute %r' % (__name__, name))


def sample_indices(n, number=5000):
    """The vertex indices the reference's ``sample_pc`` draws for a cloud of ``n`` vertices: ``np.random.seed(42)`` before every cloud,
    then the first ``number`` entries of ``permutation(n)`` when n >= number and ``randint(0, n, number)`` otherwise.  A RandomState(42)
    of its own gives the same stream and leaves the global generator alone.  Host only; int32 [number]."""
    rs = np.random.RandomState(42)
    idx = rs.permutation(n)[:number] if n >= number else rs.randint(0, n, size=number)
    return idx.astype(np.int32)


def point_clouds(meshes, number=5000):
    """``sample_pc`` + ``normalization`` of the reference for K meshes at once: float32 [K, number, 3] on the device.

    ``meshes``: a list of (verts, faces) pairs or of bare ``verts`` [V, 3] floating-point CUDA tensors (what ``marching_cubes_batch`` or
    ``sdf_to_mesh`` return; one pair or one tensor is K = 1).  Only the vertices are used, as in the reference (``obj.vertices``).  The
    indices follow ``sample_indices``; gather and normalisation run on the device (es_cloud_normalize): the mean of the gathered points
    per axis is subtracted and the cloud divided by the largest absolute coordinate that remains, in double, rounded to float once.
    A cloud whose points all coincide (``number=1``, for one) is 0 / 0 = NaN, exactly as in the reference.
    Every refusal of the arguments is a ValueError raised before any device work."""
    if torch.is_tensor(meshes) or (isinstance(meshes, tuple) and len(meshes) == 2 and torch.is_tensor(meshes[0]) and meshes[0].dim() == 2
                                   and torch.is_tensor(meshes[1]) and not meshes[1].is_floating_point()):
        meshes = [meshes]
    if not isinstance(meshes, (list, tuple)) or len(meshes) == 0:
        raise ValueError('point_clouds: expects a non-empty list of (verts, faces) pairs or verts tensors')
    if not isinstance(number, (int, np.integer)) or isinstance(number, bool) or number < 1:
        raise ValueError('point_clouds: number must be an integer >= 1, got %r' % (number,))
    number = int(number)
    verts = []
    for k, m in enumerate(meshes):
        v = m[0] if isinstance(m, (list, tuple)) and len(m) == 2 else m
        if not torch.is_tensor(v):
            raise ValueError('point_clouds: mesh %d is neither a (verts, faces) pair nor a verts tensor' % k)
        if not (v.dim() == 2 and v.shape[1] == 3 and v.is_floating_point()):
            raise ValueError('point_clouds: verts of mesh %d must be a floating-point tensor [V, 3], got %s %s' % (k, v.dtype, tuple(v.shape)))
        if v.shape[0] == 0:
            raise ValueError('point_clouds: mesh %d has no vertices' % k)
        verts.append(v)
    K = len(verts)
    if K * number * 3 >= 2 ** 31:
        raise ValueError('point_clouds: %d clouds of %d points are beyond int32 indexing' % (K, number))
    dev = None
    for k, v in enumerate(verts):
        if not v.is_cuda:
            raise ValueError('point_clouds: mesh %d is not on the device (CUDA tensors expected)' % k)
        dev = v.device if dev is None else dev
        if v.device != dev:
            raise ValueError('point_clouds: mesh %d is on %s, the first mesh on %s (different devices)' % (k, v.device, dev))
    vofs = np.cumsum([0] + [int(v.shape[0]) for v in verts])
    if int(vofs[-1]) * 3 >= 2 ** 31:
        raise ValueError('point_clouds: %d vertices in all are beyond int32 indexing' % int(vofs[-1]))
    index = np.stack([sample_indices(int(v.shape[0]), number) for v in verts])
    return _normalize(torch.cat([v.float() for v in verts]).contiguous(), vofs, index, 'point_clouds')


def _normalize(verts, vofs, index, who):
    """es_cloud_normalize on packed vertices (device), host offsets [K + 1] and host indices [K, number]"""
    dev = verts.device
    K, number = index.shape
    with torch.cuda.device(dev):
        vo = torch.from_numpy(np.asarray(vofs, np.int64)).to(dev)
        ix = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
        bad = torch.empty(K, dtype=torch.int32, device=dev)
        out = torch.empty(K, number, 3, dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        hip.check(hip.lib().es_cloud_normalize(p(verts), p(vo), p(ix), K, number, int(vofs[-1]), p(bad), p(out), hip.current_stream()),
                  'es_cloud_normalize')
        flagged = bad.cpu().nonzero().flatten().tolist()
    if flagged:
        raise ValueError('%s: clouds %s have a point index outside [0, V)' % (who, flagged))
    return out


def _check_sets(who, squares, emd=False, **sets):
    """the refusals shared by the calls that take sets of clouds, in the order: tensor, floating point, [N, P, 3], int32, (``emd``: equal
    point counts, at most EMD_MAX_POINTS,) one device, CUDA (``squares``: each set is also paired with itself)"""
    for name, x in sets.items():
        if not torch.is_tensor(x):
            raise ValueError('%s: %s must be a tensor [N, P, 3], got %s' % (who, name, type(x).__name__))
        if not x.is_floating_point():
            raise ValueError('%s: %s must be floating point, got %s' % (who, name, x.dtype))
        if not (x.dim() == 3 and x.shape[2] == 3 and x.shape[0] > 0 and x.shape[1] > 0):
            raise ValueError('%s: %s must be [N, P, 3] with N, P >= 1, got %s' % (who, name, tuple(x.shape)))
        if x.shape[0] * x.shape[1] * 3 >= 2 ** 31:
            raise ValueError('%s: %s with %d x %d x 3 coordinates is beyond int32 indexing' % (who, name, x.shape[0], x.shape[1]))
    xs = list(sets.items())
    if emd:
        for name, x in xs[1:]:
            if x.shape[1] != xs[0][1].shape[1]:
                raise ValueError('%s: the earth mover\'s distance needs equal point counts, %s has %d points per cloud and %s %d'
                                 % (who, xs[0][0], xs[0][1].shape[1], name, x.shape[1]))
        most = globals().get('EMD_MAX_POINTS') or __getattr__('EMD_MAX_POINTS')
        if xs[0][1].shape[1] > most:
            raise ValueError('%s: %d points per cloud, the earth mover\'s distance takes at most EMD_MAX_POINTS = %d'
                             % (who, xs[0][1].shape[1], most))
    for name, x in xs[1:]:
        if x.device != xs[0][1].device:
            raise ValueError('%s: %s is on %s and %s on %s (different devices)' % (who, xs[0][0], xs[0][1].device, name, x.device))
        if x.shape[0] * xs[0][1].shape[0] >= 2 ** 31:
            raise ValueError('%s: %d x %d pairs are beyond int32 indexing' % (who, xs[0][1].shape[0], x.shape[0]))
    for name, x in xs:
        if squares and x.shape[0] ** 2 >= 2 ** 31:
            raise ValueError('%s: %d x %d pairs are beyond int32 indexing' % (who, x.shape[0], x.shape[0]))
        if not x.is_cuda:
            raise ValueError('%s: %s is not on the device (a CUDA tensor is expected)' % (who, name))


def pairwise_chamfer(a, b=None):
    """The matrix of Chamfer distances between every cloud of ``a`` [Na, P, 3] and every cloud of ``b`` [Nb, Q, 3] (floating-point
    CUDA tensors): float32 [Na, Nb] on the device, ``out[i, j] = mean_p min_q |a_ip - b_jq|^2 + mean_q min_p |a_ip - b_jq|^2`` --
    the CD matrix of the reference's ``_pairwise_EMD_CD_`` (``dl.mean(1) + dr.mean(1)``).  ``b=None`` is the symmetric case of one set
    against itself: half the pairs are computed and mirrored, and the diagonal is exactly 0.

    One workgroup per pair (csrc/es_shape_metrics.hip): an entry's bits depend on its two clouds alone, so a matrix equals the
    matrices of its parts, ``pairwise_chamfer(a, b) == pairwise_chamfer(b, a).T`` bit for bit, and runs repeat.  Distances are the
    expanded form |x|^2 + |y|^2 - 2 x.y in fp32, the arithmetic of the reference's ``distChamfer``; it cancels for coordinates far
    from the origin, so the clouds are expected normalised as ``point_clouds`` (the reference's ``normalization``) leaves them:
    centred, largest |coordinate| 1.  ``chamfer.chamferDist`` (direct differences) serves clouds that are not.  A nearest-neighbour
    distance that the expansion makes slightly negative (about -1e-7 for coincident points) is counted as 0.
    Every refusal of the arguments is a ValueError raised before any device work."""
    if b is None:
        _check_sets('pairwise_chamfer', True, a=a)
    else:
        _check_sets('pairwise_chamfer', False, a=a, b=b)
    return _chamfer_matrix(a, b)


def _chamfer_matrix(a, b):
    """es_chamfer_matrix on checked arguments; b None: the symmetric mode"""
    with torch.cuda.device(a.device):
        a = a.float().contiguous()
        sym = b is None
        b = a if sym else b.float().contiguous()
        out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        hip.check(hip.lib().es_chamfer_matrix(p(a), a.shape[0], a.shape[1], p(b), b.shape[0], b.shape[1], 1 if sym else 0, p(out),
                                              hip.current_stream()), 'es_chamfer_matrix')
    return out


def pairwise_emd(a, b=None):
    """The matrix of earth mover's distances between every cloud of ``a`` [Na, P, 3] and every cloud of ``b`` [Nb, P, 3] (floating-point
    CUDA tensors with the same P, at most ``EMD_MAX_POINTS``): float32 [Na, Nb] on the device, ``out[i, j]`` = the minimum over
    one-to-one matchings sigma of ``mean_p |a_ip - b_j,sigma(p)|`` (Euclidean), the value of the reference's ``emd_approx``, within
    ``EMD_EPS`` of the exact optimum.  ``b=None`` is one set against itself: half the pairs are computed and mirrored, and the
    diagonal is exactly 0.

    One workgroup per pair runs an integer auction (csrc/es_emd.hip): an entry's bits depend on its two clouds and their order alone,
    so a matrix equals the matrices of its parts and runs repeat; ``pairwise_emd(a, b)`` and ``pairwise_emd(b, a).T`` agree within the
    guarantee, not bit for bit (bidders and objects differ).  Distances are direct differences: the clouds need not be normalised.
    Every refusal of the arguments is a ValueError raised before any device work; a pair with a non-finite coordinate, or one that
    reached the kernel's cap on bidding rounds, raises a RuntimeError that names the pairs."""
    if b is None:
        _check_sets('pairwise_emd', True, emd=True, a=a)
    else:
        _check_sets('pairwise_emd', False, emd=True, a=a, b=b)
    return _raise_on_status('pairwise_emd', *_emd_matrix(a, b))


def _emd_matrix(a, b, rounds=False):
    """es_emd_matrix on checked arguments; b None: the symmetric mode.  (out, status[, rounds]) on the device"""
    with torch.cuda.device(a.device):
        a = a.float().contiguous()
        sym = b is None
        b = a if sym else b.float().contiguous()
        out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
        status = torch.empty(a.shape[0], b.shape[0], dtype=torch.int32, device=a.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        if rounds:
            nr = torch.empty_like(status)
            hip.check(hip.lib().es_emd_matrix_rounds(p(a), a.shape[0], p(b), b.shape[0], a.shape[1], 1 if sym else 0, p(out), p(status),
                                                     p(nr), hip.current_stream()), 'es_emd_matrix_rounds')
            return out, status, nr
        hip.check(hip.lib().es_emd_matrix(p(a), a.shape[0], p(b), b.shape[0], a.shape[1], 1 if sym else 0, p(out), p(status),
                                          hip.current_stream()), 'es_emd_matrix')
    return out, status


def _raise_on_status(who, out, *status):
    """out, unless a pair of one of the status matrices is flagged"""
    for st in status:
        st = st.cpu().numpy()
        for code, what in ((2, 'have a coordinate that is not finite (or span 2^61 or more)'),
                           (1, 'reached the cap on bidding rounds (no result; please report the clouds)')):
            pairs = np.argwhere(st == code)
            if len(pairs):
                raise RuntimeError('%s: pairs %s %s' % (who, [tuple(int(v) for v in ij) for ij in pairs[:8]] + (['...'] if len(pairs) > 8 else []), what))
    return out


# ---------------------------------------------------------------------------------------------- the N x N bookkeeping, on the host
def _mmd_cov(d):
    """d [N_sample, N_ref] numpy -> (mmd, cov, mmd_smp): the mean over the references of the distance to their nearest sample, the
    fraction of references that are the nearest reference of some sample (first index wins a tie), the mean over the samples of the
    distance to their nearest reference.  Means in double."""
    nearest_ref = d.argmin(axis=1)                                  # (numpy: the first minimum)
    return d.min(axis=0).mean(dtype=np.float64), np.unique(nearest_ref).size / float(d.shape[1]), d.min(axis=1).mean(dtype=np.float64)


def _knn(xx, xy, yy, k, sqrt=False):
    """The k-NN two-sample test on the block matrix [[xx, xy], [xy^T, yy]] with the diagonal excluded: set x carries label 1, an element
    is predicted 1 when at least k / 2 of its k nearest neighbours carry label 1.  Neighbours in order of distance, first index first
    among equals.  Returns a dict of floats."""
    n0, n1 = xx.shape[0], yy.shape[0]
    m = np.concatenate([np.concatenate([xx, xy], 1), np.concatenate([xy.T, yy], 1)], 0).astype(np.float64)
    if sqrt:
        m = np.sqrt(np.abs(m))
    np.fill_diagonal(m, np.inf)
    label = np.concatenate([np.ones(n0), np.zeros(n1)])
    nn = np.argsort(m, axis=0, kind='stable')[:k]                   # [k, n0 + n1]: the neighbours of each column
    pred = (label[nn].sum(0) >= k / 2.0).astype(np.float64)
    tp, fp = (pred * label).sum(), (pred * (1 - label)).sum()
    fn, tn = ((1 - pred) * label).sum(), ((1 - pred) * (1 - label)).sum()
    f = np.float32                                                  # (the reference's quotients are float32)
    return {'tp': f(tp), 'fp': f(fp), 'fn': f(fn), 'tn': f(tn),
            'precision': f(tp) / (f(tp) + f(fp) + f(1e-10)), 'recall': f(tp) / (f(tp) + f(fn) + f(1e-10)),
            'acc_t': f(tp) / (f(tp) + f(fn) + f(1e-10)), 'acc_f': f(tn) / (f(tn) + f(fp) + f(1e-10)),
            'acc': (pred == label).astype(np.float32).mean(dtype=np.float32)}


def _matrix(x, who, name, square=False):
    if not (torch.is_tensor(x) and x.is_floating_point() and x.dim() == 2 and x.shape[0] > 0 and x.shape[1] > 0):
        raise ValueError('%s: %s must be a floating-point matrix [N, M] with N, M >= 1' % (who, name))
    if square and x.shape[0] != x.shape[1]:
        raise ValueError('%s: %s must be square, got %s' % (who, name, tuple(x.shape)))
    return x.detach().cpu().numpy()


def _scalars(d, like):
    return {k: torch.tensor(float(v), dtype=torch.float32, device=like.device) for k, v in d.items()}


def lgan_mmd_cov(all_dist):
    """``all_dist`` [N_sample, N_ref] -> {'lgan_mmd', 'lgan_cov', 'lgan_mmd_smp'} as 0-dim float32 tensors on its device (see _mmd_cov)."""
    mmd, cov, mmd_smp = _mmd_cov(_matrix(all_dist, 'lgan_mmd_cov', 'all_dist'))
    return _scalars({'lgan_mmd': mmd, 'lgan_cov': cov, 'lgan_mmd_smp': mmd_smp}, all_dist)


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """The k-NN two-sample test of the reference: {'tp', 'fp', 'fn', 'tn', 'precision', 'recall', 'acc_t', 'acc_f', 'acc'} as 0-dim
    float32 tensors on the device of ``Mxx`` (see _knn)."""
    xx, yy = _matrix(Mxx, 'knn', 'Mxx', True), _matrix(Myy, 'knn', 'Myy', True)
    xy = _matrix(Mxy, 'knn', 'Mxy')
    if xy.shape != (xx.shape[0], yy.shape[0]):
        raise ValueError('knn: Mxy must be [%d, %d], got %s' % (xx.shape[0], yy.shape[0], xy.shape))
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k < xx.shape[0] + yy.shape[0]:
        raise ValueError('knn: k must be an integer in [1, %d), got %r' % (xx.shape[0] + yy.shape[0], k))
    return _scalars(_knn(xx, xy, yy, int(k), sqrt), Mxx)


def metrics_from_matrices(M_rs, M_rr, M_ss):
    """The six CD entries of ``compute_all_metrics`` from the three matrices (numpy, on the host): M_rs [N_ref, N_sample], M_rr, M_ss."""
    mmd, cov, mmd_smp = _mmd_cov(np.ascontiguousarray(M_rs.T))
    nn1 = _knn(M_rr, M_rs, M_ss, 1)
    return dict(zip(_CD_KEYS, (mmd, cov, mmd_smp, nn1['acc_t'], nn1['acc_f'], nn1['acc'])))


def emd_metrics_from_matrices(M_rs, M_rr, M_ss):
    """The six EMD entries of ``compute_all_metrics`` from the three EMD matrices: the same statistics under the reference's EMD keys."""
    return dict(zip(_EMD_KEYS, metrics_from_matrices(M_rs, M_rr, M_ss).values()))


def _three(M_rs, M_rr, M_ss):
    """the three device matrices as numpy after one copy"""
    nr, ns = M_rr.shape[0], M_ss.shape[0]
    host = torch.cat([M_rs.flatten(), M_rr.flatten(), M_ss.flatten()]).cpu().numpy()
    return (host[:nr * ns].reshape(nr, ns), host[nr * ns:nr * ns + nr * nr].reshape(nr, nr), host[nr * ns + nr * nr:].reshape(ns, ns))


def compute_all_metrics(sample_pcs, ref_pcs, batch_size=None, accelerated_cd=True, emd=False):
    """MMD-CD, COV-CD and the 1-NN accuracy (CD) of a set of generated clouds [N_sample, P, 3] against a set of reference clouds
    [N_ref, Q, 3], as the reference's ``compute_all_metrics``: {'lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t',
    '1-NN-CD-acc_f', '1-NN-CD-acc'}, 0-dim float32 tensors on the clouds' device.  The three matrices M_rs, M_rr, M_ss come from
    ``pairwise_chamfer`` (the last two in its symmetric mode); the statistics run on the host after one copy.

    ``emd=True`` (Q must equal P, at most ``EMD_MAX_POINTS``) returns the reference's twelve keys in its order: the three ``lgan_*-CD``,
    the three ``lgan_*-EMD``, the three ``1-NN-CD-*``, the three ``1-NN-EMD-*``; the EMD entries are the same statistics of the three
    matrices of ``pairwise_emd``.  ``batch_size`` and ``accelerated_cd`` are accepted and ignored: the matrix kernels need no
    batching and are the only route."""
    _check_sets('compute_all_metrics', True, emd=bool(emd), sample_pcs=sample_pcs, ref_pcs=ref_pcs)
    cd = metrics_from_matrices(*_three(_chamfer_matrix(ref_pcs, sample_pcs), _chamfer_matrix(ref_pcs, None), _chamfer_matrix(sample_pcs, None)))
    if not emd:
        return _scalars(cd, sample_pcs)
    (E_rs, s_rs), (E_rr, s_rr), (E_ss, s_ss) = _emd_matrix(ref_pcs, sample_pcs), _emd_matrix(ref_pcs, None), _emd_matrix(sample_pcs, None)
    _raise_on_status('compute_all_metrics (ref x sample)', E_rs, s_rs)
    _raise_on_status('compute_all_metrics (ref x ref)', E_rr, s_rr)
    _raise_on_status('compute_all_metrics (sample x sample)', E_ss, s_ss)
    em = emd_metrics_from_matrices(*_three(E_rs, E_rr, E_ss))
    both = list(cd.items())[:3] + list(em.items())[:3] + list(cd.items())[3:] + list(em.items())[3:]
    return _scalars(dict(both), sample_pcs)
