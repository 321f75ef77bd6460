"""The yardstick of the earth mover's distance tests (echoscene_amd/shape_metrics.py ``pairwise_emd``, csrc/es_emd.hip) and a numpy
restatement of the kernel's auction.

Yardstick: ``emd_pair`` / ``emd_matrix`` -- Euclidean distances from direct differences in float64 and the exact assignment of
``scipy.optimize.linear_sum_assignment``; the value is mean_p |x_p - y_sigma(p)| of the optimal one-to-one matching sigma, the
definition of the reference's ``emd_approx``.

Restatement: ``auction(x, y) -> (value, rounds, bids)`` is the algorithm of csrc/es_emd.hip step by step, in the same integer
arithmetic and with the same tie rules, so that it returns the kernel's bits and the kernel's round count:

  scale   e = max(3, k + 1) with 2^(k-1) <= m < 2^k, m the largest fp32 extent of the joint bounding box: every distance is < 2^e
  cost    c_ij = rint(fl32(sqrt(fl32(fl32(dx^2 + dy^2) + dz^2))) * 2^(23 - e)), an integer <= 2^23, from fp32 differences; no fma
  phases  eps = max(1, cmax // 2), then max(1, eps // 5) down to 1; prices carry over, the assignment starts empty in each phase
  round   (Jacobi) every unassigned bidder i takes w_j = c_ij + price_j, the smallest w (lowest j among equals) and the smallest of
          the others, and bids inc = w2 - w1 + eps on j1; per object the largest inc wins, the lowest bidder among equals; the winner
          replaces the owner and the price rises by inc
  value   sum_j c(owner_j, j) * 2^(e - 23) / P in double, rounded to float32
  cap     ``round_cap(P, cmax)``: CAP_MULT * P + CAP_ADD rounds per phase, CAP_TOTAL_MULT * P + CAP_ADD over all phases (see the kernel's
          header for their origin)"""
import numpy as np

EMD_EPS = 4e-6             # the kernel's guarantee at scale e = 3 (distances below 8): derived in csrc/es_emd.hip
COST_BITS = 23             # scaled costs are integers in [0, 2^23]
MIN_SCALE_EXP = 3
MAX_SCALE_EXP = 62
THETA = 5
CAP_MULT, CAP_TOTAL_MULT, CAP_ADD = 128, 512, 4096
WAVE, BLOCK = 64, 1024     # the kernel's seams: the objects a wave scans per step, the threads of a workgroup


def pair_dists(x, y):
    """[P, P] float64 Euclidean distances from direct differences"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = np.zeros((x.shape[0], y.shape[0]))
    for c in range(3):
        d += (x[:, c, None] - y[None, :, c]) ** 2
    return np.sqrt(d)


def emd_pair(x, y):
    from scipy.optimize import linear_sum_assignment
    assert len(x) == len(y)
    d = pair_dists(x, y)
    r, c = linear_sum_assignment(d)
    return d[r, c].mean()


def emd_matrix(a, b=None):
    """float64 [Na, Nb]; a, b: sequences of [P, 3] clouds (b None: a against itself, every entry computed)"""
    b = a if b is None else b
    return np.array([[emd_pair(x, y) for y in b] for x in a])


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def scale_exponent(x, y):
    """e of the two fp32 clouds, or None when a coordinate is not finite or the extent is 2^61 or more (the kernel's status 2)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return None
    lo = np.minimum(x.min(0), y.min(0))
    hi = np.maximum(x.max(0), y.max(0))
    with np.errstate(over='ignore'):
        m = np.float32((hi - lo).max())                             # fp32 subtraction, as on the device
    if not np.isfinite(m):
        return None
    bits = int(np.float32(m).view(np.uint32))
    k = ((bits >> 23) & 0xff) - 126                                 # m < 2^k (zero and denormals: -126)
    e = max(MIN_SCALE_EXP, k + 1)
    return None if e > MAX_SCALE_EXP else e


def int_costs(x, y, e):
    """[P, P] int64: the kernel's scaled integer costs"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    dx = x[:, None, 0] - y[None, :, 0]
    dy = x[:, None, 1] - y[None, :, 1]
    dz = x[:, None, 2] - y[None, :, 2]
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)                      # float32 throughout, one rounding per operation
    assert d.dtype == np.float32
    return np.rint(d * np.float32(2.0 ** (COST_BITS - e))).astype(np.int64)


def eps_schedule(cmax):
    eps = [max(1, int(cmax) // 2)]
    while eps[-1] > 1:
        eps.append(max(1, eps[-1] // THETA))
    return eps


def round_cap(P, cmax):
    """(rounds per phase, rounds in total) at which the kernel gives up"""
    per = CAP_MULT * P + CAP_ADD
    return per, min(per * len(eps_schedule(cmax)), CAP_TOTAL_MULT * P + CAP_ADD)


def price_bound(cmax):
    """no price exceeds this (see the kernel's header): 2 * phases * (cmax + eps_0); must stay below 2^31"""
    sch = eps_schedule(cmax)
    return 2 * len(sch) * (int(cmax) + sch[0])


def auction(x, y, detail=False):
    """(float32 value, rounds, bids) of the kernel's auction on the fp32 clouds x, y [P, 3]; (nan, 0, 0) for its status 2.
    ``detail``: also the rounds per phase and the largest price"""
    n = len(x)
    assert len(y) == n
    e = scale_exponent(x, y)
    if e is None:
        return (np.float32(np.nan), 0, 0) + (([], 0) if detail else ())
    c = int_costs(x, y, e)
    price = np.zeros(n, np.int64)
    owner = -np.ones(n, np.int64)
    rounds = bids = 0
    per_phase = []
    if n == 1:
        owner[0] = 0
    else:
        for eps in eps_schedule(c.max()):
            owner[:] = -1
            has = np.zeros(n, bool)
            r0 = rounds
            while True:
                un = np.nonzero(~has)[0]
                if len(un) == 0:
                    break
                rounds += 1
                bids += len(un)
                w = c[un] + price[None, :]
                rows = np.arange(len(un))
                j1 = w.argmin(1)                                    # (numpy: the first minimum)
                w1 = w[rows, j1]
                w[rows, j1] = np.iinfo(np.int64).max
                inc = w.min(1) - w1 + eps
                order = np.lexsort((un, -inc, j1))                  # per object: the largest inc first, then the lowest bidder
                objs, first = np.unique(j1[order], return_index=True)
                win = order[first]
                old = owner[objs]
                has[old[old >= 0]] = False
                owner[objs] = un[win]
                has[un[win]] = True
                price[objs] += inc[win]
            per_phase.append(rounds - r0)
    total = int(c[owner, np.arange(n)].sum())
    value = np.float32(float(total) * 2.0 ** (e - COST_BITS) / n)
    return (value, rounds, bids) + ((per_phase, int(price.max())) if detail else ())


# ------------------------------------------------------------------------------------------------ clouds of the tests
MATRIX_P = (1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def matrix_case(P):
    """(a [Na, P, 3], b [Nb, P, 3]) of shape_metrics_ref.clouds; (Na, Nb) runs over {1, 2, 3}^2 with P; from P = 1023 on, where the host solver takes
    0.6 s per pair, one or two pairs"""
    import shape_metrics_ref as R
    k = MATRIX_P.index(P)
    Na, Nb = ((1, 1 + (P == 1025)) if P >= 1023 else (1 + k % 3, 1 + (k // 3 + k) % 3))
    return R.clouds(3000 + P, Na, P), R.clouds(3100 + P, Nb, P)


def translate_case(P, seed=3):
    """a lattice cloud (multiples of 1/64 in [-0.75, 0.75]^3) and a permuted translate of it by t = (3, 4, 0) / 64: for any translate
    the identity matching is optimal, sum |x_i - y_sigma(i)| >= |sum (x_i - y_sigma(i))| = P |t|, so the EMD is |t| = 5/64 exactly"""
    rs = np.random.RandomState(seed + P)
    a = rs.randint(-48, 49, size=(P, 3)) / 64.0
    b = (a + np.array([3, 4, 0]) / 64.0)[rs.permutation(P)]
    return a.astype(np.float32), b.astype(np.float32)


def adversarial_cases(P=257):
    """clouds that are hard on an auction: many exact ties.  {name: (x, y)} float32 [P, 3]"""
    import shape_metrics_ref as R
    rs = np.random.RandomState(1)
    a40, b40 = R.clouds(9, 1, 40)[0], R.clouds(10, 1, 40)[0]
    dup_a, dup_b = a40[rs.randint(0, 40, P)], b40[rs.randint(0, 40, P)]            # what sample_indices yields for a small mesh
    spread = R.clouds(11, 1, P)[0]
    point = np.tile(np.float32([0.25, -0.5, 0.125]), (P, 1))
    return {'duplicates': (dup_a, dup_b), 'self': (spread, spread.copy()), 'coincident': (point, point.copy()),
            'coincident_vs_spread': (point, spread), 'spread_vs_coincident': (spread, point)}
