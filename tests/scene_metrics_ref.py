"""Host yardsticks and seeded cases of the scene-metric tests (echoscene_amd/scene_metrics.py, csrc/es_scene_metrics.hip).

Three things, all numpy / pure Python:
  * a restatement of the fit and of the overlap count in the arithmetic the kernels promise: float32 arrays, one rounding per
    operation, the fit per axis in the stated order (size = max - min, p / size * box[:3], the rotation, + box[3:6]; the radians by
    numpy's deg2rad on a float32, the cosine and sine evaluated in double and rounded once), distances dx*dx + dy*dy + dz*dz summed in
    that order, the strict rule (``fit``, ``self_nn``, ``overlap_pair``, ``overlap_counts``);
  * a float64 yardstick: the same fit and the distances in double on the float32 inputs (``fit64``), and the distance of every query
    point's verdict from a tie, |dist12 - dist11| in Euclidean metres (``margins``);
  * the case builders that the golden generator (tests/golden/make_golden_scene_overlap.py) and the tests share (``CASES``, ``case``).
    Inputs are rebuilt from their seeds; nothing but the reference's outputs is stored.

A box row is (size x, y, z, centre x, y, z, angle in degrees)."""
import math

import numpy as np

F = np.float32
OBJ_NAMES = ('_scene_', 'floor', 'wall', 'ceiling', 'bed', 'table', 'chair', 'sofa', 'lamp', 'shelf', 'wardrobe', 'nightstand')
PRED_NAMES = ('none', 'left', 'right', 'front', 'behind', 'close by', 'inside', 'attached to', 'standing on', 'bigger than', 'cover')
# every name ends in the newline of a vocabulary file
VOCAB = {'object_idx_to_name': [n + '\n' for n in OBJ_NAMES], 'pred_idx_to_name': [n + '\n' for n in PRED_NAMES]}
STRUCTURAL = ('floor', 'wall', 'ceiling', '_scene_')
TOUCHING = ('none', 'inside', 'attached to', 'part of', 'cover', 'belonging to', 'build in', 'connected to')
# the least |dist12 - dist11| (metres, on the yardstick) that the generator accepts for a query point of a recorded pair; it asserts
# MARGIN >= 8 x the coordinate bar (the bar is 4 x the reference's own fit error; 2 sqrt(3) bars per distance, two distances)
MARGIN = 2e-5
OBJ = {n: i for i, n in enumerate(OBJ_NAMES)}
PRED = {n: i for i, n in enumerate(PRED_NAMES)}


# ------------------------------------------------------------------------------------------------ the restatement
def _axes(up):
    return (0, 1) if up == 'z' else (0, 2)


def fit(box, cloud, withangle=True, up='z'):
    """one object: box [7] or [6], cloud [P, 3] -> the placed cloud, float32, every operation rounded to float32 on its own"""
    box, cloud = np.asarray(box, F), np.asarray(cloud, F)
    size = cloud.max(0) - cloud.min(0)
    with np.errstate(all='ignore'):
        v = cloud / size * box[:3]
    if withangle:
        rad = np.deg2rad(F(box[6]))
        assert rad.dtype == F
        c, s = F(math.cos(float(rad))), F(math.sin(float(rad)))
        a, b = _axes(up)
        va, vb = v[:, a].copy(), v[:, b].copy()
        v[:, a] = c * va - s * vb
        v[:, b] = s * va + c * vb
    v = v + box[3:6]
    assert v.dtype == F
    return v


def fit_all(boxes, clouds, withangle=True, up='z'):
    return np.stack([fit(b, c, withangle, up) for b, c in zip(boxes, clouds)])


def fit64(box, cloud, withangle=True, up='z'):
    """the yardstick: the same fit in float64 on the float32 inputs"""
    box, cloud = np.asarray(box, F).astype(np.float64), np.asarray(cloud, F).astype(np.float64)
    v = cloud / (cloud.max(0) - cloud.min(0)) * box[:3]
    if withangle:
        rad = np.deg2rad(box[6])
        c, s = math.cos(rad), math.sin(rad)
        a, b = _axes(up)
        va, vb = v[:, a].copy(), v[:, b].copy()
        v[:, a] = c * va - s * vb
        v[:, b] = s * va + c * vb
    return v + box[3:6]


def fit64_all(boxes, clouds, withangle=True, up='z'):
    return np.stack([fit64(b, c, withangle, up) for b, c in zip(boxes, clouds)])


def _sq(q, c, rows=256):
    """squared distances [len(q), len(c)] in the dtype of q: ((dx*dx + dy*dy) + dz*dz), yielded in blocks of query rows"""
    for r in range(0, len(q), rows):
        d = c[None, :, :] - q[r:r + rows, None, :]
        d = d * d
        yield r, (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]


def self_nn(pc):
    """the squared distance from each point to the nearest point of another index; +inf for one point"""
    out = np.full(len(pc), np.inf, pc.dtype)
    for r, d in _sq(pc, pc):
        d[np.arange(len(d)), r + np.arange(len(d))] = np.inf
        out[r:r + len(d)] = d.min(1)
    return out


def cross_nn(pc1, pc2):
    out = np.empty(len(pc1), pc1.dtype)
    for r, d in _sq(pc1, pc2):
        out[r:r + len(d)] = d.min(1)
    return out


def overlap_pair(pc1, pc2):
    """the strict rule on two placed float32 clouds: points of pc1 whose nearest point of pc2 is strictly nearer than their nearest
    other point of pc1"""
    pc1, pc2 = np.ascontiguousarray(pc1, F), np.ascontiguousarray(pc2, F)
    return int((cross_nn(pc1, pc2) < self_nn(pc1)).sum())


def overlap_counts(placed, pairs):
    return [overlap_pair(placed[i], placed[j]) for i, j in np.asarray(pairs).reshape(-1, 2).tolist()]


def margins(placed64, pairs):
    """per pair: the count on the yardstick and the least |dist12 - dist11| over the query points (Euclidean)"""
    out = []
    for i, j in np.asarray(pairs).reshape(-1, 2).tolist():
        d11, d12 = np.sqrt(self_nn(placed64[i])), np.sqrt(cross_nn(placed64[i], placed64[j]))
        out.append((int((d12 < d11).sum()), float(np.abs(d12 - d11).min())))
    return out


def eligible_pairs(objs, triples, vocab=VOCAB, offsets=None):
    """the reference's selection, scene by scene: (pairs int32 [K, 2], {rule: pairs skipped by it})"""
    onames, pnames = vocab['object_idx_to_name'], vocab['pred_idx_to_name']
    offsets = [0, len(objs)] if offsets is None else list(offsets)
    pair2pred = {}
    for s, p, o in np.asarray(triples).reshape(-1, 3).tolist():
        pair2pred[(s, o)] = p
    out, skipped = [], {'structural': 0, 'stated': 0, 'reverse': 0}
    for lo, hi in zip(offsets, offsets[1:]):
        for i in range(lo, hi - 1):
            for j in range(i + 1, hi):
                if onames[objs[i]].split('\n')[0] in STRUCTURAL or onames[objs[j]].split('\n')[0] in STRUCTURAL:
                    skipped['structural'] += 1
                elif (i, j) in pair2pred and pnames[pair2pred[(i, j)]].split('\n')[0] in TOUCHING:
                    skipped['stated'] += 1
                elif (j, i) in pair2pred and pnames[pair2pred[(j, i)]].split('\n')[0] in TOUCHING:
                    skipped['reverse'] += 1
                else:
                    out.append((i, j))
    return np.array(out, np.int32).reshape(-1, 2), skipped


# ------------------------------------------------------------------------------------------------ the cases
def raw_cloud(rs, P):
    """a shape as the point sampler leaves it: P points in an arbitrary frame, an L of two slabs so that bounds say little"""
    ext = rs.uniform(0.3, 1.0, 3)
    pts = rs.uniform(-0.5, 0.5, (P, 3))
    leg = rs.rand(P) < 0.5
    pts[leg, 0] = 0.5 - 0.3 * rs.rand(int(leg.sum()))                  # one slab along x = +0.5, the rest fills the volume thinly
    return (pts * ext + rs.uniform(-0.2, 0.2, 3)).astype(F)


def _graph(O):
    """O >= 6 nodes: floor first, _scene_ last, furniture between; an `inside` triple, a `none` triple stated in the reverse direction
    and one (s, o) given twice with the later triple deciding -> every skip rule of the reference takes a pair"""
    objs = np.array([OBJ['floor']] + [OBJ[n] for n in ('bed', 'table', 'chair', 'sofa', 'lamp', 'shelf', 'wardrobe')][:O - 2] + [OBJ['_scene_']],
                    np.int64)
    t = [(1, PRED['inside'], 2),                                        # skips (1, 2) as stated
         (4, PRED['none'], 3),                                          # skips (3, 4) through the reverse direction
         (1, PRED['inside'], 3), (1, PRED['left'], 3),                  # the later triple decides: (1, 3) is judged
         (2, PRED['front'], 4), (2, PRED['close by'], 3), (0, PRED['behind'], 1), (1, PRED['standing on'], 0)]
    t += [(k, PRED['left'], O - 1) for k in range(O - 1)]
    return objs, np.array(t, np.int64)


def _scene(seed, O, P, spread, size=(0.5, 1.2), angle=180.0):
    rs = np.random.RandomState(seed)
    clouds = np.stack([raw_cloud(rs, P) for _ in range(O)])
    boxes = np.concatenate([rs.uniform(size[0], size[1], (O, 3)), spread(rs, O), rs.uniform(-angle, angle, (O, 1))], 1).astype(F)
    objs, triples = _graph(O)
    return dict(clouds=clouds, boxes=boxes, objs=objs, triples=triples, offsets=[0, O], placed=False, seven=False)


def _near(rs, O):
    return rs.uniform(-0.45, 0.45, (O, 3))


def _far(rs, O):
    grid = np.array([(x, y, 0.0) for x in (-2.6, 0.0, 2.6) for y in (-1.5, 1.5)])[:O]
    return grid + rs.uniform(-0.1, 0.1, (O, 3))


def _case_room(seed):
    return _scene(seed, 6, 257, _near)


def _case_apart(seed):
    return _scene(seed, 6, 257, _far, size=(0.4, 0.9))                  # half diagonals below 0.78, centres at least 2.4 apart on an axis


def _case_nested(seed):
    c = _scene(seed, 6, 257, _near)
    c['clouds'][3] = c['clouds'][1]                                     # object 3: the shape of object 1 in a box 0.97 times the size
    c['boxes'][3] = c['boxes'][1]
    c['boxes'][3, :3] *= F(0.97)
    return c


def _case_p1(seed):
    """one point per cloud: the fit is undefined (no extent), so the clouds are given placed and the reference is asked pair by pair"""
    rs = np.random.RandomState(seed)
    objs, triples = _graph(6)
    return dict(clouds=rs.uniform(-1, 1, (6, 1, 3)).astype(F), boxes=None, objs=objs, triples=triples, offsets=[0, 6], placed=True, seven=False)


def _case_flat7(seed):
    c = _scene(seed, 6, 257, _near, angle=400.0)
    c['boxes'][1, 6], c['boxes'][4, 6] = F(271.5), F(-385.25)          # beyond +-180 whatever the seed
    c['seven'] = True                                                   # the calls get boxes[:, :6] (a row stride of 7) and boxes[:, 6]
    return c


def _case_batch(seed):
    a, b = _scene(seed, 6, 257, _near), _scene(seed + 1000, 7, 257, _near)
    return dict(clouds=np.concatenate([a['clouds'], b['clouds']]), boxes=np.concatenate([a['boxes'], b['boxes']]),
                objs=np.concatenate([a['objs'], b['objs']]), triples=np.concatenate([a['triples'], b['triples'] + np.array([6, 0, 6])]),
                offsets=[0, 6, 13], placed=False, seven=False)


# name -> (builder, seed); a seed that fails the generator's margin is replaced by the next one that passes
CASES = {'room': (_case_room, 11), 'apart': (_case_apart, 12), 'nested': (_case_nested, 13), 'p1': (_case_p1, 14),
         'flat7': (_case_flat7, 15), 'batch': (_case_batch, 16)}
_built = {}


def case(name):
    """the case, built once per process; treat it as read-only"""
    if name not in _built:
        builder, seed = CASES[name]
        _built[name] = builder(seed)
    return _built[name]


def scenes(c):
    """the scenes of a case as (node slice, triples with local indices)"""
    out = []
    for lo, hi in zip(c['offsets'], c['offsets'][1:]):
        t = c['triples'][(c['triples'][:, 0] >= lo) & (c['triples'][:, 0] < hi)]
        out.append((slice(lo, hi), t - np.array([lo, 0, lo])))
    return out


def swap_yz(c):
    """the same scene with the y and z columns of clouds and boxes swapped: up='y' on it is up='z' on the original"""
    return dict(c, clouds=np.ascontiguousarray(c['clouds'][:, :, [0, 2, 1]]), boxes=np.ascontiguousarray(c['boxes'][:, [0, 2, 1, 3, 5, 4, 6]]))


def placed_of(c, up='z', yardstick=False):
    if c['placed']:
        return c['clouds'].astype(np.float64) if yardstick else c['clouds']
    return (fit64_all if yardstick else fit_all)(c['boxes'], c['clouds'], True, up)


def expected_counts(c, up='z'):
    """the restatement's list for the case, in the reference's order"""
    pairs, _ = eligible_pairs(c['objs'], c['triples'], VOCAB, c['offsets'])
    return overlap_counts(placed_of(c, up), pairs)


def lattice(n, offset=(0, 0, 0), step=1):
    """the n^3 integer lattice as a float32 cloud: every distance is exact"""
    g = np.arange(n) * step
    return (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + np.array(offset)).astype(F)


def staircase_pair(seed, P):
    """two placed clouds whose bounds overlap and which do not touch: points under and over the diagonal x = y, 0.4 apart"""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(0, 2, (P, 3)), rs.uniform(0, 2, (P, 3))
    a[:, 1] = a[:, 0] * rs.uniform(0, 1, P) - 0.2                       # y <= x - 0.2
    b[:, 1] = b[:, 0] + (2 - b[:, 0]) * rs.uniform(0, 1, P) + 0.2       # y >= x + 0.2
    return a.astype(F), b.astype(F)
