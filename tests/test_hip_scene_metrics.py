"""GPU tests of the scene metric: the fit, self-distance and pair kernels (csrc/es_scene_metrics.hip) behind
echoscene_amd/scene_metrics.py, against what the reference recorded (tests/golden/scene_overlap.npz, written by
tests/golden/make_golden_scene_overlap.py), the numpy restatement and the float64 yardstick of tests/scene_metrics_ref.py.

Counts are compared exactly: the generator asserted, on the yardstick, that every query point of every recorded pair is at least
MARGIN = 2e-5 m from a tie (least margin found: 2.96e-4), which is more than 8 x the coordinate bar.  The bar of a fitted coordinate is
measured on the reference: ``ref_fit_err`` = 1.78e-07 over the recorded fits, times 4 for another order of the same operations (the
precedent of test_hip_shape_metrics.py and test_hip_layout_metrics.py) -> BAR = 7.11e-07, read from the golden file.  The kernel's
fit is asserted to be the restatement's bit for bit (the cosine and sine are the correctly rounded fp32 values on both sides); the
figures measured on an MI355X are in profiles/scene_overlap_notes.md."""
import os

import numpy as np
import pytest
import torch

import scene_metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def M():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import scene_metrics
    return scene_metrics


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'scene_overlap.npz')))


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def drop_in(M, c, nodes=slice(None), triples=None, up='z', as_list=False, metric=None):
    """the reference's call on one scene of a case; the 7-column case hands over boxes[:, :6] (a row stride of 7) and boxes[:, 6]"""
    boxes = dev(c['boxes'][nodes])
    six = boxes[:, :6] if c['seven'] else boxes[:, :6].contiguous()
    clouds = dev(c['clouds'][nodes])
    return M.pointcloud_overlap(list(clouds) if as_list else clouds, dev(c['objs'][nodes]), six, boxes[:, 6],
                                dev(c['triples'] if triples is None else triples), R.VOCAB, [] if metric is None else metric, up=up)


def pairs_of(c):
    return R.eligible_pairs(c['objs'], c['triples'], R.VOCAB, c['offsets'])[0]


# ------------------------------------------------------------------------------------------------ the recorded counts
@pytest.mark.parametrize('name', list(R.CASES))
def test_drop_in_counts_are_the_recorded_ones(M, G, name):
    c = R.case(name)
    want = G[name + '/counts'].tolist()
    if c['placed']:                                                 # one point per cloud: the reference was asked pair by pair
        got = [M.pointcloud_overlap_pair(dev(c['clouds'][i]), dev(c['clouds'][j])) for i, j in pairs_of(c).tolist()]
        assert got == want and all(type(v) is int for v in got)
        assert host(M.overlap_counts(dev(c['clouds']), None, dev(pairs_of(c)), fitted=True)).tolist() == want
        return
    got = []
    for nodes, triples in R.scenes(c):
        before = len(got)
        assert drop_in(M, c, nodes, triples, metric=got) is got and len(got) > before
    assert got == want and all(type(v) is int for v in got)
    if len(c['offsets']) == 2:
        assert drop_in(M, c, as_list=True) == want                 # a list of O clouds [P, 3]


def test_batch_in_one_call_is_the_scenes_one_by_one(M, G):
    c = R.case('batch')
    pairs = M.eligible_pairs(c['objs'], c['triples'], R.VOCAB, offsets=c['offsets'])
    out = M.overlap_counts(dev(c['clouds']), dev(c['boxes']), pairs.cuda())
    assert out.dtype == torch.int32 and out.is_cuda and out.shape == (len(pairs),)
    one_by_one = []
    for nodes, triples in R.scenes(c):
        local = M.eligible_pairs(c['objs'][nodes], triples, R.VOCAB)
        one_by_one += host(M.overlap_counts(dev(c['clouds'][nodes]), dev(c['boxes'][nodes]), local.cuda())).tolist()
    assert host(out).tolist() == one_by_one == G['batch/counts'].tolist()


def test_no_eligible_pair_returns_the_list_untouched(M):
    c = R.case('room')
    metric = [7]
    assert M.pointcloud_overlap(dev(c['clouds'][:2]), dev(np.array([R.OBJ['floor'], R.OBJ['bed']])), dev(c['boxes'][:2, :6]), dev(c['boxes'][:2, 6]),
                                dev(c['triples'][:0]), R.VOCAB, metric) is metric and metric == [7]
    assert M.overlap_counts(dev(c['clouds']), dev(c['boxes']), torch.zeros(0, 2, dtype=torch.int32, device='cuda')).shape == (0,)


# ------------------------------------------------------------------------------------------------ the fit
def test_fit_against_yardstick_and_restatement(M, G):
    bar = 4 * float(G['ref_fit_err'])
    worst = worst_ref = 0.0
    same = True
    for name in R.CASES:
        c = R.case(name)
        if c['placed']:
            continue
        for up, cc in (('z', c), ('y', R.swap_yz(c))):
            got = M.fit_shapes_to_box(dev(cc['boxes']), dev(cc['clouds']), up=up)
            assert got.dtype == torch.float32 and got.is_cuda and got.shape == cc['clouds'].shape
            got = host(got)
            worst = max(worst, float(np.abs(got - R.fit64_all(cc['boxes'], cc['clouds'], True, up)).max()))
            same &= np.array_equal(got, R.fit_all(cc['boxes'], cc['clouds'], True, up))
            if up == 'z':
                worst_ref = max(worst_ref, float(np.abs(got - G[name + '/fit']).max()))
    print('fit: %.3g from the yardstick (bar %.3g), %.3g from the reference; the restatement bit for bit: %s' % (worst, bar, worst_ref, same))
    assert bar > 0 and worst <= bar
    assert same                                                     # the same IEEE operations in the same order, nothing fused


def test_fit_call_shapes(M):
    c = R.case('room')
    boxes, clouds = dev(c['boxes']), dev(c['clouds'])
    want = M.fit_shapes_to_box(boxes, clouds)
    one = M.fit_shapes_to_box(boxes[2], clouds[2])                  # one object: [7] and [P, 3]
    assert one.shape == clouds[2].shape and torch.equal(one, want[2])
    wide = torch.zeros(6, 9, device='cuda')
    wide[:, :7] = boxes
    assert torch.equal(M.fit_shapes_to_box(wide[:, :7], clouds), want)                                 # a row stride of 9
    flat = M.fit_shapes_to_box(boxes[:, :6], clouds, withangle=False)
    assert np.array_equal(host(flat), R.fit_all(c['boxes'], c['clouds'], False))
    assert torch.equal(M.fit_shapes_to_box(boxes, clouds, withangle=False), flat)                      # the angle column is not read
    assert torch.equal(M.fit_shapes_to_box(boxes[1, :6], clouds[1], withangle=False), flat[1])


# ------------------------------------------------------------------------------------------------ the kernels' own boundaries
@pytest.mark.parametrize('P', [1, 63, 257, 2049])
def test_point_counts_around_the_kernels_boundaries(M, P):
    """placed clouds, O = 3: one point, less than a wave, workgroup size + 1, LDS tile + 1"""
    rs = np.random.RandomState(P)
    clouds = (rs.uniform(-0.5, 0.5, (3, P, 3)) + rs.uniform(-0.15, 0.15, (3, 1, 3))).astype(np.float32)
    pairs = np.array([(i, j) for i in range(3) for j in range(3)], np.int32)
    want = R.overlap_counts(clouds, pairs)
    assert P == 1 or 0 < want[1] < P
    assert want[0] == want[4] == want[8] == P
    assert host(M.overlap_counts(dev(clouds), None, dev(pairs), fitted=True)).tolist() == want
    assert M.pointcloud_overlap_pair(dev(clouds[0]), dev(clouds[1])) == want[1]


def test_unequal_point_counts_in_the_pair_call(M):
    rs = np.random.RandomState(3)
    a, b = rs.uniform(0, 1, (300, 3)).astype(np.float32), rs.uniform(0.2, 1.2, (2100, 3)).astype(np.float32)
    assert M.pointcloud_overlap_pair(dev(a), dev(b)) == R.overlap_pair(a, b) > 0
    assert M.pointcloud_overlap_pair(dev(b), dev(a)) == R.overlap_pair(b, a) > 0
    assert M.pointcloud_overlap_pair(dev(a[:1]), dev(b)) == 1       # one point has no other point: it counts


def test_exact_ties_on_integer_lattices(M):
    """every distance is an exact integer; the reference is undefined here, the rule is not"""
    lat = R.lattice(4)                                              # 64 points, d11 = 1 everywhere
    pair = lambda a, b: (M.pointcloud_overlap_pair(dev(a), dev(b)), R.overlap_pair(a, b))
    assert pair(lat, R.lattice(4, (4, 0, 0))) == (0, 0)             # the face x = 3 is 1 from the other lattice: d12 == d11 counts 0
    assert pair(lat, R.lattice(4, (3, 0, 0))) == (16, 16)           # the face x = 3 is shared: a coincident point counts 1
    assert pair(lat, lat.copy()) == (64, 64)                        # pc2 == pc1 gives P
    twice = np.concatenate([lat, lat[:10]])                         # ten points twice: each of the twenty has a duplicate at 0
    assert pair(twice, lat.copy()) == (54, 54)                      # duplicate points inside pc1 count 0, the other 54 coincide with pc2
    assert pair(twice, R.lattice(4, (3, 0, 0))) == (R.overlap_pair(twice, R.lattice(4, (3, 0, 0))),) * 2
    half = R.lattice(4, (0.5, 0, 0))                                # 0.25 < 1: every point of lat has a nearer point there
    assert pair(lat, half) == (64, 64)
    clouds = np.stack([lat, R.lattice(4, (4, 0, 0)), R.lattice(4, (3, 0, 0))])
    pairs = np.array([(0, 1), (0, 2), (0, 0), (1, 2), (2, 1)], np.int32)
    want = R.overlap_counts(clouds, pairs)
    assert want[:3] == [0, 16, 64]
    assert host(M.overlap_counts(dev(clouds), None, dev(pairs), fitted=True)).tolist() == want


# ------------------------------------------------------------------------------------------------ independence
def test_a_count_depends_on_its_pair_alone(M):
    c = R.case('room')
    clouds, boxes = dev(c['clouds']), dev(c['boxes'])
    placed = R.fit_all(c['boxes'], c['clouds'])
    alone = host(M.overlap_counts(clouds, boxes, dev(np.array([(1, 3)], np.int32)))).tolist()
    back = host(M.overlap_counts(clouds, boxes, dev(np.array([(3, 1)], np.int32)))).tolist()
    assert alone == R.overlap_counts(placed, [(1, 3)]) and back == R.overlap_counts(placed, [(3, 1)]) and alone != back
    rs = np.random.RandomState(0)
    many = rs.randint(0, 6, (50, 2)).astype(np.int32)
    many[17] = (1, 3)
    many[31] = (3, 1)
    want = R.overlap_counts(placed, many)
    runs = [host(M.overlap_counts(clouds, boxes, dev(many))).tolist() for _ in range(2)]
    assert runs[0] == runs[1] == want and want[17] == alone[0] and want[31] == back[0]
    assert host(M.overlap_counts(clouds, boxes, dev(many[::-1]))).tolist() == want[::-1]


def test_up_y_is_up_z_on_the_swapped_scene(M, G):
    """the generator asserted the margin of the room for both conventions"""
    c = R.case('room')
    s = R.swap_yz(c)
    want = G['room/counts'].tolist()
    assert drop_in(M, s, up='y') == want == drop_in(M, c)
    fz, fy = M.fit_shapes_to_box(dev(c['boxes']), dev(c['clouds'])), M.fit_shapes_to_box(dev(s['boxes']), dev(s['clouds']), up='y')
    assert torch.equal(fz[:, :, [0, 2, 1]], fy)
    pairs = dev(pairs_of(c))
    assert host(M.overlap_counts(dev(s['clouds']), dev(s['boxes']), pairs, up='y')).tolist() == want
    assert drop_in(M, s, up='z') != want                            # the conventions do differ on this scene


# ------------------------------------------------------------------------------------------------ pruning
def test_pruning_changes_no_result(M, G):
    c = R.case('apart')
    assert drop_in(M, c) == [0, 0, 0, 0] == G['apart/counts'].tolist()
    every = np.array([(i, j) for i in range(6) for j in range(6) if i != j], np.int32)
    assert not host(M.overlap_counts(dev(c['clouds']), dev(c['boxes']), dev(every))).any()
    a, b = R.staircase_pair(5, 300)                                 # bounds that overlap, clouds that do not
    assert (np.maximum(a.min(0), b.min(0)) < np.minimum(a.max(0), b.max(0))).all()
    assert R.overlap_pair(a, b) == 0 == R.overlap_pair(b, a)
    assert M.pointcloud_overlap_pair(dev(a), dev(b)) == 0 == M.pointcloud_overlap_pair(dev(b), dev(a))
    b2 = b - np.array([0, 0.35, 0], np.float32)                     # pushed into each other
    want = R.overlap_pair(a, b2)
    assert 0 < want < 300 and M.pointcloud_overlap_pair(dev(a), dev(b2)) == want


# ------------------------------------------------------------------------------------------------ status words and refusals
def test_what_only_the_device_sees_raises(M):
    c = R.case('room')
    boxes, pairs = dev(c['boxes']), dev(pairs_of(c))
    flat = c['clouds'].copy()
    flat[2, :, 1] = 0.25                                            # no extent along y
    nan = c['clouds'].copy()
    nan[4, 100, 2] = np.nan
    infbox = c['boxes'].copy()
    infbox[1, 3] = np.inf
    for clouds, bx, what in ((flat, c['boxes'], 'cloud 2 has zero extent'), (nan, c['boxes'], 'cloud 4 .* not finite'), (c['clouds'], infbox, 'cloud 1 .* not finite')):
        with pytest.raises(ValueError, match=what):
            M.fit_shapes_to_box(dev(bx), dev(clouds))
        with pytest.raises(ValueError, match=what):
            M.overlap_counts(dev(clouds), dev(bx), pairs)
        metric = [3]
        with pytest.raises(ValueError, match=what):
            M.pointcloud_overlap(dev(clouds), dev(c['objs']), dev(bx[:, :6]), dev(bx[:, 6]), dev(c['triples']), R.VOCAB, metric)
        assert metric == [3]
    with pytest.raises(ValueError, match='not finite'):
        M.overlap_counts(dev(nan), None, pairs, fitted=True)
    with pytest.raises(ValueError, match='not finite'):
        M.pointcloud_overlap_pair(dev(c['clouds'][0]), dev(nan[4]))
    with pytest.raises(ValueError, match='zero extent'):
        M.fit_shapes_to_box(boxes[0], dev(c['clouds'][0, :1]))      # one point has no extent
    assert host(M.overlap_counts(dev(flat), None, pairs, fitted=True)).shape == (4,)                  # placed already: nothing to divide by


def test_a_pair_index_out_of_range_raises_and_is_not_read_through(M):
    c = R.case('room')
    clouds, boxes = dev(c['clouds']), dev(c['boxes'])
    good = pairs_of(c)
    for bad in ((6, 1), (1, 6), (-1, 2), (2, -1), (2 ** 31 - 1, 0), (0, -2 ** 31)):
        pairs = good.copy()
        pairs[2] = bad
        with pytest.raises(ValueError, match=r'outside \[0, 6\)'):
            M.overlap_counts(clouds, boxes, dev(pairs))
    assert host(M.overlap_counts(clouds, boxes, dev(good))).tolist() == R.expected_counts(c)          # the next call is served


def test_refusals_on_the_device_side(M):
    c = R.case('room')
    clouds, boxes, pairs = dev(c['clouds']), dev(c['boxes']), dev(pairs_of(c))
    objs, triples = dev(c['objs']), dev(c['triples'])
    with pytest.raises(ValueError, match='unequal sizes'):
        M.pointcloud_overlap(list(clouds[:5]) + [clouds[5, :200]], objs, boxes[:, :6], boxes[:, 6], triples, R.VOCAB, [])
    with pytest.raises(ValueError, match='different devices'):
        M.overlap_counts(clouds, boxes.cpu(), pairs)
    with pytest.raises(ValueError, match='different devices'):
        M.overlap_counts(clouds, boxes, pairs.cpu())
    with pytest.raises(ValueError, match='different devices'):
        M.fit_shapes_to_box(boxes, clouds.cpu())
    with pytest.raises(ValueError, match='different devices'):
        M.pointcloud_overlap_pair(clouds[0], clouds[1].cpu())
    with pytest.raises(ValueError, match='different devices'):
        M.pointcloud_overlap(list(clouds[:5]) + [clouds[5].cpu()], objs, boxes[:, :6], boxes[:, 6], triples, R.VOCAB, [])
    with pytest.raises(ValueError, match='different devices'):
        M.pointcloud_overlap(clouds, objs, boxes[:, :6], boxes[:, 6].cpu(), triples, R.VOCAB, [])
    for call in (lambda: M.overlap_counts(clouds.cpu(), boxes.cpu(), pairs.cpu()), lambda: M.fit_shapes_to_box(boxes.cpu(), clouds.cpu()),
                 lambda: M.pointcloud_overlap_pair(clouds[0].cpu(), clouds[1].cpu()),
                 lambda: M.pointcloud_overlap(clouds.cpu(), objs.cpu(), boxes[:, :6].cpu(), boxes[:, 6].cpu(), triples.cpu(), R.VOCAB, [])):
        with pytest.raises(ValueError, match='not on the device'):
            call()


# ------------------------------------------------------------------------------------------------ the chain
def test_point_clouds_to_counts_on_device_tensors(M):
    """shape_metrics.point_clouds -> pointcloud_overlap without a host copy in between: equal sizes by construction, angles [O, 1],
    the rotation about y of this package's boxes; the restatement runs on a host copy of the same clouds"""
    from echoscene_amd import shape_metrics
    c = R.case('room')
    clouds = shape_metrics.point_clouds([dev(v) for v in c['clouds']], number=200)
    assert clouds.shape == (6, 200, 3) and clouds.is_cuda
    boxes = dev(c['boxes'])
    got = M.pointcloud_overlap(clouds, dev(c['objs']), boxes[:, :6], boxes[:, 6:7], dev(c['triples']), R.VOCAB, [], up='y')
    want = R.overlap_counts(R.fit_all(c['boxes'], host(clouds), True, 'y'), pairs_of(c))
    assert got == want and max(want) > 0
