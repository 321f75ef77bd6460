"""Host checks of the scene metric (echoscene_amd/scene_metrics.py): the numpy restatement of tests/scene_metrics_ref.py against what
the reference recorded (tests/golden/scene_overlap.npz, written by tests/golden/make_golden_scene_overlap.py) and against the float64
yardstick, the host-only pair selection, and the refusals that need no device.  No device compute is called here.

The bar of a fitted coordinate is measured on the reference: ``ref_fit_err`` = 1.78e-07 over the recorded fits (coordinates within
+-3.2), times 4 for another order of the same operations -> 7.11e-07; the restatement is 2.07e-07 from the yardstick."""
import os

import numpy as np
import pytest
import torch

import scene_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'scene_overlap.npz')))


@pytest.fixture(scope='module')
def M():
    from echoscene_amd import scene_metrics
    return scene_metrics


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_counts_are_the_recorded_ones(G, name):
    assert R.expected_counts(R.case(name)) == G[name + '/counts'].tolist()


def test_the_cases_cover_what_they_are_for(G):
    assert not G['apart/counts'].any() and len(G['apart/counts']) == 4
    assert G['nested/counts'][0] > 0.9 * 257                       # the outer cloud against its 0.97 copy
    assert G['p1/counts'].tolist() == [1, 1, 1, 1]
    assert len(G['batch/counts']) == 4 + 8
    assert np.abs(R.case('flat7')['boxes'][:, 6]).max() > 180
    for name in R.CASES:
        c = R.case(name)
        _, skipped = R.eligible_pairs(c['objs'], c['triples'], R.VOCAB, c['offsets'])
        assert all(v > 0 for v in skipped.values()), (name, skipped)
        assert name == 'apart' or G[name + '/counts'].max() > 0


def test_restatement_fit_is_within_the_bar_of_the_yardstick(G):
    bar = 4 * float(G['ref_fit_err'])
    assert 0 < bar and R.MARGIN >= 8 * bar
    worst = worst_ref = 0.0
    for name in R.CASES:
        c = R.case(name)
        if c['placed']:
            continue
        mine, exact = R.fit_all(c['boxes'], c['clouds']), R.fit64_all(c['boxes'], c['clouds'])
        assert mine.dtype == np.float32
        worst, worst_ref = max(worst, float(np.abs(mine - exact).max())), max(worst_ref, float(np.abs(G[name + '/fit'] - exact).max()))
    print('fit: the restatement is %.3g from the yardstick, the reference %.3g (bar %.3g)' % (worst, worst_ref, bar))
    assert worst <= bar and worst_ref == float(G['ref_fit_err'])


def test_up_y_is_up_z_with_the_columns_swapped():
    c = R.case('room')
    s = R.swap_yz(c)
    assert np.array_equal(R.fit_all(s['boxes'], s['clouds'], True, 'y'), R.fit_all(c['boxes'], c['clouds'])[:, :, [0, 2, 1]])
    assert R.expected_counts(s, 'y') == R.expected_counts(c)


@pytest.mark.parametrize('name', list(R.CASES))
def test_eligible_pairs_are_the_pairs_of_the_recorded_lists(M, G, name):
    c = R.case(name)
    want, _ = R.eligible_pairs(c['objs'], c['triples'], R.VOCAB, c['offsets'])
    got = M.eligible_pairs(torch.from_numpy(c['objs']), torch.from_numpy(c['triples']), R.VOCAB, offsets=c['offsets'])
    assert got.dtype == torch.int32 and not got.is_cuda and got.shape == (len(G[name + '/counts']), 2)
    assert np.array_equal(got.numpy(), want)
    if len(c['offsets']) == 2:
        assert torch.equal(M.eligible_pairs(c['objs'].tolist(), c['triples'].tolist(), R.VOCAB), got)
    else:                                                           # scene by scene, shifted by the node offsets
        parts = [M.eligible_pairs(c['objs'][nodes], t, R.VOCAB) + nodes.start for nodes, t in R.scenes(c)]
        assert torch.equal(torch.cat(parts), got)
        assert all((got[:, 0] < 6) == (got[:, 1] < 6))              # no pair crosses the scenes


def test_eligible_pairs_rule_by_rule(M):
    names = ['bed\n', 'floor\n', 'table\n', 'wall', '_scene_\n', 'chair\nwith arms', 'ceiling\n', 'floor lamp\n']
    vocab = {'object_idx_to_name': names, 'pred_idx_to_name': ['left\n', 'none\n', 'inside', 'build in\n', 'inside of\n']}
    objs = [0, 2, 5, 7, 1, 3, 4, 6]                                 # four pieces of furniture ('floor lamp' is none of the four names)
    pairs = lambda t: M.eligible_pairs(objs, np.array(t, np.int64).reshape(-1, 3), vocab).tolist()
    every = [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert pairs([]) == every
    assert pairs([(0, 0, 1), (2, 4, 3)]) == every                   # 'left' and 'inside of' touch nothing
    assert pairs([(0, 1, 1)]) == every[1:]                          # none, as stated
    assert pairs([(3, 2, 0)]) == every[:2] + every[3:]              # inside, in the reverse direction; a name without a newline
    assert pairs([(1, 3, 2), (1, 0, 2)]) == every                   # the later triple decides ...
    assert pairs([(1, 0, 2), (1, 3, 2)]) == every[:3] + every[4:]   # ... either way
    assert pairs([(1, 0, 2), (2, 3, 1)]) == every[:3] + every[4:]   # (i, j) does not touch, (j, i) does
    assert M.eligible_pairs([1, 3], [], vocab).shape == (0, 2)
    assert M.eligible_pairs([], [], vocab).shape == (0, 2)


def test_refusals_that_need_no_device(M):
    c = R.case('room')
    clouds, boxes = torch.from_numpy(c['clouds']), torch.from_numpy(c['boxes'])
    objs, triples = torch.from_numpy(c['objs']), torch.from_numpy(c['triples'])
    pairs = torch.zeros(1, 2, dtype=torch.int32)
    bad = [
        (lambda: M.fit_shapes_to_box(boxes, clouds), 'not on the device'),
        (lambda: M.fit_shapes_to_box(boxes[0], clouds[0]), 'not on the device'),
        (lambda: M.fit_shapes_to_box(boxes[:, :6], clouds), r'\[O, 7\]'),
        (lambda: M.fit_shapes_to_box(boxes[:5], clouds), '5 boxes for 6 clouds'),
        (lambda: M.fit_shapes_to_box(boxes, clouds.double()), 'float32'),
        (lambda: M.fit_shapes_to_box(boxes, clouds[:, :, :2]), r'\[O, P, 3\]'),
        (lambda: M.fit_shapes_to_box(boxes, clouds, up='x'), 'up must be'),
        (lambda: M.fit_shapes_to_box(boxes.numpy(), clouds), 'must be a tensor'),
        (lambda: M.pointcloud_overlap_pair(clouds[0], clouds[1]), 'not on the device'),
        (lambda: M.pointcloud_overlap_pair(clouds, clouds[1]), r'\[P, 3\]'),
        (lambda: M.pointcloud_overlap_pair(clouds[0], clouds[1].half()), 'float32'),
        (lambda: M.overlap_counts(clouds, boxes, pairs), 'not on the device'),
        (lambda: M.overlap_counts(clouds, boxes, pairs.long()), 'int32'),
        (lambda: M.overlap_counts(clouds, boxes, pairs[0]), r'\[K, 2\]'),
        (lambda: M.overlap_counts(clouds, boxes[:, :6], pairs), r'\[O, 7\]'),
        (lambda: M.overlap_counts(clouds, None, pairs), 'boxes must be a tensor'),
        (lambda: M.overlap_counts(clouds, None, pairs, fitted=True), 'not on the device'),
        (lambda: M.overlap_counts(clouds, boxes, pairs, up='Z'), 'up must be'),
        (lambda: M.pointcloud_overlap(clouds, objs, boxes[:, :6], boxes[:, 6], triples, R.VOCAB, []), 'not on the device'),
        (lambda: M.pointcloud_overlap(list(clouds[:5]) + [clouds[5, :200]], objs, boxes[:, :6], boxes[:, 6], triples, R.VOCAB, []), 'unequal sizes'),
        (lambda: M.pointcloud_overlap(clouds, objs, boxes[:, :6], boxes[:, 6], triples, R.VOCAB, ()), 'must be a list'),
        (lambda: M.pointcloud_overlap(clouds, objs[:5], boxes[:, :6], boxes[:, 6], triples, R.VOCAB, []), '5 objs'),
        (lambda: M.pointcloud_overlap(clouds, objs, boxes[:, :6], boxes[:5, 6], triples, R.VOCAB, []), 'angles'),
        (lambda: M.pointcloud_overlap(clouds, objs, boxes[:, :6], boxes[:, 6], triples, {}, []), 'object_idx_to_name'),
        (lambda: M.eligible_pairs(objs + 100, triples, R.VOCAB), 'class outside'),
        (lambda: M.eligible_pairs(objs, triples + torch.tensor([0, 100, 0]), R.VOCAB), 'predicate outside'),
        (lambda: M.eligible_pairs(objs, triples[:, :2], R.VOCAB), r'\[T, 3\]'),
        (lambda: M.eligible_pairs(objs, triples, R.VOCAB, offsets=[0, 3, 5]), 'offsets'),
        (lambda: M.eligible_pairs(objs.float(), triples, R.VOCAB), 'integers'),
    ]
    for call, what in bad:
        with pytest.raises(ValueError, match=what):
            call()
