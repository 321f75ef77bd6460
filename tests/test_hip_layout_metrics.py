"""GPU tests of the layout metrics: the relation-check and box-IoU kernels (csrc/es_layout_metrics.hip) behind
echoscene_amd/layout_metrics.py, against what the reference recorded (tests/golden/layout_metrics.npz, written by
tests/golden/make_golden_layout_metrics.py), the numpy restatement and the exact yardstick of tests/layout_metrics_ref.py.

Verdicts are compared bit for bit: outside the threshold-edge case the generator asserted, on the exact yardstick, that every
deciding quantity is at least 1e-4 from its threshold, and in the edge case the deciding quantity is one float32 subtraction (or the
root of a square), which has one correct result.  The bar of an IoU is measured on the reference: ``ref_iou_err`` = 4.44e-16 over the 678
recorded values, times 4 for another order of the same operations (the precedent of test_hip_shape_metrics.py)  BAR = 1.78e-15.
Measured on an MI355X (profiles/layout_metrics_notes.md): the kernel's IoUs are the restatement's bit for bit, 4.28e-16 from the
yardstick."""
import math
import os

import numpy as np
import pytest
import torch

import layout_metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ('validate_constrains', 'validate_constrains_changes')


@pytest.fixture(scope='module')
def M():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import layout_metrics
    return layout_metrics


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'layout_metrics.npz')))


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def same_row(a, b):
    return list(a) == list(b) and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)


def recorded(G, name, fn):
    return {k: G['%s/%s/%s' % (name, fn, k)].tolist() for k in R.ALL_KEYS}


def drop_in(M, fn, c, accuracy=None):
    return getattr(M, fn)(dev(c['triples']), dev(c['boxes']), None, dev(c['keep']), R.VOCAB, R.empty_accuracy() if accuracy is None else accuracy,
                          strict=c['strict'], overlap_threshold=c['overlap_threshold'])


# ------------------------------------------------------------------------------------------------ verdicts
@pytest.mark.parametrize('name', list(R.CASES))
def test_every_recorded_verdict_bit_for_bit(M, G, name):
    """both drop-in functions, every list in the reference's order, 'total' included; the 7-column case also through
    validate_constrains_changes, where the reference itself cannot unpack the rows: against the restatement"""
    c = R.case(name)
    for fn in FUNCTIONS:
        acc = R.empty_accuracy()
        assert drop_in(M, fn, c, acc) is acc
        if fn in c['functions']:
            assert acc == recorded(G, name, fn), (name, fn)
        else:
            assert acc == R.accuracy_of(*R.check(c['triples'], c['boxes'], keep=c['keep'], mode=R.MODE_OF[fn], strict=c['strict'],
                                                 overlap_threshold=c['overlap_threshold']))


def test_lists_are_appended_to_not_replaced(M, G):
    c = R.case('random0')
    acc = drop_in(M, FUNCTIONS[0], c)
    first = {k: list(v) for k, v in acc.items()}
    drop_in(M, FUNCTIONS[0], R.case('random1'), acc)
    want = recorded(G, 'random1', FUNCTIONS[0])
    assert acc == {k: first[k] + want[k] for k in R.ALL_KEYS}


@pytest.mark.parametrize('name', ['random0', 'planted', 'planted_loose', 'keep', 'keep_planted', 'cols7', 'edges', 'random_thr'])
def test_verdicts_and_counts_agree_with_the_drop_ins(M, G, name):
    c = R.case(name)
    kw = dict(strict=c['strict'], overlap_threshold=c['overlap_threshold'])
    for mode, fn in (('unchanged', FUNCTIONS[0]), ('changed', FUNCTIONS[1]), ('all', None)):
        rule, ok = M.relation_verdicts(dev(c['triples']), dev(c['boxes']), R.VOCAB, keep=dev(c['keep']), mode=mode, **kw)
        assert rule.dtype == ok.dtype == torch.int8 and rule.is_cuda and rule.shape == ok.shape == (len(c['triples']),)
        want_rule, want_ok = R.check(c['triples'], c['boxes'], keep=c['keep'], mode=mode, **kw)
        assert np.array_equal(host(rule), want_rule) and np.array_equal(host(ok), want_ok)
        lists = R.accuracy_of(host(rule), host(ok))
        if fn is not None:
            assert lists == drop_in(M, fn, c)
        counts = M.relation_accuracy(dev(c['triples']), dev(c['boxes']), R.VOCAB, keep=dev(c['keep']), mode=mode, **kw)
        assert counts == {k: (sum(v), len(v)) for k, v in lists.items()}
        assert same_row(M.summarize(counts), M.summarize(lists))


def test_keep_mask_dtypes_and_shapes(M):
    c = R.case('keep')
    want = drop_in(M, FUNCTIONS[0], c), drop_in(M, FUNCTIONS[1], c)
    for k in (c['keep'][:, 0], c['keep'].astype(np.int64), c['keep'][:, 0].astype(np.int32), c['keep'].astype(bool), c['keep'].astype(np.uint8),
              c['keep'][:, 0].astype(np.int8)):
        assert (drop_in(M, FUNCTIONS[0], dict(c, keep=k)), drop_in(M, FUNCTIONS[1], dict(c, keep=k))) == want, (k.dtype, k.shape)
    k = c['keep'] * 0.5                                             # 0.5 is neither kept (== 1) nor changed (== 0), as in the reference
    half = dict(c, keep=k)
    n_unchanged = len(R.accuracy_of(*R.check(c['triples'], c['boxes'], keep=k, mode='unchanged'))['total'])
    n_changed = len(R.accuracy_of(*R.check(c['triples'], c['boxes'], keep=k, mode='changed'))['total'])
    assert [len(drop_in(M, fn, half)['total']) for fn in FUNCTIONS] == [n_unchanged, n_changed] and n_unchanged == 0


@pytest.mark.parametrize('T', [1, 255, 256, 257])
def test_block_seams_with_two_boxes(M, T):
    """one thread per triple, 256 per workgroup: T at and around one workgroup, O = 2"""
    boxes, triples = R.tiny(T)
    want_rule, want_ok = R.check(triples, boxes)
    rule, ok = M.relation_verdicts(dev(triples), dev(boxes), R.VOCAB)
    assert np.array_equal(host(rule), want_rule) and np.array_equal(host(ok), want_ok)
    lists = R.accuracy_of(want_rule, want_ok)
    assert M.relation_accuracy(dev(triples), dev(boxes), R.VOCAB) == {k: (sum(v), len(v)) for k, v in lists.items()}
    assert M.validate_constrains(dev(triples), dev(boxes), None, None, R.VOCAB, R.empty_accuracy()) == lists


def test_three_scenes_concatenated_are_the_three_calls(M, G):
    """node offsets as collate_fn applies them; a triple reads its own two rows only"""
    cs = [R.case(n) for n in ('random0', 'random1', 'random2')]
    ofs = np.cumsum([0] + [len(c['boxes']) for c in cs])
    boxes = np.concatenate([c['boxes'] for c in cs])
    triples = np.concatenate([c['triples'] + np.array([o, 0, o]) for c, o in zip(cs, ofs)])
    one_by_one = R.empty_accuracy()
    parts = []
    for c in cs:
        drop_in(M, FUNCTIONS[0], c, one_by_one)
        parts.append(M.relation_verdicts(dev(c['triples']), dev(c['boxes']), R.VOCAB))
    assert M.validate_constrains(dev(triples), dev(boxes), None, None, R.VOCAB, R.empty_accuracy()) == one_by_one
    assert one_by_one == {k: sum((recorded(G, n, FUNCTIONS[0])[k] for n in ('random0', 'random1', 'random2')), []) for k in R.ALL_KEYS}
    rule, ok = M.relation_verdicts(dev(triples), dev(boxes), R.VOCAB)
    assert torch.equal(rule, torch.cat([p[0] for p in parts])) and torch.equal(ok, torch.cat([p[1] for p in parts]))
    counts = M.relation_accuracy(dev(triples), dev(boxes), R.VOCAB)
    assert counts == {k: (sum(v), len(v)) for k, v in one_by_one.items()}


def test_two_runs_are_identical(M):
    c = R.case('planted')
    boxes = np.concatenate([c['boxes']] * 40)
    triples = np.concatenate([c['triples'] + np.array([80 * i, 0, 80 * i]) for i in range(40)])      # 1600 triples: seven workgroups
    b, t = dev(boxes), dev(triples)
    runs = [(M.relation_verdicts(t, b, R.VOCAB), M.relation_accuracy(t, b, R.VOCAB), M.box3d_iou(b[t[:, 0]], b[t[:, 2]], with_translation=True))
            for _ in range(2)]
    (v0, c0, i0), (v1, c1, i1) = runs
    assert torch.equal(v0[0], v1[0]) and torch.equal(v0[1], v1[1]) and c0 == c1
    assert all(np.array_equal(host(x).view(np.int64), host(y).view(np.int64)) for x, y in zip(i0, i1))
    assert c0['total'] == (40 * int(R.check(c['triples'], c['boxes'])[1].sum()), 1600)


def test_t_zero_returns_untouched_without_a_launch(M):
    c = R.case('random0')
    acc = R.empty_accuracy()
    acc['left'].append(1)
    none = dev(c['triples'][:0])
    for fn in FUNCTIONS:
        assert getattr(M, fn)(none, dev(c['boxes']), None, None, R.VOCAB, acc) is acc and acc == dict(R.empty_accuracy(), left=[1])
    rule, ok = M.relation_verdicts(none, dev(c['boxes']), R.VOCAB)
    assert rule.shape == ok.shape == (0,) and rule.dtype == torch.int8
    assert M.relation_accuracy(none, dev(c['boxes']), R.VOCAB) == {k: (0, 0) for k in R.ALL_KEYS}


def test_a_bad_index_raises_and_writes_nothing(M):
    c = R.case('random0')
    for col, value, what in ((0, 12, 'node'), (2, -1, 'node'), (2, 2 ** 40, 'node'), (1, 16, 'predicate'), (1, -1, 'predicate')):
        triples = c['triples'].copy()
        triples[77, col] = value
        acc = R.empty_accuracy()
        acc['total'].append(1)
        for fn in FUNCTIONS:
            with pytest.raises(ValueError, match=what):
                getattr(M, fn)(dev(triples), dev(c['boxes']), None, None, R.VOCAB, acc)
        assert acc == dict(R.empty_accuracy(), total=[1])
        with pytest.raises(ValueError, match=what):
            M.relation_verdicts(dev(triples), dev(c['boxes']), R.VOCAB)
        with pytest.raises(ValueError, match=what):
            M.relation_accuracy(dev(triples), dev(c['boxes']), R.VOCAB)
    assert drop_in(M, FUNCTIONS[0], c)['total']                     # the next call is served


# ------------------------------------------------------------------------------------------------ the IoU
def test_box3d_iou_against_the_exact_yardstick(M, G):
    bar = 4 * float(G['ref_iou_err'])
    worst = worst_ref = 0.0
    same = True
    n_nan = 0
    for n, (a, b, wt) in enumerate(R.iou_pairs()):
        iou, iou_2d = M.box3d_iou(dev(a), dev(b), param6=True, with_translation=wt)
        assert iou.dtype == iou_2d.dtype == torch.float64 and iou.is_cuda and iou.shape == iou_2d.shape == (len(a),)
        got = np.stack([host(iou), host(iou_2d)], 1)
        rec = G['iou_%d' % n]
        assert np.array_equal(np.isnan(got), np.isnan(rec))         # NaN where the reference has NaN, and nowhere else
        for i, (x, y) in enumerate(zip(a, b)):
            mine = R.box3d_iou(x, y, wt)
            for j, exact in enumerate(R.iou_exact(x, y, wt)):
                same &= got[i, j] == mine[j] or (math.isnan(got[i, j]) and math.isnan(mine[j]))
                if exact is None:
                    assert math.isnan(got[i, j])
                    n_nan += 1
                else:
                    worst, worst_ref = max(worst, abs(got[i, j] - float(exact))), max(worst_ref, abs(got[i, j] - rec[i, j]))
    print('box3d_iou: %.3g from the yardstick (bar %.3g), %.3g from the reference, %d NaN; the restatement bit for bit: %s'
          % (worst, bar, worst_ref, n_nan, same))
    assert bar > 0 and worst <= bar and n_nan == 12
    assert same                                                     # the same IEEE operations in the same order, nothing fused


def test_box3d_iou_call_shapes(M):
    a, b, _ = R.iou_pairs()[0]
    iou, iou_2d = M.box3d_iou(dev(a), dev(b), with_translation=True)
    seven = lambda x: dev(np.concatenate([x, np.full((len(x), 1), 33.0, np.float32)], 1))
    for got in (M.box3d_iou(seven(a), seven(b), param6=False, with_translation=True), M.box3d_iou(seven(a), dev(b), with_translation=True),
                M.box3d_iou(seven(a)[:, :6], dev(b), with_translation=True)):                          # the last: a row stride of 7
        assert torch.equal(got[0], iou) and torch.equal(got[1], iou_2d)
    one = M.box3d_iou(dev(a[2]), dev(b[2]), with_translation=True)                                     # a single row is K = 1
    assert one[0].shape == (1,) and one[0][0] == iou[2] and one[1][0] == iou_2d[2]
    centred = M.box3d_iou(dev(a), dev(b))                                                              # with_translation=False
    z = a.copy(), b.copy()
    z[0][:, 3:] = 0
    z[1][:, 3:] = 0
    want = M.box3d_iou(dev(z[0]), dev(z[1]), with_translation=True)
    assert all(np.array_equal(host(x).view(np.int64), host(y).view(np.int64)) for x, y in zip(centred, want))


def test_a_flat_box1_is_area_zero_not_an_error(M):
    """the reference's convex hull raises on these; here the footprints share nothing: iou_2d = 0, and with it the volume of box 1 is
    0, so iou = 0 / 0 = NaN, which is above no threshold"""
    big = [2, 2, 2, 0, 0, 0]
    flat = np.array([[0, 0.3, 0.3, 0, 0.1, -0.25], [0.3, 0.3, 0, 0, 0.1, -0.25], [0, 0.3, 0, 0, 0.1, -0.25]], np.float32)
    iou, iou_2d = M.box3d_iou(dev(flat), dev(np.array([big] * 3, np.float32)), with_translation=True)
    assert host(iou_2d).tolist() == [0.0, 0.0, 0.0] and np.isnan(host(iou)).all()
    assert [R.box3d_iou(f, big, True)[1] for f in flat] == [0.0, 0.0, 0.0]
    boxes = np.concatenate([flat, np.array([big], np.float32)])
    triples = np.array([(i, R.PRED_OF_RULE[R.LEFT], 3) for i in range(3)], np.int64)
    acc = M.validate_constrains(dev(triples), dev(boxes), None, None, R.VOCAB, R.empty_accuracy())
    assert acc['left'] == [1, 1, 1] == acc['total']


# ------------------------------------------------------------------------------------------------ the chain
def test_descale_then_validate_on_device_tensors(M):
    """sample -> postprocess.descale_box_params -> validate_constrains without a host copy in between; 8-column rows as the layout
    loop leaves them are cut to [O, 6] by the caller, a view with a row stride of 8"""
    from echoscene_amd import postprocess
    normed, stats, triples = R.chain_case()
    x = torch.zeros(len(normed), 8, device='cuda')
    x[:, :6] = dev(normed)
    boxes = postprocess.descale_box_params(x, stats=stats)[:, :6]
    assert boxes.stride(0) == 8
    on_host = host(boxes)
    assert np.abs(on_host - R.descale(normed, stats)).max() <= 1e-6
    assert min(R.margins(dict(boxes=on_host, triples=triples, strict=True, overlap_threshold=0.3))) >= 1e-4
    acc = M.validate_constrains(dev(triples), boxes, None, None, R.VOCAB, R.empty_accuracy())
    want = R.accuracy_of(*R.check(triples, on_host))
    assert acc == want and 0 < sum(want['total']) < len(want['total'])
    assert same_row(M.summarize(acc), M.summarize(M.relation_accuracy(dev(triples), boxes, R.VOCAB)))
