"""CPU-only checks of the layout metrics (csrc/es_layout_metrics.hip, echoscene_amd/layout_metrics.py): the additions to the C ABI and
the host refusals of the two launchers, the numpy restatement of the rules (tests/layout_metrics_ref.py) against every verdict the
reference recorded (tests/golden/layout_metrics.npz) and its IoUs against the exact yardstick, the predicate-name mapping,
``summarize`` against eval's formulas, and every refusal of the Python calls.  No device compute is called here.

The bar of an IoU is measured on the reference, not derived: ``ref_iou_err`` = 4.44e-16, the largest |reference - exact| over the
678 recorded values, times 4 for another order of the same operations (the reference takes the area of the clipped footprint from
a convex hull, the restatement and the kernel from the shoelace formula).  The restatement is 4.28e-16 from the yardstick."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import layout_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('es_relation_check', 'es_box3d_iou')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


@pytest.fixture(scope='module')
def M():
    from echoscene_amd import layout_metrics
    return layout_metrics


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'layout_metrics.npz')))


def recorded(G, name, fn):
    return {k: G['%s/%s/%s' % (name, fn, k)].tolist() for k in R.ALL_KEYS}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported(L):
    from echoscene_amd import hip, build
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip.EXPORTS and hasattr(raw, name), name
    assert 'es_layout_metrics.hip' in build.SOURCES
    assert len(hip.EXPORTS['es_relation_check'][1]) == 17 and len(hip.EXPORTS['es_box3d_iou'][1]) == 9
    assert L.es_abi_version() == 10


def test_launchers_refuse_on_the_host(L):
    """pointers, counts, the leading dimension and the two mode words are checked before anything is enqueued (no device is needed to
    get the refusal), and es_last_error names the function"""
    p = C.c_void_p(4096)                                            # never dereferenced
    good = dict(boxes=p, O=4, ld=6, triples=p, T=8, tab=p, n_pred=16, keep=None, keep_dtype=0, keep_mode=0, strict=1, thr=0.3, rule=p, ok=p,
                counts=None, status=p)

    def call(**kw):
        a = dict(good, **kw)
        rc = L.es_relation_check(a['boxes'], a['O'], a['ld'], a['triples'], a['T'], a['tab'], a['n_pred'], a['keep'], a['keep_dtype'],
                                 a['keep_mode'], a['strict'], a['thr'], a['rule'], a['ok'], a['counts'], a['status'], None)
        return rc, L.es_last_error().decode()
    for kw in (dict(boxes=None), dict(triples=None), dict(tab=None), dict(rule=None), dict(ok=None), dict(status=None), dict(O=0), dict(ld=5),
               dict(T=0), dict(T=2 ** 31 - 1), dict(n_pred=0), dict(keep_mode=3), dict(keep_mode=-1), dict(keep=p, keep_dtype=4)):
        rc, msg = call(**kw)
        assert rc == 2 and msg.startswith('es_relation_check'), (kw, rc, msg)
    for args in ((None, 6, p, 6, 1), (p, 6, None, 6, 1), (p, 5, p, 6, 1), (p, 6, p, 5, 1), (p, 6, p, 6, 0), (p, 6, p, 6, 2 ** 31 - 1)):
        a, lda, b, ldb, K = args
        assert L.es_box3d_iou(a, lda, b, ldb, K, 1, p, p, None) == 2 and L.es_last_error().decode().startswith('es_box3d_iou'), args
    assert L.es_box3d_iou(p, 6, p, 6, 1, 1, None, p, None) == 2 and L.es_box3d_iou(p, 6, p, 6, 1, 1, p, None, None) == 2


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_golden_was_recorded_under_nep50(G):
    assert int(str(G['numpy_version']).split('.')[0]) >= 2 and set(R.CASES) == {k.split('/')[0] for k in G if '/' in k}


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_reproduces_every_recorded_verdict(G, name):
    """list by list, in order, 'total' included, through both of the reference's functions"""
    c = R.case(name)
    for fn in c['functions']:
        rule, ok = R.check(c['triples'], c['boxes'], keep=c['keep'], mode=R.MODE_OF[fn], strict=c['strict'],
                           overlap_threshold=c['overlap_threshold'])
        assert R.accuracy_of(rule, ok) == recorded(G, name, fn), (name, fn)


def test_no_recorded_verdict_hangs_on_a_rounding():
    """outside the edge case every deciding quantity is at least 1e-4 from its threshold on the exact yardstick (the generator's
    condition); so are the two boxes of the T sweep of the GPU tests"""
    for name in R.CASES:
        if name != 'edges':
            assert min(R.margins(R.case(name))) >= 1e-4, name
    tab = R.rule_of_pred(R.VOCAB)
    for T in (1, 255, 256, 257):
        boxes, triples = R.tiny(T)
        assert all(R.margin(int(tab[p]), boxes[s], boxes[o]) >= 1e-4 for s, p, o in triples.tolist() if tab[p] >= 0)


def test_restatement_ious_against_the_exact_yardstick(G):
    bar = 4 * float(G['ref_iou_err'])
    assert 0 < bar < 1e-14
    worst = worst_ref = 0.0
    n_nan = 0
    for n, (a, b, wt) in enumerate(R.iou_pairs()):
        rec = G['iou_%d' % n]
        for i, (x, y) in enumerate(zip(a, b)):
            for got, exact, ref in zip(R.box3d_iou(x, y, wt), R.iou_exact(x, y, wt), rec[i]):
                if exact is None:
                    assert math.isnan(got) and math.isnan(ref)
                    n_nan += 1
                else:
                    worst, worst_ref = max(worst, abs(got - float(exact))), max(worst_ref, abs(got - ref))
    print('restatement: %.3g from the yardstick (bar %.3g), %.3g from the reference; %d NaN' % (worst, bar, worst_ref, n_nan))
    assert worst <= bar and n_nan == 12


def test_exact_yardstick_on_closed_forms():
    u = [1, 1, 1, 0, 0, 0]
    assert R.iou_exact(u, u) == (1, 1)
    assert R.iou_exact(u, [1, 1, 1, 0.5, 0, 0], True) == (Fraction_(1, 2), Fraction_(1, 3))
    assert R.iou_exact(u, [1, 1, 1, 1, 0, 0], True) == (0, 0)                      # touching
    assert R.iou_exact([0.5, 0.5, 0.5, 0, 0, 0], [2, 2, 2, 0, 0, 0]) == (1, Fraction_(1, 16))
    assert R.iou_exact(u, [-1, 1, 1, 0, 0, 0]) == (0, 0) and R.iou_exact([-1, 1, 1, 0, 0, 0], u) == (1, 1)
    assert R.iou_exact(u, [1, 1, 0, 0, 0, 0]) == (None, 0) and R.iou_exact([0, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]) == (None, None)
    assert R.box3d_iou(u, [1, 1, 1, 0.5, 0, 0], True) == (0.5, 1 / 3)


def Fraction_(a, b):
    from fractions import Fraction
    return Fraction(a, b)


# ------------------------------------------------------------------------------------------------ names and the printed row
def test_name_mapping_drops_the_last_character_whatever_it_is(M):
    want = [-1, 0, 1, 2, 3, 9, 10, 5, 4, 7, 6, 8, -1, -1, -1, -1]
    assert M.rule_of_pred(R.VOCAB).tolist() == want == R.rule_of_pred(R.VOCAB).tolist()
    assert M.rule_of_pred(R.VOCAB).dtype == np.int8
    assert M.rule_of_pred({'pred_idx_to_name': [n + 'X' for n in R.PRED_NAMES]}).tolist() == want
    bare = M.rule_of_pred({'pred_idx_to_name': list(R.PRED_NAMES)}).tolist()        # without the newline a name loses a letter
    assert bare == [-1] * 16
    assert M.rule_of_pred({'pred_idx_to_name': ['left', 'leftt', 'left \n', 'bigger than\n', 'bigger\n', '']}).tolist() == [-1, 0, -1, 5, -1, -1]
    assert M.KEYS == R.KEYS and M.RULE_NAMES == R.RULE_NAMES


def test_summarize_against_the_formulas(M, G):
    for name, fn in (('random0', 'validate_constrains'), ('planted', 'validate_constrains'), ('keep', 'validate_constrains_changes'),
                     ('self', 'validate_constrains')):
        acc = recorded(G, name, fn)
        row, want = M.summarize(acc), R.summary_row(acc)
        assert list(row) == ['L/R', 'F/B', 'Bi/Sm', 'Ta/Sh', 'Stand', 'Close', 'Symm', 'Total', 'means of mean']
        for k in want:
            assert row[k] == want[k] or (math.isnan(row[k]) and math.isnan(want[k])), (name, k, row[k], want[k])
        counts = {k: (sum(v), len(v)) for k, v in acc.items()}
        from_counts = M.summarize(counts)
        for k in want:
            assert from_counts[k] == pytest.approx(want[k], rel=4e-16, abs=0, nan_ok=True), (name, k)
    empty = M.summarize(R.empty_accuracy())
    assert all(math.isnan(v) for v in empty.values())
    acc = R.empty_accuracy()
    acc['left'], acc['right'], acc['total'] = [1, 1, 0, 1], [0], [1, 1, 0, 1, 0]
    row = M.summarize(acc)
    assert row['L/R'] == 0.375 and row['Total'] == 0.6 and math.isnan(row['F/B']) and math.isnan(row['means of mean'])
    with pytest.raises(ValueError):
        M.summarize({'left': []})


# ------------------------------------------------------------------------------------------------ refusals
def test_every_argument_refusal(M):
    """each is a ValueError before any device work: a machine without a device gets them all, the device refusal last"""
    boxes, triples = (torch.from_numpy(x) for x in R.random_scene(1))
    good = dict(triples=triples, boxes=boxes, vocab=R.VOCAB, keep=None, mode='all', strict=True, overlap_threshold=0.3)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device='meta')
    bad = [(dict(boxes=boxes.numpy()), 'must be a tensor'), (dict(boxes=boxes.double()), 'float32'), (dict(boxes=boxes[:, :5]), r'\[O, 6\]'),
           (dict(boxes=boxes[0]), r'\[O, 6\]'), (dict(boxes=boxes[:0]), 'O >= 1'), (dict(boxes=torch.zeros(3, 8)), r'\[O, 6\]'),
           (dict(triples=triples.tolist()), 'must be a tensor'), (dict(triples=triples.int()), 'int64'), (dict(triples=triples[:, :2]), r'\[T, 3\]'),
           (dict(triples=triples[0]), r'\[T, 3\]'),
           (dict(vocab=None), 'pred_idx_to_name'), (dict(vocab={}), 'pred_idx_to_name'), (dict(vocab={'pred_idx_to_name': []}), 'pred_idx_to_name'),
           (dict(vocab={'pred_idx_to_name': ['left\n', 3]}), 'pred_idx_to_name'),
           (dict(keep=[1] * 12), 'keep must be None or a tensor'), (dict(keep=torch.ones(12, dtype=torch.float64)), 'keep must be one of'),
           (dict(keep=torch.ones(11)), 'one entry per box'), (dict(keep=torch.ones(1, 12)), 'one entry per box'),
           (dict(mode='kept'), 'mode must be one of'), (dict(strict=1), 'strict must be a bool'), (dict(overlap_threshold='0.3'), 'real number'),
           (dict(overlap_threshold=None), 'real number'), (dict(overlap_threshold=True), 'real number'),
           (dict(triples=meta(triples)), 'different devices'), (dict(keep=meta(torch.ones(12, 1))), 'different devices'),
           ({}, 'not on the device')]
    for fn in (M.relation_verdicts, M.relation_accuracy):
        for kw, what in bad:
            with pytest.raises(ValueError, match=what):
                fn(**dict(good, **kw))
    for fn in (M.validate_constrains, M.validate_constrains_changes):
        for kw, what in bad:
            a = dict(good, **kw)
            if 'mode' in kw:
                continue
            with pytest.raises(ValueError, match=what):
                fn(a['triples'], a['boxes'], None, a['keep'], a['vocab'], R.empty_accuracy(), strict=a['strict'],
                   overlap_threshold=a['overlap_threshold'])
        for acc in (None, {}, {k: [] for k in R.KEYS}, dict(R.empty_accuracy(), total=0)):
            with pytest.raises(ValueError, match='accuracy must be a dict'):
                fn(triples, boxes, None, None, R.VOCAB, acc)
        with pytest.raises(ValueError, match='not on the device'):                   # T == 0 is still checked
            fn(triples[:0], boxes, None, None, R.VOCAB, R.empty_accuracy())
    for a, b, what in ((boxes.numpy(), boxes, 'must be a tensor'), (boxes, boxes.double(), 'float32'), (boxes[:, :4], boxes, r'\[O, 6\]'),
                       (boxes, boxes[:5], 'row by row'), (boxes[0], boxes, 'row by row'), (boxes, meta(boxes), 'different devices'),
                       (boxes, boxes, 'not on the device'), (boxes[0], boxes[1], 'not on the device')):
        with pytest.raises(ValueError, match=what):
            M.box3d_iou(a, b, with_translation=True)
