#!/usr/bin/env python
"""Goldens of the layout metrics (echoscene_amd/layout_metrics.py) from the reference's helpers/metrics_3dfront.py, run on CPU tensors;
the packages that module's imports want and the image lacks are the inert stand-ins of make_golden.py.

    python tests/golden/make_golden_layout_metrics.py --ref <checkout of the reference>     # writes tests/golden/layout_metrics.npz

Recorded (the inputs are not: tests/layout_metrics_ref.py rebuilds them from their seeds):
  <case>/<function>/<key>   the list the reference's validate_constrains / validate_constrains_changes leaves under each of the 12
                            accuracy keys, for every case of layout_metrics_ref.CASES (random scenes, the planted set, keep masks,
                            strict=False, 7-column boxes, s == o, negative sizes, a flat box 2, the threshold edges), int8
  iou_<n>                   box3d_iou of the n-th pair set of layout_metrics_ref.iou_pairs(), float64 [K, 2] (iou, iou_2d)
  ref_iou_err               the largest |reference - exact yardstick| over every recorded IoU that is a number, both outputs
  numpy_version             the numpy the reference ran under (its float32 scalar arithmetic follows NEP 50 from 2.0 on)
Conditions asserted before anything is written: in the planted set every rule has a fulfilled and a failed triple, and every strict
rule one that fails through the overlap alone; outside the threshold-edge case the deciding quantity of every triple is at least 1e-4
from its threshold on the exact yardstick, so a verdict does not hang on a rounding; in the edge case the deciding quantity is the
float32 threshold itself or its neighbour; a recorded NaN is a yardstick 0 / 0."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import layout_metrics_ref as R  # noqa: E402

MARGIN = 1e-4


def reference(ref):
    import make_golden
    make_golden.install_reference(ref)
    import helpers.metrics_3dfront as M
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    M = reference(ap.parse_args().ref)
    assert int(np.__version__.split('.')[0]) >= 2, 'the float32 rules are recorded under NEP 50 (numpy >= 2)'
    out = {'numpy_version': np.array(np.__version__)}

    n_triples = 0
    for name in R.CASES:
        c = R.case(name)
        boxes, triples = torch.from_numpy(c['boxes']), torch.from_numpy(c['triples'])
        keep = None if c['keep'] is None else torch.from_numpy(c['keep'])
        if name != 'edges':
            worst = min(R.margins(c))
            assert worst >= MARGIN, 'case %s: a deciding quantity is %.3g from its threshold; choose another seed' % (name, worst)
        for fn in c['functions']:
            acc = getattr(M, fn)(triples, boxes, None, keep, R.VOCAB, R.empty_accuracy(), strict=c['strict'],
                                 overlap_threshold=c['overlap_threshold'])
            for k in R.ALL_KEYS:
                out['%s/%s/%s' % (name, fn, k)] = np.array(acc[k], np.int8)
            n_triples += len(acc['total'])

    # the planted set covers every cell; a strict rule also fails through the overlap alone (it passes with strict=False)
    for k in R.KEYS:
        got = set(out['planted/validate_constrains/%s' % k].tolist())
        assert got == {0, 1}, 'planted set: rule %r has outcomes %s only' % (k, got)
    for k in R.KEYS[:4]:
        strict, loose = out['planted/validate_constrains/%s' % k], out['planted_loose/validate_constrains/%s' % k]
        assert np.any((strict == 0) & (loose == 1)), 'planted set: rule %r never fails through the overlap alone' % k
    # the edge case: every deciding quantity is a float32 threshold or its neighbour, and the three neighbours do not agree
    c = R.case('edges')
    assert max(R.margins(c)) < 1e-7
    e = out['edges/validate_constrains/total']
    assert all(len(set(e[i:i + 3].tolist())) == 2 for i in range(0, len(e), 3))
    # keep masks select: the two functions split the judged triples of a masked case between them
    for name in ('keep', 'keep_planted'):
        n = (R.rule_of_pred(R.VOCAB)[R.case(name)['triples'][:, 1]] >= 0).sum()
        assert len(out[name + '/validate_constrains/total']) + len(out[name + '/validate_constrains_changes/total']) == n
        assert 0 < len(out[name + '/validate_constrains/total']) < n

    errs, n_nan = [0.0], 0
    for n, (a, b, wt) in enumerate(R.iou_pairs()):
        rec = np.zeros((len(a), 2))
        for i, (x, y) in enumerate(zip(a, b)):
            with np.errstate(all='ignore'):
                rec[i] = M.box3d_iou(x, y, param6=True, with_translation=wt)
            for got, exact in zip(rec[i], R.iou_exact(x, y, wt)):
                if exact is None:
                    assert np.isnan(got), (x, y, got)
                    n_nan += 1
                else:
                    errs.append(abs(float(got) - float(exact)))
        out['iou_%d' % n] = rec
    out['ref_iou_err'] = np.float64(max(errs))

    path = os.path.join(HERE, 'layout_metrics.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB): %d verdicts of the reference under numpy %s; %d IoUs (%d NaN), reference error %.3g'
          % (path, os.path.getsize(path) / 1024, n_triples, np.__version__, len(errs) - 1 + n_nan, n_nan, out['ref_iou_err']))


if __name__ == '__main__':
    main()
