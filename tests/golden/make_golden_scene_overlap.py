#!/usr/bin/env python
"""Goldens of the scene metric (echoscene_amd/scene_metrics.py) from the reference's helpers/metrics_3dfront.py and helpers/util.py, run
on CPU tensors with scikit-learn's kd-tree; the packages those modules' imports want and the image lacks are the inert stand-ins of
make_golden.py.

    python tests/golden/make_golden_scene_overlap.py --ref <checkout of the reference>     # writes tests/golden/scene_overlap.npz

Recorded (the inputs are not: tests/scene_metrics_ref.py rebuilds them from their seeds), per case of scene_metrics_ref.CASES:
  <case>/counts     the list the reference's pointcloud_overlap leaves, scene after scene for the concatenated case; for the case of
                    one point per cloud, where the reference's fit divides by zero, its pointcloud_overlap_pair on the placed clouds
                    of every eligible pair
  <case>/fit        the reference's fit_shapes_to_box of every object, float32 [O, P, 3]
  ref_fit_err       the largest |reference - float64 yardstick| coordinate over every recorded fit
  numpy_version, sklearn_version, scipy_version
Conditions asserted before anything is written: on the yardstick every query point of every recorded pair has |dist12 - dist11| >=
MARGIN (for the room also with y and z swapped and the rotation about y), so no count hangs on a rounding, and the yardstick's counts
are the reference's; MARGIN >= 8 x the coordinate bar (4 x ref_fit_err); every pair of `apart` has disjoint bounds and counts 0; every
other case has a count above 0 and a pair skipped by each of the reference's three skip rules."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import scene_metrics_ref as R  # noqa: E402


def reference(ref):
    import make_golden
    make_golden.install_reference(ref)
    import helpers.metrics_3dfront as M
    import helpers.util as U
    return M, U


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    M, U = reference(ap.parse_args().ref)
    import scipy
    import sklearn
    out = {'numpy_version': np.array(np.__version__), 'sklearn_version': np.array(sklearn.__version__),
           'scipy_version': np.array(scipy.__version__)}
    err, n_counts, least = 0.0, 0, np.inf
    for name in R.CASES:
        c = R.case(name)
        pairs, skipped = R.eligible_pairs(c['objs'], c['triples'], R.VOCAB, c['offsets'])
        counts = []
        if c['placed']:
            fits = c['clouds']
            for i, j in pairs.tolist():
                counts.append(int(M.pointcloud_overlap_pair(c['clouds'][i], c['clouds'][j])))
        else:
            boxes = torch.from_numpy(c['boxes'])
            fits = np.stack([U.fit_shapes_to_box(boxes[o].clone(), torch.from_numpy(c['clouds'][o]).clone()) for o in range(len(boxes))])
            assert fits.dtype == np.float32
            err = max(err, float(np.abs(fits - R.fit64_all(c['boxes'], c['clouds'])).max()))
            for nodes, triples in R.scenes(c):
                b = boxes[nodes]
                got = M.pointcloud_overlap([torch.from_numpy(x) for x in c['clouds'][nodes]], torch.from_numpy(c['objs'][nodes]), b[:, :6],
                                           b[:, 6], torch.from_numpy(triples), R.VOCAB, [])
                counts += [int(v) for v in got]
        assert len(counts) == len(pairs), (name, len(counts), len(pairs))
        for up, cc in (('z', c),) + ((('y', R.swap_yz(c)),) if name == 'room' else ()):
            m = R.margins(R.placed_of(cc, up, yardstick=True), pairs)
            worst = min(v for _, v in m)
            assert worst >= R.MARGIN, 'case %s (up=%s): a query point is %.3g from a tie; choose another seed' % (name, up, worst)
            assert [n for n, _ in m] == counts, (name, up, [n for n, _ in m], counts)
            least = min(least, worst)
        if name == 'apart':
            placed = R.placed_of(c)
            lo, hi = placed.min(1), placed.max(1)
            assert all((lo[i] > hi[j]).any() or (lo[j] > hi[i]).any() for i, j in pairs.tolist()) and not any(counts)
        else:
            assert max(counts) > 0 and all(v > 0 for v in skipped.values()), (name, counts, skipped)
        out[name + '/counts'] = np.array(counts, np.int32)
        out[name + '/fit'] = fits
        n_counts += len(counts)
    bar = 4 * err
    assert R.MARGIN >= 8 * bar, 'MARGIN %.3g is below 8 x the coordinate bar %.3g' % (R.MARGIN, bar)
    out['ref_fit_err'] = np.float64(err)
    path = os.path.join(HERE, 'scene_overlap.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB): %d counts of the reference under numpy %s, scikit-learn %s; reference fit error %.3g, bar %.3g, least margin '
          '%.3g (MARGIN %.3g)' % (path, os.path.getsize(path) / 1024, n_counts, np.__version__, sklearn.__version__, err, bar, least, R.MARGIN))


if __name__ == '__main__':
    main()
