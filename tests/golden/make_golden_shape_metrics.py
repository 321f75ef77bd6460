#!/usr/bin/env python
"""Goldens of the shape-set metrics (echoscene_amd/shape_metrics.py) from the reference's scripts/compute_mmd_cov_1nn.py, run on CPU
tensors through its own fallbacks (distChamfer, the host assignment solver for EMD); open3d, which the script imports for a viewer
only, is replaced by an empty module.

    python tests/golden/make_golden_shape_metrics.py --ref <checkout of the reference>     # writes tests/golden/shape_metrics.npz

Recorded (the clouds themselves are not: tests/shape_metrics_ref.py rebuilds them from their seeds):
  idx_<n>_<number>, norm_<n>_<number>  sample_pc's indices (sample_pc of an index column) and normalization(sample_pc(verts)) in float64
  cd_<P>                               the CD matrix of _pairwise_EMD_CD_ for 5 x 4 clouds of P points, P in {17, 257}
  stat_* / knn1_* / knn3_* / knn1sqrt_*  lgan_mmd_cov and knn (k = 1, 3; k = 1 with sqrt=True) of recorded matrices (M_rs, M_rr, M_ss of
                                       the two metric sets)
  all_*                                the six CD entries of compute_all_metrics for the two metric sets
  ref_fp32_err                         max |distChamfer in fp32 - float64 yardstick| over the entries of every matrix the GPU tests
                                       check (a x b, a x a and b x b of MATRIX_CASES, the golden sets, the metric sets): the base of
                                       their error bar
  ref_fp32_err_by_case                 the same per case of MATRIX_CASES (for the notes)
Every rank-based golden is recorded only after the float64 yardstick shows a margin between the two candidates of each minimum."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import shape_metrics_ref as R  # noqa: E402


def reference(ref):
    sys.modules.setdefault('open3d', types.ModuleType('open3d'))
    sys.path.insert(0, os.path.join(ref, 'scripts'))
    import compute_mmd_cov_1nn as M
    return M


def cd_fp32(M, a, b):
    """the reference's expanded fp32 arithmetic, pair by pair: distChamfer -> dl.mean + dr.mean.  distChamfer indexes both clouds with
    the point count of the first, so it takes equal counts only: the smaller cloud is padded with copies of its first point, which
    changes no minimum of a real point, and the means are taken over the real points"""
    out = np.zeros((len(a), len(b)), np.float32)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            n = max(len(x), len(y))
            xp = np.concatenate([x, np.repeat(x[:1], n - len(x), 0)])
            yp = np.concatenate([y, np.repeat(y[:1], n - len(y), 0)])
            over_x, over_y = M.distChamfer(torch.from_numpy(xp)[None], torch.from_numpy(yp)[None])     # per y, per x
            out[i, j] = float(over_x[0, :len(y)].mean() + over_y[0, :len(x)].mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    M = reference(ap.parse_args().ref)
    out = {}

    # sampling and normalisation
    for n, number in R.SAMPLE_CASES:
        idx = M.sample_pc(np.arange(n, dtype=np.int64)[:, None], number=number)[:, 0]
        verts = R.sample_verts(n).astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            norm = M.normalization(M.sample_pc(verts.copy(), number=number))
        out['idx_%d_%d' % (n, number)] = idx.astype(np.int32)
        out['norm_%d_%d' % (n, number)] = norm
    # the clouds of the tests are normalised by the reference's rule: its own function leaves them as they are (up to rounding)
    for x in R.clouds(3, 3, 50):
        assert np.abs(M.normalization(x.astype(np.float64)) - x).max() < 2e-7

    # CD matrices of the reference's route
    errs = []
    for P in (17, 257):
        a, b = R.golden_sets(P)
        cd, _ = M._pairwise_EMD_CD_(torch.from_numpy(a), torch.from_numpy(b), batch_size=3, accelerated_cd=True)
        out['cd_%d' % P] = cd.numpy()
        errs.append(np.abs(cd.numpy().astype(np.float64) - R.chamfer_matrix(a, b)).max())

    # statistics, and the end-to-end metrics
    smp, ref = R.metric_sets()
    ts, tr = torch.from_numpy(smp), torch.from_numpy(ref)
    M_rs = M._pairwise_EMD_CD_(tr, ts, batch_size=4)[0]
    M_rr = M._pairwise_EMD_CD_(tr, tr, batch_size=4)[0]
    M_ss = M._pairwise_EMD_CD_(ts, ts, batch_size=4)[0]
    for name, m, y in (('M_rs', M_rs, R.chamfer_matrix(ref, smp)), ('M_rr', M_rr, R.chamfer_matrix(ref)), ('M_ss', M_ss, R.chamfer_matrix(smp))):
        out[name] = m.numpy()
        errs.append(np.abs(m.numpy().astype(np.float64) - y).max())
    for k, v in M.lgan_mmd_cov(M_rs.t()).items():
        out['stat_' + k] = np.float32(v)
    for kk in (1, 3):
        for k, v in M.knn(M_rr, M_rs, M_ss, kk, sqrt=False).items():
            out['knn%d_%s' % (kk, k)] = np.float32(v)
    for k, v in M.knn(M_rr, M_rs, M_ss, 1, sqrt=True).items():
        out['knn1sqrt_%s' % k] = np.float32(v)
    for k, v in M.compute_all_metrics(ts, tr, batch_size=4, accelerated_cd=True).items():
        if k.endswith('-CD') or '-CD-' in k:
            out['all_' + k] = np.float32(v)

    # the reference's own fp32 error on the matrices of the GPU tests
    by_case = []
    for n in range(len(R.MATRIX_CASES)):
        a, b = R.matrix_case(n)
        e = [np.abs(cd_fp32(M, a, b).astype(np.float64) - R.chamfer_matrix(a, b)).max()]
        e += [np.abs(cd_fp32(M, x, x).astype(np.float64) - R.chamfer_matrix(x)).max() for x in (a, b) if len(x) > 1]     # each set against itself
        by_case.append(max(e))
    out['ref_fp32_err_by_case'] = np.array(by_case)
    out['ref_fp32_err'] = np.float64(max(by_case + errs))

    # the margin of the rank-based goldens on the yardstick: 100 x the bar of the GPU tests (4 x the error above)
    y_rs, y_rr, y_ss = R.chamfer_matrix(ref, smp), R.chamfer_matrix(ref), R.chamfer_matrix(smp)
    gaps = R.rank_margins(y_rs, y_rr, y_ss)
    assert min(gaps) >= 100 * 4 * out['ref_fp32_err'], (gaps, out['ref_fp32_err'])

    path = os.path.join(HERE, 'shape_metrics.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB); reference fp32 error: %.3g overall' % (path, os.path.getsize(path) / 1024, out['ref_fp32_err']))
    for c, e in zip(R.MATRIX_CASES, by_case):
        print('  ', c, '%.3g' % e)
    print('   golden / metric sets', ['%.3g' % e for e in errs], 'rank margins (COV, k-NN)', gaps)


if __name__ == '__main__':
    main()
