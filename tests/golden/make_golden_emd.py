#!/usr/bin/env python
"""Goldens of the earth mover's distance (echoscene_amd/shape_metrics.py ``pairwise_emd``, ``compute_all_metrics(..., emd=True)``) from
the reference's scripts/compute_mmd_cov_1nn.py, run on CPU tensors through its exact route (emd_approx: fp32 distances, the host
assignment solver); open3d, which the script imports for a viewer only, is replaced by an empty module.

    python tests/golden/make_golden_emd.py --ref <checkout of the reference>     # writes tests/golden/emd.npz

Recorded (the clouds themselves are not: tests/shape_metrics_ref.py and tests/emd_ref.py rebuild them from their seeds):
  emd_<P>             emd_approx for the 5 x 4 clouds of R.golden_sets(P), P in {17, 257}, fp32
  M_rs, M_rr, M_ss    the EMD matrices of _pairwise_EMD_CD_(..., accelerated_emd=False) for the two metric sets
  all_*               the six EMD entries of compute_all_metrics for the two metric sets
  ref_fp32_emd_err    max |emd_approx in fp32 - float64 yardstick| over every pair the GPU tests check against the yardstick (a x b,
                      a x a and b x b of emd_ref.MATRIX_P, the golden sets, the metric sets, the duplicate-heavy clouds)
  ref_fp32_emd_err_by_P   the same per P of emd_ref.MATRIX_P (for the notes)
The rank-based goldens are recorded only after the float64 yardstick shows a margin of 10 x (EMD_EPS + 4 x ref_fp32_emd_err) between
the candidates of each minimum."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emd_ref as E  # noqa: E402
import shape_metrics_ref as R  # noqa: E402


def reference(ref):
    sys.modules.setdefault('open3d', types.ModuleType('open3d'))
    sys.path.insert(0, os.path.join(ref, 'scripts'))
    import compute_mmd_cov_1nn as M
    return M


def emd_fp32(M, a, b):
    """the reference's emd_approx, every cloud of a against every cloud of b: float32 [Na, Nb]"""
    out = np.zeros((len(a), len(b)), np.float32)
    for i, x in enumerate(a):
        xs = torch.from_numpy(np.ascontiguousarray(x))[None].expand(len(b), -1, -1).contiguous()
        out[i] = M.emd_approx(xs, torch.from_numpy(np.ascontiguousarray(b))).numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    M = reference(ap.parse_args().ref)
    out, errs = {}, []

    for P in (17, 257):
        a, b = R.golden_sets(P)
        out['emd_%d' % P] = emd_fp32(M, a, b)
        errs.append(np.abs(out['emd_%d' % P].astype(np.float64) - E.emd_matrix(a, b)).max())

    smp, ref = R.metric_sets()
    ts, tr = torch.from_numpy(smp), torch.from_numpy(ref)
    y = {'M_rs': E.emd_matrix(ref, smp), 'M_rr': E.emd_matrix(ref), 'M_ss': E.emd_matrix(smp)}
    for name, (p, q) in (('M_rs', (tr, ts)), ('M_rr', (tr, tr)), ('M_ss', (ts, ts))):
        out[name] = M._pairwise_EMD_CD_(p, q, batch_size=4, accelerated_cd=False, accelerated_emd=False)[1].numpy()
        assert out[name].dtype == np.float32
        errs.append(np.abs(out[name].astype(np.float64) - y[name]).max())
    for k, v in M.compute_all_metrics(ts, tr, batch_size=4, accelerated_cd=False).items():
        if 'EMD' in k:
            out['all_' + k] = np.float32(v)
    assert len([k for k in out if k.startswith('all_')]) == 6

    for x, yy in E.adversarial_cases().values():
        errs.append(abs(float(emd_fp32(M, x[None], yy[None])[0, 0]) - E.emd_pair(x, yy)))

    by_P = []
    for P in E.MATRIX_P:
        a, b = E.matrix_case(P)
        e = [np.abs(emd_fp32(M, a, b).astype(np.float64) - E.emd_matrix(a, b)).max()]
        e += [np.abs(emd_fp32(M, x, x).astype(np.float64) - E.emd_matrix(x)).max() for x in (a, b) if len(x) > 1]
        by_P.append(max(e))
        print('  P = %d: %.3g' % (P, by_P[-1]), flush=True)
    out['ref_fp32_emd_err_by_P'] = np.array(by_P)
    out['ref_fp32_emd_err'] = np.float64(max(by_P + errs))

    # the input condition of the end-to-end test, on the yardstick
    gaps = R.rank_margins(y['M_rs'], y['M_rr'], y['M_ss'])
    assert min(gaps) >= 10 * (E.EMD_EPS + 4 * out['ref_fp32_emd_err']), (gaps, out['ref_fp32_emd_err'])

    path = os.path.join(HERE, 'emd.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB); reference fp32 error: %.3g overall' % (path, os.path.getsize(path) / 1024, out['ref_fp32_emd_err']))
    print('   golden / metric sets / adversarial', ['%.3g' % e for e in errs], 'rank margins (COV, k-NN)', gaps)


if __name__ == '__main__':
    main()
