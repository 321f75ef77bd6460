"""Times of the layout metrics (echoscene_amd/layout_metrics.py, csrc/es_layout_metrics.hip) for one scene and for a test set of
scenes concatenated with node offsets, next to the numpy restatement of the same rules (tests/layout_metrics_ref.py) run on host
copies in the same process.  Scenes are layout_metrics_ref.random_scene: O boxes, T triples over 16 predicates, 11 with a rule.

Per size: the restatement once (whose verdicts the kernel must return), then medians and minima of wall-clock calls of
validate_constrains (launch, one copy, the Python lists), relation_accuracy (launch, 96 bytes to the host), relation_verdicts
(launch, the status word to the host), of the two memsets and the kernel between two device events, and of box3d_iou on the (s, o)
pairs of the triples.

  python tools/layout_metrics_times.py [--scenes 1 1000] [--boxes 32] [--triples 127] [--host]      (--host: the restatement alone)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import layout_metrics_ref as R  # noqa: E402


def scenes(n, O, T):
    bs, ts = [], []
    for i in range(n):
        b, t = R.random_scene(1000 + i, O, T)
        bs.append(b)
        ts.append(t + np.array([i * O, 0, i * O]))
    return np.concatenate(bs), np.concatenate(ts)


def timed(f, n):
    xs = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        xs.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(xs)), 1e6 * float(np.min(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, nargs='+', default=[1, 1000])
    ap.add_argument('--boxes', type=int, default=32)
    ap.add_argument('--triples', type=int, default=127)
    ap.add_argument('--host', action='store_true')
    a = ap.parse_args()
    if not a.host:
        import torch
        from echoscene_amd import layout_metrics as M
        print(torch.cuda.get_device_name(0))
    for n in a.scenes:
        b, t = scenes(n, a.boxes, a.triples)
        t0 = time.perf_counter()
        want = R.check(t, b)
        print('scenes %d: O %d, T %d; numpy restatement on host copies: %.1f ms' % (n, len(b), len(t), 1e3 * (time.perf_counter() - t0)), flush=True)
        if a.host:
            continue
        db, dt = torch.from_numpy(b).cuda(), torch.from_numpy(t).cuda()
        rule, ok = M.relation_verdicts(dt, db, R.VOCAB)
        assert np.array_equal(rule.cpu().numpy(), want[0]) and np.array_equal(ok.cpu().numpy(), want[1])
        torch.cuda.synchronize()
        reps = 200 if n == 1 else 30
        fmt = 'median %.1f us  min %.1f us'
        print('  validate_constrains (launch, copy, lists)   ' + fmt % timed(lambda: M.validate_constrains(dt, db, None, None, R.VOCAB, R.empty_accuracy()), reps))
        print('  relation_accuracy   (launch, 96-byte copy)  ' + fmt % timed(lambda: M.relation_accuracy(dt, db, R.VOCAB), reps))
        print('  relation_verdicts   (launch, status copy)   ' + fmt % timed(lambda: M.relation_verdicts(dt, db, R.VOCAB), reps))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ks = []
        for _ in range(reps):
            ev[0].record()
            M._launch(dt, db, R.VOCAB, None, 'all', True, 0.3, True)
            ev[1].record()
            torch.cuda.synchronize()
            ks.append(1e3 * ev[0].elapsed_time(ev[1]))
        print('  memsets + kernel between two events         ' + fmt % (float(np.median(ks)), float(np.min(ks))))
        x, y = db[dt[:, 0]].contiguous(), db[dt[:, 2]].contiguous()

        def iou():
            M.box3d_iou(x, y, with_translation=True)
            torch.cuda.synchronize()
        iou()
        print('  box3d_iou of %d pairs (launch, sync)   ' % len(t) + fmt % timed(iou, reps))
        k = min(len(t), 2000)
        t0 = time.perf_counter()
        for p, q in zip(b[t[:k, 0]], b[t[:k, 2]]):
            R.box3d_iou(p, q, True)
        print('  numpy restatement of box3d_iou: %.1f us per pair' % (1e6 * (time.perf_counter() - t0) / k), flush=True)


if __name__ == '__main__':
    main()
