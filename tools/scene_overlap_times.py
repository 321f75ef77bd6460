"""Times of the scene metric (echoscene_amd/scene_metrics.py, csrc/es_scene_metrics.hip) for one scene of O objects x P points and every
pair i < j of it, next to the reference's route on host copies in the same process: a numpy fit (tests/scene_metrics_ref.py) and, per
pair, a scikit-learn kd-tree over both clouds queried for two neighbours, where scikit-learn can be imported; the numpy restatement of
the rule on a few pairs, scaled to all of them, where it cannot.  The output says which.

Arrangements:
  room         objects on a grid over a 6 m x 6 m floor, sizes 0.4 .. 1.6 m, random angles: neighbours touch, most pairs are decided by
               the bounds test before the first tile
  interleaved  every cloud fills the same box: no pair is pruned, and the lanes that do not count scan the whole second cloud, so
               every workgroup runs all P x P candidates -- the worst case; its rate is K * P * P over the pair pass
Per arrangement: medians and minima of overlap_counts (three launches, the status copy, a synchronise) on the host clock, and of the
three launches one by one between device events.

  python tools/scene_overlap_times.py [--objects 32] [--points 5000] [--reps 30] [--host-pairs 0]     (0: every pair on the host)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import scene_metrics_ref as R  # noqa: E402


def scene(kind, O, P, seed=0):
    rs = np.random.RandomState(seed)
    clouds = np.stack([R.raw_cloud(rs, P) for _ in range(O)])
    if kind == 'room':
        side = int(np.ceil(np.sqrt(O)))
        cells = np.array([(x, y) for x in range(side) for y in range(side)])[:O] * (6.0 / side) - 3.0 + 3.0 / side
        centres = np.concatenate([cells + rs.uniform(-0.2, 0.2, (O, 2)), rs.uniform(0.3, 0.6, (O, 1))], 1)
        boxes = np.concatenate([rs.uniform(0.4, 1.6, (O, 3)), centres, rs.uniform(-180, 180, (O, 1))], 1)
    else:
        clouds = rs.uniform(-0.5, 0.5, (O, P, 3)).astype(np.float32)
        boxes = np.tile(np.array([[2.0, 2.0, 2.0, 0.0, 0.0, 1.0, 30.0]]), (O, 1))
    return clouds, boxes.astype(np.float32)


def timed(f, n):
    xs = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        xs.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(xs)), 1e6 * float(np.min(xs))


def host_route(placed, pairs):
    """(counts, seconds, name of the route)"""
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        NearestNeighbors = None
    t0 = time.perf_counter()
    if NearestNeighbors is not None:
        out = []
        for i, j in pairs:
            tree = NearestNeighbors(n_neighbors=2, algorithm='kd_tree').fit(np.concatenate([placed[i], placed[j]]))
            out.append(int((tree.kneighbors(placed[i])[1] >= len(placed[i])).sum()))
        return out, time.perf_counter() - t0, 'scikit-learn kd-tree'
    return R.overlap_counts(placed, pairs), time.perf_counter() - t0, 'numpy restatement'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=32)
    ap.add_argument('--points', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--host-pairs', type=int, default=0)
    a = ap.parse_args()
    import torch
    from echoscene_amd import scene_metrics as M
    print(torch.cuda.get_device_name(0))
    O, P = a.objects, a.points
    pairs = np.array([(i, j) for i in range(O) for j in range(i + 1, O)], np.int32)
    K = len(pairs)
    fmt = 'median %.1f us  min %.1f us'
    for kind in ('room', 'interleaved'):
        clouds, boxes = scene(kind, O, P)
        t0 = time.perf_counter()
        placed = R.fit_all(boxes, clouds)
        t_fit = time.perf_counter() - t0
        sub = pairs if a.host_pairs <= 0 else pairs[np.random.RandomState(1).choice(K, min(K, a.host_pairs), replace=False)]
        want, t_pairs, route = host_route(placed, sub.tolist())
        host_s = t_fit + t_pairs * K / len(sub)
        print('%s: O %d, P %d, K %d pairs; host: numpy fit %.1f ms + %s on %d pairs %.2f s -> %.2f s for the scene'
              % (kind, O, P, K, 1e3 * t_fit, route, len(sub), t_pairs, host_s), flush=True)
        dc, db, dp = torch.from_numpy(clouds).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(pairs).cuda()
        got = M.overlap_counts(dc, db, dp).cpu().numpy()
        torch.cuda.synchronize()
        idx = {tuple(p): n for n, p in enumerate(pairs.tolist())}
        mine = np.array([got[idx[tuple(p)]] for p in sub.tolist()])
        diff = mine - np.array(want)
        print('  counts: %d of %d pairs above 0, sum %d; pairs that differ from the host route: %d (largest difference %d)'
              % (int((got > 0).sum()), K, int(got.sum()), int((diff != 0).sum()), int(np.abs(diff).max())))
        assert np.array_equal(M.fit_shapes_to_box(db, dc).cpu().numpy(), placed)

        def whole():
            M.overlap_counts(dc, db, dp)
            torch.cuda.synchronize()
        for _ in range(3):
            whole()
        med, lo = timed(whole, a.reps)
        print('  overlap_counts (3 launches, status copy, sync)   ' + fmt % (med, lo) + '   host / device = %.0f' % (1e6 * host_s / med))
        status = torch.empty(1 + O, dtype=torch.int32, device='cuda')
        counts = torch.empty(K, dtype=torch.int32, device='cuda')
        fitted, bounds = M._fit(dc, db, True, 'z', status[1:])
        d11 = M._self_nn(fitted)
        steps = (('fit', lambda: M._fit(dc, db, True, 'z', status[1:])), ('self pass', lambda: M._self_nn(fitted)),
                 ('pair pass', lambda: M._overlap(fitted, d11, fitted, bounds, dp, counts, status[:1])))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for name, f in steps:
            f()
            torch.cuda.synchronize()
            ks = []
            for _ in range(a.reps):
                ev[0].record()
                f()
                ev[1].record()
                torch.cuda.synchronize()
                ks.append(1e3 * ev[0].elapsed_time(ev[1]))
            med = float(np.median(ks))
            work = {'fit': '', 'self pass': '   %.2e point pairs / s' % (O * P * P / (1e-6 * med)),
                    'pair pass': '   %.2e point pairs / s if every pair ran P x P' % (K * P * P / (1e-6 * med))}[name]
            print('  %-10s between two events                   ' % name + fmt % (med, float(np.min(ks))) + work, flush=True)


if __name__ == '__main__':
    main()
