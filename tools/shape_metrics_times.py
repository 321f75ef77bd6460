"""Two ways to the same matrix of Chamfer distances, N x N clouds of P points (default 128 x 128 of 2048), timed in one process:

  matrix : shape_metrics.pairwise_chamfer (es_chamfer_matrix: one workgroup per pair on the fp32 matrix instruction)
  rows   : the reference's route (_pairwise_EMD_CD_) on the per-point kernel: one cloud expanded against all the others through
           chamfer.chamferDist, dist and idx arrays written and read back, dl.mean(1) + dr.mean(1) per row

The two alternate, after a warm-up call each, in windows of at least --window seconds between device events; the time of a matrix
is the window over its count.  The matrices must agree within the bar of the GPU tests (4 x the reference's fp32 error recorded in
tests/golden/shape_metrics.npz).  Prints point pairs per second (2 N^2 P^2 per matrix) and the share of the fp32 matrix peak the
matrix kernel reaches (8 flop per pair with K = 4; 157.3 TFLOP/s).

With --emd-n N the matrix of earth mover's distances is timed too (shape_metrics.pairwise_emd, es_emd_matrix: one workgroup per
pair, an integer auction): N x N clouds of --emd-points points, a warm-up call on two clouds of that size and then --emd-calls calls
of the full matrix between device events, each reported; with them the bidding rounds the pairs took, the time of the symmetric
mode, and -- where scipy can be imported -- what the host route costs per pair on the same clouds: the reference's emd_approx step,
linear_sum_assignment on the fp32 distance matrix, over --host-pairs pairs, whose values the kernel must match within EMD_EPS.

  python tools/shape_metrics_times.py [--n 128] [--points 2048] [--window 1.0] [--rounds 3] [--out FILE]
                                      [--emd-n 128] [--emd-points 2048] [--emd-calls 2] [--host-pairs 2] [--no-cd]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from echoscene_amd.chamfer import chamferDist                       # noqa: E402
from echoscene_amd.shape_metrics import EMD_EPS, _emd_matrix, pairwise_chamfer, pairwise_emd          # noqa: E402


def clouds(N, P, seed):
    """ellipsoids, boxes and gaussians in turn, normalised as the metric script normalises (centred, max |coordinate| = 1)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(N):
        x = torch.randn(P, 3, generator=g, dtype=torch.float64)
        if i % 3 == 0:
            x = x / x.norm(dim=1, keepdim=True)
        elif i % 3 == 1:
            x = torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5
        x = x * (0.4 + torch.rand(3, generator=g, dtype=torch.float64))
        x = x - x.mean(0)
        out.append(x / x.abs().max())
    return torch.stack(out).float().cuda()


def by_rows(a, b, cd=chamferDist()):
    rows = []
    for i in range(a.shape[0]):
        dl, dr = cd(a[i].view(1, -1, 3).expand(b.shape[0], -1, -1).contiguous(), b)
        rows.append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
    return torch.cat(rows, dim=0)


def window(fn, seconds):
    """run fn until `seconds` have passed on the device; (ms per call, calls)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    calls = 0
    while True:
        fn()
        calls += 1
        e1.record()
        e1.synchronize()
        if e0.elapsed_time(e1) >= 1e3 * seconds:
            return e0.elapsed_time(e1) / calls, calls


def timed(fn):
    """one call between device events: (result, ms)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def emd_lines(N, P, calls, host_pairs):
    a, b = clouds(N, P, 1), clouds(N, P, 2)
    pairwise_emd(a[:1], b[:1])                                      # (the warm-up call: code object, LDS attribute)
    torch.cuda.synchronize()
    lines = ['EMD: %d x %d clouds of %d points' % (N, N, P)]
    for c in range(calls):
        m, ms = timed(lambda: pairwise_emd(a, b))
        lines.append('call %d matrix    %10.1f ms, %8.3f ms per pair; entries %.4f .. %.4f' % (c, ms, ms / (N * N), m.min().item(), m.max().item()))
    _, ms = timed(lambda: pairwise_emd(a))
    lines.append('symmetric mode (one set against itself, %d pairs): %.1f ms' % (N * (N - 1) // 2, ms))
    (m2, status, rounds), _ = timed(lambda: _emd_matrix(a, b, rounds=True))
    assert torch.equal(m2, m) and not status.any().item()           # runs repeat bit for bit
    r = rounds.double()
    lines.append('bidding rounds per pair: median %.0f, largest %.0f (%.2f P); one pair alone: %.1f ms'
                 % (r.median().item(), r.max().item(), r.max().item() / P, timed(lambda: pairwise_emd(a[:1], b[:1]))[1]))
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        lines.append('host route: scipy cannot be imported here, not measured')
        return lines
    host_ms, worst = [], 0.0
    for k in range(host_pairs):
        d = (a[k].cpu()[:, None, :] - b[k].cpu()[None, :, :]).norm(dim=-1).numpy()      # the reference's emd_approx on the CPU
        t0 = time.perf_counter()
        rows, cols = linear_sum_assignment(d)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        worst = max(worst, abs(float(d[rows, cols].mean()) - m[k, k].item()))
    lines.append('host route (linear_sum_assignment on the fp32 distances, this machine\'s CPU): %s ms per pair; max |kernel - host| = %.3g '
                 '(EMD_EPS %.3g)' % (', '.join('%.0f' % h for h in host_ms), worst, EMD_EPS))
    assert worst <= EMD_EPS + 4e-7, lines[-1]                        # (the host value carries its own fp32 rounding)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=128)
    ap.add_argument('--points', type=int, default=2048)
    ap.add_argument('--window', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default='')
    ap.add_argument('--emd-n', type=int, default=0, help='also time the EMD matrix of this many clouds a side (0: no)')
    ap.add_argument('--emd-points', type=int, default=2048)
    ap.add_argument('--emd-calls', type=int, default=2)
    ap.add_argument('--host-pairs', type=int, default=2)
    ap.add_argument('--no-cd', action='store_true', help='skip the Chamfer part')
    args = ap.parse_args()
    text = '' if args.no_cd else cd_text(args)
    if args.emd_n > 0:
        text += ('\n' if text else 'device: %s\n' % torch.cuda.get_device_name(0)) + \
            '\n'.join(emd_lines(args.emd_n, args.emd_points, args.emd_calls, args.host_pairs))
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text + '\n')


def cd_text(args):
    N, P = args.n, args.points
    bar = 4 * float(np.load(os.path.join(ROOT, 'tests', 'golden', 'shape_metrics.npz'))['ref_fp32_err'])
    a, b = clouds(N, P, 1), clouds(N, P, 2)
    m_new, m_old = pairwise_chamfer(a, b), by_rows(a, b)             # (the warm-up calls)
    torch.cuda.synchronize()
    diff = (m_new.double() - m_old.double()).abs().max().item()
    lines = ['device: %s; %d x %d clouds of %d points; windows of >= %.1f s, alternating' % (torch.cuda.get_device_name(0), N, N, P, args.window),
             'max |matrix - rows| = %.3g (bar %.3g); entries %.4f .. %.4f' % (diff, bar, m_old.min().item(), m_old.max().item())]
    assert diff <= bar, lines[-1]
    pairs = 2.0 * N * N * P * P
    t = {'matrix': [], 'rows': []}
    for r in range(args.rounds):
        for name, fn in (('matrix', lambda: pairwise_chamfer(a, b)), ('rows', lambda: by_rows(a, b))):
            ms, calls = window(fn, args.window)
            t[name].append(ms)
            lines.append('round %d %-6s %9.3f ms per matrix (%d calls) %10.3e pairs/s' % (r, name, ms, calls, pairs / (ms * 1e-3)))
    new, old = float(np.median(t['matrix'])), float(np.median(t['rows']))
    lines.append('median: matrix %.3f ms, rows %.3f ms, ratio %.2f; matrix kernel at %.1f%% of the fp32 matrix peak'
                 % (new, old, old / new, 100 * pairs * 8 / (new * 1e-3) / 157.3e12))
    ms_sym, _ = window(lambda: pairwise_chamfer(a), args.window)
    lines.append('symmetric mode (one set against itself): %.3f ms' % ms_sym)
    return '\n'.join(lines)


if __name__ == '__main__':
    main()
