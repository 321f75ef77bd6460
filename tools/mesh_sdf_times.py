"""Times of mesh -> SDF (es_mesh_sdf: frame + preparation + grid kernel) at n = 64 for K = 1 and K = 8 meshes of about 1e3, 1e4 and
1e5 triangles (tori of a x b quads), by HIP events around the library call after a warm-up call, median of 5; the whole Python call
(packing, workspace, flag read-back) next to it.  Prints the point-triangle pairs per second and, with --valu-per-pair N (the
vector instructions of the grid kernel's inner loop, counted from the ISA), the share of the fp32 vector issue rate:
pairs/s * N / (256 CUs * 4 SIMDs * 2.4e9 / 2 wave-instructions per SIMD and second * 64 lanes).

  python tools/mesh_sdf_times.py [--valu-per-pair 137] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoscene_amd import hip                                       # noqa: E402
from echoscene_amd.postprocess import mesh_to_sdf                   # noqa: E402


def torus(a, b, R=0.3, r=0.12):
    """closed, outward, 2 a b triangles"""
    u, v = np.meshgrid(np.arange(a) * 2 * np.pi / a, np.arange(b) * 2 * np.pi / b, indexing='ij')
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing='ij')
    p = lambda di, dj: (((i + di) % a) * b + (j + dj) % b).reshape(-1)
    faces = np.concatenate([np.stack([p(0, 0), p(1, 0), p(1, 1)], -1), np.stack([p(0, 0), p(1, 1), p(0, 1)], -1)])
    return torch.from_numpy(verts.astype(np.float32)).cuda(), torch.from_numpy(faces).cuda()


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--valu-per-pair', type=int, default=0)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    L = hip.lib()
    n = args.n
    lines = ['device: %s; n = %d; median of 5 after a warm-up call' % (torch.cuda.get_device_name(0), n),
             '%8s %3s %12s %12s %14s %s' % ('T', 'K', 'library ms', 'python ms', 'pairs/s', 'share of fp32 vector issue')]
    for a, b in ((25, 20), (100, 50), (400, 125)):
        v, f = torus(a, b)
        w = mesh_to_sdf([(v, f)], n=16, fit=None)
        assert -0.125 < w.min().item() < -0.05 and w.max().item() == np.float32(0.2)        # a torus of tube radius 0.12 came out
        for K in (1, 8):
            T = f.shape[0]
            verts, faces = torch.cat([v] * K), torch.cat([f.int()] * K).contiguous()
            vo = torch.arange(K + 1, device='cuda') * v.shape[0]
            to = torch.arange(K + 1, device='cuda') * T
            ws = torch.empty(L.es_mesh_sdf_workspace(K, K * T), dtype=torch.uint8, device='cuda')
            bad = torch.empty(K, dtype=torch.int32, device='cuda')
            out = torch.empty(K, n, n, n, device='cuda')
            p = lambda t: C.c_void_p(t.data_ptr())
            call = lambda: hip.check(L.es_mesh_sdf(p(verts), p(faces), p(vo), p(to), K, K * v.shape[0], K * T, n, 0.2, 0.0, p(ws), p(bad),
                                                   None, p(out), hip.current_stream()), 'es_mesh_sdf')
            ms = median_ms(call)
            assert int(bad.sum()) == 0
            ms_py = median_ms(lambda: mesh_to_sdf([(v, f)] * K, n=n, fit=None))
            rate = K * n ** 3 * T / (ms * 1e-3)
            share = '%.1f%%' % (100 * rate * args.valu_per_pair / (256 * 4 * 1.2e9 * 64)) if args.valu_per_pair else 'n/a'
            lines.append('%8d %3d %12.3f %12.3f %14.3e %s' % (T, K, ms, ms_py, rate, share))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text + '\n')


if __name__ == '__main__':
    main()
