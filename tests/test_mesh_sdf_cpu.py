"""CPU-only checks of mesh -> SDF (csrc/es_mesh_sdf.hip, postprocess.mesh_to_sdf): the additions to the C ABI, every refusal of the
launcher on the host and of the Python call, and the float64 reference of the GPU tests (tests/mesh_sdf_ref.py) against closed forms,
so that the yardstick is pinned by mathematics, not by code.  No device compute is called here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_sdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('es_mesh_sdf_workspace', 'es_mesh_sdf')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported(L):
    from echoscene_amd import hip, build
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip.EXPORTS and hasattr(raw, name), name
    assert 'es_mesh_sdf.hip' in build.SOURCES
    assert len(hip.EXPORTS['es_mesh_sdf'][1]) == 15 and hip.EXPORTS['es_mesh_sdf_workspace'][0] is C.c_size_t


def test_abi_version_and_op_size_did_not_move(L, tmp_path):
    from echoscene_amd import hip
    c = tmp_path / 'sz.c'
    c.write_text('#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){printf("%zu %d\\n", sizeof(es_op), ES_ABI_VERSION);return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, abi = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert size == C.sizeof(hip.Op) == 488
    assert abi == L.es_abi_version() == 10


def test_workspace_size(L):
    """K frames of four doubles, then one 36-float record per triangle"""
    assert L.es_mesh_sdf_workspace(1, 0) == 32
    assert L.es_mesh_sdf_workspace(3, 767) == 3 * 32 + 767 * 144
    assert L.es_mesh_sdf_workspace(0, 10) == 0 and L.es_mesh_sdf_workspace(2, -1) == 0


def test_launcher_refuses_bad_arguments_on_the_host(L):
    """every pointer, K, n, the two int32 limits, trunc and the workspace alignment are checked before anything is enqueued (no device
    is needed to get the refusal), and es_last_error names the function"""
    P = 4096                                                       # never dereferenced
    good = dict(verts=P, faces=P, vofs=P, tofs=P, K=2, total_V=16, total_T=24, n=16, trunc=0.2, fit=0.9, ws=P, bad=P, tf=P, sdf=P)
    order = ('verts', 'faces', 'vofs', 'tofs', 'K', 'total_V', 'total_T', 'n', 'trunc', 'fit', 'ws', 'bad', 'tf', 'sdf')

    def refused(**kw):
        a = dict(good, **kw)
        rc = L.es_mesh_sdf(*[a[k] for k in order], None)
        return rc != 0 and b'es_mesh_sdf' in L.es_last_error()
    for name in ('verts', 'faces', 'vofs', 'tofs', 'ws', 'bad', 'sdf'):
        assert refused(**{name: None}), name
        assert b'NULL' in L.es_last_error(), name
    for kw in (dict(K=0), dict(K=-3), dict(n=1), dict(n=0), dict(n=-64), dict(trunc=0.0), dict(trunc=-0.2), dict(trunc=float('nan')),
               dict(K=8192, n=64),                                # 8192 * 64^3 = 2^31
               dict(K=1, n=1291),                                 # 1291^3 > 2^31
               dict(total_T=2 ** 31), dict(total_T=-1), dict(total_V=2 ** 31), dict(total_V=-1),
               dict(fit=float('nan')), dict(ws=P + 8)):
        assert refused(**kw), kw
    assert refused(K=8192, n=64) and b'int32' in L.es_last_error()
    assert refused(total_T=2 ** 31) and b'int32' in L.es_last_error()


# ------------------------------------------------------------------------------------------------ the Python call
def test_mesh_to_sdf_refuses_before_any_device_work():
    """every ValueError of postprocess.mesh_to_sdf, on CPU tensors (which are themselves the last refusal: no device is touched)"""
    from echoscene_amd.postprocess import mesh_to_sdf
    v, f = (torch.from_numpy(a) for a in R.cube())
    v = v.float()
    ok = [(v, f)]
    for bad, what in (([], 'non-empty'), ((), 'non-empty'), (None, 'non-empty'), ([v], 'pair'), ([(v, f, f)], 'pair'),
                      ([(v.numpy(), f)], 'pair'),
                      ([(v[:, :2], f)], 'verts'), ([(v[None], f)], 'verts'), ([(v.long(), f)], 'verts'),
                      ([(v, f[:, :2])], 'faces'), ([(v, f.flatten())], 'faces'), ([(v, f.float())], 'faces'), ([(v, f.short())], 'faces'),
                      ([(v, f[:0])], 'no faces'), ([(v[:0], f)], 'no vertices'), (ok + [(v, f[:0])], 'mesh 1 has no faces')):
        with pytest.raises(ValueError, match=what):
            mesh_to_sdf(bad)
    for kw, what in ((dict(n=1), 'n must'), (dict(n=0), 'n must'), (dict(n=16.0), 'n must'), (dict(n=True), 'n must'),
                     (dict(trunc=0), 'trunc'), (dict(trunc=-0.2), 'trunc'), (dict(trunc=float('nan')), 'trunc'),
                     (dict(fit=0), 'fit'), (dict(fit=-1), 'fit'), (dict(fit=1.0001), 'fit'), (dict(fit=float('nan')), 'fit'),
                     (dict(n=2048), 'int32')):
        with pytest.raises(ValueError, match=what):
            mesh_to_sdf(ok, **kw)
    for meshes in (ok, (v, f), [(v.double(), f.int())]):           # well-formed, but on the host
        with pytest.raises(ValueError, match='not on the device'):
            mesh_to_sdf(meshes)
        with pytest.raises(ValueError, match='not on the device'):
            mesh_to_sdf(meshes, fit=None, n=8, return_transform=True)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_reference_equals_the_box_formula_on_the_cube():
    """the SDF of an axis-aligned box in closed form: |max(q, 0)| + min(max(q), 0) with q = |p - c| - h; to 1e-12, inside and outside,
    before the clamp and after it"""
    half, centre = 0.3, np.array([0.01, -0.02, 0.03])
    v, f = R.cube(half, centre)
    for n in (8, 16):
        r = R.sdf_ref(v, f, n)
        q = np.abs(R.grid_points(n) - centre) - half
        box = (np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)).reshape(n, n, n)
        assert (box < 0).sum() > 0 and (box > 0).sum() > 0
        assert np.abs(np.where(r['w'] > 0.5, -r['d'], r['d']) - box).max() <= 1e-12
        assert np.abs(r['sdf'] - np.clip(box, -0.2, 0.2)).max() <= 1e-12
        assert np.abs(r['w'] - (box < 0)).max() <= 1e-12              # closed and outward: w is 1 inside, 0 outside


def test_reference_follows_the_sphere_within_the_chord_error():
    """an inscribed polyhedron P of the sphere of radius r contains the ball of radius r - sag (sag: the largest gap between a face's
    plane and the sphere), and signed distances are monotone under inclusion: |p| - r <= sdf_P(p) <= |p| - r + sag at every point"""
    r = 0.3
    v, f = R.sphere(r, rounds=4)
    assert len(f) == 2048 and np.abs(np.linalg.norm(v, axis=1) - r).max() < 1e-15
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    plane = np.einsum('ij,ij->i', nrm, a)
    assert plane.min() > 0                                         # outward orientation
    sag = r - plane.min()
    assert 0 < sag < 0.01 * r
    p = R.grid_points(8)
    d, w = R.distance(p, v, f), R.winding(p, v, f)
    ball = np.linalg.norm(p, axis=1) - r
    inside = w > 0.5
    assert np.abs(w - inside).max() < 1e-9 and inside.sum() > 0 and (~inside).sum() > 0
    s = np.where(inside, -d, d)
    assert (s - ball).min() >= -1e-12 and (s - ball).max() <= sag + 1e-12


def test_meshes_of_the_gpu_tests_are_what_the_tests_assume():
    """triangle counts, orientation (a closed outward mesh has w = 1 at an inner point), the removed face, shared midpoints"""
    counts = {k: len(m()[1]) for k, m in R.MESHES.items()}
    assert counts == {'cube': 12, 'open_cube': 10, 'octa': 8, 'cube768': 768, 'cube767': 767, 'two': 24}
    assert len(R.cube768()[0]) == 6 * 81 - 12 * 9 + 8              # 9 x 9 points per face, edges and corners shared
    inner = {'cube': (0.01, -0.02, 0.03), 'octa': (0.02, 0.01, -0.03), 'cube768': (0.01, -0.02, 0.03), 'two': (0.21, 0.16, 0.11)}
    for k, p in inner.items():
        v, f = R.MESHES[k]()
        assert abs(R.winding(np.array([p]), v, f)[0] - 1.0) < 1e-12, k
        assert abs(R.winding(np.array([[0.49, 0.49, 0.49]]), v, f)[0]) < 1e-12, k
    v, f = R.open_cube()
    assert 0.5 < R.winding(np.array([[0.01, -0.02, 0.03]]), v, f)[0] < 1.0 - 1.0 / 6 + 1e-12      # the +z face (a sixth) is missing
    assert np.array_equal(np.unique(R.cube()[1][-2:]), [1, 3, 5, 7])
    # zero-area triangles are dropped: three equal corners, and three collinear ones
    v, f = R.cube()
    f2 = np.concatenate([f, [[3, 3, 3], [0, 8, 7]]])
    v2 = np.concatenate([v, [0.5 * (v[0] + v[7])]])
    assert len(R.drop_zero_area(v2, f2)) == 12
