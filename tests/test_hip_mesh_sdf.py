"""GPU tests of mesh -> SDF (csrc/es_mesh_sdf.hip through postprocess.mesh_to_sdf) against the float64 reference of
tests/mesh_sdf_ref.py (pinned to closed forms in tests/test_mesh_sdf_cpu.py).

Bar: max |gpu - ref64| <= 1e-6 over ALL voxels, the clamp included.  Basis: the reference itself evaluated in float32 differs from
float64 by at most 4.2e-8 on the clamped output (7.8e-8 on the raw distance) over these meshes and grids; 1e-6 leaves about 12x for FMA
contraction and the kernel's different formulation.  A wrong sign at a voxel with d > 5e-7 fails the same comparison.  The inputs
must keep the comparison well conditioned, which each test asserts on the reference: no voxel within 0.02 of the winding threshold
0.5, no grid point within 1e-5 of a surface.  The device sees float32 vertices, so the reference is evaluated on the rounded ones."""
import numpy as np
import pytest
import torch

import mesh_sdf_ref as R
from echoscene_amd.postprocess import marching_cubes_batch, mesh_to_sdf

pytestmark = pytest.mark.gpu
TOL = 1e-6
W_MARGIN, D_MARGIN = 0.02, 1e-5
_REF = {}


def ref_of(name, n):
    """the reference of a named mesh, computed once per (mesh, grid) and shared"""
    if (name, n) not in _REF:
        v, f = R.MESHES[name]()
        r = R.sdf_ref(R.as_f32(v), f, n)
        for a in r.values():
            a.setflags(write=False)
        _REF[(name, n)] = r
    return _REF[(name, n)]


def on_device(v, f):
    return torch.from_numpy(np.asarray(v, np.float32)).cuda(), torch.from_numpy(np.asarray(f, np.int64)).cuda()


def well_conditioned(r, what):
    wm, dm = np.abs(r['w'] - 0.5).min(), r['d'].min()
    print('%s: min |w - 0.5| = %.4f, min d = %.3e' % (what, wm, dm))
    assert wm >= W_MARGIN and dm >= D_MARGIN, what


def err_of(got, r, what):
    got = got.detach().cpu().numpy().astype(np.float64).reshape(r['sdf'].shape)
    assert np.isfinite(got).all()
    e = np.abs(got - r['sdf']).max()
    print('%s: max |gpu - ref64| = %.3e' % (what, e))
    return e


# ------------------------------------------------------------------------------------------------ 1. every mesh against the reference
@pytest.mark.parametrize('n', [8, 16])
@pytest.mark.parametrize('name', list(R.MESHES))
def test_mesh_vs_float64_reference(name, n):
    """a closed cube, the cube with a face removed (open: the winding number decides), a rotated octahedron with a grid point 2.2e-5
    from a face (what a cancelling distance formula gets wrong), 768 and 767 triangles (six LDS tiles of 128; five and a remainder of
    127), two components"""
    r = ref_of(name, n)
    well_conditioned(r, '%s n=%d' % (name, n))
    out = mesh_to_sdf([on_device(*R.MESHES[name]())], n=n, fit=None)
    assert tuple(out.shape) == (1, 1, n, n, n) and out.dtype == torch.float32 and out.is_cuda
    assert err_of(out, r, '%s n=%d' % (name, n)) <= TOL


@pytest.mark.parametrize('n', [8, 16])
def test_batch_of_ragged_meshes_equals_single_calls_bitwise(n):
    """K = 6 with 8 .. 768 triangles and 6 .. 386 vertices in one call: every grid equals the grid of its own call bit for bit (a
    voxel's sums run over its mesh's triangles in their order, whatever else is in the batch), hence meets the reference too"""
    meshes = [on_device(*m()) for m in R.MESHES.values()]
    assert len({m[0].shape[0] for m in meshes}) > 3 and len({m[1].shape[0] for m in meshes}) == 6
    out = mesh_to_sdf(meshes, n=n, fit=None)
    assert tuple(out.shape) == (6, 1, n, n, n)
    for k, name in enumerate(R.MESHES):
        assert torch.equal(out[k:k + 1], mesh_to_sdf([meshes[k]], n=n, fit=None)), name
        assert err_of(out[k], ref_of(name, n), 'batched %s n=%d' % (name, n)) <= TOL


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_two_calls_give_the_same_bits():
    """no atomics, a fixed order: the same bits on every run; a single pair, float64 vertices holding float32 values and int32 faces
    are the same mesh"""
    v, f = on_device(*R.cube768())
    a = mesh_to_sdf([(v, f)], n=16)
    b = mesh_to_sdf([(v, f)], n=16)
    c = mesh_to_sdf((v.double(), f.int()), n=16)
    assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 3. zero-area triangles
def test_zero_area_triangles_change_nothing():
    """The cube plus two triangles without area, against the reference of the PLAIN cube at the same bar.

    (3, 3, 3): three equal corners.  In double its cross product is exactly zero: marked in the preparation, skipped by the grid kernel.

    (2, 8, 7): corners 2 = (-0.29, 0.28, -0.27) and 7 = (0.31, 0.28, 0.33) are the ends of the diagonal along which the +y face is
    split, vertex 8 = float32(v2 + (v7 - v2) / 3) lies between them: collinear up to the rounding of its x and z (half an ulp of 0.09
    and of 0.07, 3.7e-9 each, so at most delta = 5.3e-9 off the line), distinct, and with y = float32(0.28) exactly like the other
    two.  Whether the kernel marks it or evaluates it as the sliver it is:
      * it cannot win the minimum: all three corners lie in the plane of the +y face and inside that face, so does every point of the
        sliver, and every point of the face belongs to the cube's surface -- the distance from any voxel to the sliver is at least
        its distance to the cube;
      * it cannot move w past 0.5: a planar patch subtends at most area / d^2; area <= |v7 - v2| delta / 2 = 0.849 * 5.3e-9 / 2 =
        2.3e-9, and d >= 1e-3 (asserted below), so its solid angle is below 2.3e-3 and its share of w below 2.3e-3 / 4 pi = 1.8e-4,
        against a margin of 0.5 (the cube is closed: w is 0 or 1)."""
    n = 16
    v, f = R.cube()
    v32 = np.asarray(v, np.float32)
    v8 = (v32[2] + (v32[7] - v32[2]) / np.float32(3)).astype(np.float32)
    assert v8[1] == v32[2][1] == v32[7][1] and len({tuple(v32[2]), tuple(v8), tuple(v32[7])}) == 3
    v2 = np.concatenate([v32, v8[None]])
    f2 = np.concatenate([f, [[3, 3, 3], [2, 8, 7]]])
    r = ref_of('cube', n)
    well_conditioned(r, 'cube n=%d' % n)
    dmin = R.distance(R.grid_points(n), v2.astype(np.float64), f2).min()
    print('zero-area: min d over the mesh with the extra triangles = %.3e' % dmin)
    assert dmin >= 1e-3
    out = mesh_to_sdf([on_device(v2, f2)], n=n, fit=None)
    assert err_of(out, r, 'cube + zero-area triangles n=%d' % n) <= TOL


# ------------------------------------------------------------------------------------------------ 4. fit
def test_fit_centres_and_scales_on_the_device():
    """the octahedron scaled by 37 and moved to (5, -3, 2), fit = 0.9: the grid equals the reference of the mesh fitted in float64
    (centre of the bounding box, longest side -> 0.9) at the same bar; the returned transform equals the float64 one to 1e-6"""
    n = 16
    v, f = R.octa()
    big = R.as_f32(v * 37.0 + np.array([5.0, -3.0, 2.0]))
    centre, scale = R.fit_transform(big, 0.9)
    fitted = (big - centre) * scale
    assert abs((fitted.max(0) - fitted.min(0)).max() - 0.9) < 1e-12 and np.abs(fitted.max(0) + fitted.min(0)).max() < 1e-12
    r = R.sdf_ref(fitted, f, n)
    well_conditioned(r, 'fitted octa n=%d' % n)
    out, tf = mesh_to_sdf([on_device(big, f)], n=n, fit=0.9, return_transform=True)
    assert tuple(tf.shape) == (1, 4) and tf.dtype == torch.float32
    got = tf[0].cpu().numpy().astype(np.float64)
    want = np.concatenate([centre, [scale]])
    print('fit: transform %s, rel err %s' % (got, np.abs(got - want) / np.abs(want)))
    assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all()
    assert err_of(out, r, 'fitted octa n=%d' % n) <= TOL
    # without a fit the transform is the identity
    _, tf0 = mesh_to_sdf([on_device(v, f)], n=8, fit=None, return_transform=True)
    assert tf0.cpu().tolist() == [[0.0, 0.0, 0.0, 1.0]]


# ------------------------------------------------------------------------------------------------ 5. a face index outside the mesh
def test_face_index_equal_to_v_is_flagged_not_read():
    """index V (one past the last vertex) in the SECOND mesh of a batch: the preparation clamps it, raises that mesh's flag, and the
    wrapper turns the flag into a ValueError naming the mesh.  One call."""
    v, f = R.cube()
    bad = f.copy()
    bad[5, 1] = len(v)
    with pytest.raises(ValueError, match=r'meshes \[1\] have a face index outside'):
        mesh_to_sdf([on_device(v, f), on_device(v, bad)], n=8, fit=None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. round trip
def test_round_trip_through_marching_cubes():
    """s = mesh_to_sdf(cube768, n = 32), then the level-0 surface of s: every vertex marching cubes emits sits on a grid edge whose
    ends have opposite signs in s, so the true surface crosses that same edge, whose length is 1/n -- the vertex, mapped back by
    v / n - 0.5, lies within 1/n of the cube's surface (a derived bound; measured by the float64 reference)"""
    n = 32
    v, f = R.cube768()
    s = mesh_to_sdf([on_device(v, f)], n=n, fit=None)
    mv, mf = marching_cubes_batch(s, level=0.0)[0]
    assert mv.shape[0] > 1000 and mf.shape[0] > 2000
    pts = mv.cpu().numpy().astype(np.float64) / n - 0.5
    d = R.distance(pts, R.as_f32(v), f)
    print('round trip: %d vertices, max distance to the surface %.3e (1/n = %.3e)' % (len(pts), d.max(), 1.0 / n))
    assert d.max() <= 1.0 / n


# ------------------------------------------------------------------------------------------------ 7. one scene call
def test_scene_call_keeps_the_sdf_of_a_mesh():
    """sample_box_and_shape(keep_nodes=[1], keep_sdfs=mesh_to_sdf([octa], n=64)) on the tiny scene model of test_hip_keep: the call
    runs on the device tensor as it is and the kept row comes back bit for bit"""
    from conftest import load_golden
    from echoscene_amd import synth
    from test_hip_keep import _build_sgdiff, _rnd
    g = load_golden('scene_keep_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    sdf = mesh_to_sdf([on_device(*R.octa())], n=64)
    assert tuple(sdf.shape) == (1, 1, 64, 64, 64) and sdf.is_cuda
    assert sdf.min().item() == pytest.approx(-0.2) and sdf.max().item() == pytest.approx(0.2)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), int(g['seeds'][1]) + k) for k in range(4)])
    m = _build_sgdiff('echoscene')
    d = m.sample_box_and_shape(objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda(), gen_shape=True, keep_nodes=[1], keep_sdfs=sdf,
                               keep_noise=table, layout_noise=synth.layout_noise(O, 8, 100, seed=7), shape_noise=synth.shape_noise(seed=7))
    assert tuple(d['shapes'].shape) == (O, 1, 64, 64, 64)
    assert torch.equal(d['shapes'][1].cpu(), sdf[0].cpu())
    assert torch.isfinite(d['shapes']).all()
