"""GPU tests of the shape-set metrics: the Chamfer matrix kernel and the cloud normalisation (csrc/es_shape_metrics.hip) behind
echoscene_amd/shape_metrics.py, against the float64 brute-force yardstick of tests/shape_metrics_ref.py.

The bar of a matrix entry is not derived but measured on the reference: the largest |distChamfer in fp32 - yardstick| over the
entries of every matrix checked here (a x b, a x a and b x b of the 17 cases of MATRIX_CASES, the golden sets, the metric sets),
computed on the CPU by tests/golden/make_golden_shape_metrics.py and recorded as ``ref_fp32_err``, times 4 for another product order
and FMA contraction:

    ref_fp32_err = 3.57e-7 (the two 1-point clouds of case (2, 2, 64, 1) against each other; 1e-8 .. 2e-7 on the other cases
    up to P = 65, 2.6e-10 .. 1.9e-8 from P = 255 on)                                                BAR = 1.43e-6, absolute

Measured on an MI355X (profiles/shape_metrics_notes.md): the largest |kernel - yardstick| is 3.57e-7, on that same entry; 1.0e-7 or
less on every other case, 1.6e-9 at P ~ 2048; 6.0e-8 at most against the reference's recorded matrices.  Because one absolute bar
is loose for large clouds, whose entries the reference itself gets to 1e-9, the seams of the tiling are also tested on lattice
clouds on which fp32 is exact, where the kernel must return the yardstick's bits.  The normalisation's bar is built the same way:
the formula evaluated in float32 on the CPU is off by 3.6e-7 .. 1.3e-6 on the clouds below, times 4; the kernel works in double and
rounds once: 3.0e-8 measured.

Rank-based results (COV, 1-NN) are compared only after the yardstick itself shows that no two candidates of a minimum are closer
than 100 x BAR."""
import os

import numpy as np
import pytest
import torch

import shape_metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def S():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import shape_metrics
    return shape_metrics


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'shape_metrics.npz')))


@pytest.fixture(scope='module')
def BAR(G):
    return 4 * float(G['ref_fp32_err'])


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize('n', range(len(R.MATRIX_CASES)), ids=['%dx%d_P%d_Q%d' % c for c in R.MATRIX_CASES])
def test_matrix_against_the_float64_yardstick(S, BAR, n):
    """Na, Nb in {1, 2, 3}; P, Q in {1, 15, 16, 17, 63, 64, 65} and at the seams of the tiling: the wave's query block
    (R.WAVE_QUERIES = 64) +- 1, the pass of a workgroup (R.PASS_QUERIES = 256) +- 1, the LDS chunk (R.LDS_CHUNK = 2048) +- 1"""
    a, b = R.matrix_case(n)
    got = host(S.pairwise_chamfer(dev(a), dev(b)))
    assert got.shape == (a.shape[0], b.shape[0]) and got.dtype == np.float32
    err = np.abs(got - R.chamfer_matrix(a, b)).max()
    print('case %s: max |kernel - yardstick| = %.3g (bar %.3g)' % (R.MATRIX_CASES[n], err, BAR))
    assert err <= BAR
    for x in (a, b):                                                # the symmetric mode on each set
        sym = host(S.pairwise_chamfer(dev(x)))
        y = R.chamfer_matrix(x)
        assert np.array_equal(np.diag(sym), np.zeros(len(x), np.float32))
        err = np.abs(sym - y).max()
        print('   symmetric [%d, %d, 3]: %.3g' % (x.shape[0], x.shape[1], err))
        assert err <= BAR


@pytest.mark.parametrize('n', range(len(R.LATTICE_CASES)), ids=['P%d_Q%d' % c for c in R.LATTICE_CASES])
def test_matrix_is_exact_on_lattice_clouds(S, n):
    """coordinates that are multiples of 1/64: every fp32 operation of the expanded form is exact, so the entry is float32(yardstick)
    bit for bit; a planted mutual nearest pair sits at every seam index of the tiling (tests/shape_metrics_ref.py)"""
    a, b = R.lattice_case(n)
    want = R.chamfer_matrix(a, b).astype(np.float32)
    assert np.array_equal(host(S.pairwise_chamfer(dev(a), dev(b))), want)
    assert np.array_equal(host(S.pairwise_chamfer(dev(b), dev(a))), want.T)
    both = np.concatenate([a, b if a.shape[1] == b.shape[1] else -a])              # (the mirrored lattice cloud is a lattice cloud)
    sym = host(S.pairwise_chamfer(dev(both)))
    assert np.array_equal(sym, R.chamfer_matrix(both).astype(np.float32)) and sym[0, 0] == 0 and sym[1, 1] == 0


def test_matrix_against_the_recorded_matrices_of_the_reference(S, G, BAR):
    """the reference's _pairwise_EMD_CD_ on the CPU, 5 x 4 clouds of 17 and of 257 points: the kernel is within BAR of the truth and the
    recording within ref_fp32_err of it"""
    for P in (17, 257):
        a, b = R.golden_sets(P)
        got = host(S.pairwise_chamfer(dev(a), dev(b)))
        err = np.abs(got.astype(np.float64) - G['cd_%d' % P]).max()
        print('P = %d: max |kernel - reference| = %.3g' % (P, err))
        assert err <= BAR + float(G['ref_fp32_err'])
        assert np.abs(got - R.chamfer_matrix(a, b)).max() <= BAR


def test_all_metrics_end_to_end(S, G, BAR):
    smp, ref = R.metric_sets()
    y_rs, y_rr, y_ss = R.chamfer_matrix(ref, smp), R.chamfer_matrix(ref), R.chamfer_matrix(smp)
    gaps = R.rank_margins(y_rs, y_rr, y_ss)
    print('rank margins (COV, k-NN) %s, 100 x BAR = %.3g' % (gaps, 100 * BAR))
    assert min(gaps) >= 100 * BAR                                   # a condition on the inputs, asserted on the yardstick
    got = S.compute_all_metrics(dev(smp), dev(ref), batch_size=4, accelerated_cd=True)
    keys = ('lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc')
    assert tuple(got) == keys
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
        print('%s: %.9g (reference %.9g)' % (k, float(v), float(G['all_' + k])))
    for k in ('lgan_cov-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc'):
        assert float(got[k]) == float(G['all_' + k]), k
    for k in ('lgan_mmd-CD', 'lgan_mmd_smp-CD'):                    # a mean of minima: each within BAR of the truth, the recording within its own error
        assert abs(float(got[k]) - float(G['all_' + k])) <= BAR + float(G['ref_fp32_err']) + 2.0 ** -22 * float(G['all_' + k]), k
    d = dev(smp)
    assert float(S.compute_all_metrics(d, d)['lgan_mmd-CD']) == 0.0 and float(S.compute_all_metrics(d, d)['lgan_cov-CD']) == 1.0


# ------------------------------------------------------------------------------------------------ bitwise properties
def test_entries_depend_on_their_two_clouds_alone(S):
    a, b = R.golden_sets(257)
    a, b = dev(a), dev(b)
    full = S.pairwise_chamfer(a, b)
    assert torch.equal(full, S.pairwise_chamfer(a, b))                              # two runs
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            assert torch.equal(S.pairwise_chamfer(a[i:i + 1], b[j:j + 1])[0, 0], full[i, j]), (i, j)
    assert torch.equal(full, S.pairwise_chamfer(b, a).t())                          # the order of the arguments
    sym, gen = S.pairwise_chamfer(a), S.pairwise_chamfer(a, a)
    off = ~torch.eye(a.shape[0], dtype=torch.bool, device=a.device)
    assert torch.equal(sym[off], gen[off]) and torch.equal(sym.diagonal(), torch.zeros_like(sym.diagonal()))
    assert torch.equal(sym, sym.t()) and torch.equal(sym, S.pairwise_chamfer(a))
    # unequal point counts, over the LDS chunk on one side
    n = [k for k, c in enumerate(R.MATRIX_CASES) if c == (2, 2, R.LDS_CHUNK + 1, 17)][0]
    a, b = (dev(x) for x in R.matrix_case(n))
    full = S.pairwise_chamfer(a, b)
    assert torch.equal(full, S.pairwise_chamfer(b, a).t()) and torch.equal(full[1:, :1], S.pairwise_chamfer(a[1:], b[:1]))
    assert torch.equal(S.pairwise_chamfer(a.double(), b.half().float()), S.pairwise_chamfer(a, b.half().float()))      # other float types are cast


# ------------------------------------------------------------------------------------------------ clouds
@pytest.fixture(scope='module')
def meshes():
    """two analytic SDFs at n = 16 through marching_cubes_batch (a sphere and a box), and a bare vertex tensor of 40 points"""
    from echoscene_amd.postprocess import marching_cubes_batch
    n = 16
    g = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1) / float(n) - 0.5)
    sphere = np.linalg.norm(g - np.array([0.02, -0.01, 0.03]), axis=-1) - 0.3
    q = np.abs(g - np.array([-0.03, 0.02, 0.01])) - np.array([0.3, 0.2, 0.15])
    box = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    out = marching_cubes_batch(dev(np.stack([sphere, box]).astype(np.float32)), 0.02)
    assert all(v.shape[0] >= 257 for v, _ in out)
    return out + [out[0][0][5:45].clone()]


@pytest.mark.parametrize('number', (1, 63, 64, 65, 257))
def test_point_clouds_against_the_float64_normalisation(S, meshes, number):
    got = S.point_clouds(meshes, number=number)
    assert got.shape == (3, number, 3) and got.dtype == torch.float32 and got.is_cuda
    got = host(got)
    verts = [host(m[0] if isinstance(m, tuple) else m) for m in meshes]
    assert [len(v) >= number for v in verts] == [True, True, number <= 40]          # n >= number and n < number
    gathered = [v[S.sample_indices(len(v), number)] for v in verts]
    if number == 1:
        assert np.isnan(got).all()                                                  # 0 / 0, as documented
        return
    base = max(np.abs(R.normalize_f32(x) - R.normalize(x)).max() for x in gathered)
    err = max(np.abs(got[k] - R.normalize(x)).max() for k, x in enumerate(gathered))
    print('number %d: max |kernel - float64| = %.3g, float32 formula %.3g (bar 4 x)' % (number, err, base))
    assert 0 < base < 1e-5 and err <= 4 * base
    assert np.abs(got).reshape(3, -1).max(1).tolist() == [1.0, 1.0, 1.0]
    assert torch.equal(S.point_clouds(meshes[1], number=number)[0], S.point_clouds(meshes, number=number)[1])       # one pair is K = 1
    assert torch.equal(S.point_clouds(meshes[2], number=number)[0], S.point_clouds(meshes, number=number)[2])       # one tensor too


def test_a_point_index_outside_its_cloud_is_flagged(S, meshes):
    """through the C entry point (the public call cannot produce one): the index is clamped on the device, never dereferenced as given,
    the cloud is flagged and the wrapper raises"""
    verts = torch.cat([meshes[0][0], meshes[2]]).contiguous()
    n0, n1 = meshes[0][0].shape[0], meshes[2].shape[0]
    vofs = np.array([0, n0, n0 + n1])
    index = np.stack([S.sample_indices(n0, 64), S.sample_indices(n1, 64)])
    assert S._normalize(verts, vofs, index, 'test').shape == (2, 64, 3)
    for bad in (n1, -1):                                                            # n1 is a valid row of the packed array, not of cloud 1
        ix = index.copy()
        ix[1, 7] = bad
        with pytest.raises(ValueError, match=r'clouds \[1\] have a point index outside'):
            S._normalize(verts, vofs, ix, 'test')
    ix = index.copy()
    ix[0, 0], ix[1, 63] = n0, n1
    with pytest.raises(ValueError, match=r'clouds \[0, 1\]'):
        S._normalize(verts, vofs, ix, 'test')


def test_the_whole_path_from_sdf_grids_to_metrics(S, meshes):
    """SDF -> mesh -> point cloud -> matrix -> metrics, everything on the device: two shapes against themselves"""
    pcs = S.point_clouds(meshes[:2], number=257)
    m = S.compute_all_metrics(pcs, pcs)
    assert float(m['lgan_mmd-CD']) == 0.0 and float(m['lgan_cov-CD']) == 1.0
    cd = host(S.pairwise_chamfer(pcs))
    assert cd[0, 1] == cd[1, 0] > 0 and cd[0, 0] == cd[1, 1] == 0
