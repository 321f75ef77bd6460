"""GPU tests of the earth mover's distance matrix (csrc/es_emd.hip) behind ``shape_metrics.pairwise_emd`` and
``compute_all_metrics(..., emd=True)``, against the yardstick of tests/emd_ref.py: the exact assignment of scipy on float64 distances.

The bar of a matrix entry is the kernel's stated guarantee plus the project's usual four times the reference's own fp32 error:

    BAR = EMD_EPS + 4 x ref_fp32_emd_err = 4e-6 + 4 x 1.15e-7 = 4.46e-6, absolute

``EMD_EPS`` is derived in the header of the kernel from its arithmetic; ``ref_fp32_emd_err`` is the largest |emd_approx in fp32 -
yardstick| over the pairs checked here, computed on the CPU by tests/golden/make_golden_emd.py (2e-8 .. 1.2e-7, the largest at
P = 17).  Measured on an MI355X (profiles/emd_notes.md): the largest |kernel - yardstick| is 5.4e-7 (at P = 2, where
nothing averages), 1.6e-7 from P = 15 on.

The kernel's seams are P = 1 (assigned directly), the 64 objects a wave scans per step and the 1024 threads of its workgroup; the
dynamic LDS request is proportional to P and has no tiers.  tests/test_emd_cpu.py shows the numpy restatement of the auction within
the guarantee on the same clouds; here the kernel must also return that restatement's bits and its round count.

Rank-based results (COV, 1-NN) are compared only after the yardstick itself shows that no two candidates of a minimum are closer
than 10 x BAR."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emd_ref as E
import shape_metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD_KEYS = ('lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc')
EMD_KEYS = tuple(k.replace('CD', 'EMD') for k in CD_KEYS)


@pytest.fixture(scope='module')
def S():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import shape_metrics
    return shape_metrics


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'emd.npz')))


@pytest.fixture(scope='module')
def BAR(S, G):
    assert S.EMD_EPS == E.EMD_EPS <= 1e-4
    return S.EMD_EPS + 4 * float(G['ref_fp32_emd_err'])


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize('P', E.MATRIX_P)
def test_matrix_against_the_exact_assignment(S, BAR, P):
    """(Na, Nb) over {1, 2, 3}^2; P in {1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257} and around the workgroup's 1024 threads
    (1023, 1024, 1025; one or two pairs there, the host solver takes 0.6 s per pair); the general and the symmetric mode"""
    a, b = E.matrix_case(P)
    got = host(S.pairwise_emd(dev(a), dev(b)))
    assert got.shape == (a.shape[0], b.shape[0]) and got.dtype == np.float32
    err = np.abs(got - E.emd_matrix(a, b)).max()
    print('P %d [%d x %d]: max |kernel - yardstick| = %.3g (bar %.3g)' % (P, a.shape[0], b.shape[0], err, BAR))
    assert err <= BAR
    for x in (a, b):                                                # the symmetric mode on each set
        sym = host(S.pairwise_emd(dev(x)))
        assert np.array_equal(np.diag(sym), np.zeros(len(x), np.float32)) and np.array_equal(sym, sym.T)
        if len(x) > 1:
            err = np.abs(sym - E.emd_matrix(x)).max()
            print('   symmetric [%d, %d, 3]: %.3g' % (x.shape[0], x.shape[1], err))
            assert err <= BAR


@pytest.mark.parametrize('P', (1, 2, 17, 64, 65, 257))
def test_kernel_and_restatement_are_the_same_algorithm(S, P):
    """the bits and the round count of the numpy restatement (tests/emd_ref.py ``auction``), pair by pair"""
    a, b = E.matrix_case(P)
    out, status, rounds = S._emd_matrix(dev(a), dev(b), rounds=True)
    assert not host(status).any()
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            v, r, _ = E.auction(x, y)
            assert host(out)[i, j].tobytes() == v.tobytes() and int(rounds[i, j]) == r, (i, j, float(out[i, j]), float(v), int(rounds[i, j]), r)
    print('P %d: rounds %s' % (P, host(rounds).tolist()))


@pytest.mark.parametrize('scale, shift, es', ((1000.0, 5000.0, {12}), (0.01, 0.0, {3}), (2.0, 0.0, {3, 4}), (2.5e5, -1e6, {20})))
def test_clouds_that_are_not_normalised_take_the_scale_of_their_bounding_box(S, scale, shift, es):
    """the scale exponent the device derives from the joint bounding box (e = 3 for extents below 4, then one more per doubling): the
    restatement's bits and rounds, and the guarantee EMD_EPS * 2^(e - 3) against the exact assignment on the same fp32 clouds.  Clouds
    twice the normalised size straddle the first step: a joint extent of exactly 4 is e = 4, anything below is e = 3"""
    a, b = R.clouds(5, 2, 65), R.clouds(6, 3, 65)
    a, b = a * np.float32(scale) + np.float32(shift), b * np.float32(scale) + np.float32(shift)
    assert {E.scale_exponent(x, y) for x in a for y in b} == es
    out, status, rounds = S._emd_matrix(dev(a), dev(b), rounds=True)
    assert not host(status).any()
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            v, r, _ = E.auction(x, y)
            assert host(out)[i, j].tobytes() == v.tobytes() and int(rounds[i, j]) == r, (i, j)
            assert abs(float(out[i, j]) - E.emd_pair(x, y)) <= S.EMD_EPS * 2 ** (E.scale_exponent(x, y) - 3), (i, j)


@pytest.mark.parametrize('P', (2049, 5000, 'EMD_MAX_POINTS'))
def test_permuted_lattice_translate_beyond_the_host_solver(S, P):
    """a lattice cloud against a permuted translate of itself by (3, 4, 0) / 64: 5/64 exactly (tests/emd_ref.py ``translate_case``), at
    sizes where the host solver takes 7 s and more per pair; 5000 is the reference script's point count"""
    P = S.EMD_MAX_POINTS if P == 'EMD_MAX_POINTS' else P
    x, y = E.translate_case(P)
    out, status, rounds = S._emd_matrix(dev(x[None]), dev(y[None]), rounds=True)
    print('P %d: %.9g (5/64 = %.9g), %d rounds' % (P, float(out), 5 / 64.0, int(rounds)))
    assert int(status) == 0 and abs(float(out) - 5 / 64.0) <= S.EMD_EPS
    assert int(rounds) < E.round_cap(P, 2 ** 23)[1] / 8


def test_matrix_against_the_recorded_matrices_of_the_reference(S, G, BAR):
    """the reference's emd_approx on the CPU, 5 x 4 clouds of 17 and of 257 points: the kernel is within BAR of the truth and the
    recording within ref_fp32_emd_err of it"""
    for P in (17, 257):
        a, b = R.golden_sets(P)
        got = host(S.pairwise_emd(dev(a), dev(b)))
        err = np.abs(got.astype(np.float64) - G['emd_%d' % P]).max()
        print('P = %d: max |kernel - reference| = %.3g' % (P, err))
        assert err <= BAR + float(G['ref_fp32_emd_err'])
        assert np.abs(got - E.emd_matrix(a, b)).max() <= BAR


# ------------------------------------------------------------------------------------------------ bitwise properties
def test_entries_depend_on_their_two_clouds_alone(S):
    a, b = R.golden_sets(257)
    a, b = dev(a), dev(b)
    full = S.pairwise_emd(a, b)
    assert torch.equal(full, S.pairwise_emd(a, b))                                  # two runs
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            assert torch.equal(S.pairwise_emd(a[i:i + 1], b[j:j + 1])[0, 0], full[i, j]), (i, j)
    sym, gen = S.pairwise_emd(a), S.pairwise_emd(a, a)
    off = ~torch.eye(a.shape[0], dtype=torch.bool, device=a.device)
    upper = torch.triu(off)
    assert torch.equal(sym[upper], gen[upper])                                      # the computed half: the general mode's bits
    assert torch.equal(sym, sym.t()) and torch.equal(sym.diagonal(), torch.zeros_like(sym.diagonal()))
    assert torch.equal(sym, S.pairwise_emd(a))
    assert gen.diagonal().abs().max() <= S.EMD_EPS                                  # (the general mode runs the auction on the diagonal too)
    assert (gen - gen.t()).abs().max() <= 2 * S.EMD_EPS                             # the other half: bidders and objects change roles
    assert torch.equal(S.pairwise_emd(a.double(), b.half().float()), S.pairwise_emd(a, b.half().float()))      # other float types are cast
    assert torch.equal(S.pairwise_emd(a.half(), b), S.pairwise_emd(a.half().float(), b))


# ------------------------------------------------------------------------------------------------ the metrics
def test_all_metrics_with_emd_end_to_end(S, G, BAR):
    smp, ref = R.metric_sets()
    y_rs, y_rr, y_ss = E.emd_matrix(ref, smp), E.emd_matrix(ref), E.emd_matrix(smp)
    gaps = R.rank_margins(y_rs, y_rr, y_ss)
    print('rank margins (COV, k-NN) %s, 10 x BAR = %.3g' % (gaps, 10 * BAR))
    assert min(gaps) >= 10 * BAR                                    # a condition on the inputs, asserted on the yardstick
    got = S.compute_all_metrics(dev(smp), dev(ref), batch_size=4, accelerated_cd=True, emd=True)
    assert tuple(got) == CD_KEYS[:3] + EMD_KEYS[:3] + CD_KEYS[3:] + EMD_KEYS[3:]    # the reference's order
    plain = S.compute_all_metrics(dev(smp), dev(ref))
    assert tuple(plain) == CD_KEYS
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
        if k in plain:
            assert torch.equal(v, plain[k]), k
        else:
            print('%s: %.9g (reference %.9g)' % (k, float(v), float(G['all_' + k])))
    for k in ('lgan_cov-EMD', '1-NN-EMD-acc_t', '1-NN-EMD-acc_f', '1-NN-EMD-acc'):
        assert float(got[k]) == float(G['all_' + k]), k
    for k in ('lgan_mmd-EMD', 'lgan_mmd_smp-EMD'):                  # a mean of minima: each within BAR of the truth, the recording within its own error
        assert abs(float(got[k]) - float(G['all_' + k])) <= BAR + float(G['ref_fp32_emd_err']) + 2.0 ** -22 * float(G['all_' + k]), k
    d = dev(smp)
    same = S.compute_all_metrics(d, d, emd=True)
    assert float(same['lgan_cov-EMD']) == 1.0 and 0.0 <= float(same['lgan_mmd-EMD']) <= S.EMD_EPS
    with pytest.raises(ValueError, match='equal point counts'):
        S.compute_all_metrics(d, d[:, :50], emd=True)
    assert tuple(S.compute_all_metrics(d, d[:, :50])) == CD_KEYS                    # (without emd unequal counts are fine, as before)


# ------------------------------------------------------------------------------------------------ duplicates, the whole path
def test_clouds_with_many_exact_ties(S, BAR):
    """P = 257: 40 distinct points drawn with replacement on both sides, a cloud against itself, all points coincident, one cloud
    coincident and the other spread (tests/emd_ref.py ``adversarial_cases``)"""
    for name, (x, y) in E.adversarial_cases(257).items():
        out, status, rounds = S._emd_matrix(dev(x[None]), dev(y[None]), rounds=True)
        want = E.emd_pair(x, y)
        print('%-22s kernel %.9g, yardstick %.9g, %d rounds' % (name, float(out), want, int(rounds)))
        assert int(status) == 0 and abs(float(out) - want) <= BAR
        assert int(rounds) < E.round_cap(257, 2 ** 23)[1] / 8
        assert np.float32(float(out)).tobytes() == E.auction(x, y)[0].tobytes() and int(rounds) == E.auction(x, y)[1]
        if name == 'coincident':                                    # every cost is 0
            assert float(out) == 0.0


def test_the_whole_path_from_sdf_grids_to_the_emd(S):
    """SDF -> mesh -> point cloud -> EMD matrix, everything on the device: the sphere and the box of the shape-metrics tests"""
    from echoscene_amd.postprocess import marching_cubes_batch
    n = 16
    g = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing='ij'), -1) / float(n) - 0.5)
    sphere = np.linalg.norm(g - np.array([0.02, -0.01, 0.03]), axis=-1) - 0.3
    q = np.abs(g - np.array([-0.03, 0.02, 0.01])) - np.array([0.3, 0.2, 0.15])
    box = np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)
    meshes = marching_cubes_batch(dev(np.stack([sphere, box]).astype(np.float32)), 0.02)
    pcs = S.point_clouds(meshes, number=257)
    m = host(S.pairwise_emd(pcs))
    assert m[0, 1] == m[1, 0] > 0 and m[0, 0] == m[1, 1] == 0
    assert abs(m[0, 1] - E.emd_pair(host(pcs[0]), host(pcs[1]))) <= S.EMD_EPS        # the guarantee itself: the yardstick is exact
    both = S.compute_all_metrics(pcs, pcs, emd=True)
    assert float(both['lgan_cov-EMD']) == 1.0 and 0.0 <= float(both['lgan_mmd-EMD']) <= S.EMD_EPS and float(both['lgan_mmd-CD']) == 0.0


# ------------------------------------------------------------------------------------------------ the status path
def test_a_coordinate_that_is_not_finite_is_flagged_not_iterated_on(S):
    """through the C entry point and through the wrapper: status 2, the entry NaN, zero rounds, the other entries untouched by it"""
    from echoscene_amd import hip
    a, b = R.golden_sets(17)
    want = host(S.pairwise_emd(dev(a), dev(b)))
    for bad in (np.nan, np.inf, -np.inf):
        a2 = a.copy()
        a2[2, 5, 1] = bad
        ta, tb = dev(a2), dev(b)
        out = torch.zeros(5, 4, dtype=torch.float32, device='cuda')
        status = torch.full((5, 4), -1, dtype=torch.int32, device='cuda')
        p = lambda t: C.c_void_p(t.data_ptr())
        hip.check(hip.lib().es_emd_matrix(p(ta), 5, p(tb), 4, 17, 0, p(out), p(status), hip.current_stream()), 'es_emd_matrix')
        st, o = host(status), host(out)
        assert (st[2] == 2).all() and np.isnan(o[2]).all()
        rest = [0, 1, 3, 4]
        assert (st[rest] == 0).all() and np.array_equal(o[rest], want[rest])
        _, _, rounds = S._emd_matrix(ta, tb, rounds=True)
        assert (host(rounds)[2] == 0).all() and (host(rounds)[rest] > 0).all()
        with pytest.raises(RuntimeError, match=r'pairwise_emd: pairs \[\(2, 0\), \(2, 1\), \(2, 2\), \(2, 3\)\] have a coordinate that is not finite'):
            S.pairwise_emd(ta, tb)
        with pytest.raises(RuntimeError, match=r'compute_all_metrics.*not finite'):
            S.compute_all_metrics(tb, ta, emd=True)
    # the symmetric mode flags both mirrored entries and leaves the diagonal 0
    a2 = a.copy()
    a2[1, 0, 0] = np.nan
    out, status = S._emd_matrix(dev(a2), None)
    st = host(status)
    assert (st[1, [0, 2, 3, 4]] == 2).all() and (st[[0, 2, 3, 4], 1] == 2).all() and st[1, 1] == 0 and st.sum() == 16
    assert np.isnan(host(out)[1, [0, 2, 3, 4]]).all() and float(out[1, 1]) == 0.0
