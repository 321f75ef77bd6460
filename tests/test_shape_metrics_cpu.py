"""CPU-only checks of the shape-set metrics (csrc/es_shape_metrics.hip, echoscene_amd/shape_metrics.py): the additions to the C ABI,
every refusal of the two launchers on the host and of the Python calls, the float64 yardstick of the GPU tests
(tests/shape_metrics_ref.py) against closed forms and against the matrices the reference recorded, and the host statistics
(MMD, COV, k-NN) and the sampling rule against the reference's recorded results.  No device compute is called here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import shape_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('es_chamfer_matrix', 'es_cloud_normalize')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'shape_metrics.npz')))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported(L):
    from echoscene_amd import hip, build
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip.EXPORTS and hasattr(raw, name), name
    assert 'es_shape_metrics.hip' in build.SOURCES
    assert len(hip.EXPORTS['es_chamfer_matrix'][1]) == 9 and len(hip.EXPORTS['es_cloud_normalize'][1]) == 9


def test_abi_version_and_op_size_did_not_move(L, tmp_path):
    from echoscene_amd import hip
    c = tmp_path / 'sz.c'
    c.write_text('#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){printf("%zu %d\\n", sizeof(es_op), ES_ABI_VERSION);return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, abi = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert size == C.sizeof(hip.Op) == 488
    assert abi == L.es_abi_version() == 10


def test_chamfer_matrix_launcher_refuses_on_the_host(L):
    """pointers, counts, the three int32 limits and the symmetric contract are checked before anything is enqueued (no device is needed
    to get the refusal), and es_last_error names the function"""
    P = 4096                                                        # never dereferenced
    good = dict(a=P, Na=3, P=17, b=2 * P, Nb=2, Q=5, symmetric=0, out=P)
    order = ('a', 'Na', 'P', 'b', 'Nb', 'Q', 'symmetric', 'out')

    def refused(**kw):
        v = dict(good, **kw)
        rc = L.es_chamfer_matrix(*[v[k] for k in order], None)
        return rc != 0 and b'es_chamfer_matrix' in L.es_last_error()
    for name in ('a', 'b', 'out'):
        assert refused(**{name: None}) and b'NULL' in L.es_last_error(), name
    for kw in (dict(Na=0), dict(Nb=0), dict(P=0), dict(Q=0), dict(Na=-1), dict(Nb=-2), dict(P=-17), dict(Q=-5)):
        assert refused(**kw), kw
    for kw in (dict(Na=2 ** 16, P=2 ** 14), dict(Nb=2 ** 16, Q=2 ** 14),         # 2^30 * 3 coordinates
               dict(Na=2 ** 16, P=1, Nb=2 ** 15, Q=1)):                           # 2^31 pairs
        assert refused(**kw) and b'int32' in L.es_last_error(), kw
    for kw in (dict(symmetric=1),                                                 # b != a
               dict(symmetric=1, b=P, Nb=3, Q=5), dict(symmetric=1, b=P, Nb=2, Q=17)):      # b == a, other counts
        assert refused(**kw) and b'symmetric' in L.es_last_error(), kw


def test_cloud_normalize_launcher_refuses_on_the_host(L):
    P = 4096
    good = dict(verts=P, vofs=P, index=P, K=2, number=64, total_V=100, bad=P, out=P)
    order = ('verts', 'vofs', 'index', 'K', 'number', 'total_V', 'bad', 'out')

    def refused(**kw):
        v = dict(good, **kw)
        rc = L.es_cloud_normalize(*[v[k] for k in order], None)
        return rc != 0 and b'es_cloud_normalize' in L.es_last_error()
    for name in ('verts', 'vofs', 'index', 'bad', 'out'):
        assert refused(**{name: None}) and b'NULL' in L.es_last_error(), name
    for kw in (dict(K=0), dict(K=-1), dict(number=0), dict(number=-5), dict(total_V=-1)):
        assert refused(**kw), kw
    for kw in (dict(K=2 ** 15, number=2 ** 15), dict(total_V=2 ** 30)):
        assert refused(**kw) and b'int32' in L.es_last_error(), kw


# ------------------------------------------------------------------------------------------------ the Python calls
def test_python_calls_refuse_before_any_device_work():
    """every ValueError of the public calls, on host tensors (which are themselves the last refusal: no device is touched)"""
    from echoscene_amd import shape_metrics as S
    a = torch.zeros(2, 5, 3)
    meta = torch.zeros(2, 5, 3, device='meta')
    for bad, what in ((a.numpy(), 'must be a tensor'), (a.long(), 'floating point'), (a[0], r'\[N, P, 3\]'), (a[:, :, :2], r'\[N, P, 3\]'),
                      (a[:0], r'\[N, P, 3\]'), (a[:, :0], r'\[N, P, 3\]'), (a, 'not on the device')):
        with pytest.raises(ValueError, match='pairwise_chamfer: a .*' + what):
            S.pairwise_chamfer(bad)
        with pytest.raises(ValueError, match='pairwise_chamfer: a .*' + what):
            S.pairwise_chamfer(bad, a)
        if bad is not a:
            with pytest.raises(ValueError, match='pairwise_chamfer: b .*' + what):
                S.pairwise_chamfer(a, bad)
            with pytest.raises(ValueError, match='compute_all_metrics: ref_pcs .*' + what):
                S.compute_all_metrics(a, bad)
        with pytest.raises(ValueError, match='compute_all_metrics: sample_pcs .*' + what):
            S.compute_all_metrics(bad, a, batch_size=50, accelerated_cd=True)
    with pytest.raises(ValueError, match='different devices'):
        S.pairwise_chamfer(a, meta)
    with pytest.raises(ValueError, match='different devices'):
        S.compute_all_metrics(meta, a)

    v = torch.zeros(10, 3)
    f = torch.zeros(4, 3, dtype=torch.long)
    for bad, what in (([], 'non-empty'), ((), 'non-empty'), (None, 'non-empty'), ([v.numpy()], 'neither'), ([(v, f, f)], 'neither'),
                      ([v[:, :2]], 'verts of mesh 0'), ([(v[None], f)], 'verts of mesh 0'), ([v.long()], 'verts of mesh 0'),
                      ([v, (v[:0], f)], 'mesh 1 has no vertices'), ([v[:0]], 'mesh 0 has no vertices')):
        with pytest.raises(ValueError, match='point_clouds: .*' + what):
            S.point_clouds(bad)
    for number in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='number must'):
            S.point_clouds([v], number=number)
    with pytest.raises(ValueError, match='int32'):
        S.point_clouds([v], number=2 ** 30)
    for meshes in ([v], v, (v, f), [(v.double(), f)], [v, (v, f)]):               # well-formed, but on the host
        with pytest.raises(ValueError, match='not on the device'):
            S.point_clouds(meshes, number=7)
    with pytest.raises(ValueError, match='not on the device'):                  # (the first mesh decides; a meta tensor is no device either)
        S.point_clouds([torch.zeros(4, 3, device='meta'), v])

    m = torch.rand(4, 4)
    with pytest.raises(ValueError, match='all_dist'):
        S.lgan_mmd_cov(m[0])
    with pytest.raises(ValueError, match='all_dist'):
        S.lgan_mmd_cov(m.long())
    for args, what in (((m[:, :3], m, m, 1), 'Mxx must be square'), ((m, m[:, :3], m, 1), 'Mxy must be'), ((m, m, m[:3], 1), 'Myy must be square'),
                       ((m, m, m, 0), 'k must'), ((m, m, m, 8), 'k must'), ((m, m, m, 1.0), 'k must')):
        with pytest.raises(ValueError, match=what):
            S.knn(*args)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_equals_closed_forms():
    x, y = np.array([[0.25, -0.5, 1.0]]), np.array([[-0.75, 0.5, 0.0]])
    assert R.chamfer_matrix([x], [y])[0, 0] == 2 * (1.0 + 1.0 + 1.0)              # two single points: twice their squared distance
    # a cloud and its translate by less than half the smallest spacing: every nearest neighbour is the point's own translate
    g = np.stack(np.meshgrid(*[np.arange(4) * 0.25 - 0.375] * 3, indexing='ij'), -1).reshape(-1, 3)
    t = np.array([0.0625, -0.03125, 0.09375])
    assert np.abs(t).max() < 0.125
    assert R.chamfer_matrix([g], [g + t])[0, 0] == 2 * (t ** 2).sum()              # (exact: dyadic rationals)
    assert R.chamfer_matrix([g])[0, 0] == 0.0
    # one point against a cloud: |x - nearest|^2 + the mean of all squared distances
    d = ((g - x) ** 2).sum(1)
    assert abs(R.chamfer_matrix([x], [g])[0, 0] - (d.min() + d.mean())) < 1e-15
    # a lattice of quarters: every squared distance is an integer over 16, so the whole matrix is integer arithmetic
    rs = np.random.RandomState(5)
    a, b = rs.randint(-4, 5, size=(3, 40, 3)), rs.randint(-4, 5, size=(2, 33, 3))
    want = np.zeros((3, 2))
    for i in range(3):
        for j in range(2):
            d = ((a[i][:, None, :] - b[j][None, :, :]) ** 2).sum(-1)                # int64
            want[i, j] = d.min(1).sum() / (16.0 * 40) + d.min(0).sum() / (16.0 * 33)
    assert np.abs(R.chamfer_matrix(a / 4.0, b / 4.0) - want).max() < 1e-15
    # symmetric in its arguments
    assert np.array_equal(R.chamfer_matrix(a / 4.0, b / 4.0), R.chamfer_matrix(b / 4.0, a / 4.0).T)


def test_yardstick_agrees_with_the_recorded_matrices_of_the_reference(G):
    """the reference evaluates xx + yy - 2 zz in fp32 on coordinates in [-1, 1]: three sums of magnitude <= 3, 3 and 6, about six
    roundings of relative 2^-24 on values <= 12 -> an entry is within 6 * 12 * 2^-24 = 4.3e-6 of the truth, means included; measured
    1.1e-7 at most (tests/golden/make_golden_shape_metrics.py prints it)"""
    for P in (17, 257):
        a, b = R.golden_sets(P)
        cd = G['cd_%d' % P]
        assert cd.shape == (5, 4) and cd.dtype == np.float32
        assert np.abs(cd - R.chamfer_matrix(a, b)).max() <= 4.3e-6
    smp, ref = R.metric_sets()
    for name, y in (('M_rs', R.chamfer_matrix(ref, smp)), ('M_rr', R.chamfer_matrix(ref)), ('M_ss', R.chamfer_matrix(smp))):
        assert np.abs(G[name] - y).max() <= 4.3e-6, name
    assert 0 < float(G['ref_fp32_err']) <= 4.3e-6
    assert G['ref_fp32_err_by_case'].shape == (len(R.MATRIX_CASES),) and G['ref_fp32_err_by_case'].max() <= G['ref_fp32_err']


def test_clouds_of_the_gpu_tests_are_what_the_tests_assume():
    for n, (Na, Nb, P, Q) in enumerate(R.MATRIX_CASES):
        a, b = R.matrix_case(n)
        assert a.shape == (Na, P, 3) and b.shape == (Nb, Q, 3) and a.dtype == b.dtype == np.float32
        assert np.abs(a).max() <= 1 and np.abs(b).max() <= 1 and np.isfinite(a).all() and np.isfinite(b).all()
        for x in a if P > 1 else ():
            assert abs(np.abs(x).max() - 1) < 1e-6 and np.abs(x.mean(0, dtype=np.float64)).max() < 1e-6       # normalised
    assert {c[0] for c in R.MATRIX_CASES} == {c[1] for c in R.MATRIX_CASES} == {1, 2, 3}
    sizes = {c[2] for c in R.MATRIX_CASES} | {c[3] for c in R.MATRIX_CASES}
    assert {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049} <= sizes
    assert sum(c[2] != c[3] for c in R.MATRIX_CASES) >= 8
    for n, (P, Q) in enumerate(R.LATTICE_CASES):
        a, b = R.lattice_case(n)
        assert a.shape == (1, P, 3) and b.shape == (1, Q, 3)
        assert np.array_equal(a * 64, np.round(a * 64)) and np.abs(a).max() <= 1
        d = R.pair_sq_dists(a[0], b[0])
        for s in R.SEAM_INDICES:
            if s < min(P, Q) and min(P, Q) > 1:                                    # each planted pair is a mutual, unique nearest neighbour
                assert d[s, s] == 1 / 4096.0
                assert (d[s] <= d[s, s]).sum() == 1 and (d[:, s] <= d[s, s]).sum() == 1


# ------------------------------------------------------------------------------------------------ host statistics and sampling
def test_statistics_agree_with_the_reference(G):
    from echoscene_amd import shape_metrics as S
    M_rs, M_rr, M_ss = (torch.from_numpy(G[k]) for k in ('M_rs', 'M_rr', 'M_ss'))
    y_rs, y_rr, y_ss = (G[k].astype(np.float64) for k in ('M_rs', 'M_rr', 'M_ss'))
    assert min(R.rank_margins(y_rs, y_rr, y_ss)) > 1e-4                            # no rank-based result rests on a near tie
    got = S.lgan_mmd_cov(M_rs.t())
    assert set(got) == {'lgan_mmd', 'lgan_cov', 'lgan_mmd_smp'}
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.device == M_rs.device
        # a float32 mean of six values in another order: two ulps
        assert abs(float(v) - float(G['stat_' + k])) <= 2 * 2.0 ** -24 * float(G['stat_' + k]), k
    assert float(got['lgan_cov']) == float(G['stat_lgan_cov'])
    for tag, k, sq in (('knn1', 1, False), ('knn3', 3, False), ('knn1sqrt', 1, True)):
        got = S.knn(M_rr, M_rs, M_ss, k, sqrt=sq)
        assert set(got) == {'tp', 'fp', 'fn', 'tn', 'precision', 'recall', 'acc_t', 'acc_f', 'acc'}
        for key, v in got.items():
            assert v.dim() == 0 and v.dtype == torch.float32
            assert float(v) == float(G['%s_%s' % (tag, key)]), (tag, key)
    assert float(G['knn1_acc']) not in (0.0, 1.0) or float(G['knn3_acc']) not in (0.0, 1.0)      # (the sets are not trivially separable)
    allm = S.metrics_from_matrices(G['M_rs'], G['M_rr'], G['M_ss'])
    keys = ('lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc')
    assert tuple(allm) == keys and {k[4:] for k in G if k.startswith('all_')} == set(keys)
    for k in keys:
        assert abs(float(np.float32(allm[k])) - float(G['all_' + k])) <= 2 * 2.0 ** -24 * abs(float(G['all_' + k])), k


def test_first_index_wins_a_tie():
    from echoscene_amd import shape_metrics as S
    d = torch.tensor([[1.0, 1.0, 2.0], [3.0, 1.0, 1.0]])                         # sample 0 -> ref 0 (not 1), sample 1 -> ref 1 (not 2)
    assert float(S.lgan_mmd_cov(d)['lgan_cov']) == np.float32(2 / 3.0)
    z = torch.zeros(2, 2)
    # every off-diagonal distance equal: each element's nearest neighbour is the first other index, which is in set x for all but
    # element 0, whose first other index is 1 -- also in x: everything is predicted 1
    r = S.knn(z, z, z, 1)
    assert (float(r['tp']), float(r['fp']), float(r['fn']), float(r['tn'])) == (2.0, 2.0, 0.0, 0.0)


def test_sampling_rule_agrees_with_the_reference(G):
    from echoscene_amd import shape_metrics as S
    state = np.random.get_state()[1].copy()
    for n, number in R.SAMPLE_CASES:
        idx = S.sample_indices(n, number)
        assert idx.dtype == np.int32 and np.array_equal(idx, G['idx_%d_%d' % (n, number)]), (n, number)
        # and the recorded normalisation is the float64 formula of the yardstick on those vertices
        want = G['norm_%d_%d' % (n, number)]
        got = R.normalize(R.sample_verts(n)[idx])
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(np.abs(got - want), initial=0) <= 1e-15
    assert np.array_equal(np.random.get_state()[1], state)                        # the global generator is left alone
    assert any(n >= number for n, number in R.SAMPLE_CASES) and any(n < number for n, number in R.SAMPLE_CASES)
    assert np.isnan(G['norm_7_1']).all()                                          # one point: 0 / 0, as documented
