"""CPU-only checks of the earth mover's distance (csrc/es_emd.hip, echoscene_amd/shape_metrics.py ``pairwise_emd`` and
``compute_all_metrics(..., emd=True)``): the additions to the C ABI, every refusal of the launcher on the host and of the Python calls,
the float64 yardstick of the GPU tests (tests/emd_ref.py: exact assignment on float64 distances) against closed forms and against
the matrices the reference recorded, the numpy restatement of the kernel's auction against that yardstick -- its error, its rounds
and bids, its largest price -- and the host statistics against the reference's recorded results.  No device compute is called here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import emd_ref as E
import shape_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('es_emd_matrix', 'es_emd_matrix_rounds', 'es_emd_max_points')
EMD_KEYS = ('lgan_mmd-EMD', 'lgan_cov-EMD', 'lgan_mmd_smp-EMD', '1-NN-EMD-acc_t', '1-NN-EMD-acc_f', '1-NN-EMD-acc')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'emd.npz')))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_declared_bound_and_exported(L):
    from echoscene_amd import hip, build
    hdr = open(os.path.join(ROOT, 'include', 'echoscene_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(es_[a-z0-9_]+)\s*\(', hdr))
    raw = C.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip.EXPORTS and hasattr(raw, name), name
    assert 'es_emd.hip' in build.SOURCES
    assert len(hip.EXPORTS['es_emd_matrix'][1]) == 9 and len(hip.EXPORTS['es_emd_matrix_rounds'][1]) == 10
    assert L.es_emd_max_points() >= 5000                            # the reference script's `number`


def test_abi_version_and_op_size_did_not_move(L, tmp_path):
    from echoscene_amd import hip
    c = tmp_path / 'sz.c'
    c.write_text('#include <stdio.h>\n#include "echoscene_hip.h"\nint main(){printf("%zu %d\\n", sizeof(es_op), ES_ABI_VERSION);return 0;}')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    size, abi = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert size == C.sizeof(hip.Op) == 488
    assert abi == L.es_abi_version() == 10


def test_emd_matrix_launcher_refuses_on_the_host(L):
    """pointers, counts, the point limit, the three int32 limits and the symmetric contract are checked before anything is enqueued (no
    device is needed to get the refusal), and es_last_error names the function"""
    A = 4096                                                        # never dereferenced
    good = dict(a=A, Na=3, b=2 * A, Nb=2, P=17, symmetric=0, out=A, status=A)
    order = ('a', 'Na', 'b', 'Nb', 'P', 'symmetric', 'out', 'status')

    def refused(**kw):
        v = dict(good, **kw)
        rc = L.es_emd_matrix(*[v[k] for k in order], None)
        rc2 = L.es_emd_matrix_rounds(*[v[k] for k in order], A, None)
        return rc != 0 and rc2 != 0 and b'es_emd_matrix' in L.es_last_error()
    for name in ('a', 'b', 'out', 'status'):
        assert refused(**{name: None}) and b'NULL' in L.es_last_error(), name
    for kw in (dict(Na=0), dict(Nb=0), dict(P=0), dict(Na=-1), dict(Nb=-2), dict(P=-17)):
        assert refused(**kw) and b'empty' in L.es_last_error(), kw
    most = L.es_emd_max_points()
    assert refused(P=most + 1) and b'at most' in L.es_last_error()
    assert refused(P=2 ** 20) and b'at most' in L.es_last_error()
    for kw in (dict(Na=2 ** 18, P=4096), dict(Nb=2 ** 18, P=4096),                # 2^30 * 3 coordinates
               dict(Na=2 ** 16, P=1, Nb=2 ** 15)):                                 # 2^31 pairs
        assert refused(**kw) and b'int32' in L.es_last_error(), kw
    for kw in (dict(symmetric=1),                                                 # b != a
               dict(symmetric=1, b=A, Nb=2)):                                     # b == a, another count
        assert refused(**kw) and b'symmetric' in L.es_last_error(), kw


# ------------------------------------------------------------------------------------------------ the Python calls
def test_python_calls_refuse_before_any_device_work(L):
    """every ValueError of pairwise_emd and of compute_all_metrics(..., emd=True), on host and meta tensors (which are themselves the
    last refusal: no device is touched)"""
    from echoscene_amd import shape_metrics as S
    assert S.EMD_MAX_POINTS == L.es_emd_max_points() >= 5000 and 0 < S.EMD_EPS <= 1e-4 and S.EMD_EPS == E.EMD_EPS
    a = torch.zeros(2, 5, 3)
    meta = torch.zeros(2, 5, 3, device='meta')
    for bad, what in ((a.numpy(), 'must be a tensor'), (a.long(), 'floating point'), (a[0], r'\[N, P, 3\]'), (a[:, :, :2], r'\[N, P, 3\]'),
                      (a[:0], r'\[N, P, 3\]'), (a[:, :0], r'\[N, P, 3\]'), (a, 'not on the device')):
        with pytest.raises(ValueError, match='pairwise_emd: a .*' + what):
            S.pairwise_emd(bad)
        with pytest.raises(ValueError, match='pairwise_emd: a .*' + what):
            S.pairwise_emd(bad, a)
        if bad is not a:
            with pytest.raises(ValueError, match='pairwise_emd: b .*' + what):
                S.pairwise_emd(a, bad)
            with pytest.raises(ValueError, match='compute_all_metrics: ref_pcs .*' + what):
                S.compute_all_metrics(a, bad, emd=True)
        with pytest.raises(ValueError, match='compute_all_metrics: sample_pcs .*' + what):
            S.compute_all_metrics(bad, a, batch_size=50, accelerated_cd=True, emd=True)
    with pytest.raises(ValueError, match='different devices'):
        S.pairwise_emd(a, meta)
    with pytest.raises(ValueError, match='different devices'):
        S.compute_all_metrics(meta, a, emd=True)
    # the two refusals of the EMD alone come before the device is looked at
    for x, y in ((a, torch.zeros(3, 6, 3)), (meta, torch.zeros(3, 6, 3, device='meta')), (a.double(), torch.zeros(1, 4, 3).half())):
        with pytest.raises(ValueError, match='pairwise_emd: .*equal point counts.* 5 .* (6|4)'):
            S.pairwise_emd(x, y)
        with pytest.raises(ValueError, match='compute_all_metrics: .*equal point counts'):
            S.compute_all_metrics(x, y, emd=True)
    for dev in ('cpu', 'meta'):
        big = torch.zeros(1, S.EMD_MAX_POINTS + 1, 3, device=dev)
        with pytest.raises(ValueError, match='pairwise_emd: %d points per cloud.* at most EMD_MAX_POINTS = %d' % (S.EMD_MAX_POINTS + 1, S.EMD_MAX_POINTS)):
            S.pairwise_emd(big)
        with pytest.raises(ValueError, match='pairwise_emd: .*at most EMD_MAX_POINTS'):
            S.pairwise_emd(big, big)
        with pytest.raises(ValueError, match='compute_all_metrics: .*at most EMD_MAX_POINTS'):
            S.compute_all_metrics(big, big, emd=True)
        most = torch.zeros(1, S.EMD_MAX_POINTS, 3, device=dev)                     # the largest count passes on to the device check
        with pytest.raises(ValueError, match='not on the device'):
            S.pairwise_emd(most)


def test_without_emd_the_metrics_call_refuses_and_returns_as_before():
    """the one test of the feature's own interface that passes without the feature.  (test_abi_version_and_op_size_did_not_move pins
    constants the feature must not move, and the closed forms of the yardstick run on tests/emd_ref.py alone: these pass without the
    kernel too, which is what a yardstick is for.)"""
    from echoscene_amd import shape_metrics as S
    a, b = torch.zeros(2, 5, 3), torch.zeros(3, 6, 3)
    with pytest.raises(ValueError, match='compute_all_metrics: sample_pcs is not on the device'):      # unequal counts are no refusal
        S.compute_all_metrics(a, b)
    with pytest.raises(ValueError, match='compute_all_metrics: sample_pcs is not on the device'):
        S.compute_all_metrics(a, b, 4, True)
    with pytest.raises(ValueError, match='compute_all_metrics: ref_pcs .*floating point'):
        S.compute_all_metrics(a, b.long())
    with pytest.raises(ValueError, match='different devices'):
        S.compute_all_metrics(torch.zeros(2, 5, 3, device='meta'), a)
    m = np.random.RandomState(0).rand(4, 4)
    got = S.metrics_from_matrices(m, m + m.T, m * m.T)
    assert tuple(got) == ('lgan_mmd-CD', 'lgan_cov-CD', 'lgan_mmd_smp-CD', '1-NN-CD-acc_t', '1-NN-CD-acc_f', '1-NN-CD-acc')


# ------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_equals_closed_forms():
    x, y = np.array([[0.25, -0.5, 1.0]]), np.array([[-0.5, 0.5, 1.0]])
    assert E.emd_pair(x, y) == 1.25                                               # two single points: their distance, (3, 4, 0) / 4
    # a lattice cloud against a permuted translate of itself by (3, 4, 0) / 64: exactly 5/64 (emd_ref.translate_case)
    for P in (2, 17, 257):
        a, b = E.translate_case(P)
        assert np.array_equal(a * 64, np.round(a * 64)) and np.array_equal(b * 64, np.round(b * 64))
        assert abs(E.emd_pair(a, b) - 5 / 64.0) < 1e-15
    # clouds on a line: the sorted matching is optimal
    rs = np.random.RandomState(7)
    u, v = np.sort(rs.rand(100) * 2 - 1), np.sort(rs.rand(100) * 2 - 1)
    a = np.stack([u, 0 * u, 0 * u], 1)[rs.permutation(100)]
    b = np.stack([v, 0 * v, 0 * v], 1)[rs.permutation(100)]
    assert abs(E.emd_pair(a, b) - np.abs(u - v).mean()) < 1e-15
    # a cloud against itself, and against a permutation of itself
    c = R.clouds(1, 1, 50)[0]
    assert E.emd_pair(c, c) == 0.0 and E.emd_pair(c, c[rs.permutation(50)]) == 0.0
    assert E.emd_matrix([c, a[:50]])[0, 1] == E.emd_matrix([a[:50]], [c])[0, 0]   # symmetric in its arguments


def test_yardstick_agrees_with_the_recorded_matrices_of_the_reference(G):
    """the reference takes the norm of fp32 differences in fp32 -- a difference, three squares, two sums, a root: within 4 * 2^-24 of
    each distance, relative -- solves the assignment exactly on those, and takes a float32 mean of P of them, which numpy sums
    pairwise: another (1 + ceil(log2 P)) * 2^-24.  Distances of clouds in [-1, 1]^3 are at most 2 sqrt 3, so a recorded entry is
    within (5 + ceil(log2 P)) * 2^-24 * 2 sqrt 3 of the truth: 2.1e-6 at P = 17, 2.3e-6 at 64, 2.9e-6 at 257.  Measured (the generator
    prints it): 8e-8 at most."""
    bar = lambda P: (5 + int(np.ceil(np.log2(P)))) * 2.0 ** -24 * 2 * np.sqrt(3)
    for P in (17, 257):
        a, b = R.golden_sets(P)
        rec = G['emd_%d' % P]
        assert rec.shape == (5, 4) and rec.dtype == np.float32
        err = np.abs(rec - E.emd_matrix(a, b)).max()
        print('P = %d: max |recorded - yardstick| = %.3g (bar %.3g)' % (P, err, bar(P)))
        assert err <= bar(P)
    smp, ref = R.metric_sets()
    for name, y in (('M_rs', E.emd_matrix(ref, smp)), ('M_rr', E.emd_matrix(ref)), ('M_ss', E.emd_matrix(smp))):
        assert G[name].dtype == np.float32 and np.abs(G[name] - y).max() <= bar(64), name
    assert 0 < float(G['ref_fp32_emd_err']) <= bar(1025)
    assert G['ref_fp32_emd_err_by_P'].shape == (len(E.MATRIX_P),) and G['ref_fp32_emd_err_by_P'].max() <= G['ref_fp32_emd_err']
    # the input condition of the end-to-end GPU test
    gaps = R.rank_margins(E.emd_matrix(ref, smp), E.emd_matrix(ref), E.emd_matrix(smp))
    assert min(gaps) >= 10 * (E.EMD_EPS + 4 * float(G['ref_fp32_emd_err']))


# ------------------------------------------------------------------------------------------------ the restatement of the kernel
def gpu_test_pairs():
    """every pair of clouds that tests/test_hip_emd.py compares with the yardstick, as (label, x, y)"""
    for P in E.MATRIX_P:
        a, b = E.matrix_case(P)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                yield 'P%d a%d b%d' % (P, i, j), x, y
        for s, name in ((a, 'a'), (b, 'b')):
            for i in range(len(s)):
                for j in range(i + 1, len(s)):
                    yield 'P%d %s%d %s%d' % (P, name, i, name, j), s[i], s[j]
    for P in (17, 257):
        a, b = R.golden_sets(P)
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                yield 'golden P%d %d %d' % (P, i, j), x, y
    smp, ref = R.metric_sets()
    for i in range(6):
        for j in range(6):
            yield 'metric ref%d smp%d' % (i, j), ref[i], smp[j]
            if i < j:
                yield 'metric ref%d ref%d' % (i, j), ref[i], ref[j]
                yield 'metric smp%d smp%d' % (i, j), smp[i], smp[j]


def check_restatement(label, x, y):
    """the guarantee, the cap and the price bound on one pair; returns (P, |error|, rounds, bids per point)"""
    P = len(x)
    v, rounds, bids, per_phase, pmax = E.auction(x, y, detail=True)
    e = E.scale_exponent(x, y)
    assert e == 3, label                                           # normalised clouds: the quantum is 2^-20
    cmax = int(E.int_costs(x, y, e).max())
    err = abs(float(v) - E.emd_pair(x, y))
    per, total = E.round_cap(P, cmax)
    assert v.dtype == np.float32 and err <= E.EMD_EPS, (label, err)
    assert max(per_phase or [0]) < per / 8 and rounds < total / 8, (label, per_phase, per, total)
    assert pmax <= E.price_bound(cmax) < 2 ** 31 and cmax <= 2 ** 23, (label, pmax, cmax)
    return P, err, rounds, bids / float(P)


def test_restatement_meets_the_guarantee_on_the_clouds_of_the_gpu_tests():
    """``auction`` is within EMD_EPS of the yardstick on every pair the GPU tests use up to P = 1025; its rounds stay below an eighth of
    the kernel's cap, per phase and in total, and its prices below the bound the int32 arithmetic rests on"""
    worst = {}
    for label, x, y in gpu_test_pairs():
        P, err, rounds, bpp = check_restatement(label, x, y)
        w = worst.setdefault(P, [0.0, 0, 0.0, 0])
        worst[P] = [max(w[0], err), max(w[1], rounds), max(w[2], bpp), w[3] + 1]
    for P in sorted(worst):
        print('P %5d: %3d pairs, max |auction - yardstick| %.3g, most rounds %d (%.2f P; cap %d per phase), most bids per point %.1f' % (
            P, worst[P][3], worst[P][0], worst[P][1], worst[P][1] / float(P), E.round_cap(P, 2 ** 23)[0], worst[P][2]))
    assert set(worst) == set(E.MATRIX_P) and max(w[0] for w in worst.values()) <= E.EMD_EPS
    # the cap's constants here are the kernel's
    src = open(os.path.join(ROOT, 'echoscene_amd', 'csrc', 'es_emd.hip')).read()
    assert 'EM_CAP_MULT = %d, EM_CAP_ADD = %d;' % (E.CAP_MULT, E.CAP_ADD) in src and 'EM_THETA = %d;' % E.THETA in src
    assert 'EM_CAP_TOTAL_MULT = %d;' % E.CAP_TOTAL_MULT in src
    assert 'EM_BLOCK = %d;' % E.BLOCK in src and 'EM_COST_BITS = %d;' % E.COST_BITS in src
    assert len(E.eps_schedule(2 ** 23)) == 11                       # the phase count the header's price bound uses


def test_restatement_on_clouds_that_are_hard_on_an_auction():
    """P = 257: 40 distinct points drawn with replacement on both sides (what sample_indices yields for a small mesh), a cloud against
    itself, all points coincident, one cloud coincident and the other spread (both ways: bidders and objects differ)"""
    src = open(os.path.join(ROOT, 'echoscene_amd', 'csrc', 'es_emd.hip')).read()                  # the restatement's constants are the kernel's
    assert 'EM_MIN_EXP = %d, EM_MAX_EXP = %d;' % (E.MIN_SCALE_EXP, E.MAX_SCALE_EXP) in src and 'EM_CAP_TOTAL_MULT = %d;' % E.CAP_TOTAL_MULT in src
    cases = E.adversarial_cases(257)
    assert set(cases) == {'duplicates', 'self', 'coincident', 'coincident_vs_spread', 'spread_vs_coincident'}
    assert len(np.unique(cases['duplicates'][0], axis=0)) <= 40 and len(np.unique(cases['duplicates'][1], axis=0)) <= 40
    for name, (x, y) in cases.items():
        P, err, rounds, bpp = check_restatement(name, x, y)
        print('%-22s |auction - yardstick| %.3g, %d rounds (%.1f P), %.1f bids per point' % (name, err, rounds, rounds / float(P), bpp))
    assert float(E.auction(*cases['self'])[0]) == 0.0 and float(E.auction(*cases['coincident'])[0]) == 0.0
    # the translate beyond the host solver's reach, by its closed form
    x, y = E.translate_case(2049)
    v, rounds, bids = E.auction(x, y)
    print('translate P 2049: %.9g, %d rounds, %.1f bids per point' % (v, rounds, bids / 2049.0))
    assert abs(float(v) - 5 / 64.0) <= E.EMD_EPS and rounds < E.round_cap(2049, 2 ** 23)[1] / 8
    # status 2 of the kernel: nothing is iterated on
    bad = x.copy()
    bad[5, 1] = np.nan
    assert np.isnan(E.auction(bad, y)[0]) and E.auction(bad, y)[1] == 0 and E.scale_exponent(x * np.float32(1e38), y) is None
    # clouds that are not normalised take a coarser quantum, by powers of two
    big = R.clouds(5, 2, 65) * np.float32(1000) + np.float32(5000)
    e = E.scale_exponent(big[0], big[1])
    assert e == 12 and abs(float(E.auction(big[0], big[1])[0]) - E.emd_pair(big[0], big[1])) <= E.EMD_EPS * 2 ** (e - 3)


# ------------------------------------------------------------------------------------------------ host statistics
def test_emd_statistics_agree_with_the_reference(G):
    from echoscene_amd import shape_metrics as S
    y_rs, y_rr, y_ss = (G[k].astype(np.float64) for k in ('M_rs', 'M_rr', 'M_ss'))
    assert min(R.rank_margins(y_rs, y_rr, y_ss)) > 1e-3                            # no rank-based result rests on a near tie
    got = S.emd_metrics_from_matrices(G['M_rs'], G['M_rr'], G['M_ss'])
    assert tuple(got) == EMD_KEYS and {k[4:] for k in G if k.startswith('all_')} == set(EMD_KEYS)
    for k in ('lgan_cov-EMD', '1-NN-EMD-acc_t', '1-NN-EMD-acc_f', '1-NN-EMD-acc'):
        assert float(np.float32(got[k])) == float(G['all_' + k]), k
    for k in ('lgan_mmd-EMD', 'lgan_mmd_smp-EMD'):                                # a float32 mean of six values in another order: two ulps
        assert abs(float(np.float32(got[k])) - float(G['all_' + k])) <= 2 * 2.0 ** -24 * abs(float(G['all_' + k])), k
    cd = S.metrics_from_matrices(G['M_rs'], G['M_rr'], G['M_ss'])                  # the CD call on the same matrices: same values, its own keys
    assert list(cd.values()) == list(got.values()) and all('CD' in k for k in cd)
