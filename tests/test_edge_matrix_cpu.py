"""CPU-only half of the edge matrix (tests/edge_matrix_cases.py; the launches: tests/test_hip_conv32_matrix.py and
tests/test_hip_edge_matrix.py): the conditions the cases themselves have to meet, es_pack_conv_f32 against a numpy restatement, and the
host-side refusals of es_conv_f32, es_vq_lookup, es_shape_stem and es_layernorm_tokens, each pinned with its message.  Nothing is
launched: every refusal comes back before the library touches a device, so these pass on a machine without one."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_matrix_cases as cm
import edge_matrix_cases as em


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


# ---- the case module's own conditions ---------------------------------------------------------------------------------------------------

def test_case_names_are_unique_and_the_fp32_conv_dims_are_powers_of_two():
    names = em.all_case_names()
    assert len(set(names)) == len(names)
    for c in em.CONV32_CASES:
        for d in c['dims'] + cm.input_dims(c['mode'], c['dims']):
            assert d >= 1 and d & (d - 1) == 0, (c['name'], d)
    # both families, every mode, the skip wherever a mode takes one; and the four small cases the families cannot give
    for fam in 'AB':
        have = {(c['mode'], bool(c['Cin2'])) for c in em.CONV32_CASES if c['family'] == fam}
        assert have == {(m, s) for m in range(6) for s in (False, True) if not (s and m in cm.UP_MODES)}
    assert all(c['res'] and c['rowvec'] == (c['family'] == 'A') for c in em.CONV32_CASES if c['family'])
    small = {c['name']: c for c in em.CONV32_CASES if not c['family']}
    assert small['f32-linear']['taps'] == 1 and small['f32-cin40']['Cin'] % 16 == 8 and small['f32-ncdhw-n3']['out'] == 'ncdhw'
    assert not small['f32-ncdhw-n3']['res'] and small['f32-m8']['O'] * int(np.prod(small['f32-m8']['dims'])) == 8


@pytest.mark.parametrize('case', em.VQ_CASES, ids=lambda c: c['name'])
def test_vq_inputs_are_decidable_in_float64(case):
    """varied: at most 0.5 % of the voxels have a float64 best and second best within the bound of each other (the GPU test allows 1 %
    of differing indices: the reference alone must not spend that).  on-code, duplicates, near-ties: the pinned index is the float64
    first minimum of every voxel, the runner-up that is not its duplicate is farther by more than the bound, a near-tie's gap is 64 x
    the bound and no third code is nearer than its pair."""
    n, M = case['n_embed'], case['O'] * case['V']
    r = np.arange(M)
    p = em.vq_problem(case['name'], 'varied')
    share = em.vq_undecided_share(p)
    print('%s varied: %.3f %% of the voxels undecided in float64' % (case['name'], 100 * share))
    assert share <= 0.005
    assert p['z'].shape == (case['O'], 3, case['V']) and p['z'].dtype == np.float32
    for fam in ('on_code', 'duplicates'):
        p = em.vq_problem(case['name'], fam)
        D, S, want = p['D'], p['S'], p['want']
        assert bool((D.argmin(1) == want).all()) and bool((D[r, want] == 0).all())
        others = D.copy()
        others[r, want] = np.inf
        if fam == 'duplicates':
            dup = others.argmin(1)
            assert bool((others[r, dup] == 0).all()) and bool((dup > want).all())           # the equal row lies behind: first minimum
            assert bool((p['lut'][dup] == p['lut'][want]).all())
            others[r, dup] = np.inf
            assert len(set(want)) == em.VQ_NDUP
        t = others.argmin(1)
        assert bool((others[r, t] > em.VQ_TIE_FACTOR * em.vq_bound(np.maximum(S[r, t], S[r, want]))).all()), fam
    p = em.vq_problem(case['name'], 'near_ties')
    D, S, want, pair = p['D'], p['S'], p['want'], p['pair']
    a, b = pair[:, 0], pair[:, 1]
    other = np.where(want == a, b, a)
    bound = em.vq_bound(np.maximum(S[r, a], S[r, b]))
    gap = (D[r, other] - D[r, want]) / bound
    print('%s near-ties: gap / bound %.2f .. %.2f, %d pairs, %d voxels on a, %d on b'
          % (case['name'], gap.min(), gap.max(), len(set(map(tuple, pair))), int((want == a).sum()), int((want == b).sum())))
    assert bool((D.argmin(1) == want).all())
    assert gap.min() > 0.9 * em.VQ_TIE_FACTOR and gap.max() < 1.1 * em.VQ_TIE_FACTOR
    assert (want == a).sum() >= M // 4 and (want == b).sum() >= M // 4                      # both signs of delta
    third = D.copy()
    third[r, a] = third[r, b] = np.inf
    t = third.argmin(1)
    assert bool((third[r, t] - D[r, want] > em.VQ_TIE_FACTOR * em.vq_bound(np.maximum(S[r, t], np.maximum(S[r, a], S[r, b])))).all())


def test_vq_bound_holds_for_an_fp32_emulation_of_the_kernels_expression():
    """the kernel's expression evaluated in numpy float32 (products and sums rounded one by one, as written; the device may contract
    some into FMAs, which only removes roundings): every index it picks is within the bound of the float64 minimum"""
    for case in em.VQ_CASES[:2]:
        p = em.vq_problem(case['name'], 'varied')
        z = np.ascontiguousarray(p['z'].transpose(0, 2, 1).reshape(-1, 3))
        e = p['codebook']
        f = np.float32
        zz = (z[:, 0] * z[:, 0] + z[:, 1] * z[:, 1] + z[:, 2] * z[:, 2]).astype(f)
        ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).astype(f)
        dot = (z[:, None, 2] * e[None, :, 2] + (z[:, None, 1] * e[None, :, 1] + z[:, None, 0] * e[None, :, 0]).astype(f)).astype(f)
        d = ((zz[:, None] + ee[None, :]).astype(f) - f(2.0) * dot).astype(f)
        bad, differ = em.vq_check_indices(p, d.argmin(1))
        assert not bad and differ <= 0.005 * len(z), (bad, differ)


@pytest.mark.parametrize('cin', [3, 4])
def test_stem_families_do_what_they_are_for(cin):
    """all-negative: every conv output and every pooled value is below zero.  far window: a stage-2 pool whose second window started
    at 2 instead of 4 would change most outputs by far more than the bound; the input is zero outside the eight octants."""
    x, w = em.stem_problem(3, cin, 'all_negative')
    h1, c2, out = em.stem_reference(x, w, torch.float64)
    c1 = torch.nn.functional.conv3d(x.double(), w[0].double(), w[1].double(), padding=1)
    assert c1.max() < -1 and h1.max() < -1 and c2.max() < -1 and out.max() < -1
    x, w = em.stem_problem(3, cin, 'far_window')
    nz = (x != 0).nonzero()
    assert set(nz[:, 2:].flatten().tolist()) == set(range(4, 8)) | set(range(12, 16)) and len(nz) == x.numel() // 8
    out = em.stem_reference(x, w, torch.float64)[2]
    e32 = (em.stem_reference(x, w, torch.float32)[2].double() - out).abs().max().item() / out.abs().max().item()
    moved = (em.stem_reference(x, w, torch.float64, start=2)[2] - out).abs() > 100 * em.MARGIN * e32 * out.abs().max()
    assert moved.float().mean() > 0.5


def test_layernorm_families_have_the_rows_they_name():
    for M, Cc in em.LN_SHAPES:
        for fam, r in (('ratio10', 10.0), ('ratio1000', 1000.0)):
            x = em.ln_problem(M, Cc, fam)[0].double()
            ratio = x.mean(1).abs() / x.std(1)
            assert bool(((ratio > 0.3 * r) & (ratio < 3 * r)).all()), (M, Cc, fam)
        x, gamma, beta = em.ln_problem(M, Cc, 'const_row')
        for row, c in zip((0, M // 2, M - 1), em.LN_CONST):
            assert bool((x[row] == c).all())
        ref, w, E = em.ln_yardstick(x, gamma, beta)
        assert bool((ref[0] == beta.double()).all())                       # float64: a constant row gives beta exactly
        assert 2.0 ** -27 < E < 2.0 ** -20, (M, Cc, E)


# ---- es_pack_conv_f32 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,CinW,taps', [(5, 32, 27), (5, 40, 27), (7, 16, 1), (7, 13, 1), (3, 1, 27)])
def test_pack_conv_f32_equals_its_numpy_restatement(L, N, CinW, taps):
    """[N][taps][Cin16] from the PyTorch layout [N, CinW, taps]: every value in its place, the fill up to a multiple of 16 exactly zero
    (+0.0 bits), nothing written behind the image"""
    w = np.random.default_rng(5).standard_normal((N, CinW, taps)).astype(np.float32)
    Cin = (CinW + 15) // 16 * 16
    n = L.es_pack_conv_f32_size(N, CinW, taps)
    assert n == N * taps * Cin
    out = np.full(n + 64, np.float32(np.nan))
    assert L.es_pack_conv_f32(C.c_void_p(w.ctypes.data), N, CinW, taps, C.c_void_p(out.ctypes.data)) == 0
    want = np.zeros((N, taps, Cin), np.float32)
    want[:, :, :CinW] = w.transpose(0, 2, 1)
    assert np.array_equal(out[:n].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert bool(np.isnan(out[n:]).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def _conv32_args():
    from echoscene_amd import hip
    a = hip.ConvArgs()
    a.a, a.w, a.out_f32, a.bias = 4096, 8192, 12288, 16384            # (never dereferenced: every call below is refused on the host)
    a.O, a.D, a.H, a.W = 2, 4, 4, 8
    a.Cin, a.N, a.taps, a.mode, a.out_ld = 64, 232, 27, hip.CONV_SAME, 232
    return a


def test_conv_f32_refuses_what_it_cannot_run(L):
    from echoscene_amd import hip
    for change, text in ((dict(Cin=40), b'Cin=40'), (dict(Cin=0), b'Cin=0'), (dict(a2=4096, w2=4096, Cin2=24), b'Cin2=24'),
                         (dict(taps=8), b'taps=8'), (dict(H=12), b'(4,12,8)'), (dict(D=12), b'(12,4,8)'), (dict(W=12), b'(4,4,12)'),
                         (dict(out_f16=4096), b'out_f16'), (dict(epilogue=hip.EPI_GEGLU), b'epilogue=1'),
                         (dict(gn_stats_out=4096), b'gn_stats_out'), (dict(out_ld=-1, res=4096), b'NCDHW output takes no residual'),
                         (dict(mode=6), b'unknown mode 6'), (dict(mode=-1), b'unknown mode -1'), (dict(a=None), b'NULL'),
                         (dict(w=None), b'NULL'), (dict(out_f32=None), b'NULL'), (dict(O=0), b'O=0')):
        a = _conv32_args()
        for k, v in change.items():
            setattr(a, k, v)
        assert L.es_conv_f32(C.byref(a), None) != 0, change
        msg = L.es_last_error()
        assert msg.startswith(b'es_conv_f32') and text in msg, (change, msg)


def _refused(L, fn, name, args, text):
    assert fn(C.byref(args), None) != 0, text
    msg = L.es_last_error()
    assert msg.startswith(name + b': ') and text in msg, (text, msg)


def test_vq_lookup_refuses_bad_arguments_on_the_host(L):
    from echoscene_amd import hip

    def args(**kw):
        a = hip.VQArgs()
        a.z, a.codebook, a.lut, a.out_f16, a.idx_out = 4096, 8192, 12288, 16384, 20480
        a.O, a.V, a.n_embed, a.Cpad = 2, 100, 64, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for f in ('z', 'codebook', 'lut', 'out_f16'):
        _refused(L, L.es_vq_lookup, b'es_vq_lookup', args(**{f: None}), b'NULL')
    for kw, text in ((dict(O=0), b'O=0'), (dict(O=-1), b'O=-1'), (dict(V=0), b'V=0'), (dict(V=-5), b'V=-5'), (dict(Cpad=2), b'Cpad=2'),
                     (dict(Cpad=0), b'Cpad=0'), (dict(n_embed=0), b'n_embed=0'), (dict(n_embed=16384), b'n_embed=16384')):
        _refused(L, L.es_vq_lookup, b'es_vq_lookup', args(**kw), text)


def test_shape_stem_refuses_bad_arguments_on_the_host(L):
    from echoscene_amd import hip

    def args(**kw):
        a = hip.StemArgs()
        a.x, a.w0, a.b0, a.w1, a.b1, a.scratch, a.out = (4096 * i for i in range(1, 8))
        a.O, a.Cin, a.x_ostride = 3, 0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for f in ('x', 'w0', 'b0', 'w1', 'b1', 'scratch', 'out'):
        _refused(L, L.es_shape_stem, b'es_shape_stem', args(**{f: None}), b'NULL')
    for kw, text in ((dict(O=0), b'O=0'), (dict(O=-2), b'O=-2'), (dict(Cin=1), b'Cin=1'), (dict(Cin=2), b'Cin=2'), (dict(Cin=5), b'Cin=5'),
                     (dict(Cin=-3), b'Cin=-3'), (dict(x_ostride=-1), b'x_ostride=-1'), (dict(scratch=4096 + 4), b'aligned')):
        _refused(L, L.es_shape_stem, b'es_shape_stem', args(**kw), text)


def test_layernorm_tokens_refuses_bad_arguments_on_the_host(L):
    from echoscene_amd import hip

    def args(**kw):
        a = hip.LNArgs()
        a.x, a.gamma, a.beta, a.y_f16 = 4096, 8192, 12288, 16384
        a.M, a.C, a.eps, a.y_is_f32 = 37, 448, 1e-5, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for f in ('x', 'gamma', 'beta', 'y_f16'):
        _refused(L, L.es_layernorm_tokens, b'es_layernorm_tokens', args(**{f: None}), b'NULL')
    for kw, text in ((dict(M=0), b'M=0'), (dict(M=-4), b'M=-4'), (dict(C=0), b'C=0'), (dict(C=6), b'C=6'), (dict(C=1028), b'C=1028')):
        _refused(L, L.es_layernorm_tokens, b'es_layernorm_tokens', args(**kw), text)
    # 16-byte loads of x, gamma, beta; 8-byte (f16) or 16-byte (fp32) stores
    for kw in (dict(x=4096 + 8), dict(gamma=8192 + 4), dict(beta=12288 + 8), dict(y_f16=16384 + 4), dict(y_f16=16384 + 8, y_is_f32=1)):
        _refused(L, L.es_layernorm_tokens, b'es_layernorm_tokens', args(**kw), b'aligned')
    # (an f16 output on an 8-byte boundary is fine: this one gets past the checks only on a machine with a device, so it is not called)
