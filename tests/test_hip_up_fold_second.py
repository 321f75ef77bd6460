"""GPU: the folded route of the up-sampling convs (k_conv_ws_fold) at the size of the shape step's SECOND up-sampling launch -- 32
objects, output 16 x 8 x 8, 128 row tiles of 256 rows -- reached by the library's own rule and the planner's own decision, with no
forcing option: Builder.conv(w_fold=...) asks the library what the launch does without a split-K workspace and withholds the
workspace where the answer is the folded kernel (tests/test_up_fold_second_cpu.py).  tests/test_hip_up_fold.py covers the kernel on
two tiny shapes under conv_force256; a grid of more than one round of workgroups, a last round that is only partly filled, and a
ragged last column tile at that size are covered here:

  n680           Cin = 32, N = 680: FOUR column tiles (3 x 224 + 8), the last one ragged with 8 columns: 512 tiles = two full rounds
                 on 256 CUs, one channel chunk, 12 folded K units, 17 GFLOP folded.  (The shape the issue sets.  It describes it as
                 three column tiles / 384 tiles and its unfolded launch as split; neither holds for N = 680 and 27 K units -- the
                 library's tile-quantisation split needs a last round under 80 % and >= 48 K units per part -- so here the unfolded
                 launch is asserted UNSPLIT, and the next shape carries what the description asks for.)
  partial-round  Cin = 128, N = 456: THREE column tiles (2 x 224 + 8), the last one ragged: 384 tiles = 1.5 rounds, four channel
                 chunks, 48 folded K units.  With a workspace the library splits the unfolded launch two ways (108 K units, 768
                 workgroups = 3 full rounds, k_conv_splitk_reduce): today's route of the step's second launch, asserted by name
                 and S = 2.  The folded launch takes the BALANCED schedule (es_conv_fold_balanced: two workgroups per row tile,
                 each one 256-row tile and a 128-row half of the third column tile), n680 with its full rounds the plain one.
  tiny-half-tile O = 1, output 4 x 16 x 16, Cin = 32, N = 456, under conv_force256: four row tiles, a half tile is two d-planes of one
                 parity class; the balanced schedule's edges (ragged third column tile on 32-row waves, the sums of a 64-row group
                 from two waves) at the smallest size.  (The issue names N = 680 here too: four column tiles, which the rule
                 does not balance.)

Configurations: all fused operands (bias, per-object vector, residual, fp32 + f16 output, row-group sums); none; sums only.
Bounds, helpers and guards are those of tests/test_hip_up_fold.py / tests/test_hip_conv_matrix.py:
  * grid weights (multiples of 2^-6): error against float64 <= min(MARGIN x e32, 1e-4) of the tensor scale;
  * Gaussian weights: <= 2 x the unfolded route's error on the same inputs;
  * the f16 output is the rounded fp32 output bit for bit; the row-group sums equal the float64 sums of the stored output to 1e-5,
    rows ordered (parity class, d, hi, wi); no NaN left, no guard written.
Run with -s to print the figures (profiles/up_fold_notes.md records them)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_matrix import GuardedInput, GuardedOutput, MARGIN, _cl, _options, _rnd, _set
from test_hip_up_fold import FOLD, _check, _reference

pytestmark = pytest.mark.gpu

SHAPES = {'n680': dict(O=32, dims=(16, 8, 8), Cin=32, N=680, unfolded=('ws_256_8_4_3', 1), balanced=0),
          'partial-round': dict(O=32, dims=(16, 8, 8), Cin=128, N=456, unfolded=('ws_256_8_4_3', 2), balanced=1),
          'tiny-half-tile': dict(O=1, dims=(4, 16, 16), Cin=32, N=456, unfolded=('ws_256_8_4_3', 1), balanced=1, force256=True)}
# (bias, rowvec, res, out_f16, stats)
CONFIGS = {'all': (True, True, True, True, True), 'none': (False, False, False, False, False),
           'sums-only': (False, False, False, False, True)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


@functools.lru_cache(maxsize=None)
def _problem(shape, weights):
    """operands and the float64 / float32 conv on the CPU (without bias / rowvec / res: added per configuration), once per case"""
    s = SHAPES[shape]
    O, (D, H, W), Cin, N = s['O'], s['dims'], s['Cin'], s['N']
    x = _rnd((O, Cin, D, H // 2, W // 2), 1).half().float()
    if weights == 'grid':
        wt = torch.randint(-64, 65, (N, Cin, 3, 3, 3), generator=torch.Generator().manual_seed(2)).float() / 64.0
    else:
        wt = _rnd((N, Cin, 3, 3, 3), 2) / np.sqrt(Cin * 27.0)
    conv = lambda dt: _cl(F.conv3d(F.interpolate(x.to(dt), (D, H, W), mode='nearest'), wt.to(dt), padding=1))
    return dict(x=x, wt=wt, y64=conv(torch.float64), y32=conv(torch.float32), bias=_rnd((N,), 3), rowvec=_rnd((O, N), 4),
                res=_rnd((O * D * H * W, N), 5))


def _launch(dev, L, s, p, pc, cfg, xin, folded):
    """one launch as the planner emits it (no route option touched): with the folded image the op must come back without a workspace
    and on the folded kernel, without it with the shared workspace and on the route SHAPES names; asserted before anything runs"""
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder, View
    bias, rowvec, res, f16, stats = cfg
    O, dims, N = s['O'], s['dims'], s['N']
    V = dims[0] * dims[1] * dims[2]
    M = O * V
    rv = GuardedInput(dev, p['rowvec'], torch.float32, N) if rowvec else None
    rs = GuardedInput(dev, p['res'], torch.float32, V * N) if res else None
    o32, o16 = GuardedOutput(dev, M, N, torch.float32), (GuardedOutput(dev, M, N, torch.float16) if f16 else None)
    st = torch.full((2, M // 64, N), float('nan'), device=dev) if stats else None
    found = _options(L)
    try:
        if s.get('force256'):                    # (the tiny shape only: far too few rows to reach the 256-row tiles by itself)
            _set(L, [('conv_force256', 1)])
        b = Builder(dev)
        i = b.conv(xin.view, pc, O, dims, mode=hip.CONV_UP_HW, bias=p['bias'].to(dev) if bias else None, rowvec=View(rv.view) if rv else None,
                   res=rs.view if rs else None, out_f32=o32.view, out_f16=o16.view if o16 else None, w_fold=pc.w_fold if folded else None)
        cv = b.ops[i].u.conv
        if stats:
            cv.gn_stats_out = st.data_ptr()
        name = C.create_string_buffer(32)
        S = L.es_conv_kernel_of(C.byref(cv), name, 32)
        got = (name.value.decode(), S)
        if folded:
            assert got == (FOLD, 1) and cv.w2 and not cv.workspace and cv.splitk == 0, 'routed to %s, S = %d (not run)' % got
            assert not stats or L.es_conv_emits_gn_stats(C.byref(cv)) == 1
            assert L.es_conv_fold_balanced(C.byref(cv)) == s['balanced']
        else:
            assert got == s['unfolded'] and not cv.w2 and cv.workspace and cv.splitk == -1, 'routed to %s, S = %d (not run)' % got
            assert L.es_conv_split_of(C.byref(cv)) == S and b._ws.numel() >= S * M * N
            assert L.es_conv_fold_balanced(C.byref(cv)) == 0
        b.finish().run()
        torch.cuda.synchronize()
    finally:
        _set(L, found)
    return dict(o32=o32, o16=o16, st=st, inputs=[('rowvec', rv), ('res', rs)])


@pytest.mark.parametrize('weights', ['grid', 'gauss'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_up_fold_at_the_second_launch_size(dev, shape, weights):
    from echoscene_amd import hip
    from echoscene_amd.plan_vol import PackedConv
    L = hip.lib()
    s, p = SHAPES[shape], _problem(shape, weights)
    O, (D, H, W), Cin, N = s['O'], s['dims'], s['Cin'], s['N']
    V = D * H * W
    Hi, Wi = H // 2, W // 2
    assert (D * Hi * Wi) % 256 == 0 and (s.get('force256') or (O * V // 256) * ((N + 223) // 224) >= 256)
    xin = GuardedInput(dev, _cl(p['x']), torch.float16, max(D * Hi * Wi, (Hi + 1) * Wi + 1) * Cin)
    pc = PackedConv(p['wt'], None, dev, up_fold=True)
    assert pc.w_fold is not None
    bad = []
    for cname, cfg in CONFIGS.items():
        tag = '%s %s [%s]' % (shape, weights, cname)
        ref = _reference(p, cfg, V, torch.float64).to(dev)
        scale = ref.abs().max().item()
        out = _launch(dev, L, s, p, pc, cfg, xin, True)
        e = _check(tag, s, out, ref, scale, True, bad)
        if weights == 'grid':
            e32 = (_reference(p, cfg, V, torch.float32).double().to(dev) - ref).abs().max().item() / scale
            assert 1e-8 < e32 < 2e-6, 'the fp32 CPU computation is not the yardstick it is meant to be: e32 = %.3e' % e32
            tol = min(MARGIN * e32, 1e-4)
            print('%s: folded error %.3e = %.2f x e32 (e32 = %.3e)' % (tag, e, e / e32, e32))
            if not e <= tol:
                bad.append('%s: differs from fp64 by %.3e of the tensor scale = %.1f x e32 (bound %d x)' % (tag, e, e / e32, MARGIN))
        else:
            plain = _launch(dev, L, s, p, pc, cfg[:4] + (False,), xin, False)          # (the sums of the 27-tap routes: tests/test_hip_conv_matrix.py)
            eu = _check(tag + ' unfolded', s, plain, ref, scale, False, bad)
            print('%s: folded error %.3e, unfolded %.3e (%s, S = %d), ratio %.2f' % ((tag, e, eu) + s['unfolded'] + (e / eu,)))
            if not e <= 2 * eu:
                bad.append('%s: folded error %.3e is more than twice the unfolded route\'s %.3e' % (tag, e, eu))
        if not xin.unchanged():
            bad.append('%s: the input (or its guards) was written' % tag)
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


@pytest.mark.parametrize('shape', ['tiny-half-tile', 'mid'])
def test_the_balanced_schedule_leaves_the_bits_of_the_plain_one(dev, shape):
    """Every output element is one workgroup's sum over the whole folded K range in the same unit order on both schedules.  The plain
    schedule of the same launch is reached by the library's rule too: a launch that has a workspace (and too few K units to be split:
    27 < 2 x 48) stays on the folded kernel, unbalanced.  fp32 and f16 outputs must be equal bit for bit; the row-group sums, added
    from two 32-row waves on the half tile, to 1e-6."""
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder, View
    from echoscene_amd.plan_vol import PackedConv
    L = hip.lib()
    s = dict(SHAPES['tiny-half-tile']) if shape == 'tiny-half-tile' else dict(O=32, dims=(16, 8, 8), Cin=32, N=456)
    O, (D, H, W), Cin, N = s['O'], s['dims'], s['Cin'], s['N']
    V, M = D * H * W, O * D * H * W
    x = _rnd((O, Cin, D, H // 2, W // 2), 11).half()
    wt = _rnd((N, Cin, 3, 3, 3), 12) / np.sqrt(Cin * 27.0)
    xin = GuardedInput(dev, _cl(x.float()), torch.float16, max(D * (H // 2) * (W // 2), (H // 2 + 1) * (W // 2) + 1) * Cin)
    pc = PackedConv(wt, None, dev, up_fold=True)
    bias, rowvec, res = _rnd((N,), 13).to(dev), _rnd((O, N), 14).to(dev), _rnd((M, N), 15).to(dev)
    ws = torch.empty(M * N, device=dev)
    outs = []
    found = _options(L)
    try:
        if s.get('force256'):
            _set(L, [('conv_force256', 1)])
        for balanced in (1, 0):
            o32, o16 = GuardedOutput(dev, M, N, torch.float32), GuardedOutput(dev, M, N, torch.float16)
            st = torch.full((2, M // 64, N), float('nan'), device=dev)
            b = Builder(dev)
            cv = b.ops[b.conv(xin.view, pc, O, s['dims'], mode=hip.CONV_UP_HW, bias=bias, rowvec=View(rowvec), res=res, out_f32=o32.view,
                              out_f16=o16.view, w_fold=pc.w_fold)].u.conv
            cv.gn_stats_out = st.data_ptr()
            assert not cv.workspace
            if not balanced:
                cv.workspace, cv.splitk = ws.data_ptr(), -1
            name = C.create_string_buffer(32)
            assert (L.es_conv_kernel_of(C.byref(cv), name, 32), name.value.decode()) == (1, FOLD)
            assert L.es_conv_fold_balanced(C.byref(cv)) == balanced and L.es_conv_emits_gn_stats(C.byref(cv)) == 1
            b.finish().run()
            torch.cuda.synchronize()
            assert o32.guards_unchanged() and o16.guards_unchanged() and bool(torch.isfinite(o32.view).all())
            outs.append((o32.view.clone(), o16.view.clone(), st))
    finally:
        _set(L, found)
    assert xin.unchanged()
    (a32, a16, ast), (b32, b16, bst) = outs
    assert torch.equal(a32.view(torch.int32), b32.view(torch.int32)) and torch.equal(a16.view(torch.int16), b16.view(torch.int16))
    d = ((ast.double() - bst.double()).abs().amax((1, 2)) / bst.double().abs().amax((1, 2))).max().item()
    print('%s: outputs bit-equal; row-group sums of the two schedules differ by %.2e' % (shape, d))
    assert d <= 1e-6
