"""GPU: the folded route of the up-sampling convs (k_conv_ws_fold: nearest x2 on H and W, 12 folded taps per parity class instead of 27)
against fp64, with the route asserted, on the smallest shapes at which it can go wrong:

  two-objects  O = 2, D = 16, Hi = Wi = 4, Cin = 64, N = 232: one 256-row tile per (object, parity class), two channel chunks, the
               ragged 8-column second tile;
  four-planes  O = 1, D = 4, Hi = Wi = 8, Cin = 32, N = 224: one tile spans four d-planes.

Each with all fused operands (bias, per-object vector, residual, fp32 + f16 output, row-group sums), with none of them, and with the
two halves apart (the kernel is compiled with and without the sums).  Inputs lie between NaN guards and outputs are pre-filled with NaN
between guard rows, as in tests/test_hip_conv_matrix.py, whose helpers and bound are used:

  * grid weights (multiples of 2^-6 in [-1, 1]: every folded sum of up to four taps is exact in f16): the folded route multiplies
    exactly the products of the 27-tap conv, so it must meet that test's own bound against float64, MARGIN x e32 with e32 the error
    of the same computation in fp32 on the CPU;
  * Gaussian fp32 weights (NOT pre-rounded: both routes round their weights to f16 once, the folded one after the sum): the error
    against float64 of the folded route next to the unfolded route's on the same inputs -- at most 2 x the unfolded one;
  * the f16 output is the rounded fp32 output bit for bit; the row-group sums equal the float64 sums of the stored output to 1e-5 --
    of the 64 rows a group holds on this route: the rows of an object run (parity class, d, hi, wi), and the GroupNorm that reads the
    sums adds up all groups of an object.
Measured figures: profiles/up_fold_notes.md (run with -s to print them)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_conv_matrix import GuardedInput, GuardedOutput, MARGIN, _cl, _options, _rnd, _set

pytestmark = pytest.mark.gpu

FOLD = 'ws_256_up_fold'
SHAPES = {'two-objects': dict(O=2, dims=(16, 8, 8), Cin=64, N=232), 'four-planes': dict(O=1, dims=(4, 16, 16), Cin=32, N=224)}
# (bias, rowvec, res, out_f16, stats)
CONFIGS = {'all': (True, True, True, True, True), 'none': (False, False, False, False, False),
           'operands-no-sums': (True, True, True, True, False), 'sums-only': (False, False, False, False, True)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


@functools.lru_cache(maxsize=None)
def _problem(shape, weights):
    """operands and the float64 conv (without bias / rowvec / res: added per configuration), computed once per (shape, weight set)"""
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


def _reference(p, cfg, V, dt):
    bias, rowvec, res = cfg[:3]
    y = (p['y64'] if dt == torch.float64 else p['y32']).clone()
    if bias:
        y = y + p['bias'].to(dt)
    if rowvec:
        y = y + p['rowvec'].to(dt).repeat_interleave(V, 0)
    if res:
        y = y + p['res'].to(dt)
    return y


def _launch(dev, L, s, p, pc, cfg, xin, folded):
    """one launch under conv_force256 (the shapes are far too small to reach the 256-row tiles by themselves); returns the kernel name,
    the outputs (guarded), the sums and the guarded optional inputs"""
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
        _set(L, [('conv_force256', 1)])
        b = Builder(dev)
        i = b.conv(xin.view, pc, O, dims, mode=hip.CONV_UP_HW, bias=p['bias'].to(dev) if bias else None, rowvec=View(rv.view) if rv else None,
                   res=rs.view if rs else None, out_f32=o32.view, out_f16=o16.view if o16 else None)
        cv = b.ops[i].u.conv
        if folded:
            cv.w2 = pc.w_fold.data_ptr()
        if stats:
            cv.gn_stats_out = st.data_ptr()
        name = C.create_string_buffer(32)
        S = L.es_conv_kernel_of(C.byref(cv), name, 32)
        got = (name.value.decode(), S)
        assert got == ((FOLD if folded else 'ws_256_8_4_3'), 1), 'routed to %s, S = %d (not run)' % got
        assert not stats or L.es_conv_emits_gn_stats(C.byref(cv)) == 1
        b.finish().run()
        torch.cuda.synchronize()
    finally:
        _set(L, found)
    return dict(o32=o32, o16=o16, st=st, inputs=[('rowvec', rv), ('res', rs)])


def _check(tag, s, out, ref, scale, folded, bad):
    """guards, unwritten elements, f16 = rounded fp32, row-group sums; returns the error against ref relative to the tensor scale"""
    O, (D, H, W), N = s['O'], s['dims'], s['N']
    M = O * D * H * W
    for nm, g in out['inputs']:
        if g is not None and not g.unchanged():
            bad.append('%s: input %s (or its guards) was written' % (tag, nm))
    for nm, o in (('out_f32', out['o32']), ('out_f16', out['o16'])):
        if o is None:
            continue
        if not o.guards_unchanged():
            bad.append('%s: the guard rows of %s were written' % (tag, nm))
        fin = torch.isfinite(o.view)
        if not bool(fin.all()):
            rws = (~fin).any(1).nonzero().flatten()
            bad.append('%s: %s holds %d non-finite elements (never written, or computed from a guard), rows %d..%d'
                       % (tag, nm, int((~fin).sum()), rws[0], rws[-1]))
    o32 = out['o32'].view
    e = torch.nan_to_num((o32.double() - ref).abs(), nan=float('inf')).max().item() / scale
    if out['o16'] is not None and not torch.equal(out['o16'].view.view(torch.int16), o32.half().view(torch.int16)):
        bad.append('%s: the f16 output is not the rounded fp32 output' % tag)
    if out['st'] is not None:
        y = o32.double()
        if folded:                 # the rows of an object in the order of this route's tiles: (parity class, d, hi, wi)
            y = y.view(O, D, H // 2, 2, W // 2, 2, N).permute(0, 3, 5, 1, 2, 4, 6)
        g64 = y.reshape(M // 64, 64, N)
        for k, sums in enumerate((g64.sum(1), (g64 * g64).sum(1))):
            d = torch.nan_to_num((out['st'][k].double() - sums).abs(), nan=float('inf')).max().item() / sums.abs().max().item()
            if not d < 1e-5:
                bad.append('%s: row-group sums of x^%d differ from the stored output\'s by %.3e' % (tag, k + 1, d))
    return e


@pytest.mark.parametrize('weights', ['grid', 'gauss'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_up_fold(dev, shape, weights):
    from echoscene_amd import hip
    from echoscene_amd.plan_vol import PackedConv
    L = hip.lib()
    s, p = SHAPES[shape], _problem(shape, weights)
    O, (D, H, W), Cin, N = s['O'], s['dims'], s['Cin'], s['N']
    V = D * H * W
    Hi, Wi = H // 2, W // 2
    assert (D * Hi * Wi) % 256 == 0
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
            plain = _launch(dev, L, s, p, pc, cfg, xin, False)
            eu = _check(tag + ' unfolded', s, plain, ref, scale, False, bad)
            print('%s: folded error %.3e, unfolded %.3e, ratio %.2f' % (tag, e, eu, e / eu))
            if not e <= 2 * eu:
                bad.append('%s: folded error %.3e is more than twice the unfolded route\'s %.3e' % (tag, e, eu))
        if not xin.unchanged():
            bad.append('%s: the input (or its guards) was written' % tag)
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))
