"""GPU: k_conv_f32 (csrc/es_vol32.hip), the fp32-operand conv behind "the only difference is operand rounding", on the conv matrix's
families in all six modes against fp64 (the cases: tests/edge_matrix_cases.py, whose conditions tests/test_edge_matrix_cpu.py checks
without a GPU; operands, reference and guard bookkeeping: tests/conv_matrix_ref.py, shared with tests/test_hip_conv_matrix.py).

One launch per case through Builder.fp32 = True / PackedConv32 with UNROUNDED fp32 operands:
  * the op: the plan holds one ES_OP_CONV_F32 -- the launch goes to es_conv_f32, there is one kernel;
  * the values: F.conv3d in float64 on the same operands (+ the fp64 skip conv, bias, per-object vector, residual).  The bound is
    measured, not a constant: e32 = the max-norm relative error of the same computation in fp32 on the CPU, itself required to lie in
    1e-8 .. 2e-6; the kernel must be within MARGIN * e32 and never beyond the 1e-5 of test_conv_fp32_operand_route.  MARGIN = 16 as in
    the conv matrix: K = 1728 (+ 96) products accumulated in the order of v_mfma_f32_16x16x4_f32 instead of the CPU's -- the same number
    of fp32 roundings in another order; a wrong tap or mask is off by 1e-2 and more;
  * stray reads and writes: every operand -- activations, skip activations, both weight images, bias, per-object vector, residual --
    lies inside NaN guards of at least one object's worth of elements (the weights': 64 rows, the rows of the last column tile that
    `bok` keeps the kernel from reading), the output is NaN between patterned guard rows.  No element may stay NaN, no guard may change;
  * an input width that is no multiple of 16 (f32-cin40): the activations' eight pad channels hold finite random values, so the result
    is right only if the weight image's fill is exactly zero.
Measured ratios kernel / e32: profiles/edge_matrix_notes.md (run with -s to print them)."""
import pytest
import torch

import conv_matrix_cases as cm
import edge_matrix_cases as em
from conv_matrix_ref import cl, problem, rnd, stray_findings
from guarded_buffers import GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _guarded_weights(dev, pc, rows):
    """the packed image of pc inside guards of `rows` weight rows; pc.w becomes the view"""
    g = GuardedInput(dev, pc.w.cpu(), torch.float32, rows * pc.taps * pc.Cin)
    pc.w = g.view
    return g


@pytest.mark.parametrize('case', em.CONV32_CASES, ids=lambda c: c['name'])
def test_conv_f32_matrix(dev, case):
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder, View
    from echoscene_amd.plan_vol import PackedConv32
    O, dims, N, mode, Cin = case['O'], case['dims'], case['N'], case['mode'], case['Cin']
    V = dims[0] * dims[1] * dims[2]
    p = problem(case, f16_operands=False)
    assert 1e-8 < p['e32'] < 2e-6, 'the fp32 CPU computation is not the yardstick it is meant to be: e32 = %.3e' % p['e32']
    tol = min(em.MARGIN * p['e32'], 1e-5)
    ref = p['ref'].to(dev)
    ncdhw = case['out'] == 'ncdhw'
    rows, cols = ref.shape
    Di, Hi, Wi = cm.input_dims(mode, dims)
    pc = PackedConv32(p['wt'], None, dev)
    x = cl(p['x'])
    if pc.Cin != Cin:                                    # channels-last [rows, Cin16]: the pad channels finite and NOT zero
        x = torch.cat([x, rnd((x.shape[0], pc.Cin - Cin), 8)], 1).contiguous()
    guarded = [('a', GuardedInput(dev, x, torch.float32, Di * Hi * Wi * pc.Cin)), ('w', _guarded_weights(dev, pc, 64)),
               ('bias', GuardedInput(dev, p['bias'], torch.float32, N))]
    g = dict(guarded)
    skip = rowvec = res = None
    if case['Cin2']:
        ps = PackedConv32(p['ws'], None, dev)
        guarded += [('a2', GuardedInput(dev, cl(p['xs']), torch.float32, V * case['Cin2'])), ('w2', _guarded_weights(dev, ps, 64))]
        skip = (guarded[-2][1].view, ps)
    if case['rowvec']:
        guarded.append(('rowvec', GuardedInput(dev, p['rowvec'], torch.float32, N)))
        rowvec = View(guarded[-1][1].view)
    if case['res']:
        guarded.append(('res', GuardedInput(dev, p['res'], torch.float32, V * N)))
        res = guarded[-1][1].view
    out = GuardedOutput(dev, rows, cols, torch.float32)
    b = Builder(dev)
    b.fp32 = True
    i = b.conv(g['a'].view, pc, O, dims, mode=mode, bias=g['bias'].view, rowvec=rowvec, res=res, out_f32=out.view, skip=skip, ncdhw=ncdhw)
    assert len(b.ops) == 1 and b.ops[i].kind == hip.OP_CONV_F32
    b.finish().run()
    torch.cuda.synchronize()
    tag = case['name']
    bad = stray_findings(tag, guarded, (('out_f32', out),))
    err = torch.nan_to_num((out.view.double() - ref).abs(), nan=float('inf'))
    e = err.max().item() / p['scale']
    print('%s: error %.3e = %.2f x e32 (e32 = %.3e)' % (tag, e, e / p['e32'], p['e32']))
    if not e <= tol:
        wr, wc = divmod(int(err.argmax()), cols)
        bad.append('%s: k_conv_f32 differs from fp64 by %.3e of the tensor scale = %.1f x e32 (bound %d x, and 1e-5), %d elements beyond it, '
                   'worst at row %d (object %d) column %d' % (tag, e, e / p['e32'], em.MARGIN, int((err > tol * p['scale']).sum()), wr,
                                                              wr // V if not ncdhw else wr // N, wc))
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))
