"""GPU: the kernels around the UNet of the volume path against float64, launched from guarded buffers (tests/guarded_buffers.py) --
k_vq_lookup, k_stem1 / k_stem2, k_conv_c1 and k_layernorm (the cases, inputs and references: tests/edge_matrix_cases.py, whose own
conditions tests/test_edge_matrix_cpu.py checks without a GPU; k_conv_f32: tests/test_hip_conv32_matrix.py).

  * k_vq_lookup, through es_vq_lookup with idx_out given.  Reference: float64 distances |z|^2 + |e|^2 - 2 z.e.  Every index returned
    must satisfy D64[idx] - min D64 <= 16 u S at the larger S = |z|^2 + |e|^2 + 2 sum |z_i e_i| of the two candidates (u = 2^-24: the
    kernel's expression has under 8 roundings per candidate).  Families: varied (at most 1 % of the voxels may differ from the float64
    first minimum at all; the CPU file holds the reference's own undecided share under 0.5 %), on-code (the index is that row),
    duplicates (equal rows j1 < j2: the index is j1, the documented first minimum), decidable near-ties (the gap is 64 x the bound,
    both sides: the right side every time).  out[m, :3] has the bits of lut[idx].half(), out[m, 3:] is exactly zero; a second
    launch with idx_out = NULL leaves the same bits;
  * the stem, through Builder.stem: O = 1 / 3, three / four input channels, x_ostride = 0 / larger than an object with NaN between
    the objects; varied, all-negative and far-window inputs.  Reference: the four layers in float64.  Bound: per element, MARGIN x the
    measured error of the same layers in fp32 on the CPU, against the scale of the output;
  * k_conv_c1, through Builder.conv_c1 (the f16 output set on the op's arguments: the builder offers none): N = 16 / 32 / 64 / 128,
    one voxel block whose halo is all padding and a grid whose interior block faces take their halo from neighbours, O = 2, fp32 /
    f16 / both outputs, bias given / NULL.  Float64 reference, the bound from the measured fp32 CPU error; the f16 output is the fp32
    output rounded to nearest even, bit for bit;
  * k_layernorm, through Builder.layernorm, fp32 and f16 output: widths with one to four chunks per lane and partial chunks, more
    rows than resident waves; varied rows, rows whose mean is 10 / 1000 spreads, constant rows.  Per element
    |y - y64| <= MARGIN E w, w = |gamma| (|x - mean| + |mean|) rstd + |beta| (the row's conditioning 1 + |mean| rstd on the normalised
    term), E = the largest error / w of a two-pass fp32 LayerNorm on the CPU.  The f16 output is the fp32 output rounded to nearest
    even, bit for bit (both stores cast the same fp32 value).
Every input lies between NaN guards (x of the LayerNorm: one row's worth, which the prefetch of row + nw would reach), every output and
the stem's scratch are NaN between patterned guard rows: no element may stay NaN, no guard may change.
Measured ratios and counts: profiles/edge_matrix_notes.md (run with -s to print them)."""
import ctypes as C

import pytest
import torch

import edge_matrix_cases as em
from conv_matrix_ref import stray_findings
from guarded_buffers import GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _run(b):
    b.finish().run()
    torch.cuda.synchronize()


# ---- k_vq_lookup ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', em.VQ_CASES, ids=lambda c: c['name'])
def test_vq_lookup(dev, case):
    from echoscene_amd import hip
    L = hip.lib()
    n, O, V, Cpad = case['n_embed'], case['O'], case['V'], case['Cpad']
    M = O * V
    bad = []
    for fam in em.VQ_FAMILIES:
        p = em.vq_problem(case['name'], fam)
        tag = '%s %s' % (case['name'], fam)
        ins = [(nm, GuardedInput(dev, torch.from_numpy(p[nm]), torch.float32, unit)) for nm, unit in (('z', 3 * V), ('codebook', 3 * n), ('lut', 3 * n))]
        g = dict(ins)
        out = GuardedOutput(dev, M, Cpad, torch.float16)
        idx = GuardedOutput(dev, M, 1, torch.float32)            # int32 indices; the NaN fill reads as an index far outside the codebook
        a = hip.VQArgs()
        a.z, a.codebook, a.lut = g['z'].view.data_ptr(), g['codebook'].view.data_ptr(), g['lut'].view.data_ptr()
        a.O, a.V, a.n_embed, a.Cpad = O, V, n, Cpad
        a.idx_out, a.out_f16 = idx.view.data_ptr(), out.view.data_ptr()
        hip.check(L.es_vq_lookup(C.byref(a), hip.current_stream()), 'es_vq_lookup')
        torch.cuda.synchronize()
        bad += stray_findings(tag, ins, (('out_f16', out),))
        if not idx.guards_unchanged():
            bad.append('%s: the guard rows of idx_out were written' % tag)
        got = idx.view.view(torch.int32).flatten().cpu().numpy()
        found, differ = em.vq_check_indices(p, got)
        bad += ['%s: %s' % (tag, f) for f in found]
        print('%s: %d of %d voxels differ from the float64 first minimum' % (tag, differ, M))
        if differ > (0.01 * M if fam == 'varied' else 0):
            bad.append('%s: %d of %d voxels differ from the float64 first minimum' % (tag, differ, M))
        if not found:
            want = torch.zeros(M, Cpad, dtype=torch.float16)
            want[:, :3] = torch.from_numpy(p['lut'])[torch.from_numpy(got).long()].half()
            if not torch.equal(out.view.cpu().view(torch.int16), want.view(torch.int16)):
                bad.append('%s: out_f16 is not lut[idx_out].half() with zero padding in %d elements'
                           % (tag, int((out.view.cpu().view(torch.int16) != want.view(torch.int16)).sum())))
        # ---- the product's form: no indices asked for
        first = out.view.clone()
        out.refill()
        a.idx_out = None
        hip.check(L.es_vq_lookup(C.byref(a), hip.current_stream()), 'es_vq_lookup')
        torch.cuda.synchronize()
        bad += stray_findings(tag + ' [idx_out = NULL]', ins, (('out_f16', out),))
        if not torch.equal(out.view.view(torch.int16), first.view(torch.int16)):
            bad.append('%s: idx_out = NULL leaves other bits in out_f16' % tag)
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


# ---- the conv-pool stem -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('O,cin,gap', em.STEM_LAUNCHES, ids=lambda v: str(v))
def test_shape_stem(dev, O, cin, gap):
    from echoscene_amd.plan import Builder
    bad = []
    for fam in em.STEM_FAMILIES:
        x, w = em.stem_problem(O, cin, fam)
        tag = 'stem O=%d cin=%d ostride=%s %s' % (O, cin, 'cin*4096+%d' % gap if gap else '0', fam)
        ref = em.stem_reference(x, w, torch.float64)[2]
        scale = ref.abs().max().item()
        e32 = (em.stem_reference(x, w, torch.float32)[2].double() - ref).abs().max().item() / scale
        assert 1e-8 < e32 < 2e-6, '%s: the fp32 CPU computation is not the yardstick it is meant to be: e32 = %.3e' % (tag, e32)
        ostride = cin * 4096 + gap if gap else 0
        xf = x.reshape(O, -1)
        if gap:                                          # NaN between (and behind) the objects
            xf = torch.cat([xf, torch.full((O, gap), float('nan'))], 1)
        ins = [('x', GuardedInput(dev, xf, torch.float32, cin * 4096))] + \
              [(nm, GuardedInput(dev, t.reshape(-1), torch.float32, t.numel())) for nm, t in zip(('w0', 'b0', 'w1', 'b1'), w)]
        scratch, out = GuardedOutput(dev, O * 32, 512, torch.float32), GuardedOutput(dev, O, 512, torch.float32)
        b = Builder(dev)
        b.stem(ins[0][1].view, [g.view for _, g in ins[1:]], scratch.view, out.view, O, cin=cin, ostride=ostride)
        _run(b)
        bad += stray_findings(tag, ins, (('scratch', scratch), ('out', out)))
        err = torch.nan_to_num((out.view.double().cpu() - ref).abs(), nan=float('inf'))
        e = err.max().item() / scale
        print('%s: error %.3e = %.2f x e32 (e32 = %.3e)' % (tag, e, e / e32, e32))
        if not e <= em.MARGIN * e32:
            wo, wi = divmod(int(err.argmax()), 512)
            bad.append('%s: differs from fp64 by %.3e of the output scale = %.1f x e32 (bound %d x) in %d elements, worst at object %d channel '
                       '%d window %d: got %.6g, fp64 %.6g' % (tag, e, e / e32, em.MARGIN, int((err > em.MARGIN * e32 * scale).sum()), wo, wi // 8,
                                                             wi % 8, out.view[wo, wi].item(), ref[wo, wi].item()))
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


# ---- k_conv_c1 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,dims', em.C1_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_conv_c1(dev, N, dims):
    from echoscene_amd.plan import Builder
    O, V = em.C1_O, dims[0] * dims[1] * dims[2]
    x, wt, bias, refs = em.c1_problem(N, dims)
    ins = [('x', GuardedInput(dev, x.reshape(O, V), torch.float32, V)), ('w', GuardedInput(dev, wt.reshape(N, 27), torch.float32, 27 * N)),
           ('bias', GuardedInput(dev, bias, torch.float32, N))]
    g = dict(ins)
    bad = []
    for with_bias in (True, False):
        r = refs[with_bias]
        assert 1e-8 < r['e32'] < 2e-6, 'the fp32 CPU computation is not the yardstick it is meant to be: e32 = %.3e' % r['e32']
        ref = r['ref'].to(dev)
        seen = {}
        for outs in em.C1_OUTPUTS:
            tag = 'conv_c1 N=%d %s %s %s' % (N, dims, 'bias' if with_bias else 'bias=NULL', outs)
            o32 = GuardedOutput(dev, O * V, N, torch.float32) if outs != 'f16' else None
            o16 = GuardedOutput(dev, O * V, N, torch.float16) if outs != 'f32' else None
            b = Builder(dev)
            i = b.conv_c1(g['x'].view, g['w'].view, g['bias'].view if with_bias else None, O, dims, (o32 or o16).view)
            a = b.ops[i].u.conv_c1
            a.out_f32 = o32.view.data_ptr() if o32 else None
            a.out_f16 = o16.view.data_ptr() if o16 else None
            _run(b)
            bad += stray_findings(tag, ins, (('out_f32', o32), ('out_f16', o16)))
            if o32 is not None:
                err = torch.nan_to_num((o32.view.double() - ref).abs(), nan=float('inf'))
                e = err.max().item() / r['scale']
                print('%s: error %.3e = %.2f x e32 (e32 = %.3e)' % (tag, e, e / r['e32'], r['e32']))
                if not e <= em.MARGIN * r['e32']:
                    wr, wc = divmod(int(err.argmax()), N)
                    bad.append('%s: differs from fp64 by %.3e of the tensor scale = %.1f x e32 (bound %d x) in %d elements, worst at row %d '
                               '(object %d) channel %d' % (tag, e, e / r['e32'], em.MARGIN, int((err > em.MARGIN * r['e32'] * r['scale']).sum()),
                                                           wr, wr // V, wc))
                if seen and not torch.equal(seen['o32'].view(torch.int32), o32.view.view(torch.int32)):
                    bad.append('%s: the fp32 output differs in bits from the fp32-only launch' % tag)
                seen.setdefault('o32', o32.view.clone())
            if o16 is not None and not torch.equal(o16.view.view(torch.int16), seen['o32'].half().view(torch.int16)):
                bad.append('%s: the f16 output is not the rounded fp32 output in %d elements'
                           % (tag, int((o16.view.view(torch.int16) != seen['o32'].half().view(torch.int16)).sum())))
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


# ---- k_layernorm ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family', em.LN_FAMILIES)
@pytest.mark.parametrize('M,Cc', em.LN_SHAPES)
def test_layernorm_tokens(dev, M, Cc, family):
    from echoscene_amd.plan import Builder
    x, gamma, beta = em.ln_problem(M, Cc, family)
    ref, w, E = em.ln_yardstick(x, gamma, beta)
    assert 2.0 ** -27 < E < 2.0 ** -20, 'the two-pass fp32 LayerNorm is not the yardstick it is meant to be: E = %.3e' % E
    ins = [('x', GuardedInput(dev, x, torch.float32, Cc)), ('gamma', GuardedInput(dev, gamma, torch.float32, Cc)),
           ('beta', GuardedInput(dev, beta, torch.float32, Cc))]
    g = dict(ins)
    y32, y16 = GuardedOutput(dev, M, Cc, torch.float32), GuardedOutput(dev, M, Cc, torch.float16)
    b = Builder(dev)
    b.layernorm(g['x'].view, M, Cc, g['gamma'].view, g['beta'].view, y32.view)
    b.layernorm(g['x'].view, M, Cc, g['gamma'].view, g['beta'].view, y16.view)
    assert [op.u.ln.y_is_f32 for op in b.ops] == [1, 0]
    _run(b)
    tag = 'layernorm %dx%d %s' % (M, Cc, family)
    bad = stray_findings(tag, ins, (('y fp32', y32), ('y f16', y16)))
    ref, w = ref.to(dev), w.to(dev)
    err = torch.nan_to_num((y32.view.double() - ref).abs(), nan=float('inf'))
    used = (err / w).max().item()
    print('%s: largest err / w = %.3e = %.2f x E (E = %.3e)' % (tag, used, used / E, E))
    over = err - em.MARGIN * E * w
    if not bool((over <= 0).all()):
        wr, wc = divmod(int((err / w).argmax()), Cc)
        bad.append('%s: %d elements beyond the bound (%.1f x E, bound %d x), worst at row %d column %d: got %.7g, fp64 %.7g'
                   % (tag, int((over > 0).sum()), used / E, em.MARGIN, wr, wc, y32.view[wr, wc].item(), ref[wr, wc].item()))
    if family == 'const_row':                            # float64 gives beta exactly (the CPU file): the bound above is "beta up to it"
        rows = torch.tensor([0, M // 2, M - 1], device=dev)
        dev_beta = (y32.view[rows].double() - beta.to(dev).double()).abs()
        print('%s: constant rows: largest |y - beta| / bound %.3f' % (tag, (dev_beta / (em.MARGIN * E * w[rows])).max().item()))
    if not torch.equal(y16.view.view(torch.int16), y32.view.half().view(torch.int16)):
        bad.append('%s: the f16 output is not the rounded fp32 output in %d elements'
                   % (tag, int((y16.view.view(torch.int16) != y32.view.half().view(torch.int16)).sum())))
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))

