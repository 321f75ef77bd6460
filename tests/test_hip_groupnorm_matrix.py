"""GPU: every route of es_groupnorm_vol against fp64, with the route asserted (the cases and their routes: tests/side_matrix_cases.py,
whose routes tests/test_side_matrix_cpu.py checks without a GPU), and the small element-wise kernels of the volume path.

One test per case.  For every launch:
  * the route: es_groupnorm_route_of on the REAL argument struct of the plan gives the voxel tile, the tile count, the statistics
    source, whether k_gn_finalize runs, the voxels per apply block, TX and the grids that the table names, or the launch is not run
    and the test fails;
  * stray accesses (tests/guarded_buffers.py): sources, gamma / beta, row-group sums and partials handed in sit between NaN guards;
    the output, the raw copy AND the statistics scratch are NaN-filled between patterned guard rows.  Nothing outside is written,
    nothing inside an output is left unwritten, no NaN is read in (a partial that was never written, a guard) -- it would show in the
    normalised values;
  * the values: float64, by the plain formula (mean and biased variance per (object, group), (x - mean) / sqrt(var + eps) * gamma
    + beta, x * sigmoid(x) / the erf GELU), on the operands exactly as the kernel receives them (the f16 tensor for x1_is_f16).  The
    bound is PER ELEMENT:  f16 out: err <= 2^-11 |ref| + 2^-25 + s * scale;  fp32 out: err <= s * scale,  with scale = the element's
    own pre-activation magnitude |x - mean| rstd |gamma| + |beta|.  s is measured: the largest (err - rounding terms) / scale over
    the matrix on an MI355X is 4.9e-7 (f16 out, reduce-4deep-100tiles) / 7.2e-6 (fp32 out, rows-v1-c384: twelve values per group,
    k = 16 roundings in its sums at |mean| / spread = 3) (profiles/side_matrix_notes.md; run with -s to print every case's), the bar
    4 x that rounded up to one digit -- 2e-6 / 3e-5; the factor absorbs another summation order of the same number of fp32
    roundings.  By construction of the inputs a neighbouring group's or object's statistics, or a tile lost from the sums, is off by
    1e-2 and more: every (object, group) has its own mean and spread (side_matrix_cases.gn_target), gamma and beta are of order 1
    with both signs;
  * degenerate groups: an all-zero group gives beta exactly as every other (x - mean = 0, scale = |beta|).  A CONSTANT group c has
    variance 0 in exact arithmetic; the kernels form the mean from fp32 tile sums with k = vt / 4 + 2 + gs roundings (a lane's voxels,
    the two combining levels, the channels of the group), so mean = c (1 + e), |e| <= (k + 1) 2^-24 with the cast of the mean, and
    rstd <= eps^-1/2: the result is finite and within |gamma| |c| (k + 1) 2^-24 / sqrt(eps) of beta -- 1.0e-4 |gamma| at c = 0.7,
    k = 7, eps = 1e-5 -- which is the extra term of that case;
  * cancellation: the statistics are E[x^2] - mean^2 of fp32 tile sums (added up in double).  With r = |mean| / spread the relative
    errors k 2^-24 of E[x^2] = spread^2 (1 + r^2) and 2 k 2^-24 of mean^2 = spread^2 r^2 give a relative error of the variance of at
    most 3 k 2^-24 (1 + r^2), of rstd half that, and the mean is off by k 2^-24 r spreads.  The ratio cases (r = 0, 8, 64) add
    |gamma| (|x - mean| rstd 1.5 k 2^-24 (1 + r^2) + k 2^-24 r) with the group's own r to the bound and print how much of it was used
    (measured: 0.042 of it at r = 64, where (err - rounding) / scale reaches 4.7e-5; nothing at r = 0 and 8);
  * exact equalities (torch.equal): the raw copy is the fp16-rounded (fp32 out: the unchanged) input; a second run leaves the same
    bits; part_in fed with k_gn_partial's own partials gives the bits of the plain route; a launch under o_hint > O equals the
    matching objects of the whole problem run with that O.
Measured ratios and the mutation table: profiles/side_matrix_notes.md."""
import ctypes as C
import math

import pytest
import torch

import side_matrix_cases as sm
from guarded_buffers import INT_OF, GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu

# 4 x the largest measured (err - rounding terms) / scale, one significant digit, rounded up (the docstring); never above 1e-4
S_F16 = 2e-6
S_F32 = 3e-5
assert S_F16 <= 1e-4 and S_F32 <= 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(case, O=None):
    """x [O, V, C] fp32 (f16-representable for an f16 source), gamma, beta [C]"""
    O = case['O'] if O is None else O
    V, C1, C2, G = case['V'], case['C1'], case['C2'], case['groups']
    Cc = C1 + C2
    gs = Cc // G
    x = torch.randn((O, V, G, gs), generator=_gen(11), dtype=torch.float32)
    mean, spread = torch.empty(O, G), torch.empty(O, G)
    kind = case['inputs']
    for o in range(O):
        for g in range(G):
            if isinstance(kind, tuple):
                mean[o, g], spread[o, g] = (1.0 if (o + g) % 2 == 0 else -1.0) * kind[1], 1.0
            else:
                mean[o, g], spread[o, g] = sm.gn_target(o, g)
    x = x * spread[:, None, :, None] + mean[:, None, :, None]
    if kind == 'zero_group':
        x[:, :, 1 % G] = 0.0
    if kind == 'const_group':
        x[:, :, 1 % G] = 0.7
    x = x.reshape(O, V, Cc)
    if case['x1_f16']:
        x = x.half().float()
    sign = lambda t: torch.where(t < 0.5, -1.0, 1.0)
    gamma = (0.5 + torch.rand(Cc, generator=_gen(12))) * sign(torch.rand(Cc, generator=_gen(13)))
    beta = (0.05 + torch.rand(Cc, generator=_gen(14))) * sign(torch.rand(Cc, generator=_gen(15)))
    return x.contiguous(), gamma, beta


def reference(case, x, gamma, beta, dev):
    """float64 on the device: ref, scale (the pre-activation magnitude), r = |mean| rstd and |x - mean| rstd |gamma| per element"""
    O, V, Cc = x.shape
    G = case['groups']
    xd = x.to(dev).double().view(O, V, G, Cc // G)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(case['eps'], dtype=torch.float32)))       # (the kernel's eps is the fp32 value)
    ga, be = gamma.to(dev).double().view(1, 1, G, -1), beta.to(dev).double().view(1, 1, G, -1)
    lin = (xd - mean).abs() * rstd * ga.abs()
    pre = (xd - mean) * rstd * ga + be
    if case['silu'] == 1:
        ref = pre * torch.sigmoid(pre)
    elif case['silu'] == 2:
        ref = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
    else:
        ref = pre
    r = (mean.abs() * rstd).expand_as(xd)
    f = lambda t: t.reshape(O * V, Cc)
    return f(ref), f(lin + be.abs()), f(r), f(lin), f(ga.abs().expand_as(xd))


def rowgroup_sums(t, O, V):
    """[2][O * V / 64][C] fp32: per 64-row group and channel the sum and the sum of squares, as a producing conv leaves them"""
    g = t.double().view(O * V // 64, 64, -1)
    return torch.stack([g.sum(1), (g * g).sum(1)]).float()


class Launch:
    """one es_groupnorm_vol launch of a case through a plan, every buffer guarded"""

    def __init__(self, dev, case, x, gamma, beta, part_in=None, o_hint=None, O=None):
        from echoscene_amd import hip
        from echoscene_amd.plan import Builder
        import echoscene_amd.plan_vol  # noqa: F401
        self.case, self.L = case, hip.lib()
        O = case['O'] if O is None else O
        V, C1, C2, G = case['V'], case['C1'], case['C2'], case['groups']
        Cc = C1 + C2
        self.O, self.rows, self.Cc = O, O * V, Cc
        xf = x.view(O * V, Cc)
        in_dt = torch.float16 if case['x1_f16'] else torch.float32
        out_dt = torch.float32 if case['fp32'] else torch.float16
        self.inputs = [('x1', GuardedInput(dev, xf[:, :C1].contiguous(), in_dt, V * C1))]
        if C2:
            self.inputs.append(('x2', GuardedInput(dev, xf[:, C1:].contiguous(), torch.float32, V * C2)))
        self.inputs += [('gamma', GuardedInput(dev, gamma, torch.float32, Cc)), ('beta', GuardedInput(dev, beta, torch.float32, Cc))]
        ins = dict(self.inputs)
        self.y = GuardedOutput(dev, O * V, Cc, out_dt)
        self.raw = GuardedOutput(dev, O * V, Cc, out_dt) if case['raw'] else None
        need = O * ((V + 7) // 8) * G * 2 + O * G * 2                 # what es_gn_args.stats documents
        self.scratch = GuardedOutput(dev, need // 2, 2, torch.float32)
        b = Builder(dev)
        b.o_hint = case['o_hint'] if o_hint is None else o_hint
        b.fp32 = case['fp32']
        if case['src'] == 'rowgroup':
            self.inputs.append(('stats1', GuardedInput(dev, rowgroup_sums(ins['x1'].view, O, V), torch.float32, C1)))
            if C2:
                self.inputs.append(('stats2', GuardedInput(dev, rowgroup_sums(ins['x2'].view, O, V), torch.float32, C2)))
            ins = dict(self.inputs)
            if case['x1_f16']:
                b._f16_stats = {ins['x1'].view.data_ptr(): ins['stats1'].view}
        i = b.groupnorm(ins['x1'].view, C1, ins['x2'].view if C2 else None, C2, O, V, ins['gamma'].view, ins['beta'].view, case['eps'],
                        case['silu'], self.y.view, self.raw.view if self.raw else None, groups=G)
        a = b.ops[i].u.gn
        a.stats = self.scratch.view.data_ptr()
        if case['src'] == 'rowgroup':
            a.stats1 = ins['stats1'].view.data_ptr()
            a.stats2 = ins['stats2'].view.data_ptr() if C2 else None
        if part_in is not None:                                          # exactly the partials, nothing behind them but the guard
            self.inputs.append(('part_in', GuardedInput(dev, part_in, torch.float32, 64)))
            a.part_in = self.inputs[-1][1].view.data_ptr()
        self.args, self.builder = a, b
        self.route = sm.gn_route_of(self.L, a)

    def run(self):
        self.plan = self.builder.finish()
        self.plan.run()
        torch.cuda.synchronize()

    def partials(self):
        """the [O][ntiles][groups][2] partial sums k_gn_partial left at the front of the scratch"""
        n = self.O * self.route[0]['ntiles'] * self.case['groups'] * 2
        return self.scratch.view.reshape(-1)[:n].clone()

    def findings(self, tag):
        bad = []
        for nm, g in self.inputs:
            if not g.unchanged():
                bad.append('%s: input %s (or its guards) was written' % (tag, nm))
        for nm, o in (('y', self.y), ('raw', self.raw), ('stats scratch', self.scratch)):
            if o is None:
                continue
            if not o.guards_unchanged():
                bad.append('%s: the guard rows of %s were written' % (tag, nm))
            if nm != 'stats scratch' and not bool(torch.isfinite(o.view).all()):
                nf = ~torch.isfinite(o.view)
                rws = nf.any(1).nonzero().flatten()
                bad.append('%s: %s holds %d non-finite elements (never written, or computed from a guard or an unwritten partial): rows '
                           '%d..%d' % (tag, nm, int(nf.sum()), rws[0], rws[-1]))
        return bad


@pytest.mark.parametrize('case', sm.GN_CASES, ids=lambda c: c['name'])
def test_groupnorm_matrix(dev, case):
    x, gamma, beta = make_inputs(case)
    ref, scale, r, lin, ga_abs = reference(case, x, gamma, beta, dev)
    bad = []
    plain = None
    part = None
    if case['src'] == 'part_in':
        # the partials of k_gn_partial itself, from a first plan on the plain route; this launch must then leave ITS bits
        plain = Launch(dev, dict(case, src='pass'), x, gamma, beta)
        assert plain.route is not None and plain.route[0]['stats_src'] == 'pass' and plain.route[0]['ntiles'] == case['route']['ntiles']
        plain.run()
        bad += plain.findings(case['name'] + ' [plain route]')
        part = plain.partials()
        assert bool(torch.isfinite(part).all())
    ln = Launch(dev, case, x, gamma, beta, part_in=part)
    assert ln.route is not None, ln.L.es_last_error().decode()
    route, grids, _ = ln.route
    assert route == case['route'] and grids == sm.gn_grids(case), \
        '%s: routed to %s %s; the table says %s %s (not run)' % (case['name'], route, grids, case['route'], sm.gn_grids(case))
    ln.run()
    tag = case['name']
    bad += ln.findings(tag)
    y = ln.y.view.clone()
    # ---- values against fp64, per element
    err = torch.nan_to_num((y.double() - ref).abs(), nan=float('inf'))
    rounding = 0.0 if case['fp32'] else ref.abs() * 2.0 ** -11 + 2.0 ** -25
    s = S_F32 if case['fp32'] else S_F16
    extra = torch.zeros_like(ref)
    G, gs = case['groups'], (case['C1'] + case['C2']) // case['groups']
    k = case['route']['vt'] // 4 + 2 + gs                               # fp32 roundings in a tile's sums (the docstring)
    if case['inputs'] == 'const_group':
        sel = torch.zeros(G, gs, dtype=torch.bool, device=dev)
        sel[1 % G] = True
        extra = torch.where(sel.view(1, -1), ga_abs * 0.7 * (k + 1) * 2.0 ** -24 / math.sqrt(case['eps']), extra)
    if isinstance(case['inputs'], tuple):
        extra = ga_abs * (lin / ga_abs * 1.5 * k * 2.0 ** -24 * (1 + r * r) + k * 2.0 ** -24 * r)
    used = ((err - rounding).clamp(min=0) / scale).max().item()
    print('%s: largest (err - rounding) / scale = %.3e (bar s = %.0e)%s' % (tag, used, s, '' if not extra.any() else
          '; largest (err - rounding - s scale) / derived term = %.3f' % ((err - rounding - s * scale).clamp(min=0) / extra.clamp(min=1e-300)).max().item()))
    over = err - (rounding + s * scale + extra)
    if not bool((over <= 0).all()):
        wr, wc = divmod(int(over.argmax()), ref.shape[1])
        bad.append('%s: %d elements beyond the bound, worst at row %d (object %d) channel %d (group %d): got %.6g, fp64 %.6g, bound %.3e'
                   % (tag, int((over > 0).sum()), wr, wr // case['V'], wc, wc // gs, y[wr, wc].item(), ref[wr, wc].item(),
                      (rounding + s * scale + extra)[wr, wc].item() if not case['fp32'] else (s * scale + extra)[wr, wc].item()))
    # ---- exact equalities
    xin = x.view(-1, x.shape[2]).to(dev)
    if ln.raw is not None:
        want = xin if case['fp32'] else xin.half()
        if not torch.equal(ln.raw.view.view(INT_OF[want.dtype]), want.view(INT_OF[want.dtype])):
            bad.append('%s: the raw copy is not the %s input' % (tag, 'unchanged' if case['fp32'] else 'fp16-rounded'))
    if plain is not None and not torch.equal(plain.y.view.view(ln.y.it), y.view(ln.y.it)):
        bad.append('%s: part_in fed with the partials of the plain route does not give its bits (%d elements differ)'
                   % (tag, int((plain.y.view.view(ln.y.it) != y.view(ln.y.it)).sum())))
    ln.y.refill()
    ln.scratch.refill()
    ln.plan.run()
    torch.cuda.synchronize()
    if not torch.equal(ln.y.view.view(ln.y.it), y.view(ln.y.it)):
        bad.append('%s: a second run leaves other bits' % tag)
    bad += [m for m in ln.findings(tag + ' [second run]')]
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


@pytest.mark.parametrize('name', sm.GN_SHARD_CASES)
def test_a_shard_under_o_hint_equals_the_matching_objects_of_the_whole_problem(dev, name):
    """objects k .. k + O of the whole problem (O = o_hint, no hint) and the launch of those objects alone under o_hint: equal bits,
    the raw copy included; both routes asserted (the same voxel tile, the whole problem on its own grid)"""
    case = next(c for c in sm.GN_CASES if c['name'] == name)
    Ow, O, V = case['o_hint'], case['O'], case['V']
    x, gamma, beta = make_inputs(case, O=Ow)
    whole = Launch(dev, case, x, gamma, beta, o_hint=0, O=Ow)
    assert whole.route is not None and whole.route[0]['vt'] == case['route']['vt'] and whole.route[0]['ntiles'] == case['route']['ntiles']
    whole.run()
    bad = whole.findings(name + ' [whole]')
    for k in (0, Ow - O):
        shard = Launch(dev, case, x[k:k + O].contiguous(), gamma, beta)
        assert shard.route is not None and shard.route[0] == case['route']
        shard.run()
        bad += shard.findings('%s [objects %d..]' % (name, k))
        for nm, w, sh in (('y', whole.y, shard.y), ('raw', whole.raw, shard.raw)):
            if w is not None and not torch.equal(w.view[k * V:(k + O) * V].view(w.it), sh.view.view(w.it)):
                bad.append('%s: %s of objects %d.. alone differs from the whole problem\'s' % (name, nm, k))
    assert not bad, '\n'.join(bad)


def test_groupnorm_refuses_what_it_cannot_run(dev):
    """es_groupnorm_vol itself (not only the query) refuses: groups that do not divide C, an f16 source without row-group sums, part_in
    with two sources.  Nothing is launched: the output keeps its NaN fill."""
    from echoscene_amd import hip
    case = next(c for c in sm.GN_CASES if c['name'] == 'v100-last4')
    x, gamma, beta = make_inputs(case)
    for change, text in ((dict(groups=5), 'groups=5'), (dict(x1_is_f16=1), 'f16 source')):
        ln = Launch(dev, case, x, gamma, beta)
        for kk, vv in change.items():
            setattr(ln.args, kk, vv)
        with pytest.raises(RuntimeError, match=text):
            hip.check(ln.L.es_groupnorm_vol(C.byref(ln.args), hip.current_stream()), 'es_groupnorm_vol')
        torch.cuda.synchronize()
        assert bool(torch.isnan(ln.y.view).all()) and ln.y.guards_unchanged()


# ---- the small element-wise kernels ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', sm.TOCL_CASES, ids=lambda c: c['name'])
def test_to_cl_is_the_rounded_input_with_zero_padding(dev, case):
    """k_to_cl: NCDHW fp32 [O, C, V] -> channels-last [O * V, Cpad], f16 or fp32: exactly the (rounded) input, the padding exactly zero"""
    from echoscene_amd.plan import Builder
    import echoscene_amd.plan_vol  # noqa: F401
    O, Cc, V, Cpad = case['O'], case['C'], case['V'], case['Cpad']
    dt = torch.float32 if case['fp32'] else torch.float16
    x = torch.randn((O, Cc, V), generator=_gen(3)) * 3
    xin = GuardedInput(dev, x, torch.float32, Cc * V)
    out = GuardedOutput(dev, O * V, Cpad, dt)
    b = Builder(dev)
    b.to_cl(xin.view, O, Cc, V, Cpad, out.view)
    b.finish().run()
    torch.cuda.synchronize()
    assert xin.unchanged() and out.guards_unchanged()
    want = torch.zeros(O, V, Cpad, dtype=dt, device=dev)
    want[:, :, :Cc] = x.to(dev).permute(0, 2, 1).to(dt)
    assert torch.equal(out.view.view(out.it), want.view(O * V, Cpad).view(out.it))


@pytest.mark.parametrize('case', sm.GEGLU_CASES, ids=lambda c: c['name'])
def test_geglu(dev, case):
    """k_geglu: value * gelu(gate) of fp32 [M, 2 C4] against fp64, per element, with scale = |value| max(|gate|, 1).  fp32 out (the
    exact erf GELU): 8 x 2^-24 scale -- erff to a few ulp of a value <= 1 that 0.5 |gate| multiplies, three products, one sum.  f16
    out: one f16 rounding of the value, es_gelu_fast's 2.2e-7 absolute error times |value|, two fp32 roundings of the result."""
    from echoscene_amd.plan import Builder
    import echoscene_amd.plan_vol  # noqa: F401
    M, C4 = case['M'], case['C4']
    dt = torch.float32 if case['fp32'] else torch.float16
    h = torch.randn((M, 2 * C4), generator=_gen(4)) * 2
    hin = GuardedInput(dev, h, torch.float32, 2 * C4)
    out = GuardedOutput(dev, M, C4, dt)
    b = Builder(dev)
    b.geglu(hin.view, M, C4, out.view)
    b.finish().run()
    torch.cuda.synchronize()
    assert hin.unchanged() and out.guards_unchanged() and bool(torch.isfinite(out.view).all())
    v, g = h.to(dev).double().chunk(2, -1)
    ref = v * 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))
    err = (out.view.double() - ref).abs()
    scale = v.abs() * g.abs().clamp(min=1.0)
    bound = 8 * 2.0 ** -24 * scale if case['fp32'] else ref.abs() * (2.0 ** -11 + 2.0 ** -23) + 2.0 ** -25 + 2.2e-7 * v.abs()
    print('%s: largest err / bound %.3f' % (case['name'], (err / bound).max().item()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('case', sm.SPLIT_CASES, ids=lambda c: c['name'])
def test_split_operand_image(dev, case):
    """k_split_f16x3 through Builder.split3: out = [hi | lo | hi], hi = x.half() bit for bit, and hi + lo reproduces the fp32 input to
    the 22 mantissa bits its comment states: |x - hi - lo| <= 2^-22 |x| + 2^-25 (lo = f16(x - hi), |x - hi| <= 2^-11 |x|, one more
    f16 rounding of that, or the f16 subnormal step below 2^-14)"""
    from echoscene_amd.plan import Builder
    import echoscene_amd.plan_vol  # noqa: F401
    M, Cc = case['M'], case['C']
    x = torch.randn((M, Cc), generator=_gen(5)) * torch.logspace(-6, 3, Cc)
    xin = GuardedInput(dev, x, torch.float32, Cc)
    b = Builder(dev)
    out = b.split3(xin.view, Cc)
    out.fill_(float('nan'))
    b.finish().run()
    torch.cuda.synchronize()
    assert xin.unchanged() and out.shape == (M, 3 * Cc) and bool(torch.isfinite(out).all())
    hi, lo, hi2 = out[:, :Cc], out[:, Cc:2 * Cc], out[:, 2 * Cc:]
    want = x.to(dev).half()
    assert torch.equal(hi.view(torch.int16), want.view(torch.int16)) and torch.equal(hi2.view(torch.int16), want.view(torch.int16))
    xd = x.to(dev).double()
    err = (xd - hi.double() - lo.double()).abs()
    bound = xd.abs() * 2.0 ** -22 + 2.0 ** -25
    print('%s: largest |x - hi - lo| / bound %.3f' % (case['name'], (err / bound).max().item()))
    assert bool((err <= bound).all())
