"""GPU: every conv kernel x every conv mode against fp64, with the route asserted (the cases and the routes: tests/conv_matrix_cases.py,
whose routes tests/test_conv_matrix_cpu.py checks without a GPU).

One test per case; inside it the reference is computed once and every route of the case is launched in-process under its route
options (always restored).  For every launch:
  * the route: es_conv_kernel_of on the REAL argument struct of the plan names the kernel and the split the table expects, or the
    launch is not run and the test fails -- a routing change cannot move a case onto another kernel unnoticed;
  * the values: F.conv3d in float64 on the fp16-rounded operands (+ the fp64 skip conv, bias, per-object vector, residual).  The bound
    is measured, not a constant: e32 = the max-norm relative error of the same computation in fp32 on the CPU; the fp32 output
    must be within MARGIN * e32 of the fp64 result (and never beyond the 1e-4 of the older conv tests).  MARGIN = 16: the kernels
    accumulate K = 1728 ... 1824 products in the MFMA's order, not the CPU's, and add up to 11 partial sums of a split -- a different
    order of the same number of fp32 roundings, for which a factor of a few is expected and 16 is generous; a wrong tap, a wrong mask
    or a lost K unit is off by 1e-2 and more;
  * the f16 output is the fp32 output rounded to nearest even, bit for bit (both stores cast the same fp32 value);
  * stray reads and writes: every input lies inside a larger allocation whose guards (at least one object's worth, multiples of
    256 bytes) hold NaN -- a tap read from outside the tensor poisons a stored row; every output is pre-filled with NaN between guard
    rows of a fixed bit pattern -- an element never written stays NaN, a row written outside the tensor changes a guard.  Nothing
    is read or written outside an allocation;
  * the bit-equality the sharding design rests on: whatever tile runs, the bits are those of the plain split it realises -- all
    unsplit launches are equal, k_conv_kw with 4 / 2 K streams equals the plain split of 4 / 2, a split on 64- or 128-row
    producer/consumer tiles equals the same split on k_conv_lean, the automatic split equals the explicit one;
  * the row-group sums (gn_stats_out; family A, SAME / UP_HW / DOWN_HW): formed in the epilogue exactly by the kernels that claim it,
    equal to the fp64 sums of the stored output to 1e-5, and the same bits whichever route ran.
Measured error ratios and findings: profiles/conv_matrix_notes.md (run with -s to print them)."""
import ctypes as C

import pytest
import torch

import conv_matrix_cases as cm
from conv_matrix_ref import cl as _cl, problem as _problem, rnd as _rnd, stray_findings
from guarded_buffers import INT_OF, GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu

MARGIN = 16


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _options(L):
    buf = C.create_string_buffer(1024)
    L.es_vol_options(buf, 1024)
    return [(k, int(v)) for k, v in (kv.split('=') for kv in buf.value.decode().strip(';').split(';'))]


def _set(L, pairs):
    from echoscene_amd import hip
    for k, v in pairs:
        hip.check(L.es_vol_set_option(k.encode(), int(v)), 'es_vol_set_option')


@pytest.mark.parametrize('case', cm.CASES, ids=lambda c: c['name'])
def test_conv_matrix(dev, case):
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder, View
    from echoscene_amd.plan_vol import PackedConv
    L = hip.lib()
    O, dims, N, mode = case['O'], case['dims'], case['N'], case['mode']
    V = dims[0] * dims[1] * dims[2]
    M = O * V
    p = _problem(case)
    assert 1e-8 < p['e32'] < 2e-6, 'the fp32 CPU computation is not the yardstick it is meant to be: e32 = %.3e' % p['e32']
    tol = min(MARGIN * p['e32'], 1e-4)
    ref = p['ref'].to(dev)
    ncdhw, geglu = case['out'] == 'ncdhw', case['geglu']
    rows, cols = ref.shape
    # operands, each inside its own guarded allocation; the weights are packed images of the library's own layout (tile padding inside)
    # (the 3x3x3 kernels address A from a descriptor that begins one tap halo -- (Hi + 1) Wi + 1 voxels -- in front of the tensor: the
    #  guard covers it where that is more than an object)
    Di, Hi, Wi = cm.input_dims(mode, dims)
    xin = GuardedInput(dev, _cl(p['x']), torch.float16, max(Di * Hi * Wi, (Hi + 1) * Wi + 1) * case['Cin'])
    guarded = [('a', xin)]
    pc = PackedConv(p['wt'], p['bias'], dev, geglu=geglu)
    assert pc.geglu == geglu
    skip = rowvec = res = None
    if case['Cin2']:
        a2 = GuardedInput(dev, _cl(p['xs']), torch.float16, V * case['Cin2'])
        skip = (a2.view, PackedConv(p['ws'], None, dev))
        guarded.append(('a2', a2))
    if case['rowvec']:
        rowvec = GuardedInput(dev, p['rowvec'], torch.float32, N)
        guarded.append(('rowvec', rowvec))
    if case['res']:
        res = GuardedInput(dev, p['res'], torch.float32, V * N)
        guarded.append(('res', res))
    found = _options(L)
    bad, done = [], {}
    for r in case['routes']:
        label = cm.route_label(r)
        for with_stats in ((False, True) if case['stats'] else (False,)):
            tag = '%s [%s]%s' % (case['name'], label, ' +stats' if with_stats else '')
            o32 = GuardedOutput(dev, rows, cols, torch.float32) if case['out'] != 'f16' else None
            o16 = GuardedOutput(dev, rows, cols, torch.float16) if case['out'] in ('both', 'f16') else None
            st = torch.full((2, M // 64, N), float('nan'), device=dev) if with_stats else None
            try:
                _set(L, r.options.items())
                b = Builder(dev)
                i = b.conv(xin.view, pc, O, dims, mode=mode, rowvec=View(rowvec.view) if rowvec else None, res=res.view if res else None,
                           out_f32=o32.view if o32 else None, out_f16=o16.view if o16 else None, skip=skip, ncdhw=ncdhw, splitk=r.splitk,
                           epilogue=hip.EPI_GEGLU if geglu else hip.EPI_NONE, out_ld=N // 2 if geglu else None)
                cv = b.ops[i].u.conv
                if with_stats:
                    cv.gn_stats_out = st.data_ptr()
                name = C.create_string_buffer(32)
                S = L.es_conv_kernel_of(C.byref(cv), name, 32)
                got = (name.value.decode(), S)
                if got != (cm.expected_kernel(r.kernel), r.S):
                    bad.append('%s: routed to %s, S = %d; the table says %s, S = %d (not run)' % ((tag,) + got + (r.kernel, r.S)))
                    continue
                emits = L.es_conv_emits_gn_stats(C.byref(cv))
                b.finish().run()
                torch.cuda.synchronize()
            finally:
                _set(L, found)
            me = dict(kernel=got[0], S=S, o32=o32.view.clone() if o32 else None, o16=o16.view.clone() if o16 else None, st=st)
            # ---- stray writes, unwritten elements
            bad += stray_findings(tag, guarded, (('out_f32', o32), ('out_f16', o16)))
            # ---- values against fp64
            if o32 is not None:
                err = (o32.view.double() - ref).abs()
                e = torch.nan_to_num(err, nan=float('inf')).max().item() / p['scale']
                print('%s: %s S = %d: error %.3e = %.2f x e32 (e32 = %.3e)' % (tag, got[0], S, e, e / p['e32'], p['e32']))
                if not e <= tol:
                    wr, wc = divmod(int(torch.nan_to_num(err, nan=float('inf')).argmax()), cols)
                    bad.append('%s: %s differs from fp64 by %.3e of the tensor scale = %.1f x e32 (bound %d x), worst at row %d (object %d) '
                               'column %d' % (tag, got[0], e, e / p['e32'], MARGIN, wr, wr // V if not ncdhw else wr // N, wc))
                if o16 is not None and not torch.equal(o16.view.view(torch.int16), o32.view.half().view(torch.int16)):
                    n = int((o16.view.view(torch.int16) != o32.view.half().view(torch.int16)).sum())
                    bad.append('%s: the f16 output is not the rounded fp32 output in %d elements' % (tag, n))
            else:
                # f16 only (GEGLU): one f16 rounding of the exact value (2^-11 relative, 2^-25 absolute below the normal range), the fp32
                # error of the sum as above, and es_gelu_fast's 2.2e-7 on a gate that multiplies a value of at most the tensor scale
                err = (o16.view.double() - ref).abs()
                bound = ref.abs() * 2.0 ** -11 + 2.0 ** -25 + tol * p['scale'] + 2.2e-7 * max(1.0, p['scale'])
                ex = torch.nan_to_num(err - bound, nan=float('inf'))
                print('%s: %s S = %d: f16 output, largest error / bound %.3f' % (tag, got[0], S, torch.nan_to_num(err / bound, nan=float('inf')).max().item()))
                if not bool((ex <= 0).all()):
                    wr, wc = divmod(int(ex.argmax()), cols)
                    bad.append('%s: %s: f16 output beyond one rounding of the fp64 value by %.3e at row %d column %d (%d elements)'
                               % (tag, got[0], ex.max().item(), wr, wc, int((ex > 0).sum())))
            # ---- row-group sums
            if with_stats:
                want = got[0] in cm.STATS_KERNELS and S == 1
                if emits != int(want):
                    bad.append('%s: es_conv_emits_gn_stats = %d on %s, S = %d' % (tag, emits, got[0], S))
                g64 = o32.view.double().view(M // 64, 64, N)
                for k, sums in enumerate((g64.sum(1), (g64 * g64).sum(1))):
                    d = torch.nan_to_num((st[k].double() - sums).abs(), nan=float('inf')).max().item() / sums.abs().max().item()
                    if not d < 1e-5:
                        bad.append('%s: row-group sums of x^%d differ from the stored output\'s by %.3e' % (tag, k + 1, d))
                plain = done.get((label, False))
                if plain is not None and not (torch.equal(plain['o32'], me['o32']) and torch.equal(plain['o16'], me['o16'])):
                    bad.append('%s: forming the row-group sums changed the output bits' % tag)
            done[(label, with_stats)] = me
    # ---- the bits are those of the plain split a launch realises, whatever tile ran: one class per effective split of K
    classes = {}
    for (label, with_stats), me in done.items():
        eff = {'kw_4_1': 4, 'kw_2_2': 2}.get(me['kernel'], 1) * me['S'] if not geglu else (me['kernel'] if me['kernel'].startswith('kw') else 'unsplit')
        classes.setdefault(eff, []).append(('%s%s' % (label, ' +stats' if with_stats else ''), me))
    for eff, members in sorted(classes.items(), key=lambda kv: str(kv[0])):
        l0, m0 = members[0]
        for l1, m1 in members[1:]:
            for k in ('o32', 'o16'):
                if m0[k] is not None and not torch.equal(m0[k].view(INT_OF[m0[k].dtype]), m1[k].view(INT_OF[m1[k].dtype])):
                    n = int((m0[k].view(INT_OF[m0[k].dtype]) != m1[k].view(INT_OF[m1[k].dtype])).sum())
                    bad.append('%s: %s of [%s] (%s) and of [%s] (%s) differ in %d elements; both realise a K split of %s'
                               % (case['name'], k, l0, m0['kernel'], l1, m1['kernel'], n, eff))
        with_st = [(l, m) for l, m in members if m['st'] is not None]
        for l1, m1 in with_st[1:]:
            if not torch.equal(with_st[0][1]['st'].view(torch.int32), m1['st'].view(torch.int32)):
                bad.append('%s: the row-group sums of [%s] (%s) and of [%s] (%s) differ in bits'
                           % (case['name'], with_st[0][0], with_st[0][1]['kernel'], l1, m1['kernel']))
    assert len(done) + sum('(not run)' in s for s in bad) == len(case['routes']) * (2 if case['stats'] else 1)
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


def test_up_modes_refuse_a_fused_skip(dev):
    """the nearest-up modes take no second contraction phase: the planner's query fails, nothing is launched"""
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder
    from echoscene_amd.plan_vol import PackedConv
    O, dims, Cin, Cs, N = 2, (2, 4, 4), 64, 96, 232
    b = Builder(dev)
    pc, ps = PackedConv(_rnd((N, Cin, 3, 3, 3), 1), _rnd((N,), 2), dev), PackedConv(_rnd((N, Cs), 3), None, dev)
    for mode in (hip.CONV_UP_HW, hip.CONV_UP_DHW):
        x = b.buf(O * 8, Cin, dtype=torch.float16, zero=True)
        xs = b.buf(O * 32, Cs, dtype=torch.float16, zero=True)
        with pytest.raises(RuntimeError, match='without a fused skip'):
            b.conv(x, pc, O, dims, mode=mode, out_f32=b.buf(O * 32, N, zero=True), skip=(xs, ps))
    assert len(b.ops) == 0
