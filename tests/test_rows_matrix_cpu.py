"""Host-only checks of the rows kernel matrix (tests/rows_matrix_cases.py) and of the routing rule behind it (csrc/es_rows.hip:
rows_route, read through es_linear_rows_route_of).  No device: the query launches nothing and dereferences no operand.

  * every case takes the route its table entry names, field by field: kernel, fall-back reason, grid, block, LDS bytes, the prefetch
    descriptor, and per problem S, kbps, Jw, the cuts, the k-blocks per wave of every slice and wg0 / ny / xw / fw;
  * the matrix is complete: all 47 instantiations, every fall-back reason, every class boundary on both sides, every kernel of the
    shipped layout step and set-up GCNs, every k_rows_x instantiation with a ragged row tile, a short wave and an empty wave, every
    kernel a fused launch can select (NP = 3 of k_rows_x; k_linear_rows but its LayerNorm kernels) with a folded rider and without;
  * the routes recorded from the launchers before their decisions moved into rows_route() are reproduced (tests/golden/rows_routes.npz);
  * a row's route does not depend on M; a problem's own numbers do not depend on what it is fused with;
  * the launcher's refusals; the 2 GiB window rule; the prefetch descriptor walked as the ninth wave walks it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rows_matrix_cases as rm
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


@pytest.fixture
def family(L):
    """sets the process's kernel family for a test and puts back what it was"""
    was = L.es_rows_get_kernel_family()
    yield lambda f: L.es_rows_set_kernel_family(f)
    L.es_rows_set_kernel_family(was)


def _check_case(L, c, M=None):
    args, nxt = rm.case_args(c, M)
    got = rm.route_of(L, args, nxt)
    assert got is not None, '%s: refused: %s' % (c['name'], L.es_last_error().decode())
    assert len(got) == len(c['route']), (c['name'], [g['kernel'] for g in got])
    for li, (g, e) in enumerate(zip(got, c['route'])):
        exp = rm.expected_launch(c, e, M)
        for k, v in exp.items():
            assert g[k] == v, '%s launch %d: %s is %s, the table says %s' % (c['name'], li, k, g[k], v)
        pf = rm.NO_PREFETCH
        if e.get('prefetch'):
            pf = rm.expected_prefetch(c['next'], c['pf_nt'])
        assert g['pf'] == pf, (c['name'], g['pf'], pf)
        assert g['tparam'][:len(g['kernel'].split(','))] == [int(v) for v in g['kernel'][g['kernel'].index('<') + 1:-1].split(',')]
    return got


@pytest.mark.parametrize('c', [c for c in rm.CASES if not c['env']], ids=lambda c: c['name'])
def test_route_of_every_case(L, family, c):
    family(c['family'])
    _check_case(L, c)


def test_routes_of_the_switch_cases_in_a_child_process():
    """ES_ROWS_U1 is read once per process: the cases that need it are asked about in ONE child process that has it set"""
    names = [c['name'] for c in rm.CASES if c['env']]
    assert names and all(c['env'] == {'ES_ROWS_U1': '2'} for c in rm.CASES if c['env'])
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'import rows_matrix_cases as rm, test_rows_matrix_cpu as t\n'
            'from echoscene_amd import hip\n'
            'L = hip.lib()\n'
            'for n in %r:\n'
            '    c = rm.BY_NAME[n]; L.es_rows_set_kernel_family(c["family"]); t._check_case(L, c)\n'
            'print("ok", len(%r))\n') % (ROOT, os.path.join(ROOT, 'tests'), names, names)
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, ES_ROWS_U1='2'), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'ok %d' % len(names), out.stdout + out.stderr


def _table_launches(family=None):
    """(case, launch entry, full expected launch) of the whole table"""
    for c in rm.CASES:
        if family is None or c['family'] == family:
            for e in c['route']:
                yield c, e, rm.expected_launch(c, e)


def _wave_blocks(q, i):
    """k-blocks of the 8 waves in slice i of a k_rows_x problem"""
    n, jw = q['cut'][i + 1] - q['cut'][i], q['jws'][i]
    return [min(max(n - w * jw, 0), jw) for w in range(8)], jw


def test_the_matrix_reaches_every_instantiation_reason_and_boundary(L):
    from echoscene_amd import hip
    names = [L.es_rows_kernel_name(i).decode() for i in range(L.es_rows_kernel_count())]
    assert len(names) == 47 and len(set(names)) == 47 and L.es_rows_kernel_name(47) is None and L.es_rows_kernel_name(-1) is None
    assert sum(n.startswith('k_rows_x<') for n in names) == 20 and sum(n.startswith('k_linear_rows<') for n in names) == 27
    launches = list(_table_launches())
    reached = {e['kernel'] for _, e, _ in launches}
    assert reached == set(names), (sorted(set(names) - reached), sorted(reached - set(names)))
    # the U1 variants of plain one- and two-slab operands come from the switch only, everything else in-process
    sw = {e['kernel'] for c, e, _ in launches if c['env']}
    assert sw == {rm.K0(1, 0, u1=1), rm.K0(2, 0, u1=1)} and not sw & {e['kernel'] for c, e, _ in launches if not c['env']}
    # every fall-back reason, and only under the default family
    reasons = {x['fallback'] for c, e, x in launches if c['family'] == 1}
    # ('extent' needs an operand of 2 GiB: no case a GPU could run; test_operands_beyond_the_2gib_window_... reaches it with dummy pointers)
    assert 'extent' not in reasons and reasons | {'extent'} == set(hip.ROWS_FALLBACKS), set(hip.ROWS_FALLBACKS) ^ reasons
    assert all(x['fallback'] == 'none' for c, e, x in launches if c['family'] == 0)
    # every instantiation a fused launch can select -- the NP = 3 kernels of k_rows_x, and every k_linear_rows kernel but the eight
    # LayerNorm ones (fused problems take no LayerNorm) -- once with a folded rider, once without
    multi = [n for n in names if (n.startswith('k_rows_x<') and n.split(',')[6] == '3') or (n.startswith('k_linear_rows<') and n.split(',')[3] == '0')]
    assert len(multi) == 7 + 19
    for k in multi:
        fw = {any(q['fw'] > 0 for q in x['prob']) for _, e, x in launches if e['kernel'] == k and x['nprob'] > 1}
        assert fw == {True, False}, (k, fw)
    # every k_rows_x instantiation: a ragged last row tile, a wave with fewer blocks than Jw, a wave with no block
    for k in [n for n in names if n.startswith('k_rows_x<')]:
        ragged = short = empty = False
        for c, e, x in launches:
            if e['kernel'] != k:
                continue
            for p, q in zip(c['probs'][e['first']:], x['prob']):
                ragged = ragged or p['M'] % 16 != 0
                for i in range(q['S']):
                    nb, jw = _wave_blocks(q, i)
                    short = short or any(0 < b < jw for b in nb)
                    empty = empty or any(b == 0 for b in nb)
        assert ragged and short and empty, (k, ragged, short, empty)
    # class boundaries: slices of these widths, on whatever side of the class they fall; slab counts; residual slabs
    widths, slabs, res = set(), set(), set()
    for c in rm.CASES:
        for p in c['probs']:
            _, _, cuts = rm.slices_of(p)
            widths |= {16 * (b - a) for a, b in zip(cuts, cuts[1:])}
            slabs |= {sg['ns'] for sg in p['segs']}
            res.add(p['res'])
    assert {256, 272, 512, 528, 1024, 1040, 1536, 1552} <= widths and {1, 2, 3, 4, 5, 6, 8} <= slabs and {6, 7} <= res
    by = {c['name']: c['route'][0]['kernel'] for c in rm.CASES}
    assert by['x2-k256'] != by['x4-k272'] and by['x4-k512'] != by['x8-k528'] and by['x8-k1024'] != by['x12-k1040'] and by['x12-k1536'] != by['f0-jw13']
    assert by['x4-k512-4slab'].startswith('k_rows_x') and by['f0-5slab'].startswith('k_linear_rows')
    assert by['x2-res6-res2-6'].startswith('k_rows_x') and by['f0-res7'].startswith('k_linear_rows')


def test_the_matrix_reaches_every_kernel_of_the_shipped_plans():
    """every kernel that the layout step (model_channels 128 / 384 / 512, three conditioning variants) and the set-up GCNs launch
    under the default family, by the recorded sweep, is one the matrix runs"""
    z = np.load(os.path.join(GOLDEN, 'rows_routes.npz'))
    import make_rows_routes as mk
    stride = len(mk.LAUNCH) + 3 * len(mk.PROB)
    shipped = set()
    for ei, t in enumerate(z['tags']):
        v = z['routes'][0, ei]
        if str(t).startswith('matrix') or v[0] < 0:
            continue
        shipped |= {str(z['kernels'][v[2 + li * stride]]) for li in range(int(v[0]))}
    reached = {e['kernel'] for _, e, _ in _table_launches()}
    assert len(shipped) >= 10 and shipped <= reached, sorted(shipped - reached)


def test_recorded_routes_are_reproduced(L):
    """tests/golden/rows_routes.npz: the routes of the launchers before rows_route() existed, both families, every field"""
    import make_rows_routes as mk
    z = np.load(os.path.join(GOLDEN, 'rows_routes.npz'))
    assert [str(k) for k in z['kernels']] == [L.es_rows_kernel_name(i).decode() for i in range(L.es_rows_kernel_count())]
    entries = mk.entries_of(z)
    tags = {t for t, _, _ in entries}
    assert {'matrix ' + c['name'] for c in rm.CASES} <= tags and sum(t.startswith('layout') for t in tags) > 500 and \
        sum(t.startswith('setup') for t in tags) >= 20
    # the table's own problems are the recorded ones (a case that changed without a new recording would compare nothing)
    for c in rm.CASES:
        args, nxt = rm.case_args(c)
        ei = [t for t, _, _ in entries].index('matrix ' + c['name'])
        assert [list(r) for r in entries[ei][1]] == [mk.record(a) for a in args], c['name']
        assert (entries[ei][2] is None) == (nxt is None) and (nxt is None or list(entries[ei][2]) == mk.record(nxt)), c['name']
    ans = mk.answers(L, entries)
    diff = (ans != z['routes']).any(-1)
    assert not diff.any(), ['family %d: %s' % (1 - f, entries[e][0]) for f, e in zip(*np.nonzero(diff))][:10]
    assert (z['routes'][:, :, 0] > 0).sum() > 2000


def _without_u1(kernel):
    """the U1 variants are chosen by the number of workgroups (a timing rule: the same loads, arithmetic and order)"""
    if kernel.startswith('k_rows_x'):
        return kernel
    t = kernel[kernel.index('<') + 1:-1].split(',')
    return 'k_linear_rows<%s>' % ','.join(t[:5] + ['0'] + t[6:])


@pytest.mark.parametrize('c', [c for c in rm.CASES if not c['env'] and c['name'] not in ('x2-grid-5460', 'f0-grid-5466')], ids=lambda c: c['name'])
def test_route_does_not_depend_on_m(L, family, c):
    """the same kernel, S, kbps, Jw, cuts and k-blocks per wave at M = 5, 16, 37 and 124 rows (every problem of the case alike); what may
    move with M -- row tiles, folding, and the U1 rule that counts workgroups -- is pinned by the table at the case's own M"""
    family(c['family'])
    ref = None
    for M in (5, 16, 37, 124):
        args, nxt = rm.case_args(c, M)
        got = rm.route_of(L, args, nxt)
        assert got is not None, L.es_last_error().decode()
        key = [(_without_u1(g['kernel']), g['first'], g['fallback'],
                [(q['S'], q['kbps'], q['Jw'], q['cut'], q['jws'], q['xw'] if g['nprob'] == 1 else 0) for q in g['prob']]) for g in got]
        ref = key if ref is None else ref
        assert key == ref, (c['name'], M, key, ref)


def test_a_problems_own_numbers_do_not_depend_on_the_launch(L, family):
    """S, kbps, Jw, the cuts and the k-blocks per wave of every problem of a fused case, a folded rider included, are those of the
    problem launched alone -- and a group that splits puts every member on the very route it takes alone"""
    n = 0
    for c in rm.CASES:
        if len(c['probs']) == 1 or c['env']:
            continue
        family(c['family'])
        args, _ = rm.case_args(c)
        got = rm.route_of(L, args)
        own = lambda q: (q['S'], q['kbps'], q['Jw'], q['cut'], q['jws'])
        for g in got:
            for i in range(g['nprob']):
                alone = rm.route_of(L, [args[g['first'] + i]])
                assert len(alone) == 1
                if g['family'] == alone[0]['family']:
                    assert own(g['prob'][i]) == own(alone[0]['prob'][0]), (c['name'], i)
                else:               # (a group none of whose members k_rows_x takes... or takes alone but not fused: same S and kbps)
                    assert own(g['prob'][i])[:2] == own(alone[0]['prob'][0])[:2], (c['name'], i)
                if len(got) > 1:
                    assert {k: v for k, v in g.items() if k != 'first'} == {k: v for k, v in alone[0].items() if k != 'first'}, (c['name'], i)
                n += 1
    assert n >= 60


def _refused(L, a, text, multi=None):
    from echoscene_amd import hip
    args = multi or [a]
    arr = (C.POINTER(hip.LinearArgs) * len(args))(*[C.pointer(x) for x in args])
    info = hip.RowsRouteInfo()
    info.nlaunch = 77
    assert L.es_linear_rows_route_of(arr, len(args), None, C.byref(info)) == -1
    assert text in L.es_last_error().decode(), (text, L.es_last_error().decode())
    assert info.nlaunch == 77                      # untouched


def test_refusals(L, family):
    """every ES_REQUIRE of rows_prepare and of the route: return code -1, the launcher's own message, *out untouched"""
    from echoscene_amd import hip
    family(1)
    base = lambda **kw: rm.case_args(dict(probs=[rm.P(kw.pop('segs', [rm.S(96)]), **kw)], next=None))[0][0]
    def mod(a, **kw):
        for k, v in kw.items():
            tgt = a
            if k.startswith('seg0_'):
                tgt, k = a.seg[0], k[5:]
            setattr(tgt, k, v)
        return a
    _refused(L, mod(base(), nseg=0), 'nseg=0')
    _refused(L, mod(base(), nseg=4), 'nseg=4')
    _refused(L, mod(base(), seg0_width=94, K=94), 'multiples of 4')
    _refused(L, mod(base(), seg0_ld=102), 'multiples of 4')
    _refused(L, mod(base(segs=[rm.S(96, ns=2)]), seg0_slab_stride=4001), 'slab stride 4001')
    _refused(L, mod(base(), seg0_mode=5), 'mode 5')
    _refused(L, mod(base(segs=[rm.S(64, mode=rm.CSRWAVG)], M=7), seg0_ent_wt=None), 'weighted pooling needs')
    _refused(L, mod(base(), act=5), 'epilogue activation 5')
    _refused(L, mod(base(), K=112), 'segment widths sum to 96, K=112')
    _refused(L, mod(base(), M=0), 'empty problem')
    _refused(L, mod(base(), prologue=hip.PRO_LN), 'norm prologue without affine')
    _refused(L, mod(base(), prologue=hip.PRO_GN, gamma=0x100, beta=0x200), 'K % 128 == 0')
    _refused(L, mod(base(segs=[rm.S(128, pro=rm.PRO_SILU)]), prologue=hip.PRO_GN, gamma=0x100, beta=0x200), 'exclusive')
    _refused(L, mod(base(segs=[rm.GN(96, 8)]), seg0_beta=None), 'GroupNorm segments are direct')
    _refused(L, mod(base(segs=[rm.GN(96, 8)]), seg0_gs=12), 'GroupNorm group size 12')
    _refused(L, mod(base(segs=[rm.GN(96, 8)]), seg0_gs=64), 'GroupNorm group size 64')
    _refused(L, base(segs=[rm.LN(1040)]), 'ONE direct segment of width <= 1024')
    _refused(L, base(segs=[rm.LN(96), rm.S(16)]), 'ONE direct segment of width <= 1024')
    _refused(L, base(segs=[rm.LA(528)], res=1, res2=1), 'ES_PRO_LN_ATTN needs')
    _refused(L, mod(base(segs=[rm.LA(128)], res=1, res2=1), res2=None), 'ES_PRO_LN_ATTN needs')
    _refused(L, mod(base(segs=[rm.LA(128)], res=1, res2=1), seg0_gs=64), 'ES_PRO_LN_ATTN needs')
    _refused(L, base(segs=[rm.S(96, pro=rm.PRO_GEGLU), rm.S(16)]), 'GEGLU prologue needs one direct segment')
    _refused(L, mod(base(), seg0_pro=9), 'unknown prologue 9')
    _refused(L, mod(base(), seg0_pre_act=hip.ACT_SILU), 'segment input activation 2')
    _refused(L, base(nbatch=2, res=1), 'batched launch supports')
    _refused(L, base(N=24, act=rm.ACT_GEGLU), 'GEGLU epilogue needs N % 16 == 0')
    _refused(L, base(N=32, act=rm.ACT_GEGLU, res2=1), 'GEGLU epilogue needs N % 16 == 0')
    _refused(L, base(segs=[rm.GN(128, 32)], kbps=2, ss=1 | 2), 'would cut a GroupNorm group')         # half of 2 k-blocks: one, half a group
    _refused(L, base(segs=[rm.S(40), rm.S(56)], kbps=2, ss=1), 'multiples of 16')
    _refused(L, base(kbps=2, act=rm.ACT_RELU), 'a K split (3 slices) needs no activation epilogue')
    _refused(L, mod(base(kbps=2), out_slab_stride=8), 'a K split (3 slices) needs')
    _refused(L, base(segs=[rm.S(96, ns=9)]), '9 slabs (max 8)')
    _refused(L, base(segs=[rm.LN(96, ns=3)]), 'at most 2 slabs (3)')
    # of the route: what may not be fused, the formed row without its kernel, segment-aligned cuts k_linear_rows cannot make
    two = lambda p: rm.case_args(dict(probs=[p, rm.P([rm.S(96)])], next=None))[0]
    _refused(L, None, 'fused problems take no LayerNorm', multi=two(rm.P([rm.LN(96)])))
    _refused(L, None, 'fused problems take no LayerNorm', multi=two(rm.P([rm.S(96)], N=32, act=rm.ACT_GEGLU)))
    _refused(L, None, 'fused problems take no LayerNorm', multi=two(rm.P([rm.S(96)], nbatch=2)))
    _refused(L, base(segs=[rm.LA(128, ns=3)], res=1, res2=1), 'at most 2 slabs')
    _refused(L, base(segs=[rm.S(96, step=1), rm.S(32)], kbps=4, ss=1 | 2), 'per-segment slice lengths need k_rows_x')
    _refused(L, base(segs=[rm.S(96, step=1), rm.S(32)], kbps=4, ss=1), 'do not tile segment 0')
    family(0)
    _refused(L, base(segs=[rm.LA(128)], res=1, res2=1), 'runs on the register-operand kernel only')
    a = base(segs=[rm.LA(128)], res=1, res2=1)
    assert L.es_linear_rows_takes_ln_attn(C.byref(a)) == 0
    family(1)
    assert L.es_linear_rows_takes_ln_attn(C.byref(a)) == 1
    assert L.es_linear_rows_takes_ln_attn(C.byref(base(segs=[rm.LA(512, ns=2)], res=1, res2=1, kbps=16))) == 0     # two slices
    assert L.es_linear_rows_takes_ln_attn(C.byref(base())) == 0
    assert L.es_linear_rows_takes_ln_attn(C.byref(mod(base(), nseg=0))) == -1
    from echoscene_amd import hip as h
    arr = (C.POINTER(h.LinearArgs) * 1)(C.pointer(a))
    assert L.es_linear_rows_route_of(arr, 0, None, C.byref(h.RowsRouteInfo())) == -1 and L.es_linear_rows_route_of(arr, 4, None, C.byref(h.RowsRouteInfo())) == -1


def test_operands_beyond_the_2gib_window_stay_on_64_bit_pointers(L, family):
    """k_rows_x addresses with 32-bit byte offsets inside a 2 GiB window: an operand, output or residual whose extent reaches
    2^31 - 4096 bytes goes to k_linear_rows; one row less stays.  Gathered segments index tables and do not count M rows."""
    family(1)
    lim = (1 << 31) - 4096

    def fam(p, **kw):
        args, _ = rm.case_args(dict(probs=[p], next=None))
        a = args[0]
        for k, v in kw.items():
            setattr(a.seg[0] if k in ('ld', 'slab_stride') else a, k, v)
        r = rm.route_of(L, [a])
        assert r is not None, L.es_last_error().decode()
        return r[0]['family'], r[0]['fallback']
    M = 1 << 20
    # segment: (M * ld + width) * 4 >= lim  <=>  ld >= (lim / 4 - 96) / M
    ld_hit = -(-(lim // 4 - 96) // M)
    ld_hit += -ld_hit % 4
    p = rm.P([rm.S(96)], M=M)
    assert (M * ld_hit + 96) * 4 >= lim > (M * (ld_hit - 4) + 96) * 4
    assert fam(p, ld=ld_hit) == (0, 'extent') and fam(p, ld=ld_hit - 4) == (1, 'none')
    assert fam(rm.P([rm.S(96, mode=rm.GATHER)], M=M), ld=ld_hit) == (1, 'none')
    # slabs count: (nslab - 1) * slab_stride * 4 on top
    p2 = rm.P([rm.S(96, ns=2)], M=64)
    big = (lim - (64 * 104 + 96) * 4) // 4
    big += -big % 4
    assert fam(p2, slab_stride=big) == (0, 'extent') and fam(p2, slab_stride=big - 8) == (1, 'none')
    # output and residuals: (M * ld + N) * 4
    old_hit = -(-(lim // 4 - 24) // M)
    assert fam(p, out_ld=old_hit) == (0, 'extent') and fam(p, out_ld=old_hit - 1) == (1, 'none')
    pr = rm.P([rm.S(96)], M=M, res=1, res2=1)
    assert fam(pr, res_ld=old_hit) == (0, 'extent') and fam(pr, res2_ld=old_hit) == (0, 'extent') and fam(pr, res_ld=old_hit - 1, res2_ld=old_hit - 1) == (1, 'none')


@pytest.mark.parametrize('c', [c for c in rm.CASES if c['next'] is not None], ids=lambda c: c['name'])
def test_prefetch_descriptor_covers_exactly_the_next_weight_image(L, family, c):
    """the ninth wave of k_rows_x (es_rows_x.h), walked here from the route's fields alone: workgroup `id` of the carrying launch
    fetches, for b = id, id + w8, ... < gx (w8 = the launch's workgroups rounded down to a multiple of 8), the 1 KiB k-blocks
    cut[slice] .. cut[slice + 1] of the nt column tiles of tile b.  What that touches must be exactly the packed image of the next
    launch, es_pack_linear_f32_size(N, K) floats: every k-block of every tile, nothing behind the end -- by the workgroups below w8
    exactly once.  (The up to 7 workgroups from w8 on repeat the fetches of id - w8: the same XCD, L2 hits; counted and bounded here.)
    Fewer than 8 workgroups fetch nothing; a next op k_rows_x does not take alone gives no descriptor."""
    family(c['family'])
    args, nxt = rm.case_args(c)
    got = rm.route_of(L, args, nxt)
    g, pf = got[0], got[0]['pf']
    if not c['route'][0].get('prefetch'):
        assert pf == rm.NO_PREFETCH and g['block'] == 512
        return
    assert g['block'] == 576
    nx = c['next']
    nblocks = L.es_pack_linear_f32_size(nx['N'], nx['K']) * 4 // 1024
    assert nblocks * 1024 == L.es_pack_linear_f32_size(nx['N'], nx['K']) * 4
    total = g['grid'][0] * g['grid'][1]
    w8 = total & ~7
    S, mag = pf['S'], (32768 + pf['S'] - 1) // pf['S']
    once, again = np.zeros(nblocks + 64, dtype=np.int64), np.zeros(nblocks + 64, dtype=np.int64)
    for wid in range(total):
        b = wid
        while b < pf['gx'] and w8 > 0:
            pct = (b * mag) >> 15
            psl = b - pct * S
            assert 0 <= psl < S
            k0, nk = pf['cut'][psl], pf['cut'][psl + 1] - pf['cut'][psl]
            for t in range(pf['nt']):
                first = (pct * pf['nt'] + t) * pf['nkb_total'] + k0
                assert first + nk <= nblocks, 'workgroup %d fetches behind the end of the image' % wid
                (once if wid < w8 else again)[first:first + nk] += 1
            b += w8
    if total < 8:
        assert not once.any() and not again.any()
        return
    assert (once[:nblocks] == 1).all() and not once[nblocks:].any(), 'k-blocks fetched %s times' % sorted(set(once[:nblocks].tolist()))
    assert again.max() <= 1 and again.sum() <= (total - w8) * -(-nblocks // w8)
    # the next launch's own route reads the same image the same way
    nr = rm.route_of(L, [nxt])[0]
    assert nr['family'] == 1 and nr['grid'][0] == pf['gx'] and nr['prob'][0]['cut'] == pf['cut'] and nr['tparam'][4] == pf['nt']
