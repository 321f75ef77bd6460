"""The rows kernel matrix: cases, their argument structs and the routes they must take (tests/test_rows_matrix_cpu.py checks the
routes without a GPU, tests/test_hip_rows_matrix.py runs every case on its route).  A plain module: no fixtures, no test.

A case = up to three problems of ONE launch call (es_linear_rows_f32 / es_linear_rows_multi_f32), the kernel family the process is
set to, an optional next op (the prefetch hint) and the expected route.  A problem is a small dict (P(...)) of segments (S(...));
`geometry()` derives every leading dimension, stride and buffer size from it, `make_args()` fills the es_linear_args from a table of
addresses -- dummy ones for the host-only route query, guarded device buffers on the GPU -- so both tests ask about the same structs.

Shapes are the smallest that reach the route: N = 24 (two column tiles, the second ragged), M = 37 (three row tiles, the last with 5
rows) unless the route needs otherwise.  Slices are set explicitly (kbps / ss = kb_per_slice / seg_slices), never planned.

What the table names by hand per launch: the kernel, the fall-back reason, per problem S and Jw.  Grid, block, LDS, cuts, the
k-blocks per wave of every slice and the tile bookkeeping of fused launches are derived here from the documented rules
(expected_launch) -- a second statement of them, independent of the library's."""
import ctypes as C

DIRECT, GATHER, CSRMEAN, CSRSUM, CSRWAVG = 0, 1, 2, 3, 4
PRO_NONE, PRO_SILU, PRO_GN, PRO_GN_SILU, PRO_LN, PRO_GEGLU, PRO_LN_ATTN = 0, 1, 2, 3, 4, 5, 6
ACT_NONE, ACT_RELU, ACT_SILU, ACT_GEGLU, ACT_SIGMOID = 0, 1, 2, 3, 4
NSTEP, STEP = 3, 2                       # step-indexed operands: tables of 3 rows, the device counter holds 2
CSR_T = 30                               # source rows (triples) of a CSR segment
CSR_DEG = (0, 1, 12, 13, 25, 3, 0)       # entries per node: none, one, the 12-entry batches and their edges, two batches and one


def S(w, ns=1, mode=DIRECT, relu=0, pro=PRO_NONE, gs=0, affine=1, step=0, inputs='spread'):
    """one segment: width, slabs, mode, ReLU on the slab sum, prologue (gs: GroupNorm group size), affine vectors present,
    step-indexed; inputs: 'spread' (every (row, group) its own mean and spread), 'const' (one constant group), 'ratio' (|mean| / spread = 64)"""
    return dict(w=w, ns=ns, mode=mode, relu=relu, pro=pro, gs=gs, affine=affine, step=step, inputs=inputs)


def P(segs, M=37, N=24, kbps=0, ss=0, act=ACT_NONE, bias=1, res=0, res2=0, res_step=0, nbatch=1, eps=1e-5):
    """one problem: res / res2 = slab count of the residuals (0: none)"""
    return dict(segs=segs, M=M, N=N, K=sum(s['w'] for s in segs), kbps=kbps, ss=ss, act=act, bias=bias, res=res, res2=res2,
                res_step=res_step, nbatch=nbatch, eps=eps)


def nout(p):
    return p['N'] // 2 if p['act'] == ACT_GEGLU else p['N']


def is_lnattn(p):
    return p['segs'][0]['pro'] == PRO_LN_ATTN


def csr_entries(M, w):
    """row pointers, source rows and column offsets of a CSR segment: node m has CSR_DEG[m % 7] entries, the source rows walk through
    the table with a stride coprime to it, the slot (column offset 0 or w + 8) alternates with a period of 3"""
    ptr, rows, offs = [0], [], []
    e = 0
    for m in range(M):
        for _ in range(CSR_DEG[m % len(CSR_DEG)]):
            rows.append((7 * e + 3) % CSR_T)
            offs.append(0 if e % 3 else w + 8)
            e += 1
        ptr.append(len(rows))
    return ptr, rows, offs


def gather_index(M, rows):
    """a non-identity map with repeats that hits the last table row"""
    idx = [(5 * m + 2) % rows for m in range(M)]
    idx[0] = rows - 1
    if M > 3:
        idx[3] = idx[1]
    return idx


def geometry(p):
    """every buffer of a problem: name -> (floats or ints, dtype); and the strides.  Returns (bufs, g)"""
    M, N, K = p['M'], p['N'], p['K']
    g, bufs = dict(seg=[]), {}
    for s, sg in enumerate(p['segs']):
        w = sg['w']
        d = dict()
        if sg['pro'] == PRO_GEGLU:
            d['ld'] = 2 * K + 8
        elif sg['pro'] == PRO_LN_ATTN:
            d['gs'] = w + 8
            d['ld'] = d['gs'] + w + 8
        elif sg['mode'] >= CSRMEAN:
            d['ld'] = 2 * w + 16
        else:
            d['ld'] = w + 8
        d['rows'] = M + 11 if sg['mode'] == GATHER else CSR_T if sg['mode'] >= CSRMEAN else M
        d['mat'] = d['rows'] * d['ld'] + (8 if p['nbatch'] > 1 else 0)
        d['sstr'] = d['mat'] + 16
        d['step_stride'] = d['mat'] * max(sg['ns'], 1) + 16 * max(sg['ns'], 1) + 8
        nmat = (NSTEP if sg['step'] else 1) * p['nbatch']
        d['floats'] = nmat * d['mat'] if sg['ns'] <= 1 and not sg['step'] else (NSTEP if sg['step'] else 1) * d['step_stride']
        bufs['a%d' % s] = (d['floats'], 'f')
        if sg['mode'] == GATHER:
            bufs['idx%d' % s] = (M, 'i')
        if sg['mode'] >= CSRMEAN:
            ptr, rows, offs = csr_entries(M, w)
            bufs['idx%d' % s], bufs['ent_row%d' % s], bufs['ent_off%d' % s] = (M + 1, 'i'), (max(len(rows), 1), 'i'), (max(len(offs), 1), 'i')
            if sg['mode'] == CSRWAVG:
                bufs['ent_wt%d' % s] = (2 * CSR_T, 'f')
        if sg['step']:
            bufs['step'] = (1, 'i')
        if sg['pro'] in (PRO_GN, PRO_GN_SILU, PRO_LN) and sg['affine']:
            bufs['gamma%d' % s], bufs['beta%d' % s] = (w, 'f'), (w, 'f')
        g['seg'].append(d)
    No = nout(p)
    g['wfloats'] = ((N + 15) // 16) * ((K + 15) // 16) * 256
    bufs['w'] = (g['wfloats'] * p['nbatch'], 'f')
    if p['bias']:
        bufs['bias'] = (N * p['nbatch'], 'f')
    g['out_ld'] = No + 8
    g['out_mat'] = M * g['out_ld']
    g['out_sstr'] = g['out_bstride'] = (M + 2) * g['out_ld']          # two spare rows between slabs / batches
    if is_lnattn(p):
        w = p['segs'][0]['w']
        g['res_ld'], g['res2_ld'] = w + 4, w + 12
        bufs['res'], bufs['res2'] = (M * g['res_ld'], 'f'), (M * g['res2_ld'], 'f')
    else:
        g['res_ld'], g['res2_ld'] = No + 4, No + 12
        g['res_sstr'], g['res2_sstr'] = M * g['res_ld'] + 8, M * g['res2_ld'] + 8
        g['res_step_stride'] = M * g['res_ld'] + 12
        if p['res']:
            bufs['res'] = (NSTEP * g['res_step_stride'] if p['res_step'] else p['res'] * g['res_sstr'], 'f')
            if p['res_step']:
                bufs['step'] = (1, 'i')
        if p['res2']:
            bufs['res2'] = (p['res2'] * g['res2_sstr'], 'f')
    return bufs, g


def make_args(p, addr, S_out=1):
    """the es_linear_args of a problem; addr: name -> address of the buffer of that name (geometry()); S_out: the slab count of the
    output (only tells whether out_slab_stride is set)"""
    from echoscene_amd import hip
    bufs, g = geometry(p)
    a = hip.LinearArgs()
    a.nseg, a.M, a.K, a.N = len(p['segs']), p['M'], p['K'], p['N']
    for s, sg in enumerate(p['segs']):
        d, q = g['seg'][s], a.seg[s]
        q.ptr, q.ld, q.width, q.mode = addr['a%d' % s], d['ld'], sg['w'], sg['mode']
        if sg['ns'] > 1:
            q.nslab, q.slab_stride = sg['ns'], d['sstr']
        q.pre_act = ACT_RELU if sg['relu'] else ACT_NONE
        q.pro, q.eps = sg['pro'], p['eps']
        q.gs = d.get('gs', sg['gs'])
        if sg['pro'] == PRO_LN:
            q.gs = sg['w']
        if 'gamma%d' % s in bufs:
            q.gamma, q.beta = addr['gamma%d' % s], addr['beta%d' % s]
        if sg['mode'] == GATHER or sg['mode'] >= CSRMEAN:
            q.idx = addr['idx%d' % s]
        if sg['mode'] >= CSRMEAN:
            q.ent_row, q.ent_off = addr['ent_row%d' % s], addr['ent_off%d' % s]
        if sg['mode'] == CSRWAVG:
            q.ent_wt = addr['ent_wt%d' % s]
        if sg['step']:
            q.step, q.step_stride = addr['step'], d['step_stride']
    a.wpack = addr['w']
    a.bias = addr['bias'] if p['bias'] else None
    a.eps, a.act = p['eps'], p['act']
    if 'res' in bufs:
        a.res, a.res_ld = addr['res'], g['res_ld']
        if p['res'] > 1:
            a.res_nslab, a.res_slab_stride = p['res'], g['res_sstr']
        if p['res_step']:
            a.res_step, a.res_step_stride = addr['step'], g['res_step_stride']
    if 'res2' in bufs:
        a.res2, a.res2_ld = addr['res2'], g['res2_ld']
        if p['res2'] > 1:
            a.res2_nslab, a.res2_slab_stride = p['res2'], g['res2_sstr']
    a.out, a.out_ld = addr['out'], g['out_ld']
    if p['nbatch'] > 1:
        a.nbatch, a.a_bstride, a.out_bstride = p['nbatch'], g['seg'][0]['mat'], g['out_bstride']
    a.kb_per_slice, a.seg_slices = p['kbps'], p['ss']
    a.out_slab_stride = g['out_sstr']
    return a


def dummy_addresses(p, base):
    """addresses nobody dereferences, 256-byte aligned, laid out back to back from `base`; returns (addr, end)"""
    bufs, g = geometry(p)
    addr, at = {}, base
    for name, (n, _) in list(bufs.items()) + [('out', (8 * (g['out_sstr'] + 64), 'f'))]:
        addr[name] = at
        at += (4 * n + 255) // 256 * 256 + 256
    return addr, at


def route_of(L, args, nxt=None):
    """the library's route of the launch call on these es_linear_args as plain Python data, or None (es_last_error tells why)"""
    from echoscene_amd import hip
    arr = (C.POINTER(hip.LinearArgs) * len(args))(*[C.pointer(a) for a in args])
    info = hip.RowsRouteInfo()
    if L.es_linear_rows_route_of(arr, len(args), None if nxt is None else C.byref(nxt), C.byref(info)) != 0:
        return None
    out = []
    for li in range(info.nlaunch):
        l = info.launch[li]
        d = dict(family=l.family, kernel=l.name.decode(), index=l.kernel, tparam=list(l.tparam), first=l.first, nprob=l.nprob,
                 grid=(l.grid_x, l.grid_y, l.grid_z), block=l.block, lds=l.lds, fallback=hip.ROWS_FALLBACKS[l.fallback],
                 pf=dict(gx=l.pf_gx, nt=l.pf_nt, nkb_total=l.pf_nkb_total, S=l.pf_S, cut=list(l.pf_cut)), prob=[])
        for i in range(l.nprob):
            q = l.prob[i]
            d['prob'].append(dict(S=q.S, kbps=q.kbps, Jw=q.Jw, cut=list(q.cut), jws=list(q.jws), wg0=q.wg0, ny=q.ny, xw=q.xw, fw=q.fw))
        out.append(d)
    return out


def case_args(case, M=None):
    """the es_linear_args of a case's problems (and of its next op) over dummy addresses"""
    base, args = 0x10000000, []
    for p in case['probs']:
        p = dict(p, M=p['M'] if M is None else M)
        addr, base = dummy_addresses(p, base)
        args.append(make_args(p, addr))
    nxt = None
    if case.get('next') is not None:
        addr, base = dummy_addresses(case['next'], base)
        nxt = make_args(case['next'], addr)
    return args, nxt


# ---- the documented rules, stated a second time ----------------------------------------------------------------------------------------------

def slices_of(p):
    """(S, rounded kbps, cuts) of a problem from kb_per_slice / seg_slices: the rule of es_linear_rows_slices"""
    nkb = (p['K'] + 15) // 16
    kal = 1
    for sg in p['segs']:
        if sg['pro'] in (PRO_GN, PRO_GN_SILU) and sg['gs'] > 16 * kal:
            kal = (sg['gs'] + 15) // 16
    kbps = p['kbps']
    if kbps <= 0 or kbps >= nkb:
        return 1, nkb, [0, nkb]
    kbps = (kbps + kal - 1) // kal * kal
    if kbps >= nkb:
        return 1, nkb, [0, nkb]
    cuts = []
    if p['ss']:
        kb = 0
        for s, sg in enumerate(p['segs']):
            step = (kbps + 1) // 2 if (p['ss'] >> (1 + s)) & 1 else kbps
            cuts += list(range(kb, kb + sg['w'] // 16, step))
            kb += sg['w'] // 16
    else:
        cuts = list(range(0, nkb, kbps))
    return len(cuts), kbps, cuts + [nkb]


def seg_of_kblock(p, kb):
    c = 0
    for sg in p['segs']:
        c += sg['w'] // 16
        if kb < c:
            return sg
    return p['segs'][-1]


def expected_launch(case, exp, M=None):
    """the full route of one launch of a case: the hand-named fields of `exp` plus everything the rules derive"""
    probs = [dict(p, M=p['M'] if M is None else M) for p in case['probs'][exp['first']:exp['first'] + exp['nprob']]]
    fam = 1 if exp['kernel'].startswith('k_rows_x') else 0
    tp = [int(v) for v in exp['kernel'][exp['kernel'].index('<') + 1:-1].split(',')]
    n = len(probs)
    out = dict(family=fam, kernel=exp['kernel'], first=exp['first'], nprob=n, fallback=exp.get('fallback', 'none'), prob=[])
    gy = max((p['M'] + 15) // 16 for p in probs)
    gx, kcmax = 0, 16
    for p, e in zip(probs, exp['prob']):
        Sn, kbps, cuts = slices_of(p)
        assert Sn == e['S'], (case['name'], Sn, e)
        ny, xw = (p['M'] + 15) // 16, (p['N'] + 15) // 16 * Sn
        fw = (xw * ny + gy - 1) // gy if n > 1 and ny < gy else 0
        q = dict(S=Sn, kbps=kbps, Jw=e.get('Jw', 0) if fam else 0, cut=[0] * 7, jws=[0] * 6, wg0=gx, ny=ny, xw=xw, fw=fw)
        if fam:
            ln = p['segs'][0]['pro'] in (PRO_LN, PRO_LN_ATTN)
            q['cut'] = cuts + [0] * (7 - len(cuts))
            for i in range(Sn):
                j = (cuts[i + 1] - cuts[i] + 7) // 8
                sg = seg_of_kblock(p, cuts[i])
                if sg['pro'] in (PRO_GN, PRO_GN_SILU) and sg['gs'] == 32 and j % 2:
                    j += 1
                q['jws'][i] = q['Jw'] if ln else j
        gx += fw if fw else xw
        kcmax = max(kcmax, min(kbps * 16, 1024))
        out['prob'].append(q)
    nt = tp[4] if fam else tp[6]
    if nt == 2:
        gx //= 2
        if fam:
            out['prob'][0]['xw'] = gx
    out['grid'] = (gx, gy, probs[0]['nbatch'])
    out['block'] = 576 if exp.get('prefetch') else 512
    out['lds'] = 0 if fam else (16 * (kcmax + 8) + nt * 8 * 256) * 4
    return out


def expected_prefetch(nxt, nt=1):
    """the descriptor of the ninth wave for the next op `nxt` (a problem k_rows_x takes alone)"""
    Sn, _, cuts = slices_of(nxt)
    return dict(gx=(nxt['N'] + 15) // 16 // nt * Sn, nt=nt, nkb_total=nxt['K'] // 16, S=Sn, cut=cuts + [0] * (7 - len(cuts)))


NO_PREFETCH = dict(gx=0, nt=0, nkb_total=0, S=0, cut=[0] * 7)


def X(jw, ns, proc, sln=1, nt=1, ge=0, np_=1, g=0):
    return 'k_rows_x<%d,%d,%d,%d,%d,%d,%d,%d>' % (jw, ns, proc, sln, nt, ge, np_, g)


def K0(ns, proc, csr=0, lnu=0, ge=0, u1=0, nt=1):
    return 'k_linear_rows<%d,%d,%d,%d,%d,%d,%d>' % (ns, proc, csr, lnu, ge, u1, nt)


def one(kernel, S=1, Jw=0, fallback='none', prefetch=False):
    """the route of a single-problem case"""
    return [dict(kernel=kernel, first=0, nprob=1, fallback=fallback, prefetch=prefetch, prob=[dict(S=S, Jw=Jw)])]


def fused(kernel, probs, fallback='none'):
    """ONE launch of all problems: probs = [(S, Jw), ...]"""
    return [dict(kernel=kernel, first=0, nprob=len(probs), fallback=fallback, prob=[dict(S=s, Jw=j) for s, j in probs])]


def split(*launches):
    """a group that comes out as single launches: (kernel, S, Jw, fallback) per problem"""
    return [dict(kernel=k, first=i, nprob=1, fallback=fb, prob=[dict(S=s, Jw=j)]) for i, (k, s, j, fb) in enumerate(launches)]


CASES = []


def case(name, probs, route, family=1, nxt=None, env=None, **kw):
    assert all(c['name'] != name for c in CASES), name
    CASES.append(dict(name=name, probs=probs if isinstance(probs, list) else [probs], route=route, family=family, next=nxt, env=env, **kw))


GN = lambda w, gs, ns=1, silu=1, affine=1, relu=0, inputs='spread': S(w, ns=ns, pro=PRO_GN_SILU if silu else PRO_GN, gs=gs, affine=affine,
                                                                       relu=relu, inputs=inputs)

# ---- family 1, single problem -------------------------------------------------------------------------------------------------------------
case('x2-k256-3slab-relu', P([S(256, ns=3, relu=1)]), one(X(2, 4, 0), 1, 2))
case('x2-k176-ragged-waves', P([S(176)]), one(X(2, 4, 0), 1, 2))                       # 11 k-blocks at Jw 2: wave 5 has one, 6 and 7 none
for gs_, aff in ((4, 1), (8, 0), (16, 1)):
    case('x2gn-k256-2x128-gs%d' % gs_, P([GN(256, gs_, ns=4, affine=aff)], kbps=8, ss=1, res=2), one(X(2, 4, 1), 2, 1))
case('x2gn-k176-gs16-ragged-waves', P([GN(176, 16, silu=0)]), one(X(2, 4, 1), 1, 2))
case('x2gn-const-group', P([GN(256, 16, inputs='const')], kbps=8, ss=1), one(X(2, 4, 1), 2, 1))
case('x2gn-ratio64', P([GN(256, 16, inputs='ratio')], kbps=8, ss=1), one(X(2, 4, 1), 2, 1))
case('x2gn-nosilu-const-group', P([GN(256, 8, silu=0, inputs='const')], kbps=8, ss=1), one(X(2, 4, 1), 2, 1))       # plain ES_PRO_GN
case('x2gn-nosilu-ratio64', P([GN(256, 8, silu=0, inputs='ratio')], kbps=8, ss=1), one(X(2, 4, 1), 2, 1))
case('x4gn-nosilu-gs32-ratio64', P([GN(384, 32, silu=0, affine=0, inputs='ratio')]), one(X(4, 4, 1), 1, 4))
case('x4-k512-4slab', P([S(512, ns=4)]), one(X(4, 4, 0), 1, 4))
case('x4-k272', P([S(272)]), one(X(4, 4, 0), 1, 3))                                     # 17 k-blocks at Jw 3: wave 5 has two, 6 and 7 none
case('x4gn-k384-gs32', P([GN(384, 32)]), one(X(4, 4, 1), 1, 4))                        # Jw 3 rounded to 4
case('x4gn-plain-gn-plain-half', P([S(384), GN(384, 32, ns=2), S(128, relu=1)], kbps=24, ss=1 | 4), one(X(4, 4, 1), 4, 4))
case('x4gn-k272-gs16', P([GN(272, 16)]), one(X(4, 4, 1), 1, 3))
case('x8-k1024-2slab', P([S(1024, ns=2)]), one(X(8, 2, 0), 1, 8))
case('x8-k656', P([S(656)]), one(X(8, 2, 0), 1, 6))                                     # 41 k-blocks at Jw 6: wave 6 has five, wave 7 none
case('x12-k1536', P([S(1536)]), one(X(12, 1, 0), 1, 12))
case('x12-k1296', P([S(1296)]), one(X(12, 1, 0), 1, 11))                                # 81 k-blocks at Jw 11: wave 7 has four
case('x12-k1040-and-16', P([S(1040), S(16)], kbps=65, ss=1), one(X(12, 1, 0), 2, 9))  # 65 at Jw 9: wave 7 has two; the 16-column slice: seven waves with none
for nm, act in (('relu', ACT_RELU), ('silu', ACT_SILU), ('sigmoid', ACT_SIGMOID)):
    case('x4-k272-act-' + nm, P([S(272)], act=act, res=1), one(X(4, 4, 0), 1, 3))
for r in (1, 2, 3, 4, 5, 6):
    case('x2-res%d' % r, P([S(96)], res=r, res2=2 if r == 2 else 0), one(X(2, 4, 0), 1, 1))
case('x2-res-step', P([S(96)], res=1, res_step=1), one(X(2, 4, 0), 1, 1))
for s_ in (3, 5, 6):
    case('x2-s%d-one-kblock-each' % s_, P([S(16 * s_, ns=2)], kbps=1), one(X(2, 4, 0), s_, 1))
case('x2-grid-5460', P([S(96)], M=5, N=14560, kbps=1), one(X(2, 4, 0), 6, 1))
case('f0-grid-5466', P([S(96)], M=5, N=14576, kbps=1), one(K0(1, 0), 6, fallback='grid'))

# ---- family 1, gather ---------------------------------------------------------------------------------------------------------------------
G3 = lambda: [S(64, mode=GATHER), S(32), S(64, mode=GATHER)]          # (a workgroup reads ONE segment: cut at the segments)
case('x8g-gather-direct-gather', P(G3(), kbps=4, ss=1), one(X(8, 2, 0, g=1), 3, 1))
case('x8g-k176-2slab', P([S(176, ns=2, mode=GATHER)]), one(X(8, 2, 0, g=1), 1, 2))
case('x8g-k656', P([S(656, mode=GATHER)]), one(X(8, 2, 0, g=1), 1, 6))
case('x12g-k1040', P([S(1040, mode=GATHER), S(16)], kbps=65, ss=1), one(X(12, 1, 0, g=1), 2, 9))
case('x12g-k1296', P([S(1296, mode=GATHER)]), one(X(12, 1, 0, g=1), 1, 11))
case('x8g3-of-three', [P(G3(), M=100, kbps=4, ss=1), P([S(96)], M=100), P([S(176, ns=2)], M=20)], fused(X(8, 2, 0, np_=3, g=1), [(3, 1), (1, 1), (1, 2)]))
case('x8g3-k656-pair', [P([S(656, mode=GATHER)]), P([S(96)])], fused(X(8, 2, 0, np_=3, g=1), [(1, 6), (1, 1)]))
case('x12g3-of-three', [P([S(1040, mode=GATHER), S(16)], kbps=65, ss=1, M=100), P([S(96)], M=100), P([S(1296)], M=20)],
     fused(X(12, 1, 0, np_=3, g=1), [(2, 9), (1, 1), (1, 11)]))
case('x12g3-pair', [P([S(1296, mode=GATHER)]), P([S(96)])], fused(X(12, 1, 0, np_=3, g=1), [(1, 11), (1, 1)]))
case('f0-gather-3slab', P([S(64, ns=3, mode=GATHER)]), one(K0(4, 0), 1, fallback='gather'))

# ---- family 1, three problems -------------------------------------------------------------------------------------------------------------
case('x2-3-pair', [P([S(176)]), P([S(96, ns=3, relu=1)])], fused(X(2, 4, 0, np_=3), [(1, 2), (1, 1)]))
case('x2-3-of-three-rider', [P([S(176)], M=100), P([S(96)], M=100, kbps=2), P([S(256, ns=2)], M=20)],
     fused(X(2, 4, 0, np_=3), [(1, 2), (3, 1), (1, 2)]))
case('x2gn-3-pair', [P([GN(176, 16)]), P([S(96)])], fused(X(2, 4, 1, np_=3), [(1, 2), (1, 1)]))
case('x2gn-3-of-three-rider', [P([S(96)], M=100), P([GN(256, 8, ns=2)], M=100, kbps=8, ss=1), P([GN(176, 4, silu=0)], M=20)],
     fused(X(2, 4, 1, np_=3), [(1, 1), (2, 1), (1, 2)]))
case('x4-3-pair', [P([S(272)]), P([S(96)])], fused(X(4, 4, 0, np_=3), [(1, 3), (1, 1)]))
case('x4-3-of-three-rider', [P([S(512, ns=4)], M=100), P([S(96)], M=100), P([S(272)], M=20)], fused(X(4, 4, 0, np_=3), [(1, 4), (1, 1), (1, 3)]))
case('x4gn-3-pair', [P([GN(272, 16)]), P([S(96)])], fused(X(4, 4, 1, np_=3), [(1, 3), (1, 1)]))
case('x4gn-3-of-three-rider', [P([GN(384, 32)], M=100), P([S(96)], M=100), P([GN(272, 16)], M=20)],
     fused(X(4, 4, 1, np_=3), [(1, 4), (1, 1), (1, 3)]))
case('x8-3-pair', [P([S(656)]), P([S(96)])], fused(X(8, 2, 0, np_=3), [(1, 6), (1, 1)]))
case('x8-3-of-three-rider', [P([S(1024, ns=2)], M=100), P([S(96)], M=100), P([S(656)], M=20)], fused(X(8, 2, 0, np_=3), [(1, 8), (1, 1), (1, 6)]))
# a group k_rows_x does not take as a whole (one member needs the class of 12 k-blocks per wave, no gather): single launches
case('split-x12-member', [P([S(96)]), P([S(1296)])], split((X(2, 4, 0), 1, 1, 'none'), (X(12, 1, 0), 1, 11, 'none')))
case('split-csr-member', [P([S(96)], M=7), P([S(64, mode=CSRMEAN)], M=7)], split((X(2, 4, 0), 1, 1, 'none'), (K0(1, 0, csr=1), 1, 0, 'csr')))
case('f0-group-no-member', [P([S(72)]), P([S(96, ns=8)])], fused(K0(8, 0), [(1, 0), (1, 0)], fallback='k16'))

# ---- family 1, LayerNorm ------------------------------------------------------------------------------------------------------------------
LN = lambda w, ns=1, affine=1, inputs='spread': S(w, ns=ns, pro=PRO_LN, affine=affine, inputs=inputs)
case('xln-k192', P([LN(192)]), one(X(4, 2, 2, ge=1), 1, 2))
case('xln-k512-2slab-noaffine', P([LN(512, ns=2, affine=0)]), one(X(4, 2, 2, ge=1), 1, 4))
case('xln-k272', P([LN(272, ns=2)]), one(X(4, 2, 2, ge=1), 1, 3))
case('xln-const-row', P([LN(192, inputs='const')]), one(X(4, 2, 2, ge=1), 1, 2))
case('xln-ratio64', P([LN(192, inputs='ratio')]), one(X(4, 2, 2, ge=1), 1, 2))
case('xln-geglu-n48', P([LN(192)], N=48, act=ACT_GEGLU, res=1), one(X(4, 2, 2, ge=1), 1, 2))
case('xln-nt2-geglu-n32', P([LN(272, ns=2)], N=32, act=ACT_GEGLU), one(X(4, 2, 2, nt=2, ge=1), 1, 3))
case('xln2-k512-two-slices', P([LN(512)], kbps=16), one(X(2, 2, 2, sln=2, ge=1), 2, 2))
case('xln2-k352', P([LN(352, ns=2, affine=0)], kbps=11), one(X(2, 2, 2, sln=2, ge=1), 2, 2))
LA = lambda w, ns=1, inputs='spread': S(w, ns=ns, pro=PRO_LN_ATTN, affine=0, inputs=inputs)
case('xlnattn-w128', P([LA(128)], res=1, res2=1), one(X(4, 2, 3, ge=1), 1, 1))
# the statistics of t0 (the first of the two rounds): a constant t0 row drives rstd(t0) to eps^-1/2; |mean| / spread = 64
case('xlnattn-const-t0-row', P([LA(272, inputs='const')], res=1, res2=1), one(X(4, 2, 3, ge=1), 1, 3))
case('xlnattn-ratio64', P([LA(272, inputs='ratio')], res=1, res2=1), one(X(4, 2, 3, ge=1), 1, 3))
case('xlnattn-nt2-ratio64', P([LA(128, ns=2, inputs='ratio')], N=32, act=ACT_GEGLU, res=1, res2=1), one(X(4, 2, 3, nt=2, ge=1), 1, 1))
case('xlnattn-w512-2slab', P([LA(512, ns=2)], res=1, res2=1), one(X(4, 2, 3, ge=1), 1, 4))
case('xlnattn-w272', P([LA(272)], res=1, res2=1), one(X(4, 2, 3, ge=1), 1, 3))
case('xlnattn-nt2-w128', P([LA(128)], N=32, act=ACT_GEGLU, res=1, res2=1), one(X(4, 2, 3, nt=2, ge=1), 1, 1))
case('xlnattn-nt2-w272', P([LA(272, ns=2)], N=32, act=ACT_GEGLU, res=1, res2=1), one(X(4, 2, 3, nt=2, ge=1), 1, 3))
case('f0-ln-k1024', P([LN(1024)]), one(K0(1, 0, lnu=8, ge=1), 1, fallback='ln_shape'))
case('f0-ln-k520', P([LN(520, ns=2)]), one(K0(2, 0, lnu=8, ge=1), 1, fallback='k16'))

# ---- family 0 under the default family ----------------------------------------------------------------------------------------------------
for nm, mode in (('mean', CSRMEAN), ('sum', CSRSUM), ('wavg', CSRWAVG)):
    case('f0-csr-%s-relu' % nm, P([S(64, mode=mode, relu=1)], M=7), one(K0(1, 0, csr=1), 1, fallback='csr'))
    case('f0-csr-%s-slabs' % nm, P([S(64, ns=2, mode=mode)], M=7), one(K0(2, 2, csr=1, ge=1), 1, fallback='csr'))
for ns_ in (1, 2, 4, 8):
    case('f0-silu-prologue-%dslab' % ns_, P([S(96, ns=ns_, pro=PRO_SILU)]), one(K0(ns_, 2, csr=1, ge=1), 1, fallback='prologue'))
    case('f0-geglu-prologue-%dslab' % ns_, P([S(96, ns=ns_, pro=PRO_GEGLU)]), one(K0(ns_, 2, csr=1, ge=1), 1, fallback='prologue'))
case('f0-batch3', P([S(96)], nbatch=3), one(K0(1, 0), 1, fallback='batch'))
case('f0-k72', P([S(72)]), one(K0(1, 0), 1, fallback='k16'))
case('f0-5slab', P([S(96, ns=5, relu=1)]), one(K0(8, 0), 1, fallback='class'))
case('f0-8slab', P([S(96, ns=8)]), one(K0(8, 0), 1, fallback='seg_slabs'))
case('f0-gn-8slab', P([GN(96, 8, ns=8)]), one(K0(8, 1), 1, fallback='seg_slabs'))
case('f0-res7', P([S(96)], res=7), one(K0(1, 0), 1, fallback='res_slabs'))
case('x2-res6-res2-6', P([S(96)], res=6, res2=6), one(X(2, 4, 0), 1, 1))
case('f0-step-segment', P([S(96, step=1)]), one(K0(1, 0), 1, fallback='step'))
case('f0-straddle', P([S(48), S(48, ns=2)], kbps=2), one(K0(2, 0), 3, fallback='straddle'))
case('f0-geglu-epilogue', P([S(96)], N=32, act=ACT_GEGLU, res=1), one(K0(1, 2, csr=1, ge=1), 1, fallback='geglu_epi'))
case('f0-k1040-2slab', P([S(1040, ns=2)]), one(K0(2, 0), 1, fallback='class'))
case('f0-7-slices', P([S(112)], kbps=1), one(K0(1, 0), 7, fallback='slices'))
case('f0-jw13', P([S(1552)]), one(K0(1, 0), 1, fallback='jw'))
case('f0-gn-class8', P([GN(656, 16)]), one(K0(1, 1), 1, fallback='class'))
case('f0-gather-gn', P([S(64, mode=GATHER), GN(64, 16)], kbps=4, ss=1), one(K0(1, 1), 2, fallback='gather'))

# ---- class boundaries: a slice of 256 / 272 / 512 / 528 / 1024 / 1040 / 1536 / 1552 columns ------------------------------------------------
case('x2-k256', P([S(256)]), one(X(2, 4, 0), 1, 2))
case('x4-k512', P([S(512)]), one(X(4, 4, 0), 1, 4))
case('x8-k528', P([S(528)]), one(X(8, 2, 0), 1, 5))
case('x8-k1024', P([S(1024)]), one(X(8, 2, 0), 1, 8))
case('x12-k1040', P([S(1040)]), one(X(12, 1, 0), 1, 9))
case('f0-k528-3slab', P([S(528, ns=3)]), one(K0(4, 0), 1, fallback='class'))
case('x4-k512-3slab', P([S(512, ns=3)]), one(X(4, 4, 0), 1, 4))
case('x2-6slab', P([S(96, ns=6)]), one(K0(8, 0), 1, fallback='class'))

# ---- family 0 forced ----------------------------------------------------------------------------------------------------------------------
for ns_ in (1, 2, 4, 8):
    case('F0-plain-%dslab' % ns_, P([S(272, ns=ns_, relu=1)], res=2), one(K0(ns_, 0), 1), family=0)
    case('F0-gn-%dslab' % ns_, P([GN(176, 16, ns=ns_)], kbps=4), one(K0(ns_, 1), 3), family=0)
case('F0-k1040-two-chunks', P([S(1040 + 1040)], kbps=130), one(K0(1, 0), 1), family=0)
case('F0-gn-gs32-const', P([GN(128, 32, inputs='const')]), one(K0(1, 1), 1), family=0)
case('F0-gn-gs4-ratio64', P([GN(128, 4, inputs='ratio')]), one(K0(1, 1), 1), family=0)
case('F0-ln-k192', P([LN(192)]), one(K0(1, 0, lnu=4, ge=1), 1), family=0)
case('F0-ln-k512-2slab', P([LN(512, ns=2, affine=0)], N=48, act=ACT_GEGLU), one(K0(2, 0, lnu=4, ge=1), 1), family=0)
case('F0-ln-k1024-2slab', P([LN(1024, ns=2)]), one(K0(2, 0, lnu=8, ge=1), 1), family=0)
case('F0-ln-const-row', P([LN(192, inputs='const')]), one(K0(1, 0, lnu=4, ge=1), 1), family=0)
case('F0-ln-ratio64', P([LN(192, inputs='ratio')]), one(K0(1, 0, lnu=4, ge=1), 1), family=0)
case('F0-lnnt2-k192', P([LN(192)], N=32, act=ACT_GEGLU, res=1), one(K0(1, 0, lnu=4, ge=1, nt=2), 1), family=0)
case('F0-lnnt2-k272-2slab', P([LN(272, ns=2)], N=32, act=ACT_GEGLU), one(K0(2, 0, lnu=4, ge=1, nt=2), 1), family=0)
case('F0-lnnt2-k520', P([LN(520)], N=32, act=ACT_GEGLU), one(K0(1, 0, lnu=8, ge=1, nt=2), 1), family=0)
case('F0-lnnt2-k1024-2slab', P([LN(1024, ns=2, affine=0)], N=32, act=ACT_GEGLU), one(K0(2, 0, lnu=8, ge=1, nt=2), 1), family=0)
case('F0-fused-pair-rider', [P([S(176)], M=100), P([S(96, ns=2)], M=20)], fused(K0(2, 0), [(1, 0), (1, 0)]), family=0)
# every k_linear_rows instantiation a fused launch can select (all but the LayerNorm kernels), as a pair of equal row counts and
# with an M = 20 rider folded over an M = 100 host: the problem lookup (pi > 0) and the folding (fw > 0) of each of them.  Few
# workgroups: the GroupNorm and 4-slab groups stay on the ordinary (not U1) variants
for ns_ in (1, 2, 4, 8):
    for nm_, Mh, Mr in (('pair', 37, 37), ('rider', 100, 20)):
        case('F0-fused-plain-%dslab-%s' % (ns_, nm_), [P([S(176, ns=ns_, relu=1)], M=Mh), P([S(96)], M=Mr, res=1)],
             fused(K0(ns_, 0), [(1, 0), (1, 0)]), family=0)
        case('F0-fused-gn-%dslab-%s' % (ns_, nm_), [P([S(96)], M=Mh), P([GN(176, 16, ns=ns_)], M=Mr)], fused(K0(ns_, 1), [(1, 0), (1, 0)]), family=0)
        case('F0-fused-general-%dslab-%s' % (ns_, nm_), [P([S(96, ns=ns_, pro=PRO_SILU)], M=Mh), P([S(176)], M=Mr, kbps=4)],
             fused(K0(ns_, 2, csr=1, ge=1), [(1, 0), (3, 0)]), family=0)
for nm_, Mh, Mr in (('pair', 37, 37), ('rider', 100, 20)):
    case('F0-fused-csr-' + nm_, [P([S(64, mode=CSRMEAN)], M=Mh), P([S(64, mode=CSRSUM, relu=1)], M=Mr)], fused(K0(1, 0, csr=1), [(1, 0), (1, 0)]), family=0)
# the U1 variants by the default rule: a fused launch of more than 256 workgroups with a GroupNorm prologue or 4-slab operands
case('F0-u1-4slab', [P([S(128, ns=4)], N=512, kbps=2, M=37), P([S(128, ns=4)], N=512, kbps=2, M=37)],
     fused(K0(4, 0, u1=1), [(4, 0), (4, 0)]), family=0)
case('F0-u1-gn-4slab-rider', [P([GN(128, 16, ns=4)], N=512, kbps=2, M=37), P([S(128, ns=3)], N=512, kbps=2, M=20)],
     fused(K0(4, 1, u1=1), [(4, 0), (4, 0)]), family=0)
case('F0-u1-gn-1slab', [P([GN(128, 8)], N=512, kbps=2, M=37), P([S(96)], N=512, kbps=2, M=37)], fused(K0(1, 1, u1=1), [(4, 0), (3, 0)]), family=0)
case('F0-u1-gn-2slab', [P([GN(128, 4, ns=2)], N=512, kbps=2, M=37), P([S(96)], N=512, kbps=2, M=37)], fused(K0(2, 1, u1=1), [(4, 0), (3, 0)]), family=0)
case('F0-u1-4slab-rider', [P([S(128, ns=4)], N=512, kbps=2, M=37), P([S(128, ns=3)], N=24, kbps=2, M=5)],
     fused(K0(4, 0, u1=1), [(4, 0), (4, 0)]), family=0)
case('F0-u1-gn-4slab', [P([GN(128, 16, ns=4)], N=512, kbps=2, M=37), P([S(128, ns=3)], N=24, kbps=2, M=37)],
     fused(K0(4, 1, u1=1), [(4, 0), (4, 0)]), family=0)
case('F0-u1-gn-1slab-rider', [P([GN(128, 8)], N=512, kbps=2, M=37), P([S(96)], N=24, M=5)], fused(K0(1, 1, u1=1), [(4, 0), (1, 0)]), family=0)
case('F0-u1-gn-2slab-rider', [P([GN(128, 4, ns=2)], N=512, kbps=2, M=37), P([S(96)], N=24, M=5)], fused(K0(2, 1, u1=1), [(4, 0), (1, 0)]), family=0)
case('F0-no-u1-256-workgroups', [P([S(128, ns=4)], N=512, kbps=4, M=32), P([S(128, ns=4)], N=512, kbps=4, M=32)],
     fused(K0(4, 0), [(2, 0), (2, 0)]), family=0)
# ES_ROWS_U1=2 (timing-only switch, read once per process: these two run in one child process)
case('F0-u1env-1slab', [P([S(176)], M=100), P([S(96)], M=20)], fused(K0(1, 0, u1=1), [(1, 0), (1, 0)]), family=0, env={'ES_ROWS_U1': '2'})
case('F0-u1env-1slab-pair', [P([S(176)]), P([S(96)])], fused(K0(1, 0, u1=1), [(1, 0), (1, 0)]), family=0, env={'ES_ROWS_U1': '2'})
case('F0-u1env-2slab-rider', [P([S(176, ns=2)], M=100), P([S(96)], M=20)], fused(K0(2, 0, u1=1), [(1, 0), (1, 0)]), family=0, env={'ES_ROWS_U1': '2'})
case('F0-u1env-2slab', [P([S(176, ns=2, relu=1)]), P([S(96)])], fused(K0(2, 0, u1=1), [(1, 0), (1, 0)]), family=0, env={'ES_ROWS_U1': '2'})

# ---- prefetch: a two-op plan, the first launch carries the ninth wave for the second --------------------------------------------------------
case('pf-plain-next', P([S(96)], N=136), one(X(2, 4, 0), 1, 1, prefetch=True), nxt=P([S(272)], N=40), pf_nt=1)
case('pf-sliced-next', P([S(176)], N=136), one(X(2, 4, 0), 1, 2, prefetch=True), nxt=P([S(384), GN(384, 32, ns=2), S(128)], N=40, kbps=24, ss=1 | 4), pf_nt=1)
case('pf-nt2-next', P([S(96)], N=136), one(X(2, 4, 0), 1, 1, prefetch=True), nxt=P([LN(272)], N=64, act=ACT_GEGLU), pf_nt=2)
case('pf-fewer-than-8-workgroups', P([S(96)], M=16), one(X(2, 4, 0), 1, 1, prefetch=True), nxt=P([S(272)], N=40), pf_nt=1)
case('pf-next-on-family0', P([S(96)]), one(X(2, 4, 0), 1, 1), nxt=P([S(72)]), pf_nt=0)

BY_NAME = {c['name']: c for c in CASES}
