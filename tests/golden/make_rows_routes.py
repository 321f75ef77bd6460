"""Writes rows_routes.npz: every field of the route of es_linear_rows_f32 / es_linear_rows_multi_f32 (es_linear_rows_route_of: per
launch the kernel, grid, block, LDS bytes, the prefetch descriptor, per problem S, kbps, Jw, the cuts, the k-blocks per wave of
every slice and the tile bookkeeping) under both kernel families over
  * the cases of tests/rows_matrix_cases.py,
  * every launch group of the layout step as the planner emits it on a CPU Builder (tools/plan_dryrun.py) at model_channels 128, 384
    and 512, cross-attention / concat / no time embedding, each with the next rows op of the plan as its prefetch hint,
  * the set-up GCNs (gconv_net_ec, gconv_net_manipulation: 640- and 1344-wide node vectors).
No device is needed: the query launches nothing and dereferences no operand.  tests/test_rows_matrix_cpu.py replays the table against
the built library, so a change of the routing rule shows as a changed entry; regenerate the file only when such a change is intended,
and say so in the commit.  The file in this commit was recorded from the launchers as they were BEFORE their decisions moved into
rows_route() (profiles/rows_matrix_notes.md); the fall-back reason is the one field those launchers did not know and is not recorded.

usage: python tests/golden/make_rows_routes.py

The file holds no pointers and no tensors: one row of small integers per problem (REC: what of an es_linear_args the routing can
read; optional pointers as present / absent flags), the tag and the problem count of every entry, its next op, and one route vector per
(family, entry) (VEC), -1 throughout where the launcher refuses."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

SEG_INTS = ('width', 'ld', 'mode', 'nslab', 'slab_stride', 'pre_act', 'pro', 'gs', 'step_stride')
SEG_PTRS = ('idx', 'ent_row', 'ent_off', 'step', 'gamma', 'beta', 'ent_wt')
ARG_INTS = ('nseg', 'M', 'K', 'N', 'prologue', 'act', 'res_ld', 'res_nslab', 'res_slab_stride', 'res2_ld', 'res2_nslab', 'res2_slab_stride',
            'out_ld', 'nbatch', 'a_bstride', 'out_bstride', 'kb_per_slice', 'out_slab_stride', 'res_step_stride', 'seg_slices')
ARG_PTRS = ('bias', 'gamma', 'beta', 'res', 'res2', 'res_step')
REC = 3 * (len(SEG_INTS) + len(SEG_PTRS)) + len(ARG_INTS) + len(ARG_PTRS)

PROB = ('S', 'kbps', 'Jw') + tuple('cut%d' % i for i in range(7)) + tuple('jws%d' % i for i in range(6)) + ('wg0', 'ny', 'xw', 'fw')
LAUNCH = ('family', 'kernel', 'first', 'nprob', 'grid_x', 'grid_y', 'grid_z', 'block', 'lds', 'pf_gx', 'pf_nt', 'pf_nkb_total', 'pf_S') + \
    tuple('pf_cut%d' % i for i in range(7))
VEC = 1 + 3 * (len(LAUNCH) + 3 * len(PROB))


def record(a):
    """the routing-relevant content of an es_linear_args as a row of REC integers"""
    r = []
    for s in range(3):
        r += [int(getattr(a.seg[s], f)) for f in SEG_INTS] + [int(bool(getattr(a.seg[s], f))) for f in SEG_PTRS]
    return r + [int(getattr(a, f)) for f in ARG_INTS] + [int(bool(getattr(a, f))) for f in ARG_PTRS]


def args_of(rec):
    """an es_linear_args with that content; every pointer that is present is a dummy nobody dereferences"""
    from echoscene_amd import hip
    a = hip.LinearArgs()
    it = iter(int(v) for v in rec)
    at = 0x10000
    for s in range(3):
        for f in SEG_INTS:
            setattr(a.seg[s], f, next(it))
        a.seg[s].ptr = at
        for f in SEG_PTRS:
            at += 0x1000
            setattr(a.seg[s], f, at if next(it) else None)
        at += 0x1000
    for f in ARG_INTS:
        setattr(a, f, next(it))
    a.wpack, a.out = 0x80000, 0x90000
    for f in ARG_PTRS:
        at += 0x1000
        setattr(a, f, at if next(it) else None)
    return a


def route_vector(L, args, nxt):
    from echoscene_amd import hip
    arr = (C.POINTER(hip.LinearArgs) * len(args))(*[C.pointer(a) for a in args])
    info = hip.RowsRouteInfo()
    if L.es_linear_rows_route_of(arr, len(args), None if nxt is None else C.byref(nxt), C.byref(info)) != 0:
        return [-1] * VEC
    v = [info.nlaunch]
    for li in range(3):
        l = info.launch[li]
        v += [int(getattr(l, f)) for f in LAUNCH[:13]] + list(l.pf_cut)
        for i in range(3):
            q = l.prob[i]
            v += [q.S, q.kbps, q.Jw] + list(q.cut) + list(q.jws) + [q.wg0, q.ny, q.xw, q.fw]
    assert len(v) == VEC
    return v


def plan_groups(b, tag):
    """(tag, [es_linear_args of one launch call], next op or None) for every rows launch of a plan, as es_plan_run groups and hints them"""
    import plan_dryrun
    from echoscene_amd import hip
    ops, out = b.ops, []
    for gi, (i0, grp) in enumerate(plan_dryrun.launches(b)):
        if grp[0].kind != hip.OP_LINEAR:
            continue
        k, nxt = i0 + len(grp) - 1, None
        for step in range(1, len(ops) + 1):
            o2 = ops[(k + step) % len(ops)]
            if o2.kind != hip.OP_LINEAR:
                continue
            if not o2.u.linear.fuse_next and (k + step) % len(ops) != i0:
                nxt = o2.u.linear
            break
        out.append(('%s launch %d' % (tag, gi), [op.u.linear for op in grp], nxt))
    return out


def gcn_plan(din, dpred, layers, O):
    import torch
    from echoscene_amd import synth
    from echoscene_amd.model.graph import GraphTripleConvNet
    from echoscene_amd.plan import Builder, GraphIndex, GCNWeights, View, emit_gcn
    from echoscene_amd.samplers import _cap, _cpu_sd
    dev = torch.device('cpu')
    net = GraphTripleConvNet(din, dpred, num_layers=layers, hidden_dim=256, output_dim=640, pooling='avg', residual=True,
                             mlp_normalization='batch')
    synth.seeded_fill_(net, prefix='dry.gcn.')
    gw = GCNWeights({'n.' + k: v for k, v in _cpu_sd(net).items()}, 'n', dev, 'avg')
    _, triples = synth.synthetic_graph(O, seed=3)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    b = Builder(dev)
    emit_gcn(b, gw, g, View(b.dev(torch.zeros(O, din))), din, View(b.dev(torch.zeros(triples.shape[0], dpred))), dpred)
    return b


def sweep():
    """[(tag, [record per problem], next record or None)]"""
    import plan_dryrun
    import rows_matrix_cases as rm
    out = []
    for c in rm.CASES:
        for M in (None, 5, 124):
            args, nxt = rm.case_args(c, M)
            out.append(('matrix %s%s' % (c['name'], '' if M is None else ' M=%d' % M), [record(a) for a in args], None if nxt is None else record(nxt)))
    for mc in (128, 384, 512):
        for nm, kw in (('crossattn', {}), ('no_t_emb', dict(enable_t_emb=False)), ('concat', dict(concat=True))):
            b, _ = plan_dryrun.emit_layout_step_cpu(mc=mc, O=8, **kw)
            out += [(t, [record(a) for a in args], None if nxt is None else record(nxt)) for t, args, nxt in plan_groups(b, 'layout mc%d %s' % (mc, nm))]
    for nm, (din, dpred, layers) in (('gconv_net_ec', (640, 640, 5)), ('gconv_net_manipulation', (1344, 640, 5))):
        b = gcn_plan(din, dpred, layers, 8)
        out += [(t, [record(a) for a in args], None if nxt is None else record(nxt)) for t, args, nxt in plan_groups(b, 'setup ' + nm)]
    return out


def answers(L, entries):
    """[family 1, family 0][entry][VEC]; the process's family is restored"""
    was = L.es_rows_get_kernel_family()
    out = np.full((2, len(entries), VEC), -1, dtype=np.int64)
    try:
        for fi, fam in enumerate((1, 0)):
            assert L.es_rows_set_kernel_family(fam) == 0
            for ei, (_, recs, nxt) in enumerate(entries):
                out[fi, ei] = route_vector(L, [args_of(r) for r in recs], None if nxt is None else args_of(nxt))
    finally:
        L.es_rows_set_kernel_family(was)
    return out


def tables(entries):
    n = len(entries)
    recs, nprob, nxt = np.full((n, 3, REC), -1, dtype=np.int32), np.zeros(n, dtype=np.int8), np.full((n, REC), -1, dtype=np.int32)
    for ei, (_, rs, nx) in enumerate(entries):
        nprob[ei] = len(rs)
        recs[ei, :len(rs)] = rs
        if nx is not None:
            nxt[ei] = nx
    return recs, nprob, nxt


def entries_of(z):
    """the entries of a loaded file"""
    return [(str(t), [z['recs'][ei, i] for i in range(int(z['nprob'][ei]))], None if z['next'][ei, 0] < 0 else z['next'][ei])
            for ei, t in enumerate(z['tags'])]


if __name__ == '__main__':
    from echoscene_amd import hip
    L = hip.lib()
    entries = sweep()
    ans = answers(L, entries)
    recs, nprob, nxt = tables(entries)
    path = os.path.join(HERE, 'rows_routes.npz')
    np.savez_compressed(path, tags=np.asarray([t for t, _, _ in entries]), recs=recs, nprob=nprob, next=nxt, routes=ans.astype(np.int32),
                        kernels=np.asarray([L.es_rows_kernel_name(i).decode() for i in range(L.es_rows_kernel_count())]))
    used = sorted(set(int(k) for f in range(2) for v in ans[f] if v[0] > 0 for k in v[1:][1::len(LAUNCH) + 3 * len(PROB)][:int(v[0])]))
    print('%d entries x 2 families, %d refused, %d of %d kernels, %d bytes' % (len(entries), int((ans[:, :, 0] < 0).sum()), len(used),
                                                                                  L.es_rows_kernel_count(), os.path.getsize(path)))
