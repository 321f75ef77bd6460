"""Writes vol_plans.npz: the op stream of every plan the volume planner (echoscene_amd/plan_vol.py) emits for some caller, in a form
that depends neither on addresses nor on the order of allocations.  Everything is emitted on a CPU Builder (the planner's questions
to the library are host-only queries); nothing runs.  tests/test_vol_plan_stream_cpu.py re-emits every configuration and compares it
with the file field by field, so a change of what a plan contains shows as a named (configuration, op, field).

Canonical form of an op: [kind, lane, value of every field of the member of Op.u the kind uses], the fields in the order of a
generic walk over the ctypes struct (arrays and nested structs included: FIELDS).  A pointer is [buffer ordinal, byte offset]: the
buffer is the tensor storage, kept alive by the plan (Builder.keep) or handed in by the caller (weights, tables, graph index), that
contains the address; ordinals are given in order of first appearance.  Per buffer: byte size, the dtypes of the tensors on it,
whether the plan claims it as scratch.  Per plan also weight_bytes, flops, the tags and what the step hands back to its caller.

The file was recorded from the planner as it was BEFORE its refactoring; regenerate it only when a change of the plans is intended,
and say so in the commit.  (Regenerated once since: `tiny lanes` forks and joins the predicate projection of every GCN layer -- the
race tests/test_plan_footprint_cpu.py found; the other 24 documents did not change.)

usage: python tests/golden/make_vol_plans.py"""
import bisect
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, 'vol_plans.npz')
RESULT_TENSORS = ('codes_local', 'codes_all', 'xc', 'cdev', 'pred', 'objbuf', 'x', 'eps', 'step', 'x0', 'mask', 'knoise', 'snoise')
RESULT_VALUES = ('split', 'code_cols', 'n_eps_ops', 'n_blend', 'ucw')


def kind_members():
    """op kind -> the member of Op.u it uses (None: FORK / JOIN carry no arguments)"""
    from echoscene_amd import hip as h
    return {h.OP_LINEAR: 'linear', h.OP_DDPM: 'update', h.OP_DDIM: 'update', h.OP_COPY: 'copy', h.OP_CONV: 'conv', h.OP_GN: 'gn',
            h.OP_LN: 'ln', h.OP_ATTN: 'attn', h.OP_GEGLU: 'geglu', h.OP_TO_CL: 'tocl', h.OP_STEM: 'stem', h.OP_VQ: 'vq', h.OP_FORK: None,
            h.OP_JOIN: None, h.OP_ROWSEL: 'rowsel', h.OP_CONV_F32: 'conv', h.OP_ATTN_F32: 'attn', h.OP_DDIM_BLEND: 'blend',
            h.OP_CONV_C1: 'conv_c1', h.OP_DDPM_KEEP: 'keep', h.OP_PLMS: 'plms', h.OP_PLMS_FIRST_A: 'plms', h.OP_PLMS_FIRST_B: 'plms',
            h.OP_DDIM_ROWS: 'keep', h.OP_DDIM_BLEND_VOX: 'blend_vox'}


def flatten(inst, prefix=''):
    """[(field name, is pointer, value)] of a ctypes struct instance, arrays and nested structs walked generically"""
    out = []
    for fname, ftype in inst._fields_:
        v = getattr(inst, fname)
        if issubclass(ftype, C.Array):
            for i in range(ftype._length_):
                if issubclass(ftype._type_, C.Structure):
                    out += flatten(v[i], '%s%s[%d].' % (prefix, fname, i))
                else:
                    out.append(('%s%s[%d]' % (prefix, fname, i), ftype._type_ is C.c_void_p, v[i]))
        elif issubclass(ftype, C.Structure):
            out += flatten(v, prefix + fname + '.')
        else:
            out.append((prefix + fname, ftype is C.c_void_p, v))
    return out


def field_names():
    """member of Op.u -> its flattened field names"""
    from echoscene_amd import hip
    return {m: [n for n, _, _ in flatten(t())] for m, t in hip._OpU._fields_}


class Buffers:
    """the tensor storages reachable from the roots, and the ordinals handed out so far"""

    def __init__(self, roots, scratch):
        self.by_start, self.scratch, self.order, self.ordinal = {}, scratch, [], {}
        seen = set()

        def walk(o):
            if o is None or id(o) in seen:
                return
            seen.add(id(o))
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                if st.nbytes():
                    ent = self.by_start.setdefault(st.data_ptr(), [st.nbytes(), set()])
                    ent[1].add(str(o.dtype).replace('torch.', ''))
            elif isinstance(o, (list, tuple, set)):
                for v in o:
                    walk(v)
            elif isinstance(o, dict):
                for v in o.values():
                    walk(v)
            elif hasattr(o, '__dict__') and type(o).__module__.startswith('echoscene_amd'):
                walk(vars(o))

        walk(roots)
        self.starts = sorted(self.by_start)

    def ref(self, p, what):
        if not p:
            return None
        assert p != 1, '%s: the workspace placeholder survived into the finished stream' % what
        i = bisect.bisect_right(self.starts, p) - 1
        if i < 0 or p >= self.starts[i] + self.by_start[self.starts[i]][0]:
            raise AssertionError('%s: pointer 0x%x lies in no tensor the plan keeps' % (what, p))
        s = self.starts[i]
        if s not in self.ordinal:
            self.ordinal[s] = len(self.order)
            self.order.append(s)
        return [self.ordinal[s], p - s]

    def table(self):
        return [[self.by_start[s][0], sorted(self.by_start[s][1]), s in self.scratch] for s in self.order]


def canon_op(op, bufs, what):
    member = kind_members()[int(op.kind)]
    rec = [int(op.kind), int(op.lane)]
    if member is not None:
        for name, is_ptr, v in flatten(getattr(op.u, member)):
            rec.append(bufs.ref(v, '%s %s' % (what, name)) if is_ptr else v)
    return rec


def canonical(b, roots, out=None):
    """the canonical document of the plan on Builder ``b``; ``out``: what emit_shape_step returned"""
    bufs = Buffers([b.keep, roots, out], set(b.scratch))
    doc = dict(ops=[canon_op(op, bufs, 'op %d' % i) for i, op in enumerate(b.ops)])
    first = (out or {}).get('first_ops', (None, None))
    doc['first_ops'] = [None if op is None else canon_op(op, bufs, 'first op %d' % i) for i, op in enumerate(first)]
    doc['tags'] = {n: bufs.ref(b.tags[n].ptr, 'tag ' + n) for n in sorted(b.tags)}
    doc['weight_bytes'], doc['flops'] = int(b.weight_bytes), int(b.flops)
    if out is not None:
        doc['values'] = {k: (list(out[k]) if isinstance(out[k], tuple) else out[k]) for k in RESULT_VALUES}
        doc['tensors'] = {k: None if out.get(k) is None else [list(out[k].shape), bufs.ref(out[k].data_ptr(), k)] for k in RESULT_TENSORS}
    doc['buffers'] = bufs.table()
    return doc


# ------------------------------------------------------------------------------------------------ the configurations
TINY = dict(width=32, ctx=64, O=6)
STEP_CONFIGS = {
    'tiny': {},
    'tiny lanes': dict(use_lanes=True),
    'tiny force_exchange': dict(force_exchange=True),
    'tiny shard 0:3': dict(lo=0, hi=3, shard_block=3),
    'tiny shard 3:6': dict(lo=3, hi=6, shard_block=3),
    'tiny deterministic': dict(deterministic=True),
    'tiny concat': dict(concat=True),
    'tiny no_mp': dict(mp=False),
    'tiny concat no_mp': dict(concat=True, mp=False),
    'tiny fp32': dict(precision='fp32'),
    'tiny fp32x': dict(precision='fp32x'),
    'tiny keep': dict(keep=True),
    'tiny keep_vox': dict(keep_vox=True),
    'tiny plms': dict(plms=True),
    'tiny plms shard 0:3': dict(plms=True, lo=0, hi=3, shard_block=3),
    'tiny step_noise': dict(step_noise=True),
    'tiny VOL_GN_RG_ANY': dict(switch=('VOL_GN_RG_ANY', True)),
    'tiny VOL_GN_F16 off': dict(switch=('VOL_GN_F16', False)),
    'tiny VOL_GN_PART_FUSED off': dict(switch=('VOL_GN_PART_FUSED', False)),
    'tiny gn_rg off': dict(gn_rg=0),
    'full O=32': dict(width=224, ctx=1280, O=32),
    'full O=32 up_fold off': dict(width=224, ctx=1280, O=32, up_fold=False),
    'full O=16': dict(width=224, ctx=1280, O=16),
}
VQ_CONFIGS = ('vq decode', 'vq encode fp16')          # (the encoder accepts fp16 only: samplers.VQEncoder)
CONFIGS = tuple(STEP_CONFIGS) + VQ_CONFIGS

_weights = {}


def make_builder(dev, precision='fp16', o_hint=0, up_fold=False, shard_block=None, force_exchange=False, use_lanes=False):
    """a CPU Builder with the volume path's hints (the one place that spells how they are given)"""
    from echoscene_amd.plan import Builder
    import echoscene_amd.plan_vol  # noqa: F401
    b = Builder(dev, precision=precision, o_hint=o_hint, up_fold=up_fold, shard_block=shard_block, force_exchange=force_exchange)
    b.use_lanes = use_lanes
    return b


def unet_weights(width, ctx, concat, mp, precision, dev='cpu'):
    """packed UNet3DWeights, once per process, network and device (the full-width one takes seconds on the host)"""
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.unet import DiffusionUNet
    from echoscene_amd.plan_vol import UNet3DWeights
    from echoscene_amd.samplers import _cpu_sd
    key = (width, ctx, concat, mp, precision, str(dev))
    if key not in _weights:
        p = escfg.shape_unet_params(width, concat=concat, mp=mp)
        if not concat:
            p['context_dim'] = ctx
        df = DiffusionUNet(p, conditioning_key='concat' if concat else 'crossattn')
        synth.seeded_fill_(df, prefix='vol_plans.%d.' % width)
        sd = {k[len('diffusion_net.'):]: v for k, v in _cpu_sd(df).items()}
        _weights[key] = UNet3DWeights(sd, df.diffusion_net, torch.device(dev), precision)
    return _weights[key]


def emit_step(width=32, ctx=64, O=6, concat=False, mp=True, precision='fp16', lo=0, hi=None, shard_block=None, deterministic=False,
              up_fold=True, force_exchange=False, use_lanes=False, switch=None, gn_rg=1, dev='cpu', fill=None, **step_kw):
    """samplers.emit_shape_step, as ShapeDenoiser._build_state calls it, on a CPU Builder -> (Builder, roots, its result).
    ``dev`` / ``fill``: another device, and fill(name, *shape) for the contents of the host tables instead of zeros (the GPU witness,
    tests/test_hip_plan_footprint.py: the recorded streams do not depend on either)"""
    from echoscene_amd import synth, hip, plan_vol
    from echoscene_amd.plan import GraphIndex
    from echoscene_amd.samplers import _cap, emit_shape_step, CANON_OBJECTS
    dev = torch.device(dev)
    mk = (lambda name, *shape: torch.zeros(*shape)) if fill is None else fill
    w = unet_weights(width, ctx, concat, mp, precision, dev)
    hi = O if hi is None else hi
    S, V0 = 4, 16 * 16 * 16
    ucw = V0 if concat else ctx
    _, triples = synth.synthetic_graph(O, seed=6)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    b = make_builder(dev, precision=precision, o_hint=-CANON_OBJECTS if deterministic else 0, up_fold=up_fold and not deterministic,
                     shard_block=(hi - lo) if shard_block is None else shard_block, force_exchange=force_exchange, use_lanes=use_lanes)
    tables = dict(emb=None, emb_all=mk('emb_all', S, w.emb_all.N), t_lin=mk('t_lin', S, 64) if w.enable_t_emb else None)
    temb, coef, keep_tab = mk('temb', S, w.mc), mk('coef', S, 5 if step_kw.get('step_noise') else 4), mk('keep_tab', S, 2)
    c = None
    if concat or not mp:
        c = mk('c', O, V0 if concat else ctx)[lo:hi]
    world = O // (hi - lo)
    was = getattr(plan_vol, switch[0]) if switch else None
    try:
        if switch:
            setattr(plan_vol, switch[0], switch[1])
        hip.check(hip.lib().es_vol_set_option(b'gn_rg', gn_rg), 'es_vol_set_option')
        out = emit_shape_step(b, w, g, mk('uc', O, ucw), temb, tables, coef, keep_tab, S, (3, 16, 16, 16), lo, hi, c_local=c,
                              gather_rows=(hi - lo) * world, **step_kw)
    finally:
        if switch:
            setattr(plan_vol, switch[0], was)
        hip.check(hip.lib().es_vol_set_option(b'gn_rg', 1), 'es_vol_set_option')
    return b, [w, g, tables, temb, coef, keep_tab], out


def emit_vq(which, dev='cpu', Oc=2):
    """emit_vq_decode / emit_vq_encode at a chunk of 2 objects with their default dims, as VQDecoder._plan / VQEncoder._plan call them"""
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.vqvae import VQVAE
    from echoscene_amd.plan_vol import VQWeights, VQEncWeights, emit_vq_decode, emit_vq_encode
    from echoscene_amd.samplers import _cpu_sd
    dev = torch.device(dev)
    if 'vq' not in _weights:
        p = escfg.vqvae_conf().model.params
        vq = VQVAE(dict(p.ddconfig), 64, p.embed_dim)
        synth.seeded_fill_(vq, prefix='vol_plans.vq.')
        _weights['vq'] = _cpu_sd(vq)
    b = make_builder(dev)
    if which == 'vq decode':
        w = VQWeights(_weights['vq'], dev)
        z, sdf = b.buf(Oc, 3, 16, 16, 16), b.buf(Oc, 1, 64, 64, 64)
        assert tuple(emit_vq_decode(b, w, z, sdf, Oc)) == (64, 64, 64)
    else:
        w = VQEncWeights(_weights['vq'], dev)
        sdf, z = b.buf(Oc, 1, 64, 64, 64), b.buf(Oc, w.embed_dim, 16, 16, 16)
        assert tuple(emit_vq_encode(b, w, sdf, z, Oc)) == (16, 16, 16)
    return b, [w], None


def emit(name):
    """(Builder, roots, result of emit_shape_step or None) of the configuration ``name``"""
    return emit_vq(name) if name in VQ_CONFIGS else emit_step(**{**TINY, **STEP_CONFIGS[name]})


def document(name):
    return canonical(*emit(name))


def load(path=PATH):
    z = np.load(path)
    return {str(n): json.loads(bytes(z['doc%d' % i]).decode()) for i, n in enumerate(z['names'])}, json.loads(bytes(z['fields']).decode())


if __name__ == '__main__':
    import __graft_entry__ as ge
    ge.build()
    docs = {n: json.loads(json.dumps(document(n))) for n in CONFIGS}
    arrays = {'doc%d' % i: np.frombuffer(json.dumps(docs[n], separators=(',', ':')).encode(), dtype=np.uint8) for i, n in enumerate(CONFIGS)}
    np.savez_compressed(PATH, names=np.asarray(CONFIGS), fields=np.frombuffer(json.dumps(field_names()).encode(), dtype=np.uint8), **arrays)
    for n in CONFIGS:
        print('%-28s %4d ops  %4d buffers' % (n, len(docs[n]['ops']), len(docs[n]['buffers'])))
    print('%d plans, %d bytes' % (len(docs), os.path.getsize(PATH)))
