"""GPU: the footprints of tests/plan_footprint.py witnessed by the kernels, one launch at a time.

The static checks of tests/test_plan_footprint_cpu.py are only as good as the footprint functions, so every function is held against
what its kernel really touches.  A plan is emitted on the device as the samplers emit it (the tiny shape network at 3 objects, the
VQ-VAE plans at one object, one layout denoiser step and the layout loop step with each of its updates; seeded inputs; the configurations plan_footprint.WITNESSED, which the CPU file shows to
hold every op kind and route).  Its launch groups run one by one on the main stream (plan.sub_plan on copies with lane 0), next to a
shadow copy of ALL the plan's buffers that is advanced with each op's declared writes:

  * determinism       -- run twice from the same state: the declared write regions have the same bits;
  * writes <= declared -- after the op every byte of every buffer outside the declared write regions equals the shadow;
  * `full` means full -- with the declared-full regions pre-filled with 0x5A, then 0xA5: no byte keeps its fill in both runs
    (regions the op also reads in place are filled in a pass of their own);
  * reads <= declared  -- every byte of every fp32 / f16 buffer (int16 weight images count as f16) outside the declared read regions
    is 0xFF (NaN in both types): the declared write regions keep the bits of the unpoisoned run.  int32 / int64 tensors are never
    poisoned or filled (a poisoned index could fault); the CPU file bounds their share of the plan's bytes.
Scratch an op fills and consumes itself (`internal`: split-K slabs, statistics partials, the stem's pooled map) counts as written and
is left out of the bit comparisons.  At the end one replay of the captured graph, with its parallel branch, must leave the bits of the
serial op-by-op run in every result tensor."""
import ctypes as C
import os
import sys
import time

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import plan_footprint as pf      # noqa: E402
from plan_footprint import mv    # noqa: E402

pytestmark = pytest.mark.gpu

O_STEP, O_VQ = 3, 1              # the smallest object counts: synth.synthetic_graph accepts 3
POISONED = {'float32', 'float16', 'int16'}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import __graft_entry__ as ge
    ge.build()
    return torch.device('cuda')


def _fill(dev):
    """seeded contents of the per-step tables: N(0, 1), the update coefficients in [0.5, 1.5) (they divide)"""
    gen = torch.Generator().manual_seed(11)

    def fill(name, *shape):
        t = torch.rand(*shape, generator=gen) + 0.5 if name in ('coef', 'keep_tab') else torch.randn(*shape, generator=gen)
        return t.to(dev)
    return fill


def emit(name, dev):
    """(Builder, extended document, result tensors by name, roots, first-iteration ops) of a witnessed configuration, on the device"""
    if name in pf.LOOP_CONFIGS:                      # the whole layout loop step, with its update op
        b, doc, io, roots = pf.emit_layout_loop(name, dev=dev, fill=_fill(dev), want_builder=True)
        torch.cuda.synchronize()
        results = {k: v for k, v in io.items() if isinstance(v, torch.Tensor)}
        return b, doc, results, [roots, results], []
    log = []
    with pf.recording_allocations(log):
        if name in mv.VQ_CONFIGS:
            b, roots, out = mv.emit_vq(name, dev=dev, Oc=O_VQ)
        elif name in pf.LAYOUT_CONFIGS:
            import plan_dryrun
            b, io = plan_dryrun.emit_layout_step_cpu(mc=128, O=8, dev=dev, fill=_fill(dev))
            roots, out = [io], None
        else:
            b, roots, out = mv.emit_step(**{**mv.TINY, **mv.STEP_CONFIGS[name], 'O': O_STEP, 'dev': dev, 'fill': _fill(dev)})
    torch.cuda.synchronize()
    doc = pf.extend(b, roots, out, log)
    results = {k: v for k, v in (out or {}).items() if isinstance(v, torch.Tensor)}
    if name in pf.LAYOUT_CONFIGS:
        results = {k: v for k, v in io.items() if isinstance(v, torch.Tensor)}
    if name in mv.VQ_CONFIGS:                        # (emit_vq allocates its input, then its output, before anything else)
        results = dict(vq_in=b.keep[0], vq_out=b.keep[1])
    first = [op for op in (out or {}).get('first_ops', ()) if op is not None]
    return b, doc, results, [roots, results], first


class Arena:
    """every buffer of the plan as a uint8 view of its storage, and flat snapshots of all of them"""

    def __init__(self, b, roots, doc, dev):
        by_start = {}

        seen = set()

        def walk(o):
            if o is None or id(o) in seen:
                return
            seen.add(id(o))
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                if st.nbytes():
                    by_start.setdefault(st.data_ptr(), st)
            elif isinstance(o, (list, tuple, set)):
                for v in o:
                    walk(v)
            elif isinstance(o, dict):
                for v in o.values():
                    walk(v)
            elif hasattr(o, '__dict__') and type(o).__module__.startswith('echoscene_amd'):
                walk(vars(o))
        walk([b.keep, roots])
        self.views, self.base, n = [], [], 0
        for k, start in enumerate(doc['starts']):
            st = by_start[start]
            assert st.nbytes() == doc['buffers'][k][0]
            self.views.append(torch.empty(0, dtype=torch.uint8, device=dev).set_(st))
            self.base.append(n)
            n += st.nbytes()
        self.size, self.dev = n, dev
        self.floats = torch.zeros(n, dtype=torch.bool, device=dev)       # bytes of the buffers that may be poisoned / filled
        for k, (size, dtypes, _) in enumerate(doc['buffers']):
            if set(dtypes) <= POISONED:
                self.floats[self.base[k]:self.base[k] + size] = True

    def snapshot(self):
        return torch.cat(self.views)

    def load(self, flat):
        torch._foreach_copy_(self.views, [flat[b0:b0 + v.numel()] for b0, v in zip(self.base, self.views)])

    def window(self, flat, g):
        """the bytes of region ``g`` inside a flat snapshot, as a [rows, width] view"""
        return torch.as_strided(flat, (g.rows, g.width), (g.pitch, 1), self.base[g.buf] + g.off)

    def mask(self, regions):
        m = torch.zeros(self.size, dtype=torch.bool, device=self.dev)
        for g in regions:
            self.window(m, g).fill_(True)
        return m


def _where(t, mask, other):
    return torch.where(mask, torch.full((), other, dtype=torch.uint8, device=t.device), t)


def witness(name, dev):
    from echoscene_amd import hip, plan
    t0 = time.time()
    b, doc, results, roots, first_ops = emit(name, dev)
    gen = torch.Generator().manual_seed(5)
    for k, t in results.items():                     # seeded inputs: latents / volumes and, for the masked loops, shapes, draws and a mask
        if k in ('x', 'x0', 'knoise', 'snoise', 'noise', 'codes_all', 'vq_in'):          # (codes_all: what the echo all-gather would deliver)
            t.copy_((torch.randn(t.shape, generator=gen) * (0.1 if k == 'vq_in' else 1.0)).to(dev))
        if k == 'mask':
            t.copy_((torch.rand(t.shape, generator=gen) < 0.5).float().to(dev))
    ar = Arena(b, roots, doc, dev)
    torch.cuda.synchronize()
    state0 = ar.snapshot()
    shadow = state0.clone()
    groups = [(i0, b.ops[i0:i0 + n], doc['ops'][i0:i0 + n]) for i0, n in pf.launch_groups(doc['ops'])]
    # PLMS: the two ops of iteration 0 are no part of the steady step: witnessed behind it, from the state it leaves
    groups += [('first_ops[%d]' % k, [op], [rec]) for k, (op, rec) in enumerate(zip(first_ops, [r for r in doc['first_ops'] if r]))]
    findings, kinds = [], set()

    def locate(mask):
        at = int(mask.nonzero()[0])
        k = max(j for j, b0 in enumerate(ar.base) if b0 <= at)
        return 'first in buffer %d at +%d' % (k, at - ar.base[k])

    for i0, members, recs in groups:
        if recs[0][0] in (hip.OP_FORK, hip.OP_JOIN):
            continue
        own = []
        for op in members:
            o = hip.Op()
            C.memmove(C.byref(o), C.byref(op), C.sizeof(hip.Op))
            o.lane = 0
            own.append(o)
        p = plan.sub_plan(b, own)
        R, W = [], []
        for rec in recs:
            r, w = pf.op_footprint(doc, rec)
            R += r
            W += w
            kinds.add(pf.kind_name(rec[0]))
        where = '%s: op %s (%s)' % (name, i0, '+'.join(pf.kind_name(r[0]) for r in recs))
        wmask = ar.mask(W)
        cmp_mask = ar.mask([g for g in W if not g.internal])            # what a later op may read: compared bit for bit
        # 1. writes <= declared
        p.run()
        f1 = ar.snapshot()
        stray = (f1 != shadow) & ~wmask
        if bool(stray.any()):
            findings.append('%s writes outside its declared regions: %d bytes, %s' % (where, int(stray.sum()), locate(stray)))
        # 2. determinism
        ar.load(shadow)
        p.run()
        diff = (ar.snapshot() != f1) & cmp_mask
        if bool(diff.any()):
            findings.append('%s is not deterministic: %d bytes of its declared writes differ between two runs' % (where, int(diff.sum())))
        # 3. full means full (float buffers only: an int tensor is never filled).  Regions the op also reads -- the in-place state of
        #    an update -- are filled in a pass of their own: es_plms_first_a copies x to xsave, fill included
        reads = ar.mask(R + [g for g in W if not g.full and not g.internal])
        full = ar.mask([g for g in W if g.full and not g.internal]) & ar.floats
        for part in (full & ~reads, full & reads):
            if not bool(part.any()):
                continue
            kept = part
            for pat in (0x5A, 0xA5):
                ar.load(_where(shadow, part, pat))
                p.run()
                kept = kept & (ar.snapshot() == pat)
            if bool(kept.any()):
                findings.append('%s leaves %d bytes of a region declared full unwritten, %s' % (where, int(kept.sum()), locate(kept)))
        # 4. reads <= declared
        ar.load(_where(shadow, ar.floats & ~reads, 0xFF))
        p.run()
        diff = (ar.snapshot() != f1) & cmp_mask
        if bool(diff.any()):
            findings.append('%s reads outside its declared regions: %d bytes of its writes change when everything else is NaN, %s' % (
                where, int(diff.sum()), locate(diff)))
        # advance the shadow with the declared writes
        shadow = torch.where(wmask, f1, shadow)
        ar.load(shadow)
        if isinstance(i0, int) and i0 + len(recs) == len(doc['ops']):
            serial = shadow                                               # the state behind the steady step
    torch.cuda.synchronize()
    # the whole plan, once: one replay of the captured graph (with its parallel branch) against the serial op-by-op run
    ar.load(state0)
    whole = b.finish()
    step = results.get('step')
    if step is None:
        step = torch.zeros(1, dtype=torch.int32, device=dev)             # (es_sampler_run sets a counter; these plans read none)
    first_step = int(step.item())
    whole.sample(step, first_step, 1, use_graph=True)
    torch.cuda.synchronize()
    graph = ar.snapshot()
    rm = ar.mask([pf.Region(k, [doc['starts'].index(t.untyped_storage().data_ptr()), 0], 1, t.untyped_storage().nbytes())
                  for k, t in results.items() if k in ('x', 'eps', 'step', 'objbuf', 'pred', 'vq_out')])
    assert bool(rm.any())
    diff = (graph != serial) & rm
    if bool(diff.any()):
        findings.append('%s: the captured graph and the serial run differ in %d bytes of the result tensors, %s' % (name, int(diff.sum()), locate(diff)))
    print('%s: %d launch groups, kinds %s, %.1f MB, %.1f s' % (name, len(groups), sorted(kinds), ar.size / 1e6, time.time() - t0))
    return findings


@pytest.mark.parametrize('name', pf.WITNESSED)
def test_kernels_touch_what_their_footprints_declare(dev, name):
    try:
        findings = witness(name, dev)
    except AssertionError:
        raise
    except Exception as e:                           # a runtime error of the device ends the session: nothing more is started on it
        pytest.exit('%s: %s: %s' % (name, type(e).__name__, e), returncode=3)
    assert not findings, '%d findings\n  ' % len(findings) + '\n  '.join(findings[:25])
